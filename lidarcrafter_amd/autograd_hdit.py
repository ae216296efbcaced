"""Training graph of HDiT (lidargen/models/dits/hdit.py): the forward as a differentiable composition over the HIP kernels.

The inference forward of HDiT writes the q / k preparation in place, hoists the time path out of the steps and reads
detached caches of the modulation weights and the positional embedding, so, as for the UNets (autograd.py), training
takes a second composition of the same parameters, in the reference's arithmetic order:

  Linear (qkv, out_proj, GEGLU, FFN linear, merge / expand, detokenizer)
                      autograd.ConvRing as a 1x1 conv (residual in the epilogue); qkv_proj in exact fp32, as in inference
  (Ada)RMSNorm        lc_hdit_rmsnorm_fwd / lc_hdit_rmsnorm_bwd (dx, d(mod) [B, C] or d(gain) [C])
  GEGLU               lc_hdit_geglu_fwd / lc_hdit_geglu_bwd
  q / k preparation   lc_hdit_qk_prep_fwd on copies (the raw q / k stay for the backward) / lc_hdit_qk_prep_bwd
  neighbourhood attn  lc_hdit_na_train_fwd (o + log-sum-exp) / lc_hdit_na_bwd
  global attention    autograd.FlashAttention (mid level), exact fp32 as in inference
  permutes            space_to_depth / depth_to_space, each the other's adjoint
  PatchExpanding      depth_to_space(y, skip, alpha) / lc_hdit_lerp_bwd (d(skip), dy, d(alpha))
  Tokenizer + PE      space_to_depth(x, 1, P) + a 1x1 fp32 ConvRing with the (C, P * Cin) view of the Conv2d weight and
                      the channel-major positional embedding as its residual
  time path           differentiable torch ops on the device ([B, 256] rows): Fourier features (lc_hdit_fourier_fwd,
                      no gradient), mapping network and the 42 modulation rows in one product

dropout > 0 is refused (no shipped config sets it).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import autograd as AG
from . import ops as K


class RMSNormGrid(torch.autograd.Function):
    """y = x * rsqrt(mean_c x^2 + eps) * (1 + mod[b, c] | gain[c] | 1) on a [B, C, h, w] token grid."""

    @staticmethod
    def forward(ctx, x, mod, gain, eps):
        x = AG._c4(x)
        y = K.hdit_rmsnorm(x, mod=mod, gain=gain, eps=eps)
        ctx.save_for_backward(x, mod, gain)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mod, gain = ctx.saved_tensors
        want = (mod is not None and ctx.needs_input_grad[1]) or (gain is not None and ctx.needs_input_grad[2])
        dx, df = K.hdit_rmsnorm_bwd(x, dy, mod=mod, gain=gain, eps=ctx.eps, want_param=want)
        return dx, (df if mod is not None else None), (df if gain is not None else None), None


class GEGLUGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = AG._c4(x)
        ctx.save_for_backward(x)
        return K.hdit_geglu(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return K.hdit_geglu_bwd(x, dy)


class QKPrep(torch.autograd.Function):
    """(q', k') = normalise, clamped scale, axial RoPE of the raw q / k slices, out of place."""

    @staticmethod
    def forward(ctx, q, k, scale, cos_t, sin_t, heads):
        qp = q.clone(memory_format=torch.contiguous_format)
        kp = k.clone(memory_format=torch.contiguous_format)
        K.hdit_qk_prep(qp, kp, heads, scale, cos_t, sin_t)
        ctx.save_for_backward(q, k, scale)
        # the RoPE tables are constants of the coords buffer, cached by the model -- possibly built by a sampling run
        # under inference_mode, whose tensors save_for_backward refuses; they are held as they are
        ctx.heads, ctx.tables = heads, (cos_t, sin_t)
        return qp, kp

    @staticmethod
    def backward(ctx, gq, gk):
        q, k, scale = ctx.saved_tensors
        cos_t, sin_t = ctx.tables
        gq = torch.zeros_like(q) if gq is None else gq
        gk = torch.zeros_like(k) if gk is None else gk
        dq, dk, ds = K.hdit_qk_prep_bwd(q, k, gq, gk, ctx.heads, scale.detach(), cos_t, sin_t,
                                        want_scale=ctx.needs_input_grad[2])
        return dq, dk, ds, None, None, None


class NeighbourhoodAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, h, w, kernel_size):
        o, lse = K.hdit_na_train(q, k, v, heads, h, w, kernel_size, scale=1.0)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.geom = (heads, h, w, tuple(kernel_size))
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        heads, h, w, ks = ctx.geom
        dq, dk, dv = K.hdit_na_bwd(q, k, v, o, do, lse, heads, h, w, ks, scale=1.0)
        return dq, dk, dv, None, None, None, None


class SpaceToDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p1, p2):
        ctx.p = (p1, p2)
        return K.space_to_depth(AG._c4(x), p1, p2)

    @staticmethod
    def backward(ctx, dy):
        return K.depth_to_space(AG._c4(dy), *ctx.p), None, None


class DepthToSpace(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p1, p2):
        ctx.p = (p1, p2)
        return K.depth_to_space(AG._c4(x), p1, p2)

    @staticmethod
    def backward(ctx, dy):
        return K.space_to_depth(AG._c4(dy), *ctx.p), None, None


class ExpandLerp(torch.autograd.Function):
    """torch.lerp(skip, depth_to_space(y, 2, 2), sigmoid(alpha)) (PatchExpanding)."""

    @staticmethod
    def forward(ctx, y, skip, alpha):
        y, skip = AG._c4(y), AG._c4(skip)
        ctx.save_for_backward(y, skip, alpha)
        return K.depth_to_space(y, 2, 2, skip=skip, alpha=alpha)

    @staticmethod
    def backward(ctx, dout):
        y, skip, alpha = ctx.saved_tensors
        dy, dskip, da = K.hdit_lerp_bwd(dout, y, skip, alpha.detach(), 2, 2, want_alpha=ctx.needs_input_grad[2])
        return dy, dskip, da


class _Linear1x1:
    """An nn.Linear seen as a 1x1 conv for autograd.conv (its packs live on the Linear)."""

    def __init__(self, lin):
        self.weight, self.bias = lin.weight[:, :, None, None], lin.bias
        d = lin.__dict__
        if "_train_packed" not in d:
            d["_train_packed"] = {"fwd": K.PackedConv("train.fwd"), "bwd": K.PackedConv("train.bwd")}
        self.__dict__["_train_packed"] = d["_train_packed"]


def _lin(lin, x, res=None, precision=None):
    return AG.conv(_Linear1x1(lin), x, res=res, precision=precision)


def _rms_rows(x, scale, eps):
    """The reference's RMSNorm on [M, C] rows: (x * rsqrt(mean x^2 + eps)) * scale."""
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)) * scale


def _geglu_rows(x):
    a, g = x.chunk(2, dim=-1)
    return a * F.gelu(g)


def time_features(m, log_snr):
    """Differentiable counterpart of HDiT.time_features: (emb [B, T], modulation rows [B, sum C])."""
    rff, mapping = m.timestep_pe[0], m.timestep_pe[1]
    h = F.linear(K.hdit_fourier(log_snr.float().contiguous(), rff.freqs), rff.linear.weight)
    h = _rms_rows(h, mapping[0].scale, mapping[0].eps)
    for ffn in list(mapping)[1:-1]:
        a = _rms_rows(h, ffn.norm.scale, ffn.norm.eps)
        h = h + F.linear(_geglu_rows(F.linear(a, ffn.gegelu.weight)), ffn.linear.weight)
    emb = _rms_rows(h, mapping[-1].scale, mapping[-1].eps)
    ws = [w for b in m._blocks() for w in (b.residual_attn.norm.proj[0].weight, b.residual_ffn.adarms.proj[0].weight)]
    return emb, F.linear(emb, torch.cat(ws, 0))


def _attention(blk, x, mod, cos_t, sin_t, qk_precision):
    B, C, H, W = x.shape
    L = H * W
    heads = blk.num_heads
    a = RMSNormGrid.apply(x, mod, None, blk.norm.eps)
    t = _lin(blk.qkv_proj, a, precision=qk_precision).view(B, 3 * C, L)
    q, k, v = t.split(C, dim=1)
    qp, kp = QKPrep.apply(q, k, blk.scale, cos_t, sin_t, heads)
    if blk.local:
        o = NeighbourhoodAttention.apply(qp, kp, v, heads, H, W, blk.kernel_size)
    else:
        d = C // heads
        o = AG.FlashAttention.apply(qp.view(B, heads, d, L), kp.view(B, heads, d, L), v.reshape(B, heads, d, L), 1.0,
                                    qk_precision)
    return _lin(blk.out_proj, o.reshape(B, C, H, W), res=x)


def _ffn(ffn, x, mod):
    a = RMSNormGrid.apply(x, mod, None, ffn.adarms.eps)
    return _lin(ffn.linear, GEGLUGrid.apply(_lin(ffn.gegelu, a)), res=x)


def _tokenize(m, x):
    """Conv2d(kernel = stride = (1, P)) + positional embedding as space_to_depth + an exact 1x1 conv whose residual is
    the embedding.  The derived [C, P * Cin] weight is a new tensor every forward, so its pack is never cached (the
    allocator may return the previous step's address at version 0) and it stays out of the step's weight plan."""
    wt = m.tokenizer[0].weight                                          # [C, Cin, P1, P2]
    C, Cin, P1, P2 = wt.shape
    B = x.shape[0]
    xs = SpaceToDepth.apply(x, P1, P2)                                  # channel (p1 P2 + p2) Cin + c
    w1 = wt.permute(0, 2, 3, 1).reshape(C, P1 * P2 * Cin, 1, 1)
    pe = m.spatial_pe.embedding[0].permute(2, 0, 1)                     # [h, w, C] -> [C, h, w]
    holder = m.tokenizer[0].__dict__.setdefault(
        "_train_packed", {"fwd": K.PackedConv("train.fwd"), "bwd": K.PackedConv("train.bwd")})
    holder["fwd"]._key = None
    return AG.ConvRing.apply(xs, w1, None, holder, None, pe.expand(B, -1, -1, -1), 1.0, "f32")


def hdit_forward(m, x: torch.Tensor, log_snr: torch.Tensor) -> torch.Tensor:
    """Differentiable forward of HDiT (reference hdit.py HDiT.forward) on the Functions above."""
    from .lidargen.models.dits import hdit as H

    if any(isinstance(mod, torch.nn.Dropout) and mod.p > 0 for mod in m.modules()):
        raise NotImplementedError("HDiT training graph: dropout > 0 is not built (no shipped config sets it)")
    B = x.shape[0]
    AG.begin_training_forward(x.device)
    if log_snr.dim() == 0:
        log_snr = log_snr[None].repeat_interleave(B, dim=0)
    _, mods = time_features(m, log_snr.to(x))
    tables = m._rope_tables()
    qk_precision = H._QK_PRECISION
    h = _tokenize(m, x.float())
    it = iter(tables)
    off = 0

    def run(blocks, h):
        nonlocal off
        for b in blocks:
            C = h.shape[1]
            cos_t, sin_t = next(it)
            h = _attention(b.residual_attn, h, mods[:, off:off + C], cos_t, sin_t, qk_precision)
            h = _ffn(b.residual_ffn, h, mods[:, off + C:off + 2 * C])
            off += 2 * C
        return h

    n = len(m.depths) - 1
    stack = []
    for i in range(n):
        h = run(m.down_levels[f"level_{i}"], h)
        stack.append(h)
        h = _lin(m.down_levels[f"merge_{i}"][1], SpaceToDepth.apply(h, 2, 2))
    h = run(m.mid_levels, h)
    for i in reversed(range(n)):
        ex = m.up_levels[f"expand_{i}"]
        h = ExpandLerp.apply(_lin(ex.linear, h), stack.pop(), ex.alpha)
        h = run(m.up_levels[f"level_{i}"], h)
    det = m.detokenizer
    a = RMSNormGrid.apply(h, None, det[0].scale, det[0].eps)
    return DepthToSpace.apply(_lin(det[1], a), *det.patch_size)
