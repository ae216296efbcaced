"""HDiT: the Hourglass Diffusion Transformer range-image generator on the gfx950 kernels.

API / state_dict mirror of the reference's `lidargen/models/dits/hdit.py` (itself after k-diffusion's
image_transformer_v2): module names, parameter and buffer keys (`coords`, `timestep_pe.0.freqs`, every
`...rope.freqs_h / freqs_w`) are the reference's, so its checkpoints load as they are.  The reference needs natten, the
CUDA neighbourhood-attention library; here the whole forward runs on the channel-major token grid [B, C, h, w]:

  * every Linear is a 1x1 conv (`K.conv2d_ring`, f16x2 kernels), the residual adds its `res` operand;
  * (Ada)RMSNorm, GEGLU, the q / k preparation (normalise, clamped scale, axial RoPE), the neighbourhood attention,
    the patch permutes, the tokenizer and the Fourier features are csrc/hdit.hip; the mid level's global attention is
    `K.attention_cm` with scale 1;
  * the time path (`time_features`): emb and the 42 AdaRMSNorm modulation rows of all blocks (one `lc_linear_fwd` on
    the concatenated weights) once per sampling run, so a step's graph holds the spatial network only;
  * derived tensors -- the RoPE cos / sin tables of every block (from the `coords` buffer and the block's frequencies),
    the channel-major positional embedding, the concatenated modulation weights -- are rebuilt when their sources
    change (address / version) and the rebuild bumps the pack epoch, so no captured step graph reads a stale table.

Training (lidarcrafter_amd/autograd_hdit.py): a forward builds an autograd graph over the HIP backward kernels when grad
mode is on, something requires grad AND the module is in train mode -- the state `ddpm.train()` leaves it in, as in the
reference's training scripts.  An eval-mode forward in grad mode still raises: the inference forward is not a graph (in-place
q / k preparation, detached caches), and EfficientUNet's rule (the graph follows grad mode alone) would silently swap the
sampler's inference kernels for the slower training composition wherever a caller forgot `torch.no_grad()`.
"""
from __future__ import annotations

import math
import os
from typing import List

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.modules.utils import _pair

from lidarcrafter_amd import autograd as AG
from lidarcrafter_amd import ops as K

from ..unets import encoding, ops


# arithmetic of the qkv projections and of the mid level's global attention ("f32": exact fp32 MFMA kernels; "f16x2":
# the default split of the other projections).  LC_HDIT_QK_PRECISION=f16x2 is a developer A/B switch.
_QK_PRECISION = os.environ.get("LC_HDIT_QK_PRECISION", "f32")


def _ver(t: torch.Tensor) -> int:
    try:
        return t._version
    except RuntimeError:        # inference-mode tensors carry no version counter
        return -1


def _sig(*ts) -> tuple:
    return tuple((t.data_ptr(), _ver(t), t.device) for t in ts)


def _w1x1(lin: nn.Linear) -> torch.Tensor:
    return lin.weight[:, :, None, None]


class RMSNorm(nn.Module):
    """Parameter container of the reference's RMSNorm (x * rsqrt(mean x^2 + eps) * scale); applied by ops.hdit_rmsnorm."""

    def __init__(self, in_dim: int, scale: bool = True, eps: float = 1e-6):
        super().__init__()
        self.in_dim, self.eps = in_dim, eps
        self.scale = nn.Parameter(torch.ones(in_dim)) if scale else 1.0


class AdaRMSNorm(RMSNorm):
    def __init__(self, in_dim: int, embed_dim: int):
        super().__init__(in_dim, scale=False)
        # (the reference's Rearrange("B C -> B 1 1 C") at index 1 holds no parameters)
        self.proj = nn.Sequential(nn.Linear(embed_dim, in_dim, bias=False).apply(ops.zero_out), nn.Identity())


class AxialRoPE(nn.Module):
    def __init__(self, dim: int, num_heads: int, max_harmonics: List[int]):
        super().__init__()
        freqs_h = self.setup_freqs(num_heads * dim // 4, int(max_harmonics[0]))
        freqs_w = self.setup_freqs(num_heads * dim // 4, int(max_harmonics[1]))
        self.register_buffer("freqs_h", freqs_h.view(dim // 4, num_heads).T)
        self.register_buffer("freqs_w", freqs_w.view(dim // 4, num_heads).T)

    @staticmethod
    def setup_freqs(dim: int, max_harmonics: int):
        return torch.linspace(math.log(1), math.log(max_harmonics), dim).exp().round()


class GlobalSelfAttentionBlock(nn.Module):
    local = False

    def __init__(self, dim: int, embed_dim: int, num_heads: int, dropout: float = 0.0,
                 rope_max_harmonics: List[int] = (1, 1), bias=False, eps=1e-6):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.eps = eps
        self.norm = AdaRMSNorm(dim, embed_dim)
        self.scale = nn.Parameter(torch.full([num_heads, 1], math.log(10.0)))
        self.qkv_proj = nn.Linear(dim, dim * 3, bias=bias)
        self.rope = AxialRoPE(self.head_dim, num_heads, rope_max_harmonics)
        self.dropout = nn.Dropout(dropout)
        self.out_proj = nn.Linear(dim, dim, bias=bias).apply(ops.zero_out)
        self._pk_qkv, self._pk_out = K.PackedConv(), K.PackedConv()

    def forward(self, x, mod, cos_t, sin_t):
        """x + out_proj(attn(q, k, v)) with q, k, v from qkv_proj(AdaRMSNorm(x)); x [B, C, h, w], mod [B, C] rows."""
        B, C, H, W = x.shape
        a = K.hdit_rmsnorm(x, mod=mod, eps=self.norm.eps)
        # q and k enter logits of up to 100 (unit vectors times sqrt(100) each): the projection and the global attention
        # take the exact fp32 kernels, whose operand error the logits scale up 100-fold less than the f16x2 split's
        t = K.conv2d_ring(a, self._pk_qkv, _w1x1(self.qkv_proj), precision=_QK_PRECISION).view(B, 3 * C, H * W)
        q, k, v = t[:, :C], t[:, C:2 * C], t[:, 2 * C:]
        K.hdit_qk_prep(q, k, self.num_heads, self.scale, cos_t, sin_t)        # in place: scale_qk + apply_rope_qk
        if self.local:
            o = K.hdit_na(q, k, v, self.num_heads, H, W, self.kernel_size, scale=1.0)
        else:
            o = K.attention_cm(q, k, v, self.num_heads, scale=1.0, precision=_QK_PRECISION)
        return K.conv2d_ring(o.view(B, C, H, W), self._pk_out, _w1x1(self.out_proj), res=x)


class CircularNeighborhoodSelfAttentionBlock(GlobalSelfAttentionBlock):
    local = True

    def __init__(self, dim: int, embed_dim: int, num_heads: int, kernel_size: List[int], dilation: List[int] = 1,
                 dropout: float = 0.0, rope_max_harmonics: List[int] = (1, 1)):
        super().__init__(dim=dim, embed_dim=embed_dim, num_heads=num_heads, dropout=dropout,
                         rope_max_harmonics=rope_max_harmonics)
        self.kernel_size = _pair(kernel_size)
        self.dilation = _pair(dilation)
        if self.dilation != (1, 1):
            raise NotImplementedError(f"HDiT: dilation={self.dilation} -- dilated neighbourhood windows are not built "
                                      "(no shipped config uses them)")
        if self.kernel_size[0] % 2 == 0 or self.kernel_size[1] % 2 == 0:
            raise ValueError(f"HDiT: window_size={self.kernel_size} must be odd")


class PatchMerging(nn.Sequential):
    def __init__(self, dim: int):
        # (index 0: the reference's Rearrange "B (H P1) (W P2) C -> B H W (P1 P2 C)")
        super().__init__(nn.Identity(), nn.Linear(4 * dim, 2 * dim, bias=False))
        self._pk = K.PackedConv()

    def forward(self, x):
        return K.conv2d_ring(K.space_to_depth(x, 2, 2), self._pk, _w1x1(self[1]))


class PatchExpanding(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.linear = nn.Linear(dim, dim * 2, bias=False)
        self.alpha = nn.Parameter(torch.zeros(dim // 2))
        self._pk = K.PackedConv()

    def forward(self, x, skip):
        y = K.conv2d_ring(x, self._pk, _w1x1(self.linear))
        return K.depth_to_space(y, 2, 2, skip=skip, alpha=self.alpha)


class Tokenizer(nn.Sequential):
    def __init__(self, in_channels: int, out_channels: int, patch_size: List[int]):
        patch_size = _pair(patch_size)
        super().__init__(nn.Conv2d(in_channels, out_channels, kernel_size=patch_size, stride=patch_size, padding=0,
                                   bias=False), nn.Identity())


class Detokenizer(nn.Sequential):
    def __init__(self, in_channels: int, out_channels: int, patch_size: List[int]):
        patch_size = _pair(patch_size)
        super().__init__(RMSNorm(in_channels),
                         nn.Linear(in_channels, out_channels * patch_size[0] * patch_size[1],
                                   bias=False).apply(ops.zero_out),
                         nn.Identity())
        self.patch_size = patch_size
        self._pk = K.PackedConv()

    def forward(self, x):
        a = K.hdit_rmsnorm(x, gain=self[0].scale, eps=self[0].eps)
        return K.depth_to_space(K.conv2d_ring(a, self._pk, _w1x1(self[1])), *self.patch_size)


class GEGLU(nn.Linear):
    def __init__(self, in_features, out_features, bias):
        super().__init__(in_features, out_features * 2, bias=bias)


class FeedForwardNetwork(nn.Module):
    def __init__(self, dim, mid_dim, embed_dim, dropout=0.0):
        super().__init__()
        self.adarms = AdaRMSNorm(dim, embed_dim)
        self.gegelu = GEGLU(dim, mid_dim, bias=False)
        self.dropout = nn.Dropout(dropout)
        self.linear = nn.Linear(mid_dim, dim, bias=False).apply(ops.zero_out)
        self._pk_g, self._pk_l = K.PackedConv(), K.PackedConv()

    def forward(self, x, mod):
        a = K.hdit_rmsnorm(x, mod=mod, eps=self.adarms.eps)
        u = K.hdit_geglu(K.conv2d_ring(a, self._pk_g, _w1x1(self.gegelu)))
        return K.conv2d_ring(u, self._pk_l, _w1x1(self.linear), res=x)


class Block(nn.Module):
    def __init__(self, in_dim: int, time_embed_dim: int, num_heads: int, attn_type: str = "global",
                 kernel_size: List[int] = None, dilation: List[int] = 1, rope_max_harmonics: List[int] = (1, 1),
                 mlp_ratio: float = 3.0, dropout: float = 0.0):
        super().__init__()
        if attn_type == "global":
            self.residual_attn = GlobalSelfAttentionBlock(dim=in_dim, embed_dim=time_embed_dim, num_heads=num_heads,
                                                          dropout=dropout, rope_max_harmonics=rope_max_harmonics)
        else:
            self.residual_attn = CircularNeighborhoodSelfAttentionBlock(
                dim=in_dim, embed_dim=time_embed_dim, num_heads=num_heads, kernel_size=kernel_size, dilation=dilation,
                dropout=dropout, rope_max_harmonics=rope_max_harmonics)
        self.residual_ffn = FeedForwardNetwork(dim=in_dim, mid_dim=int(in_dim * mlp_ratio), embed_dim=time_embed_dim,
                                               dropout=dropout)

    def forward(self, x, mod_attn, mod_ffn, cos_t, sin_t):
        x = self.residual_attn(x, mod_attn, cos_t, sin_t)
        return self.residual_ffn(x, mod_ffn)


class RandomFourierFeatures(nn.Module):
    def __init__(self, dim, std=1.0):
        super().__init__()
        self.register_buffer("freqs", torch.randn(dim // 2) * std)
        self.linear = nn.Linear(dim, dim, bias=False)


class MappingFeedForwardNetwork(nn.Module):
    def __init__(self, dim, mid_dim, dropout=0.0):
        super().__init__()
        self.norm = RMSNorm(dim)
        self.gegelu = GEGLU(dim, mid_dim, bias=False)
        self.dropout = nn.Dropout(dropout)
        self.linear = nn.Linear(mid_dim, dim, bias=False).apply(ops.zero_out)


class MappingNetwork(nn.Sequential):
    def __init__(self, dim, mid_dim, depth=1, dropout=0.0):
        super().__init__(RMSNorm(dim), *[MappingFeedForwardNetwork(dim, mid_dim, dropout) for _ in range(depth)],
                         RMSNorm(dim))


class LearnablePositionalEmbedding(nn.Module):
    def __init__(self, out_dim: int, resolution: List[int]):
        super().__init__()
        self.embedding = nn.Parameter(torch.zeros(1, *resolution, out_dim))
        nn.init.trunc_normal_(self.embedding, std=0.02)


class HDiT(nn.Module):
    def __init__(self, resolution: List[int], in_channels: int, out_channels: int | None = None,
                 base_channels: int = 128, time_embed_channels: int = 256, patch_size: List[int] = (1, 4),
                 window_size: List[int] = (3, 9), depths: List[int] = (2, 2, 2, 2),
                 num_heads: List[int] = (2, 4, 8, 16), dilation: List[int] = (1, 1, 1, 1), mlp_ratio: float = 3.0,
                 dropout: float = 0.0, mapping_depth: int = 2, positional_embedding: str = "learnable_embedding",
                 ring: bool = True):
        """`ring` is accepted and unused, as in the reference."""
        super().__init__()
        if positional_embedding != "learnable_embedding":
            raise NotImplementedError(f"HDiT: positional_embedding={positional_embedding!r} is not built (only "
                                      "'learnable_embedding', the one of nuscenes-hdit-uncond)")
        if any(int(d) != 1 for d in dilation):
            raise NotImplementedError(f"HDiT: dilation={tuple(dilation)} -- dilated neighbourhood windows are not "
                                      "built (no shipped config uses them)")
        self.resolution = _pair(resolution)
        self.in_channels = in_channels
        self.out_channels = out_channels if out_channels else in_channels
        self.patch_size = _pair(patch_size)
        self.depths = depths
        self.register_buffer("coords", encoding.generate_polar_coords(*self.resolution))
        token_size = torch.tensor(self.resolution) // torch.tensor(self.patch_size)
        self.spatial_pe = LearnablePositionalEmbedding(out_dim=base_channels, resolution=token_size.tolist())
        self.timestep_pe = nn.Sequential(
            RandomFourierFeatures(time_embed_channels),
            MappingNetwork(time_embed_channels, int(time_embed_channels * mlp_ratio), depth=mapping_depth))
        self.tokenizer = Tokenizer(in_channels=in_channels, out_channels=base_channels, patch_size=patch_size)
        max_harmonics = (token_size / 2).int()
        self.down_levels = nn.ModuleDict()
        self.up_levels = nn.ModuleDict()
        for i, num_blocks in enumerate(depths[:-1]):
            kw = dict(in_dim=base_channels << i, time_embed_dim=time_embed_channels, num_heads=num_heads[i],
                      attn_type="local", kernel_size=window_size, mlp_ratio=mlp_ratio, dropout=dropout,
                      rope_max_harmonics=(max_harmonics >> i).clamp(min=1))
            self.down_levels[f"level_{i}"] = nn.ModuleList(
                [Block(dilation=1 if j % 2 == 0 else dilation[i], **kw) for j in range(num_blocks)])
            self.down_levels[f"merge_{i}"] = PatchMerging(base_channels << i)
            self.up_levels[f"level_{i}"] = nn.ModuleList(
                [Block(dilation=1 if j % 2 == 0 else dilation[i], **kw) for j in range(num_blocks)])
            self.up_levels[f"expand_{i}"] = PatchExpanding(base_channels << (i + 1))
        i = len(depths) - 1
        self.mid_levels = nn.ModuleList([
            Block(in_dim=base_channels << i, time_embed_dim=time_embed_channels, num_heads=num_heads[-1],
                  attn_type="global", mlp_ratio=mlp_ratio, dropout=dropout,
                  rope_max_harmonics=(max_harmonics >> i).clamp(min=1))
            for _ in range(depths[-1])])
        self.detokenizer = Detokenizer(in_channels=base_channels, out_channels=self.out_channels,
                                       patch_size=patch_size)
        self.nfe = 0
        self._mod_cache = self._rope_cache = self._pe_cache = None

    # ---- derived tensors (rebuilt when their sources change) ---------------------------------------------------
    def _levels(self):
        """[(blocks, level index)] in forward order: down 0 .. n-2, mid, up n-2 .. 0."""
        n = len(self.depths) - 1
        out = [(self.down_levels[f"level_{i}"], i) for i in range(n)]
        out.append((self.mid_levels, n))
        out += [(self.up_levels[f"level_{i}"], i) for i in reversed(range(n))]
        return out

    def _blocks(self):
        return [b for blocks, _ in self._levels() for b in blocks]

    def _mod_weights(self):
        """All AdaRMSNorm projections of the forward, concatenated [sum C, T] (two per block: attention, FFN)."""
        ws = [w for b in self._blocks() for w in (b.residual_attn.norm.proj[0].weight,
                                                  b.residual_ffn.adarms.proj[0].weight)]
        key = _sig(*ws)
        if self._mod_cache is None or self._mod_cache[0] != key:
            self._mod_cache = (key, torch.cat([w.detach() for w in ws], 0).contiguous())
            K.bump_epoch()
        return self._mod_cache[1]

    def _pe(self):
        e = self.spatial_pe.embedding
        key = _sig(e)
        if self._pe_cache is None or self._pe_cache[0] != key:
            self._pe_cache = (key, e.detach()[0].permute(2, 0, 1).contiguous())     # [h, w, C] -> [C, h, w]
            K.bump_epoch()
        return self._pe_cache[1]

    def _rope_tables(self):
        """Per block (forward order) the RoPE (cos, sin) tables [heads, d/2, h*w] of its level: theta = (c_h freqs_h |
        c_w freqs_w) with (c_h, c_w) the `coords` buffer average-pooled by the patch size, then by 2 per level."""
        blocks = self._blocks()
        srcs = [self.coords] + [t for b in blocks for t in (b.residual_attn.rope.freqs_h, b.residual_attn.rope.freqs_w)]
        key = _sig(*srcs)
        if self._rope_cache is None or self._rope_cache[0] != key:
            with torch.no_grad():
                c = F.avg_pool2d(self.coords.detach().float(), self.patch_size, self.patch_size)
                cs = [c]
                for _ in range(len(self.depths) - 1):
                    cs.append(F.avg_pool2d(cs[-1], 2, 2))
                tables = []
                for blocks_, lvl in self._levels():
                    ch, cw = cs[lvl][0, 0].reshape(-1), cs[lvl][0, 1].reshape(-1)
                    for b in blocks_:
                        rope = b.residual_attn.rope
                        th = torch.cat([ch[None, None, :] * rope.freqs_h.float()[:, :, None],
                                        cw[None, None, :] * rope.freqs_w.float()[:, :, None]], 1)
                        tables.append((th.cos().contiguous(), th.sin().contiguous()))
            self._rope_cache = (key, tables)
            K.bump_epoch()
        return self._rope_cache[1]

    # ---- time path -----------------------------------------------------------------------------------------------
    def time_features(self, log_snr: torch.Tensor):
        """log-SNR [M] -> (emb [M, T], the AdaRMSNorm modulation rows of every block [M, sum C])."""
        rff, mapping = self.timestep_pe[0], self.timestep_pe[1]
        h = K.linear(K.hdit_fourier(log_snr.float(), rff.freqs), rff.linear.weight)
        h = K.hdit_rmsnorm(h, gain=mapping[0].scale, eps=mapping[0].eps)
        for ffn in list(mapping)[1:-1]:
            a = K.hdit_rmsnorm(h, gain=ffn.norm.scale, eps=ffn.norm.eps)
            r = K.linear(K.hdit_geglu(K.linear(a, ffn.gegelu.weight)), ffn.linear.weight)
            h = K.add_scale(h[:, :, None, None], r[:, :, None, None], 1.0)[:, :, 0, 0]
        emb = K.hdit_rmsnorm(h, gain=mapping[-1].scale, eps=mapping[-1].eps)
        return emb, K.linear(emb, self._mod_weights())

    # ---- forward ---------------------------------------------------------------------------------------------------
    @torch.compiler.disable
    @K.range_checked
    def forward(self, x: torch.Tensor, t: torch.Tensor, *args, time_features=None, **kwargs) -> torch.Tensor:
        """x [B, C, H, W], t = log-SNR [B] (or 0-d) -> [B, C_out, H, W].  `time_features`: optional precomputed
        `self.time_features(log_snr)` (the sampler hoists them out of the steps)."""
        if AG.training_active(self, x):
            if not self.training:
                raise NotImplementedError("HDiT training is not built for eval-mode forwards: call .train(), or run "
                                          "under torch.no_grad()")
            if not x.is_cuda:
                raise NotImplementedError("HDiT runs on the GPU kernels only; there is no CPU path")
            from lidarcrafter_amd.autograd_hdit import hdit_forward

            self.nfe += 1
            return hdit_forward(self, x, t)
        if not x.is_cuda:
            raise NotImplementedError("HDiT runs on the GPU kernels only; there is no CPU path")
        B = x.shape[0]
        if time_features is None:
            if t.dim() == 0:
                t = t[None].repeat_interleave(B, dim=0)
            time_features = self.time_features(t.to(x))
        mods = time_features[1]
        tables = self._rope_tables()
        h = K.hdit_tokenize(x, self.tokenizer[0].weight, self._pe())
        it = iter(range(len(tables)))
        off = [0]

        def run(blocks, h):
            for b in blocks:
                C = h.shape[1]
                o = off[0]
                cos_t, sin_t = tables[next(it)]
                h = b(h, mods[:, o:o + C], mods[:, o + C:o + 2 * C], cos_t, sin_t)
                off[0] = o + 2 * C
            return h

        n = len(self.depths) - 1
        stack = []
        for i in range(n):
            h = run(self.down_levels[f"level_{i}"], h)
            stack.append(h)
            h = self.down_levels[f"merge_{i}"](h)
        h = run(self.mid_levels, h)
        for i in reversed(range(n)):
            h = self.up_levels[f"expand_{i}"](h, stack.pop())
            h = run(self.up_levels[f"level_{i}"], h)
        self.nfe += 1
        return self.detokenizer(h)
