"""Denoiser of the scene-graph layout generator -- constructor signature, module tree and `state_dict` keys of the
reference's lidargen/models/unets/unet_1d.py:368-717 (`UNet1DModel`), so a reference checkpoint loads strictly.

The signal has length 1 (one 20-vector per object), which makes the operator set degenerate:
every `Conv1d(k=3, padding=1)` is its centre tap, `Downsample` / `Upsample` are dense layers, GroupNorm / LayerNorm are
per-row statistics, attention over one key is `to_out(to_v(context))` (`to_q` / `to_k` stay in the checkpoint and are
never read), eval-mode BatchNorm folds into the `Linear` in front of it.  `pack_layout_gen` turns the module tree into a
flat PROGRAM of four op kinds over named row-major buffers,

    ("gemm", out, segments, w, bias, act, vec, res)    csrc/layout_gen.hip lc_skinny_gemm_fwd + lc_skinny_combine_fwd
    ("prep", out, segments, groups, eps, gamma, beta, silu)                  lc_rowprep_fwd
    ("pool", out, src, s_col, o_col, H)                                      lc_graph_pool_fwd
    ("temb", out, src)                                                       lc_time_embed_fwd

with the time path hoisted (time_embed, all ResBlock `emb_layers` as ONE product and `box_time_emb` are evaluated per
DISTINCT time value, rows index into the result).  `forward` runs the program on the HIP kernels; `run_program_torch`
evaluates the same program on the same packed operands with torch ops in any dtype (tests pin the pack's algebra on the
reference's float64 output with it, before any kernel runs).  There is no eager-PyTorch route through `forward`."""
from __future__ import annotations

import math

import torch
from torch import nn

from .graph import GraphTripleConvNet, _init_weights, edge_csr

TRAINING_MSG = ("layout generator training is not built (BatchNorm batch statistics and the backward kernels of the "
                "skinny dense layers are the next step): call .eval() and run under torch.no_grad()")


# Pack-time algebra switch, measured in profiles/layout_gen.txt: fold `to_out . to_v` of every one-key attention into ONE
# matrix (22 dense layers fewer per step).  Exact algebra, other rounding; off by default: the default is what every
# parity test ran with.
FOLD_ATTENTION_VALUE = False


def _zero(m):
    for p in m.parameters():
        p.detach().zero_()
    return m


class ResBlock(nn.Module):
    def __init__(self, channels, emb_channels, out_channels=None):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels or channels
        self.in_layers = nn.Sequential(nn.GroupNorm(32, channels), nn.SiLU(),
                                       nn.Conv1d(channels, self.out_channels, 3, padding=1))
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, self.out_channels))
        self.out_layers = nn.Sequential(nn.GroupNorm(32, self.out_channels), nn.SiLU(), nn.Dropout(p=0),
                                        _zero(nn.Conv1d(self.out_channels, self.out_channels, 3, padding=1)))
        self.skip_connection = (nn.Identity() if self.out_channels == channels
                                else nn.Conv1d(channels, self.out_channels, 1))


class Downsample(nn.Module):
    def __init__(self, channels, out_channels=None):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels or channels
        self.op = nn.Conv1d(channels, self.out_channels, 3, stride=2, padding=1)


class Upsample(nn.Module):
    def __init__(self, channels, out_channels=None):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels or channels
        self.conv = nn.Conv1d(channels, self.out_channels, 3, padding=1)


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.Sequential(GEGLU(dim, dim * mult), nn.Dropout(0.0), nn.Linear(dim * mult, dim))


class CrossAttention(nn.Module):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64):
        super().__init__()
        inner = dim_head * heads
        context_dim = query_dim if context_dim is None else context_dim
        self.heads, self.scale = heads, dim_head ** -0.5
        self.to_q = nn.Linear(query_dim, inner, bias=False)       # one query, one key: the softmax is 1, to_q / to_k
        self.to_k = nn.Linear(context_dim, inner, bias=False)     # never reach the output (checkpoint keys only)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(0.0))


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, d_head, context_dim=None):
        super().__init__()
        self.attn1 = CrossAttention(dim, heads=n_heads, dim_head=d_head)
        self.ff = FeedForward(dim)
        self.attn2 = CrossAttention(dim, context_dim=context_dim, heads=n_heads, dim_head=d_head)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)


class SpatialTransformer1D(nn.Module):
    def __init__(self, in_channels, n_heads, d_head, depth=1, context_dim=None):
        super().__init__()
        self.in_channels = in_channels
        inner = n_heads * d_head
        self.norm = nn.GroupNorm(32, in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Conv1d(in_channels, inner, 1)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner, n_heads, d_head, context_dim=context_dim) for _ in range(depth)])
        self.proj_out = _zero(nn.Conv1d(inner, in_channels, 1))


def _refuse(name, value, why="is not built for the layout generator"):
    raise NotImplementedError(f"UNet1DModel: {name}={value!r} {why} (the shipped nuscenes-layout config does not set it)")


class UNet1DModel(nn.Module):
    def __init__(self, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=1, use_checkpoint=False, use_fp16=False,
                 num_heads=-1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False,
                 resblock_updown=False, use_new_attention_order=False, use_spatial_transformer=False,
                 transformer_depth=1, concat_dim=None, crossattn_dim=None, conditioning_key="crossattn",
                 using_clip=True, enable_t_emb=False):
        super().__init__()
        if conditioning_key != "crossattn":
            _refuse("conditioning_key", conditioning_key)
        if not use_spatial_transformer:
            _refuse("use_spatial_transformer", use_spatial_transformer)
        if use_scale_shift_norm:
            _refuse("use_scale_shift_norm", use_scale_shift_norm)
        if resblock_updown:
            _refuse("resblock_updown", resblock_updown)
        if num_head_channels != -1:
            _refuse("num_head_channels", num_head_channels)
        if num_heads == -1:
            _refuse("num_heads", num_heads, "must be set")
        if dropout != 0:
            _refuse("dropout", dropout)
        if use_fp16:
            _refuse("use_fp16", use_fp16)
        if dims != 1:
            _refuse("dims", dims)
        if not enable_t_emb:
            _refuse("enable_t_emb", enable_t_emb)
        if not conv_resample:
            _refuse("conv_resample", conv_resample)
        if crossattn_dim is None:
            _refuse("crossattn_dim", crossattn_dim, "must be set")
        if model_channels % 32 != 0 or model_channels % 2 != 0:
            _refuse("model_channels", model_channels, "must be a multiple of 32")
        context_dim = int(crossattn_dim)
        if concat_dim != context_dim:
            _refuse("concat_dim", concat_dim, "must equal crossattn_dim (the graph network's output is the context)")
        self.conditioning_key, self.using_clip = conditioning_key, using_clip
        self.in_channels, self.resolution = in_channels, (1,)
        self.model_channels, self.out_channels = model_channels, out_channels
        self.num_res_blocks, self.attention_resolutions = num_res_blocks, attention_resolutions
        self.dropout, self.channel_mult, self.conv_resample = dropout, channel_mult, conv_resample
        self.use_checkpoint, self.dtype = use_checkpoint, torch.float32
        self.num_heads, self.num_head_channels = num_heads, num_head_channels
        self.num_heads_upsample = num_heads if num_heads_upsample == -1 else num_heads_upsample

        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.SiLU(), nn.Linear(ted, ted))

        def st(ch):
            return SpatialTransformer1D(ch, num_heads, ch // num_heads, depth=transformer_depth, context_dim=context_dim)

        self.input_blocks = nn.ModuleList([nn.Sequential(nn.Conv1d(in_channels, model_channels, 3, padding=1))])
        chans, ch, ds = [model_channels], model_channels, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, ted, out_channels=mult * model_channels)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(st(ch))
                self.input_blocks.append(nn.Sequential(*layers))
                chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(nn.Sequential(Downsample(ch, out_channels=ch)))
                chans.append(ch)
                ds *= 2
        self.middle_block = nn.Sequential(ResBlock(ch, ted), st(ch), ResBlock(ch, ted))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [ResBlock(ch + ich, ted, out_channels=model_channels * mult)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(st(ch))
                if level and i == num_res_blocks:
                    layers.append(Upsample(ch, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(nn.Sequential(*layers))
        self.out = nn.Sequential(nn.GroupNorm(32, ch), nn.SiLU(),
                                 _zero(nn.Conv1d(model_channels, out_channels, 3, padding=1)))

        gconv_dim = 64
        add_dim = 512 if using_clip else 0
        self.pred_embeddings = nn.Embedding(16, gconv_dim * 2)
        self.box_embeddings = nn.Linear(in_channels, gconv_dim)
        self.box_embeddings.apply(_init_weights)
        self.enable_t_emb = enable_t_emb
        self.box_time_emb = nn.Linear(ted, gconv_dim)
        self.box_graph_cov = GraphTripleConvNet(
            input_dim_obj=gconv_dim * 2 + add_dim + gconv_dim + gconv_dim, input_dim_pred=gconv_dim * 2,
            hidden_dim=gconv_dim * 4, pooling="avg", num_layers=5, mlp_normalization="batch", residual=True,
            output_dim=concat_dim)
        self.__dict__["_pack"] = None          # (fingerprint, program): rebuilt when any weight changes

    # ---- packed operands -------------------------------------------------------------------------------------------
    def _fingerprint(self):
        """(address, version) of every parameter and buffer, or None when one of them is an inference tensor: those
        carry no version counter, an in-place change could not be seen, so the pack is then rebuilt on every call."""
        fp = []
        for t in list(self.parameters()) + list(self.buffers()):
            if t.is_inference():
                return None
            fp.append((t.data_ptr(), t._version, t.device, t.dtype))
        fp.append(FOLD_ATTENTION_VALUE)
        return tuple(fp)

    def packed(self):
        """The program over packed operands of the CURRENT weights (pack epoch: rebuilt, and ops.bump_epoch() called,
        whenever a parameter or buffer was replaced or written in place since the last pack)."""
        fp = self._fingerprint()
        cur = self.__dict__.get("_pack")
        if cur is None or fp is None or cur[0] != fp:
            from lidarcrafter_amd import ops as K

            with torch.no_grad():
                cur = (fp, pack_layout_gen(self))
            self.__dict__["_pack"] = cur
            K.bump_epoch()
        return cur[1]

    def _apply(self, fn, *a, **k):
        self.__dict__["_pack"] = None
        return super()._apply(fn, *a, **k)

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_pack"] = None
        return d

    # ---- the HIP path ----------------------------------------------------------------------------------------------
    def _guard(self, box_t):
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(TRAINING_MSG)
        from lidarcrafter_amd import ops as K

        K._req(box_t, "box_t")

    def make_plan(self, uc_b, triples, num_times=1, time_rows=None):
        """Buffers, index arrays and launch arguments of one (objects, triples, distinct times) problem; built once per
        `sample()` call (or per plain forward), nothing is allocated afterwards."""
        return _Plan(self, uc_b, triples, num_times, time_rows)

    def run_plan(self, plan, box_t=None, times=None):
        """One denoiser evaluation on the plan's buffers; box_t / times are copied into them when given (a sampler
        works in place on plan.x / plan.t).  -> plan.y [O, out_channels]."""
        if box_t is not None:
            plan.x.copy_(box_t)
        if times is not None:
            plan.t.copy_(times)
        plan.run()
        return plan.y

    def forward(self, box_t, cond_dict):
        self._guard(box_t)
        other = cond_dict["other_condition"]
        times = cond_dict["time_condition"].to(device=box_t.device, dtype=torch.float32).reshape(-1)
        tvals, tidx = torch.unique(times, return_inverse=True)
        with torch.cuda.device(box_t.device):
            plan = self.make_plan(other["uc_b"], other["preds"], tvals.numel(), tidx)
            return self.run_plan(plan, box_t.to(torch.float32), tvals).clone()


# ------------------------------------------------------------------------------------------------------ the program
def timestep_freqs(dim, max_period=10000):
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)


def _fold_bn(lin, bn):
    """Linear followed by eval-mode BatchNorm1d as one affine map."""
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return lin.weight * s[:, None], (lin.bias - bn.running_mean) * s + bn.bias


class Program:
    def __init__(self):
        self.ops, self.bufs, self.w = [], {}, {}
        self.tags, self.section = [], "time"       # per op: time | gcn | res | attn | io (devtools/layout_gen_time.py)
        self.modules = {}      # state_dict prefix of a torso layer -> (first op, last op, input segments, output buffer)
        self.context = None    # buffer of the cross-attention context (the graph network's output)

    def buf(self, name, kind, width):
        prev = self.bufs.setdefault(name, (kind, width))
        assert prev == (kind, width), (name, prev, kind, width)
        return name

    def weight(self, name, t):
        if t is not None:
            self.w[name] = t.detach().contiguous()
            return name
        return None


def pack_layout_gen(m: UNet1DModel) -> Program:
    """Module tree -> program.  Operands keep the dtype / device of the module (float64 modules give a float64 program
    for `run_program_torch`)."""
    P = Program()
    C, ted = m.model_channels, m.model_channels * 4
    cnt = [0]

    def uid(prefix):
        cnt[0] += 1
        return f"{prefix}{cnt[0]}"

    def full(name):
        return (name, 0, P.bufs[name][1], None)

    def gemm(out, kind, segs, w, b, act=None, vec=None, res=None):
        n = uid("w")
        N = w.shape[0]
        P.buf(out, kind, N // 2 if act == "geglu" else N)
        P.ops.append(("gemm", out, tuple(segs), P.weight(n, w), P.weight(n + "b", b), act, vec, res))
        P.tags.append(P.section)
        return out

    def prep(out, kind, segs, groups=0, eps=1e-5, gamma=None, beta=None, silu=False):
        n = uid("n")
        P.buf(out, kind, sum(s[2] for s in segs))
        P.ops.append(("prep", out, tuple(segs), groups, eps, P.weight(n + "g", gamma), P.weight(n + "b", beta), silu))
        P.tags.append(P.section)
        return out

    def centre(conv):
        return conv.weight[:, :, conv.weight.shape[2] // 2]

    # inputs
    P.buf("x", "O", m.in_channels), P.buf("t", "U1", 1), P.buf("uc_b", "O", m.box_graph_cov.gconvs[0].input_dim_obj - 128)
    P.buf("pred0", "T", 128)
    # ---- time path, per distinct time value
    P.buf("temb", "U", C)
    P.ops.append(("temb", "temb", "t"))
    P.tags.append("time")
    gemm("te1", "U", [full("temb")], m.time_embed[0].weight, m.time_embed[0].bias)
    prep("te1s", "U", [full("te1")], silu=True)
    gemm("emb", "U", [full("te1s")], m.time_embed[2].weight, m.time_embed[2].bias)
    gemm("box_t_emb", "U", [full("emb")], m.box_time_emb.weight, m.box_time_emb.bias)
    prep("embs", "U", [full("emb")], silu=True)
    resblocks = [b for b in m.modules() if isinstance(b, ResBlock)]
    gemm("embproj", "U", [full("embs")], torch.cat([b.emb_layers[1].weight for b in resblocks], 0),
         torch.cat([b.emb_layers[1].bias for b in resblocks], 0))
    emb_off, o = {}, 0
    for b in resblocks:
        emb_off[id(b)] = o
        o += b.out_channels
    # ---- graph network -> cross-attention context
    P.section = "gcn"
    gemm("box_e", "O", [full("x")], m.box_embeddings.weight, m.box_embeddings.bias)
    wu = P.bufs["uc_b"][1]
    prep("obj0", "O", [("uc_b", 0, wu, None), ("box_e", 0, 64, None), ("box_t_emb", 0, 64, "tidx")])
    obj, pred = "obj0", "pred0"
    nl = len(m.box_graph_cov.gconvs)
    for li, g in enumerate(m.box_graph_cov.gconvs):
        Do, Dp, H = g.input_dim_obj, g.input_dim_pred, g.hidden_dim
        w, b = _fold_bn(g.net1[0], g.net1[1])
        gemm("g_t1", "T", [(obj, 0, Do, "s"), (pred, 0, Dp, None), (obj, 0, Do, "o")], w, b, act="relu")
        w, b = _fold_bn(g.net1[3], g.net1[4])
        gemm(f"g_t2_{li % 2}", "T", [full("g_t1")], w, b, act="relu")
        t2 = f"g_t2_{li % 2}"
        P.buf("g_pool", "O", H)
        P.ops.append(("pool", "g_pool", t2, 0, H + Dp, H))
        P.tags.append("gcn")
        w, b = _fold_bn(g.net2[0], g.net2[1])
        gemm("g_h", "O", [full("g_pool")], w, b, act="relu")
        gemm(f"g_proj{g.output_dim}", "O", [full(obj)], g.linear_projection.weight, g.linear_projection.bias)
        w, b = _fold_bn(g.net2[3], g.net2[4])
        nobj = f"g_obj{li}"
        gemm(nobj, "O", [full("g_h")], w, b, act="relu", res=(f"g_proj{g.output_dim}", 0))
        if li != nl - 1:
            npred = f"g_pred{li % 2}"
            gemm(npred, "T", [full(pred)], g.linear_projection_pred.weight, g.linear_projection_pred.bias,
                 res=(t2, H))
            pred = npred
        obj = nobj
    ctx = P.context = obj

    # ---- torso
    def resblock(b, segs, out):
        cin = sum(s[2] for s in segs)
        gn = b.in_layers[0]
        prep(f"r_n{cin}", "O", segs, gn.num_groups, gn.eps, gn.weight, gn.bias, silu=True)
        conv = b.in_layers[2]
        gemm("r_h", "O", [full(f"r_n{cin}")], centre(conv), conv.bias, vec=("embproj", emb_off[id(b)], "tidx"))
        gn = b.out_layers[0]
        prep("r_n2", "O", [full("r_h")], gn.num_groups, gn.eps, gn.weight, gn.bias, silu=True)
        conv = b.out_layers[3]
        if isinstance(b.skip_connection, nn.Identity):
            assert len(segs) == 1
            return gemm(out, "O", [full("r_n2")], centre(conv), conv.bias, res=(segs[0][0], 0))
        sk = b.skip_connection              # 1x1 conv on the raw input: one product over [n2 | x] with [W_out | W_skip]
        assert len(segs) <= 2
        return gemm(out, "O", [full("r_n2")] + list(segs), torch.cat([centre(conv), sk.weight[:, :, 0]], 1),
                    conv.bias + sk.bias)

    def transformer(s, xin, out):
        gn = s.norm
        prep("s_n", "O", [full(xin)], gn.num_groups, gn.eps, gn.weight, gn.bias)
        z = gemm(uid("s_z"), "O", [full("s_n")], s.proj_in.weight[:, :, 0], s.proj_in.bias)
        for blk in s.transformer_blocks:
            ln = blk.norm1
            prep("s_l", "O", [full(z)], 1, ln.eps, ln.weight, ln.bias)
            for att, src in ((blk.attn1, "s_l"), (blk.attn2, ctx)):
                if FOLD_ATTENTION_VALUE:
                    z = gemm(uid("s_z"), "O", [full(src)], att.to_out[0].weight @ att.to_v.weight, att.to_out[0].bias,
                             res=(z, 0))
                else:
                    gemm("s_v", "O", [full(src)], att.to_v.weight, None)
                    z = gemm(uid("s_z"), "O", [full("s_v")], att.to_out[0].weight, att.to_out[0].bias, res=(z, 0))
            ln = blk.norm3
            prep("s_l", "O", [full(z)], 1, ln.eps, ln.weight, ln.bias)
            gemm("s_g", "O", [full("s_l")], blk.ff.net[0].proj.weight, blk.ff.net[0].proj.bias, act="geglu")
            z = gemm(uid("s_z"), "O", [full("s_g")], blk.ff.net[2].weight, blk.ff.net[2].bias, res=(z, 0))
        return gemm(out, "O", [full(z)], s.proj_out.weight[:, :, 0], s.proj_out.bias, res=(xin, 0))

    def block(seq, segs, tag):
        h = None
        for j, layer in enumerate(seq):
            out = f"{tag}.{j}"
            cur = segs if h is None else [full(h)]
            first = len(P.ops)
            P.section = "res" if isinstance(layer, ResBlock) else "attn" if isinstance(layer, SpatialTransformer1D) else "io"
            if isinstance(layer, ResBlock):
                h = resblock(layer, cur, out)
            elif isinstance(layer, SpatialTransformer1D):
                h = transformer(layer, h, out)
            elif isinstance(layer, Downsample):
                h = gemm(out, "O", cur, centre(layer.op), layer.op.bias)
            elif isinstance(layer, Upsample):
                h = gemm(out, "O", cur, centre(layer.conv), layer.conv.bias)
            elif isinstance(layer, nn.Conv1d):
                h = gemm(out, "O", cur, centre(layer), layer.bias)
            else:
                raise NotImplementedError(type(layer).__name__)
            P.modules[out] = (first, len(P.ops) - 1, tuple(cur), h)
        return h

    hs, h = [], None
    for i, seq in enumerate(m.input_blocks):
        h = block(seq, [full("x")] if h is None else [full(h)], f"input_blocks.{i}")
        hs.append(h)
    h = block(m.middle_block, [full(h)], "middle_block")
    for i, seq in enumerate(m.output_blocks):
        h = block(seq, [full(h), full(hs.pop())], f"output_blocks.{i}")
    gn = m.out[0]
    P.section = "io"
    prep("o_n", "O", [full(h)], gn.num_groups, gn.eps, gn.weight, gn.bias, silu=True)
    gemm("y", "O", [full("o_n")], centre(m.out[2]), m.out[2].bias)
    P.w["freqs"] = timestep_freqs(C).to(device=m.out[2].weight.device, dtype=m.out[2].weight.dtype)
    P.w["pred_embeddings"] = m.pred_embeddings.weight.detach()
    return P


def run_program_torch(P: Program, box_t, times, tidx, uc_b, triples):
    """The program on its packed operands with torch ops, in the operands' dtype (float64 for the algebra test).  box_t
    [O, 20], times [U] distinct time values, tidx [O] row -> time value, uc_b [O, 640], triples [T, 3]."""
    s, p, o = triples[:, 0].long(), triples[:, 1].long(), triples[:, 2].long()
    O = box_t.shape[0]
    row_ptr, slots = edge_csr(s, o, O)
    idx = {"s": s, "o": o, "tidx": tidx.long()}
    B = {"x": box_t, "t": times.reshape(-1, 1), "uc_b": uc_b, "pred0": P.w["pred_embeddings"][p]}

    def gather(segs):
        return torch.cat([(B[n] if ix is None else B[n][idx[ix]])[:, c0:c0 + w] for n, c0, w, ix in segs], dim=1)

    for op in P.ops:
        kind, out = op[0], op[1]
        if kind == "temb":
            a = B[op[2]].float() * P.w["freqs"].float()[None]       # float32 whatever the module's dtype, as nn.py
            B[out] = torch.cat([torch.cos(a), torch.sin(a)], dim=-1).to(box_t.dtype)
        elif kind == "prep":
            _, _, segs, G, eps, gamma, beta, silu = op
            x = gather(segs)
            if G:
                xg = x.reshape(x.shape[0], G, -1)
                x = ((xg - xg.mean(-1, keepdim=True)) / torch.sqrt(xg.var(-1, unbiased=False, keepdim=True) + eps)).reshape(x.shape)
                if gamma is not None:
                    x = x * P.w[gamma] + P.w[beta]
            B[out] = x * torch.sigmoid(x) if silu else x
        elif kind == "gemm":
            _, _, segs, w, b, act, vec, res = op
            y = gather(segs) @ P.w[w].t()
            if b is not None:
                y = y + P.w[b]
            if act == "relu":
                y = torch.relu(y)
            elif act == "geglu":
                a, g = y.chunk(2, dim=-1)
                y = a * torch.nn.functional.gelu(g)
            n = y.shape[1]
            if vec is not None:
                y = y + B[vec[0]][idx[vec[2]]][:, vec[1]:vec[1] + n]
            if res is not None:
                y = y + B[res[0]][:, res[1]:res[1] + n]
            B[out] = y
        elif kind == "pool":
            _, _, src, sc, oc, H = op
            t = B[src]
            rows = []
            for i in range(O):                  # the kernel's order: subject slots, then object slots, ascending
                v = torch.zeros(H, dtype=t.dtype, device=t.device)
                sl = slots[row_ptr[i]:row_ptr[i + 1]].tolist()
                for q in sl:
                    v = v + t[q >> 1, (oc if q & 1 else sc):(oc if q & 1 else sc) + H]
                rows.append(v / max(len(sl), 1))
            B[out] = torch.stack(rows)
    return B["y"]


class _Plan:
    """One (objects, triples, distinct times) problem on the device: named buffers, int32 index arrays, the CSR of the
    pooling, the split-K workspace and the launch list of the program."""

    def __init__(self, model, uc_b, triples, num_times, time_rows):
        from lidarcrafter_amd import ops as K
        from lidarcrafter_amd import ops_skinny as S

        K._req(uc_b, "uc_b")
        P = model.packed()
        dev = uc_b.device
        tr = triples.detach().to("cpu", torch.int64)
        O, T, U = uc_b.shape[0], tr.shape[0], int(num_times)
        if T < 1 or O < 1:
            raise ValueError("the layout generator needs at least one object and one triple")
        if tr.dim() != 2 or tr.shape[1] != 3:
            raise ValueError("triples must be [T, 3] (subject, predicate, object)")
        if int(tr[:, 1].min()) < 0 or int(tr[:, 1].max()) >= P.w["pred_embeddings"].shape[0]:
            raise ValueError("a predicate id lies outside UNet1DModel.pred_embeddings")
        row_ptr, slots = edge_csr(tr[:, 0], tr[:, 2], O)            # validates subject / object ids against O
        if tuple(uc_b.shape) != (O, P.bufs["uc_b"][1]):
            raise ValueError(f"uc_b must be [O, {P.bufs['uc_b'][1]}], got {tuple(uc_b.shape)}")
        if time_rows is None:
            if U != 1:
                raise ValueError("several time values need the row -> time value map")
            time_rows = torch.zeros(O, dtype=torch.int64)
        time_rows = time_rows.detach().to("cpu", torch.int64)
        if time_rows.numel() != O or int(time_rows.min()) < 0 or int(time_rows.max()) >= U:
            raise ValueError("time_rows must map every object row to one of the time values")
        self.O, self.T, self.U, self.P = O, T, U, P
        i32 = lambda t: t.to(torch.int32).to(dev)
        self.idx = {"s": i32(tr[:, 0]), "o": i32(tr[:, 2]), "tidx": i32(time_rows)}
        self.row_ptr, self.slots = row_ptr.to(dev), slots.to(dev)
        rows = {"O": O, "T": T, "U": U, "U1": U}
        self.B = {n: torch.zeros((rows[k], w), device=dev, dtype=torch.float32) for n, (k, w) in P.bufs.items()}
        self.B["uc_b"].copy_(uc_b)
        self.B["pred0"].copy_(P.w["pred_embeddings"][tr[:, 1].to(dev)])
        self.x, self.t, self.y = self.B["x"], self.B["t"].view(-1), self.B["y"]
        need = 1
        for op in P.ops:
            if op[0] == "gemm":
                M = self.B[op[1]].shape[0]
                N, Kd = P.w[op[3]].shape
                need = max(need, S.skinny_parts(M, N, Kd) * M * N)
        self.parts = torch.empty(need, device=dev, dtype=torch.float32)
        self.dev = dev

    def run(self):
        from lidarcrafter_amd import ops_skinny as S

        P, B, ix = self.P, self.B, self.idx

        def segs(ss):
            return [(B[n], c0, w, None if i is None else ix[i]) for n, c0, w, i in ss]

        for op in P.ops:
            kind, out = op[0], B[op[1]]
            if kind == "gemm":
                _, _, ss, w, b, act, vec, res = op
                S.skinny_linear(segs(ss), out.shape[0], P.w[w], None if b is None else P.w[b], act,
                                None if vec is None else (B[vec[0]], vec[1], ix[vec[2]]),
                                None if res is None else (B[res[0]], res[1]), out=out, parts=self.parts)
            elif kind == "prep":
                _, _, ss, G, eps, gamma, beta, silu = op
                S.rowprep(segs(ss), out.shape[0], G, eps, None if gamma is None else P.w[gamma],
                          None if beta is None else P.w[beta], silu, out=out)
            elif kind == "pool":
                _, _, src, sc, oc, H = op
                S.graph_pool(B[src], sc, oc, H, self.row_ptr, self.slots, out=out)
            else:
                S.time_embed(self.t, P.w["freqs"], out=out)
