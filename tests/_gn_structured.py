"""Channel-structured activations for the GroupNorm statistics-entry routes (tests/test_gn_structured.py on the GPU,
tests/test_gn_structured_host.py on the CPU): one place, so the two files cannot drift apart.  No GPU code here.

Every other kernel test feeds GroupNorm with data whose channels all sit at one level.  A trained network does not: its
channels carry bias levels, and the units of one channel octet (pairs / quads of GroupNorm32 at 64 / 128 channels) sit at
different levels.  The producers' statistics entries (pivot, n, sum(v - p), sum((v - p)^2)) sum in float32, so what an
entry is worth depends on how far its values are from its pivot:

    R = |group mean - first value of the group's channel octet| / group std

The level table puts the units of an octet 2 apart and the channels inside a unit `step` apart; the spatial spread is
`a * step`.  R grows as step shrinks (cpg = 2: R ~ 49 / 385 / 3070 at step 2^-2 / 2^-5 / 2^-8).

The bound of the GPU test, per (sample, group): rel-L2 against float64 <= max(tol, 4 x the largest per-group error of the
float32 oracle on the same stored tensor).  tol = 2e-6 (the entry routes' existing tolerance), 1e-4 for the common-level
case (test_groupnorm_large_mean's).  The factor 4 is the margin over the reference's own float32 error: it covers the
route's float32 roundings of the mean, of rstd * gamma * (1 + s) and of the apply."""
import ast
import os

import torch

from lidarcrafter_amd.testing import seeded_randn

EPS = 1e-6
TOL_ENTRY = 2e-6           # test_hip_parity::test_conv_fused_groupnorm_from_pair_stats and the other entry-route tests
TOL_COMMON = 1e-4          # test_hip_parity::test_groupnorm_large_mean
MARGIN = 4.0
R_MIN = 32.0               # every pair / quad route reaches this in at least one case
F32_ULP = 2.0 ** -23

# (name, step, a): the control; three steps, each with a small spatial spread and with exactly constant planes
DATA = [("control", 1.0, 1.0)] + [(f"step{-e}-{'a4' if a else 'a0'}", 2.0 ** e, a)
                                   for e in (-2, -5, -8) for a in (2.0 ** -4, 0.0)]
SPECIAL = ["common", "constant"]     # 0.01 randn + 30 through the bias; one group exactly constant
DATA_NAMES = [d[0] for d in DATA] + SPECIAL


def levels(C, G, step):
    """lvl[c] = 2 ((c % 8) // cpg - (8 / cpg - 1) / 2) + step (c % cpg) + 0.5 ((c // 8) % 3), cpg = C / G: the units of
    an octet at -3, -1, 1, 3 (cpg = 2) or -1, 1 (cpg = 4), one level for whole-octet groups.  Where a group is no divisor
    of an octet (6 per group at 192 channels: groups straddle octets) four consecutive GROUPS take the four levels, so a
    group still sits at one level while its entries' octets begin in another group."""
    cpg = C // G
    c = torch.arange(C)
    nu = 1 if cpg >= 8 else (8 // cpg if 8 % cpg == 0 else 4)
    unit = (torch.div(c, cpg, rounding_mode="floor") % nu).double()
    blk = c // 8 if cpg >= 8 else c // (cpg * nu)               # (= c // 8 wherever a group divides an octet)
    return (2.0 * (unit - (nu - 1.0) / 2.0) + step * (c % cpg).double() + 0.5 * (blk % 3).double()).float()


def data_spec(name):
    for n, step, a in DATA:
        if n == name:
            return step, a
    raise KeyError(name)


def conv_params(Co, Ci, ks, G, data, seed=0, fan=None, const_level=None):
    """(weight [Co, Ci, ks, ks], bias [Co], const_group or None) of a conv whose output on unit-variance input sits at
    lvl[c] with spatial spread a * step.  `fan`: the number of unit-variance terms behind one output (default Ci ks^2)."""
    fan = fan or Ci * ks * ks
    w = seeded_randn(Co, Ci, ks, ks, seed=7000 + seed) / fan ** 0.5
    const_group = None
    if data == "common":
        return w * 0.01, torch.full((Co,), 30.0), None
    if data == "constant":
        step, a = 2.0 ** -5, 2.0 ** -4
        cpg = Co // G
        const_group = G // 2 + 1 if G > 2 else G - 1          # a unit away from its octet's first channel where there is one
        lv = levels(Co, G, step)
        w = w * (a * step)
        c0 = const_group * cpg
        w[c0:c0 + cpg] = 0.0
        # (not a dyadic level: v - pivot rounds in float32.  const_level = 0: a producer whose border rows carry 7/8 of
        #  a constant keeps a group exactly constant at level 0 only)
        lv[c0:c0 + cpg] = lv[c0] + 0.1 if const_level is None else const_level
        return w, lv, const_group
    step, a = data_spec(data)
    return w * (a * step), levels(Co, G, step), None


def tensor_data(B, C, H, W, G, data, seed=0, const_level=None):
    """The same structure as a tensor (producers that are no convolution: the down-sampler)."""
    r = seeded_randn(B, C, H, W, seed=7100 + seed)
    if data == "common":
        return r * 0.01 + 30.0, None
    if data == "constant":
        step, a = 2.0 ** -5, 2.0 ** -4
        cpg = C // G
        g = G // 2 + 1 if G > 2 else G - 1
        lv = levels(C, G, step)
        t = lv[None, :, None, None] + a * step * r
        t[:, g * cpg:(g + 1) * cpg] = lv[g * cpg] + 0.1 if const_level is None else const_level
        return t, g
    step, a = data_spec(data)
    return levels(C, G, step)[None, :, None, None] + a * step * r, None


def gn_params(B, C, seed=0):
    return dict(ga=1 + 0.1 * seeded_randn(C, seed=7200 + seed), be=0.1 * seeded_randn(C, seed=7201 + seed),
                ss=0.3 * seeded_randn(B, 2 * C, seed=7202 + seed))


def gn_eval(y, G, p, silu, dtype):
    """silu?((1 + scale) GroupNorm(y; gamma, beta) + shift) through oracle.denoiser, evaluated in `dtype` on the CPU."""
    from oracle import denoiser as D

    C = y.shape[1]
    t = lambda v: None if v is None else v.detach().cpu().to(dtype)
    h = D.group_norm(t(y), G, t(p.get("ga")), t(p.get("be")), EPS)
    ss = t(p.get("ss"))
    if ss is not None:
        h = h * (1 + ss[:, :C, None, None]) + ss[:, C:, None, None]
    return D.silu(h) if silu else h


def group_view(y, G):
    B, C = y.shape[:2]
    return y.detach().cpu().double().reshape(B, G, -1)


def group_err(got, ref64, G):
    """rel-L2 per (sample, group) -> [B, G]."""
    g, r = group_view(got, G), group_view(ref64, G)
    return (g - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-30)


def group_stats64(y, G):
    """(mean, var, rstd) per (sample, group) of the stored tensor in float64."""
    v = group_view(y, G)
    mean, var = v.mean(-1), v.var(-1, unbiased=False)
    return mean, var, (var + EPS).rsqrt()


def measure_R(y, G):
    """[B, G]: |group mean - first value of the group's channel octet| / group std on the stored tensor (the farther of
    the two octets where a group straddles them); 0 for a constant group (no spread to lose)."""
    B, C = y.shape[:2]
    cpg = C // G
    mean, var, _ = group_stats64(y, G)
    first = y.detach().cpu().double()[:, :, 0, 0]                       # [B, C]
    lo = (torch.arange(G) * cpg) // 8 * 8
    hi = (torch.arange(G) * cpg + cpg - 1) // 8 * 8
    d = torch.maximum((mean - first[:, lo]).abs(), (mean - first[:, hi]).abs())
    return torch.where(var > 0, d / var.sqrt().clamp_min(1e-300), torch.zeros_like(d))


def bound_for(y, G, p, silu, tol, skip_group=None):
    """-> (bound, e32 [B, G], ref64): max(tol, 4 x the worst per-group error of the float32 oracle on `y`)."""
    ref64 = gn_eval(y, G, p, silu, torch.float64)
    e32 = group_err(gn_eval(y, G, p, silu, torch.float32), ref64, G)
    if skip_group is not None:
        e32 = e32.clone()
        e32[:, skip_group] = 0.0
    worst = float(e32.max())
    assert worst == worst and worst < float("inf"), "the float32 oracle is not finite"
    return max(tol, MARGIN * worst), e32, ref64


def constant_bound(level, ga, be, ss, c, b, C, ulp=F32_ULP):
    """Condition 3: 1000 ulp |level| |gamma (1 + s)| -- one rounding of the mean times 1 / sqrt(eps), with a factor 2 --
    plus the apply's own roundings of beta (1 + s) + shift (4 ulp of the larger term; all there is at level 0)."""
    sc = 1 + float(ss[b, c])
    terms = max(abs(float(be[c]) * sc), abs(float(ss[b, C + c])), abs(float(be[c]) * sc + float(ss[b, C + c])))
    return 1000.0 * ulp * abs(level) * abs(float(ga[c]) * sc) + 4.0 * ulp * terms


def constant_closed_form(be, ss, c, b, C, silu):
    """GroupNorm of an exactly constant group: (v - mean) = 0, so the output is silu?(beta (1 + s) + shift)."""
    from oracle import denoiser as D

    v = be.double()[c] * (1 + ss.double()[b, c]) + ss.double()[b, C + c]
    return D.silu(v) if silu else v


# ------------------------------------------------------------------------------------------------ the routes
class Route:
    """One producer launch.  entry: the function of lidarcrafter_amd/ops.py whose `_attach_stats` call site the launch
    goes through; unit: channels per entry; shape: (B, Ci, Co, H, W) of the producer (H, W = its INPUT plane); cfg: its
    tile configuration; G: groups of the consumer GroupNorm; ragged: a shape for the common-level case where the producer
    takes one (H off the tile rows, W off the tile width)."""

    def __init__(self, name, entry, unit, shape, G, cfg=0, ks=3, ragged=None, sub_octet=False):
        self.name, self.entry, self.unit, self.shape, self.G, self.cfg, self.ks = name, entry, unit, shape, G, cfg, ks
        self.ragged, self.sub_octet = ragged, sub_octet

    def out_shape(self, shape=None):
        B, Ci, Co, H, W = shape or self.shape
        if self.entry in ("conv_down2", "resample2x"):
            return B, Co, H // 2, W // 2
        if self.entry == "conv_up2":
            return B, Co, 2 * H, 2 * W
        return B, Co, H, W

    def __repr__(self):
        return self.name


RAG = (2, 32, 64, 5, 50)
ROUTES = [
    # 3x3 deferred epilogue (fp32-input kernels): octet and pair entries, every tile shape of the pair-entry test
    Route("def3x3-oct-c23", "conv2d_ring", 8, (2, 32, 64, 8, 128), 8, cfg=23),
    Route("def3x3-oct-c25", "conv2d_ring", 8, (3, 32, 64, 6, 96), 8, cfg=25),
    Route("def3x3-oct-c13", "conv2d_ring", 8, (2, 32, 64, 8, 128), 8, cfg=13, ragged=RAG),
    Route("def3x3-pair-c23", "conv2d_ring", 2, (2, 32, 64, 8, 128), 32, cfg=23, sub_octet=True),
    Route("def3x3-pair-c25", "conv2d_ring", 2, (3, 32, 64, 6, 96), 32, cfg=25, sub_octet=True),
    Route("def3x3-pair-c13", "conv2d_ring", 2, (2, 32, 64, 8, 128), 32, cfg=13, ragged=RAG, sub_octet=True),
    Route("def3x3-pair-g16", "conv2d_ring", 2, (2, 32, 64, 8, 128), 16, cfg=23, sub_octet=True),     # 4 per group from pairs
    Route("def3x3-pair-c192", "conv2d_ring", 2, (2, 32, 192, 8, 128), 32, cfg=23, sub_octet=True),   # 6 per group: straddles octets
    # the ping-pong kernel's epilogue (tile cfg 33, one strip group)
    Route("pp-oct", "conv2d_ring", 8, (2, 64, 64, 8, 128), 8, cfg=133),
    Route("pp-pair", "conv2d_ring", 2, (2, 64, 64, 8, 128), 32, cfg=133, sub_octet=True),
    # pre-split 3x3 kernel: octets and quads; split-K reduction: octets
    Route("ps-oct-c23", "_conv2d_ring_presplit", 8, (2, 64, 64, 8, 128), 8, cfg=23),
    Route("ps-oct-c13", "_conv2d_ring_presplit", 8, (2, 48, 64, 8, 128), 8, cfg=13, ragged=(2, 48, 64, 5, 50)),
    Route("ps-quad-c23", "_conv2d_ring_presplit", 4, (2, 64, 64, 8, 128), 16, cfg=23, sub_octet=True),
    Route("ps-quad-c13", "_conv2d_ring_presplit", 4, (2, 48, 64, 8, 128), 16, cfg=13, ragged=(2, 48, 64, 5, 50),
          sub_octet=True),
    Route("splitk-oct", "_conv2d_ring_presplit", 8, (2, 128, 64, 4, 64), 8, cfg=0, ragged=(1, 64, 64, 5, 50)),
    # non-pipelined 1x1
    Route("conv1x1-c0", "conv2d_ring", 8, (1, 64, 72, 6, 50), 9, cfg=0, ks=1, ragged=(1, 64, 72, 6, 50)),
    Route("conv1x1-c3", "conv2d_ring", 8, (1, 64, 72, 6, 50), 9, cfg=3, ks=1, ragged=(1, 64, 72, 6, 50)),
    Route("conv1x1-c5", "conv2d_ring", 8, (1, 64, 72, 6, 50), 9, cfg=5, ks=1, ragged=(1, 64, 72, 6, 50)),
    Route("conv1x1-c1", "conv2d_ring", 8, (1, 64, 72, 6, 50), 9, cfg=1, ks=1, ragged=(1, 64, 72, 6, 50)),
    # stride-2 fold-down: octets, quads.  16 input rows: the bias reaches the first / last output row with the factor
    # 7/8, which alone spreads a group by |level| / 8 on those rows; with 8 output rows R still passes R_MIN
    Route("down-oct", "conv_down2", 8, (2, 32, 64, 16, 256), 8),
    Route("down-quad", "conv_down2", 4, (2, 32, 64, 16, 256), 16, sub_octet=True),
    # up-fold and the down-sampler: one entry per channel (every entry has a pivot of its own)
    Route("up-chan-g32", "conv_up2", 1, (2, 32, 64, 2, 128), 32),
    Route("up-chan-g8", "conv_up2", 1, (2, 32, 64, 2, 128), 8),
    Route("resample-chan-g32", "resample2x", 1, (2, 64, 64, 8, 256), 32),
    Route("resample-chan-g8", "resample2x", 1, (2, 64, 64, 8, 256), 8),
]
ROUTE_BY_NAME = {r.name: r for r in ROUTES}


def attach_sites():
    """[(enclosing function, line)] of every `_attach_stats(...)` call in lidarcrafter_amd/ops.py."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidarcrafter_amd", "ops.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    out = []
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)) and fn.name != "_attach_stats":
            for node in ast.walk(fn):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_attach_stats":
                    out.append((fn.name, node.lineno))
    return sorted(set(out), key=lambda s: s[1])


def make_case(route, data):
    """Seeded float32 operands of one (route, data) case: dict(shape, x, w, b, const) -- `x` is the producer's input (for
    the down-sampler: the structured tensor itself, no weights).  The common-level case runs at the route's ragged shape
    where the producer takes one."""
    shape = route.ragged if (data == "common" and route.ragged) else route.shape
    B, Ci, Co, H, W = shape
    seed = sum(map(ord, route.name)) % 97
    const_level = 0.0 if route.entry in ("conv_down2", "resample2x") else None
    if route.entry == "resample2x":
        x, const = tensor_data(B, Ci, H, W, route.G, data, seed=seed, const_level=const_level)
        return dict(shape=shape, x=x, w=None, b=None, const=const)
    w, b, const = conv_params(Co, Ci, route.ks, route.G, data, seed=seed, const_level=const_level)
    return dict(shape=shape, x=seeded_randn(B, Ci, H, W, seed=7300 + seed), w=w, b=b, const=const)


def cpu_produce(route, case, dtype=torch.float64):
    """The producer's operation in plain torch through oracle.denoiser (the host file measures R and the float32 oracle's
    error on this; the GPU file uses the tensor the kernel stored)."""
    from oracle import denoiser as D

    x = case["x"].to(dtype)
    if route.entry == "resample2x":
        return D.resample_down2(x)
    w, b = case["w"].to(dtype), case["b"].to(dtype)
    if route.entry == "conv_down2":
        return D.resample_down2(D.conv_ring(x, w, b))
    if route.entry == "conv_up2":
        return D.conv_ring(D.resample_up2(x), w, b)
    return D.conv_ring(x, w, b)
