"""Case tables, float64 references, float32 oracles and bounds of the MeanFlow tangent-kernel edge tests
(tests/test_flow_jvp_edges.py on the GPU, tests/test_flow_jvp_edges_host.py on the CPU): one place, so the two files cannot
drift apart.  No GPU code here.

The kernels: csrc/flow_jvp.hip (GroupNorm JVP statistics and apply, q / k RMSNorm JVP and backward with its dg reduce,
flash attention with its tangent).  Which branch a row takes is asked of the library (lc_groupnorm_jvp_route,
lc_qk_norm_cm_route, lc_attention_jvp_route: the functions the launchers and kernels switch on, csrc/flow_jvp_route.h),
never restated here.

Every reference is written out in closed form and evaluated twice: in float64 (the reference) and in float32 (the oracle,
whose own error against float64 sets the second term of every bound).  The host file holds the closed forms against
torch.func.jvp / autograd of the plain formulas of tests/test_meanflow_training.py.

q / k RMSNorm.  Per (sample, head, token): e = |got - ref64|_2 / |ref64|_2 for y, dy (tangent) and gx (backward); a
token whose reference is all zero must come back exactly zero.  Bound: max(TOL_QK = 1e-6, 4 x the float32 oracle's worst
token on the same row).  Tokens of norm 0, 1e-14 (clamped: y = sqrt(d) g v / 1e-12, the tangent is the linear map
sqrt(d) g / 1e-12, about 1e12 |dx|) and 3e-12 (just above the clamp: the projection applies, at a factor of 3e11) are mixed
among ordinary ones.  d = 1: I - v v^T / |v|^2 is the 1 x 1 zero matrix, so the tangent and the backward of an unclamped
token are zero in exact arithmetic and whatever w - v (v w / v^2) rounds to in any finite precision; float64 itself leaves
1e-16 |s w| there.  A quotient by that reference means nothing, so on those tokens (and only those) the reference is the
exact 0 and the error is |got| / (|s| |w|), the size of the two terms that cancel, under the same bound.
dg against the float64 sum of its terms gy . y / g, scaled by the sum of their absolute values, same two-term bound.

GroupNorm JVP.  The rule of tests/_gn_structured.py per (sample, group), for y and for dy: rel-L2 <= max(tol, 4 x the
float32 oracle's worst group), tol = TOL_ENTRY, TOL_COMMON for the common-level data.  An exactly constant group has
var = 0, rstd = 1000: y is held to the closed form silu?(beta (1 + s) + shift) under GS.constant_bound's rule
(gn_const_bounds); with a constant tangent dy is the closed form silu'(a) (beta ds + dsh) under the analogous bound, with a
random tangent the group stays in the rel-L2 rule (dn = 1000 (dx - mean dx) is well conditioned).  The float32 oracle forms
mean(n dx) as mean(n (dx - mean dx)): the same number (mean(n) = 0), and the form that keeps float32 conditioned at a large
common level -- the uncentred one is off by 80 % on the step-2^-8 rows and would make their bound vacuous.

Attention JVP.  Per element of o and do: e = |got - ref64| / S with S the float64 sum of the absolute terms of the element's
contraction as the kernel forms it: o = sum p v: S = sum p |v|;  do = sum p (dS v + dv) - mu o: S = sum p (|dS| |v| + |dv|)
+ |mu| sum p |v|.  Bound: max(TOL_ATTN = 2e-6, 4 x the float32 oracle's worst element on the same row).  The base-2
log-sum-exp per row under 1e-5 max(1, |ref|).

A designed defect (one key dropped, the last channel of a lane dropped, the mu correction skipped, the projection dropped
next to the clamp, the primal's maxima handed to the tangent) moves some element by at least SIGNAL_OVER_BOUND = 16
bounds on every row it applies to, and the float32 oracle stays under ORACLE_CAP = 8 floors on every q / k and attention
row: the host file asserts both."""
import collections
import functools
import math

import torch

from lidarcrafter_amd.testing import seeded_randn
from tests import _gn_structured as GS
from tests._profile_cases import TOL_ATTN_BWD, TOL_CONV  # noqa: F401  (no new tolerance)
from tests._train_edges import (GUARD, MARGIN, SIGNAL_OVER_BOUND, addr_mod16, batch_stride, guarded, layout, outside,  # noqa: F401
                                place)

TOL_QK = 1e-6            # test_meanflow_training::test_qk_norm_jvp_and_backward_against_float64
TOL_ATTN = 2e-6          # test_meanflow_training::test_attention_jvp_against_float64
LSE_TOL = 1e-5           # the same test: 1e-5 * max(1, |lse|)
ORACLE_CAP = 8.0         # the float32 oracle's worst figure is at most 8 floors on every q / k and attention row
EPS = 1e-6
QK_CLAMP = 1e-12
LOG2E = 1.4426950408889634


def _route(fn, n, *args):
    import ctypes

    from lidarcrafter_amd import _lib

    out = (ctypes.c_int32 * n)()
    rc = getattr(_lib.lib(), fn)(*args, out)
    return rc, list(out)


# ------------------------------------------------------------------------------------------------ q / k RMSNorm
QCase = collections.namedtuple("QCase", "name edge B heads d L xl tiny")


def Q_(name, edge, B, heads, d, L, xl="contig", tiny=True):
    return QCase(name, edge, B, heads, d, L, xl, tiny)


QK_CASES = [
    Q_("d1", "d = 1: DMAX = 16 with 15 padded channels; the projection is the zero matrix", 2, 3, 1, 257),
    Q_("d5", "d = 5: DMAX = 16, 11 padded channels", 2, 3, 5, 257),
    Q_("d16", "d = 16: DMAX = 16 exactly", 2, 3, 16, 257),
    Q_("d17", "d = 17: the first width on DMAX = 32", 2, 3, 17, 257),
    Q_("d32", "d = 32: DMAX = 32 exactly", 2, 3, 32, 257),
    Q_("d33", "d = 33: the first width on DMAX = 64", 2, 3, 33, 257),
    Q_("d48", "d = 48: DMAX = 64, 16 padded channels", 2, 3, 48, 257),
    Q_("d64", "d = 64: DMAX = 64 exactly", 2, 3, 64, 257),
    Q_("L1", "L = 1: one live lane in the only block (an ordinary token)", 2, 3, 17, 1, tiny=False),
    Q_("L255", "L = 255: the last lane of the block idle", 2, 3, 17, 255),
    Q_("L256", "L = 256: exactly one block", 2, 3, 5, 256),
    Q_("L513", "L = 513: three blocks, the last with one token", 2, 3, 64, 513),
    Q_("qkv-slice", "x the middle third of a qkv tensor (batch stride 3 C L, offset C L)", 2, 3, 33, 257, xl="qkv"),
    Q_("x-cs", "x with a channel stride of L + 3", 2, 3, 5, 255, xl="cs"),
    Q_("x-cs-d64", "x with a channel stride of L + 3 on DMAX = 64", 1, 2, 64, 130, xl="cs"),
    Q_("dg-260-partials", "L = 257, B heads = 130: 260 partials of dg, a second trip of the reduce's strided loop", 2, 65, 5, 257),
    Q_("ordinary", "no tiny token: the clamp branch is not taken (the control)", 2, 3, 32, 130, tiny=False),
]


def qk_route(c):
    return _route("lc_qk_norm_cm_route", 4, c.B, c.heads, c.d, c.L)


def qk_tiny_tokens(L):
    """{token: kind} -- kind 0: exactly zero, 1: norm 1e-14 (clamped), 2: norm 3e-12 (the clamp's neighbour): the first and
    last token of every block and tokens 255 / 256, cycling through the kinds, ordinary tokens in between."""
    want = sorted({t for t in (0, 1, 2, 127, 254, 255, 256, 257, 258, 511, 512, L - 3, L - 2, L - 1) if 0 <= t < L})
    return {t: i % 3 for i, t in enumerate(want)}


def qk_operands(c):
    """-> dict x, dx, gy [B, C, L] float32 (CPU), g [1], kinds {token: kind}."""
    seed = 9500 + sum(map(ord, c.name))
    C = c.heads * c.d
    x = seeded_randn(c.B, C, c.L, seed=seed)
    kinds = qk_tiny_tokens(c.L) if c.tiny else {}
    xh = x.reshape(c.B, c.heads, c.d, c.L).double()
    for t, kind in kinds.items():
        u = xh[..., t] / xh[..., t].norm(dim=2, keepdim=True)
        xh[..., t] = u * (0.0, 1e-14, 3e-12)[kind]
    x = xh.reshape(c.B, C, c.L).float()
    return dict(x=x, dx=seeded_randn(c.B, C, c.L, seed=seed + 1), gy=seeded_randn(c.B, C, c.L, seed=seed + 2),
                g=torch.tensor([-1.75]), kinds=kinds)


def qk_closed(x, w, g, heads, defect=None):
    """(y, J w, s, nrm) of y = sqrt(d) g x / max(|x|, 1e-12) per (sample, head, token) in the dtype of x; J w =
    s (w - x (x . w) / |x|^2) above the clamp, s w below.  defect "no-proj": the clamp's linear map everywhere."""
    B, C, L = x.shape
    d = C // heads
    xh, wh = x.reshape(B, heads, d, L), w.reshape(B, heads, d, L)
    ss = (xh * xh).sum(2, keepdim=True)
    nrm = ss.sqrt()
    s = math.sqrt(d) * g.to(x.dtype) / nrm.clamp_min(QK_CLAMP)
    live = nrm > QK_CLAMP
    proj = torch.where(live, (xh * wh).sum(2, keepdim=True) / torch.where(live, ss, torch.ones_like(ss)), torch.zeros_like(ss))
    if defect == "no-proj":
        proj = torch.zeros_like(proj)
    return (xh * s).reshape(B, C, L), (s * (wh - xh * proj)).reshape(B, C, L), s, nrm


def qk_dg_terms(x, gy, g, heads):
    """The terms gy . y / g of dL/dg [B, heads, d, L] in the dtype of x."""
    B, C, L = x.shape
    d = C // heads
    xh = x.reshape(B, heads, d, L)
    nrm = (xh * xh).sum(2, keepdim=True).sqrt()
    return gy.reshape(B, heads, d, L) * xh * (math.sqrt(d) / nrm.clamp_min(QK_CLAMP))


def qk_token_err(got, ref64, heads, scale=None):
    """-> (e [B, heads, L], tokens whose reference is zero without a scale and that are not exactly zero).  e =
    |got - ref64|_2 / |ref64|_2; where `scale` [B, heads, L] is positive (d = 1 above the clamp) the quotient is by it."""
    B, C, L = ref64.shape
    d = C // heads
    g = got.detach().cpu().double().reshape(B, heads, d, L)
    r = ref64.reshape(B, heads, d, L)
    den = r.norm(dim=2)
    if scale is not None:
        den = torch.where(scale > 0, scale, den)
    num = (g - r).norm(dim=2)
    zero = den == 0
    e = torch.where(zero, torch.zeros_like(num), num / den.clamp_min(1e-300))
    return e, int((zero & (g.abs().amax(dim=2) != 0)).sum())


QRef = collections.namedtuple("QRef", "t y dy gx dg S_dg scale_dy scale_gx e32 bound bound_dg e32_dg")


def _qk_cancel_scale(c, s, nrm, w):
    """d = 1 above the clamp: |s| |w| per token (see the module docstring); None for every other width."""
    if c.d != 1:
        return None
    B, C, L = w.shape
    wn = w.reshape(B, c.heads, 1, L).abs()
    return torch.where(nrm > QK_CLAMP, s.abs() * wn, torch.zeros_like(wn)).reshape(B, c.heads, L)


@functools.lru_cache(maxsize=None)
def qk_ref(c):
    t = qk_operands(c)
    x, dx, gy, g = (t[k].double() for k in ("x", "dx", "gy", "g"))
    y, dy, s, nrm = qk_closed(x, dx, g, c.heads)
    _, gx, _, _ = qk_closed(x, gy, g, c.heads)
    sc_dy, sc_gx = _qk_cancel_scale(c, s, nrm, dx), _qk_cancel_scale(c, s, nrm, gy)
    if c.d == 1:                                                  # the exact zero, not float64's roundoff of it
        live = (nrm > QK_CLAMP).reshape(c.B, c.heads * c.d, c.L)
        dy, gx = torch.where(live, torch.zeros_like(dy), dy), torch.where(live, torch.zeros_like(gx), gx)
    terms = qk_dg_terms(x, gy, g, c.heads)
    dg, S_dg = float(terms.sum()), float(terms.abs().sum())
    # the float32 oracle: the same closed forms in float32
    y32, dy32, _, _ = qk_closed(t["x"], t["dx"], t["g"], c.heads)
    _, gx32, _, _ = qk_closed(t["x"], t["gy"], t["g"], c.heads)
    e32 = max(float(qk_token_err(y32, y, c.heads)[0].max()), float(qk_token_err(dy32, dy, c.heads, sc_dy)[0].max()),
              float(qk_token_err(gx32, gx, c.heads, sc_gx)[0].max()))
    e32_dg = abs(float(qk_dg_terms(t["x"], t["gy"], t["g"], c.heads).sum()) - dg) / S_dg
    assert e32 == e32 and e32 < float("inf") and e32_dg == e32_dg, "the float32 oracle is not finite"
    return QRef(t, y, dy, gx, dg, S_dg, sc_dy, sc_gx, e32, max(TOL_QK, MARGIN * e32), max(TOL_QK, MARGIN * e32_dg), e32_dg)


# ------------------------------------------------------------------------------------------------ GroupNorm JVP
NCase = collections.namedtuple("NCase", "name edge B C G H W affine ada act xl dxl data dxmode")


def N_(name, edge, B, C, G, H, W, affine=True, ada=True, act=True, xl="contig", dxl="contig", data=None, dxmode="rand"):
    return NCase(name, edge, B, C, G, H, W, affine, ada, act, xl, dxl, data, dxmode)


_BASE = (3, 8, 2, 6, 50)            # H W = 300, n = 1200: the vector branch; the layout rows differ from it by ONE operand
GN_CASES = [
    N_("base-vec", "the float4 statistics loop with float4 loads of dx: the shape the cause rows differ from", *_BASE),
    N_("n-mod4", "n % 4 != 0: the scalar loop (H W = 37, 3 channels per group); later groups and samples are off 16 bytes too", 3, 6, 2, 1, 37),
    N_("n-mod4-alone", "n % 4 != 0 ALONE: one sample, one group, so x and dx are on 16 bytes (n = 111)", 1, 3, 1, 1, 37),
    N_("dx-slice-hi-odd", "x contiguous, dx a channel slice 12 H W bytes in with H W % 4 != 0, n % 4 == 0: dvec == false", 3, 8, 2, 5, 37,
       dxl="slice_hi"),
    N_("x-slice-hi-odd", "the reverse: x off 16 bytes, dx contiguous: the scalar loop by the address of x", 3, 8, 2, 5, 37,
       xl="slice_hi"),
    N_("x-slice-lo", "x with a batch stride above C H W alone", *_BASE, xl="slice_lo"),
    N_("dx-slice-lo", "dx with a batch stride above C H W alone", *_BASE, dxl="slice_lo"),
    N_("x-bs1", "x_bs = C H W + 1: the branch differs by sample", *_BASE, xl="bs1"),
    N_("dx-bs1", "dx_bs = C H W + 1: dvec differs by sample", *_BASE, dxl="bs1"),
    N_("x-off1", "the scalar loop because of the address of x alone", *_BASE, xl="off1"),
    N_("dx-off1", "dvec == false because of the address of dx alone", *_BASE, dxl="off1"),
    N_("chunks-8193", "n = 8193: two chunks of 4096 and a last chunk of ONE element (scalar loop); H W > 4096: three slabs", 2, 2, 2, 3, 2731),
    N_("chunks-8196", "n = 8196: two chunks of 4096 and a last chunk of one float4; three slabs", 2, 2, 2, 3, 2732),
    N_("chunk-16384", "512 statistics blocks: the 16384-element chunk, a last chunk of 4 elements; five slabs; one channel per group",
       1, 256, 256, 4, 4097),
    N_("hw4096", "H W = 4096: exactly one slab, two channels per group", 1, 4, 2, 64, 64),
    N_("hw4097", "H W = 4097: two slabs of 2049, the second one short", 1, 4, 2, 17, 241),
    N_("cpb2", "two channels per apply block", 4, 1024, 512, 2, 3),
    N_("cpb4", "four channels per apply block", 4, 1024, 256, 2, 3),
    N_("cpb8", "eight channels per apply block", 4, 1024, 128, 2, 3),
    N_("cpg1", "one channel per group at a small plane", 3, 8, 8, 5, 37),
    # the affine / AdaGN / SiLU combinations of test_groupnorm_jvp_against_float64
    N_("ada-act", "scale / shift without gamma / beta, SiLU", 3, 12, 2, 5, 50, affine=False, ada=True, act=True),
    N_("affine-noact", "gamma / beta alone, no SiLU", 3, 12, 2, 5, 50, affine=True, ada=False, act=False),
    N_("plain-act", "neither, SiLU", 3, 12, 2, 5, 37, affine=False, ada=False, act=True),
    N_("both-noact", "both, no SiLU", 3, 12, 2, 5, 50, affine=True, ada=True, act=False),
] + [N_(f"{d}-{m}", f"channel-structured activations ({d}), tangent {'random' if m == 'rand' else 'proportional to x'}" +
        ("; one group constant in x" + (" and in dx" if m == "prop" else " with a random tangent") if d == "constant" else ""),
        2, 16, 8, 4, 64, data=d, dxmode=m) for d in GS.DATA_NAMES for m in ("rand", "prop")]
GN_CHAINED = [("dy-1e3", 1e3), ("dy-1e-3", 1e-3)]          # group_norm_jvp -> conv_tangent with |dy| ~ f |y|
PROP = 0.75                          # dx = PROP * x (exact in float32)


def gn_route(c):
    HW = c.H * c.W
    return _route("lc_groupnorm_jvp_route", 8, c.B, c.C, c.H, c.W, c.G, batch_stride(c.xl, c.C, HW), batch_stride(c.dxl, c.C, HW),
                  addr_mod16(c.xl, c.C, HW), addr_mod16(c.dxl, c.C, HW))


def gn_operands(c):
    """-> (dict of float32 CPU leaves: x, dx, gamma, beta [C], scale, shift, dscale, dshift [B, C] where present;
    the group constant in x or None)."""
    seed = 9700 + sum(map(ord, c.name))
    const = None
    if c.data is None:
        x = seeded_randn(c.B, c.C, c.H, c.W, seed=seed) * 2 + 0.3
    else:
        x, const = GS.tensor_data(c.B, c.C, c.H, c.W, c.G, c.data, seed=seed % 97)
        x = x.float()
    dx = x * PROP if c.dxmode == "prop" else seeded_randn(c.B, c.C, c.H, c.W, seed=seed + 1)
    t = dict(x=x, dx=dx)
    if c.affine:
        t.update(gamma=1 + 0.2 * seeded_randn(c.C, seed=seed + 2), beta=0.3 * seeded_randn(c.C, seed=seed + 3))
    if c.ada:
        t.update(scale=0.3 * seeded_randn(c.B, c.C, seed=seed + 4), shift=0.3 * seeded_randn(c.B, c.C, seed=seed + 5),
                 dscale=0.3 * seeded_randn(c.B, c.C, seed=seed + 6), dshift=0.3 * seeded_randn(c.B, c.C, seed=seed + 7))
    return t, const


def gn_closed(t, G, act, dtype, defect=None):
    """(y, dy) of y = silu?((GN(x) gamma + beta)(1 + s) + sh) and its tangent along (dx, ds, dsh), written out, in `dtype`:
    n = (x - mu) rho, dn = rho (dx - mean dx - n mean(n dx)), da = dn gamma (1 + s) + (n gamma + beta) ds + dsh,
    dy = silu'(a) da.  defect "no-mndx": the mean(n dx) term left out."""
    x, dx = t["x"].to(dtype), t["dx"].to(dtype)
    B, C = x.shape[:2]
    v, dv = x.reshape(B, G, -1), dx.reshape(B, G, -1)
    mu = v.mean(-1, keepdim=True)
    rho = (v.var(-1, unbiased=False, keepdim=True) + EPS).rsqrt()
    n = (v - mu) * rho
    dc = dv - dv.mean(-1, keepdim=True)
    mndx = (n * dc).mean(-1, keepdim=True)          # = mean(n dx): mean(n) = 0; the centred form keeps float32 conditioned
    if defect == "no-mndx":
        mndx = torch.zeros_like(mndx)
    dn = rho * (dc - n * mndx)
    n, dn = n.reshape(x.shape), dn.reshape(x.shape)
    one = lambda k, shape: t[k].to(dtype).reshape(shape) if k in t else None
    ga, be = one("gamma", (1, C, 1, 1)), one("beta", (1, C, 1, 1))
    sc, sh, dsc, dsh = (one(k, (B, C, 1, 1)) for k in ("scale", "shift", "dscale", "dshift"))
    aff = n * ga + be if ga is not None else n
    da = dn * ga if ga is not None else dn
    a = aff
    if sc is not None:
        a = aff * (1 + sc) + sh
        da = da * (1 + sc) + aff * dsc + dsh
    if act:
        sg = torch.sigmoid(a)
        return a * sg, da * sg * (1 + a * (1 - sg))
    return a, da


def gn_group_err(got, ref64, G, skip=None):
    e = GS.group_err(got, ref64, G)
    if skip is not None:
        e = e.clone()
        e[:, skip] = 0.0
    return e


def gn_const_closed(t, c, const):
    """The constant group's closed forms [B, cpg] in float64: y = silu?(a), a = beta (1 + s) + sh; with a constant tangent
    dy = silu'(a) (beta ds + dsh)."""
    cpg = c.C // c.G
    sl = slice(const * cpg, (const + 1) * cpg)
    z = torch.zeros(c.B, cpg, dtype=torch.float64)
    be = t["beta"].double()[None, sl] + z if "beta" in t else z
    a, da = be, z
    if "scale" in t:
        a = be * (1 + t["scale"].double()[:, sl]) + t["shift"].double()[:, sl]
        da = be * t["dscale"].double()[:, sl] + t["dshift"].double()[:, sl]
    if c.act:
        sg = torch.sigmoid(a)
        return a * sg, da * sg * (1 + a * (1 - sg))
    return a, da


def gn_const_bounds(t, c, const):
    """Absolute bounds [B, cpg] on the constant group's y and (constant tangent) dy: one rounding of the mean times
    1 / sqrt(eps) with GS.constant_bound's factor 2 for y; the tangent's mean is a float32 sum per lane of up to 16 equal
    values (four roundings) before it is float64: 8 ulp instead of 2.  Plus 4 ulp of the largest term of the affine part."""
    cpg = c.C // c.G
    sl = slice(const * cpg, (const + 1) * cpg)
    one = torch.ones(c.B, cpg, dtype=torch.float64)
    ga = t["gamma"].double()[None, sl] * one if "gamma" in t else one
    be = t["beta"].double()[None, sl] * one if "beta" in t else 0 * one
    sc = 1 + t["scale"].double()[:, sl] if "scale" in t else one
    sh = t["shift"].double()[:, sl] if "shift" in t else 0 * one
    dsc = t["dscale"].double()[:, sl] if "dscale" in t else 0 * one
    dsh = t["dshift"].double()[:, sl] if "dshift" in t else 0 * one
    lvl = t["x"].double()[:, sl, 0, 0].abs()
    dlvl = t["dx"].double()[:, sl, 0, 0].abs()
    ulp = GS.F32_ULP
    by = 1000.0 * ulp * lvl * (ga * sc).abs() + 4.0 * ulp * torch.stack([(be * sc).abs(), sh.abs(), (be * sc + sh).abs()]).amax(0)
    # silu' <= 1.1; the primal's own rounding (rstd (x - mu) within `by` / |ga sc|) reaches dy through ds
    bdy = 1.1 * (4000.0 * ulp * dlvl * (ga * sc).abs() + by * dsc.abs() / sc.abs().clamp_min(1e-3) +
                 4.0 * ulp * torch.stack([(be * dsc).abs(), dsh.abs(), (be * dsc + dsh).abs()]).amax(0)) + by
    return by, bdy


NRef = collections.namedtuple("NRef", "t const y dy e32_y e32_dy bound_y bound_dy skip_y skip_dy")


@functools.lru_cache(maxsize=None)
def gn_ref(c):
    t, const = gn_operands(c)
    y, dy = gn_closed(t, c.G, c.act, torch.float64)
    y32, dy32 = gn_closed(t, c.G, c.act, torch.float32)
    skip_y = const
    skip_dy = const if (const is not None and c.dxmode == "prop") else None      # constant in x AND in dx
    e32_y = float(gn_group_err(y32, y, c.G, skip_y).max())
    e32_dy = float(gn_group_err(dy32, dy, c.G, skip_dy).max())
    assert all(v == v and v < float("inf") for v in (e32_y, e32_dy)), "the float32 oracle is not finite"
    tol = GS.TOL_COMMON if c.data == "common" else GS.TOL_ENTRY
    return NRef(t, const, y, dy, e32_y, e32_dy, max(tol, MARGIN * e32_y), max(tol, MARGIN * e32_dy), skip_y, skip_dy)


def gn_chained_operands(name, f):
    """x, dx [2, 64, 8, 64] with |dx| ~ f |x| through GroupNorm(8, affine) + SiLU, then a 3 x 3 ring conv 64 -> 64."""
    seed = 9900 + sum(map(ord, name))
    B, C, H, W = 2, 64, 8, 64
    t = dict(x=seeded_randn(B, C, H, W, seed=seed) * 2 + 0.3, dx=seeded_randn(B, C, H, W, seed=seed + 1) * f,
             gamma=1 + 0.2 * seeded_randn(C, seed=seed + 2), beta=0.3 * seeded_randn(C, seed=seed + 3))
    w = seeded_randn(C, C, 3, 3, seed=seed + 4) / (C * 9) ** 0.5
    return t, w


# ------------------------------------------------------------------------------------------------ attention JVP
ACase = collections.namedtuple("ACase", "name edge dqk dv Lq Lk pattern")
BH = 3


def A_(name, edge, dqk, dv, Lq, Lk, pattern="random"):
    return ACase(name, edge, dqk, dv, Lq, Lk, pattern)


WIDTHS = [(1, 1), (8, 8), (20, 20), (32, 32), (32, 33), (33, 32), (20, 40), (40, 8), (48, 48), (64, 64)]
PATTERNS = ["rising", "falling", "hot0", "hot15", "hot16", "hotlast", "equal", "tied", "offset500"]
PATTERN_EDGE = {
    "rising": "scores rise by half a nat per key: the running maximum rises in every 16-key tile",
    "falling": "scores fall by 4 nats per key: the tail is below 2^-150 of the head, p underflows to exactly 0",
    "hot0": "one-hot at key 0 (200 nats above the rest)",
    "hot15": "one-hot at key 15: the last key of the first tile",
    "hot16": "one-hot at key 16: the first key of the second tile",
    "hotlast": "one-hot at the last key: the maximum rises only there, everything before is rescaled to 0",
    "equal": "k = 0: all scores equal, dS comes from dk alone",
    "tied": "two tied maxima (keys 3 and 20: identical columns of k) in different tiles",
    "offset500": "a common score offset of about +500 in base-2 units",
}
ATTN_CASES = (
    [A_(f"w{a}x{b}", f"widths ({a}, {b})", a, b, 65, 33) for a, b in WIDTHS] +
    [A_(f"d32-lq{n}", f"Lq = {n} on the 64-row blocks of D = 32", 20, 20, n, 17) for n in (1, 63, 64, 65)] +
    [A_(f"d64-lq{n}", f"Lq = {n} on the 32-row blocks of D = 64", 48, 48, n, 17) for n in (1, 31, 32, 33)] +
    [A_(f"d32-lk{n}", f"Lk = {n} on D = 32", 32, 32, 5, n) for n in (1, 15, 16, 17, 33)] +
    [A_(f"d64-lk{n}", f"Lk = {n} on D = 64", 64, 64, 5, n) for n in (1, 15, 16, 17, 33)] +
    # (offset500: a power-of-two scale and k[1:] = 0 keep the scores exact in float32, so the oracle stays under its cap)
    [A_(f"d32-{p}", PATTERN_EDGE[p], 16 if p == "offset500" else 32, 32, 7, 33, p) for p in PATTERNS] +
    [A_(f"d64-{p}", PATTERN_EDGE[p], 64 if p == "offset500" else 33, 64, 7, 33, p) for p in PATTERNS] +
    [A_(f"d1-{p}", PATTERN_EDGE[p] + "; one channel", 1, 1, 3, 33, p) for p in ("rising", "hotlast")])
# FlashAttentionJvp's backward on the saved o, lse: widths 32 and 64 at the Lq and Lk edges
ATTN_BWD_CASES = ([A_(f"bwd-d32-lq{n}", "backward", 32, 32, n, 17) for n in (1, 63, 64, 65)] +
                  [A_(f"bwd-d64-lq{n}", "backward", 64, 64, n, 17) for n in (1, 31, 32, 33)] +
                  [A_(f"bwd-d{d}-lk{n}", "backward", d, d, 33, n) for d in (32, 64) for n in (1, 15, 16, 17, 33)])


def attn_route(c):
    return _route("lc_attention_jvp_route", 8, BH, c.Lq, c.Lk, c.dqk, c.dv)


def attn_win(c):
    """The winning key of a one-hot row, else None."""
    if c.pattern.startswith("hot"):
        return c.Lk - 1 if c.pattern == "hotlast" else int(c.pattern[3:])
    return None


def attn_operands(c):
    """-> dict q, dq [BH, dqk, Lq]; k, dk [BH, dqk, Lk]; v, dv [BH, dv, Lk] float32 (CPU), scale.  A designed pattern
    lives in channel 0: q[0] = 1 exactly, k[0] = b_s / scale; the other channels of k are 0.01 randn (0 where the pattern
    needs exact ties), far below the gaps, so that float32 and float64 agree on the order."""
    seed = 9800 + sum(map(ord, c.name))
    mk = lambda ch, L, i: seeded_randn(BH, ch, L, seed=seed + i)
    q, k, v = mk(c.dqk, c.Lq, 0), mk(c.dqk, c.Lk, 1), mk(c.dv, c.Lk, 2)
    dq, dk, dv = mk(c.dqk, c.Lq, 3), mk(c.dqk, c.Lk, 4), mk(c.dv, c.Lk, 5)
    scale = c.dqk ** -0.5
    s = torch.arange(c.Lk, dtype=torch.float64)
    b = None
    if c.pattern == "rising":
        b = 0.5 * s
    elif c.pattern == "falling":
        b = -4.0 * s
    elif c.pattern.startswith("hot"):
        b = seeded_randn(c.Lk, seed=seed + 6).double()
        b[attn_win(c)] = 200.0
    elif c.pattern == "tied":
        b = seeded_randn(c.Lk, seed=seed + 6).double()
        b[3] = b[20] = 30.0
    elif c.pattern == "offset500":
        b = (500.0 / LOG2E + seeded_randn(c.Lk, seed=seed + 6).double()).float().double()
    if c.pattern == "equal":
        k = torch.zeros_like(k)
    elif b is not None:
        q[:, 0] = 1.0
        k = k * (0.0 if c.pattern == "offset500" else 0.01)
        k[:, 0] = (b / scale).float()[None]
        if c.pattern == "tied":
            k[:, :, 20] = k[:, :, 3]
    return dict(q=q, k=k, v=v, dq=dq, dk=dk, dv=dv, scale=scale)


def attn_closed(t, dtype, defect=None, drop=None):
    """-> dict o, do [BH, dv, Lq], lse [BH, Lq] (base 2), S_o, S_do, p [BH, Lq, Lk] in `dtype`, written out:
    p = softmax(S), dS = scale (dq^T k + q^T dk), mu = sum p dS, o = sum p v, do = sum p (dS v + dv) - mu o.
    defects: "drop-key" (key `drop` left out), "drop-channel" (channel `drop` of q / k left out of S and dS), "no-mu"."""
    q, k, v, dq, dk, dv = (t[n].to(dtype) for n in ("q", "k", "v", "dq", "dk", "dv"))
    scale = t["scale"]
    if defect == "drop-channel":
        keep = [i for i in range(q.shape[1]) if i != drop]
        q, k, dq, dk = q[:, keep], k[:, keep], dq[:, keep], dk[:, keep]
    if defect == "drop-key":
        keep = [i for i in range(k.shape[2]) if i != drop]
        k, dk, v, dv = k[:, :, keep], dk[:, :, keep], v[:, :, keep], dv[:, :, keep]
    S = torch.einsum("bct,bcs->bts", q, k) * scale
    dS = (torch.einsum("bct,bcs->bts", dq, k) + torch.einsum("bct,bcs->bts", q, dk)) * scale
    m = S.amax(-1, keepdim=True)
    e = (S - m).exp()
    l = e.sum(-1, keepdim=True)
    p = e / l
    mu = (p * dS).sum(-1)                                                    # [BH, Lq]
    o = torch.einsum("bts,bcs->bct", p, v)
    T = torch.einsum("bts,bcs->bct", p * dS, v) + torch.einsum("bts,bcs->bct", p, dv)
    do = T if defect == "no-mu" else T - mu[:, None, :] * o
    S_o = torch.einsum("bts,bcs->bct", p, v.abs())
    S_do = torch.einsum("bts,bcs->bct", p * dS.abs(), v.abs()) + torch.einsum("bts,bcs->bct", p, dv.abs()) + mu.abs()[:, None, :] * S_o
    lse = (m[..., 0] + l[..., 0].log()) * LOG2E
    return dict(o=o, do=do, lse=lse, S_o=S_o, S_do=S_do, p=p)


def attn_elem_err(got, ref64, S):
    """worst |got - ref64| / S over the elements (S > 0 everywhere: v and dv have no zero column)."""
    return float(((got.detach().cpu().double().reshape(ref64.shape) - ref64).abs() / S).max())


ARef = collections.namedtuple("ARef", "t r e32_o e32_do e32_lse bound_o bound_do")


@functools.lru_cache(maxsize=None)
def attn_ref(c):
    t = attn_operands(c)
    r = attn_closed(t, torch.float64)
    r32 = attn_closed(t, torch.float32)
    assert float(r["S_o"].min()) > 0 and float(r["S_do"].min()) > 0
    e_o, e_do = attn_elem_err(r32["o"], r["o"], r["S_o"]), attn_elem_err(r32["do"], r["do"], r["S_do"])
    e_lse = float(((r32["lse"].double() - r["lse"]).abs() / r["lse"].abs().clamp_min(1.0)).max())
    assert all(v == v and v < float("inf") for v in (e_o, e_do, e_lse)), "the float32 oracle is not finite"
    return ARef(t, r, e_o, e_do, e_lse, max(TOL_ATTN, MARGIN * e_o), max(TOL_ATTN, MARGIN * e_do))


def attn_bwd_ref(c, dtype):
    """Autograd of the plain attention in `dtype` -> (o, dq, dk, dv) for the row's q, k, v and go = the row's dv-shaped seed."""
    t = attn_operands(c)
    q, k, v = (t[n].to(dtype).clone().requires_grad_() for n in ("q", "k", "v"))
    go = seeded_randn(BH, c.dv, c.Lq, seed=9899 + c.Lq + c.Lk).to(dtype)
    p = (torch.einsum("bct,bcs->bts", q, k) * t["scale"]).softmax(-1)
    o = torch.einsum("bts,bcs->bct", p, v)
    o.backward(go)
    return go, o.detach(), q.grad, k.grad, v.grad
