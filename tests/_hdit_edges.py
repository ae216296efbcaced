"""Case tables, float64 oracles and bounds of the HDiT edge tests (tests/test_hdit_edges.py on the GPU,
tests/test_hdit_edges_host.py on the CPU): one place, so the two files cannot drift apart.  No GPU code here.

The kernels: csrc/hdit.hip (9 entry points) and csrc/hdit_bwd.hip (5).  One table per entry point; every row names the edge
it is there for.  Every oracle is a plain torch restatement that runs in the dtype of its operands: float64 is the
reference, the same restatement in float32 on the CPU is the yardstick.

Metrics (never one figure per tensor):
  per-token kernels (RMSNorm, qk_prep, their dx / dq / dk)   rel-L2 over the channels of each (sample[, head], token)
  neighbourhood attention o, dq, dk, dv                      rel-L2 over the channels of each (sample, head, token)
  its log-sum-exp                                            |err| / max(1, |lse64|)
  elementwise and reduced results                            |got - ref64| / S per element, S the float64 sum of the absolute
                                                             terms of that element; where S == 0 the result is exactly 0
  a slice whose float64 reference is exactly zero (the all-zero token, the one-key window) must be exactly zero
Bounds: no new tolerance.  Each figure is at most max(T, MARGIN x the float32 oracle's worst figure of the same metric on
the same row), MARGIN = _gn_structured.MARGIN, T the constant the existing test of that kernel uses (below).

What S is where the result is not a plain sum:
  GEGLU        a * 0.5 g (1 + erf(g / sqrt 2)):  S = |a| 0.5 |g| (1 + |erf|); the cancellation of 1 + erf at g << 0 is the
               formula's own (torch's float32 GELU has it too).  The backward likewise, term by term.
  lerp         s + w (z - s):  S = |s| + w (|z| + |s|); from weight 0.5 the kernel (as torch.lerp) evaluates
               z - (z - s)(1 - w), whose own absolute terms are at most three times that
  d(skip)      (1 - w) g = g - w g:  S = (1 + w) |g|
  Fourier      cos / sin of the float32 argument: absolute error (S = 1)
The restatements write 1 - sigmoid(alpha) as sigmoid(-alpha): the float32 yardstick then keeps d(alpha) at alpha = 20,
where 1 - 1.0f is 0."""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from lidarcrafter_amd.testing import seeded_randn
from tests import _gn_structured as GS
from tests._profile_cases import TOL_NA, TOL_NA_BWD   # noqa: F401  (no new tolerance)
from tests._train_edges import GUARD, SIGNAL_OVER_BOUND, guarded, layout, outside, place, rel_to_S   # noqa: F401

MARGIN = GS.MARGIN
# block constants the tables depend on
RMS_TOKENS, RMS_QUARTERS = 64, 4     # rmsnorm_kernel / rmsnorm_bwd_kernel: 64 tokens x 4 channel quarters per block
LANES = 256                          # every other kernel of csrc/hdit.hip and csrc/hdit_bwd.hip: 256 lanes per block
GRID_CAP = 4096                      # grid_for() of both files: at most 4096 blocks, then the grid-stride loop
PASS = GRID_CAP * LANES              # elements of one pass of a grid-stride kernel
# the constants of the existing tests
T_FWD = 1e-6         # test_hdit: RMSNorm, GEGLU, lerp, tokenizer
T_QK = 2e-6          # test_hdit::test_qk_prep_against_float64, test_hdit_training::test_qk_prep_backward_against_float64
T_FOURIER = 2e-6     # test_hdit::test_tokenize_and_fourier_against_float64
T_BWD = 2e-6         # test_hdit_training: RMSNorm / GEGLU backward (and, by the issue's list, the lerp backward)
T_DSCALE = 1e-5      # test_hdit_training::test_qk_prep_backward_against_float64, d(scale)
EPS = 1e-6
NORM_CLAMP = 1e-6    # qk_prep: F.normalize(eps = 1e-6)
LN100_F32 = torch.tensor(math.log(100), dtype=torch.float32).item()
LC_EINVAL, LC_EUNSUP = -1, -2
INF = float("inf")


def blocks(n, per=LANES):
    """-> (number of blocks, live lanes of the last one)."""
    return -(-n // per), (n - 1) % per + 1


def passes(n):
    """-> (passes of a grid-stride kernel over n elements, elements of the last pass)."""
    return -(-n // PASS), (n - 1) % PASS + 1


# ------------------------------------------------------------------------------------------------ layouts and metrics
def place3(values, kind, device, fill=float("nan")):
    """[B, C, L] values as a view of `place`'s layouts (L in the role of H W) -> (view [B, C, L], buffer)."""
    v, buf = place(values[:, :, None, :], kind, device, fill)
    return v[:, :, 0, :], buf


def place_pitch(values, pad, device, fill=float("nan")):
    """[B, C, L] values with a channel pitch of L + pad inside a `fill`ed buffer -> (view, buffer)."""
    B, C, L = values.shape
    buf = torch.full((2 * GUARD + B * C * (L + pad),), fill, dtype=torch.float32, device=device)
    view = buf.as_strided((B, C, L), (C * (L + pad), L + pad, 1), GUARD)
    view.copy_(values)
    return view, buf


def vec_err(got, ref64, dim):
    """rel-L2 over `dim` of every remaining slice; a slice whose reference is exactly zero gives 0 if `got` is exactly
    zero there and inf otherwise."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    num, den = (got - ref64).pow(2).sum(dim).sqrt(), ref64.pow(2).sum(dim).sqrt()
    e = num / den.clamp_min(1e-300)
    zero = torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, INF))
    return torch.where(den == 0, zero, e)


def worst(e):
    """The largest figure; NaN (a NaN in the result) counts as inf."""
    e = torch.nan_to_num(e.reshape(-1), nan=INF, posinf=INF)
    return float(e.max()) if e.numel() else 0.0


def elem_err(got, ref64, S):
    """rel_to_S with an element that is nonzero where S == 0, or not finite, counted as inf."""
    e, nz, fin = rel_to_S(got.reshape(ref64.shape), ref64, S)
    return INF if (nz or not fin or e != e) else e


def bound(T, e32):
    return max(T, MARGIN * e32)


def heads_view(t, heads):
    B, C, L = t.shape
    return t.reshape(B, heads, C // heads, L)


def token_err(got, ref64, heads=None):
    """[B, C, L] -> worst rel-L2 over the channels of a (sample, token), or of a (sample, head, token)."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    if heads is None:
        return worst(vec_err(got, ref64, 1))
    return worst(vec_err(heads_view(got, heads), heads_view(ref64, heads), 2))


def zero_last_token(ref):
    """Mutant: the last token of a partial block left at zero."""
    out = ref.clone()
    out[..., -1] = 0
    return out


def zero_second_pass(ref):
    """Mutant: element e + 4096 * 256 of every sample ([B, ...]) left unwritten (zero)."""
    out = ref.clone().reshape(ref.shape[0], -1)
    out[:, PASS:] = 0
    return out.reshape(ref.shape)


# ------------------------------------------------------------------------------------------------ RMSNorm
RCase = collections.namedtuple("RCase", "name edge form B C L mode xl xmag zero_token")
MODES = ("plain", "mod", "gain")


def R_(name, edge, B, C, L, mode, form="grid", xl="contig", xmag=3.0, zero_token=False):
    return RCase(name, edge, form, B, C, L, mode, xl, xmag, zero_token)


def _rms_rows():
    rows = []
    quarter = {1: "C = 1 < 4: one quarter holds the channel, three are empty", 2: "C = 2 < 4: two empty quarters",
               3: "C = 3 < 4: one empty quarter", 5: "C = 5, cq = 2: the third quarter holds one channel, the fourth starts past C",
               96: "C = 96: four whole quarters", 130: "C = 130, cq = 33: a short last quarter of 31"}
    for C in (1, 2, 3, 5, 96, 130):
        for mode in MODES:
            # C = 1: dx = r g eps / (x^2 + eps) cancels to nothing unless x^2 is of the order of eps
            rows.append(R_(f"c{C}-{mode}", quarter[C] + "; L = 65: one live lane in the second block", 2, C, 65, mode,
                           xmag=2e-3 if C == 1 else 3.0))
    tok = {1: "L = 1", 63: "L = 63: one short block", 64: "L = 64: exactly one block", 65: "L = 65", 129: "L = 129: three blocks"}
    for i, L in enumerate((1, 63, 64, 65, 129)):
        rows.append(R_(f"l{L}", tok[L], 2, 5, L, MODES[(i + 1) % 3]))
    rows.append(R_("l128-full", "L = 128: exactly two blocks", 2, 6, 128, "mod"))
    for M, C, mode in ((1, 3, "plain"), (5, 3, "mod"), (1, 256, "gain"), (5, 256, "mod"), (5, 256, "plain"), (5, 3, "gain")):
        rows.append(R_(f"rows-m{M}-c{C}-{mode}", f"row form [M, C] = [{M}, {C}]: L = 1, unit channel stride", M, C, 1, mode, form="rows"))
    rows += [
        R_("x-slice-hi", "x a channel slice: batch stride > C L and a base 3 L floats in", 2, 5, 65, "mod", xl="slice_hi"),
        R_("x-bs1", "x with a batch stride of C L + 1", 3, 6, 63, "gain", xl="bs1"),
        R_("rows-slice-hi", "row form with a row pitch of C + 3", 5, 3, 1, "mod", form="rows", xl="slice_hi"),
        R_("zero-token", "the lone live token of the second block is all zeros: y = 0, r = 1 / sqrt(eps) in the backward", 2, 5, 65,
           "gain", zero_token=True),
    ]
    for L in (1, 255, 257):
        rows.append(R_(f"dgain-l{L}", f"d(gain) over B = 3 samples, L = {L}: the 256-stride token loop and its tree", 3, 5, L, "gain"))
        rows.append(R_(f"dmod-l{L}", f"d(mod), L = {L}", 2, 5, L, "mod"))
    return rows


RMS = _rms_rows()


def rms_last_quarter(C):
    """Channels [lo, hi) of the highest non-empty quarter (cq = (C + 3) / 4)."""
    cq = (C + 3) // 4
    q = (C - 1) // cq
    return q * cq, min(C, (q + 1) * cq)


def rms_operands(c):
    seed = sum(map(ord, c.name))
    x = seeded_randn(c.B, c.C, c.L, seed=7100 + seed) * c.xmag
    if c.zero_token:
        x[c.B - 1, :, c.L - 1] = 0.0
    dy = seeded_randn(c.B, c.C, c.L, seed=7101 + seed)
    f = None
    if c.mode == "mod":
        f = seeded_randn(c.B, 2 * c.C, seed=7102 + seed)[:, c.C:]           # a strided [B, C] view
    elif c.mode == "gain":
        f = 1 + 0.1 * seeded_randn(c.C, seed=7103 + seed)
    return x, dy, f


def _rms_factor(f, mode):
    if mode == "plain":
        return 1.0
    return (1 + f)[:, :, None] if mode == "mod" else f[None, :, None]


def _rms_r(x, skip_last_quarter):
    sq = x.pow(2)
    if skip_last_quarter:
        lo, hi = rms_last_quarter(x.shape[1])
        sq = sq.clone()
        sq[:, lo:hi] = 0
    return torch.rsqrt(sq.sum(1, keepdim=True) / x.shape[1] + EPS)


def rms_fwd(x, f, mode, skip_last_quarter=False):
    """x [B, C, L] -> x rsqrt(mean_c x^2 + eps) f.  skip_last_quarter: the mutant whose sum of squares misses a quarter."""
    return x * _rms_r(x, skip_last_quarter) * _rms_factor(f, mode)


def rms_bwd(x, f, mode, dy, skip_last_quarter=False):
    """-> (dx, df or None, S of df or None): dx = r g - x r^3 (sum_c g x) / C with g = dy f; df = sum dy x r."""
    r = _rms_r(x, skip_last_quarter)
    g = dy * _rms_factor(f, mode)
    dx = r * g - x * r.pow(3) * (g * x).sum(1, keepdim=True) / x.shape[1]
    if mode == "plain":
        return dx, None, None
    t = dy * x * r
    dims = (2,) if mode == "mod" else (0, 2)
    return dx, t.sum(dims), t.abs().sum(dims)


def rms_autograd(x, f, mode, dy):
    x = x.clone().requires_grad_()
    f = None if f is None else f.clone().requires_grad_()
    y = x * torch.rsqrt(x.pow(2).mean(1, keepdim=True) + EPS)
    if mode == "mod":
        y = y * (1 + f)[:, :, None]
    elif mode == "gain":
        y = y * f[None, :, None]
    y.backward(dy)
    return y.detach(), x.grad, None if f is None else f.grad


RRef = collections.namedtuple("RRef", "x dy f y dx df S_df e32 bound")


@functools.lru_cache(maxsize=None)
def rms_ref(c):
    x, dy, f = rms_operands(c)
    d = lambda t: None if t is None else t.double()  # noqa: E731
    y = rms_fwd(d(x), d(f), c.mode)
    dx, df, S = rms_bwd(d(x), d(f), c.mode, d(dy))
    dx32, df32, _ = rms_bwd(x, f, c.mode, dy)
    e32 = dict(y=token_err(rms_fwd(x, f, c.mode), y), dx=token_err(dx32, dx))
    bnd = dict(y=bound(T_FWD, e32["y"]), dx=bound(T_BWD, e32["dx"]))
    if df is not None:
        e32["df"] = elem_err(df32, df, S)
        bnd["df"] = bound(T_BWD, e32["df"])
    return RRef(x, dy, f, y, dx, df, S, e32, bnd)


# ------------------------------------------------------------------------------------------------ GEGLU
GCase = collections.namedtuple("GCase", "name edge form B mid L xl")
PLANTED_GATES = (0.0, -0.0, 0.5, -0.5, 6.0, -6.0, 10.0, -10.0, 40.0)    # erf saturation, the underflow of exp(-g g / 2)
GEGLU = [
    GCase("n1", "mid L = 1", "grid", 2, 1, 1, "contig"),
    GCase("n255", "mid L = 255: one short block", "grid", 2, 5, 51, "slice_hi"),
    GCase("n257", "mid L = 257: one live lane in the second block", "grid", 2, 1, 257, "bs1"),
    GCase("n512-full", "mid L = 512: exactly two blocks", "grid", 2, 2, 256, "contig"),
    GCase("second-pass", "mid L = 1 049 400 > 4096 * 256, % 256 != 0: a partial second pass of the grid-stride loop", "grid", 1, 33,
          31800, "contig"),
    GCase("rows-m3", "row form [M, 2 mid] = [3, 96]: L = 1", "rows", 3, 48, 1, "contig"),
]
INV_SQRT2, INV_SQRT2PI = 0.70710678118654752, 0.39894228040143268


def geglu_operands(c):
    seed = sum(map(ord, c.name))
    x = seeded_randn(c.B, 2 * c.mid, c.L, seed=7200 + seed) * 2
    n = c.mid * c.L
    k = min(n, len(PLANTED_GATES))
    planted = torch.tensor(PLANTED_GATES[:k])
    x[0, c.mid:].reshape(-1)[:k] = planted                      # the first gates of the first sample
    x[c.B - 1, c.mid:].reshape(-1)[n - k:] = planted            # the last gates of the last: the second pass where there is one
    return x, seeded_randn(c.B, c.mid, c.L, seed=7201 + seed)


def geglu_fwd(x, mid):
    """-> (y, S)."""
    a, g = x[:, :mid], x[:, mid:]
    erf = torch.erf(g * INV_SQRT2)
    return a * (0.5 * g * (1 + erf)), a.abs() * (0.5 * g.abs() * (1 + erf.abs()))


def geglu_bwd(x, dy, mid):
    """-> (dx [B, 2 mid, L], S): da = dy gelu(g), dg = dy a (Phi(g) + g phi(g))."""
    a, g = x[:, :mid], x[:, mid:]
    erf = torch.erf(g * INV_SQRT2)
    phi = INV_SQRT2PI * torch.exp(-0.5 * g * g)
    dx = torch.cat([dy * (0.5 * g * (1 + erf)), dy * a * (0.5 * (1 + erf) + g * phi)], 1)
    S = torch.cat([dy.abs() * (0.5 * g.abs() * (1 + erf.abs())), (dy * a).abs() * (0.5 * (1 + erf.abs()) + g.abs() * phi)], 1)
    return dx, S


def geglu_autograd(x, dy, mid):
    x = x.clone().requires_grad_()
    y = x[:, :mid] * F.gelu(x[:, mid:])
    y.backward(dy)
    return y.detach(), x.grad


GRef = collections.namedtuple("GRef", "x dy y S_y dx S_dx e32 bound")


@functools.lru_cache(maxsize=None)
def geglu_ref(c):
    x, dy = geglu_operands(c)
    y, S_y = geglu_fwd(x.double(), c.mid)
    dx, S_dx = geglu_bwd(x.double(), dy.double(), c.mid)
    e32 = dict(y=elem_err(geglu_fwd(x, c.mid)[0], y, S_y), dx=elem_err(geglu_bwd(x, dy, c.mid)[0], dx, S_dx))
    return GRef(x, dy, y, S_y, dx, S_dx, e32, dict(y=bound(T_FWD, e32["y"]), dx=bound(T_BWD, e32["dx"])))


# ------------------------------------------------------------------------------------------------ q / k preparation
QCase = collections.namedtuple("QCase", "name edge d L separate scales")
QK_B, QK_HEADS = 2, 3
QK_PAD = 4                                          # channels between the q, k and v slices of the shared buffer
SCALE_SETS = ((0.7, LN100_F32, 5.2), (20.0, -30.0, LN100_F32))     # below, exactly at and above ln 100; far above; far below
PLANT_NORMS = (0.0, 5e-7, 2e-6)                     # all zero; clamped; not clamped: a factor 2 either side of 1e-6
QK_EDGE = {1: "L = 1", 255: "L = 255: one short block", 256: "L = 256: exactly one block", 257: "L = 257: one live lane in the second block"}
QK = [QCase(f"d{d}-l{L}", QK_EDGE[L] + "; q, k slices of one [B, 3C + 4, L] buffer", d, L, False, SCALE_SETS[(i + j) % 2])
      for i, d in enumerate((32, 64)) for j, L in enumerate((1, 255, 256, 257))] + [
    QCase("separate-pitch", "q and k in separate buffers with channel pitches L + 3 and L + 5", 32, 257, True, SCALE_SETS[1]),
]


def qk_plants(L):
    """(tensor, sample, head, token, norm) of the planted tokens: each norm once in q and once in k, in the last block's
    last lane and in lane 0."""
    z, cl, un = PLANT_NORMS
    return (("q", 0, 0, L - 1, z), ("q", 1, 1, 0, cl), ("q", 1, 2, L - 1, un),
            ("k", 0, 2, 0, z), ("k", 0, 1, L - 1, cl), ("k", 1, 0, 0, un))


def qk_operands(c):
    """-> dict: q, k, v [B, C, L], gq, gk, scale [heads], cos_t, sin_t [heads, d/2, L] (float32)."""
    seed = sum(map(ord, c.name))
    C = QK_HEADS * c.d
    t = {n: seeded_randn(QK_B, C, c.L, seed=7300 + i + seed) for i, n in enumerate(("q", "k", "v", "gq", "gk"))}
    for n, b, h, tok, norm in qk_plants(c.L):
        v = t[n][b, h * c.d:(h + 1) * c.d, tok].double()
        t[n][b, h * c.d:(h + 1) * c.d, tok] = (v * (norm / v.norm())).float()
    th = seeded_randn(QK_HEADS, c.d // 2, c.L, seed=7310 + seed).double() * 3
    t.update(scale=torch.tensor(c.scales, dtype=torch.float32), cos_t=th.cos().float(), sin_t=th.sin().float())
    # a tenth of the rotated unit token in the incoming gradients: d(scale) = s / 2 sum g . R u is then no sum of random signs
    # that could cancel below 16 bounds of what the `<` mutant takes away
    unit = torch.zeros(QK_HEADS)
    for n, g in (("q", "gq"), ("k", "gk")):
        t[g] = (t[g].double() + 0.1 * qk_fwd(t[n].double(), unit.double(), t["cos_t"].double(), t["sin_t"].double())).float()
    return t


def _qk_s(scale):
    return scale.clamp(max=math.log(100)).exp().sqrt().reshape(1, -1, 1, 1)


def qk_fwd(x, scale, cos_t, sin_t):
    """x [B, heads d, L] -> normalise each head's token (eps 1e-6), times sqrt(exp(min(scale, ln 100))), RoPE."""
    heads, h2 = cos_t.shape[0], cos_t.shape[1]
    v = heads_view(x, heads)
    u = v / v.pow(2).sum(2, keepdim=True).sqrt().clamp_min(NORM_CLAMP) * _qk_s(scale)
    x1, x2, c, s = u[:, :, :h2], u[:, :, h2:], cos_t[None], sin_t[None]
    return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], 2).reshape(x.shape)


def qk_bwd_one(x, g, scale, cos_t, sin_t, keep_projection=False):
    """Closed form -> (dx, sum over samples and tokens of dp . u per head, the same of |dp u|).  dp = R^T g, du = s dp,
    dx = (du - u (u . du)) / ||x||, and du / 1e-6 with no projection term where the norm was clamped.
    keep_projection: the mutant that keeps the term there."""
    heads, h2 = cos_t.shape[0], cos_t.shape[1]
    v, gg, c, s = heads_view(x, heads), heads_view(g, heads), cos_t[None], sin_t[None]
    g1, g2 = gg[:, :, :h2], gg[:, :, h2:]
    dp = torch.cat([g1 * c + g2 * s, g2 * c - g1 * s], 2)
    nrm = v.pow(2).sum(2, keepdim=True).sqrt()
    clamped = nrm <= NORM_CLAMP
    n = nrm.clamp_min(NORM_CLAMP)
    u = v / n
    du = _qk_s(scale) * dp
    proj = u * (u * du).sum(2, keepdim=True)
    if not keep_projection:
        proj = torch.where(clamped, torch.zeros_like(proj), proj)
    return ((du - proj) / n).reshape(x.shape), (dp * u).sum((0, 2, 3)), (dp * u).abs().sum((0, 2, 3))


def qk_bwd(t, dtype, keep_projection=False, strict=False):
    """-> (dq, dk, dscale [heads], S of dscale).  The gradient passes where scale <= ln 100 compared in float32 (torch's
    clamp rule); strict: the mutant that compares with <."""
    c = lambda n: t[n].to(dtype)  # noqa: E731
    dq, pq, aq = qk_bwd_one(c("q"), c("gq"), c("scale"), c("cos_t"), c("sin_t"), keep_projection)
    dk, pk, ak = qk_bwd_one(c("k"), c("gk"), c("scale"), c("cos_t"), c("sin_t"), keep_projection)
    sc = t["scale"].float()
    ok = ((sc < LN100_F32) if strict else (sc <= LN100_F32)).to(dtype)
    half_s = 0.5 * _qk_s(c("scale")).reshape(-1) * ok
    return dq, dk, half_s * (pq + pk), half_s * (aq + ak)


def qk_autograd(t):
    """float64 torch autograd of the forward, the clamp's pass rule taken from torch's own float32 clamp."""
    s32 = t["scale"].clone().requires_grad_()
    s32.clamp(max=math.log(100)).sum().backward()
    ok = s32.grad.double()
    sd = t["scale"].double().requires_grad_()
    eff = ok * (sd - sd.detach()) + sd.detach().clamp(max=math.log(100))      # the clamped value; the gradient where torch passes it
    xs = [t[n].double().requires_grad_() for n in ("q", "k")]
    c, s, h2 = t["cos_t"].double()[None], t["sin_t"].double()[None], t["cos_t"].shape[1]
    loss = 0.0
    for x, g in zip(xs, ("gq", "gk")):
        v = heads_view(x, QK_HEADS)
        v = v / v.norm(dim=2, keepdim=True).clamp_min(NORM_CLAMP) * eff.exp().sqrt().reshape(1, -1, 1, 1)    # torch.norm: 0 at 0
        x1, x2 = v[:, :, :h2], v[:, :, h2:]
        loss = loss + (torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], 2).reshape(x.shape) * t[g].double()).sum()
    loss.backward()
    return xs[0].grad, xs[1].grad, sd.grad


QRef = collections.namedtuple("QRef", "t q k dq dk ds S_ds e32 bound")


@functools.lru_cache(maxsize=None)
def qk_ref(c):
    t = qk_operands(c)
    dd = lambda n: t[n].double()  # noqa: E731
    q, k = (qk_fwd(dd(n), dd("scale"), dd("cos_t"), dd("sin_t")) for n in ("q", "k"))
    q32, k32 = (qk_fwd(t[n], t["scale"], t["cos_t"], t["sin_t"]) for n in ("q", "k"))
    dq, dk, ds, S = qk_bwd(t, torch.float64)
    dq32, dk32, ds32, _ = qk_bwd(t, torch.float32)
    H = QK_HEADS
    e32 = dict(q=token_err(q32, q, H), k=token_err(k32, k, H), dq=token_err(dq32, dq, H), dk=token_err(dk32, dk, H),
               ds=elem_err(ds32, ds, S))
    bnd = {n: bound(T_QK, e32[n]) for n in ("q", "k", "dq", "dk")}
    bnd["ds"] = bound(T_DSCALE, e32["ds"])
    return QRef(t, q, k, dq, dk, ds, S, e32, bnd)


# ------------------------------------------------------------------------------------------------ neighbourhood attention
NCase = collections.namedtuple("NCase", "name edge d grid scale o_strided")
NA_B, NA_HEADS = 2, 3
NA_GRIDS = (
    ((5, 52, 5, 7), "L = 260: the second block holds 4 live lanes; h == kh"),
    ((1, 257, 1, 9), "h = kh = 1, L = 257"),
    ((3, 4, 3, 9), "kw / 2 == w: every key sits in a window two or three times"),
    ((3, 1, 3, 3), "w = 1: one column, every key three times"),
    # kh kw = 81 with w < kw.  9 x 3 (kw / 2 = 4 > w = 3) is outside the entries' contract: NA_REFUSED_GRID
    ((9, 4, 9, 9), "kh kw = 81, the limit, with w < kw and kw / 2 == w"),
    ((2, 2, 1, 1), "the window is the query itself: o == v bit for bit, dq = dk = 0, dv = do"),
    ((4, 64, 3, 5), "L = 256: exactly one block; every key once"),
)
NA_REFUSED_GRID = (9, 3, 9, 9)
NA_SCALES = (1.0, 0.125, 2.5)
NA_SCORE_STD = 0.5
NA_KAPPA_MAX = 128.0
NA = [NCase(f"{'x'.join(map(str, g))}-d{d}-s{s}", e, d, g, s, g == (3, 4, 3, 9) and d == 32)
      for g, e in NA_GRIDS for d in (32, 64) for s in NA_SCALES]


@functools.lru_cache(maxsize=None)
def na_keys(grid, clamp=False):
    """[L, kh kw] key indices by an explicit loop over (query, window row, window slot) that appends keys: a key that sits in
    a window twice is there twice by construction.  clamp: the mutant that clamps the column where the kernel wraps it."""
    h, w, kh, kw = grid
    keys = []
    for i in range(h):
        r0 = min(max(i - kh // 2, 0), h - kh)
        for j in range(w):
            win = []
            for r in range(r0, r0 + kh):
                for s in range(kw):
                    col = j - kw // 2 + s
                    win.append(r * w + (min(max(col, 0), w - 1) if clamp else col % w))
            keys.append(win)
    return torch.tensor(keys)


def na_multiplicities(grid):
    """The set of how often one key sits in one window, over every window of the grid."""
    out = set()
    for win in na_keys(grid).tolist():
        out |= set(collections.Counter(win).values())
    return out


def na_dedup_mask(grid):
    """Mutant mask: -inf on every repeated occurrence of a key in a window (a repeated key counted once)."""
    key = na_keys(grid)
    m = torch.zeros(key.shape, dtype=torch.float64)
    for t, win in enumerate(key.tolist()):
        seen = set()
        for n, kk in enumerate(win):
            if kk in seen:
                m[t, n] = -INF
            seen.add(kk)
    return m


def na_operands(c):
    """q carries NA_SCORE_STD / (scale sqrt d): the scaled scores have that spread on every row.  dq and dk are sums of
    dS = P (dP - D) that cancel twice (D = sum P dP, then sum dS = 0), so a per-token relative figure carries the token's
    condition number `na_kappa`.  At the spread of test_hdit (3 sqrt d) one key takes all the weight of most windows and the
    figure is noise even in float32 (1e+9 on the CPU); at a spread of 2, kappa reaches 500 to 4800 and a correct float32
    evaluation lands anywhere up to 1e-4 (the kernel measured 1.0e-4 on the 1 x 257 row where the CPU float32 run happened
    to give 1.3e-5).  At 0.5 kappa stays under NA_KAPPA_MAX on every row (asserted on the CPU): a few 2^-24 per term times
    kappa is then inside TOL_NA_BWD, and the yardstick means the same for either evaluation."""
    h, w, kh, kw = c.grid
    seed = sum(map(ord, c.name))
    C, L = NA_HEADS * c.d, h * w
    qkv = seeded_randn(NA_B, 3 * C, L, seed=7400 + seed)
    return dict(q=qkv[:, :C] * (NA_SCORE_STD / (c.scale * math.sqrt(c.d))), k=qkv[:, C:2 * C].contiguous(), v=qkv[:, 2 * C:].contiguous(),
                do=seeded_randn(NA_B, C, L, seed=7401 + seed))


def na_fwd(q, k, v, key, scale, mask=None):
    """-> (o [B, C, L], lse [B heads, L], softmax weights [B, heads, L, n])."""
    B, C, L = q.shape
    qd, kd, vd = (heads_view(x, NA_HEADS) for x in (q, k, v))
    s = scale * torch.einsum("bhdl,bhdln->bhln", qd, kd[..., key])
    if mask is not None:
        s = s + mask.to(s.dtype)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    return torch.einsum("bhln,bhdln->bhdl", p, vd[..., key]).reshape(B, C, L), lse.reshape(-1, L), p


def na_all(t, c, dtype, key=None, mask=None):
    """Forward and autograd backward in `dtype` -> dict o, lse, dq, dk, dv."""
    key = na_keys(c.grid) if key is None else key
    ts = [t[n].to(dtype).clone().requires_grad_() for n in ("q", "k", "v")]
    o, lse, _ = na_fwd(*ts, key, c.scale, mask)
    o.backward(t["do"].to(dtype))
    return dict(o=o.detach(), lse=lse.detach(), dq=ts[0].grad, dk=ts[1].grad, dv=ts[2].grad)


def na_gather_ref(t, c):
    """The `% w` index gather of test_hdit.py (independent of the looped table), float64 -> o."""
    h, w, kh, kw = c.grid
    r0 = (torch.arange(h) - kh // 2).clamp(0, h - kh)
    rows = r0[:, None] + torch.arange(kh)[None]
    cols = (torch.arange(w)[:, None] - kw // 2 + torch.arange(kw)[None]) % w
    key = (rows[:, None, :, None] * w + cols[None, :, None, :]).reshape(h * w, kh * kw)
    return na_fwd(t["q"].double(), t["k"].double(), t["v"].double(), key, c.scale)[0]


def na_drop_mask(t, c):
    """Mutant mask: the key of the largest weight dropped from ONE window (sample 0, head 0, the middle query)."""
    key = na_keys(c.grid)
    p = na_fwd(t["q"].double(), t["k"].double(), t["v"].double(), key, c.scale)[2]
    q0 = key.shape[0] // 2
    m = torch.zeros(key.shape, dtype=torch.float64)
    m[q0, int(p[0, 0, q0].argmax())] = -INF
    return m


def na_kappa(c):
    """-> (worst condition number of a token's dq, of a token's dk): the sum of the absolute terms
    scale P (|dP| + sum P |dP|) ||k|| (for dk: ||q||) over the norm of the result, float64."""
    t = na_operands(c)
    key = na_keys(c.grid)
    q, k, v, do = (heads_view(t[n].double(), NA_HEADS) for n in ("q", "k", "v", "do"))
    p = na_fwd(t["q"].double(), t["k"].double(), t["v"].double(), key, c.scale)[2]
    dP = torch.einsum("bhdl,bhdln->bhln", do, v[..., key])
    dS = p * (dP - (p * dP).sum(-1, keepdim=True))
    terms = p * (dP.abs() + (p * dP.abs()).sum(-1, keepdim=True))                       # [B, heads, L, n]
    dq = torch.einsum("bhln,bhdln->bhdl", dS, k[..., key]).norm(dim=2)
    kq = (terms * k[..., key].norm(dim=2)).sum(-1) / dq
    B, H, L, n = terms.shape
    flat = key.reshape(-1)
    dk = torch.zeros(B, H, q.shape[2], L, dtype=torch.float64).index_add_(
        3, flat, (dS[:, :, None] * q[..., None]).reshape(B, H, -1, L * n)).norm(dim=2)
    num = torch.zeros(B, H, L, dtype=torch.float64).index_add_(2, flat, (terms * q.norm(dim=2)[..., None]).reshape(B, H, L * n))
    return float(kq.max()), float((num / dk).max())


NA_OUT = ("o", "lse", "dq", "dk", "dv")


def na_figures(got, ref64):
    """{name: worst figure} of whichever of o, lse, dq, dk, dv `got` holds."""
    out = {}
    for n in NA_OUT:
        if n not in got:
            continue
        if n == "lse":
            g = got[n].detach().cpu().double().reshape(ref64[n].shape)
            out[n] = worst((g - ref64[n]).abs() / ref64[n].abs().clamp_min(1.0))
        else:
            out[n] = token_err(got[n], ref64[n], NA_HEADS)
    return out


NRef = collections.namedtuple("NRef", "t ref e32 bound")


@functools.lru_cache(maxsize=None)
def na_ref(c):
    t = na_operands(c)
    ref = na_all(t, c, torch.float64)
    e32 = na_figures(na_all(t, c, torch.float32), ref)
    bnd = {n: bound(TOL_NA if n in ("o", "lse") else TOL_NA_BWD, e32[n]) for n in NA_OUT}
    return NRef(t, ref, e32, bnd)


# ------------------------------------------------------------------------------------------------ permutes, lerp
PCase = collections.namedtuple("PCase", "name edge B C H W P1 P2 il ol")     # H, W: of the UNMERGED grid [B, C, H, W]
PERMUTES = [
    PCase("n1", "n = 1", 2, 1, 1, 1, 1, 1, "contig", "contig"),
    PCase("p22-n420", "(2, 2), n = 420: one full block and a short one", 2, 7, 6, 10, 2, 2, "slice_lo", "contig"),
    PCase("p14-n540", "(1, 4), the Detokenizer's order, n = 540", 2, 3, 5, 36, 1, 4, "contig", "slice_hi"),
    PCase("p21-n90", "(2, 1), n = 90", 3, 5, 6, 3, 2, 1, "bs1", "bs1"),
    PCase("p32-n702", "(3, 2), n = 702", 2, 3, 9, 26, 3, 2, "slice_hi", "slice_lo"),
    PCase("p22-n1024-full", "n = 1024: exactly four blocks", 2, 8, 8, 16, 2, 2, "contig", "contig"),
    PCase("second-pass", "n = 1 054 000 > 4096 * 256, % 256 != 0: a partial second pass", 1, 17, 62, 1000, 2, 2, "contig", "contig"),
]


def s2d_ref(x, P1, P2):
    """PatchMerging's "B (H P1) (W P2) C -> B H W (P1 P2 C)" on the channel-major grid."""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // P1, P1, W // P2, P2).permute(0, 3, 5, 1, 2, 4).reshape(B, P1 * P2 * C, H // P1, W // P2)


def d2s_ref(z, P1, P2):
    B, Cz, h, w = z.shape
    C = Cz // (P1 * P2)
    return z.reshape(B, P1, P2, C, h, w).permute(0, 3, 4, 1, 5, 2).reshape(B, C, h * P1, w * P2)


def permute_operands(c):
    return seeded_randn(c.B, c.C, c.H, c.W, seed=7500 + sum(map(ord, c.name)))


LCase = collections.namedtuple("LCase", "name edge B C h w P1 P2 sl")        # h, w: of the MERGED grid [B, P1 P2 C, h, w]
ALPHAS = (-20.0, -3.0, -1e-3, 0.0, 1e-3, 0.4, 20.0)    # both saturations, both branches of torch.lerp, weight exactly 0.5
LERP = [
    LCase("n1", "n = 1 (alpha = 0: weight exactly 0.5)", 3, 1, 1, 1, 1, 1, "contig"),
    LCase("p22-n420", "(2, 2), n = 420; B = 3 for d(alpha)", 3, 7, 3, 5, 2, 2, "slice_lo"),
    LCase("p14-n504", "(1, 4), n = 504", 2, 7, 4, 18, 1, 4, "bs1"),
    LCase("p22-n1024-full", "n = 1024: exactly four blocks", 3, 8, 4, 8, 2, 2, "contig"),
    LCase("second-pass", "n = 1 049 536 > 4096 * 256, % 256 != 0: a partial second pass (in the eighth channel: alpha = -20)", 1, 8, 62, 529, 2, 2, "contig"),
]


def lerp_alpha(c):
    a = [0.0] if c.C == 1 else [ALPHAS[i % len(ALPHAS)] for i in range(c.C)]
    return torch.tensor(a, dtype=torch.float32)


def lerp_operands(c):
    seed = sum(map(ord, c.name))
    H, W = c.h * c.P1, c.w * c.P2
    return dict(y=seeded_randn(c.B, c.C * c.P1 * c.P2, c.h, c.w, seed=7600 + seed), skip=seeded_randn(c.B, c.C, H, W, seed=7601 + seed),
                dout=seeded_randn(c.B, c.C, H, W, seed=7602 + seed), alpha=lerp_alpha(c))


def lerp_fwd(t, c, dtype, swap_at_half=False):
    """torch.lerp(skip, d2s(y), sigmoid(alpha)) written out -> (out, S).  swap_at_half: the mutant that takes the low
    branch's formula at weight exactly 0.5 (the same value in exact arithmetic: it shows in float32 bits only)."""
    z, s = d2s_ref(t["y"].to(dtype), c.P1, c.P2), t["skip"].to(dtype)
    al = t["alpha"].to(dtype)[None, :, None, None]
    w = 1 / (1 + torch.exp(-al))
    low = (w <= 0.5) if swap_at_half else (w < 0.5)
    out = torch.where(low, s + w * (z - s), z - (z - s) * (1 - w))
    return out, s.abs() + w * (z.abs() + s.abs())


def lerp_bwd(t, c, dtype):
    """-> dict dy, dskip, dalpha and S_dy, S_dskip, S_dalpha."""
    z, s, g = d2s_ref(t["y"].to(dtype), c.P1, c.P2), t["skip"].to(dtype), t["dout"].to(dtype)
    al = t["alpha"].to(dtype)
    a, na = torch.sigmoid(al)[None, :, None, None], torch.sigmoid(-al)[None, :, None, None]
    aa = (a * na).reshape(-1)
    return dict(dy=s2d_ref(a * g, c.P1, c.P2), S_dy=s2d_ref((a * g).abs(), c.P1, c.P2), dskip=na * g, S_dskip=(1 + a) * g.abs(),
                dalpha=aa * (g * (z - s)).sum((0, 2, 3)), S_dalpha=aa * (g.abs() * (z.abs() + s.abs())).sum((0, 2, 3)))


def lerp_autograd(t, c):
    y, s, al = (t[n].double().requires_grad_() for n in ("y", "skip", "alpha"))
    out = torch.lerp(s, d2s_ref(y, c.P1, c.P2), torch.sigmoid(al)[None, :, None, None])
    out.backward(t["dout"].double())
    return out.detach(), y.grad, s.grad, al.grad


LRef = collections.namedtuple("LRef", "t out S_out out32 bwd e32 bound")
LERP_OUT = ("dy", "dskip", "dalpha")


@functools.lru_cache(maxsize=None)
def lerp_ref(c):
    t = lerp_operands(c)
    out, S = lerp_fwd(t, c, torch.float64)
    out32 = lerp_fwd(t, c, torch.float32)[0]
    bwd, b32 = lerp_bwd(t, c, torch.float64), lerp_bwd(t, c, torch.float32)
    e32 = dict(out=elem_err(out32, out, S), **{n: elem_err(b32[n], bwd[n], bwd["S_" + n]) for n in LERP_OUT})
    bnd = dict(out=bound(T_FWD, e32["out"]), **{n: bound(T_BWD, e32[n]) for n in LERP_OUT})
    return LRef(t, out, S, out32, bwd, e32, bnd)


# ------------------------------------------------------------------------------------------------ tokenizer, Fourier
TCase = collections.namedtuple("TCase", "name edge B Cin C H W P xl yl")
TOKENIZE = [
    TCase("n1", "(Cin, P) = (1, 1), n = 1", 2, 1, 1, 1, 1, 1, "contig", "contig"),
    TCase("p4-n255", "(2, 4), n = 255: one short block", 2, 2, 5, 3, 68, 4, "slice_lo", "slice_hi"),
    TCase("p2-n256-full", "(3, 2), n = 256: exactly one block", 2, 3, 4, 2, 64, 2, "contig", "contig"),
    TCase("p2-n387", "(3, 2), n = 387: one live lane past the first block and a half", 3, 3, 3, 3, 86, 2, "bs1", "slice_lo"),
    TCase("second-pass", "n = 1 049 728 > 4096 * 256, % 256 != 0: a partial second pass", 1, 2, 16, 8, 32804, 4, "contig", "contig"),
]


def tokenize_operands(c):
    seed = sum(map(ord, c.name))
    return dict(x=seeded_randn(c.B, c.Cin, c.H, c.W, seed=7700 + seed), w=seeded_randn(c.C, c.Cin, 1, c.P, seed=7701 + seed),
                pe=seeded_randn(c.C, c.H, c.W // c.P, seed=7702 + seed))


def tokenize_fwd(t, c, dtype):
    """-> (y, S): Conv2d(Cin -> C, kernel = stride = (1, P), no bias)(x) + pe."""
    x, w, pe = (t[n].to(dtype) for n in ("x", "w", "pe"))
    return F.conv2d(x, w, stride=(1, c.P)) + pe[None], F.conv2d(x.abs(), w.abs(), stride=(1, c.P)) + pe.abs()[None]


def tokenize_naive(t, c):
    """The same by a loop over the Cin P products, float64."""
    x, w, pe = (t[n].double() for n in ("x", "w", "pe"))
    y = pe[None].repeat(c.B, 1, 1, 1)
    for ci in range(c.Cin):
        for p in range(c.P):
            y = y + w[None, :, ci, 0, p, None, None] * x[:, None, ci, :, p::c.P]
    return y


TRef = collections.namedtuple("TRef", "t y S e32 bound")


@functools.lru_cache(maxsize=None)
def tokenize_ref(c):
    t = tokenize_operands(c)
    y, S = tokenize_fwd(t, c, torch.float64)
    e32 = elem_err(tokenize_fwd(t, c, torch.float32)[0], y, S)
    return TRef(t, y, S, e32, bound(T_FWD, e32))


FCase = collections.namedtuple("FCase", "name edge M half")
FOURIER = [FCase("n1", "M half = 1", 1, 1), FCase("n255", "M half = 255: one short block", 5, 51),
           FCase("n256-full", "M half = 256: exactly one block", 4, 64), FCase("n257", "M half = 257: one live lane in the second block", 1, 257)]
FOURIER_T = (-15.0, -3.3, 0.0, 7.25, 15.0)


def fourier_operands(c):
    return torch.tensor(FOURIER_T[-c.M:], dtype=torch.float32), seeded_randn(c.half, seed=7800 + sum(map(ord, c.name)))


def fourier_fwd(t, fr, dtype):
    """[cos | sin] of the float32 arguments t (2 pi freqs), rounded as torch rounds them, evaluated in `dtype`."""
    a = (t[:, None] * (2 * math.pi * fr)[None]).to(dtype)
    return torch.cat([a.cos(), a.sin()], 1)


FRef = collections.namedtuple("FRef", "t fr y e32 bound")


@functools.lru_cache(maxsize=None)
def fourier_ref(c):
    t, fr = fourier_operands(c)
    y = fourier_fwd(t, fr, torch.float64)
    e32 = elem_err(fourier_fwd(t, fr, torch.float32), y, torch.ones_like(y))
    return FRef(t, fr, y, e32, bound(T_FOURIER, e32))


TABLES = dict(rmsnorm=RMS, geglu=GEGLU, qk_prep=QK, na=NA, permute=PERMUTES, lerp=LERP, tokenize=TOKENIZE, fourier=FOURIER)
