"""Case tables, float64 references, float32 oracles and bounds of the skinny dense-layer edge tests
(tests/test_skinny_edges.py on the GPU, tests/test_skinny_edges_host.py on the CPU): one place, so the two files cannot
drift apart.  No GPU code here.

The kernels: csrc/layout_gen.hip (sk_gemm_kernel + sk_combine_kernel, sk_rowprep_kernel, sk_pool_kernel,
sk_time_embed_kernel) through lidarcrafter_amd.ops_skinny, the path the layout denoiser and the PointNet heads use.  The
GEMM tile is SK_BM x SK_BN = 32 x 64, K is staged SK_KS = 32 at a time and summed in chunks of SK_KC = 128; whether a row
takes the K split is asked of the library (lc_skinny_parts), never restated here.

Skinny linear, two tiers per row.
  exact     x, w, bias, vec, res are integers in [-7, 7] stored as float32.  With K <= 2048 every partial sum is an integer
            below 2^24, so every summation order gives the same float32: the kernel equals the int64 evaluation of
            act(x w^T + bias) + vec[idx] + res BIT FOR BIT, element for element.  A wrong, missing or doubled index cannot
            hide; there is no tolerance.  (GEGLU is left out: erff is not exact.)
  rounding  seeded_randn operands (w / sqrt(K)).  Per element e = |got - ref64| / S, S the float64 sum of the absolute terms
            of the element as the kernel forms it: sum |x_k w_k| + |bias| + |vec| + |res|; for GEGLU the product part is
            S_a |gelu(g)| + |a| 1.13 S_g (1.13 >= sup |gelu'|; S_a, S_g the sums of the two halves with their bias).
            Bound: max(TOL_SKINNY, MARGIN x the float32 torch oracle's worst element on the same row); the oracle is at
            most ORACLE_CAP = 8 floors on every row (asserted in the host file).
Every operand segment is a column range of a tensor whose other columns (and spare rows) hold NaN, so an element read one
column or one row off poisons the output instead of passing as noise.

Rowprep.  Per (row, group) rel-L2 against float64 F.group_norm (+ SiLU) under the rule of tests/_gn_structured.py:
max(TOL_SKINNY, MARGIN x the float32 torch oracle's worst group on the row).  G = 0 without SiLU: bit-equal to the gathered
input.  A constant group (a constant row, or one channel per group) has (x - mean) = 0 exactly, so y = silu?(beta) in closed
form, held per element under GS.constant_bound's rule with rstd = eps^(-1/2) (const_bound; through SiLU, whose slope is at
most 1.1 and whose own evaluation is a few roundings: 1.1 x that + 4 ulp |silu(beta)|).

Pool.  Bit-equal to two sequential float32 scatter_add calls divided by the clamped count.
Time embedding.  Per element |got - cos / sin in float64 of the float32 product t f| <= max(TOL_SKINNY, MARGIN x the worst
element of torch's float32 cos / sin on the same operands).

A designed defect (DEFECTS), applied to the reference and not to the library, moves some element of every row it applies
to by at least SIGNAL_OVER_BOUND = 16 bounds: the host file asserts it."""
import collections
import functools

import torch
import torch.nn.functional as F

from lidarcrafter_amd.testing import seeded_randn
from tests import _gn_structured as GS
from tests._profile_cases import TOL_SKINNY                               # no new tolerance
from tests._train_edges import GUARD, MARGIN, SIGNAL_OVER_BOUND, guarded  # noqa: F401

ORACLE_CAP = 8.0         # the float32 oracle's worst figure is at most 8 floors on every rounding-tier linear row
SK_BM, SK_BN, SK_KS, SK_KC = 32, 64, 32, 128
EXACT_LIMIT = 2 ** 24
GELU_SLOPE = 1.13        # >= sup |gelu'| = 1.1289...
EPS = 1e-5               # the denoiser's GroupNorm / LayerNorm epsilon
VEC_ROWS, VEC_C0, RES_C0 = 3, 2, 8
NAN = float("nan")
DEFECTS = ("drop-last-k", "seam", "no-idx", "gate-at-n", "gate-bias", "vec-row0", "res-c0", "one-pass", "prev-group",
           "pool-s-col")


def lib_parts(M, N, K):
    from lidarcrafter_amd import ops_skinny

    return ops_skinny.skinny_parts(M, N, K)


def nchunks(K):
    return (K + SK_KC - 1) // SK_KC


def _ints(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-7, 8, tuple(shape), generator=g).float()


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100000


def make_idx(kind, M, j, seed):
    """"perm": a permutation of the rows; "rep": every row one of (at most) five, so rows repeat."""
    if kind == "perm":
        return torch.randperm(M, generator=torch.Generator(device="cpu").manual_seed(seed + 40 + j)).to(torch.int32)
    assert kind == "rep"
    return ((7 * torch.arange(M) + 3 + j) % min(M, 5)).to(torch.int32)


def make_sources(segs, M, pad, draw):
    """{name: [M + 2, cols] float32}: the columns some segment covers hold values, every other column, `pad` columns past
    the last one and the two spare rows hold NaN."""
    out = {}
    for name in dict.fromkeys(s.src for s in segs):
        mine = [s for s in segs if s.src == name]
        cols = max(s.c0 + s.w for s in mine) + pad
        t = draw(M + 2, cols, i=20 + len(out))
        keep = torch.zeros(cols, dtype=torch.bool)
        for s in mine:
            keep[s.c0:s.c0 + s.w] = True
        t[:, ~keep] = NAN
        t[M:] = NAN
        out[name] = t
    return out


def gather_x(src, idx, segs, M, no_idx=None):
    """The gathered concatenation [M, K] (float32); `no_idx`: the segment whose index is ignored (the defect)."""
    cols = []
    for j, s in enumerate(segs):
        rows = idx[j].long() if (s.idx and j != no_idx) else torch.arange(M)
        cols.append(src[s.src][rows][:, s.c0:s.c0 + s.w])
    return torch.cat(cols, 1)


# ------------------------------------------------------------------------------------------------ skinny linear
Seg = collections.namedtuple("Seg", "src c0 w idx")
LCase = collections.namedtuple("LCase", "name edge M N segs act bias vec res out pad tiers")
BOTH, EXACT, ROUND = ("exact", "round"), ("exact",), ("round",)


def L_(name, edge, M, N, segs, act=None, bias=True, vec=None, res=False, out="contig", pad=0, tiers=None):
    """segs: K (one plain segment) or a tuple of Seg.  vec: None | "idx" (a row index per row) | "row0" (idx=None: row 0 for
    every row).  out: "contig" | "pad" (y_ld = No + 5) | "inplace" (input columns [0, K) and output columns [K, K + No) of
    one tensor).  pad: NaN columns past the last segment of every source (ld > c0 + width)."""
    if isinstance(segs, int):
        segs = (Seg("a", 0, segs, None),)
    return LCase(name, edge, M, N, tuple(segs), act, bias, vec, res, out, pad, tiers or (ROUND if act == "geglu" else BOTH))


def _three(widths, c0s, idxs, srcs="abc"):
    return tuple(Seg(srcs[j], c0s[j], widths[j], idxs[j]) for j in range(3))


_K_EDGE = {
    1: "K = 1: one live k of the first slab", 31: "K = 31: the first slab one short", 32: "K = 32: exactly one slab",
    127: "K = 127: the fourth slab one short", 128: "K = 128: exactly one chunk",
    129: "K = 129: a second chunk of ONE element (a slab filled by one k above the first)",
    160: "K = 160: one full chunk plus one slab, so k0 >= K breaks inside the second chunk",
    257: "K = 257: two chunks plus one element", 385: "K = 385: three chunks plus one element",
}
_EPI = [("bias", dict(bias=True)), ("vec-idx", dict(bias=False, vec="idx")), ("vec-row0", dict(bias=False, vec="row0")),
        ("res", dict(bias=False, res=True)), ("all", dict(bias=True, vec="idx", res=True))]
LIN_CASES = (
    [L_("base", "M = 33, N = 65, K = 33: a second row tile, column tile and slab of one element each", 33, 65, 33)] +
    [L_(f"m{m}", f"M = {m} at N = 65, K = 33", m, 65, 33) for m in (1, 31, 32, 65)] +
    [L_(f"n{n}", f"N = {n} at M = 33, K = 33", 33, n, 33) for n in (1, 63, 64, 129)] +
    [L_(f"k{k}", e, 33, 65, k) for k, e in _K_EDGE.items()] +
    [
        L_("seg-5-30-7-g0", "seams at 5 and 35 inside slabs 0 and 1; a repeating index on segment 0, c0 > 0 and ld > width there",
           33, 65, _three((5, 30, 7), (3, 0, 0), ("rep", None, None)), pad=2),
        L_("seg-5-30-7-g1", "a permutation index on segment 1, c0 > 0 there", 33, 65, _three((5, 30, 7), (0, 4, 0), (None, "perm", None)),
           pad=1),
        L_("seg-5-30-7-g2", "a repeating index on segment 2, c0 > 0 there", 33, 65, _three((5, 30, 7), (0, 0, 2), (None, None, "rep")),
           pad=3),
        L_("seg-5-30-7-gall", "an index on all three segments; segments 0 and 2 drawn from the same tensor ([obj[s] | pred | obj[o]])",
           33, 65, _three((5, 30, 7), (1, 2, 9), ("rep", "perm", "perm"), srcs="aba"), pad=2),
        L_("seg-33-1-94", "widths (33, 1, 94): K = 128, a one-column segment right behind a slab edge, every c0 > 0, no index",
           33, 65, _three((33, 1, 94), (2, 5, 1), (None, None, None)), pad=1),
        L_("seg-33-1-94-gall", "the same seams with an index on every segment (the one-column segment gathered)", 33, 65,
           _three((33, 1, 94), (2, 5, 1), ("perm", "rep", "perm")), pad=1),
        L_("seg-1-1-1", "widths (1, 1, 1): K = 3, every k a segment of its own, all gathered", 33, 65,
           _three((1, 1, 1), (4, 0, 2), ("perm", "rep", "perm")), pad=2),
        L_("seg2-20-13", "two segments, the index on segment 1 only", 33, 65, (Seg("a", 0, 20, None), Seg("b", 3, 13, "perm")), pad=1),
        L_("seg-k257-gall", "three gathered segments over three chunks (100 | 57 | 100): the K split with seams inside slabs", 33, 65,
           _three((100, 57, 100), (1, 0, 3), ("perm", "rep", "perm"), srcs="aba"), pad=1),
    ] +
    [L_(f"epi-{n}-{a or 'none'}", f"epilogue: {n} alone" if n != "all" else "epilogue: bias, vec with idx and res together", 33, 65, 33,
        act=a, **kw) for a in (None, "relu") for n, kw in _EPI] +
    [
        L_("geglu-n2", "GEGLU at N = 2, No = 1: the gate is column 1", 33, 2, 33, act="geglu", vec="idx", res=True),
        L_("geglu-n66", "GEGLU at N = 66, No = 33: the gate of column 32 sits in the next column tile's threads", 33, 66, 33, act="geglu",
           vec="idx", res=True),
        L_("geglu-n130", "GEGLU at N = 130, No = 65 (odd), K = 160: two chunks", 33, 130, 160, act="geglu", vec="idx", res=True),
        L_("geglu-gathered", "GEGLU over three gathered segments, seams (5, 30, 7), out with y_ld > No", 33, 66,
           _three((5, 30, 7), (1, 2, 9), ("rep", "perm", "perm"), srcs="aba"), act="geglu", vec="row0", res=True, out="pad", pad=2),
        L_("out-pad", "out a column slice of a wider tensor (y_ld = No + 5), the other columns NaN guards", 33, 65, 33, act="relu",
           vec="idx", res=True, out="pad"),
        L_("out-inplace", "PointNet's form: input columns [0, K), output columns [K, K + N) of ONE tensor, vec = (eye, 0, None)", 33, 65,
           160, act="relu", vec="row0", out="inplace"),
        L_("grid-stride", "M = 2049, K = 8, N = 512: 1 049 088 outputs against the 1 048 576 of 4096 blocks; the last 512 come from "
           "the second trip of the combine's loop", 2049, 512, 8, act="relu", vec="idx", res=True, tiers=EXACT),
    ])


LIN_RUNS = [(c, tier) for c in LIN_CASES for tier in c.tiers]     # GEGLU: no exact tier (erff); grid-stride: exact only


def lin_K(c):
    return sum(s.w for s in c.segs)


def lin_No(c):
    return c.N // 2 if c.act == "geglu" else c.N


def lin_operands(c, tier):
    """-> dict: src {name: tensor}, idx [per segment: int32 or None], w [N, K], bias [N], vec [3, No + 2], vidx [M],
    res [M, No + 9] (float32 / int32, CPU)."""
    seed = 11000 + _seed(c.name) + (0 if tier == "exact" else 50000)
    K, No = lin_K(c), lin_No(c)
    if tier == "exact":
        draw = lambda *shape, i: _ints(shape, seed + i)
    else:
        draw = lambda *shape, i: seeded_randn(*shape, seed=seed + i)
    t = dict(src=make_sources(c.segs, c.M, c.pad, draw),
             idx=[make_idx(s.idx, c.M, j, seed) if s.idx else None for j, s in enumerate(c.segs)])
    w = draw(c.N, K, i=1)
    t["w"] = w if tier == "exact" else w / K ** 0.5
    t["bias"], t["vec"], t["res"] = draw(c.N, i=2), draw(VEC_ROWS, No + VEC_C0, i=3), draw(c.M, No + RES_C0 + 1, i=4)
    t["vidx"] = ((2 * torch.arange(c.M) + 1) % VEC_ROWS).to(torch.int32)
    return t


def lin_closed(t, c, dtype, defect=None, seg=None):
    """(y [M, No], S [M, No]) of act(x w^T + bias) + vec[row] + res in `dtype`, written as the kernel forms it; S the sum
    of the absolute terms (see the module docstring).  `defect`: one of DEFECTS (`seg`: the segment "no-idx" ignores)."""
    x = gather_x(t["src"], t["idx"], c.segs, c.M, no_idx=seg if defect == "no-idx" else None).to(dtype)
    if defect == "seam":                                        # the first element of segment 1 read from segment 0's last
        x = x.clone()
        x[:, c.segs[0].w] = x[:, c.segs[0].w - 1]
    if defect == "drop-last-k":
        x = x.clone()
        x[:, -1] = 0
    w = t["w"].to(dtype)
    b = t["bias"].to(dtype) if c.bias else torch.zeros(c.N, dtype=dtype)
    z = x @ w.t() + b
    S = x.abs() @ w.abs().t() + b.abs()
    No = lin_No(c)
    if c.act == "relu":
        y = z.clamp_min(0)
    elif c.act == "geglu":
        a, g = z[:, :No], z[:, No:]
        if defect == "gate-at-n":
            g = a
        if defect == "gate-bias":
            g = g - b[No:]
        gl = F.gelu(g)
        y, S = a * gl, S[:, :No] * gl.abs() + a.abs() * GELU_SLOPE * S[:, No:]
    else:
        y = z
    if c.vec:
        rows = t["vidx"].long() if (c.vec == "idx" and defect != "vec-row0") else torch.zeros(c.M, dtype=torch.long)
        v = t["vec"][rows][:, VEC_C0:VEC_C0 + No].to(dtype)
        y, S = y + v, S + v.abs()
    if c.res:
        c0 = 0 if defect == "res-c0" else RES_C0
        r = t["res"][:, c0:c0 + No].to(dtype)
        y, S = y + r, S + r.abs()
    return y, S


def lin_defects(c):
    """[(defect, segment or None)] that apply to a row."""
    K, out = lin_K(c), []
    if K % SK_KS:
        out.append(("drop-last-k", None))
    if len(c.segs) > 1:
        out.append(("seam", None))
    out += [("no-idx", j) for j, s in enumerate(c.segs) if s.idx]
    if c.act == "geglu":
        out.append(("gate-at-n", None))
        if c.bias:
            out.append(("gate-bias", None))
    if c.vec == "idx":
        out.append(("vec-row0", None))
    if c.res:
        out.append(("res-c0", None))
    return out


def elem_err(got, ref64, S):
    """worst |got - ref64| / S over the elements (a NaN anywhere gives inf)."""
    e = (got.detach().cpu().double().reshape(ref64.shape) - ref64).abs() / S
    return float("inf") if bool(torch.isnan(e).any()) else float(e.max())


LRef = collections.namedtuple("LRef", "t y S e32 bound")


@functools.lru_cache(maxsize=None)
def lin_ref(c, tier):
    """exact: y the int64 evaluation (as float32: exact below 2^24), S the int64 sum of the absolute terms, no bound.
    round: y, S in float64, e32 the float32 oracle's worst element, bound = max(TOL_SKINNY, MARGIN e32)."""
    t = lin_operands(c, tier)
    if tier == "exact":
        y, S = lin_closed(t, c, torch.int64)
        return LRef(t, y, S, 0.0, 0.0)
    y, S = lin_closed(t, c, torch.float64)
    assert float(S.min()) > 0
    e32 = elem_err(lin_closed(t, c, torch.float32)[0], y, S)
    assert e32 == e32 and e32 < float("inf"), "the float32 oracle is not finite"
    return LRef(t, y, S, e32, max(TOL_SKINNY, MARGIN * e32))


# ------------------------------------------------------------------------------------------------ rowprep
RCase = collections.namedtuple("RCase", "name edge M segs G silu affine data pad")


def R_(name, edge, M, segs, G, silu=True, affine=True, data="rand", pad=0):
    """segs: C (one plain segment at c0 = 0) or a tuple of Seg.  data: "rand" (3 randn + 1) | "const3" | "const1000" (every
    value of the row that level) | "common" (1000 + randn).  pad: NaN columns past the row in `out` (y_ld = C + pad)."""
    if isinstance(segs, int):
        segs = (Seg("a", 0, segs, None),)
    return RCase(name, edge, M, tuple(segs), G, silu, affine and G > 0, data, pad)


def _two(widths, idxs):
    return (Seg("a", 2, widths[0], idxs[0]), Seg("b", 1, widths[1], idxs[1]))


ROW_CASES = (
    [R_(f"g0-c{C}", f"no normalisation, C = {C}: the copy loop's tail at 256 threads", 5, C, 0, silu=False) for C in (1, 255, 256, 257)] +
    [R_("g0-c257-silu", "no normalisation, SiLU alone, C = 257", 5, 257, 0), R_("g0-c1-silu", "SiLU alone on one column", 1, 1, 0)] +
    [R_(f"ln-c{C}", f"LayerNorm (G = 1), C = {C}" + (": the LDS row limit" if C == 4096 else ": the lane loop's tail"), 5, C, 1,
        silu=(C != 64)) for C in (63, 64, 65, 4096)] +
    [R_(f"g{G}-cs{cs}", f"G = {G} (one wave takes two groups, another one), group width {cs}" + (": every group constant, y = beta"
                                                                                                  if cs == 1 else ""),
        5, G * cs, G, silu=(G == 3)) for G in (3, 5) for cs in (1, 63, 64, 65)] +
    [
        R_("g32-cs16", "G = 32 at cs = 16: every wave takes eight groups, 48 idle lanes", 5, 512, 32),
        R_("const3", "a constant row at 3.0, cs = 64: y = silu(beta) in closed form", 5, 192, 3, data="const3"),
        R_("const1000", "a constant row at 1000.0, cs = 64, no SiLU: y = beta", 5, 192, 3, silu=False, data="const1000"),
        R_("common-cs64", "1000 + N(0, 1) at cs = 64: a one-pass variance is off by orders of magnitude", 5, 192, 3, data="common"),
        R_("common-cs512", "1000 + N(0, 1) at cs = 512: eight values per lane", 5, 1024, 2, silu=False, data="common"),
        R_("gather-5-59-g0", "two segments, seam at 5, a repeating index on segment 0", 5, _two((5, 59), ("rep", None)), 4),
        R_("gather-5-59-g1", "two segments, seam at 5, a permutation index on segment 1", 5, _two((5, 59), (None, "perm")), 4, silu=False),
        R_("gather-130-126-g0", "two segments, seam at 130, a permutation index on segment 0", 5, _two((130, 126), ("perm", None)), 4,
           silu=False),
        R_("gather-130-126-g1", "two segments, seam at 130, a repeating index on segment 1", 5, _two((130, 126), (None, "rep")), 4),
        R_("gather-g0", "no normalisation of a gathered concatenation (obj0 of the denoiser): bit-equal", 5, _two((5, 59), ("perm", "rep")),
           0, silu=False),
        R_("no-affine", "gamma and beta both None with G > 0", 5, 195, 3, affine=False),
        R_("out-strided", "out a column slice of a wider tensor (y_ld = C + 3) between NaN guards", 5, 195, 3, pad=3),
        R_("m1", "M = 1: one block", 1, 195, 3),
    ])
ROW_REFUSED = [("c4097", 4097, 1, "C = 4097: past the LDS row"), ("c-mod-g", 64, 3, "C % G != 0")]


def row_C(c):
    return sum(s.w for s in c.segs)


def row_operands(c):
    """-> dict src, idx (as make_sources / make_idx), gamma, beta [C] or None (float32, CPU)."""
    seed = 12000 + _seed(c.name)
    C = row_C(c)
    if c.data == "rand":
        draw = lambda *shape, i: seeded_randn(*shape, seed=seed + i) * 3 + 1
    elif c.data == "common":
        draw = lambda *shape, i: seeded_randn(*shape, seed=seed + i) + 1000.0
    else:
        draw = lambda *shape, i: torch.full(shape, float(c.data[5:]))
    t = dict(src=make_sources(c.segs, c.M, 2, draw), idx=[make_idx(s.idx, c.M, j, seed) if s.idx else None for j, s in enumerate(c.segs)])
    t["gamma"] = 1 + 0.2 * seeded_randn(C, seed=seed + 2) if c.affine else None
    t["beta"] = 0.3 * seeded_randn(C, seed=seed + 3) if c.affine else None
    return t


def row_x(t, c, no_idx=None):
    return gather_x(t["src"], t["idx"], c.segs, c.M, no_idx=no_idx)


def row_torch(x, c, t, dtype):
    """The plain torch formula: F.group_norm (+ F.silu) in `dtype`."""
    y = x.to(dtype)
    if c.G:
        p = lambda k: None if t[k] is None else t[k].to(dtype)
        y = F.group_norm(y[:, :, None], c.G, p("gamma"), p("beta"), EPS)[:, :, 0]
    return F.silu(y) if c.silu else y


def row_closed(x, c, t, dtype, defect=None):
    """The same written out.  defect "one-pass": var = E[x^2] - mean^2; "prev-group": the statistics of group g - 1."""
    y = x.to(dtype)
    if c.G:
        v = y.reshape(c.M, c.G, -1)
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
        if defect == "one-pass":
            var = (v * v).mean(-1, keepdim=True) - mean * mean
        if defect == "prev-group":
            mean, var = mean.roll(1, 1), var.roll(1, 1)
        y = ((v - mean) / (var + EPS).sqrt()).reshape(c.M, -1)
        if t["gamma"] is not None:
            y = y * t["gamma"].to(dtype) + t["beta"].to(dtype)
    return y * torch.sigmoid(y) if c.silu else y


def row_group_err(got, ref64, c):
    """rel-L2 per (row, group) -> [M, max(G, 1)]; a NaN counts as inf."""
    e = GS.group_err(got, ref64, max(c.G, 1))
    return torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)


def const_bound(level, ga, be, eps=EPS, ulp=GS.F32_ULP):
    """GS.constant_bound's rule with rstd = eps^(-1/2) and no scale / shift: one rounding of the mean times rstd, with a
    factor 2, plus 4 ulp of beta.  Tensors [..., C] in float64."""
    return eps ** -0.5 * ulp * level.abs() * ga.abs() + 4.0 * ulp * be.abs()


def row_const(c, t, x):
    """For a row whose groups are all constant (a constant row, cs = 1): (closed form silu?(beta) [M, C], bound [M, C])."""
    C = row_C(c)
    ga = t["gamma"].double() if t["gamma"] is not None else torch.ones(C, dtype=torch.float64)
    be = t["beta"].double() if t["beta"] is not None else torch.zeros(C, dtype=torch.float64)
    b = const_bound(x.double(), ga[None], be[None])
    y = be[None].expand(c.M, C)
    if c.silu:
        y = y * torch.sigmoid(y)
        b = 1.1 * b + 4.0 * GS.F32_ULP * y.abs()
    return y, b


def row_is_const(c):
    return c.G > 0 and (c.data.startswith("const") or row_C(c) == c.G)


RRef = collections.namedtuple("RRef", "t x y e32 bound")


@functools.lru_cache(maxsize=None)
def row_ref(c):
    t = row_operands(c)
    x = row_x(t, c)
    y = row_torch(x, c, t, torch.float64)
    # (constant groups are held to the closed form alone: torch's float32 group_norm does not keep (x - mean) at exactly 0
    #  there -- it is off by 3e-4 at one channel per group and by 3e-2 on the row at 1000.0 -- so it is no yardstick)
    e32 = 0.0 if row_is_const(c) else float(row_group_err(row_torch(x, c, t, torch.float32), y, c).max())
    assert e32 < float("inf"), "the float32 oracle is not finite"
    return RRef(t, x, y, e32, max(TOL_SKINNY, MARGIN * e32))


# ------------------------------------------------------------------------------------------------ pool
PCase = collections.namedtuple("PCase", "name edge O H s_col o_col extra pad")
POOL_T = 45


def P_(name, edge, O, H, s_col=0, o_col=None, extra=0, pad=0):
    return PCase(name, edge, O, H, s_col, H if o_col is None else o_col, extra, pad)


POOL_CASES = (
    [P_(f"h{H}", f"H = {H}" + {1: ": one live thread", 255: ": the block stride one short", 256: ": one block stride exactly",
                                257: ": a second trip of one column", 600: ": three trips, the last short"}[H], 6, H)
     for H in (1, 255, 256, 257, 600)] +
    [
        P_("o1", "O = 1: every triple is a self loop of the only object (90 slots)", 1, 257),
        P_("overlap", "s_col and o_col ranges that overlap (o_col = s_col + H / 2)", 6, 130, s_col=3, o_col=68),
        P_("t-ld", "t_ld > 2 H + gap: a gap between the halves and 7 columns behind them", 6, 65, s_col=2, o_col=80, extra=7),
        P_("out-strided", "out a column slice of a wider tensor (y_ld = H + 3) between NaN guards", 6, 257, pad=3),
    ])


def pool_triples(c):
    """(s, o) int64 [45].  O = 6: object 0 only ever a subject, object 1 only ever an object, object 2 in no triple (zeros),
    object 3 in 40 triples (20 as subject, 20 as object), objects 4 and 5 on both sides."""
    if c.O == 1:
        return torch.zeros(POOL_T, dtype=torch.long), torch.zeros(POOL_T, dtype=torch.long)
    i = torch.arange(20)
    s = torch.cat([torch.full((20,), 3), 4 + i % 2, torch.zeros(5, dtype=torch.long)])
    o = torch.cat([4 + (i // 2) % 2, torch.full((20,), 3), torch.ones(5, dtype=torch.long)])
    order = torch.randperm(POOL_T, generator=torch.Generator(device="cpu").manual_seed(7))
    return s[order], o[order]


def pool_operands(c):
    s, o = pool_triples(c)
    t = seeded_randn(POOL_T, max(c.s_col, c.o_col) + c.H + c.extra, seed=13000 + _seed(c.name))
    return t, s, o


def pool_ref(t, s, o, c, defect=None):
    """Two sequential float32 scatter_add calls divided by the clamped count.  defect "pool-s-col": the object slots read
    from s_col."""
    oc = c.s_col if defect == "pool-s-col" else c.o_col
    T = s.numel()
    y = torch.zeros(c.O, c.H).scatter_add(0, s.view(-1, 1).expand(T, c.H), t[:, c.s_col:c.s_col + c.H])
    y = y.scatter_add(0, o.view(-1, 1).expand(T, c.H), t[:, oc:oc + c.H])
    cnt = (torch.bincount(s, minlength=c.O) + torch.bincount(o, minlength=c.O)).clamp(min=1).float()
    return y / cnt.view(-1, 1)


# ------------------------------------------------------------------------------------------------ time embedding
TCase = collections.namedtuple("TCase", "name edge U half")
TIME_CASES = [
    TCase("u1-h1", "U = 1, half = 1: one live thread", 1, 1),
    TCase("u1-h255", "U = 1, half = 255 (odd): the block one thread short", 1, 255),
    TCase("u3-h85", "U half = 255 over three rows of an odd half: u = e / half at every row seam", 3, 85),
    TCase("u5-h256", "U half = 1280: five whole blocks", 5, 256),
    TCase("u7-h37", "U half = 259: a second block of three elements", 7, 37),
]
TIME_VALUES = [-15.0, 0.0, 15.0, 4.2, -0.3, 7.77, -11.1]          # the range of the log-SNR condition, 0 included


def time_operands(c):
    t = torch.tensor(TIME_VALUES[:c.U])
    f = torch.exp(-torch.log(torch.tensor(10000.0)) * torch.arange(c.half, dtype=torch.float32) / c.half)
    return t, f


TRef = collections.namedtuple("TRef", "t f y e32 bound")


@functools.lru_cache(maxsize=None)
def time_ref(c):
    t, f = time_operands(c)
    a = t[:, None] * f[None]                                      # the float32 product the kernel forms
    y = torch.cat([a.double().cos(), a.double().sin()], 1)
    e32 = float((torch.cat([a.cos(), a.sin()], 1).double() - y).abs().max())
    return TRef(t, f, y, e32, max(TOL_SKINNY, MARGIN * e32))
