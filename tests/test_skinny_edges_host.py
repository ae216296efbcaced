"""The case tables of tests/test_skinny_edges.py, and the proof that they are complete (CPU only).

Every value the tables are there for is present (the M, N, K, group-width and H classes against the tile constants of
csrc/layout_gen.hip, the position of the gather index, each epilogue option alone), lc_skinny_parts answers both ways over
the rows' default routes, the exact tier's partial sums stay below 2^24, the float64 references equal plain torch formulas,
every designed defect moves some element of every row it applies to by at least 16 bounds, and the float32 oracle stays
under 8 floors on every rounding-tier linear row."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import _gn_structured as GS
from tests import _skinny_edges as SE

ids = lambda c: c.name
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN_ROUND = [c for c in SE.LIN_CASES if "round" in c.tiers]
LIN_EXACT = [c for c in SE.LIN_CASES if "exact" in c.tiers]


def test_names_are_unique_and_every_row_names_its_edge():
    for table in (SE.LIN_CASES, SE.ROW_CASES, SE.POOL_CASES, SE.TIME_CASES):
        assert len({c.name for c in table}) == len(table)
        assert all(c.edge for c in table)
    assert all(e for *_, e in SE.ROW_REFUSED)


def test_the_tile_constants_are_the_kernel_s():
    src = open(os.path.join(ROOT, "lidarcrafter_amd", "csrc", "layout_gen.hip")).read()
    for name in ("SK_BM", "SK_BN", "SK_KS", "SK_KC"):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == getattr(SE, name)
    assert "blocks > 4096" in src and "row[4096]" in src and SE.ORACLE_CAP == 8.0


# ------------------------------------------------------------------------------------------------ the tables
def test_linear_table_covers_every_edge():
    plain = [c for c in SE.LIN_CASES if len(c.segs) == 1 and c.out == "contig" and c.act is None and not c.vec and not c.res]
    shape = lambda c: (c.M, c.N, SE.lin_K(c))
    assert {c.M for c in plain if shape(c)[1:] == (65, 33)} >= {1, 31, 32, 33, 65}
    assert {c.N for c in plain if (c.M, SE.lin_K(c)) == (33, 33)} >= {1, 63, 64, 65, 129}
    assert {SE.lin_K(c) for c in plain if (c.M, c.N) == (33, 65)} >= {1, 31, 32, 33, 127, 128, 129, 160, 257, 385}
    assert {c.M % SE.SK_BM for c in plain} >= {0, 1, 31} and {c.N % SE.SK_BN for c in plain} >= {0, 1, 63}
    assert {SE.lin_K(c) % SE.SK_KS for c in plain} >= {0, 1, 31} and {SE.lin_K(c) % SE.SK_KC for c in plain} >= {0, 1, 31, 32, 127}
    assert max(SE.lin_K(c) for c in SE.LIN_CASES) <= 2048
    # a K slab partly filled above the first, a chunk partly filled, k0 >= K inside a chunk
    assert any(SE.lin_K(c) > SE.SK_KS and SE.lin_K(c) % SE.SK_KS for c in plain)
    assert any(SE.lin_K(c) > SE.SK_KC and 0 < SE.lin_K(c) % SE.SK_KC <= SE.SK_KC - SE.SK_KS for c in plain)
    # segments: the widths, the position of the gather index, c0 and ld on every position, both index kinds, a shared tensor
    three = [c for c in SE.LIN_CASES if len(c.segs) == 3]
    assert {tuple(s.w for s in c.segs) for c in three} >= {(5, 30, 7), (33, 1, 94), (1, 1, 1)}
    where = {tuple(j for j, s in enumerate(c.segs) if s.idx) for c in three if tuple(s.w for s in c.segs) == (5, 30, 7)}
    assert where >= {(0,), (1,), (2,), (0, 1, 2)}
    for j in range(3):
        assert any(c.segs[j].c0 > 0 and c.pad > 0 for c in three)
        assert any(s.w % SE.SK_KS for c in three for s in c.segs[:j + 1])
    assert {s.idx for c in SE.LIN_CASES for s in c.segs} == {None, "rep", "perm"}
    assert any(c.segs[0].src == c.segs[2].src for c in three)
    assert any(len(c.segs) == 2 and not c.segs[0].idx and c.segs[1].idx for c in SE.LIN_CASES)
    # a seam inside a 32-wide K slab
    assert any(c.segs[0].w % SE.SK_KS and (c.segs[0].w + c.segs[1].w) % SE.SK_KS for c in three)
    # every epilogue option alone and all together, for act none and relu
    epi = {(c.act, c.bias, c.vec, c.res) for c in SE.LIN_CASES if len(c.segs) == 1 and c.out == "contig"}
    for act in (None, "relu"):
        assert epi >= {(act, True, None, False), (act, False, "idx", False), (act, False, "row0", False), (act, False, None, True),
                       (act, True, "idx", True)}
    # GEGLU with bias, vec and res at N = 2, 66, 130 and over gathered segments; never in the exact tier
    geglu = [c for c in SE.LIN_CASES if c.act == "geglu"]
    assert {c.N for c in geglu if c.bias and c.vec and c.res} >= {2, 66, 130} and all(c.tiers == SE.ROUND for c in geglu)
    assert any(len(c.segs) == 3 and all(s.idx for s in c.segs) and tuple(s.w for s in c.segs) == (5, 30, 7) for c in geglu)
    assert any(SE.lin_No(c) % 2 for c in geglu) and any(SE.lin_No(c) == 33 for c in geglu)
    assert {c.out for c in SE.LIN_CASES} == {"contig", "pad", "inplace"}
    # the grid-stride row: the last 512 outputs come from the second trip; every element held (exact tier only)
    g = next(c for c in SE.LIN_CASES if c.name == "grid-stride")
    assert (g.M, SE.lin_K(g), g.N) == (2049, 8, 512) and g.M * g.N - 4096 * 256 == 512 and g.tiers == SE.EXACT
    assert all(c.M * c.N <= 4096 * 256 for c in SE.LIN_CASES if c is not g)
    assert all(c.M > 1 for c in SE.LIN_CASES if c.vec == "idx" or any(s.idx for s in c.segs))


def test_both_answers_of_lc_skinny_parts_occur():
    routes = {}
    for c in SE.LIN_CASES:
        K = SE.lin_K(c)
        routes[c.name] = (SE.lib_parts(c.M, c.N, K), SE.nchunks(K))
        assert routes[c.name][0] in (1, routes[c.name][1]), c.name
    assert {r for r, _ in routes.values()} >= {1, 2, 3, 4}
    assert routes["k128"] == (1, 1) and routes["k129"] == (2, 2) and routes["k160"] == (2, 2) and routes["k385"] == (4, 4)
    assert routes["geglu-n130"][0] == 2 and routes["out-inplace"][0] == 2 and routes["seg-k257-gall"][0] == 3


def test_rowprep_pool_and_time_tables_cover_every_edge():
    rows = {c.name: c for c in SE.ROW_CASES}
    C, cs = SE.row_C, lambda c: SE.row_C(c) // c.G
    assert {C(c) for c in SE.ROW_CASES if c.G == 0 and not c.silu} >= {1, 255, 256, 257} and any(c.G == 0 and c.silu for c in SE.ROW_CASES)
    assert {C(c) for c in SE.ROW_CASES if c.G == 1} >= {63, 64, 65, 4096}
    for G in (3, 5):
        assert {cs(c) for c in SE.ROW_CASES if c.G == G and c.data == "rand"} >= {1, 63, 64, 65}
    assert {cs(c) % 64 for c in SE.ROW_CASES if c.G} >= {0, 1, 63, 16} and {c.G % 4 for c in SE.ROW_CASES if c.G} >= {0, 1, 2, 3}
    assert (rows["g32-cs16"].G, cs(rows["g32-cs16"])) == (32, 16)
    assert (rows["const3"].data, cs(rows["const3"]), rows["const1000"].data, cs(rows["const1000"])) == ("const3", 64, "const1000", 64)
    assert {cs(c) for c in SE.ROW_CASES if c.data == "common"} == {64, 512}
    seams = {(tuple(s.w for s in c.segs), tuple(j for j, s in enumerate(c.segs) if s.idx)) for c in SE.ROW_CASES if c.G and len(c.segs) == 2}
    assert seams >= {((5, 59), (0,)), ((5, 59), (1,)), ((130, 126), (0,)), ((130, 126), (1,))}
    assert any(c.G == 0 and any(s.idx for s in c.segs) for c in SE.ROW_CASES)
    assert any(c.G and not c.affine for c in SE.ROW_CASES) and any(c.pad for c in SE.ROW_CASES)
    assert {c.M for c in SE.ROW_CASES} == {1, 5} and {c.silu for c in SE.ROW_CASES if c.G} == {True, False}
    assert max(C(c) for c in SE.ROW_CASES) == 4096 and [r[1] for r in SE.ROW_REFUSED][0] == 4097
    assert all(c.M > 1 for c in SE.ROW_CASES if any(s.idx for s in c.segs))
    # pool
    assert {c.H for c in SE.POOL_CASES} >= {1, 255, 256, 257, 600} and {c.O for c in SE.POOL_CASES} == {1, 6}
    assert any(c.s_col < c.o_col < c.s_col + c.H for c in SE.POOL_CASES)
    assert any(c.extra and c.o_col > c.s_col + c.H for c in SE.POOL_CASES) and any(c.pad for c in SE.POOL_CASES)
    c = SE.POOL_CASES[0]
    s, o = SE.pool_triples(c)
    cnt_s, cnt_o = torch.bincount(s, minlength=6), torch.bincount(o, minlength=6)
    assert cnt_s[0] > 0 and cnt_o[0] == 0 and cnt_s[1] == 0 and cnt_o[1] > 0 and cnt_s[2] + cnt_o[2] == 0
    assert cnt_s[3] + cnt_o[3] == 40 and cnt_s[3] > 0 and cnt_o[3] > 0 and s.numel() == SE.POOL_T
    # time embedding
    assert {(c.U, c.half) for c in SE.TIME_CASES} == {(1, 1), (1, 255), (3, 85), (5, 256), (7, 37)}
    assert 0.0 in SE.TIME_VALUES[:3] and min(SE.TIME_VALUES) == -15.0 and max(SE.TIME_VALUES) == 15.0
    assert {c.U * c.half % 256 for c in SE.TIME_CASES} >= {0, 1, 3, 255}


# ------------------------------------------------------------------------------------------------ skinny linear
def _plain_linear(t, c, dtype):
    """cat -> F.linear -> act -> adds, written independently of SE.lin_closed."""
    cols = []
    for j, s in enumerate(c.segs):
        src = t["src"][s.src]
        rows = src[t["idx"][j].long()] if s.idx else src[:c.M]
        cols.append(rows[:, s.c0:s.c0 + s.w])
    z = F.linear(torch.cat(cols, 1).to(dtype), t["w"].to(dtype), t["bias"].to(dtype) if c.bias else None)
    if c.act == "relu":
        z = F.relu(z)
    if c.act == "geglu":
        a, g = z.chunk(2, dim=-1)
        z = a * F.gelu(g)
    No = z.shape[1]
    if c.vec == "idx":
        z = z + t["vec"].to(dtype)[t["vidx"].long(), SE.VEC_C0:SE.VEC_C0 + No]
    if c.vec == "row0":
        z = z + t["vec"].to(dtype)[0, SE.VEC_C0:SE.VEC_C0 + No]
    if c.res:
        z = z + t["res"].to(dtype)[:, SE.RES_C0:SE.RES_C0 + No]
    return z


@pytest.mark.parametrize("c", LIN_EXACT, ids=ids)
def test_exact_tier_stays_below_two_to_the_24(c):
    r = SE.lin_ref(c, "exact")
    t = r.t
    for a in [t["w"], t["bias"], t["vec"], t["res"]] + list(t["src"].values()):
        v = a[~torch.isnan(a)]
        assert bool((v == v.round()).all()) and float(v.abs().max()) <= 7
    assert r.y.dtype == torch.int64 and int(r.S.max()) < SE.EXACT_LIMIT and int(r.y.abs().max()) <= int(r.S.max())
    assert torch.equal(r.y.float().long(), r.y)
    # the int64 evaluation is the plain formula (float64 is exact on these integers too)
    assert torch.equal(_plain_linear(t, c, torch.float64), r.y.double())
    assert int((r.y != 0).sum()) > r.y.numel() // 3               # (ReLU leaves about half)


@pytest.mark.parametrize("c", LIN_ROUND, ids=ids)
def test_linear_references_oracle_cap_and_defects(c):
    r = SE.lin_ref(c, "round")
    assert r.y.dtype == torch.float64 and bool(torch.isfinite(r.y).all()) and float(r.S.min()) > 0
    assert SE.elem_err(_plain_linear(r.t, c, torch.float64), r.y, r.S) <= 1e-14
    # the float32 oracle: not exact, and under the cap (the two-term bound is not vacuous)
    assert 0 < r.e32 <= SE.ORACLE_CAP * SE.TOL_SKINNY, (c.name, r.e32)
    assert r.bound == max(SE.TOL_SKINNY, SE.MARGIN * r.e32)
    for defect, seg in SE.lin_defects(c):
        bad, _ = SE.lin_closed(r.t, c, torch.float64, defect=defect, seg=seg)
        assert SE.elem_err(bad, r.y, r.S) >= SE.SIGNAL_OVER_BOUND * r.bound, (c.name, defect, seg, SE.elem_err(bad, r.y, r.S), r.bound)


def test_every_linear_defect_applies_somewhere():
    seen = {d for c in LIN_ROUND for d, _ in SE.lin_defects(c)}
    assert seen == set(SE.DEFECTS[:7])
    assert {seg for c in LIN_ROUND for d, seg in SE.lin_defects(c) if d == "no-idx"} == {0, 1, 2}
    # a NaN column or row next to every segment: an off-by-one read poisons the output
    for c in SE.LIN_CASES:
        if c.pad:
            t = SE.lin_ref(c, c.tiers[0]).t
            assert all(bool(torch.isnan(a[:, -1]).all()) and bool(torch.isnan(a[c.M:]).all()) for a in t["src"].values())


# ------------------------------------------------------------------------------------------------ rowprep
@pytest.mark.parametrize("c", SE.ROW_CASES, ids=ids)
def test_rowprep_references_and_defects(c):
    r = SE.row_ref(c)
    assert bool(torch.isfinite(r.x).all()) and bool(torch.isfinite(r.y).all())
    closed = SE.row_closed(r.x, c, r.t, torch.float64)
    assert float(SE.row_group_err(closed, r.y, c).max()) <= 1e-9, c.name
    assert r.bound == max(SE.TOL_SKINNY, SE.MARGIN * r.e32) and r.bound <= 1e-3
    if c.G == 0 and not c.silu:
        assert torch.equal(r.y.float(), r.x)
    if SE.row_is_const(c):
        y, b = SE.row_const(c, r.t, r.x)
        # (F.group_norm in float64 leaves 3e-11 at level 1000: its mean is not exact, times rstd = 316)
        assert float((r.y - y).abs().max()) <= 1e-9 and float(b.max()) <= 0.1 and float(b.min()) >= 0     # (0.06 at level 1000)
    if c.data == "common":
        v = r.x.double().reshape(c.M, c.G, -1)
        assert float((v.mean(-1).abs() / v.std(-1)).min()) >= 800
        bad = SE.row_closed(r.x, c, r.t, torch.float32, defect="one-pass")
        assert float(SE.row_group_err(bad, r.y, c).max()) >= SE.SIGNAL_OVER_BOUND * r.bound, c.name
    if c.G >= 2 and not c.data.startswith("const"):
        bad = SE.row_closed(r.x, c, r.t, torch.float64, defect="prev-group")
        assert float(SE.row_group_err(bad, r.y, c).max()) >= SE.SIGNAL_OVER_BOUND * r.bound, c.name
    for j, s in enumerate(c.segs):
        if s.idx:                                                     # the gather index ignored on one segment
            bad = SE.row_torch(SE.row_x(r.t, c, no_idx=j), c, r.t, torch.float64)
            assert float(SE.row_group_err(bad, r.y, c).max()) >= SE.SIGNAL_OVER_BOUND * r.bound, (c.name, j)


def test_const_bound_is_the_rule_of_gn_structured():
    C = 4
    ga, be = torch.tensor([1.3, -0.7, 0.0, 2.0], dtype=torch.float64), torch.tensor([0.2, -0.4, 0.9, 0.0], dtype=torch.float64)
    ss = torch.zeros(1, 2 * C, dtype=torch.float64)
    for level in (3.0, 1000.0):
        b = SE.const_bound(torch.full((C,), level, dtype=torch.float64), ga, be, eps=1e-6)
        for ch in range(C):
            assert abs(float(b[ch]) - GS.constant_bound(level, ga, be, ss, ch, 0, C)) <= 1e-12 * float(b[ch]) + 1e-300
    # at the denoiser's eps the factor is eps^(-1/2) = 316
    assert abs(float(SE.const_bound(torch.tensor(1.0, dtype=torch.float64), torch.tensor(1.0), torch.tensor(0.0))) /
               (GS.F32_ULP * SE.EPS ** -0.5) - 1) <= 1e-12


# ------------------------------------------------------------------------------------------------ pool, time embedding
@pytest.mark.parametrize("c", SE.POOL_CASES, ids=ids)
def test_pool_reference_and_defect(c):
    t, s, o = SE.pool_operands(c)
    want = SE.pool_ref(t, s, o, c)
    # the plain formula in float64: index_add of both roles over the clamped count
    y = torch.zeros(c.O, c.H, dtype=torch.float64)
    y.index_add_(0, s, t[:, c.s_col:c.s_col + c.H].double())
    y.index_add_(0, o, t[:, c.o_col:c.o_col + c.H].double())
    cnt = torch.bincount(torch.cat([s, o]), minlength=c.O).clamp(min=1).double()
    y = y / cnt[:, None]
    assert t.shape[1] >= max(c.s_col, c.o_col) + c.H + c.extra
    assert float((want.double() - y).abs().max()) <= 1e-5
    bad = SE.pool_ref(t, s, o, c, defect="pool-s-col")
    assert float(((bad - want).abs() / (want.abs() + 1)).max()) >= SE.SIGNAL_OVER_BOUND * SE.TOL_SKINNY, c.name
    from lidargen.models.unets.graph import edge_csr

    row_ptr, slots = edge_csr(s, o, c.O)
    assert row_ptr.numel() == c.O + 1 and int(row_ptr[-1]) == slots.numel() == 2 * SE.POOL_T


@pytest.mark.parametrize("c", SE.TIME_CASES, ids=ids)
def test_time_reference(c):
    r = SE.time_ref(c)
    assert r.y.shape == (c.U, 2 * c.half) and r.e32 <= SE.TOL_SKINNY and r.bound == SE.TOL_SKINNY
    assert float(r.t.abs().max()) <= 15 and float(r.f[0]) == 1.0 and bool((r.f > 1e-4 - 1e-9).all())
    assert float((r.y[:, :c.half] ** 2 + r.y[:, c.half:] ** 2 - 1).abs().max()) <= 1e-14
