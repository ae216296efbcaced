"""The case tables of tests/test_train_edges.py, and the proof that they are complete (CPU only).

`lc_conv2d_ring_wgrad_route` / `lc_groupnorm_bwd_route` are the host functions the launchers and kernels of
csrc/conv_bwd.hip and csrc/norm.hip switch on (csrc/conv_bwd_route.h, csrc/gn_bwd_route.h), so "which branch does this
row take" is asked of the library: every value of every field is hit, the Python predicate of ConvRing.backward agrees
with the split entry's refusals on every row, the scratch query agrees with the layout, the two float64 references of the
weight gradient agree, the float32 reference stays inside every bound, and one missing term would be 16 bounds."""
import ctypes

import pytest
import torch

from tests import _train_edges as TE

ALL_W = TE.WGRAD_F32 + TE.WGRAD_SPLIT + TE.WGRAD_REFUSED
ids = lambda c: c.name


def _rows():
    """(row, ks, split requested) of everything the GPU file runs."""
    out = [(c, ks, 0) for c in ALL_W for ks in TE.KS]
    return out + [(c, ks, 1) for c in TE.WGRAD_SPLIT + TE.WGRAD_REFUSED for ks in TE.KS]


def test_names_are_unique_and_every_row_names_its_edge():
    for table in (ALL_W, TE.GN_CASES):
        assert len({c.name for c in table}) == len(table)
        assert all(c.edge for c in table)


def test_every_weight_gradient_route_is_hit():
    fam, staging, bias, causes, rel = set(), set(), set(), set(), {TE.F32: set(), TE.SPLIT: set()}
    for c, ks, split in _rows():
        rc, o = TE.wgrad_route(c, ks, split)
        if split and c in TE.WGRAD_REFUSED:
            assert rc == TE.LC_EUNSUP, c.name
            continue
        assert rc == 0, (c.name, rc)
        fam.add(o[0]); staging.add((o[0], o[1])); bias.add(o[4])
        if o[0] == TE.F32:
            causes.add(o[6])
            assert (o[1] == 1) == (o[6] == 0)
            assert o[3] == c.B * c.H * -(-c.W // 64)
        else:
            assert o[1] == 1 and o[6] == 0 and o[3] == c.B * (c.H // 2) * (c.W // 32)
        # both kernels take nsplit from the 64-column tile count
        assert 1 <= o[2] <= c.B * c.H * -(-c.W // 64)
        rel[o[0]].add("equal" if o[2] == o[3] else ("below" if o[2] < o[3] else "above"))
        if o[2] < o[3] and o[3] % o[2]:
            rel[o[0]].add("not a multiple")
        if o[3] == 1:
            rel[o[0]].add("one tile")
        assert o[5] % 2 == 0 and o[5] >= o[2] * c.Co * c.Ci * ks * ks and o[7] == 0
    assert fam == {TE.F32, TE.SPLIT}
    assert staging == {(TE.F32, 0), (TE.F32, 1), (TE.SPLIT, 1)}
    assert bias == {0, 1, 2}
    # each cause of the scalar branch ALONE on a shape that otherwise takes the vector branch.  H W % 4 cannot fail alone:
    # W % 64 == 0 implies H W % 4 == 0, so it is there with W % 64 (W = 63, 65, 130, ...)
    for cause in (TE.CAUSE_W, TE.CAUSE_XBS, TE.CAUSE_DYBS, TE.CAUSE_XADDR, TE.CAUSE_DYADDR):
        assert cause in causes, f"no row takes the scalar branch because of cause {cause} alone"
    assert any(k & TE.CAUSE_HW for k in causes) and 0 in causes
    assert all(not (k & TE.CAUSE_HW) or (k & TE.CAUSE_W) for k in causes)
    # the fp32 kernel never has more splits than tiles; the split kernel (2 x 32 tiles, splits from 64-column tiles) does
    assert rel[TE.F32] >= {"equal", "below", "not a multiple", "one tile"} and "above" not in rel[TE.F32]
    assert rel[TE.SPLIT] >= {"equal", "below", "above", "not a multiple", "one tile"}


def test_scalar_cause_rows_differ_from_the_vector_row_by_one_condition():
    base = next(c for c in TE.WGRAD_F32 if c.name == "w64-vec")
    assert TE.wgrad_route(base, 3, 0)[1][1] == 1
    for name, cause in (("cause-xbs", TE.CAUSE_XBS), ("cause-dybs", TE.CAUSE_DYBS), ("cause-xaddr", TE.CAUSE_XADDR),
                        ("cause-dyaddr", TE.CAUSE_DYADDR)):
        c = next(r for r in TE.WGRAD_F32 if r.name == name)
        assert c[2:7] == base[2:7] and TE.wgrad_route(c, 3, 0)[1][6] == cause


def test_named_weight_gradient_edges_are_in_the_table():
    f, s = TE.WGRAD_F32, TE.WGRAD_SPLIT
    assert {c.W for c in f} >= {1, 2, 3, 16, 63, 64, 65, 128, 130} and {c.H for c in f} >= {1, 2, 3}
    assert {c.Ci for c in f} >= {1, 5, 63, 64, 65, 130} and {c.Co for c in f} >= {1, 5, 63, 64, 65, 130}
    assert {c.B for c in f} >= {1, 3} and {c.B for c in s} >= {1, 3}
    assert {c.W for c in s} >= {32, 64, 96} and {c.H for c in s} >= {2, 4, 6}
    assert {c.Ci for c in s} >= {5, 63, 64, 65, 130} and {c.Co for c in s} >= {5, 63, 64, 65, 130}
    assert any(c.W == 64 and c.H == 1 and TE.wgrad_route(c, 3, 0)[1][1] == 1 for c in f), "ring wrap inside one vector tile, H = 1"
    for t in (f, s):
        assert {c.xl for c in t} >= {"contig", "slice_lo", "slice_hi"} and {c.dyl for c in t} >= {"contig", "slice_lo", "slice_hi"}
        assert any(c.dymag == 1e-4 and c.xmag == 900.0 for c in t) and any(c.xmag == 1e-4 and c.dymag == 900.0 for c in t)
        assert any(c.zero_dy for c in t) and any(c.dymag == 1e-30 for c in t)
    assert {c.xl for c in f} >= {"off1", "bs1"} and {c.dyl for c in f} >= {"off1", "bs1"}
    # a slice whose byte offset is, and is not, a multiple of 16
    mods = {TE.addr_mod16(c.xl, c.Ci, c.H * c.W) for c in f if c.xl == "slice_hi"}
    assert 0 in mods and mods - {0}
    assert any(c.bound_mult == 4.0 / 3.0 for c in s)
    assert all(c.B * c.H * c.W <= 8200 and c.Ci <= 130 and c.Co <= 130 for c in ALL_W)


def test_python_predicate_agrees_with_the_split_entry():
    from lidarcrafter_amd import autograd as AG

    seen = set()
    for c in ALL_W:
        HW = c.H * c.W
        args = (c.H, c.W, TE.batch_stride(c.xl, c.Ci, HW), TE.batch_stride(c.dyl, c.Co, HW))
        for base in (0, 4096):          # the predicate sees whole addresses, the route their last four bits
            py = AG.wgrad_split_accepts(*args, base + TE.addr_mod16(c.xl, c.Ci, HW), base + TE.addr_mod16(c.dyl, c.Co, HW))
            for ks in TE.KS:
                rc, _ = TE.wgrad_route(c, ks, 1)
                assert rc in (0, TE.LC_EUNSUP) and py == (rc == 0), (c.name, py, rc)
            seen.add(py)
    assert seen == {True, False}
    assert all(TE.wgrad_route(c, 3, 1)[0] == 0 for c in TE.WGRAD_SPLIT)
    assert all(TE.wgrad_route(c, 3, 1)[0] == TE.LC_EUNSUP and TE.wgrad_route(c, 3, 0)[0] == 0 for c in TE.WGRAD_REFUSED)
    assert [c.edge for c in TE.WGRAD_REFUSED] == ["H odd", "W % 32 != 0", "x_bs % 4", "dy_bs % 4", "x off 16 bytes", "dy off 16 bytes"]


def test_scratch_query_agrees_with_the_layout():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    for c, ks, split in _rows():
        rc, o = TE.wgrad_route(c, ks, split)
        if rc == 0:
            assert h.lc_conv2d_ring_wgrad_scratch_elems(c.B, c.Ci, c.Co, c.H, c.W, ks) == o[5] + 2 * c.Co * c.B, c.name
    assert h.lc_conv2d_ring_wgrad_scratch_elems(1, 1, 1, 1, 1, 3) == 10 + 2     # 9 partials rounded up to an even count


@pytest.mark.parametrize("c", ALL_W, ids=ids)
def test_weight_gradient_references_agree_and_bounds_are_reachable(c):
    for ks in TE.KS:
        r = TE.wgrad_ref(c, ks)
        dw, db = TE.wgrad_autograd(r.x.double(), r.dy.double(), ks)
        scale = max(float(r.S_dw.max()), 1e-300)
        assert float((dw - r.dw).abs().max()) / scale < 1e-12 and float((db - r.db).abs().max()) / max(float(r.S_db.max()), 1e-300) < 1e-12
        # H = 1: the ky = 0, 2 taps see only padding
        if c.H == 1 and ks == 3:
            assert float(r.S_dw[:, :, (0, 2)].max()) == 0.0
        assert bool((r.S_dw > 0).any()) != c.zero_dy
        # the float32 reference is inside both bounds, and one missing term is not
        assert max(r.e32_dw, r.e32_db) <= min(r.bound_f32, TE.SPLIT_BOUND), (r.e32_dw, r.e32_db)
        for bound in (r.bound_f32, TE.SPLIT_BOUND) if c in TE.WGRAD_SPLIT else (r.bound_f32,):
            assert r.signal >= TE.SIGNAL_OVER_BOUND * bound, (c.name, ks, r.signal, bound)
        if not c.zero_dy:
            # dropping ONE term of the worst-placed element is seen
            i = tuple(int(v) for v in (r.S_dw == r.S_dw.max()).nonzero()[0])
            broken = r.dw.clone()
            broken[i] -= 0.25 * c.xmag * c.dymag                  # the smallest product there is
            assert TE.rel_to_S(broken, r.dw, r.S_dw)[0] >= TE.SIGNAL_OVER_BOUND * r.bound_f32 * (1 - 1e-9)


def test_every_groupnorm_route_is_hit():
    from lidarcrafter_amd import _lib

    slabs, branch, outer, per4 = set(), set(), set(), set()
    for c in TE.GN_CASES:
        rc, o = TE.gn_route(c)
        assert rc == 0, c.name
        HW = c.H * c.W
        assert o[0] == -(-HW // 4096) == o[3] and o[1] == -(-HW // o[0])
        # one partial maximum of |dx| per block of the apply pass
        assert _lib.lib().lc_groupnorm_amax_partials(c.B, c.C, c.H, c.W, c.G, 1) == o[0] * c.C * c.B
        slabs.add(o[0]); branch.add(o[2]); outer.add(o[3]); per4.add((HW % 4 == 0, o[1] % 4 == 0))
    assert slabs == {1, 2, 3} and outer == {1, 2, 3} and branch == {0, 1, 2}
    assert per4 >= {(False, False), (True, False), (True, True)}
    # each address alone sends a vector-branch shape to the scalar branch
    base = next(c for c in TE.GN_CASES if c.name == "hw4104-cpg2")
    assert TE.gn_route(base)[1][2] == 1
    for name in ("x-off1", "dy-off1", "dx-off1"):
        c = next(r for r in TE.GN_CASES if r.name == name)
        assert c[2:7] == base[2:7] and TE.gn_route(c)[1][2] == 0
    assert TE.gn_route(next(c for c in TE.GN_CASES if c.name == "slices"))[1][2] == 1


def test_named_groupnorm_edges_are_in_the_table():
    g = TE.GN_CASES
    assert {c.H * c.W for c in g} >= {1, 3, 250, 4096, 4100, 4104, 8192, 8200}
    assert all(c.W % 2 == 0 for c in g if c.H * c.W in (8192, 8200))
    assert {c.C // c.G for c in g} >= {1, 2, 6, 8, 16} and any(c.G == 1 for c in g) and {c.B for c in g} >= {1, 3}
    assert {(c.affine, c.adagn) for c in g} == {(True, True), (True, False), (False, True), (False, False)}
    assert {c.act for c in g} == {True, False}
    for shape in {(c.B, c.C, c.G, c.H, c.W) for c in g}:
        assert any((c.B, c.C, c.G, c.H, c.W) == shape and c.affine and c.adagn for c in g), shape
    for cpg in (2, 8):
        assert {c.data for c in g if c.data and c.C // c.G == cpg} == set(TE.GS.DATA_NAMES)
    assert any(c.dxl == "slice_hi" for c in g) and {c.xl for c in g} >= {"slice_lo", "slice_hi", "off1", "bs1"}
    assert all(c.C * c.H * c.W <= 2 * 130 * 130 * 8 and c.H * c.W <= 8200 for c in g)


@pytest.mark.parametrize("c", TE.GN_CASES, ids=ids)
def test_groupnorm_references_and_bounds(c):
    r = TE.gn_ref(c)
    sums, S = TE.gn_terms(r.t, c.G, c.act)
    # the terms whose absolute sums normalise the parameter errors are the terms of the autograd gradients
    for k in sums:
        assert float((sums[k] - r.ref64[k]).abs().max()) <= 1e-10 * max(float(S[k].max()), 1e-300), k
        assert float(S[k].min()) > 0 or r.const is not None, k
    assert torch.isfinite(r.ref64["x"]).all() and torch.isfinite(r.ref32["x"]).all()
    assert (r.const is not None) == (c.data == "constant")
    # not vacuous: the float32 oracle errs, and every bound stays three orders below a wrong or missing term (O(1))
    assert r.e32_dx > 0
    assert r.bound_dx <= 1e-3 and all(v <= 1e-3 for v in r.bound_p.values()), (r.bound_dx, r.bound_p)


def test_structured_rows_reach_a_large_mean():
    """|group mean| / group std of the stored float32 tensor: what xh = (x - mu) rstd from a float32 mu has to survive.
    Pairs: the level table reaches 1700 at step 2^-8; whole-octet groups sit at one level, so only the common-level data
    (0.01 randn + 30) is far from zero there."""
    def ratio(c):
        mean, var, _ = TE.GS.group_stats64(TE.gn_operands(c)[0]["x"], c.G)
        live = var > 0
        return float((mean.abs()[live] / var[live].sqrt()).max())

    rows = {c.name: c for c in TE.GN_CASES if c.data}
    for name, least in (("step8-a4-cpg2", 1700), ("step8-a0-cpg2", 1700), ("step5-a4-cpg2", 200), ("common-cpg2", 3000),
                        ("common-cpg8", 3000)):
        assert ratio(rows[name]) >= least, (name, ratio(rows[name]))


def test_refusals_come_before_any_hip_call():
    """Dummy non-null pointers, no GPU: every refusal of the two weight-gradient entries and of the GroupNorm backward is
    returned before anything is launched or dereferenced, with the code the route function gives."""
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p = (p + 15) // 16 * 16
    out = (ctypes.c_int32 * 8)()
    f32 = lambda B=1, Ci=1, Co=1, H=2, W=32, ks=3: h.lc_conv2d_ring_wgrad(p, Ci * H * W, p, Co * H * W, p, p, p, B, Ci, Co, H, W, ks, 0, None)
    spl = lambda B=1, Ci=1, Co=1, H=2, W=32, ks=3, xb=None, db=None, xo=0, do=0: h.lc_conv2d_ring_wgrad_f16x2(
        p + xo, Ci * H * W if xb is None else xb, p + do, Co * H * W if db is None else db, p, p, p, p, p, B, Ci, Co, H, W, ks, 0, None)
    rt = lambda split, B=1, Ci=1, Co=1, H=2, W=32, ks=3, xb=64, db=64, xo=0, do=0: h.lc_conv2d_ring_wgrad_route(
        split, B, Ci, Co, H, W, ks, xb, db, xo, do, out)
    for kw in (dict(B=0), dict(Ci=0), dict(Co=0), dict(H=0), dict(W=0), dict(B=-1)):
        assert f32(**kw) == spl(**kw) == rt(0, **kw) == rt(1, **kw) == TE.LC_EINVAL, kw
    for kw in (dict(ks=2), dict(ks=5), dict(ks=0)):
        assert f32(**kw) == spl(**kw) == rt(0, **kw) == rt(1, **kw) == TE.LC_EUNSUP, kw
    assert f32(B=0, ks=2) == spl(B=0, ks=2) == rt(1, B=0, ks=2) == TE.LC_EINVAL           # sizes are judged first
    for kw in (dict(H=3), dict(W=48), dict(xb=65), dict(db=65), dict(xo=4), dict(do=8)):
        assert spl(**kw) == rt(1, **kw) == TE.LC_EUNSUP and rt(0, **kw) == 0, kw
    assert h.lc_conv2d_ring_wgrad(None, 64, p, 64, p, p, p, 1, 1, 1, 2, 32, 3, 0, None) == TE.LC_EINVAL
    assert h.lc_conv2d_ring_wgrad_f16x2(p, 64, p, 64, None, p, p, p, p, 1, 1, 1, 2, 32, 3, 0, None) == TE.LC_EINVAL
    assert h.lc_conv2d_ring_wgrad_route(0, 1, 1, 1, 2, 32, 3, 64, 64, 0, 0, None) == TE.LC_EINVAL
    assert h.lc_conv2d_ring_wgrad_scratch_elems(0, 1, 1, 2, 32, 3) == 0 == h.lc_conv2d_ring_wgrad_scratch_elems(1, 1, 1, 2, 32, 2)
    gn = lambda B=1, C=4, H=2, W=2, G=2: h.lc_groupnorm_bwd_train(p, C * H * W, p, C * H * W, p, None, None, None, None, C, p, p,
                                                                 C * H * W, None, None, None, None, B, C, H, W, G, 1, None, None)
    gr = lambda B=1, C=4, H=2, W=2, G=2: h.lc_groupnorm_bwd_route(B, C, H, W, G, 16, 16, 16, 0, 0, 0, out)
    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(G=0), dict(G=3), dict(C=-4)):
        assert gn(**kw) == gr(**kw) == TE.LC_EINVAL, kw
    assert gr() == 0 and list(out)[:4] == [1, 4, 1, 1]
