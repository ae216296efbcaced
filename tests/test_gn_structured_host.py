"""CPU side of tests/test_gn_structured.py: the structured data reaches the R it is meant to reach, the float32 oracle
(what the GPU test's bound is built from) is finite on every case, the closed form of an exactly constant group holds in
float64, and every statistics-emitting entry point of ops.py has a case in the GPU file.  No GPU."""
import functools

import pytest
import torch

from tests import _gn_structured as S

CASES = [(r.name, d) for r in S.ROUTES for d in S.DATA_NAMES]


@functools.lru_cache(maxsize=None)
def _stored(route_name, data):
    """The producer's result as the kernel stores it (float32), from the float64 evaluation of the same operation."""
    route = S.ROUTE_BY_NAME[route_name]
    case = S.make_case(route, data)
    return case, S.cpu_produce(route, case, torch.float64).float()


def test_every_statistics_entry_point_has_a_case():
    """Every `_attach_stats` call site of ops.py is the entry of at least one route of the GPU file -- a new producer of
    statistics entries fails here until it has structured-data cases."""
    sites = S.attach_sites()
    assert len(sites) >= 5, sites
    entries = {r.entry for r in S.ROUTES}
    missing = [f"{fn} (ops.py:{line})" for fn, line in sites if fn not in entries]
    assert not missing, f"statistics-emitting entry points without a case in tests/test_gn_structured.py: {missing}"
    assert entries <= {fn for fn, _ in sites}, "a route names an entry point that attaches no statistics"
    # every unit a producer can be asked for: octets everywhere, pairs (deferred epilogues), quads (pre-split, fold-down),
    # one channel (up-fold, down-sampler)
    units = {(r.entry, r.unit) for r in S.ROUTES}
    assert {("conv2d_ring", 8), ("conv2d_ring", 2), ("_conv2d_ring_presplit", 8), ("_conv2d_ring_presplit", 4),
            ("conv_down2", 8), ("conv_down2", 4), ("conv_up2", 1), ("resample2x", 1)} <= units
    for r in S.ROUTES:
        B, C, H, W = r.out_shape()
        assert B <= 3 and C <= 192 and C % r.G == 0 and (C // r.G) % r.unit == 0, r.name


def test_level_table():
    lv = S.levels(64, 32, 0.25)
    assert lv[:8].tolist() == [-3.0, -2.75, -1.0, -0.75, 1.0, 1.25, 3.0, 3.25]
    assert lv[8:10].tolist() == [-2.5, -2.25] and lv[24:26].tolist() == [-3.0, -2.75]
    assert S.levels(64, 16, 0.5)[:8].tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5]
    assert S.levels(64, 8, 1.0)[:9].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 0.5]
    # 6 per group: a group sits at one level, octets begin inside other groups
    l6 = S.levels(192, 32, 2.0 ** -5)
    assert float((l6[6:12] - l6[6]).abs().max()) <= 5 * 2.0 ** -5 and abs(float(l6[8] - l6[0])) >= 1.5


@pytest.mark.parametrize("route_name,data", CASES)
def test_structured_case_on_the_cpu(route_name, data):
    route = S.ROUTE_BY_NAME[route_name]
    case, y = _stored(route_name, data)
    assert tuple(y.shape) == route.out_shape(case["shape"])
    B, C = y.shape[:2]
    G = route.G
    R = S.measure_R(y, G)
    p = S.gn_params(B, C)
    silu = data != "constant"
    tol = S.TOL_COMMON if data == "common" else S.TOL_ENTRY
    bound, e32, ref64 = S.bound_for(y, G, p, silu, tol, case["const"])
    assert bool(torch.isfinite(ref64).all()) and bound >= tol and bound < 1e-2, bound
    if data in S.SPECIAL:
        if data == "constant":
            g = case["const"]
            cpg = C // G
            blk = y[:, g * cpg:(g + 1) * cpg]
            assert bool((blk == blk[:, :1, :1, :1]).all()), "the group is not exactly constant as stored"
            for b in range(B):
                for c in range(g * cpg, (g + 1) * cpg):
                    want = S.constant_closed_form(p["be"], p["ss"], c, b, C, silu)
                    # (condition 3 of the GPU file in float64: one rounding of the mean, times 1 / sqrt(eps))
                    lim = S.constant_bound(float(blk.abs().max()), p["ga"], p["be"], p["ss"], c, b, C, ulp=2.0 ** -52)
                    assert float((ref64[b, c] - want).abs().max()) <= lim, (b, c, float((ref64[b, c] - want).abs().max()))
        return
    # the intended R: the level table's own (constant planes), which the spatial spread a * step barely moves; a
    # producer with a border rule (rows 0 and H - 1 of the down-sampled plane carry 7/8 of a constant) spreads the group
    # by |level| / 8 on those rows instead
    step, a = S.data_spec(data)
    table = S.measure_R(S.levels(C, G, step)[None, :, None, None].expand(1, C, 2, 2), G)
    border = route.entry in ("conv_down2", "resample2x")
    if not border and data != "control":
        assert float(R.max()) >= 0.9 * float(table.max()), (float(R.max()), float(table.max()))
    if route.sub_octet and data == "step8-a4":
        assert float(R.max()) >= S.R_MIN, float(R.max())
