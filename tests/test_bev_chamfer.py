"""GPU checks of the Minimum Matching Distance feature against tests/_bev_chamfer_oracle.py: lc_chamfer2d_fwd bit for bit
against the float32 restatement of the reference kernel; pcd2bev_bin array for array; the grid route (csrc/bev_chamfer.hip,
ops.bev_chamfer_min) against the exact integer value to 1e-12 relative; compute_mmd against both.

Tolerance between the reference's float32 arithmetic (the literal route) and the exact value, per pair, relative:
2^-21 max(nx, ny) + 1e-5 (O.tolerance) -- coordinates k / n rounded to float32 carry 2^-24 each, a difference 2^-23 against
a smallest non-zero difference of 1 / n, the square doubles it, 1e-5 covers the float32 means.  Derived, not measured."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bev_chamfer_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

R32, R64, ANISO = ((-30, 30), (-30, 30)), ((-50, 50), (-50, 50)), ((-6, 6), (-10, 10))


def _cuda(clouds):
    return [torch.from_numpy(c).cuda() for c in clouds]


def _exact(ref, smp, rng_xy):
    nx, ny, _ = O.grid(rng_xy[0], rng_xy[1], 0.5)
    cr = [O.bev_cells(c, rng_xy[0], rng_xy[1], 0.5) for c in ref]
    cs = [O.bev_cells(c, rng_xy[0], rng_xy[1], 0.5) for c in smp]
    return O.exact_matrix(cr, cs, nx, ny), cr, cs, (nx, ny)


def _grid(ref, smp, rng_xy, **kw):
    from lidarcrafter_amd import ops

    mn, arg, mat = ops.bev_chamfer_min(_cuda(ref), _cuda(smp), rng_xy[0], rng_xy[1], 0.5, return_matrix=True, **kw)
    assert mn.dtype == torch.float64 and arg.dtype == torch.int64 and mat.dtype == torch.float64
    return mn.cpu().numpy(), arg.cpu().numpy(), mat.cpu().numpy()


def _check(ref, smp, rng_xy, **kw):
    want, _, _, _ = _exact(ref, smp, rng_xy)
    mn, arg, mat = _grid(ref, smp, rng_xy, **kw)
    err = np.abs(mat - want) / np.where(want > 0, want, 1.0)
    print(f"grid route: worst relative error {err.max():.2e} over {want.shape} pairs")
    assert mat.shape == want.shape and (err <= 1e-12).all()
    assert np.array_equal(mn, mat.min(axis=1))
    assert np.array_equal(mat[np.arange(len(ref)), arg], mn)
    srt = np.sort(want, axis=1)
    clear = (srt[:, 1] - srt[:, 0] > 1e-9 * srt[:, 1]) if want.shape[1] > 1 else np.ones(len(ref), bool)
    assert np.array_equal(arg[clear], np.argmin(want, axis=1)[clear])
    return mn, arg, mat, want


# ---------------------------------------------------------------------------------------------- chamfer2d
def _grid_points(rng, b, n):
    return (rng.integers(0, 6, (b, n, 2)) / 6.0).astype(np.float32)


@pytest.mark.parametrize("B,N,M,ties", [(1, 1, 1, False), (2, 96, 513, False), (1, 700, 1030, False), (3, 40, 40, True)],
                         ids=["1x1", "96x513", "700x1030", "ties40"])
def test_chamfer2d_is_the_reference_kernel_bit_for_bit(B, N, M, ties):
    from lidargen.metrics.chamfer import chamfer_2DDist

    rng = np.random.default_rng(100 + N)
    if ties:
        a, b = _grid_points(rng, B, N), _grid_points(rng, B, M)      # 36 distinct points among 40: ties are certain
    else:
        a, b = rng.random((B, N, 2), np.float32), rng.random((B, M, 2), np.float32)
    want = O.chamfer2d(a, b)
    got = chamfer_2DDist()(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert [tuple(g.shape) for g in got] == [(B, N), (B, M), (B, N), (B, M)]
    assert got[0].dtype == torch.float32 and got[2].dtype == torch.int32
    for g, w, name in zip(got, want, ("dist1", "dist2", "idx1", "idx2")):
        assert np.array_equal(g.cpu().numpy(), w), name
    if ties:
        assert (want[0] == 0).any()


def test_pairwise_cd_batch_takes_2d_clouds():
    from lidargen.metrics.chamfer import compute_pairwise_cd_batch

    clouds = O.sweeps(11, 4, *R32)
    (sets,) = O.pcd2bev_bin("32", clouds)
    want = O.pairwise_cd_batch(sets[0], sets[1:])
    got = compute_pairwise_cd_batch(sets[0], sets[1:])
    assert np.allclose(got, want, rtol=1e-5, atol=0)          # the same float32 distances; the means' order differs


# ---------------------------------------------------------------------------------------------- pcd2bev_bin
@pytest.mark.parametrize("data", ["32", "64"])
@pytest.mark.parametrize("kind", ["numpy", "cuda"])
def test_pcd2bev_bin_equals_the_oracle(data, kind):
    from lidargen.metrics import metric_utils

    cfg = O.DATA_CONFIG[data]
    a = O.sweeps(21, 3, cfg["x"], cfg["y"])
    a.append(np.full((9, 3), 1000.0, np.float32))                         # every point out of range
    a.append(O.cloud_of_cells([[3, 4], [0, 0], [3, 4]], cfg["x"], cfg["y"], repeat=3))   # duplicate cells
    b = O.sweeps(22, 2, cfg["x"], cfg["y"])
    b[1] = np.ascontiguousarray(np.concatenate([b[1], b[1][:, :1]], axis=1))   # a cloud with four columns
    want = O.pcd2bev_bin(data, a, b)
    if kind == "cuda":
        got = metric_utils.pcd2bev_bin(data, _cuda(a), _cuda(b))
        assert all(isinstance(g, torch.Tensor) and g.is_cuda for part in got for g in part)
        got = tuple([g.cpu().numpy() for g in part] for part in got)
    else:
        got = metric_utils.pcd2bev_bin(data, a, b)
        assert all(isinstance(g, np.ndarray) for part in got for g in part)
    assert len(got) == 2 and [len(p) for p in got] == [5, 2]
    for gp, wp in zip(got, want):
        for g, w in zip(gp, wp):
            assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w)
    assert got[0][3].shape == (0, 2) and got[0][4].shape == (2, 2)


# ---------------------------------------------------------------------------------------------- the grid route
def test_grid_route_32():
    _check(O.sweeps(31, 3, *R32), O.sweeps(32, 5, *R32), R32)


def test_grid_route_64():
    _check(O.sweeps(33, 2, *R64), O.sweeps(34, 3, *R64), R64)


def test_grid_route_anisotropic_24x40():
    assert O.grid(ANISO[0], ANISO[1], 0.5)[:2] == (24, 40)
    _check(O.sweeps(35, 3, *ANISO), O.sweeps(36, 4, *ANISO), ANISO)


def test_grid_route_integer_sums_are_exact():
    """The integer level under the float64 division: bitmaps -> cell lists -> transforms -> pair sums, entry by entry."""
    from lidarcrafter_amd import ops
    from lidarcrafter_amd._lib import check, lib

    ref, smp = O.sweeps(37, 2, *ANISO), O.sweeps(38, 3, *ANISO)
    _, cr, cs, (nx, ny) = _exact(ref, smp, ANISO)
    bits, counts, _ = ops._bev_bits(_cuda(ref + smp), ANISO[0], ANISO[1], 0.5, "clouds")
    cells, offs, host = ops._bev_cell_lists(bits, counts, nx, ny)
    assert host == [len(c) for c in cr + cs]
    flat = np.concatenate([c[:, 0] * ny + c[:, 1] for c in cr + cs])
    assert np.array_equal(cells.cpu().numpy()[:len(flat)], flat)
    tmp = torch.empty(3 * nx * ny, device="cuda", dtype=torch.int32)
    dt = torch.empty(nx * ny * 16, device="cuda", dtype=torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    check(lib().lc_bev_distance_transform(bits[2].data_ptr(), 3, nx, ny, tmp.data_ptr(), dt.data_ptr(), 16, s), "dt")
    d = dt.cpu().numpy().view(np.uint32).reshape(nx * ny, 16)
    ii, jj = np.divmod(np.arange(nx * ny), ny)
    for m, c in enumerate(cs):
        want = ((ii[:, None] - c[None, :, 0]) ** 2 * ny * ny + (jj[:, None] - c[None, :, 1]) ** 2 * nx * nx).min(axis=1)
        assert np.array_equal(d[:, m], want), m
    assert not d[:, 3:].any()
    a = torch.empty(2 * 3, device="cuda", dtype=torch.int64)
    check(lib().lc_bev_pair_sums(cells.data_ptr(), offs.data_ptr(), 2, dt.data_ptr(), 16, 3, a.data_ptr(), s), "sums")
    want = [[O.exact_sums(r, c, nx, ny)[0] for c in cs] for r in cr]
    assert a.cpu().numpy().reshape(2, 3).tolist() == want


def test_grid_route_degenerate_sets():
    """A single-cell set, identical sets (exactly 0), a full row and a full column of occupied cells."""
    xr, yr = ANISO
    nx, ny = 24, 40
    row = O.cloud_of_cells([[5, j] for j in range(ny)], xr, yr)
    col = O.cloud_of_cells([[i, 39] for i in range(nx)], xr, yr)
    one = O.cloud_of_cells([[23, 0]], xr, yr, repeat=4)
    rnd = O.sweeps(39, 1, xr, yr)[0]
    ref, smp = [one, row, rnd, col], [row, one, col, rnd.copy()]
    mn, arg, mat, want = _check(ref, smp, ANISO)
    assert mat[1, 0] == 0.0 and mat[0, 1] == 0.0 and mat[2, 3] == 0.0 and mat[3, 2] == 0.0
    assert mn.tolist() == [0.0] * 4 and arg.tolist() == [1, 0, 3, 2]
    # one cell against the full row: ((18^2 / 24^2) + mean over j of (18^2 / 24^2 + j^2 / 40^2)) / 2
    assert mat[0, 0] == pytest.approx((0.5625 + 0.5625 + sum(j * j for j in range(ny)) / ny / 1600.0) / 2, rel=1e-14)


def test_grid_route_ragged_lane_tail():
    """S = 65 sets of 10 points: the second 64-lane tile of the pair sums holds one live lane."""
    rng = np.random.default_rng(40)
    mk = lambda: O.cloud_of_cells(rng.integers(0, (24, 40), (10, 2)), *ANISO)
    _check([mk() for _ in range(3)], [mk() for _ in range(65)], ANISO)


def test_grid_route_chunks_are_bit_equal():
    """A scratch cap that splits both the references and the samples into several chunks changes no bit."""
    ref, smp = O.sweeps(41, 3, *R32), O.sweeps(42, 5, *R32)
    whole = _grid(ref, smp, R32)
    cap = 2 * 12 * 120 * 120 + 64                     # room for chunks of two clouds: R -> 2 chunks, S -> 3
    n = (math.isqrt((12 * 14400) ** 2 + 64 * cap) - 12 * 14400) // 32
    assert n == 2
    parts = _grid(ref, smp, R32, max_scratch_bytes=cap)
    ones = _grid(ref, smp, R32, max_scratch_bytes=0)  # chunks of one
    for w, p, o in zip(whole, parts, ones):
        assert np.array_equal(w, p) and np.array_equal(w, o)
    from lidarcrafter_amd import ops

    mn, arg = ops.bev_chamfer_min(_cuda(ref), _cuda(smp), R32[0], R32[1], 0.5, max_scratch_bytes=cap)
    assert np.array_equal(mn.cpu().numpy(), whole[0]) and np.array_equal(arg.cpu().numpy(), whole[1])


def test_grid_route_names_an_empty_cloud():
    from lidarcrafter_amd import ops

    ref = O.sweeps(43, 2, *R32)
    smp = [ref[0], np.full((6, 3), 500.0, np.float32)]
    with pytest.raises(ValueError, match="sample cloud 1"):
        ops.bev_chamfer_min(_cuda(ref), _cuda(smp), R32[0], R32[1], 0.5)
    with pytest.raises(ValueError, match="reference cloud 0"):
        ops.bev_chamfer_min(_cuda(smp[1:]), _cuda(ref), R32[0], R32[1], 0.5)


def test_oversized_grid_falls_back_to_the_literal_route():
    """70 000 cells wide: 2 nx^2 ny^2 does not fit 32 bits, the grid route refuses, bev_min_matching takes route 1."""
    from lidarcrafter_amd import ops
    from lidargen.metrics.chamfer import bev_min_matching

    xr, yr = (0, 35000), (-1, 1)
    nx, ny, _ = O.grid(xr, yr, 0.5)
    assert (nx, ny) == (70000, 4)
    rng = np.random.default_rng(44)
    mk = lambda n: np.stack([rng.uniform(0, 35000, n), rng.uniform(-1, 1, n), np.zeros(n)], axis=1).astype(np.float32)
    ref, smp = [mk(60), mk(90)], [mk(70), mk(50), mk(120)]
    with pytest.raises(ops.BevGridUnsupported):
        ops.bev_chamfer_min(_cuda(ref), _cuda(smp), xr, yr, 0.5)
    want, _, _, _ = _exact(ref, smp, (xr, yr))
    mn, arg = bev_min_matching(ref, smp, xr, yr, 0.5)
    tol = O.tolerance(nx, ny)
    err = np.abs(mn - want.min(axis=1)) / want.min(axis=1)
    print(f"literal route on 70000 x 4: worst relative error {err.max():.2e}, tolerance {tol:.2e}")
    assert (err <= tol).all() and np.array_equal(arg, np.argmin(want, axis=1))


# ---------------------------------------------------------------------------------------------- compute_mmd
@pytest.mark.parametrize("data", ["32", "64"])
def test_compute_mmd(data, capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils
    from lidargen.metrics.chamfer import bev_min_matching

    cfg = O.DATA_CONFIG[data]
    rng_xy = (cfg["x"], cfg["y"])
    ref, smp = O.sweeps(51, 3, *rng_xy), O.sweeps(52, 4, *rng_xy)
    want, _, _, (nx, ny) = _exact(ref, smp, rng_xy)
    score = eval_utils.compute_mmd(ref, smp, data)
    out = capsys.readouterr().out
    assert out == "Evaluating (MMD) ...\n" + OUTPUT_TEMPLATE.format("MMD ", score) + "\n"
    exact = float(np.mean(want.min(axis=1)))
    assert isinstance(score, float) and abs(score - exact) <= 1e-12 * exact
    assert eval_utils.compute_mmd(_cuda(ref), _cuda(smp), data, verbose=False) == score
    lit, arg = bev_min_matching(ref, smp, cfg["x"], cfg["y"], 0.5, route="literal")
    err = np.abs(lit - want.min(axis=1)) / want.min(axis=1)
    print(f"literal route, '{data}': worst relative error {err.max():.2e}, tolerance {O.tolerance(nx, ny):.2e}")
    assert (err <= O.tolerance(nx, ny)).all()
    assert abs(float(lit.mean()) - score) <= O.tolerance(nx, ny) * score
    with pytest.raises(ValueError, match="sample cloud 0"):
        eval_utils.compute_mmd(ref, [np.full((4, 3), 900.0, np.float32)], data)
