"""Voxel scatter of the metrics front-end (SURVEY.md §8f-3 ii): `pcd2bev_sum`, `sparse_quantize`,
`ravel_hash` of lidargen/metrics/metric_utils.py on the device vs outputs of the reference's own
functions (tests/golden/voxel.npz) -- integer / index work: BIT-EXACT.  `pytest -m gpu`
(`test_ravel_hash` runs on the CPU).  `sparse_quantize` also against the reference's lines restated in numpy
(`_quantize_lines`), on coordinates that sit on cell boundaries -- where a voxel size rounded to float32 on its way to the
kernel puts a third of the rows into the cell below --, at block tails, on -0.0 and on a ravel hash beyond 2^32."""
import numpy as np
import pytest
import torch

from lidarcrafter_amd.testing import synth_points

T = torch.from_numpy


def test_ravel_hash(golden):
    from lidargen.metrics import metric_utils as M

    g = golden("voxel")
    q = np.floor(synth_points(20000, seed=11)[:500, :3] / 0.7).astype(np.int32)
    assert np.array_equal(M.ravel_hash(q), g["hash"])


@pytest.mark.gpu
@pytest.mark.parametrize("tag,cols,vs", [("2d", 2, 0.5), ("3d", 3, (0.4, 0.4, 0.2))])
def test_sparse_quantize_bit_exact(golden, tag, cols, vs):
    from lidargen.metrics import metric_utils as M

    g = golden("voxel")
    pts = synth_points(20000, seed=11)[:, :cols].copy()
    c, idx, inv = M.sparse_quantize(pts, vs, return_index=True, return_inverse=True)     # numpy path
    assert np.array_equal(c, g[f"sq_{tag}_coords"]) and c.dtype == np.int32
    assert np.array_equal(idx, g[f"sq_{tag}_index"])
    assert np.array_equal(inv, g[f"sq_{tag}_inverse"])
    d = T(pts).cuda()
    cd, id_, iv = M.sparse_quantize(d, vs, return_index=True, return_inverse=True)         # device path
    assert cd.is_cuda and torch.equal(cd.cpu(), T(g[f"sq_{tag}_coords"]))
    assert torch.equal(id_.cpu(), T(g[f"sq_{tag}_index"])) and torch.equal(iv.cpu(), T(g[f"sq_{tag}_inverse"]))
    only = M.sparse_quantize(d, vs)
    assert torch.equal(only, cd)
    # property at a size the CPU reference would take long for: unique rows reproduce the input
    big = T(synth_points(1 << 20, seed=12)[:, :3].copy()).cuda()
    cb, ib, vb = M.sparse_quantize(big, 0.25, return_index=True, return_inverse=True)
    q = torch.floor(big.double() / 0.25).to(torch.int32)
    assert torch.equal(cb[vb], q) and torch.equal(q[ib], cb)
    assert torch.equal(cb, torch.unique(q, dim=0))              # lexicographic order, no duplicates


def _quantize_lines(coords, voxel_size, divisor=np.array):
    """The reference's lines (metric_utils.py:28-40, 49-59) restated in numpy: a scalar voxel size becomes a tuple, the
    tuple a float64 ARRAY, so the quotient of float32 coordinates is float64; floor, int32, ravel_hash, np.unique.
    `divisor` builds the array the coordinates are divided by.  -> (coords, index, inverse, the hash of every row)."""
    if isinstance(voxel_size, (float, int)):
        voxel_size = (voxel_size,) * coords.shape[1]
    q = np.floor(coords / divisor(voxel_size)).astype(np.int32)
    x = (q - np.min(q, axis=0)).astype(np.uint64)
    xmax = np.max(x, axis=0).astype(np.uint64) + np.uint64(1)
    h = np.zeros(x.shape[0], dtype=np.uint64)
    for k in range(x.shape[1] - 1):
        h += x[:, k]
        h *= xmax[k + 1]
    h += x[:, -1]
    _, index, inverse = np.unique(h, return_index=True, return_inverse=True)
    return q[index], index, inverse.reshape(-1), h


def _narrowed(voxel_size):
    """The voxel sizes rounded to float32 on their way: what a `float` argument of the C entry makes of them."""
    return np.array(voxel_size, np.float32).astype(np.float64)


def _quantize_equals_the_lines(M, c, vs):
    """Device path and numpy path of M.sparse_quantize on c against the restated lines, bit for bit."""
    want_c, want_i, want_v, _ = _quantize_lines(c, vs)
    cd, id_, iv = M.sparse_quantize(T(c).cuda(), vs, return_index=True, return_inverse=True)
    assert cd.dtype == torch.int32 and id_.dtype == torch.int64 and iv.dtype == torch.int64
    bad = int((cd.cpu().numpy() != want_c).any(1).sum()) if tuple(cd.shape) == want_c.shape else -1
    assert bad == 0, f"{bad} of {len(want_c)} voxels differ (-1: another number of voxels, {tuple(cd.shape)})"
    assert np.array_equal(id_.cpu().numpy(), want_i) and np.array_equal(iv.cpu().numpy(), want_v)
    assert torch.equal(M.sparse_quantize(T(c).cuda(), vs), cd)
    nc, ni, nv = M.sparse_quantize(c, vs, return_index=True, return_inverse=True)
    assert np.array_equal(nc, want_c) and np.array_equal(ni, want_i) and np.array_equal(nv, want_v)


def _boundary_case(D, vs):
    """(c, voxel sizes of the D columns): c[:, d] = float32(k * v_d), k = -2000 .. 1999 in an order of its own for every
    column: every coordinate sits on a cell boundary as well as float32 can say it."""
    g = np.random.default_rng(D)
    v = vs if isinstance(vs, float) else vs[:D]
    k = np.stack([g.permutation(np.arange(-2000, 2000)) for _ in range(D)], 1)
    return (k * np.array(v, np.float64)).astype(np.float32), v


def _moved(c, v):
    """The fraction of the rows that the restated lines put into another voxel when the voxel size is rounded to float32
    on its way (0.5 / 0.1 floors to 5, 0.5 / float32(0.1) to 4)."""
    v = (v,) * c.shape[1] if isinstance(v, float) else v
    return float((np.floor(c / np.array(v)) != np.floor(c / _narrowed(v))).any(1).mean())


BOUNDARY_VOXELS = [0.05, 0.1, 0.2, 0.4, 0.7, (0.4, 0.1, 0.2)]


@pytest.mark.parametrize("vs", BOUNDARY_VOXELS, ids=str)
@pytest.mark.parametrize("D", [2, 3])
def test_boundary_inputs_tell_a_narrowed_voxel_apart(D, vs):
    """The guard of the boundary test below, on the host: a float32 voxel size moves at least 10 % of these rows."""
    c, v = _boundary_case(D, vs)
    moved = _moved(c, v)
    print(f"D={D} voxel {vs}: {100 * moved:.1f} % of the rows move with a float32 voxel")
    assert moved >= 0.10
    assert c.shape == (4000, D) and len(np.unique(c[:, 0])) == 4000
    narrow = _quantize_lines(c, v, _narrowed)[0]
    assert narrow.shape != _quantize_lines(c, v)[0].shape or not np.array_equal(narrow, _quantize_lines(c, v)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("vs", BOUNDARY_VOXELS, ids=str)
@pytest.mark.parametrize("D", [2, 3])
def test_sparse_quantize_on_cell_boundaries(D, vs):
    """Grid-aligned coordinates: the voxel of float32(k v) is decided by the float64 quotient with the float64 voxel size.
    (With the voxel size handed to the kernel as a float32 this failed: a third to a half of the 4000 voxels differed.)"""
    from lidargen.metrics import metric_utils as M

    c, v = _boundary_case(D, vs)
    assert _moved(c, v) >= 0.10                                      # the inputs can tell the two apart
    _quantize_equals_the_lines(M, c, v)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257])
@pytest.mark.parametrize("D", [2, 3])
def test_sparse_quantize_block_tails(D, N):
    """One row, two, and one below / at / above the 256 rows of a block, on a grid so small that rows repeat."""
    from lidargen.metrics import metric_utils as M

    g = np.random.default_rng(10 * N + D)
    c = (g.integers(-4, 5, (N, D)) * 0.1).astype(np.float32)
    _quantize_equals_the_lines(M, c, 0.1)
    if N >= 255:
        assert len(_quantize_lines(c, 0.1)[1]) < N


@pytest.mark.gpu
def test_sparse_quantize_edge_values():
    from lidargen.metrics import metric_utils as M

    # all rows equal: one voxel, its first occurrence is row 0
    c = np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (1000, 1))
    cd, id_, iv = M.sparse_quantize(T(c).cuda(), 0.1, return_index=True, return_inverse=True)
    assert tuple(cd.shape) == (1, 3) and id_.tolist() == [0] and bool((iv == 0).all()) and len(iv) == 1000
    _quantize_equals_the_lines(M, c, 0.1)
    # -0.0 is in cell 0, -1e-7 in cell -1, and float32(-0.2) lies below -0.2: cell -2 of a 0.2 grid, as float32(-0.6) does
    c = np.array([[-0.0, 0.0, -1e-7], [0.0, -0.0, 0.0], [-0.2, -0.4, -1e-7], [-1e-7, 0.2, -0.6], [-0.0, -0.0, -0.0],
                  [-0.4, -0.2, 0.6], [-1e-7, -1e-7, -1e-7], [0.2, 0.4, -0.2]], np.float32)
    want = _quantize_lines(c, 0.2)[0]
    assert [-2, -3, -1] in want.tolist() and [0, 0, 0] in want.tolist() and [-1, -1, -1] in want.tolist()
    for D in (2, 3):
        _quantize_equals_the_lines(M, np.ascontiguousarray(c[:, :D]), 0.2)
        _quantize_equals_the_lines(M, np.ascontiguousarray(c[:, :D]), (0.2, 0.1, 0.4)[:D])
    # a ravel hash beyond 2^32: x and y span about 2^22 cells each (integers in float32 are exact up to 2^24)
    g = np.random.default_rng(4)
    c = np.concatenate([g.integers(-(1 << 20), 1 << 20, (1500, 2)), g.integers(-3, 4, (1500, 1))], 1)
    c[:300] = c[300:600]                                            # rows that repeat
    c[0], c[1] = (-(1 << 20), -(1 << 20), -3), ((1 << 20) - 1, (1 << 20) - 1, 3)
    c = c[g.permutation(1500)].astype(np.float32)
    want_c, _, _, h = _quantize_lines(c, 0.5)
    assert int(h.max()) > 1 << 32 and np.abs(want_c).max() < 1 << 31 and len(want_c) < len(c)
    _quantize_equals_the_lines(M, c, 0.5)


@pytest.mark.gpu
def test_pcd2bev_sum_bit_exact(golden):
    from lidargen.metrics import metric_utils as M

    g = golden("voxel")
    sets = [[synth_points(30000, seed=20 + 10 * k + i) for i in range(3)] for k in range(2)]
    sets[0][0][:6, :2] = [[30.0, 0.0], [-30.0, 0.0], [29.999998, 1.0], [-29.999998, 1.0],
                          [0.0, 29.999998], [0.025, 0.05]]
    vols = M.pcd2bev_sum("32", sets[0], sets[1])
    dev_sets = [[T(p).cuda() for p in s] for s in sets]
    dvols = M.pcd2bev_sum("32", dev_sets[0], dev_sets[1])
    for k in range(2):
        ref = np.zeros(tuple(g[f"bev{k}_shape"]), np.float32)
        ref.flat[g[f"bev{k}_idx"]] = g[f"bev{k}_cnt"]
        assert vols[k].dtype == np.float32 and np.array_equal(vols[k], ref)
        assert dvols[k].is_cuda and np.array_equal(dvols[k].cpu().numpy(), ref)
    # a sweep counts once per voxel however many points it has there; JSD of a set with itself is 0
    assert float(vols[0].max()) <= 3.0
    assert M.compute_jsd(dev_sets[0], dev_sets[0], "32") < 1e-12
    assert 0.0 < M.compute_jsd(dev_sets[0], dev_sets[1], "32") < 1.0
