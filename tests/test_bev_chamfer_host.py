"""CPU-side checks of the Minimum Matching Distance feature (csrc/bev_chamfer.hip, lc_chamfer2d_fwd, metric_utils.pcd2bev_bin,
eval_utils.compute_mmd): the numpy oracle the GPU tests compare against (tests/_bev_chamfer_oracle.py) is itself checked --
its exact integer value against a scipy cKDTree nearest neighbour on the integer cells, its float32 restatement of the
reference kernel against that exact value within the derived tolerance --; every new C entry refuses bad arguments before
any launch; the Python layers refuse CPU tensors and dist='emd'."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bev_chamfer_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"32": ((-30, 30), (-30, 30)), "64": ((-50, 50), (-50, 50)), "120x40": ((-30, 30), (-10, 10))}


def _cells(name, seed, count):
    xr, yr = GRIDS[name]
    nx, ny, _ = O.grid(xr, yr, 0.5)
    return [O.bev_cells(p, xr, yr, 0.5) for p in O.sweeps(seed, count, xr, yr)], nx, ny


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_exact_value_is_the_kdtree_nearest_neighbour(name):
    """Independent of the restatement: the cells scaled to (i ny, j nx) are integer points whose Euclidean nearest
    neighbour distance, squared and rounded, is the weighted integer distance."""
    from scipy.spatial import cKDTree

    cells, nx, ny = _cells(name, 3, 4)
    assert (nx, ny) == {"32": (120, 120), "64": (200, 200), "120x40": (120, 40)}[name]
    scale = np.array([ny, nx], np.float64)
    for r in cells[:2]:
        for s in cells[2:]:
            dr, _ = cKDTree(s * scale).query(r * scale)
            ds, _ = cKDTree(r * scale).query(s * scale)
            want = (int(np.rint(dr * dr).sum()), int(np.rint(ds * ds).sum()))
            assert O.exact_sums(r, s, nx, ny) == want
            cd = (want[0] / len(r) + want[1] / len(s)) / (2.0 * nx * nx * ny * ny)
            assert O.exact_cd(r, s, nx, ny) == pytest.approx(cd, rel=1e-15)


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_float32_restatement_is_within_the_tolerance_of_the_exact_value(name):
    xr, yr = GRIDS[name]
    clouds = O.sweeps(5, 5, xr, yr)
    nx, ny, _ = O.grid(xr, yr, 0.5)
    cells = [O.bev_cells(p, xr, yr, 0.5) for p in clouds]
    (sets,) = O.bev_bin(xr, yr, 0.5, clouds)
    worst = 0.0
    for i in range(2):
        got = O.pairwise_cd_batch(sets[i], sets[2:])
        for g, s in zip(got, cells[2:]):
            want = O.exact_cd(cells[i], s, nx, ny)
            worst = max(worst, abs(g - want) / want)
    print(f"{name}: worst relative error of the float32 restatement {worst:.2e}, tolerance {O.tolerance(nx, ny):.2e}")
    assert worst <= O.tolerance(nx, ny)


def test_oracle_cells_and_edge_points():
    xr, yr = GRIDS["32"]
    p = O.sweeps(0, 1, xr, yr)[0][:7]     # the special points alone
    c = O.bev_cells(p, xr, yr, 0.5)
    # on a bound / outside: dropped; the cell-edge point belongs to the cell it starts; two points share cell (60, 60)
    assert c.tolist() == [[60, 60], [62, 57]]
    (sets,) = O.pcd2bev_bin("32", [p])
    assert sets[0].dtype == np.float32 and np.array_equal(sets[0], (c / 120.0).astype(np.float32))
    (empty,) = O.pcd2bev_bin("32", [np.full((5, 3), 99.0, np.float32)])
    assert empty[0].shape == (0, 2)
    d, i = O.nm_distance(np.zeros((1, 2), np.float32), np.array([[1, 0], [0, 1], [-1, 0]], np.float32))
    assert d.tolist() == [1.0] and i.tolist() == [0]          # first of three equal minima


def test_c_entries_refuse_bad_arguments():
    """Every new entry validates before any launch (callable without a GPU)."""
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    EINVAL, EUNSUP = -1, -2
    p = 4096
    assert h.lc_bev_grid_supported(120, 120) == 0 and h.lc_bev_grid_supported(200, 200) == 0
    assert h.lc_bev_grid_supported(24, 40) == 0
    assert h.lc_bev_grid_supported(0, 5) == EINVAL and h.lc_bev_grid_supported(5, -1) == EINVAL
    assert h.lc_bev_grid_supported(216, 215) == EUNSUP        # 2 nx^2 ny^2 >= 2^32 (46440 cells)
    assert h.lc_bev_grid_supported(70000, 2) == EUNSUP
    assert h.lc_bev_grid_supported(2000, 20) == EUNSUP        # representable, but a strip does not fit the LDS

    def c2d(a=p, b=p, d1=p, i1=p, d2=p, i2=p, B=1, N=4, M=4):
        return h.lc_chamfer2d_fwd(a, b, B, N, M, d1, i1, d2, i2, None)

    for null in ("a", "b", "d1", "i1", "d2", "i2"):
        assert c2d(**{null: None}) == EINVAL, null
    assert c2d(B=0) == EINVAL and c2d(N=0) == EINVAL and c2d(M=-1) == EINVAL and c2d(B=65536) == EUNSUP

    def occ(pts=p, offs=p, bits=p, counts=p, n=2, mx=10, stride=3, voxel=0.5, nx=120, ny=120):
        return h.lc_bev_occupancy_bits(pts, stride, offs, n, mx, -30.0, 30.0, -30.0, 30.0, voxel, -60, -60, nx, ny, bits,
                                       counts, None)

    for null in ("pts", "offs", "bits", "counts"):
        assert occ(**{null: None}) == EINVAL, null
    assert occ(n=0) == EINVAL and occ(mx=-1) == EINVAL and occ(stride=1) == EINVAL and occ(voxel=0.0) == EINVAL
    assert occ(voxel=float("nan")) == EINVAL and occ(nx=0) == EINVAL and occ(ny=0) == EINVAL
    assert occ(nx=1 << 30, ny=1 << 10) == EUNSUP

    def lists(bits=p, offs=p, cells=p, n=2, nx=120, ny=120):
        return h.lc_bev_cell_lists(bits, n, nx, ny, offs, cells, None)

    for null in ("bits", "offs", "cells"):
        assert lists(**{null: None}) == EINVAL, null
    assert lists(n=0) == EINVAL and lists(nx=0) == EINVAL and lists(ny=-3) == EINVAL
    assert lists(nx=1 << 20, ny=1 << 20) == EUNSUP

    def dt(bits=p, tmp=p, out=p, n=2, nx=120, ny=120, ld=16):
        return h.lc_bev_distance_transform(bits, n, nx, ny, tmp, out, ld, None)

    for null in ("bits", "tmp", "out"):
        assert dt(**{null: None}) == EINVAL, null
    assert dt(n=0) == EINVAL and dt(nx=0) == EINVAL and dt(ld=1) == EINVAL
    assert dt(nx=70000, ny=2) == EUNSUP and dt(nx=216, ny=215) == EUNSUP and dt(n=65536, ld=65536) == EUNSUP

    def ps(cells=p, offs=p, d=p, a=p, nI=2, ld=16, nJ=3):
        return h.lc_bev_pair_sums(cells, offs, nI, d, ld, nJ, a, None)

    for null in ("cells", "offs", "d", "a"):
        assert ps(**{null: None}) == EINVAL, null
    assert ps(nI=0) == EINVAL and ps(nJ=0) == EINVAL and ps(ld=2) == EINVAL and ps(nI=65536) == EUNSUP

    def cb(ars=p, asr=p, cr=p, cs=p, mn=p, am=p, mat=None, nI=2, nJ=3, j0=0, nx=120, ny=120, ldm=3):
        return h.lc_bev_chamfer_combine(ars, asr, cr, cs, nI, nJ, j0, 1, nx, ny, mn, am, mat, ldm, None)

    for null in ("ars", "asr", "cr", "cs", "mn", "am"):
        assert cb(**{null: None}) == EINVAL, null
    assert cb(nI=0) == EINVAL and cb(nJ=0) == EINVAL and cb(j0=-1) == EINVAL and cb(mat=p, j0=1, ldm=3) == EINVAL
    assert cb(nx=0) == EINVAL and cb(nx=70000, ny=2) == EUNSUP


def test_python_layers_refuse_cpu_tensors():
    from lidarcrafter_amd import ops
    from lidargen.metrics import eval_utils, metric_utils
    from lidargen.metrics.chamfer import bev_min_matching, chamfer_2DDist

    a = torch.zeros(1, 8, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.chamfer2d(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chamfer_2DDist()(a, a)
    cloud = torch.rand(50, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bev_chamfer_min([cloud], [cloud], (-30, 30), (-30, 30), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bev_chamfer_min([cloud], [cloud], (0, 35000), (-1, 1), 0.5)       # refused before the grid is
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bev_cells([cloud], (-30, 30), (-30, 30), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric_utils.pcd2bev_bin("32", [cloud])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bev_min_matching([cloud], [cloud], (-30, 30), (-30, 30), route="literal")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_utils.compute_mmd([cloud], [cloud], "32")
    meta = torch.zeros(1, 8, 2, device="meta")
    with pytest.raises(RuntimeError):
        ops.chamfer2d(meta, meta)


def test_compute_mmd_refuses_emd_and_evaluate_points_at_it(capsys):
    from lidargen.metrics import eval_utils

    with pytest.raises(NotImplementedError, match="emd"):
        eval_utils.compute_mmd([], [], "32", dist="emd")
    with pytest.raises(AssertionError):
        eval_utils.compute_mmd([], [], "32", dist="l2")
    assert "Evaluating (MMD) ..." in capsys.readouterr().out
    with pytest.raises(NotImplementedError, match="compute_mmd"):
        eval_utils.evaluate([], [], ["mmd"], "32")


def test_symbols_in_header_binding_and_build():
    from lidarcrafter_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "lidarcrafter_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    h = _lib.lib()
    for name in ("lc_chamfer2d_fwd", "lc_bev_grid_supported", "lc_bev_occupancy_bits", "lc_bev_cell_lists",
                 "lc_bev_distance_transform", "lc_bev_pair_sums", "lc_bev_chamfer_combine"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(h, name)
    assert "bev_chamfer.hip" in build.SOURCES
    assert h.lc_abi_version() == 6 and _lib.ABI_VERSION == 6
