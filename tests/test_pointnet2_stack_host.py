"""CPU tests of lidargen.ops.pointnet2.pointnet2_stack: the import lines, the modules' state_dict layout, the refusals by
name, and the oracle's own properties (tests/_pointnet2_stack_oracle.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointmlp_oracle as PO  # noqa: E402
import _pointnet2_stack_oracle as O  # noqa: E402


def test_import_lines_resolve():
    import lidargen.ops.pointnet2.pointnet2_stack  # noqa: F401
    from lidargen.ops.pointnet2.pointnet2_stack import pointnet2_modules, pointnet2_utils, voxel_pool_modules, voxel_query_utils
    from lidargen.ops.pointnet2.pointnet2_stack.pointnet2_modules import (StackPointnetFPModule, StackSAModuleMSG,  # noqa: F401
                                                                          build_local_aggregation_module)

    for name in ("ball_query", "grouping_operation", "QueryAndGroup", "farthest_point_sample", "furthest_point_sample",
                 "stack_farthest_point_sample", "three_nn", "three_interpolate", "BallQuery", "GroupingOperation",
                 "FarthestPointSampling", "StackFarthestPointSampling", "ThreeNN", "ThreeInterpolate",
                 "three_nn_for_vector_pool_by_two_step", "vector_pool_with_voxel_query_op"):
        assert hasattr(pointnet2_utils, name), name
    for name in ("voxel_query", "VoxelQuery", "VoxelQueryAndGrouping"):
        assert hasattr(voxel_query_utils, name), name
    assert hasattr(voxel_pool_modules, "NeighborVoxelSAModuleMSG")
    for name in ("VectorPoolLocalInterpolateModule", "VectorPoolAggregationModule", "VectorPoolAggregationModuleMSG"):
        assert hasattr(pointnet2_modules, name), name
    assert pointnet2_utils.farthest_point_sample is pointnet2_utils.furthest_point_sample


def _bn(prefix, c):
    return {prefix + ".weight": (c,), prefix + ".bias": (c,), prefix + ".running_mean": (c,), prefix + ".running_var": (c,),
            prefix + ".num_batches_tracked": ()}


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_state_dict_layout():
    from lidargen.ops.pointnet2.pointnet2_stack.pointnet2_modules import StackPointnetFPModule, StackSAModuleMSG
    from lidargen.ops.pointnet2.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG

    specs = [[16, 24, 32], [16, 8, 8, 40]]
    m = StackSAModuleMSG(radii=[0.4, 0.8], nsamples=[16, 32], mlps=[list(s) for s in specs], use_xyz=True)
    want = {}
    for k, spec in enumerate(specs):
        spec = [spec[0] + 3] + spec[1:]
        for j in range(len(spec) - 1):
            want[f"mlps.{k}.{3 * j}.weight"] = (spec[j + 1], spec[j], 1, 1)
            want.update(_bn(f"mlps.{k}.{3 * j + 1}", spec[j + 1]))
    assert _shapes(m) == want
    assert StackSAModuleMSG(radii=[1.0], nsamples=[4], mlps=[[5, 7]], use_xyz=False).mlps[0][0].weight.shape == (7, 5, 1, 1)

    fp = StackPointnetFPModule(mlp=[12, 20, 9])
    want = {"mlp.0.weight": (20, 12, 1, 1), "mlp.3.weight": (9, 20, 1, 1)}
    want.update(_bn("mlp.1", 20))
    want.update(_bn("mlp.4", 9))
    assert _shapes(fp) == want

    nv = NeighborVoxelSAModuleMSG(query_ranges=[[1, 1, 1], [2, 1, 1]], radii=[1.0, 2.0], nsamples=[4, 8],
                                  mlps=[[6, 10, 12], [6, 8, 5]])
    want = {}
    for k, (ci, cm, co) in enumerate([(6, 10, 12), (6, 8, 5)]):
        want[f"mlps_in.{k}.0.weight"] = (cm, ci, 1)
        want.update(_bn(f"mlps_in.{k}.1", cm))
        want[f"mlps_pos.{k}.0.weight"] = (cm, 3, 1, 1)
        want.update(_bn(f"mlps_pos.{k}.1", cm))
        want[f"mlps_out.{k}.0.weight"] = (co, cm, 1)
        want.update(_bn(f"mlps_out.{k}.1", co))
    assert _shapes(nv) == want


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def test_build_local_aggregation_module():
    from lidargen.ops.pointnet2.pointnet2_stack.pointnet2_modules import StackSAModuleMSG, build_local_aggregation_module

    layer, c = build_local_aggregation_module(16, _Cfg(NAME="StackSAModuleMSG", MLPS=[[16, 16], [16, 24]],
                                                       POOL_RADIUS=[0.4, 0.8], NSAMPLE=[16, 16]))
    assert isinstance(layer, StackSAModuleMSG) and c == 40 and layer.mlps[0][0].weight.shape == (16, 19, 1, 1)
    with pytest.raises(NotImplementedError, match="VectorPoolAggregationModuleMSG"):
        build_local_aggregation_module(16, _Cfg(NAME="VectorPoolAggregationModuleMSG"))
    with pytest.raises(NotImplementedError):
        build_local_aggregation_module(16, _Cfg(NAME="SomethingElse"))


def test_refusals_by_name():
    from lidargen.ops.pointnet2.pointnet2_stack import pointnet2_modules as PM
    from lidargen.ops.pointnet2.pointnet2_stack import pointnet2_utils as PU
    from lidargen.ops.pointnet2.pointnet2_stack import voxel_query_utils as VQ

    for name in ("three_nn_for_vector_pool_by_two_step", "vector_pool_with_voxel_query_op"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(PU, name)()
    for name in ("VectorPoolLocalInterpolateModule", "VectorPoolAggregationModule", "VectorPoolAggregationModuleMSG"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(PM, name)(16, None)
    xyz, cnt = torch.zeros(4, 3), torch.tensor([4], dtype=torch.int32)
    idx = torch.zeros(4, 2, dtype=torch.int32)
    cases = {
        "ball_query": lambda: PU.ball_query(1.0, 2, xyz, cnt, xyz, cnt),
        "grouping_operation": lambda: PU.grouping_operation(xyz, cnt, idx, cnt),
        "farthest_point_sample": lambda: PU.farthest_point_sample(xyz[None], 2),
        "stack_farthest_point_sample": lambda: PU.stack_farthest_point_sample(xyz, cnt, 2),
        "three_nn": lambda: PU.three_nn(xyz, cnt, xyz, cnt),
        "three_interpolate": lambda: PU.three_interpolate(xyz, torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3)),
        "voxel_query": lambda: VQ.voxel_query([1, 1, 1], 1.0, 2, xyz, xyz, torch.zeros(4, 4, dtype=torch.int32),
                                              torch.zeros(1, 2, 2, 2, dtype=torch.int32)),
    }
    for name, call in cases.items():
        with pytest.raises(NotImplementedError, match=name + ": CPU tensors are not built"):
            call()


def test_argument_checks_refuse_before_any_launch():
    """The C entries validate before anything is dereferenced or launched (callable without a GPU)."""
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    p = 4096
    EINVAL, EUNSUP = -1, -2
    big = h.lc_pn2_limit(0) + 1
    assert h.lc_pn2_limit(0) >= 128
    assert h.lc_pn2_scratch_elems(3, 10) == 2 * 4 + 10
    assert h.lc_pn2_ball_query_fwd(p, p, p, p, p, p, 1, 4, 4, 1.0, big, None) == EUNSUP
    assert h.lc_pn2_ball_query_fwd(p, p, p, p, p, p, 0, 4, 4, 1.0, 4, None) == EINVAL
    assert h.lc_pn2_ball_query_fwd(p, p, p, p, None, p, 1, 4, 4, 1.0, 4, None) == EINVAL
    assert h.lc_pn2_ball_query_fwd(p, p, p, p, p, p, 1, 4, 4, float("nan"), 4, None) == EINVAL
    assert h.lc_pn2_ball_query_fwd(None, None, None, None, None, None, 1, 4, 0, 1.0, 4, None) == 0     # no centres
    assert h.lc_pn2_group_fwd(p, p, p, p, p, p, 1, 4, 0, 4, 4, None) == EINVAL
    assert h.lc_pn2_group_fwd(p, p, p, p, p, p, h.lc_pn2_limit(1) + 1, 4, 2, 4, 4, None) == EUNSUP
    assert h.lc_pn2_three_nn_fwd(p, p, p, p, None, p, p, 1, 4, 4, None) == EINVAL
    assert h.lc_pn2_three_interpolate_fwd(p, p, p, p, 4, 0, 4, None) == EINVAL
    assert h.lc_pn2_three_interpolate_bwd(p, p, None, p, p, 4, 2, 4, None) == EINVAL
    assert h.lc_pn2_voxel_query_fwd(p, p, p, p, p, 4, 4, 1, 2, 2, 2, big, 1.0, 1, 1, 1, None) == EUNSUP
    assert h.lc_pn2_voxel_query_fwd(p, p, p, p, p, 4, 4, 1, 2, 2, 2, 4, 1.0, -1, 1, 1, None) == EINVAL
    assert h.lc_pn2_sa_first_fwd(p, p, p, p, p, p, p, p, p, p, 1, 4, 4, 0, 16, 4, 0, None) == EINVAL    # no input rows
    assert h.lc_pn2_sa_first_fwd(p, p, p, p, p, p, p + 4, p, p, p, 1, 4, 4, 8, 16, 4, 1, None) == EUNSUP  # wpk alignment
    assert h.lc_fps_stack_fwd(p, p, h.lc_pointmlp_limit(0) + 1, 4, 0, None) == EUNSUP
    assert h.lc_fps_stack_fwd(p, p, 0, 4, 0, None) == EINVAL


# ---- the oracle's own properties ---------------------------------------------------------------------------------------
def test_quarter_grid_distances_are_exact():
    rng = np.random.default_rng(0)
    p = rng.integers(0, 17, (300, 3)) / 4
    q = rng.integers(0, 17, (67, 3)) / 4
    on_sphere = 0
    for c in q:
        d32, d64 = O.sqdist(p, c, np.float32), O.sqdist(p, c, np.float64)
        assert np.array_equal(d32.astype(np.float64), d64)
        on_sphere += int((d64 == 1.25 * 1.25).sum())
    assert O.radius2(1.25) == 1.5625 and on_sphere > 0


def test_ball_query_rows():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [3, 0, 0], [9, 9, 9]], np.float32)
    raw = O.ball_query(xyz, [4, 1], np.array([[0, 0, 0], [9, 9, 8]], np.float32), [1, 1], 1.0, 4)
    assert raw.tolist() == [[0, 2, 0, 0], [-1, 0, 0, 0]]            # d == r2 is outside; pre-filled with the first hit
    idx, mask = O.finish_query(raw)
    assert idx.tolist() == [[0, 2, 0, 0], [0, 0, 0, 0]] and mask.tolist() == [False, True]
    assert O.ball_query(xyz, [4, 1], xyz[:1], [1, 0], 3.5, 2).tolist() == [[0, 1]]


def test_stacked_fps_rule():
    """The 1024-thread rule equals the batch kernel's rule (the largest power of two <= min(n, 1024)) for n >= 1024.  Below,
    the two trees order ties by the same key -- the bit reversal of k mod bs first, and thread t of the smaller block keeps
    the smaller of k, k + bs, which is also the smaller 10-bit reversal -- so no tie separates them either: clouds on a
    3 x 3 x 3 lattice (ties at every pick) give the same sequence under both."""
    rng = np.random.default_rng(5)
    for n in (1024, 1025, 2500):
        c = rng.integers(0, 9, (n, 3)).astype(np.float32) / 4
        assert np.array_equal(O.fps_stack(c, [n], [24]), PO.fps(c, 24))
    for n in (1, 2, 3, 5, 6, 7, 9, 12, 33, 300, 1023):
        c = rng.integers(0, 3, (n, 3)).astype(np.float32)
        m = min(n + 2, 16)
        assert np.array_equal(O.fps_stack(c, [n], [m]), PO.fps(c, m)), n
    c = rng.random((12, 3)).astype(np.float32)
    both = O.fps_stack(np.concatenate([c, c + 7]), [12, 12], [5, 3])
    assert np.array_equal(both[:5], PO.fps(c, 5)) and np.array_equal(both[5:] - 12, PO.fps(c + 7, 3))


def test_three_nn_and_interpolation_oracle():
    known = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5]], np.float32)
    d2, idx = O.three_nn(np.array([[1, 0, 0], [5, 5, 4]], np.float32), [1, 1], known, [4, 1])
    assert idx.tolist() == [[1, 2, 0], [4, 4, 4]]                    # equal distances keep index order; unfilled: the start
    assert d2[0].tolist() == [0, 0, 1] and d2[1, 0] == 1 and np.isinf(d2[1, 1:]).all()
    f = np.arange(10, dtype=np.float32).reshape(5, 2)
    w = np.array([[0.5, 0.25, 0.25], [1, 0, 0]], np.float32)
    out = O.three_interpolate(f, np.array([[1, 2, 0], [4, 7, -1]]), w)
    assert out.tolist() == [[2.0, 3.0], [8.0, 9.0]]
    g = O.three_interpolate_bwd(np.ones((2, 2), np.float32), np.array([[1, 2, 0], [4, 7, -1]]), w, 5)
    assert g[:, 0].tolist() == [0.25, 0.5, 0.25, 0, 1]


def test_group_oracle_round_trip():
    f = np.arange(12, dtype=np.float32).reshape(6, 2)
    idx = np.array([[0, 3], [1, -1], [0, 2]])
    out = O.group(f, [4, 2], idx, [2, 1])
    assert out.shape == (3, 2, 2) and out[0, :, 1].tolist() == [6, 7] and out[1, :, 1].tolist() == [0, 0]
    assert out[2, :, 0].tolist() == [8, 9] and out[2, :, 1].tolist() == [0, 0]      # 2 is past the second cloud's end
    g = O.group_bwd(np.ones((3, 2, 2), np.float32), 6, [4, 2], idx, [2, 1])
    assert g[:, 0].tolist() == [1, 1, 0, 1, 1, 0]
