"""Mirror of the reference's `lidargen/ops/pointnet2/pointnet2_batch/pointnet2_utils.py` for the one operator the
evaluator reaches: `furthest_point_sample` / `farthest_point_sample` (the import line of extractor/pointmlp.py).  The kernel
reproduces the reference's `farthest_point_sampling_kernel` index for index (lidarcrafter_amd.ops_pointmlp.fps, DESIGN.md
section 5o).  Ball query, grouping, three-NN, interpolation and gather are not built and say so by name."""
import torch

from lidarcrafter_amd import ops_pointmlp as KM


def furthest_point_sample(xyz: torch.Tensor, npoint: int) -> torch.Tensor:
    """xyz (B, N, 3) contiguous float32 on the device -> int32 (B, npoint), the farthest-point sequence from index 0."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise NotImplementedError("furthest_point_sample: CPU tensors are not built -- `xyz` must be a CUDA(HIP) tensor")
    assert xyz.is_contiguous()
    return KM.fps(xyz.detach(), int(npoint))


farthest_point_sample = furthest_point_sample


def _not_built(name, what):
    def op(*args, **kwargs):
        raise NotImplementedError(f"pointnet2_utils.{name}: {what} is not built (the PointMLP extractor needs farthest "
                                  "point sampling only)")

    op.__name__ = name
    return op


gather_operation = _not_built("gather_operation", "gather")
three_nn = _not_built("three_nn", "three-NN")
three_interpolate = _not_built("three_interpolate", "interpolate")
grouping_operation = _not_built("grouping_operation", "grouping")
ball_query = _not_built("ball_query", "ball query")


class QueryAndGroup(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("pointnet2_utils.QueryAndGroup: ball query and grouping are not built")


class GroupAll(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("pointnet2_utils.GroupAll: grouping is not built")
