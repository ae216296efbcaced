"""Mirror of the reference's `lidargen/ops/pointnet2/pointnet2_stack/pointnet2_utils.py` on the HIP kernels of
csrc/pointnet2_stack.hip (lidarcrafter_amd.ops_pointnet2): the reference's names, signatures, asserts
and return types.  Stacked tensors: `xyz` (N1 + N2 + ..., 3) with `xyz_batch_cnt` (batch_size) int32.  CPU tensors and the
vector-pool family are not built and say so by name; so does the backward pass of `grouping_operation`."""
import torch
import torch.nn as nn
from torch.autograd import Function

from lidarcrafter_amd import ops_pointmlp as KM
from lidarcrafter_amd import ops_pointnet2 as KP


def _device_only(who, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise NotImplementedError(f"pointnet2_stack.{who}: CPU tensors are not built -- every operand must be a "
                                      "CUDA(HIP) tensor, there is no CPU fallback on the hot path")


def _cnt(t):
    return t.detach().to(torch.int32).contiguous()


class BallQuery(Function):

    @staticmethod
    def forward(ctx, radius: float, nsample: int, xyz: torch.Tensor, xyz_batch_cnt: torch.Tensor,
                new_xyz: torch.Tensor, new_xyz_batch_cnt):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3) and their counts -> idx (M1 + M2 ..., nsample) int32 local
        indices with the empty rows set to 0, empty_ball_mask (M1 + M2 ...) bool."""
        _device_only("ball_query", xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        assert new_xyz.is_contiguous()
        assert new_xyz_batch_cnt.is_contiguous()
        assert xyz.is_contiguous()
        assert xyz_batch_cnt.is_contiguous()

        idx = KP.ball_query(radius, nsample, xyz.detach().float(), _cnt(xyz_batch_cnt), new_xyz.detach().float(),
                            _cnt(new_xyz_batch_cnt))
        empty_ball_mask = (idx[:, 0] == -1)
        idx[empty_ball_mask] = 0

        ctx.mark_non_differentiable(idx)
        ctx.mark_non_differentiable(empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None


ball_query = BallQuery.apply


class GroupingOperation(Function):

    @staticmethod
    def forward(ctx, features: torch.Tensor, features_batch_cnt: torch.Tensor,
                idx: torch.Tensor, idx_batch_cnt: torch.Tensor):
        """features (N1 + N2 ..., C), idx (M1 + M2 ..., nsample) local indices -> (M1 + M2 ..., C, nsample)."""
        _device_only("grouping_operation", features, features_batch_cnt, idx, idx_batch_cnt)
        assert features.is_contiguous()
        assert features_batch_cnt.is_contiguous()
        assert idx.is_contiguous()
        assert idx_batch_cnt.is_contiguous()

        assert features.shape[0] == features_batch_cnt.sum(), \
            'features: %s, features_batch_cnt: %s' % (str(features.shape), str(features_batch_cnt))
        assert idx.shape[0] == idx_batch_cnt.sum(), \
            'idx: %s, idx_batch_cnt: %s' % (str(idx.shape), str(idx_batch_cnt))

        N = features.shape[0]
        B = idx_batch_cnt.shape[0]
        f_cnt, i_cnt, idx32 = _cnt(features_batch_cnt), _cnt(idx_batch_cnt), idx.detach().to(torch.int32).contiguous()
        output = KP.group(features.detach().float(), f_cnt, idx32, i_cnt)

        ctx.for_backwards = (B, N, idx32, f_cnt, i_cnt)
        return output

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        raise NotImplementedError("pointnet2_stack.grouping_operation: the backward pass is not built -- call it under "
                                  "torch.no_grad() or on features that do not require grad")


grouping_operation = GroupingOperation.apply


class QueryAndGroup(nn.Module):
    def __init__(self, radius: float, nsample: int, use_xyz: bool = True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz: torch.Tensor, xyz_batch_cnt: torch.Tensor,
                new_xyz: torch.Tensor, new_xyz_batch_cnt: torch.Tensor,
                features: torch.Tensor = None):
        """-> new_features (M1 + M2 ..., C [+ 3], nsample), idx (M1 + M2 ..., nsample)."""
        assert xyz.shape[0] == xyz_batch_cnt.sum(), 'xyz: %s, xyz_batch_cnt: %s' % (str(xyz.shape), str(new_xyz_batch_cnt))
        assert new_xyz.shape[0] == new_xyz_batch_cnt.sum(), \
            'new_xyz: %s, new_xyz_batch_cnt: %s' % (str(new_xyz.shape), str(new_xyz_batch_cnt))

        idx, empty_ball_mask = ball_query(self.radius, self.nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        grouped_xyz = grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)  # (M1 + M2, 3, nsample)
        grouped_xyz -= new_xyz.unsqueeze(-1)
        grouped_xyz[empty_ball_mask] = 0

        if features is not None:
            grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
            grouped_features[empty_ball_mask] = 0
            if self.use_xyz:
                new_features = torch.cat([grouped_xyz, grouped_features], dim=1)
            else:
                new_features = grouped_features
        else:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            new_features = grouped_xyz

        return new_features, idx


class FarthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz: torch.Tensor, npoint: int):
        """xyz (B, N, 3) -> (B, npoint) int32: the batch kernel (lidarcrafter_amd.ops_pointmlp.fps)."""
        _device_only("farthest_point_sample", xyz)
        assert xyz.is_contiguous()
        return KM.fps(xyz.detach().float(), int(npoint))

    @staticmethod
    def backward(xyz, a=None):
        return None, None


farthest_point_sample = furthest_point_sample = FarthestPointSampling.apply


class StackFarthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, xyz_batch_cnt, npoint):
        """xyz (N1 + N2 + ..., 3), xyz_batch_cnt [N1, N2, ...], npoint an int, a list or a tensor ->
        (npoint.sum()) int32 global rows."""
        _device_only("stack_farthest_point_sample", xyz)
        assert xyz.is_contiguous() and xyz.shape[1] == 3

        batch_size = xyz_batch_cnt.__len__()
        if not isinstance(npoint, torch.Tensor):
            if not isinstance(npoint, list):
                npoint = [npoint for i in range(batch_size)]
            npoint = torch.tensor(npoint, device=xyz.device).int()
        counts = xyz_batch_cnt.tolist() if isinstance(xyz_batch_cnt, torch.Tensor) else list(xyz_batch_cnt)
        return KP.fps_stack(xyz.detach().float(), counts, npoint.tolist())

    @staticmethod
    def backward(xyz, a=None):
        return None, None


stack_farthest_point_sample = StackFarthestPointSampling.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, unknown_batch_cnt, known, known_batch_cnt):
        """unknown (N1 + N2 ..., 3), known (M1 + M2 ..., 3) -> dist (N1 + N2 ..., 3) l2 distances to the three nearest
        known points of the same cloud, idx (N1 + N2 ..., 3) int32 in [0, M1 + M2 + ...)."""
        _device_only("three_nn", unknown, unknown_batch_cnt, known, known_batch_cnt)
        assert unknown.shape.__len__() == 2 and unknown.shape[1] == 3
        assert known.shape.__len__() == 2 and known.shape[1] == 3
        assert unknown_batch_cnt.__len__() == known_batch_cnt.__len__()

        dist2, idx = KP.three_nn(unknown.detach().float().contiguous(), _cnt(unknown_batch_cnt),
                                 known.detach().float().contiguous(), _cnt(known_batch_cnt))
        ctx.mark_non_differentiable(idx)
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):

    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor):
        """features (M1 + M2 ..., C), idx / weight [N1 + N2 ..., 3] -> (N1 + N2 ..., C)."""
        _device_only("three_interpolate", features, idx, weight)
        assert idx.shape[0] == weight.shape[0] and idx.shape[1] == weight.shape[1] == 3

        idx32, w = idx.detach().to(torch.int32).contiguous(), weight.detach().float().contiguous()
        ctx.three_interpolate_for_backward = (idx32, w, features.shape[0])
        return KP.three_interpolate(features.detach().float().contiguous(), idx32, w)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        """grad_out (N1 + N2 ..., C) -> grad_features (M1 + M2 ..., C)."""
        idx, weight, M = ctx.three_interpolate_for_backward
        grad_features = KP.three_interpolate_bwd(grad_out.detach().float().contiguous(), idx, weight, M)
        return grad_features, None, None


three_interpolate = ThreeInterpolate.apply


def _not_built(name):
    def op(*args, **kwargs):
        raise NotImplementedError(f"pointnet2_stack.pointnet2_utils.{name}: the vector-pool family is not built")

    op.__name__ = name
    return op


three_nn_for_vector_pool_by_two_step = _not_built("three_nn_for_vector_pool_by_two_step")
vector_pool_with_voxel_query_op = _not_built("vector_pool_with_voxel_query_op")
