"""Mirror of the reference's `lidargen/ops/pointnet2/pointnet2_stack/voxel_query_utils.py` on the HIP voxel query of
csrc/pointnet2_stack.hip (lidarcrafter_amd.ops_pointnet2.voxel_query)."""
import torch
import torch.nn as nn
from torch.autograd import Function

from lidarcrafter_amd import ops_pointnet2 as KP

from . import pointnet2_utils


class VoxelQuery(Function):

    @staticmethod
    def forward(ctx, max_range, radius: float, nsample: int, xyz: torch.Tensor,
                new_xyz: torch.Tensor, new_coords: torch.Tensor, point_indices: torch.Tensor):
        """max_range (z, y, x) cells to each side, new_coords (M1 + M2, 4) [batch_id, z, y, x], point_indices
        (batch_size, Z, Y, X) the row of `xyz` in every voxel or -1 -> idx (M1 + M2, nsample) int32 global rows with the
        empty rows set to 0, empty_ball_mask (M1 + M2)."""
        pointnet2_utils._device_only("voxel_query", xyz, new_xyz, new_coords, point_indices)
        assert new_xyz.is_contiguous()
        assert xyz.is_contiguous()
        assert new_coords.is_contiguous()
        assert point_indices.is_contiguous()

        idx = KP.voxel_query(max_range, radius, nsample, xyz.detach().float(), new_xyz.detach().float(),
                             new_coords.detach().to(torch.int32), point_indices.detach().to(torch.int32))
        empty_ball_mask = (idx[:, 0] == -1)
        idx[empty_ball_mask] = 0
        ctx.mark_non_differentiable(idx)
        ctx.mark_non_differentiable(empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None, None


voxel_query = VoxelQuery.apply


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range: int, radius: float, nsample: int):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def forward(self, new_coords: torch.Tensor, xyz: torch.Tensor, xyz_batch_cnt: torch.Tensor,
                new_xyz: torch.Tensor, new_xyz_batch_cnt: torch.Tensor,
                features: torch.Tensor, voxel2point_indices: torch.Tensor):
        """-> grouped_features (M1 + M2, C, nsample), grouped_xyz (M1 + M2, 3, nsample), empty_ball_mask (M1 + M2).  As in
        the reference the global rows are made local per cloud through a (batch_size, -1, nsample) view: every cloud has
        the same number of centres."""
        assert xyz.shape[0] == xyz_batch_cnt.sum(), 'xyz: %s, xyz_batch_cnt: %s' % (str(xyz.shape), str(new_xyz_batch_cnt))
        assert new_coords.shape[0] == new_xyz_batch_cnt.sum(), \
            'new_coords: %s, new_xyz_batch_cnt: %s' % (str(new_coords.shape), str(new_xyz_batch_cnt))
        batch_size = xyz_batch_cnt.shape[0]

        idx1, empty_ball_mask1 = voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords,
                                             voxel2point_indices)

        idx1 = idx1.view(batch_size, -1, self.nsample)
        count = 0
        for bs_idx in range(batch_size):
            idx1[bs_idx] -= count
            count += xyz_batch_cnt[bs_idx]
        idx1 = idx1.view(-1, self.nsample)
        idx1[empty_ball_mask1] = 0

        idx = idx1
        empty_ball_mask = empty_ball_mask1

        grouped_xyz = pointnet2_utils.grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_features = pointnet2_utils.grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)

        return grouped_features, grouped_xyz, empty_ball_mask
