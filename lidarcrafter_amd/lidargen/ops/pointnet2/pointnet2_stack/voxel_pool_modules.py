"""Mirror of the reference's `lidargen/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py`: `NeighborVoxelSAModuleMSG`
with the reference's constructor arguments and state_dict keys (`mlps_in.{k}.0.weight`, `mlps_in.{k}.1.*`, `mlps_pos...`,
`mlps_out...`).  Operator route only: the voxel query and the grouping run on the HIP kernels of csrc/pointnet2_stack.hip,
the layers are torch's."""
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import voxel_query_utils


class NeighborVoxelSAModuleMSG(nn.Module):

    def __init__(self, *, query_ranges: List[List[int]], radii: List[float],
                 nsamples: List[int], mlps: List[List[int]], use_xyz: bool = True, pool_method='max_pool'):
        """query_ranges[k] = (z, y, x) cells to each side, mlps[k] = [C_in, C_mid, C_out]."""
        super().__init__()

        assert len(query_ranges) == len(nsamples) == len(mlps)

        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for i in range(len(query_ranges)):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(query_ranges[i], radii[i], nsamples[i]))
            c_in, c_mid, c_out = mlps[i][0], mlps[i][1], mlps[i][2]
            self.mlps_in.append(nn.Sequential(nn.Conv1d(c_in, c_mid, kernel_size=1, bias=False), nn.BatchNorm1d(c_mid)))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, c_mid, kernel_size=1, bias=False), nn.BatchNorm2d(c_mid)))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(c_mid, c_out, kernel_size=1, bias=False), nn.BatchNorm1d(c_out),
                                               nn.ReLU()))

        self.relu = nn.ReLU()
        self.pool_method = pool_method

        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d) or isinstance(m, nn.Conv1d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d) or isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt,
                new_coords, features, voxel2point_indices):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), new_coords (M1 + M2 ..., 4) [batch, x, y, z], features
        (N1 + N2 ..., C), voxel2point_indices (B, Z, Y, X) -> new_features (M1 + M2 ..., sum_k mlps[k][-1])."""
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()      # [batch, z, y, x]
        new_features_list = []
        for k in range(len(self.groupers)):
            features_in = features.permute(1, 0).unsqueeze(0)       # (1, C, N1 + N2)
            features_in = self.mlps_in[k](features_in)
            features_in = features_in.permute(0, 2, 1).contiguous()
            features_in = features_in.view(-1, features_in.shape[-1])   # (N1 + N2, C)
            grouped_features, grouped_xyz, empty_ball_mask = self.groupers[k](
                new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in, voxel2point_indices
            )
            grouped_features[empty_ball_mask] = 0

            grouped_features = grouped_features.permute(1, 0, 2).unsqueeze(dim=0)   # (1, C, M1 + M2, nsample)
            grouped_xyz = grouped_xyz - new_xyz.unsqueeze(-1)
            grouped_xyz[empty_ball_mask] = 0
            grouped_xyz = grouped_xyz.permute(1, 0, 2).unsqueeze(0)                 # (1, 3, M1 + M2, nsample)
            position_features = self.mlps_pos[k](grouped_xyz)
            new_features = grouped_features + position_features
            new_features = self.relu(new_features)

            if self.pool_method == 'max_pool':
                new_features = F.max_pool2d(
                    new_features, kernel_size=[1, new_features.size(3)]
                ).squeeze(dim=-1)  # (1, C, M1 + M2 ...)
            elif self.pool_method == 'avg_pool':
                new_features = F.avg_pool2d(
                    new_features, kernel_size=[1, new_features.size(3)]
                ).squeeze(dim=-1)  # (1, C, M1 + M2 ...)
            else:
                raise NotImplementedError

            new_features = self.mlps_out[k](new_features)
            new_features = new_features.squeeze(dim=0).permute(1, 0)  # (M1 + M2 ..., C)
            new_features_list.append(new_features)

        new_features = torch.cat(new_features_list, dim=1)
        return new_features
