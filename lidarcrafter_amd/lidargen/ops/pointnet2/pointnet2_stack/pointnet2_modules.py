"""Mirror of the reference's `lidargen/ops/pointnet2/pointnet2_stack/pointnet2_modules.py`: `StackSAModuleMSG`,
`StackPointnetFPModule` and `build_local_aggregation_module`, with the reference's constructor arguments and state_dict keys
(`mlps.{k}.{3j}.weight`, `mlps.{k}.{3j+1}.*`, `mlp.{3j}.weight`, ...).

`StackSAModuleMSG.forward` has two routes:
  * fused -- eval mode under torch.no_grad() with pool_method='max_pool': BatchNorm folded on the host in float64, the
    ball query, the gathered first layer (the grouped tensor is never written), the remaining layers on the dense engine
    and the group maximum written straight into its columns of the result.  LC_PN2_FUSED=0 turns it off.
  * operator -- everything else (training, grad mode, avg_pool, the switch): the reference's formulation over this package's
    operators and torch layers.  Forward only: `grouping_operation` has no backward pass in this build, `.backward()`
    through it raises NotImplementedError by name.
The vector-pool modules are not built and say so by name."""
import os
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from lidarcrafter_amd import ops_pointmlp as KM
from lidarcrafter_amd import ops_pointnet2 as KP

from . import pointnet2_utils


def fused_enabled() -> bool:
    """The A/B switch of the fused route: LC_PN2_FUSED=0 sends every call down the operator route."""
    return os.environ.get("LC_PN2_FUSED", "1") != "0"


def build_local_aggregation_module(input_channels, config):
    local_aggregation_name = config.get('NAME', 'StackSAModuleMSG')

    if local_aggregation_name == 'StackSAModuleMSG':
        mlps = config.MLPS
        for k in range(len(mlps)):
            mlps[k] = [input_channels] + mlps[k]
        cur_layer = StackSAModuleMSG(
            radii=config.POOL_RADIUS, nsamples=config.NSAMPLE, mlps=mlps, use_xyz=True, pool_method='max_pool',
        )
        num_c_out = sum([x[-1] for x in mlps])
    elif local_aggregation_name == 'VectorPoolAggregationModuleMSG':
        raise NotImplementedError("build_local_aggregation_module: NAME == 'VectorPoolAggregationModuleMSG' is not built "
                                  "(the vector-pool family)")
    else:
        raise NotImplementedError

    return cur_layer, num_c_out


def _shared_mlp(spec):
    layers = []
    for k in range(len(spec) - 1):
        layers.extend([
            nn.Conv2d(spec[k], spec[k + 1], kernel_size=1, bias=False),
            nn.BatchNorm2d(spec[k + 1]),
            nn.ReLU()
        ])
    return nn.Sequential(*layers)


class StackSAModuleMSG(nn.Module):

    def __init__(self, *, radii: List[float], nsamples: List[int], mlps: List[List[int]],
                 use_xyz: bool = True, pool_method='max_pool'):
        """radii, nsamples, mlps: one entry per scale; mlps[k] = [C_in, C_1, ..., C_out] (C_in grows by 3 in place when
        use_xyz, as in the reference)."""
        super().__init__()

        assert len(radii) == len(nsamples) == len(mlps)

        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for i in range(len(radii)):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz))
            mlp_spec = mlps[i]
            if use_xyz:
                mlp_spec[0] += 3
            self.mlps.append(_shared_mlp(mlp_spec))
        self.pool_method = pool_method

        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    # ---- the fused route ---------------------------------------------------------------------------------------------
    def _fingerprint(self):
        fp = []
        for seq in self.mlps:
            for m in seq:
                for t in list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)):
                    fp.append((t.data_ptr(), t._version, str(t.device), t.dtype))
        return tuple(fp)

    def packed(self, dev):
        """[[(packed weight, bias, Co) per layer] per scale] on `dev`: BatchNorm folded in float64 on the host; folded and
        packed again when any parameter or buffer changed."""
        from lidargen.metrics.extractor.pointnet import fold_bn

        key = (self._fingerprint(), str(dev))
        hit = self.__dict__.get("_lc_packed")
        if hit is None or hit[0] != key:
            scales = []
            with torch.no_grad():
                for seq in self.mlps:
                    layers = []
                    for j in range(0, len(seq), 3):
                        conv, bn = seq[j], seq[j + 1]
                        bias = conv.bias if conv.bias is not None else torch.zeros(conv.weight.shape[0],
                                                                                    device=conv.weight.device)
                        w, b = fold_bn(conv.weight, bias, bn)
                        layers.append((KM.pack_weight(w.cpu().contiguous()).to(dev), b.to(dev).contiguous(), w.shape[0]))
                    scales.append(layers)
            hit = (key, scales)
            self.__dict__["_lc_packed"] = hit
        return hit[1]

    def _fused_ok(self, xyz, new_xyz, features):
        if self.training or torch.is_grad_enabled() or self.pool_method != 'max_pool' or not fused_enabled():
            return False
        if any(isinstance(bn, nn.BatchNorm2d) and bn.running_var is None for seq in self.mlps for bn in seq):
            return False
        return all(t is None or (isinstance(t, torch.Tensor) and t.is_cuda) for t in (xyz, new_xyz, features))

    def _forward_fused(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        dev = xyz.device
        scales = self.packed(dev)
        xyz32, new32 = xyz.detach().float().contiguous(), new_xyz.detach().float().contiguous()
        feat32 = None if features is None else features.detach().float().contiguous()
        xc, nc = pointnet2_utils._cnt(xyz_batch_cnt), pointnet2_utils._cnt(new_xyz_batch_cnt)
        M = new32.shape[0]
        out = torch.empty((M, sum(layers[-1][2] for layers in scales)), device=dev, dtype=torch.float32)
        col = 0
        for grouper, layers in zip(self.groupers, scales):
            if feat32 is None:
                assert grouper.use_xyz, "Cannot have not features and not use xyz as a feature!"
            if M:
                idx = KP.ball_query(grouper.radius, grouper.nsample, xyz32, xc, new32, nc)
                wpk, b, Co = layers[0]
                y = KP.sa_first(xyz32, xc, new32, nc, feat32, idx, wpk, b, Co, use_xyz=grouper.use_xyz or feat32 is None)
                for wpk, b, Co in layers[1:]:
                    y = KM.conv(y, wpk, b, Co, True)
                KP.groupmax_into(y, grouper.nsample, out, col)
            col += layers[-1][2]
        return out

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), features (N1 + N2 ..., C) ->
        new_xyz, new_features (M1 + M2 ..., sum_k mlps[k][-1])."""
        if self._fused_ok(xyz, new_xyz, features):
            return new_xyz, self._forward_fused(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features)

        new_features_list = []
        for k in range(len(self.groupers)):
            new_features, ball_idxs = self.groupers[k](
                xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features
            )  # (M1 + M2, C, nsample)
            new_features = new_features.permute(1, 0, 2).unsqueeze(dim=0)  # (1, C, M1 + M2 ..., nsample)
            new_features = self.mlps[k](new_features)  # (1, C, M1 + M2 ..., nsample)

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
            new_features = new_features.squeeze(dim=0).permute(1, 0)  # (M1 + M2 ..., C)
            new_features_list.append(new_features)

        new_features = torch.cat(new_features_list, dim=1)  # (M1 + M2 ..., C)

        return new_xyz, new_features


class StackPointnetFPModule(nn.Module):
    def __init__(self, *, mlp: List[int]):
        super().__init__()
        self.mlp = _shared_mlp(mlp)

    def forward(self, unknown, unknown_batch_cnt, known, known_batch_cnt, unknown_feats=None, known_feats=None):
        """unknown (N1 + N2 ..., 3), known (M1 + M2 ..., 3), unknown_feats (N1 + N2 ..., C1), known_feats
        (M1 + M2 ..., C2) -> new_features (N1 + N2 ..., C_out)."""
        dist, idx = pointnet2_utils.three_nn(unknown, unknown_batch_cnt, known, known_batch_cnt)
        dist_recip = 1.0 / (dist + 1e-8)
        norm = torch.sum(dist_recip, dim=-1, keepdim=True)
        weight = dist_recip / norm

        interpolated_feats = pointnet2_utils.three_interpolate(known_feats, idx, weight)

        if unknown_feats is not None:
            new_features = torch.cat([interpolated_feats, unknown_feats], dim=1)  # (N1 + N2 ..., C2 + C1)
        else:
            new_features = interpolated_feats
        new_features = new_features.permute(1, 0)[None, :, :, None]  # (1, C, N1 + N2 ..., 1)
        new_features = self.mlp(new_features)

        new_features = new_features.squeeze(dim=0).squeeze(dim=-1).permute(1, 0)  # (N1 + N2 ..., C)
        return new_features


def _not_built_module(name):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"pointnet2_stack.pointnet2_modules.{name}: the vector-pool family is not built")

    return type(name, (nn.Module,), {"__init__": __init__})


VectorPoolLocalInterpolateModule = _not_built_module("VectorPoolLocalInterpolateModule")
VectorPoolAggregationModule = _not_built_module("VectorPoolAggregationModule")
VectorPoolAggregationModuleMSG = _not_built_module("VectorPoolAggregationModuleMSG")
