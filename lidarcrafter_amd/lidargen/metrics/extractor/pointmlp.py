"""PointMLP object extractor -- mirror of the reference's `lidargen/metrics/extractor/pointmlp.py`: the same modules,
arguments and state-dict keys, so the evaluator's checkpoint (`nusc_object_classification_model.pth`, `['net']`) loads.

Inference only.  `Model.forward` runs one plan over the kernels of csrc/pointmlp.hip (lidarcrafter_amd.ops_pointmlp;
DESIGN.md section 5o): per stage farthest point sampling and k nearest neighbours on the coordinates, the grouped and
normalised operand, the `transfer` layer and the residual blocks as dense layers with every BatchNorm folded on the host in
float64 (`extractor.pointnet.fold_bn`, kept under the fingerprint of every parameter and buffer), and the maximum over the
neighbours.  The sub-modules hold parameters; their own `forward` raises.

Not built (NotImplementedError by name): groups > 1, activations other than ReLU, use_xyz=True, normalize other than
'anchor', kernel sizes other than 1, training mode, grad mode, CPU tensors."""
from __future__ import annotations

import torch
import torch.nn as nn

from lidarcrafter_amd import ops_pointmlp as KM
from lidargen.ops.pointnet2.pointnet2_batch import pointnet2_utils

from .pointnet import _Folded, _plain, fold_bn

_OTHER_ACTIVATIONS = ("gelu", "rrelu", "selu", "silu", "hardswish", "leakyrelu")


def _no_forward(self, *args, **kwargs):
    raise NotImplementedError(f"{type(self).__name__}.forward is not built on its own: the network runs as one plan "
                              "through Model.forward")


def get_activation(activation):
    if activation.lower() in _OTHER_ACTIVATIONS:
        raise NotImplementedError(f"get_activation: '{activation}' is not built; the dense kernel applies ReLU only (the "
                                  "activation of pointMLP and pointMLPElite)")
    return nn.ReLU(inplace=True)


def _check_conv_args(who, kernel_size, groups=1):
    if kernel_size != 1:
        raise NotImplementedError(f"{who}: kernel_size = {kernel_size} is not built (the reference builds 1 only)")
    if groups != 1:
        raise NotImplementedError(f"{who}: groups = {groups} is not built (grouped convolutions; pointMLP and pointMLPElite "
                                  "use groups = 1)")


class LocalGrouper(nn.Module):
    def __init__(self, channel, groups, kneighbors, use_xyz=True, normalize="center", **kwargs):
        """`groups` anchors (farthest point sampling), `kneighbors` neighbours each; holds affine_alpha / affine_beta."""
        super().__init__()
        if use_xyz:
            raise NotImplementedError("LocalGrouper: use_xyz=True is not built (the coordinates as extra feature channels; "
                                      "pointMLP and pointMLPElite pass use_xyz=False)")
        if normalize is None or normalize.lower() != "anchor":
            raise NotImplementedError(f"LocalGrouper: normalize = {normalize!r} is not built; only 'anchor' (the setting of "
                                      "pointMLP and pointMLPElite) is")
        self.groups = groups
        self.kneighbors = kneighbors
        self.use_xyz = use_xyz
        self.normalize = normalize.lower()
        self.affine_alpha = nn.Parameter(torch.ones([1, 1, 1, channel]))
        self.affine_beta = nn.Parameter(torch.zeros([1, 1, 1, channel]))

    forward = _no_forward


class ConvBNReLU1D(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, bias=True, activation="relu"):
        super().__init__()
        _check_conv_args("ConvBNReLU1D", kernel_size)
        self.act = get_activation(activation)
        self.net = nn.Sequential(
            nn.Conv1d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, bias=bias),
            nn.BatchNorm1d(out_channels),
            self.act)

    forward = _no_forward

    def plan_layers(self):
        return [(self.net[0], self.net[1])]


class ConvBNReLURes1D(nn.Module):
    def __init__(self, channel, kernel_size=1, groups=1, res_expansion=1.0, bias=True, activation="relu"):
        super().__init__()
        _check_conv_args("ConvBNReLURes1D", kernel_size, groups)
        self.act = get_activation(activation)
        mid = int(channel * res_expansion)
        if mid < 1:
            raise ValueError(f"ConvBNReLURes1D: int({channel} * {res_expansion}) = {mid} channels")
        self.net1 = nn.Sequential(
            nn.Conv1d(in_channels=channel, out_channels=mid, kernel_size=kernel_size, groups=groups, bias=bias),
            nn.BatchNorm1d(mid),
            self.act)
        self.net2 = nn.Sequential(
            nn.Conv1d(in_channels=mid, out_channels=channel, kernel_size=kernel_size, bias=bias),
            nn.BatchNorm1d(channel))

    forward = _no_forward

    def plan_layers(self):
        return [(self.net1[0], self.net1[1]), (self.net2[0], self.net2[1])]


class PreExtraction(nn.Module):
    def __init__(self, channels, out_channels, blocks=1, groups=1, res_expansion=1, bias=True, activation="relu",
                 use_xyz=True):
        super().__init__()
        if use_xyz:
            raise NotImplementedError("PreExtraction: use_xyz=True is not built")
        self.transfer = ConvBNReLU1D(2 * channels, out_channels, bias=bias, activation=activation)
        self.operation = nn.Sequential(*[ConvBNReLURes1D(out_channels, groups=groups, res_expansion=res_expansion, bias=bias,
                                                         activation=activation) for _ in range(blocks)])

    forward = _no_forward


class PosExtraction(nn.Module):
    def __init__(self, channels, blocks=1, groups=1, res_expansion=1, bias=True, activation="relu"):
        super().__init__()
        self.operation = nn.Sequential(*[ConvBNReLURes1D(channels, groups=groups, res_expansion=res_expansion, bias=bias,
                                                         activation=activation) for _ in range(blocks)])

    forward = _no_forward


class Model(_Folded):
    def __init__(self, points=1024, class_num=40, embed_dim=64, groups=1, res_expansion=1.0,
                 activation="relu", bias=True, use_xyz=True, normalize="center",
                 dim_expansion=[2, 2, 2, 2], pre_blocks=[2, 2, 2, 2], pos_blocks=[2, 2, 2, 2],
                 k_neighbors=[32, 32, 32, 32], reducers=[2, 2, 2, 2], **kwargs):
        super().__init__()
        self.stages = len(pre_blocks)
        self.class_num = class_num
        self.points = points
        if groups != 1:
            raise NotImplementedError(f"Model: groups = {groups} is not built (grouped convolutions)")
        self.embedding = ConvBNReLU1D(3, embed_dim, bias=bias, activation=activation)
        assert len(pre_blocks) == len(k_neighbors) == len(reducers) == len(pos_blocks) == len(dim_expansion), \
            "Please check stage number consistent for pre_blocks, pos_blocks k_neighbors, reducers."
        self.local_grouper_list = nn.ModuleList()
        self.pre_blocks_list = nn.ModuleList()
        self.pos_blocks_list = nn.ModuleList()
        last_channel = embed_dim
        anchor_points = self.points
        for i in range(len(pre_blocks)):
            out_channel = last_channel * dim_expansion[i]
            anchor_points = anchor_points // reducers[i]
            if anchor_points < 1 or not 1 <= k_neighbors[i] <= KM_MAX_K:
                raise ValueError(f"Model: stage {i} has {anchor_points} anchors and {k_neighbors[i]} neighbours (1 .. "
                                 f"{KM_MAX_K} neighbours are built)")
            self.local_grouper_list.append(LocalGrouper(last_channel, anchor_points, k_neighbors[i], use_xyz, normalize))
            self.pre_blocks_list.append(PreExtraction(last_channel, out_channel, pre_blocks[i], groups=groups,
                                                      res_expansion=res_expansion, bias=bias, activation=activation,
                                                      use_xyz=use_xyz))
            self.pos_blocks_list.append(PosExtraction(out_channel, pos_blocks[i], groups=groups,
                                                      res_expansion=res_expansion, bias=bias, activation=activation))
            last_channel = out_channel
        self.act = get_activation(activation)
        self.classifier = nn.Sequential(
            nn.Linear(last_channel, 512),
            nn.BatchNorm1d(512),
            self.act,
            nn.Dropout(0.5),
            nn.Linear(512, 256),
            nn.BatchNorm1d(256),
            self.act,
            nn.Dropout(0.5),
            nn.Linear(256, self.class_num))

    # ---- the fold ----------------------------------------------------------------------------------------------------
    def _pairs(self):
        """(layer, BatchNorm or None) in plan order: embedding; per stage transfer, the pre blocks, the pos blocks; the
        three classifier layers."""
        out = list(self.embedding.plan_layers())
        for pre, pos in zip(self.pre_blocks_list, self.pos_blocks_list):
            out += pre.transfer.plan_layers()
            for blk in list(pre.operation) + list(pos.operation):
                out += blk.plan_layers()
        c = self.classifier
        return out + [(c[0], c[1]), (c[4], c[5]), (c[8], None)]

    def _fingerprint(self):
        fp = list(super()._fingerprint())
        for g in self.local_grouper_list:
            for t in (g.affine_alpha, g.affine_beta):
                fp.append((t.data_ptr(), t._version, str(t.device), t.dtype))
        return tuple(fp)

    def _fold_pair(self, lin, bn):
        bias = lin.bias if lin.bias is not None else torch.zeros(lin.weight.shape[0], device=lin.weight.device)
        return fold_bn(lin.weight, bias, bn) if bn is not None else _plain(lin.weight, bias)

    def packed(self, dev):
        """[(packed weight, bias, Co)] per layer of `_pairs()` and [(alpha, beta)] per stage, on `dev`; packed again when
        any parameter or buffer changed (`_Folded.folded`)."""
        ws = self.folded()
        hit = self.__dict__.get("_lc_packed")
        if hit is None or hit[0] is not ws or hit[1] != str(dev):
            layers = [(KM.pack_weight(w.cpu().contiguous()).to(dev), b.to(dev).contiguous(), w.shape[0]) for w, b in ws]
            affine = [(g.affine_alpha.detach().float().reshape(-1).contiguous().to(dev),
                       g.affine_beta.detach().float().reshape(-1).contiguous().to(dev)) for g in self.local_grouper_list]
            hit = (ws, str(dev), layers, affine)
            self.__dict__["_lc_packed"] = hit
        return hit[2], hit[3]

    # ---- the plan ----------------------------------------------------------------------------------------------------
    def _check(self, x, who):
        if self.training:
            raise NotImplementedError(f"{who}: training mode is not built (BatchNorm batch statistics, Dropout) -- call "
                                      ".eval() first")
        if torch.is_grad_enabled() and (getattr(x, "requires_grad", False) or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(f"{who}: grad mode is not built (no backward kernels) -- call under torch.no_grad() "
                                      "or after .requires_grad_(False)")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise NotImplementedError(f"{who}: CPU tensors are not built -- `x` must be a CUDA(HIP) tensor, there is no CPU "
                                      "fallback on the hot path")
        if x.dim() != 3 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"{who}: `x` must be [B,3,N], got {tuple(x.shape)}")
        for i, g in enumerate(self.local_grouper_list):
            n = x.shape[2] if i == 0 else self.local_grouper_list[i - 1].groups
            if g.kneighbors > n:
                raise ValueError(f"{who}: stage {i} asks for {g.kneighbors} neighbours among {n} points")
        return x.float().contiguous()

    def geometry(self, xyz: torch.Tensor):
        """[(fps_idx int32 [B,S], knn_idx int32 [B,S,K])] per stage from `xyz` [B,N,3]: the index tables depend on the
        coordinates only."""
        xyz = xyz.float().contiguous()
        tables = []
        with torch.cuda.device(xyz.device), torch.no_grad():
            for g in self.local_grouper_list:
                fps_idx = pointnet2_utils.furthest_point_sample(xyz, g.groups)
                tables.append((fps_idx, KM.knn(xyz, fps_idx, g.kneighbors)))
                xyz = torch.gather(xyz, 1, fps_idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        return tables

    def dense(self, x: torch.Tensor, tables, return_features=False):
        """The network from the checked input `x` [B,3,N] and the index tables of `geometry`."""
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            layers, affine = self.packed(dev)
            it = iter(layers)

            def run(t, act, res=None):
                wpk, b, Co = next(it)
                return KM.conv(t, wpk, b, Co, act, res=res)

            def block(t):
                return run(run(t, True), True, res=t)

            feat = run(x, True)
            for i, (fps_idx, knn_idx) in enumerate(tables):
                g = KM.group(feat, fps_idx, knn_idx, *affine[i])
                t = run(g, True)
                for _ in self.pre_blocks_list[i].operation:
                    t = block(t)
                feat = KM.groupmax(t, knn_idx.shape[2])
                for _ in self.pos_blocks_list[i].operation:
                    feat = block(feat)
            f = KM.groupmax(feat, feat.shape[2], channel_major=True)           # [1, C, B]
            if return_features:
                return f[0].t().contiguous()
            h = run(run(f, True), True)
            return run(h, False)[0].t().contiguous()

    def forward(self, x, return_features=False):
        """x [B,3,N] -> the logits [B, class_num], or with return_features the global feature [B, C]."""
        x = self._check(x, "Model.forward")
        return self.dense(x, self.geometry(x.permute(0, 2, 1)), return_features)


KM_MAX_K = 32     # lc_knn_fwd: LC_KNN_MAX_K


def pointMLP(num_classes=40, **kwargs) -> Model:
    return Model(points=1024, class_num=num_classes, embed_dim=64, groups=1, res_expansion=1.0,
                 activation="relu", bias=False, use_xyz=False, normalize="anchor",
                 dim_expansion=[2, 2, 2, 2], pre_blocks=[2, 2, 2, 2], pos_blocks=[2, 2, 2, 2],
                 k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2], **kwargs)


def pointMLPElite(num_classes=40, **kwargs) -> Model:
    return Model(points=1024, class_num=num_classes, embed_dim=32, groups=1, res_expansion=0.25,
                 activation="relu", bias=False, use_xyz=False, normalize="anchor",
                 dim_expansion=[2, 2, 2, 1], pre_blocks=[1, 1, 2, 1], pos_blocks=[1, 1, 2, 1],
                 k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2], **kwargs)
