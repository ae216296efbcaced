"""MinkUNet feature extractor of the Frechet Sparse Volume Distance -- mirror of the reference's
`lidargen/metrics/models/minkowskinet/model.py` (`Model` :12-141): the same module tree and state-dict names
(`stem.0.kernel`, `stage1.1.net.0.kernel`, `stage1.1.downsample.1.running_mean`, `up1.1.0.net.3.weight`,
`classifier.0.weight`, ...), so `ckpt['state_dict']` of the reference's `model.ckpt` loads.

Inference only.  Every convolution runs in csrc/spconv.hip (ops_spconv.sparse_conv) with the BatchNorm behind it folded
into (w, b) on the host in float64, the ReLU and the residual sum in its epilogue; `torchsparse.cat` is no copy: the
producers of both halves write their columns of one buffer.  The folded weights are kept under the (address, _version) of
every parameter and buffer (extractor/pointnet.py `_Folded`); coordinate levels and neighbour tables are built per call
(ops_spconv.CoordLevels) and shared by the layers of that call only."""
from __future__ import annotations

import torch
import torch.nn as nn

from lidarcrafter_amd import ops_spconv as KS

from ...extractor.pointnet import _Folded
from ..ts import basic_blocks
from ..ts.basic_blocks import BatchNorm, Conv3d, ReLU


def _field(obj, name):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


def fold_conv_bn(conv: Conv3d, bn, dtype=torch.float32):
    """(w [K, Ci, Co], b [Co]) with bn(conv(x)) = sum_k x_k w[k] + b in eval mode: w = kernel * s, b = beta - mean * s,
    s = gamma / sqrt(var + eps), computed in float64.  Without a norm b is None."""
    w = conv.kernel.detach().double().reshape(conv.kernel_volume, conv.in_channels, conv.out_channels)
    if bn is None:
        return w.to(dtype).contiguous(), None
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return (w * s).to(dtype).contiguous(), b.to(dtype).contiguous()


class Model(_Folded):
    def __init__(self, config):
        super().__init__()
        mp = _field(config, "model_params")
        cr = _field(mp, "cr")
        cs = [int(cr * x) for x in _field(mp, "layer_num")]
        if len(cs) != 9:
            raise ValueError(f"Model: layer_num must have nine entries, got {len(cs)}")
        self.cs = cs
        self.pres = self.vres = _field(mp, "voxel_size")
        self.num_classes = _field(mp, "num_class")
        inc = _field(mp, "input_dims")
        for name, c in (("input_dims", inc),) + tuple((f"cs[{i}]", c) for i, c in enumerate(cs)):
            if c not in KS.WIDTHS_IN or (name != "input_dims" and c not in KS.WIDTHS_OUT):
                raise NotImplementedError(f"Model: {name} = {c} is not a width the sparse convolution kernel is built for "
                                          f"(inputs {KS.WIDTHS_IN}, outputs {KS.WIDTHS_OUT})")
        B, R, D = basic_blocks.BasicConvolutionBlock, basic_blocks.ResidualBlock, basic_blocks.BasicDeconvolutionBlock

        self.stem = nn.Sequential(Conv3d(inc, cs[0], kernel_size=3, stride=1), BatchNorm(cs[0]), ReLU(True),
                                  Conv3d(cs[0], cs[0], kernel_size=3, stride=1), BatchNorm(cs[0]), ReLU(True))
        for i in range(1, 5):
            setattr(self, f"stage{i}", nn.Sequential(B(cs[i - 1], cs[i - 1], ks=2, stride=2, dilation=1),
                                                     R(cs[i - 1], cs[i], ks=3, stride=1, dilation=1),
                                                     R(cs[i], cs[i], ks=3, stride=1, dilation=1)))
        for i in range(1, 5):
            skip = cs[4 - i]
            for c in (cs[4 + i] + skip,):
                if c not in KS.WIDTHS_IN:
                    raise NotImplementedError(f"Model: the concatenated width {c} of up{i} is not built")
            setattr(self, f"up{i}", nn.ModuleList([
                D(cs[3 + i], cs[4 + i], ks=2, stride=2),
                nn.Sequential(R(cs[4 + i] + skip, cs[4 + i], ks=3, stride=1, dilation=1),
                              R(cs[4 + i], cs[4 + i], ks=3, stride=1, dilation=1))]))
        self.classifier = nn.Sequential(nn.Linear(cs[8], self.num_classes))
        self.weight_initialization()
        self.dropout = nn.Dropout(0.3, True)

    def weight_initialization(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    # ---- folded weights -------------------------------------------------------------------------------------------
    def _pairs(self):
        """(conv, the BatchNorm behind it) of every Sequential, in module order."""
        out = []
        for seq in self.modules():
            if isinstance(seq, nn.Sequential):
                kids = list(seq)
                for i, m in enumerate(kids):
                    if isinstance(m, Conv3d):
                        bn = kids[i + 1] if i + 1 < len(kids) and isinstance(kids[i + 1], nn.BatchNorm1d) else None
                        out.append((m, bn))
        return out

    def _fold_pair(self, conv, bn):
        return fold_conv_bn(conv, bn)

    # ---- forward --------------------------------------------------------------------------------------------------
    def _check_inputs(self, feats, coords, return_logits, return_final_logits):
        if self.training:
            raise RuntimeError("Model: inference only -- call .eval() first (BatchNorm batch statistics are not built)")
        for t, n in ((feats, "feats"), (coords, "coords")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"Model: `{n}` must be a CUDA(HIP) tensor -- no CPU fallback on the hot path")
        if not (return_logits or return_final_logits):
            raise NotImplementedError("Model: the classifier head is not on the path of the Frechet distances "
                                      "and is not built; pass return_final_logits=True")
        if feats.dim() != 2 or coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] != feats.shape[0] or \
                feats.shape[0] < 1:
            raise ValueError(f"Model: feats [N, C] and coords [N, 4] expected, got {tuple(feats.shape)}, "
                             f"{tuple(coords.shape)}")

    def _layer_ops(self):
        """(conv, block): one folded layer / one residual block through the sparse convolution kernel."""
        W = {id(conv): wb for (conv, _), wb in zip(self._pairs(), self.folded())}

        def conv(m, x, nbr, relu, res=None, out=None, col=0):
            w, b = W[id(m)]
            y = KS.sparse_conv(x, nbr, w, b, residual=res, relu=relu, out=out, out_col=col)
            return y[:, col:col + w.shape[2]]

        def block(blk, x, nbr, out=None, col=0):
            h = conv(blk.net[0], x, nbr, True)
            r = x if len(blk.downsample) == 0 else conv(blk.downsample[0], x, None, False)
            return conv(blk.net[3], h, nbr, True, res=r, out=out, col=col)

        return conv, block

    def _cat_buffers(self, L, dev):
        """cat[i]: the input of up{i}[1] at level 4 - i = [the up-sampled rows | the skip of that level]"""
        cs = self.cs
        return {i: torch.empty((L.rows(4 - i), cs[4 + i] + cs[4 - i]), device=dev, dtype=torch.float32)
                for i in range(1, 5)}

    def _up(self, i, x, L, cat, conv, block):
        """up{i}: the transposed convolution into the left columns of cat[i], then the two residual blocks."""
        up = getattr(self, f"up{i}")
        lvl = 4 - i
        conv(up[0].net[0], x, L.up(lvl), True, out=cat[i], col=0)
        x = block(up[1][0], cat[i], L.same(lvl))
        return block(up[1][1], x, L.same(lvl))

    def _stages(self, x, L, cat, conv, block):
        """stage1 .. stage4 from the level-0 rows x; the skips of levels 1 .. 3 land in their cat buffers."""
        cs = self.cs
        for i in range(1, 5):
            stage = getattr(self, f"stage{i}")
            x = conv(stage[0].net[0], x, L.down(i - 1), True)
            x = block(stage[1], x, L.same(i))
            if i < 4:
                x = block(stage[2], x, L.same(i), out=cat[4 - i], col=cs[8 - i])
            else:
                x = block(stage[2], x, L.same(i))
        return x

    def forward(self, feats: torch.Tensor, coords: torch.Tensor, return_logits=False, return_final_logits=True):
        """feats [N, input_dims] float32 and coords [N, 4] = (x, y, z, batch) of the collated batch, on the GPU ->
        {'logits' [N, cs[8]], 'coords' [N, 3], 'batch_indices' [N]} over the input voxels in input order (the reference's
        `return_final_logits=True`); `return_logits=True`: the bottleneck features and their batch indices."""
        self._check_inputs(feats, coords, return_logits, return_final_logits)
        cs, dev = self.cs, feats.device
        with torch.cuda.device(dev), torch.no_grad():
            feats = feats.float().contiguous()
            coords = coords.to(torch.int32).contiguous()
            top = coords.max(dim=0).values.tolist()          # one read: the limits are checked on the host
            if int(coords.min().item()) < 0:
                raise ValueError("Model: negative coordinates (pcd2voxel subtracts the minimum)")
            conv, block = self._layer_ops()
            L = KS.CoordLevels(coords, n_batch=top[3] + 1, max_coord=max(top[:3]))
            cat = self._cat_buffers(L, dev)
            same0 = L.same(0)
            x = conv(self.stem[0], feats, same0, True)
            x = conv(self.stem[3], x, same0, True, out=cat[4], col=cs[8])
            x = self._stages(x, L, cat, conv, block)
            if return_logits:
                return {"logits": x, "batch_indices": L.coords[4][:, 3]}
            for i in range(1, 5):
                x = self._up(i, x, L, cat, conv, block)
        return {"logits": x, "coords": coords[:, :3], "batch_indices": coords[:, 3]}
