"""PointNet feature extractor of the Frechet Point Distance -- mirror of the reference's
`lidargen/metrics/extractor/pointnet.py` (`STN3d` :7-31, `PointNetfeat` :34-61, `PointNet1` :64-80, `pretrained_pointnet`
:83-98): the same modules, parameter and buffer names, so the reference's checkpoint (`cls_model_39.pth`) loads.

Inference only.  The two per-point trunks 3 -> 64 -> 128 -> 1024 + max run in the fused kernel of csrc/pointnet.hip
(ops_pointnet.pointnet_trunk), the dense heads on the skinny family (ops_skinny.skinny_linear); every BatchNorm is folded
into the layer in front of it on the host (`fold_bn`), in float64, once per weight state: the folded tensors are kept on
the module under a key of every parameter's and buffer's (address, _version), so `load_state_dict`, `.to(device)` and an
in-place edit of any of them fold again.  Work buffers are kept per (B, N, device)."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from lidarcrafter_amd import ops_pointnet as KP
from lidarcrafter_amd import ops_skinny as KS

CHECKPOINT_NAME = "cls_model_39.pth"   # the file name the reference's load_state_dict_from_url caches under
_MAX_SHAPES = 8                        # work-buffer sets kept per module
TRUNK = (3, 64, 128, 1024)             # widths of a per-point trunk: the only ones the reference builds


def _add_layers(mod: nn.Module, kind, stem: str, widths, *extra) -> None:
    """mod.<stem>1 ... : a chain of `kind` layers through `widths` (registered in this order: the checkpoint's names)."""
    for i in range(1, len(widths)):
        setattr(mod, f"{stem}{i}", kind(widths[i - 1], widths[i], *extra))


def _add_norms(mod: nn.Module, widths) -> None:
    for i, c in enumerate(widths, 1):
        setattr(mod, f"bn{i}", nn.BatchNorm1d(c))


def fold_bn(weight: torch.Tensor, bias: torch.Tensor, bn: nn.BatchNorm1d, dtype=torch.float32):
    """(w, b) with bn(W x + bias) = w x + b in eval mode: w = s W, b = s (bias - mean) + beta, s = gamma / sqrt(var + eps),
    computed in float64.  `weight` [Co, Ci] or [Co, Ci, 1].  s may be negative: it belongs in w, never behind a max."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = weight.detach().double().reshape(weight.shape[0], -1) * s[:, None]
    b = (bias.detach().double() - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return w.to(dtype).contiguous(), b.to(dtype).contiguous()


def _plain(weight, bias, dtype=torch.float32):
    return (weight.detach().double().reshape(weight.shape[0], -1).to(dtype).contiguous(),
            bias.detach().double().to(dtype).contiguous())


def _check_input(mod: nn.Module, x: torch.Tensor) -> torch.Tensor:
    if mod.training:
        raise RuntimeError(f"{type(mod).__name__}: inference only -- call .eval() first (BatchNorm batch statistics are "
                           "not built)")
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{type(mod).__name__}: `x` must be a CUDA(HIP) tensor -- no CPU fallback on the hot path")
    if x.dim() != 3 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"{type(mod).__name__}: `x` must be [B,3,N], got {tuple(x.shape)}")
    return x.float().contiguous()


class _Folded(nn.Module):
    """Keeps the folded weights and the work buffers of one module (not its children)."""

    def _pairs(self):
        raise NotImplementedError

    def _fingerprint(self):
        fp = []
        for lin, bn in self._pairs():
            for m in (lin, bn):
                if m is None:
                    continue
                for t in list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)):
                    fp.append((t.data_ptr(), t._version, str(t.device), t.dtype))
        return tuple(fp)

    def _fold_pair(self, lin, bn):
        """(w, b) of one layer of `_pairs()` (the sparse extractors fold a `kernel` without a bias instead)."""
        return fold_bn(lin.weight, lin.bias, bn) if bn is not None else _plain(lin.weight, lin.bias)

    def folded(self):
        """[(w, b)] per layer of `_pairs()`, float32 on the parameters' device."""
        key = self._fingerprint()
        hit = self.__dict__.get("_lc_folded")
        if hit is None or hit[0] != key:
            with torch.no_grad():
                ws = [self._fold_pair(l, bn) for l, bn in self._pairs()]
            hit = (key, ws)
            self.__dict__["_lc_folded"] = hit
            self.__dict__["_lc_work"] = {}
        return hit[1]

    def _work(self, B: int, N: int, dev, make):
        cache = self.__dict__.setdefault("_lc_work", {})
        k = (B, N, str(dev))
        if k not in cache:
            if len(cache) >= _MAX_SHAPES:
                cache.clear()
            cache[k] = make()
        return cache[k]


def _head_parts(B: int, dev) -> torch.Tensor:
    n = max(KS.skinny_parts(B, 512, 1024) * B * 512, KS.skinny_parts(B, 256, 512) * B * 256,
            KS.skinny_parts(B, 9, 256) * B * 9)
    return torch.empty(n, device=dev, dtype=torch.float32)


class STN3d(_Folded):
    def __init__(self):
        super().__init__()
        _add_layers(self, nn.Conv1d, "conv", TRUNK, 1)
        _add_layers(self, nn.Linear, "fc", (1024, 512, 256, 9))
        _add_norms(self, TRUNK[1:] + (512, 256))

    def _pairs(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3), (self.fc1, self.bn4),
                (self.fc2, self.bn5), (self.fc3, None)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = _check_input(self, x)
        B, _, N = x.shape
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            (w1, b1), (w2, b2), (w3, b3), (w4, b4), (w5, b5), (w6, b6) = self.folded()
            wk = self._work(B, N, dev, lambda: dict(
                scratch=torch.empty(KP.trunk_scratch_elems(B, N), device=dev, dtype=torch.float32),
                g=torch.empty((B, 1024), device=dev, dtype=torch.float32),
                f1=torch.empty((B, 512), device=dev, dtype=torch.float32),
                f2=torch.empty((B, 256), device=dev, dtype=torch.float32),
                parts=_head_parts(B, dev),
                eye=torch.eye(3, device=dev, dtype=torch.float32).reshape(1, 9).contiguous()))
            KP.pointnet_trunk(x, None, w1, b1, w2, b2, w3, b3, True, out=wk["g"], scratch=wk["scratch"])
            KS.skinny_linear([(wk["g"], 0, 1024, None)], B, w4, b4, "relu", out=wk["f1"], parts=wk["parts"])
            KS.skinny_linear([(wk["f1"], 0, 512, None)], B, w5, b5, "relu", out=wk["f2"], parts=wk["parts"])
            trans = torch.empty((B, 9), device=dev, dtype=torch.float32)
            KS.skinny_linear([(wk["f2"], 0, 256, None)], B, w6, b6, None, vec=(wk["eye"], 0, None), out=trans,
                             parts=wk["parts"])
        return trans.view(B, 3, 3)


class PointNetfeat(_Folded):
    def __init__(self, global_feat=True):
        super().__init__()
        if not global_feat:
            raise NotImplementedError("PointNetfeat(global_feat=False): the per-point feature map is not built (the "
                                      "Frechet Point Distance reads the global feature only)")
        self.stn = STN3d()
        _add_layers(self, nn.Conv1d, "conv", TRUNK, 1)
        _add_norms(self, TRUNK[1:])
        self.global_feat = global_feat

    def _pairs(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]

    def _run(self, x: torch.Tensor, out: torch.Tensor):
        """x checked [B,3,N]; writes columns 0:1024 of `out`, returns trans [B,3,3]."""
        B, _, N = x.shape
        dev = x.device
        trans = self.stn(x)
        with torch.cuda.device(dev), torch.no_grad():
            (w1, b1), (w2, b2), (w3, b3) = self.folded()
            wk = self._work(B, N, dev, lambda: dict(
                scratch=torch.empty(KP.trunk_scratch_elems(B, N), device=dev, dtype=torch.float32)))
            KP.pointnet_trunk(x, trans, w1, b1, w2, b2, w3, b3, False, out=out, scratch=wk["scratch"])
        return trans

    def forward(self, x: torch.Tensor):
        if not self.global_feat:
            raise NotImplementedError("PointNetfeat: global_feat=False is not built")
        x = _check_input(self, x)
        out = torch.empty((x.shape[0], 1024), device=x.device, dtype=torch.float32)
        trans = self._run(x, out)
        return out, trans


class PointNet1(_Folded):
    def __init__(self, k=2):
        super().__init__()
        self.feat = PointNetfeat(global_feat=True)
        _add_layers(self, nn.Linear, "fc", (1024, 512, 256, k))
        _add_norms(self, (512, 256))

    def _pairs(self):
        return [(self.fc1, self.bn1), (self.fc2, self.bn2), (self.fc3, None)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[B,3,N] -> [B, 1024 + 512 + 256 + k] = cat(x1, x2, x3, x4); every layer writes its own columns."""
        if not self.feat.global_feat:
            raise NotImplementedError("PointNet1: global_feat=False is not built")
        x = _check_input(self, x)
        B, dev, k = x.shape[0], x.device, self.fc3.out_features
        feature = torch.empty((B, 1792 + k), device=dev, dtype=torch.float32)
        self.feat._run(x, feature)
        with torch.cuda.device(dev), torch.no_grad():
            (w1, b1), (w2, b2), (w3, b3) = self.folded()
            wk = self._work(B, k, dev, lambda: dict(parts=torch.empty(
                max(KS.skinny_parts(B, 512, 1024) * B * 512, KS.skinny_parts(B, 256, 512) * B * 256,
                    KS.skinny_parts(B, k, 256) * B * k), device=dev, dtype=torch.float32)))
            KS.skinny_linear([(feature, 0, 1024, None)], B, w1, b1, "relu", out=feature[:, 1024:1536], parts=wk["parts"])
            KS.skinny_linear([(feature, 1024, 512, None)], B, w2, b2, "relu", out=feature[:, 1536:1792], parts=wk["parts"])
            KS.skinny_linear([(feature, 1536, 256, None)], B, w3, b3, None, out=feature[:, 1792:], parts=wk["parts"])
        return feature


def default_checkpoint_path() -> str:
    """Where the reference's `load_state_dict_from_url` would have cached the ShapeNet classifier."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", CHECKPOINT_NAME)


def pretrained_pointnet(dataset: str = "shapenet", device="cpu", compile: bool = True, checkpoint=None) -> nn.Module:
    """PointNet1(k=16) with the ShapeNet classifier's weights, read from `checkpoint` or from the hub cache directory.
    The file is never fetched: when it is absent this raises FileNotFoundError naming the path to put it at.  `compile`
    is accepted for the reference's signature and ignored (there is nothing for torch.compile to trace)."""
    if dataset != "shapenet":
        raise ValueError(f"Unknown dataset: {dataset}")
    path = os.fspath(checkpoint) if checkpoint is not None else default_checkpoint_path()
    if not os.path.isfile(path):
        raise FileNotFoundError(f"pretrained_pointnet: no checkpoint at {path} -- place the reference's {CHECKPOINT_NAME} "
                                "there or pass checkpoint=<path>; this build does not fetch it")
    model = PointNet1(k=16)
    model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    model.eval().requires_grad_(False)
    return model.to(device)
