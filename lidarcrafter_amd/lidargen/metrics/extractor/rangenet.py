"""RangeNet under the state-dict names of the reference's `lidargen/metrics/extractor/rangenet.py` (`stem.0.weight`,
`enc3.residual_blocks.5.residual.1.0.weight`, `dec5.conv.0.bias`, `head.1.bias`): the extractor of the evaluator's FRD.
The modules hold parameters only; the forward is the same `models.rangenet.plan.Plan` as the FRID model's, over the HIP
convolutions of csrc/rangenet.hip -- eval mode, no autograd, CUDA(HIP) tensors only.

Nothing is ever fetched: a URL, or a `weights=` name whose archive is not in the torch hub cache, raises
FileNotFoundError naming the path that was looked at.  The kNN and CRF-RNN post-processors and the colour map of the
reference are not built; their names resolve to stubs that say so."""
from __future__ import annotations

import io
import os
import random
import tarfile
from collections import OrderedDict
from typing import Any
from urllib.parse import urlparse

import torch
from torch import nn

from ..models.rangenet.plan import MODEL_BLOCKS, Layer, Plan, check_call
from lidarcrafter_amd import ops_rangenet as KR

N_SUBSAMPLE = 4096
_LOCAL_ARCH = "2025-7-17-06:41"     # the folder name inside the reference's own local archive
# the archives of the official checkpoints (http://www.ipb.uni-bonn.de/html/projects/bonnetal/lidar/semantic/models/)
_ARCHIVES = {21: {"SemanticKITTI_64x2048": "darknet21.tar.gz"},
             53: {"SemanticKITTI_64x2048": "darknet53.tar.gz", "SemanticKITTI_64x1024": "darknet53-1024.tar.gz",
                  "SemanticKITTI_64x512": "darknet53-512.tar.gz"}}
_OFFICIAL = "http://www.ipb.uni-bonn.de/html/projects/bonnetal/lidar/semantic/models/{}"


def _count_in_ch(modalities) -> int:
    channels = {"xyz": 3, "range": 1, "remission": 1, "mask": 1}
    return sum(channels[m] for m, enabled in modalities.items() if enabled)


def _no_forward(self, *args, **kwargs):
    raise NotImplementedError(f"{type(self).__name__}.forward is not built on its own: the network runs as one plan "
                              "through RangeNet.forward")


class ConvNormLReLU(nn.Sequential):
    def __init__(self, in_ch, out_ch, kernel_size, stride, padding, momentum, transposed=False, bias=False):
        conv_cls = nn.ConvTranspose2d if transposed else nn.Conv2d
        super().__init__(conv_cls(in_ch, out_ch, kernel_size, stride, padding, bias=bias),
                         nn.BatchNorm2d(out_ch, momentum=momentum), nn.LeakyReLU(0.1))

    forward = _no_forward


class ResidualBlock(nn.Module):
    def __init__(self, in_ch, mid_ch, out_ch, momentum=0.1):
        super().__init__()
        self.residual = nn.Sequential(ConvNormLReLU(in_ch, mid_ch, 1, 1, 0, momentum),
                                      ConvNormLReLU(mid_ch, out_ch, 3, 1, 1, momentum))

    forward = _no_forward


_GEOMETRY = {"same": ((3, 3), (1, 1), (1, 1), 1), "up": ((1, 4), (1, 2), (0, 1), 3), "down": ((3, 3), (1, 2), (1, 1), 2)}


class Block(nn.Module):
    def __init__(self, in_ch, out_ch, num_blocks, momentum, mode="same"):
        super().__init__()
        if mode not in _GEOMETRY:
            raise ValueError(f"Unknown mode: {mode}")
        kernel_size, stride, padding, self._conv_mode = _GEOMETRY[mode]
        self.conv = ConvNormLReLU(in_ch, out_ch, kernel_size, stride, padding, momentum, transposed=mode == "up",
                                  bias=mode == "up")
        self.residual_blocks = nn.ModuleList(ResidualBlock(out_ch, in_ch, out_ch, momentum) for _ in range(num_blocks))
        self._tag = {"same": "stem", "up": "up", "down": "down"}[mode]

    forward = _no_forward

    def plan_layers(self):
        out = [Layer(self.conv[0], self.conv[1], self._conv_mode, True, self._tag)]
        for blk in self.residual_blocks:
            out += [Layer(blk.residual[0][0], blk.residual[0][1], 0, True, "c1"),
                    Layer(blk.residual[1][0], blk.residual[1][1], 1, True, "c2")]
        return out


def subsample_indices(n: int, k: int = N_SUBSAMPLE):
    """The k indices the reference's flatten_and_subsample draws (`random.seed(0); random.sample(range(n), k)`), from a
    generator of its own: the process-wide one is not reseeded."""
    return random.Random(0).sample(range(n), k)


class RangeNet(nn.Module):
    def __init__(self, inputs, num_classes, momentum=0.01, dropout=0.05, backbone=53):
        super().__init__()
        self.inputs = inputs
        self.num_classes = num_classes
        self.in_ch = _count_in_ch(inputs)
        self.backbone = backbone
        if backbone not in MODEL_BLOCKS:
            raise ValueError(f"RangeNet: backbone = {backbone} is none of {sorted(MODEL_BLOCKS)}")
        n = MODEL_BLOCKS[backbone]
        ch = lambda i: 32 << i  # noqa: E731
        momentum = nn.modules.utils._pair(momentum)
        dropout = nn.modules.utils._triple(dropout)
        self.stem = ConvNormLReLU(self.in_ch, 32, 3, 1, 1, momentum[0])
        for i in range(1, 6):
            setattr(self, f"enc{i}", Block(ch(i - 1), ch(i), n[i - 1], momentum[0], "down"))
        self.dropout1 = nn.Dropout2d(p=dropout[0])
        for i in range(5, 0, -1):
            setattr(self, f"dec{i}", Block(ch(i), ch(i - 1), 1, momentum[1], "up"))
        self.dropout2 = nn.Dropout2d(p=dropout[1])
        self.head = nn.Sequential(nn.Dropout2d(p=dropout[2]), nn.Conv2d(32, num_classes, 3, 1, 1))
        self._plan = None
        self._idx = {}

    def plan(self) -> Plan:
        if self._plan is None:
            layers = [Layer(self.stem[0], self.stem[1], 1, True, "stem")]
            for i in range(1, 6):
                layers += getattr(self, f"enc{i}").plan_layers()
            for i in range(5, 0, -1):
                layers += getattr(self, f"dec{i}").plan_layers()
            layers.append(Layer(self.head[1], None, 1, False, "head"))
            self._plan = Plan(layers)
        return self._plan

    def flatten_and_subsample(self, fmaps: torch.Tensor) -> torch.Tensor:
        """4096 fixed columns of the flattened [C*H*W] map: the sequence of the reference's `random.seed(0);
        random.sample(range(C*H*W), 4096)`, drawn from a private `random.Random(0)` -- the process-wide generator is NOT
        reseeded (the reference reseeds it on every call)."""
        B, C, H, W = fmaps.shape
        n = C * H * W
        key = (n, str(fmaps.device))
        if key not in self._idx:
            self._idx[key] = torch.tensor(subsample_indices(n), dtype=torch.long, device=fmaps.device)
        return fmaps.reshape(B, n)[:, self._idx[key]]

    def forward(self, img: torch.Tensor, feature=None) -> torch.Tensor:
        """feature None: the logits [B,num_classes,H,W] of the head; 'decoder': the decoder map [B,32,H,W]; 'lidargen':
        its 4096-column subsample (flatten_and_subsample)."""
        check_call(self, img, "RangeNet.forward")
        if feature not in (None, "decoder", "lidargen"):
            raise ValueError(f"RangeNet.forward: feature {feature!r} is none of None, 'decoder', 'lidargen'")
        if img.shape[1] != self.in_ch:
            raise ValueError(f"RangeNet.forward: {img.shape[1]} input channels, the model takes {self.in_ch}")
        x = img.float().contiguous()
        if feature is None:
            return self.plan().run(x, "head")
        h = self.plan().run(x, "decoder")
        return self.flatten_and_subsample(h) if feature == "lidargen" else h

    def extra_repr(self):
        return f"inputs={self.inputs}"


class Preprocess(nn.Module):
    """img * mask (mask: img[:, [0]] > 0 when not given).  `mean` / `std` are kept for the reference's signature: its
    normalisation is switched off there too."""

    def __init__(self, mean=None, std=None):
        super().__init__()
        # (range, x, y, z, remission) order
        if mean is None:
            mean = [12.12, 10.88, 0.23, -1.04, 0.21]
        if std is None:
            std = [12.32, 11.47, 6.91, 0.86, 0.16]
        assert len(mean) == len(std)
        self.num_channels = len(mean)
        self.mean, self.std = list(mean), list(std)

    def forward(self, img: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
        assert img.ndim == 4
        assert img.shape[1] == self.num_channels
        if mask is None:
            mask = (img[:, [0]] > 0).float()
        assert mask.ndim == 4
        return img * mask


def _translate_param_name(src_name: str) -> str:
    """A key of the official checkpoint's three state dicts -> the key of `RangeNet`."""
    p = src_name.split(".")
    if p[0] == "1":
        p[0] = "head.1"
    elif p[0] == "conv1":
        p[0] = "stem.0"
    elif p[0] == "bn1":
        p[0] = "stem.1"
    elif p[1] in ("conv", "upconv"):
        p[1] = "conv.0"
    elif p[1] == "bn":
        p[1] = "conv.1"
    elif p[1] == "residual" or p[1].startswith("residual_"):
        blk = 0 if p[1] == "residual" else int(p[1].split("_")[-1])
        p[1] = f"residual_blocks.{blk}.residual"
        for kind, slot in (("conv", 0), ("bn", 1)):
            if p[2].startswith(kind):
                p[2] = f"{int(p[2][-1]) - 1}.{slot}"
                break
    return ".".join(p)


def _archive_path(url_or_file: str) -> str:
    """Where the archive is read from: the file itself, or for a URL <torch hub dir>/checkpoints/<file name>.  Never
    fetched: FileNotFoundError names the path when nothing is there."""
    url_or_file = os.fspath(url_or_file)
    if os.path.exists(url_or_file):
        return url_or_file
    parts = urlparse(url_or_file)
    if parts.scheme and parts.netloc:
        path = os.path.join(torch.hub.get_dir(), "checkpoints", os.path.basename(parts.path))
        if not os.path.exists(path):
            raise FileNotFoundError(f"rangenet: no archive at {path} (the cache path of {url_or_file}) -- place the file "
                                    "there or pass url_or_file=<local path>; this build does not fetch it")
        return path
    raise FileNotFoundError(f"rangenet: no archive at {url_or_file}; this build does not fetch it")


def _load_pretrained_weights(url_or_file: str):
    """(state dict under RangeNet's keys, Preprocess, constructor arguments) of a .tar.gz with the members
    <arch>/backbone, /segmentation_decoder, /segmentation_head, /arch_cfg.yaml."""
    import yaml

    path = _archive_path(url_or_file)
    arch_cfg, state_dict = None, OrderedDict()
    with tarfile.open(path, "r:gz") as tar:
        members = [m.name for m in tar.getmembers()]
        archs = [_LOCAL_ARCH, os.path.basename(path).replace(".tar.gz", "")] + \
                [m[:-len("/backbone")] for m in members if m.endswith("/backbone")]
        arch = next((a for a in archs if f"{a}/backbone" in members), None)
        if arch is None:
            raise KeyError(f"rangenet: {path} has no member <arch>/backbone")
        for member in (f"{arch}/backbone", f"{arch}/segmentation_decoder", f"{arch}/segmentation_head",
                       f"{arch}/arch_cfg.yaml"):
            if member not in members:
                raise KeyError(f"rangenet: {path} lacks the member {member}")
            stream = io.BytesIO(tar.extractfile(member).read())
            if member.endswith(".yaml"):
                arch_cfg = yaml.safe_load(stream)
                continue
            for name, params in torch.load(stream, map_location="cpu", weights_only=False).items():
                new_name = _translate_param_name(name)
                assert new_name not in state_dict, new_name
                state_dict[new_name] = params.cpu()
    inputs = arch_cfg["backbone"]["input_depth"]
    in_channels = _count_in_ch(inputs)
    sensor = arch_cfg["dataset"]["sensor"]
    cfg = dict(inputs=inputs, num_classes=state_dict["head.1.bias"].shape[0], backbone=arch_cfg["backbone"]["extra"]["layers"])
    return state_dict, Preprocess(mean=sensor["img_means"][:in_channels], std=sensor["img_stds"][:in_channels]), cfg


def build_rangenet(url_or_file, compile: bool = False, device="cpu", **user_cfg: Any):
    """(model, preprocess) from a local archive (or None: a fresh model from `user_cfg`, preprocess None).  `compile` is
    accepted for the reference's signature and ignored (there is nothing for torch.compile to trace)."""
    if url_or_file is not None:
        state_dict, preprocess, loaded_cfg = _load_pretrained_weights(url_or_file)
        preprocess.to(device)
    else:
        state_dict, preprocess, loaded_cfg = None, None, dict()
    model = RangeNet(**loaded_cfg, **user_cfg)
    model.to(device)
    if state_dict is not None:
        model.load_state_dict(state_dict, strict=True)
        model.eval().requires_grad_(False)
    return model, preprocess


def _named_archive(backbone: int, weights: str) -> str:
    if weights not in _ARCHIVES[backbone]:
        raise KeyError(f"rangenet{backbone}: weights {weights!r} is none of {sorted(_ARCHIVES[backbone])}")
    return _OFFICIAL.format(_ARCHIVES[backbone][weights])


def rangenet21(weights=None, compile: bool = False, device="cpu", **user_cfg: Any):
    """RangeNet with the DarkNet-21 backbone.  `weights`: a name of the official archives, read from the hub cache."""
    if weights is not None:
        url_or_file = _named_archive(21, weights)
    else:
        url_or_file = None
        user_cfg["backbone"] = 21
    return build_rangenet(url_or_file=url_or_file, compile=compile, device=device, **user_cfg)


def rangenet53(url_or_file=None, weights=None, compile: bool = False, device="cpu", **user_cfg: Any):
    """RangeNet with the DarkNet-53 backbone from a local archive, a named official archive in the hub cache, or fresh."""
    if url_or_file is None:
        if weights is not None:
            url_or_file = _named_archive(53, weights)
        else:
            user_cfg["backbone"] = 53
    return build_rangenet(url_or_file=url_or_file, compile=compile, device=device, **user_cfg)


def _not_built(name, what):
    def stub(*args, **kwargs):
        raise NotImplementedError(f"extractor.rangenet.{name}: {what} is not built (post-processing of the segmentation, "
                                  "which no score of the evaluator uses)")
    stub.__name__ = name
    return stub


kNN = knn = _not_built("kNN", "the k-NN label filter")
CRFRNN = crf_rnn = _not_built("CRFRNN", "the CRF-RNN refinement")
make_semantickitti_cmap = _not_built("make_semantickitti_cmap", "the SemanticKITTI colour map")
