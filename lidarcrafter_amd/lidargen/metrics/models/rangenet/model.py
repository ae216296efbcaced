"""RangeNet++ under the state-dict names of the reference's `lidargen/metrics/models/rangenet/model.py` (lidar-bonnetal's
DarkNet backbone and decoder): `backbone.conv1.weight`, `backbone.enc3.residual_5.conv2.weight`, `decoder.dec5.upconv.bias`,
the `num_batches_tracked` buffers.  The modules hold parameters only; the forward is `plan.Plan` over the HIP convolutions
of csrc/rangenet.hip, in eval mode and without autograd.

Built: `layers` 21 and 53, every combination of the `input_depth` flags, OS = 32, the decoder map, `return_logits` (the
pooled encoder output) and `return_final_logits` with the three aggregations.  Refused by name (NotImplementedError):
OS != 32, `return_list`, training mode, grad mode.  A CPU tensor raises RuntimeError: there is no CPU fallback."""
from __future__ import annotations

import os
from collections import OrderedDict

import torch
from torch import nn

from lidarcrafter_amd import ops_rangenet as KR

from .plan import MODEL_BLOCKS, Layer, Plan, check_call

model_blocks = MODEL_BLOCKS


def _no_forward(self, *args, **kwargs):
    raise NotImplementedError(f"{type(self).__name__}.forward is not built on its own: the network runs as one plan "
                              "through Model.forward")


class BasicBlock(nn.Module):
    """1x1 to planes[0], 3x3 to planes[1], each with BatchNorm and LeakyReLU(0.1); the input is added after the second."""

    def __init__(self, inplanes, planes, bn_d=0.1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes[0], kernel_size=1, stride=1, padding=0, bias=False)
        self.bn1 = nn.BatchNorm2d(planes[0], momentum=bn_d)
        self.relu1 = nn.LeakyReLU(0.1)
        self.conv2 = nn.Conv2d(planes[0], planes[1], kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes[1], momentum=bn_d)
        self.relu2 = nn.LeakyReLU(0.1)

    forward = _no_forward

    def plan_layers(self):
        return [Layer(self.conv1, self.bn1, 0, True, "c1"), Layer(self.conv2, self.bn2, 1, True, "c2")]


def _require_os32(params_os, who):
    if params_os != 32:
        raise NotImplementedError(f"{who}: OS = {params_os} is not built; only the output stride 32 of the pretrained "
                                  "checkpoints (five (1,2) strides) is")


class Backbone(nn.Module):
    def __init__(self, params):
        super().__init__()
        self.use_range = params["input_depth"]["range"]
        self.use_xyz = params["input_depth"]["xyz"]
        self.use_remission = params["input_depth"]["remission"]
        self.drop_prob = params["dropout"]
        self.bn_d = params["bn_d"]
        self.OS = params["OS"]
        self.layers = params["extra"]["layers"]
        _require_os32(self.OS, "Backbone")
        self.input_idxs = ([0] if self.use_range else []) + ([1, 2, 3] if self.use_xyz else []) + \
                          ([4] if self.use_remission else [])
        self.input_depth = len(self.input_idxs)
        if self.input_depth < 1:
            raise ValueError("Backbone: no input channel selected")
        self.strides = [2, 2, 2, 2, 2]
        if self.layers not in model_blocks:
            raise ValueError(f"Backbone: layers = {self.layers} is none of {sorted(model_blocks)}")
        self.blocks = model_blocks[self.layers]

        self.conv1 = nn.Conv2d(self.input_depth, 32, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(32, momentum=self.bn_d)
        self.relu1 = nn.LeakyReLU(0.1)
        for i, n in enumerate(self.blocks, start=1):
            setattr(self, f"enc{i}", self._make_enc_layer([16 << i, 32 << i], n, self.bn_d))
        self.dropout = nn.Dropout2d(self.drop_prob)
        self.last_channels = 1024

    @staticmethod
    def _make_enc_layer(planes, blocks, bn_d):
        layers = [("conv", nn.Conv2d(planes[0], planes[1], kernel_size=3, stride=[1, 2], dilation=1, padding=1, bias=False)),
                  ("bn", nn.BatchNorm2d(planes[1], momentum=bn_d)),
                  ("relu", nn.LeakyReLU(0.1))]
        layers += [(f"residual_{i}", BasicBlock(planes[1], planes, bn_d)) for i in range(blocks)]
        return nn.Sequential(OrderedDict(layers))

    forward = _no_forward

    def plan_layers(self):
        out = [Layer(self.conv1, self.bn1, 1, True, "stem")]
        for i, n in enumerate(self.blocks, start=1):
            enc = getattr(self, f"enc{i}")
            out.append(Layer(enc.conv, enc.bn, 2, True, "down"))
            for r in range(n):
                out += getattr(enc, f"residual_{r}").plan_layers()
        return out

    def get_last_depth(self):
        return self.last_channels

    def get_input_depth(self):
        return self.input_depth


class Decoder(nn.Module):
    def __init__(self, params, OS=32, feature_depth=1024):
        super().__init__()
        self.backbone_OS = OS
        self.backbone_feature_depth = feature_depth
        self.drop_prob = params["dropout"]
        self.bn_d = params["bn_d"]
        _require_os32(OS, "Decoder")
        self.strides = [2, 2, 2, 2, 2]
        widths = [feature_depth, 512, 256, 128, 64, 32]
        for k, i in enumerate(range(5, 0, -1)):
            setattr(self, f"dec{i}", self._make_dec_layer([widths[k], widths[k + 1]], self.bn_d))
        self.layers = [self.dec5, self.dec4, self.dec3, self.dec2, self.dec1]
        self.dropout = nn.Dropout2d(self.drop_prob)
        self.last_channels = 32

    @staticmethod
    def _make_dec_layer(planes, bn_d):
        return nn.Sequential(OrderedDict([
            ("upconv", nn.ConvTranspose2d(planes[0], planes[1], kernel_size=[1, 4], stride=[1, 2], padding=[0, 1])),
            ("bn", nn.BatchNorm2d(planes[1], momentum=bn_d)),
            ("relu", nn.LeakyReLU(0.1)),
            ("residual", BasicBlock(planes[1], planes, bn_d))]))

    forward = _no_forward

    def plan_layers(self):
        out = []
        for dec in self.layers:
            out.append(Layer(dec.upconv, dec.bn, 3, True, "up"))
            out += dec.residual.plan_layers()
        return out

    def get_last_depth(self):
        return self.last_channels


class Model(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.backbone = Backbone(params=self.config["backbone"])
        self.decoder = Decoder(params=self.config["decoder"], OS=self.config["backbone"]["OS"],
                               feature_depth=self.backbone.get_last_depth())
        self._plan = None

    def load_pretrained_weights(self, path):
        """The state dicts `<path>/backbone` and `<path>/segmentation_decoder`, strictly."""
        for name, module in (("backbone", self.backbone), ("segmentation_decoder", self.decoder)):
            f = os.path.join(os.fspath(path), name)
            if not os.path.isfile(f):
                raise FileNotFoundError(f"Model.load_pretrained_weights: {f} is missing; this build does not fetch it")
            module.load_state_dict(torch.load(f, map_location="cpu", weights_only=False), strict=True)

    def plan(self) -> Plan:
        if self._plan is None:
            self._plan = Plan(self.backbone.plan_layers() + self.decoder.plan_layers())
        return self._plan

    def forward(self, x, return_logits=False, return_final_logits=False, return_list=None, agg_type="depth"):
        """default: the decoder map [B,32,H,W] (a CUDA tensor); return_logits: the encoder output averaged over the map,
        squeezed, as numpy; return_final_logits: the decoder map aggregated by `agg_type` ('all' [B,32], 'sector' /
        'depth' [B,512]: 16 column / row bands per channel) as numpy."""
        if return_list is not None:
            raise NotImplementedError("Model.forward: return_list (the per-level dictionaries) is not built")
        check_call(self, x, "Model.forward")
        x = x[:, self.backbone.input_idxs].float().contiguous()
        if return_logits:
            return KR.reduce(self.plan().run(x, "encoder"), "all").squeeze().cpu().numpy()
        y = self.plan().run(x, "decoder")
        if return_final_logits:
            assert agg_type in ["all", "sector", "depth"]
            return KR.reduce(y, agg_type).cpu().numpy()
        return y
