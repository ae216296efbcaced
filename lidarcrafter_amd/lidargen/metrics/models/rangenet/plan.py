"""The one forward plan of RangeNet++ (DarkNet-21 / -53 encoder and decoder): a list of convolution calls over folded,
packed weights (lidarcrafter_amd.ops_rangenet, csrc/rangenet.hip).  Both module trees that carry the network --
`models.rangenet.model.Model` (FRID) and `extractor.rangenet.RangeNet` (FRD) -- describe themselves as a list of `Layer`s
and run through `Plan.run`; nothing else computes a convolution of this network.

    stem   3x3                              -> h0
    enc_i  3x3 stride (1,2), then n_i blocks [1x1 to half the width, 3x3 back, + block input]        i = 1 .. 5
    dec_i  transposed 1x4 stride (1,2), then one block [1x1 to twice the width, 3x3 back, + block input + skip h_{i-1}]
    head   3x3 with bias, no activation (the extractor tree only)

Every conv but the head is followed by eval-mode BatchNorm (folded into weight and bias on the host, float64, rounded
once) and LeakyReLU(0.1); the addends come after the activation, the block input first.  Dropout is the identity in eval
mode, the only mode there is."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn

from lidarcrafter_amd import ops_rangenet as KR

MODEL_BLOCKS = {21: [1, 1, 2, 2, 1], 53: [1, 2, 8, 8, 4]}


@dataclass
class Layer:
    conv: nn.Module                      # Conv2d / ConvTranspose2d: weight, maybe bias
    bn: Optional[nn.Module]              # BatchNorm2d or None
    mode: int                            # ops_rangenet.conv mode
    act: bool
    tag: str                             # 'stem', 'down', 'up', 'c1', 'c2', 'head'


def flops_per_pixel(layers: int = 53, in_ch: int = 5, head: int = 0) -> float:
    """Multiply-adds per full-resolution pixel of the encoder + decoder (+ a head of `head` classes): the formula of
    DESIGN.md section 5n.  Level i (i = 0 full width) has 2^-i of the pixels and width c_i = 32 * 2^i."""
    ch = lambda i: 32 << i
    macs = 9.0 * in_ch * 32
    for i, n in enumerate(MODEL_BLOCKS[layers], start=1):
        px = 2.0 ** -i
        macs += px * 9 * ch(i - 1) * ch(i)                                  # down conv, output pixels
        macs += px * n * (ch(i) * ch(i - 1) + 9 * ch(i - 1) * ch(i))        # blocks
    for i in range(5, 0, -1):
        px = 2.0 ** -(i - 1)
        macs += px * 2 * ch(i) * ch(i - 1)                                  # up conv: two taps per output pixel
        macs += px * (ch(i - 1) * ch(i) + 9 * ch(i) * ch(i - 1))            # block
    return macs + 9.0 * 32 * head


def _tensors(layer: Layer):
    ts = [layer.conv.weight, layer.conv.bias]
    if layer.bn is not None:
        ts += [layer.bn.weight, layer.bn.bias, layer.bn.running_mean, layer.bn.running_var]
    return [t for t in ts if t is not None]


class Plan:
    """The layer list of one module tree with its packed weights, cached under the parameters' addresses and versions
    (an in-place change of a weight or a BatchNorm buffer bumps the version: the next call folds and packs again)."""

    def __init__(self, layers):
        self.layers = list(layers)
        self._key = None
        self._packed = None

    def packed(self, device):
        key = (str(device),) + tuple((t.data_ptr(), t._version) for L in self.layers for t in _tensors(L))
        if key != self._key:
            packed = []
            for L in self.layers:
                bn = None if L.bn is None else (L.bn.weight, L.bn.bias, L.bn.running_mean, L.bn.running_var, L.bn.eps)
                w, b = KR.fold_bn(L.conv.weight, L.conv.bias, bn, L.mode)
                packed.append((KR.pack_weight(w, L.mode).to(device), b.to(device), b.numel()))
            self._packed, self._key = packed, key
        return self._packed

    def run(self, x: torch.Tensor, want: str = "decoder") -> torch.Tensor:
        """x: contiguous CUDA float32 [B, Ci, H, W].  want: 'encoder' (the last encoder map), 'decoder' (the [B,32,H,W]
        map), 'head' (the logits)."""
        packed = self.packed(x.device)
        skips, h, blk_in, skip = [], x, None, None
        for L, (wpk, bias, Co) in zip(self.layers, packed):
            if L.tag == "up" and want == "encoder":
                return h
            if L.tag == "head" and want != "head":
                return h
            if L.tag == "down":
                skips.append(h)
            if L.tag == "c1":
                blk_in, h = h, KR.conv(h, wpk, bias, L.mode, Co, L.act)
            elif L.tag == "c2":
                h = KR.conv(h, wpk, bias, L.mode, Co, L.act, res1=blk_in, res2=skip)
                blk_in = skip = None
            else:
                h = KR.conv(h, wpk, bias, L.mode, Co, L.act)
                if L.tag == "up":
                    skip = skips.pop()
        if want == "head" and self.layers[-1].tag != "head":
            raise ValueError("Plan.run: this tree has no head")
        return h


def check_call(module: nn.Module, x, who: str) -> None:
    """The refusals both trees share: training mode, grad mode, CPU tensors."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{who}: the input must be a tensor, got {type(x).__name__}")
    if module.training:
        raise NotImplementedError(f"{who}: training mode is not built (BatchNorm is folded, Dropout2d dropped); call "
                                  ".eval()")
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())):
        raise NotImplementedError(f"{who}: grad mode is not built (no backward kernels); call under torch.no_grad() or "
                                  "requires_grad_(False)")
    if not x.is_cuda:
        raise RuntimeError(f"{who}: the input must be a CUDA(HIP) tensor -- no CPU fallback on the hot path")
    if x.dim() != 4:
        raise ValueError(f"{who}: the input must be [B, C, H, W], got {tuple(x.shape)}")
