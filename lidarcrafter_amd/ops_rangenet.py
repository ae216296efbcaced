"""Tensor-level wrappers over the dense RangeNet convolutions of csrc/rangenet.hip (include/lidarcrafter_hip.h:
lc_rangenet_*).  Like ops.py: CUDA(HIP) float32 tensors only, no CPU / eager-PyTorch fallback.  The
BatchNorm fold and the weight packing run on the host (float64 fold, one rounding to float32)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream

# tile extents of RangeNet's geometries of df_conv_kernel (csrc/dense_f32.h; tests/test_rangenet_host.py compares them with
# lc_rangenet_tile_extent)
TILE_W = 32          # pixels per wave: a block row is TILE_W * 4 / CW pixels, CW = 1 (Co <= 32), 2 (Co <= 64) or 4
TILE_H = 2           # output rows per block
TILE_CO = 32         # output channels per wave
TILE_W_MAX = 128     # the widest block row
K_CHUNK = {0: 32, 1: 16, 2: 16, 3: 16}     # input channels per accumulation chunk
TAPS = {0: 1, 1: 9, 2: 9, 3: 4}
REDUCE_KINDS = {"all": 0, "sector": 1, "depth": 2}
BANDS = 16


def out_width(mode: int, W: int) -> int:
    return (W - 1) // 2 + 1 if mode == 2 else (2 * W if mode == 3 else W)


def weight_shape(mode: int, Ci: int, Co: int):
    """The torch shape of a layer's weight: Conv2d [Co,Ci,k,k], ConvTranspose2d [Ci,Co,1,4]."""
    return {0: (Co, Ci, 1, 1), 1: (Co, Ci, 3, 3), 2: (Co, Ci, 3, 3), 3: (Ci, Co, 1, 4)}[mode]


def fold_bn(w, conv_bias, bn, mode: int):
    """(weight, bias) float32 CPU tensors of conv + eval-mode BatchNorm: w * g / sqrt(var + eps) and
    beta - mean * g / sqrt(var + eps) (+ the scaled conv bias), formed in float64 and rounded once.  `bn`: (gamma, beta,
    mean, var, eps) or None (the head: weight and bias as they are)."""
    w64 = w.detach().double().cpu()
    Co = w64.shape[1] if mode == 3 else w64.shape[0]
    b64 = torch.zeros(Co, dtype=torch.float64) if conv_bias is None else conv_bias.detach().double().cpu()
    if bn is not None:
        g, beta, mean, var, eps = bn
        scale = g.detach().double().cpu() / torch.sqrt(var.detach().double().cpu() + float(eps))
        w64 = w64 * (scale.view(1, -1, 1, 1) if mode == 3 else scale.view(-1, 1, 1, 1))
        b64 = beta.detach().double().cpu() + (b64 - mean.detach().double().cpu()) * scale
    return w64.float().contiguous(), b64.float().contiguous()


def packed_weight_elems(mode: int, Ci: int, Co: int) -> int:
    return int(lib().lc_rangenet_packed_weight_elems(mode, Ci, Co))


def pack_weight(w: torch.Tensor, mode: int) -> torch.Tensor:
    """Host: a float32 CPU weight in torch layout -> the float32 CPU vector df_conv_kernel (csrc/dense_f32.h) reads."""
    if w.is_cuda or w.dtype != _F32 or w.dim() != 4:
        raise ValueError("pack_weight: a float32 CPU tensor [Co,Ci,k,k] (mode 3: [Ci,Co,1,4])")
    Ci, Co = (w.shape[0], w.shape[1]) if mode == 3 else (w.shape[1], w.shape[0])
    if mode not in TAPS or tuple(w.shape) != weight_shape(mode, Ci, Co):
        raise ValueError(f"pack_weight: mode {mode} does not take a weight of shape {tuple(w.shape)}")
    w = np.ascontiguousarray(w.numpy())
    out = np.empty(packed_weight_elems(mode, Ci, Co), np.float32)
    check(lib().lc_rangenet_pack_weight(w.ctypes.data, mode, Ci, Co, out.ctypes.data), "lc_rangenet_pack_weight")
    return torch.from_numpy(out)


@_entry
def conv(x: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, mode: int, Co: int, act: bool,
         res1: Optional[torch.Tensor] = None, res2: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = [leaky_relu_0.1](conv_mode(x, w) + bias) + res1 + res2 on contiguous NCHW tensors; `wpk` the device copy of
    pack_weight(w, mode), `bias` [Co].  Zero padding; the modes are those of lc_rangenet_conv_fwd."""
    _req(x, "x")
    _req(wpk, "wpk")
    _req(bias, "bias")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"rangenet.conv: `x` must be contiguous [B,Ci,H,W], got {tuple(x.shape)} strides {x.stride()}")
    if mode not in TAPS:
        raise ValueError(f"rangenet.conv: mode {mode}")
    B, Ci, H, W = x.shape
    if min(B, Ci, H, W) < 1:
        raise ValueError("rangenet.conv: an empty tensor")
    if wpk.numel() != packed_weight_elems(mode, Ci, Co) or not wpk.is_contiguous():
        raise ValueError(f"rangenet.conv: `wpk` has {wpk.numel()} elements, mode {mode} {Ci} -> {Co} packs to "
                         f"{packed_weight_elems(mode, Ci, Co)}")
    if tuple(bias.shape) != (Co,) or not bias.is_contiguous():
        raise ValueError(f"rangenet.conv: `bias` must be contiguous [{Co}]")
    shape = (B, Co, H, out_width(mode, W))
    for r, n in ((res1, "res1"), (res2, "res2")):
        if r is not None:
            _req(r, n)
            if tuple(r.shape) != shape or not r.is_contiguous():
                raise ValueError(f"rangenet.conv: `{n}` must be contiguous {shape}, got {tuple(r.shape)}")
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=_F32)
    _req(out, "out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"rangenet.conv: `out` must be contiguous {shape}, got {tuple(out.shape)}")
    check(lib().lc_rangenet_conv_fwd(x.data_ptr(), wpk.data_ptr(), bias.data_ptr(),
                                     None if res1 is None else res1.data_ptr(), None if res2 is None else res2.data_ptr(),
                                     out.data_ptr(), B, Ci, Co, H, W, mode, 1 if act else 0, _stream()),
          "lc_rangenet_conv_fwd")
    return out


@_entry
def reduce(x: torch.Tensor, kind: str) -> torch.Tensor:
    """The aggregations of the reference's Model.forward on a contiguous [B,C,H,W] map: 'all' -> [B, C] means; 'sector'
    -> [B, 16 C], column c*16+n the mean over all rows and the n-th of 16 column bands; 'depth' -> the same over row
    bands.  H (W) must be a multiple of 16 for 'depth' ('sector')."""
    _req(x, "x")
    if kind not in REDUCE_KINDS:
        raise ValueError(f"rangenet.reduce: kind {kind!r} is none of {sorted(REDUCE_KINDS)}")
    if x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"rangenet.reduce: `x` must be contiguous non-empty [B,C,H,W], got {tuple(x.shape)}")
    B, C, H, W = x.shape
    if (kind == "depth" and H % BANDS) or (kind == "sector" and W % BANDS):
        raise ValueError(f"rangenet.reduce: '{kind}' needs {'H' if kind == 'depth' else 'W'} % {BANDS} == 0, got {H}x{W}")
    out = torch.empty((B, C * (1 if kind == "all" else BANDS)), device=x.device, dtype=_F32)
    check(lib().lc_rangenet_reduce_fwd(x.data_ptr(), out.data_ptr(), B, C, H, W, REDUCE_KINDS[kind], _stream()),
          "lc_rangenet_reduce_fwd")
    return out
