"""Tensor-level wrappers over the PointMLP kernels of csrc/pointmlp.hip (include/lidarcrafter_hip.h: lc_fps_fwd, lc_knn_fwd,
lc_pointmlp_*).  Like ops.py: CUDA(HIP) float32 / int32 tensors only, no CPU / eager-PyTorch
fallback.  The BatchNorm fold and the weight packing run on the host."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream

_I32 = torch.int32


def limit(which: str) -> int:
    """The kernels' limits and tile extents: 'fps_max_n', 'knn_max_n', 'knn_max_k', 'k_chunk', 'tile_co', 'tile_l',
    'group_cols'."""
    names = ("fps_max_n", "knn_max_n", "knn_max_k", "k_chunk", "tile_co", "tile_l", "group_cols")
    return int(lib().lc_pointmlp_limit(names.index(which)))


def conv_block_cols(Co: int) -> int:
    """Columns per block of the pointwise geometry (csrc/dense_pointwise.h: PwGeom) for a layer of Co output channels (256 for
    Co <= 32, 128 for Co <= 64, else 64)."""
    return limit("tile_l") * (4 if Co <= 32 else (2 if Co <= 64 else 1))


def _req_i32(t: torch.Tensor, name: str, shape) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ops_pointmlp: `{name}` must be a CUDA(HIP) tensor -- the hot path has no CPU fallback")
    if t.dtype != _I32:
        raise TypeError(f"`{name}` must be int32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"`{name}` must be contiguous {tuple(shape)}, got {tuple(t.shape)}")


def _req_xyz(xyz: torch.Tensor, who: str):
    _req(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.shape[0] < 1 or xyz.shape[1] < 1 or not xyz.is_contiguous():
        raise ValueError(f"{who}: `xyz` must be contiguous [B,N,3], got {tuple(xyz.shape)} strides {xyz.stride()}")
    return xyz.shape[0], xyz.shape[1]


@_entry
def fps(xyz: torch.Tensor, npoint: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [B, npoint]: the farthest-point sequence of every cloud of `xyz` [B,N,3] from index 0, the reference
    kernel's picks index for index (its distance expression and its tie rule).  Coordinates must be finite."""
    B, N = _req_xyz(xyz, "fps")
    npoint = int(npoint)
    if npoint < 1:
        raise ValueError(f"fps: npoint = {npoint}")
    if out is None:
        out = torch.empty((B, npoint), device=xyz.device, dtype=_I32)
    _req_i32(out, "out", (B, npoint))
    check(lib().lc_fps_fwd(xyz.data_ptr(), out.data_ptr(), B, N, npoint, _stream()), "lc_fps_fwd")
    return out


@_entry
def knn(xyz: torch.Tensor, query_idx: torch.Tensor, K: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [B,S,K]: the K points of `xyz` [B,N,3] nearest to xyz[b, query_idx[b,s]], ascending (distance, index)."""
    B, N = _req_xyz(xyz, "knn")
    if query_idx.dim() != 2:
        raise ValueError(f"knn: `query_idx` must be [B,S], got {tuple(query_idx.shape)}")
    S, K = query_idx.shape[1], int(K)
    _req_i32(query_idx, "query_idx", (B, S))
    if S < 1 or K < 1:
        raise ValueError(f"knn: S = {S}, K = {K}")
    if out is None:
        out = torch.empty((B, S, K), device=xyz.device, dtype=_I32)
    _req_i32(out, "out", (B, S, K))
    check(lib().lc_knn_fwd(xyz.data_ptr(), query_idx.data_ptr(), out.data_ptr(), B, N, S, K, _stream()), "lc_knn_fwd")
    return out


def group_scratch_elems(B: int, S: int, K: int) -> int:
    return int(lib().lc_pointmlp_group_scratch_elems(B, S, K))


@_entry
def group(x: torch.Tensor, fps_idx: torch.Tensor, knn_idx: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor,
          out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None,
          sigma: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The operand of a stage's `transfer` layer, [B, 2d, S K], from the stage input `x` [B,d,N]: rows 0..d-1
    alpha (x[knn] - x[anchor]) / (sigma_b + 1e-5) + beta, rows d..2d-1 x[anchor]; `sigma` [B] (optional) receives the
    unbiased deviation per cloud.  `scratch`: float64, at least group_scratch_elems(B,S,K) elements."""
    for t, n in ((x, "x"), (alpha, "alpha"), (beta, "beta")):
        _req(t, n)
    if x.dim() != 3 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"group: `x` must be contiguous non-empty [B,d,N], got {tuple(x.shape)}")
    B, d, N = x.shape
    if knn_idx.dim() != 3:
        raise ValueError(f"group: `knn_idx` must be [B,S,K], got {tuple(knn_idx.shape)}")
    S, K = knn_idx.shape[1], knn_idx.shape[2]
    _req_i32(fps_idx, "fps_idx", (B, S))
    _req_i32(knn_idx, "knn_idx", (B, S, K))
    for t, n in ((alpha, "alpha"), (beta, "beta")):
        if t.numel() != d or not t.is_contiguous():
            raise ValueError(f"group: `{n}` must hold {d} contiguous values, got {tuple(t.shape)}")
    if out is None:
        out = torch.empty((B, 2 * d, S * K), device=x.device, dtype=_F32)
    _req(out, "out")
    if tuple(out.shape) != (B, 2 * d, S * K) or not out.is_contiguous():
        raise ValueError(f"group: `out` must be contiguous {(B, 2 * d, S * K)}, got {tuple(out.shape)}")
    need = group_scratch_elems(B, S, K)
    if scratch is None:
        scratch = torch.empty(need, device=x.device, dtype=torch.float64)
    if not scratch.is_cuda or scratch.dtype != torch.float64 or scratch.numel() < need or not scratch.is_contiguous():
        raise ValueError(f"group: `scratch` must be a contiguous float64 CUDA tensor of at least {need} elements")
    if sigma is not None:
        _req(sigma, "sigma")
        if tuple(sigma.shape) != (B,) or not sigma.is_contiguous():
            raise ValueError(f"group: `sigma` must be contiguous [{B}]")
    check(lib().lc_pointmlp_group_fwd(x.data_ptr(), fps_idx.data_ptr(), knn_idx.data_ptr(), alpha.data_ptr(), beta.data_ptr(),
                                      out.data_ptr(), scratch.data_ptr(), None if sigma is None else sigma.data_ptr(),
                                      B, d, N, S, K, _stream()), "lc_pointmlp_group_fwd")
    return out


def packed_weight_elems(Ci: int, Co: int) -> int:
    return int(lib().lc_pointmlp_packed_weight_elems(Ci, Co))


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """Host: a float32 CPU weight [Co,Ci] -> the float32 CPU vector df_conv_kernel (csrc/dense_f32.h) reads:
    ops_rangenet.pack_weight's at one tap."""
    if w.is_cuda or w.dtype != _F32 or w.dim() != 2 or w.numel() == 0:
        raise ValueError("pack_weight: a non-empty float32 CPU tensor [Co,Ci]")
    Co, Ci = w.shape
    w = np.ascontiguousarray(w.numpy())
    out = np.empty(packed_weight_elems(Ci, Co), np.float32)
    check(lib().lc_pointmlp_pack_weight(w.ctypes.data, Ci, Co, out.ctypes.data), "lc_pointmlp_pack_weight")
    return torch.from_numpy(out)


@_entry
def conv(x: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, Co: int, act: bool, res: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [B,Co,L] = [relu](W x + bias [+ res]) on contiguous [B,Ci,L]; `wpk` the device copy of pack_weight(W)."""
    for t, n in ((x, "x"), (wpk, "wpk"), (bias, "bias")):
        _req(t, n)
    if x.dim() != 3 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"pointmlp.conv: `x` must be contiguous non-empty [B,Ci,L], got {tuple(x.shape)} strides {x.stride()}")
    B, Ci, L = x.shape
    if Co < 1 or wpk.numel() != packed_weight_elems(Ci, Co) or not wpk.is_contiguous():
        raise ValueError(f"pointmlp.conv: `wpk` has {wpk.numel()} elements, {Ci} -> {Co} packs to {packed_weight_elems(Ci, Co)}")
    if tuple(bias.shape) != (Co,) or not bias.is_contiguous():
        raise ValueError(f"pointmlp.conv: `bias` must be contiguous [{Co}]")
    shape = (B, Co, L)
    if res is not None:
        _req(res, "res")
        if tuple(res.shape) != shape or not res.is_contiguous():
            raise ValueError(f"pointmlp.conv: `res` must be contiguous {shape}, got {tuple(res.shape)}")
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=_F32)
    _req(out, "out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"pointmlp.conv: `out` must be contiguous {shape}, got {tuple(out.shape)}")
    check(lib().lc_pointmlp_conv_fwd(x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), None if res is None else res.data_ptr(),
                                     out.data_ptr(), B, Ci, Co, L, 1 if act else 0, _stream()), "lc_pointmlp_conv_fwd")
    return out


@_entry
def groupmax(x: torch.Tensor, K: int, out: Optional[torch.Tensor] = None, channel_major: bool = False) -> torch.Tensor:
    """[B,C,G] = the maximum over every group of K consecutive columns of `x` [B,C,G K].  channel_major (G must be 1): the
    result is written as [1,C,B], the operand layout of a dense layer with the batch as its columns."""
    _req(x, "x")
    K = int(K)
    if x.dim() != 3 or not x.is_contiguous() or x.numel() == 0 or K < 1 or x.shape[2] % K:
        raise ValueError(f"groupmax: `x` must be contiguous non-empty [B,C,G*{K}], got {tuple(x.shape)}")
    B, C, G = x.shape[0], x.shape[1], x.shape[2] // K
    if channel_major and G != 1:
        raise ValueError("groupmax: channel_major needs one group per row")
    shape = (1, C, B) if channel_major else (B, C, G)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=_F32)
    _req(out, "out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"groupmax: `out` must be contiguous {shape}, got {tuple(out.shape)}")
    bs, cs, gs = (1, B, 1) if channel_major else (C * G, G, 1)
    check(lib().lc_pointmlp_groupmax_fwd(x.data_ptr(), out.data_ptr(), B, C, G, K, bs, cs, gs, _stream()),
          "lc_pointmlp_groupmax_fwd")
    return out
