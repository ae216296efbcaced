"""Tensor-level wrappers over csrc/metric_preprocess.hip (include/lidarcrafter_hip.h: lc_range_batch_fwd, lc_voxel_batch_*;
DESIGN.md section 5u): the step in front of the FRID / FSVD / FPVD networks for a ragged batch of clouds -- one contiguous
[N, 3] buffer of float32 or float64 points and int32 offsets [B + 1].  Like ops_stats.py: CUDA(HIP) tensors only, no CPU /
eager-PyTorch fallback.  The front-end is lidargen/metrics/metric_utils.py (preprocess_range_batch, pcd2voxel_batch)."""
from __future__ import annotations

import ctypes
import threading
from typing import Sequence, Tuple

import numpy as np
import torch

from ._lib import check, lib
from .ops import _entry, _stream

_DTYPES = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def _device(device, need_gpu: bool = True) -> torch.device:
    """The CUDA(HIP) device of the route; anything else -- and a missing GPU -- raises, there is no fallback."""
    try:
        dev = torch.device(device)
    except (RuntimeError, TypeError) as e:
        raise ValueError(f"metric preprocessing on the device: `{device}` is not a device") from e
    if dev.type != "cuda":
        raise ValueError(f"metric preprocessing on the device: `{device}` is not a CUDA(HIP) device")
    if not need_gpu:
        return dev
    if not torch.cuda.is_available():
        raise RuntimeError("metric preprocessing on the device needs the MI355X: no CPU fallback on the hot path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def ragged(clouds: Sequence, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """[N_i, 3] clouds -> (points [N, 3] on the device, offsets int32 [B + 1] on the device).
    numpy clouds are concatenated on the host and uploaded in one copy, CUDA tensors are concatenated on the device.  All
    clouds of a batch are of one kind and one dtype, float32 or float64."""
    clouds = list(clouds)
    if not clouds:
        raise ValueError("metric preprocessing: an empty batch")
    dev = _device(device)
    for c in clouds:
        if c.ndim != 2 or c.shape[1] != 3:
            raise ValueError(f"metric preprocessing: a cloud must be [N, 3], got {tuple(c.shape)}")
    if all(isinstance(c, np.ndarray) for c in clouds):
        if len({c.dtype for c in clouds}) != 1 or clouds[0].dtype not in _DTYPES:
            raise TypeError(f"metric preprocessing: clouds must share one dtype, float32 or float64, got "
                            f"{sorted({str(c.dtype) for c in clouds})}")
        pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds, axis=0))).to(dev)
    elif all(isinstance(c, torch.Tensor) and c.is_cuda for c in clouds):
        if len({c.dtype for c in clouds}) != 1 or clouds[0].dtype not in _DTYPES.values():
            raise TypeError(f"metric preprocessing: clouds must share one dtype, float32 or float64, got "
                            f"{sorted({str(c.dtype) for c in clouds})}")
        pts = torch.cat([c.to(dev) for c in clouds], dim=0).contiguous()
    else:
        raise TypeError("metric preprocessing: a batch is numpy arrays or CUDA(HIP) tensors, not a mixture (and not CPU tensors)")
    offs = [0]
    for c in clouds:
        offs.append(offs[-1] + int(c.shape[0]))
    if offs[-1] >= 2 ** 31:
        raise NotImplementedError(f"metric preprocessing: {offs[-1]} points in one batch do not fit the kernels' int32 indices")
    return pts, torch.tensor(offs, dtype=torch.int32).to(dev)


def _batch(pts: torch.Tensor, offsets: torch.Tensor, who: str) -> Tuple[int, int]:
    if not isinstance(pts, torch.Tensor) or not pts.is_cuda or not isinstance(offsets, torch.Tensor) or not offsets.is_cuda:
        raise RuntimeError(f"{who}: points and offsets must be CUDA(HIP) tensors -- the hot path has no CPU fallback")
    if pts.dtype not in _DTYPES.values() or pts.dim() != 2 or pts.shape[1] != 3 or not pts.is_contiguous():
        raise ValueError(f"{who}: points must be contiguous float32 / float64 [N, 3], got {pts.dtype} {tuple(pts.shape)}")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
        raise ValueError(f"{who}: offsets must be contiguous int32 [B + 1], B >= 1")
    return int(offsets.numel()) - 1, int(pts.shape[0])


# ---------------------------------------------------------------------------------------------------------------------
# range images

def _fov_terms(fov) -> Tuple[float, float]:
    """(|fov_down|, |fov_down| + |fov_up|) in radians, by pcd2range's own lines."""
    fov_up, fov_down = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
    return float(abs(fov_down)), float(abs(fov_down) + abs(fov_up))


def ray_directions_host(H: int, W: int, fov) -> np.ndarray:
    """float64 [3, H, W]: cos(yaw) cos(pitch), -sin(yaw) cos(pitch), sin(pitch) at scan_x = j / W, scan_y = i / H, by
    range2xyz's numpy lines -- what that function multiplies the depth image with."""
    size = (int(H), int(W))
    fov_up, fov_down = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
    fov_range = abs(fov_down) + abs(fov_up)
    scan_x, scan_y = np.meshgrid(np.arange(size[1]), np.arange(size[0]))
    scan_x = scan_x.astype(np.float64) / size[1]
    scan_y = scan_y.astype(np.float64) / size[0]
    yaw = np.pi * (scan_x * 2 - 1)
    pitch = (1.0 - scan_y) * fov_range - abs(fov_down)
    return np.stack([np.cos(yaw) * np.cos(pitch), -np.sin(yaw) * np.cos(pitch), np.sin(pitch)])


# One table per (H, W, fov, device): it outlives a call (tests/test_metric_preprocess.py runs a call sequence over it).
_DIRS: dict = {}
_DIRS_LOCK = threading.Lock()
DIRS_BUILT = 0          # tables computed so far (the call-sequence test reads it)


def ray_directions(H: int, W: int, fov, device) -> torch.Tensor:
    global DIRS_BUILT
    dev = _device(device)
    key = (int(H), int(W), float(fov[0]), float(fov[1]), dev.index)
    with _DIRS_LOCK:
        t = _DIRS.get(key)
        if t is None:
            t = _DIRS[key] = torch.from_numpy(ray_directions_host(H, W, fov)).to(dev)
            DIRS_BUILT += 1
    return t


@_entry
def range_images(pts: torch.Tensor, offsets: torch.Tensor, size, fov, depth_range) -> torch.Tensor:
    """float32 [B, 4, H, W] = (depth, x, y, z): preprocess_range of every cloud widened to float64, the nearest point of a
    pixel wins, -1 where none falls (depth) or the float32 depth is outside the open `depth_range` (x, y, z)."""
    B, N = _batch(pts, offsets, "ops_metric_pre.range_images")
    H, W = int(size[0]), int(size[1])
    lo, hi = float(depth_range[0]), float(depth_range[1])
    if H < 1 or W < 1 or not (0.0 <= lo < hi):
        raise ValueError(f"ops_metric_pre.range_images: size {tuple(size)} / depth_range {tuple(depth_range)}")
    down, span = _fov_terms(fov)
    dirs = ray_directions(H, W, fov, pts.device)
    zbuf = torch.empty((B, H, W), device=pts.device, dtype=torch.int32)
    out = torch.empty((B, 4, H, W), device=pts.device, dtype=torch.float32)
    check(lib().lc_range_batch_fwd(pts.data_ptr() if N else None, int(pts.dtype == torch.float64), offsets.data_ptr(), B, N, H,
                                   W, lo, hi, float(np.float32(lo)), float(np.float32(hi)), down, span, dirs.data_ptr(),
                                   zbuf.data_ptr(), out.data_ptr(), _stream()), "lc_range_batch_fwd")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# voxels

def voxel_key_bits(B: int, hi: float, voxel: float) -> Tuple[int, int]:
    """(bits of the cloud field, bits of the three axis fields) of the batch's sort key; NotImplementedError by name when
    they exceed 64 together (host code, no GPU)."""
    bits = (ctypes.c_int32 * 2)()
    code = lib().lc_voxel_batch_key_bits(int(B), float(hi), float(voxel), bits)
    if code == -2:
        raise NotImplementedError(f"voxel batch sort key: {bits[0]} cloud-index bits ({B} clouds) plus {bits[1]} key bits "
                                  f"(depth below {hi} at voxel size {voxel}) exceed 64")
    check(code, "lc_voxel_batch_key_bits")
    return int(bits[0]), int(bits[1])


@_entry
def voxelize(pts: torch.Tensor, offsets: torch.Tensor, depth_range, voxel: float):
    """(feats float32 [n, 4], coords int32 [n, 4] = (x, y, z, cloud), offsets int32 [B + 1]): per cloud the points with
    depth_range[0] < |p| < depth_range[1], rint(p / voxel) minus its per-cloud minimum, unique in ravel-hash order, each
    voxel with its first point and -1 -- filter and quotient in the dtype of `pts`.  One device->host read (n)."""
    B, N = _batch(pts, offsets, "ops_metric_pre.voxelize")
    lo, hi = float(depth_range[0]), float(depth_range[1])
    if not (0.0 <= lo < hi) or not voxel > 0:
        raise ValueError(f"ops_metric_pre.voxelize: depth_range {tuple(depth_range)} / voxel {voxel}")
    voxel_key_bits(B, hi, voxel)
    dev = pts.device
    if N == 0:
        return (torch.zeros((0, 4), device=dev), torch.zeros((0, 4), device=dev, dtype=torch.int32),
                torch.zeros(B + 1, device=dev, dtype=torch.int32))
    scratch = torch.empty(int(lib().lc_voxel_batch_scratch_bytes(N, B)), device=dev, dtype=torch.uint8)
    feats = torch.empty((N, 4), device=dev, dtype=torch.float32)
    coords = torch.empty((N, 4), device=dev, dtype=torch.int32)
    out_off = torch.empty(B + 1, device=dev, dtype=torch.int32)
    check(lib().lc_voxel_batch_fwd(pts.data_ptr(), int(pts.dtype == torch.float64), offsets.data_ptr(), B, N, lo, hi,
                                   float(voxel), scratch.data_ptr(), feats.data_ptr(), coords.data_ptr(), out_off.data_ptr(),
                                   _stream()), "lc_voxel_batch_fwd")
    n = int(out_off[B].item())                 # the one read-back of the batch
    return feats[:n], coords[:n], out_off
