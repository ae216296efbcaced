"""Tensor-level wrappers over the rotated-box kernels of csrc/iou3d_nms.hip (include/lidarcrafter_hip.h:
lc_boxes_iou_pairwise_fwd, lc_boxes_iou_aligned_fwd, lc_nms_mask_fwd, lc_nms_select_fwd).  Like
ops.py: CUDA(HIP) float32 tensors only, no CPU / eager-PyTorch fallback.  Boxes are rows [x, y, z, dx, dy, dz, heading]."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream

NMS_MAX_BOXES = 65536          # include/lidarcrafter_hip.h LC_NMS_MAX_BOXES: the mask of more boxes would pass 512 MiB
WORD = 64                      # boxes per mask word
_OVERLAP, _IOU_BEV, _IOU_3D = 0, 1, 2


def _boxes(t: torch.Tensor, name: str, who: str) -> int:
    _req(t, name)
    if t.dim() != 2 or t.shape[1] != 7 or not t.is_contiguous():
        raise ValueError(f"{who}: `{name}` must be contiguous [N,7], got {tuple(t.shape)}")
    return t.shape[0]


def _pairwise(a: torch.Tensor, b: torch.Tensor, mode: int, who: str) -> torch.Tensor:
    N, M = _boxes(a, "boxes_a", who), _boxes(b, "boxes_b", who)
    out = torch.empty((N, M), device=a.device, dtype=_F32)
    if N and M:
        check(lib().lc_boxes_iou_pairwise_fwd(a.data_ptr(), N, b.data_ptr(), M, mode, out.data_ptr(), _stream()),
              "lc_boxes_iou_pairwise_fwd")
    return out


@_entry
def boxes_overlap_bev(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """[N,M]: the overlap area of the rotated BEV rectangles of every pair."""
    return _pairwise(boxes_a, boxes_b, _OVERLAP, "boxes_overlap_bev")


@_entry
def boxes_iou_bev(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """[N,M]: overlap / max(sa + sb - overlap, 1e-8) of every pair."""
    return _pairwise(boxes_a, boxes_b, _IOU_BEV, "boxes_iou_bev")


@_entry
def boxes_iou3d(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """[N,M]: the 3-D IoU of every pair -- the BEV overlap times the height overlap over the union of the volumes, the
    reference's torch expressions in their order."""
    return _pairwise(boxes_a, boxes_b, _IOU_3D, "boxes_iou3d")


@_entry
def boxes_aligned_iou3d(boxes_a: torch.Tensor, boxes_b: torch.Tensor, overlap_only: bool = False) -> torch.Tensor:
    """[N]: the 3-D IoU (or, with `overlap_only`, the BEV overlap area) of row i of `boxes_a` with row i of `boxes_b`: the
    bits of entry [i, i] of the pairwise form."""
    N = _boxes(boxes_a, "boxes_a", "boxes_aligned_iou3d")
    if _boxes(boxes_b, "boxes_b", "boxes_aligned_iou3d") != N:
        raise ValueError("boxes_aligned_iou3d: the boxes are paired, their row counts differ")
    out = torch.empty((N,), device=boxes_a.device, dtype=_F32)
    if N:
        check(lib().lc_boxes_iou_aligned_fwd(boxes_a.data_ptr(), boxes_b.data_ptr(), N, _OVERLAP if overlap_only else _IOU_3D,
                                             out.data_ptr(), _stream()), "lc_boxes_iou_aligned_fwd")
    return out


def _nms_count(boxes: torch.Tensor, who: str) -> int:
    N = _boxes(boxes, "boxes", who)
    if N > NMS_MAX_BOXES:
        raise ValueError(f"{who}: {N} boxes, the NMS kernels take {NMS_MAX_BOXES} at the most (the mask of more would "
                         "pass 512 MiB); cut the candidates first (nms_gpu's pre_maxsize)")
    return N


def _mask(boxes: torch.Tensor, thresh: float, normal: bool, N: int, zero: bool) -> torch.Tensor:
    words = (N + WORD - 1) // WORD
    mask = (torch.zeros if zero else torch.empty)((N, words), device=boxes.device, dtype=torch.int64)
    if N:
        check(lib().lc_nms_mask_fwd(boxes.data_ptr(), N, float(thresh), int(bool(normal)), mask.data_ptr(), _stream()),
              "lc_nms_mask_fwd")
    return mask


@_entry
def nms_mask(boxes: torch.Tensor, thresh: float, normal: bool = False) -> torch.Tensor:
    """int64 [N, ceil(N/64)] (64-bit words): bit c of word [r, w] is set iff iou(r, 64 w + c) > thresh and 64 w + c > r,
    with the BEV IoU, or with `normal` the IoU of the unrotated extents.  The words left of the diagonal are zero."""
    return _mask(boxes, thresh, normal, _nms_count(boxes, "nms_mask"), zero=True)


def _select(mask: torch.Tensor, N: int) -> torch.Tensor:
    keep = torch.empty((N,), device=mask.device, dtype=torch.int64)
    if N == 0:
        return keep
    count = torch.empty((1,), device=mask.device, dtype=torch.int32)
    check(lib().lc_nms_select_fwd(mask.data_ptr(), N, keep.data_ptr(), count.data_ptr(), _stream()), "lc_nms_select_fwd")
    return keep[:int(count.item())]            # 4 bytes back: the result's length depends on the data


def nms_select(mask: torch.Tensor) -> torch.Tensor:
    """int64 [K], ascending: the greedy walk over an `nms_mask` -- box i is kept unless an earlier kept box has its bit
    set -- on the device; only the words at or right of the diagonal are read."""
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise RuntimeError("lidarcrafter_amd.ops: `mask` must be a CUDA(HIP) tensor -- the hot path has no CPU fallback")
    if mask.dtype != torch.int64 or mask.dim() != 2 or not mask.is_contiguous() or \
            mask.shape[1] != (mask.shape[0] + WORD - 1) // WORD:
        raise ValueError(f"nms_select: `mask` must be contiguous int64 [N, ceil(N/64)], got {mask.dtype} {tuple(mask.shape)}")
    if mask.shape[0] > NMS_MAX_BOXES:
        raise ValueError(f"nms_select: {mask.shape[0]} boxes, the NMS kernels take {NMS_MAX_BOXES} at the most")
    with torch.cuda.device(mask.device):
        return _select(mask, mask.shape[0])


@_entry
def nms(boxes: torch.Tensor, thresh: float, normal: bool = False) -> torch.Tensor:
    """int64 [K], ascending: the indices the greedy NMS keeps among `boxes` taken in their order (sort by score first)."""
    N = _nms_count(boxes, "nms")
    return _select(_mask(boxes, thresh, normal, N, zero=False), N)


def boxes_iou_bev_host(boxes_a: np.ndarray, boxes_b: np.ndarray) -> np.ndarray:
    """float32 [N,M] on the CPU (no GPU touched): the BEV IoU of every pair through the same geometry header as the
    kernels.  `boxes_a`, `boxes_b`: C-contiguous float32 [N,7], [M,7] numpy arrays."""
    for t in (boxes_a, boxes_b):
        if not isinstance(t, np.ndarray) or t.dtype != np.float32 or t.ndim != 2 or t.shape[1] != 7 or \
                not t.flags.c_contiguous:
            raise ValueError("boxes_iou_bev_host: the boxes must be C-contiguous float32 [N,7] numpy arrays")
    out = np.zeros((boxes_a.shape[0], boxes_b.shape[0]), np.float32)
    if out.size:
        check(lib().lc_boxes_iou_bev_host(boxes_a.ctypes.data, boxes_a.shape[0], boxes_b.ctypes.data, boxes_b.shape[0],
                                          out.ctypes.data), "lc_boxes_iou_bev_host")
    return out
