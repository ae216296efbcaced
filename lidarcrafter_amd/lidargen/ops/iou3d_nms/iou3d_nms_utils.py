"""Rotated 3-D IoU and NMS -- API mirror of the reference's lidargen/ops/iou3d_nms/iou3d_nms_utils.py on the HIP kernels
of csrc/iou3d_nms.hip (lidarcrafter_amd.ops_iou3d): the same seven functions, signatures, asserts
and return types.  Differences, all on the side of doing less on the host: the 3-D IoU's height / volume epilogue runs inside
the overlap kernel (same float32 expressions, same order, same bits as the torch lines over the kernel's overlap), the
NMS walk runs on the device and only the kept count comes back, and an empty input returns an empty index tensor where the
reference would launch a zero-sized grid.  `boxes_bev_iou_cpu` alone runs on the CPU, as in the reference."""
from __future__ import annotations

import numpy as np
import torch

from lidarcrafter_amd import ops_iou3d as K


def boxes_bev_iou_cpu(boxes_a, boxes_b):
    """boxes_a (N,7), boxes_b (M,7) [x, y, z, dx, dy, dz, heading] -> (N,M) BEV IoU on the CPU.  numpy arrays are taken as
    float32; the result is a numpy array when `boxes_b` was one (the reference's rule), else a CPU tensor."""
    as_numpy = isinstance(boxes_b, np.ndarray)
    boxes_a, boxes_b = (torch.from_numpy(t).float() if isinstance(t, np.ndarray) else t for t in (boxes_a, boxes_b))
    assert not (boxes_a.is_cuda or boxes_b.is_cuda), 'Only support CPU tensors'
    assert boxes_a.shape[1] == 7 and boxes_b.shape[1] == 7
    if boxes_a.dtype != torch.float32 or boxes_b.dtype != torch.float32:
        raise TypeError("boxes_bev_iou_cpu: float32 boxes (the reference's extension reads float data)")
    iou = K.boxes_iou_bev_host(boxes_a.detach().contiguous().numpy(), boxes_b.detach().contiguous().numpy())
    return iou if as_numpy else torch.from_numpy(iou)


def boxes_iou_bev(boxes_a, boxes_b):
    """boxes_a (N,7), boxes_b (M,7) -> (N,M) BEV IoU."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return K.boxes_iou_bev(boxes_a.contiguous(), boxes_b.contiguous())


def boxes_iou3d_gpu(boxes_a, boxes_b):
    """boxes_a (N,7), boxes_b (M,7) -> (N,M) 3-D IoU."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return K.boxes_iou3d(boxes_a.contiguous(), boxes_b.contiguous())


def boxes_aligned_iou3d_gpu(boxes_a, boxes_b):
    """boxes_a (N,7), boxes_b (N,7) -> (N,1) 3-D IoU of row i with row i."""
    assert boxes_a.shape[0] == boxes_b.shape[0]
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return K.boxes_aligned_iou3d(boxes_a.contiguous(), boxes_b.contiguous()).view(-1, 1)


def _nms(boxes, scores, thresh, pre_maxsize, normal):
    assert boxes.shape[1] == 7
    _, ranked = scores.sort(0, descending=True)         # the caller's indices, best score first
    if pre_maxsize is not None:
        ranked = ranked[:pre_maxsize]
    survivors = K.nms(boxes[ranked].contiguous(), thresh, normal=normal)      # positions in `ranked`, ascending
    return ranked[survivors].contiguous(), None


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """boxes (N,7), scores (N) -> (indices into the caller's arrays in descending score order, None): rotated NMS."""
    return _nms(boxes, scores, thresh, pre_maxsize, False)


def nms_normal_gpu(boxes, scores, thresh, **kwargs):
    """As nms_gpu on the unrotated extents (the heading is not read)."""
    return _nms(boxes, scores, thresh, None, True)


def paired_boxes_iou3d_gpu(boxes_a, boxes_b):
    """boxes_a (N,7), boxes_b (N,7) -> (N,) 3-D IoU of row i with row i."""
    assert boxes_a.shape[0] == boxes_b.shape[0]
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return K.boxes_aligned_iou3d(boxes_a.contiguous(), boxes_b.contiguous()).view(-1)
