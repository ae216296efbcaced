"""Tensor-level wrappers over the GLENet / rotated-IoU kernels of csrc/glenet.hip (include/lidarcrafter_hip.h:
lc_segment_center_fwd, lc_glenet_trunk_fwd, lc_rbox_inter_fwd, lc_riou3d_paired_fwd, lc_glenet_score_fwd; DESIGN.md section
5q).  Like ops.py: CUDA(HIP) float32 / int32 tensors only, no CPU / eager-PyTorch fallback."""
from __future__ import annotations

import math
from typing import Optional

import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream
from .ops_pointmlp import _req_i32

ANCHOR = (3.9, 1.6, 1.56)                                  # the reference's nuScenes point_anchor_size (dxa, dya, dza)
DIAGONAL = math.sqrt(ANCHOR[0] ** 2 + ANCHOR[1] ** 2)      # a float64 in the reference too
TRUNK_WIDTHS = (3, 64, 128, 512)
SIDE_WIDTH = 8
TILE = 128                                                 # points per tile of the trunk kernel (csrc/glenet.hip GL_T)


def _ragged(points: torch.Tensor, offsets: torch.Tensor, who: str):
    _req(points, "points")
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1 or not points.is_contiguous():
        raise ValueError(f"{who}: `points` must be contiguous non-empty [total,3], got {tuple(points.shape)}")
    if not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError(f"{who}: `offsets` must be int32 [B+1]")
    _req_i32(offsets, "offsets", (offsets.numel(),))
    return points.shape[0], offsets.numel() - 1


@_entry
def segment_center(points: torch.Tensor, offsets: torch.Tensor, scales=(DIAGONAL, DIAGONAL, ANCHOR[2])):
    """(out [total,3], mean [B,3]): per object of the ragged batch (`points` [total,3], `offsets` int32 [B+1]) the mean of
    its points -- a float64 sum in a fixed order, rounded once -- and out = float32((p - mean) / scales), the float32
    difference divided in float64 by the float64 `scales`."""
    total, B = _ragged(points, offsets, "segment_center")
    sx, sy, sz = (float(v) for v in scales)
    out = torch.empty_like(points)
    mean = torch.empty((B, 3), device=points.device, dtype=_F32)
    check(lib().lc_segment_center_fwd(points.data_ptr(), offsets.data_ptr(), B, total, sx, sy, sz, out.data_ptr(),
                                      mean.data_ptr(), _stream()), "lc_segment_center_fwd")
    return out, mean


@_entry
def glenet_trunk(norm: torch.Tensor, offsets: torch.Tensor, choice: torch.Tensor, main, side,
                 out: Optional[tuple] = None):
    """(featA [512,R], featS [8,R]), channel-major, R = D B: row r = d B + b gathers its K points as norm[offsets[b] +
    choice[d,b,:]] and runs PointNetfeat's 3 -> 64 -> 128 -> 512 + max and SimPointNetfeat's 3 -> 8 -> 8 -> 8 + max over
    them.  `choice` int32 [D,B,K]; `main` = (w1, b1, w2, b2, w3, b3), `side` likewise, BatchNorm folded in."""
    total, B = _ragged(norm, offsets, "glenet_trunk")
    if not isinstance(choice, torch.Tensor) or choice.dim() != 3 or choice.shape[1] != B or choice.numel() == 0:
        raise ValueError(f"glenet_trunk: `choice` must be int32 [D,{B},K], got {tuple(getattr(choice, 'shape', ()))}")
    D, _, K = choice.shape
    _req_i32(choice, "choice", (D, B, K))
    R = D * B
    cm, cs = TRUNK_WIDTHS, SIDE_WIDTH
    shapes = ((cm[1], 3), (cm[1],), (cm[2], cm[1]), (cm[2],), (cm[3], cm[2]), (cm[3],))
    sshapes = ((cs, 3), (cs,), (cs, cs), (cs,), (cs, cs), (cs,))
    for group, want, tag in ((main, shapes, "main"), (side, sshapes, "side")):
        if len(group) != 6:
            raise ValueError(f"glenet_trunk: `{tag}` must be (w1, b1, w2, b2, w3, b3)")
        for t, shape in zip(group, want):
            _req(t, tag)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"glenet_trunk: a `{tag}` tensor must be contiguous {shape}, got {tuple(t.shape)}")
    if out is None:
        out = (torch.empty((cm[3], R), device=norm.device, dtype=_F32), torch.empty((cs, R), device=norm.device, dtype=_F32))
    featA, featS = out
    for t, shape in ((featA, (cm[3], R)), (featS, (cs, R))):
        _req(t, "out")
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"glenet_trunk: `out` must be contiguous {shape}, got {tuple(t.shape)}")
    check(lib().lc_glenet_trunk_fwd(norm.data_ptr(), total, offsets.data_ptr(), choice.data_ptr(), B, K, R,
                                    *[t.data_ptr() for t in main], *[t.data_ptr() for t in side], featA.data_ptr(),
                                    featS.data_ptr(), _stream()), "lc_glenet_trunk_fwd")
    return featA, featS


def _req_rows(t: torch.Tensor, name: str, cols: int, who: str, at_least: bool = False) -> int:
    _req(t, name)
    if t.dim() != 2 or t.shape[0] < 1 or not t.is_contiguous() or (t.shape[1] < cols if at_least else t.shape[1] != cols):
        raise ValueError(f"{who}: `{name}` must be contiguous non-empty [N,{'>=' if at_least else ''}{cols}], "
                         f"got {tuple(t.shape)}")
    return t.shape[0]


@_entry
def rbox_intersection(corners_g: torch.Tensor, corners_q: torch.Tensor):
    """(pts [N,16], cnt int32 [N], area [N]) of the reference's compute_vertex / sort_vertex / area_polygon on the paired
    corner sets [N,8]: `pts` are compute_vertex's vertices in its order (zeros past `cnt`)."""
    N = _req_rows(corners_g, "corners_g", 8, "rbox_intersection")
    if _req_rows(corners_q, "corners_q", 8, "rbox_intersection") != N:
        raise ValueError("rbox_intersection: the corner sets are paired, their row counts differ")
    dev = corners_g.device
    pts = torch.empty((N, 16), device=dev, dtype=_F32)
    cnt = torch.empty((N,), device=dev, dtype=torch.int32)
    area = torch.empty((N,), device=dev, dtype=_F32)
    check(lib().lc_rbox_inter_fwd(corners_g.data_ptr(), corners_q.data_ptr(), N, pts.data_ptr(), cnt.data_ptr(),
                                  area.data_ptr(), _stream()), "lc_rbox_inter_fwd")
    return pts, cnt, area


@_entry
def riou3d_paired(g: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """[N]: the reference's iou3d of the paired boxes g[i], q[i] = (x, y, z, dx, dy, dz, ry, ...), float32 [N, >= 7]."""
    N = _req_rows(g, "g", 7, "riou3d_paired", at_least=True)
    if _req_rows(q, "q", 7, "riou3d_paired", at_least=True) != N:
        raise ValueError("riou3d_paired: the boxes are paired, their row counts differ")
    iou = torch.empty((N,), device=g.device, dtype=_F32)
    check(lib().lc_riou3d_paired_fwd(g.data_ptr(), g.shape[1], q.data_ptr(), q.shape[1], N, iou.data_ptr(), _stream()),
          "lc_riou3d_paired_fwd")
    return iou


@_entry
def glenet_score(box: torch.Tensor, gt: torch.Tensor, anchor=ANCHOR):
    """(pred [D,B,9], overlap [D,B], variance float64 [B,7], mean_overlap float64 [B]) from the sampler's `box` [D,B,9] and
    the normalised `gt` [B,7]: the decoded draws, their IoU with the decoded gt, and per object the population variance of
    the seven box columns (the heading as the sine of its offset from the gt heading) and the mean IoU over the draws."""
    _req(box, "box")
    _req(gt, "gt")
    if box.dim() != 3 or box.shape[2] != 9 or box.numel() == 0 or not box.is_contiguous():
        raise ValueError(f"glenet_score: `box` must be contiguous non-empty [D,B,9], got {tuple(box.shape)}")
    D, B, _ = box.shape
    if tuple(gt.shape) != (B, 7) or not gt.is_contiguous():
        raise ValueError(f"glenet_score: `gt` must be contiguous [{B},7], got {tuple(gt.shape)}")
    dxa, dya, dza = (float(v) for v in anchor)
    dev = box.device
    pred = torch.empty_like(box)
    overlap = torch.empty((D, B), device=dev, dtype=_F32)
    variance = torch.empty((B, 7), device=dev, dtype=torch.float64)
    mean_overlap = torch.empty((B,), device=dev, dtype=torch.float64)
    check(lib().lc_glenet_score_fwd(box.data_ptr(), gt.data_ptr(), D, B, math.sqrt(dxa ** 2 + dya ** 2), dxa, dya, dza,
                                    pred.data_ptr(), overlap.data_ptr(), variance.data_ptr(), mean_overlap.data_ptr(),
                                    _stream()), "lc_glenet_score_fwd")
    return pred, overlap, variance, mean_overlap
