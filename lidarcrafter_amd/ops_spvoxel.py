"""Tensor-level wrapper over the point <-> voxel exchanges of csrc/spvoxel.hip (include/lidarcrafter_hip.h: lc_spvox_*).
Like ops_spconv.py: CUDA(HIP) tensors only, no CPU / eager-PyTorch fallback; shapes and dtypes are checked here, before
any launch; limits come back from the C entry as LC_EUNSUP.

Points are float32 rows (x, y, z, batch) in voxel units.  `query` finds the eight voxels around every point in a level's
coordinate hash (ops_spconv.hash_build) and their trilinear weights, `devoxelize` interpolates voxel rows at the points,
`voxelize` takes the mean of the points of every voxel, added in ascending point order (`voxel_order` puts the points in
that order: a stable sort and a prefix sum, plumbing)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream
from .ops_spconv import _I32, _rows

WIDTHS_DEVOX = (16, 48, 64, 128)
WIDTHS_VOX = (4, 16, 64, 128)


def _req_i32(t: torch.Tensor, name: str, shape_ok) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"lidarcrafter_amd.ops_spvoxel: `{name}` must be a CUDA(HIP) tensor -- no CPU fallback on the "
                           "hot path")
    if t.dtype != _I32 or not t.is_contiguous() or not shape_ok(t):
        raise ValueError(f"`{name}`: contiguous int32 of another shape expected, got {t.dtype} {tuple(t.shape)}")


@_entry
def query(points: torch.Tensor, stride: int, table: torch.Tensor, n_table: int,
          weights: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(idx [N, 8] int32, w [N, 8] float32 or None): for every point (x, y, z, batch) the rows of `table` (hash_build of
    `n_table` coordinates at `stride`) at floor(p / stride) * stride + {0, stride}^3, z fastest, -1 when absent, and the
    normalised trilinear weights (zeros where absent).  `weights=False`: idx only (voxelize needs idx[:, 0])."""
    _req(points, "points")
    if points.dim() != 2 or points.shape[1] != 4 or not points.is_contiguous() or points.shape[0] < 1:
        raise ValueError(f"query: `points` must be contiguous float32 [N >= 1, 4] = (x, y, z, batch), got "
                         f"{tuple(points.shape)}")
    if not table.is_cuda or table.dtype != torch.int64 or table.numel() * 8 < int(lib().lc_spconv_hash_bytes(n_table)):
        raise ValueError("query: `table` is not the hash_build of `n_table` rows")
    n = points.shape[0]
    idx = torch.empty((n, 8), device=points.device, dtype=_I32)
    w = torch.empty((n, 8), device=points.device, dtype=_F32) if weights else None
    check(lib().lc_spvox_query(points.data_ptr(), n, int(stride), table.data_ptr(), int(n_table), idx.data_ptr(),
                               None if w is None else w.data_ptr(), _stream()), "lc_spvox_query")
    return idx, w


@_entry
def devoxelize(feats: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, addend: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = sum_k w[i, k] feats[idx[i, k]] + addend[i].  feats [n_rows, C] rows (a column slice of a wider buffer is
    fine), idx / w [N, 8] of `query`, addend [N, C] rows or None, out [N, C] rows (may be `addend` itself).  An entry of
    idx that is -1 or outside [0, n_rows) reads nothing."""
    ldf = _rows(feats, "feats", "devoxelize")
    C = feats.shape[1]
    _req_i32(idx, "idx", lambda t: t.dim() == 2 and t.shape[1] == 8 and t.shape[0] >= 1)
    _req(w, "w")
    N = idx.shape[0]
    if tuple(w.shape) != (N, 8) or not w.is_contiguous():
        raise ValueError(f"devoxelize: `w` must be contiguous [{N}, 8], got {tuple(w.shape)}")
    lda = 0
    if addend is not None:
        lda = _rows(addend, "addend", "devoxelize")
        if tuple(addend.shape) != (N, C):
            raise ValueError(f"devoxelize: `addend` must be [{N}, {C}], got {tuple(addend.shape)}")
    if out is None:
        out = torch.empty((N, C), device=feats.device, dtype=_F32)
    ldo = _rows(out, "out", "devoxelize")
    if tuple(out.shape) != (N, C):
        raise ValueError(f"devoxelize: `out` must be [{N}, {C}], got {tuple(out.shape)}")
    check(lib().lc_spvox_devoxelize(feats.data_ptr(), ldf, feats.shape[0], idx.data_ptr(), w.data_ptr(),
                                    None if addend is None else addend.data_ptr(), lda, out.data_ptr(), ldo, N, C,
                                    _stream()), "lc_spvox_devoxelize")
    return out


def voxel_order(idx0: torch.Tensor, n_voxels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(perm int32 [N], offsets int32 [n_voxels + 1]) of the points' voxel rows `idx0` [N] (-1: in no voxel): perm is the
    stable ascending order of idx0, so a voxel's points keep their own order; perm[offsets[v] : offsets[v + 1]] are the
    points of voxel v (the points in no voxel come first and belong to none).  Plumbing in torch."""
    _req_i32(idx0, "idx0", lambda t: t.dim() == 1 and t.shape[0] >= 1)
    perm = torch.sort(idx0, stable=True).indices.to(_I32)
    counts = torch.bincount(idx0.long() + 1, minlength=int(n_voxels) + 1)
    if counts.numel() != int(n_voxels) + 1:
        raise ValueError(f"voxel_order: an entry of `idx0` is not below {n_voxels}")
    return perm, torch.cumsum(counts, 0).to(_I32)


@_entry
def voxelize(feats: torch.Tensor, perm: torch.Tensor, offsets: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[v] = the mean of feats[perm[offsets[v] : offsets[v + 1]]], each row divided by their number and then added, in
    that order; zeros for a voxel without points.  feats [N, C] rows, (perm, offsets) of `voxel_order`, out [V, C] rows."""
    ldf = _rows(feats, "feats", "voxelize")
    C = feats.shape[1]
    _req_i32(perm, "perm", lambda t: t.dim() == 1 and t.shape[0] >= 1)
    _req_i32(offsets, "offsets", lambda t: t.dim() == 1 and t.shape[0] >= 2)
    V = offsets.shape[0] - 1
    if out is None:
        out = torch.empty((V, C), device=feats.device, dtype=_F32)
    ldo = _rows(out, "out", "voxelize")
    if tuple(out.shape) != (V, C):
        raise ValueError(f"voxelize: `out` must be [{V}, {C}], got {tuple(out.shape)}")
    check(lib().lc_spvox_voxelize(feats.data_ptr(), ldf, feats.shape[0], perm.data_ptr(), perm.shape[0], offsets.data_ptr(),
                                  V, out.data_ptr(), ldo, C, _stream()), "lc_spvox_voxelize")
    return out
