"""Tensor-level wrappers over the stacked pointnet2 kernels of csrc/pointnet2_stack.hip (include/lidarcrafter_hip.h:
lc_pn2_*, lc_fps_stack_fwd).  Like ops_pointmlp.py: CUDA(HIP) contiguous float32 / int32 tensors
only, no CPU / eager-PyTorch fallback.  A stacked tensor holds cloud b in rows start_b .. start_b + n_b - 1; the counts are
int32 device tensors [B]."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream

_I32 = torch.int32


def limit(which: str) -> int:
    """'max_nsample', 'max_batch', 'first_cols' (columns per block of the gathered first layer at Co <= 32)."""
    names = ("max_nsample", "max_batch", "first_cols")
    return int(lib().lc_pn2_limit(names.index(which)))


def _f(t: torch.Tensor, name: str, cols: Optional[int]) -> int:
    """`t` is a contiguous float32 device tensor [rows, cols]; returns rows."""
    _req(t, name)
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols) or not t.is_contiguous():
        raise ValueError(f"ops_pointnet2: `{name}` must be contiguous [rows, {cols if cols is not None else 'C'}], got "
                         f"{tuple(t.shape)} strides {t.stride()}")
    return t.shape[0]


def _i(t: torch.Tensor, name: str, shape=None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ops_pointnet2: `{name}` must be a CUDA(HIP) tensor -- the hot path has no CPU fallback")
    if t.dtype != _I32:
        raise TypeError(f"`{name}` must be int32, got {t.dtype}")
    if not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"`{name}` must be contiguous {shape}, got {tuple(t.shape)}")


def _counts(a: torch.Tensor, b: torch.Tensor, na: str, nb: str) -> int:
    _i(a, na)
    _i(b, nb)
    if a.dim() != 1 or b.dim() != 1 or a.shape[0] != b.shape[0] or a.shape[0] < 1:
        raise ValueError(f"ops_pointnet2: `{na}` and `{nb}` must be [B] with the same B >= 1, got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    return a.shape[0]


def _nsample(nsample: int, who: str) -> int:
    nsample = int(nsample)
    if nsample < 1:
        raise ValueError(f"{who}: nsample = {nsample}")
    if nsample > limit("max_nsample"):
        raise NotImplementedError(f"{who}: nsample = {nsample} is not built -- LC_PN2_MAX_NSAMPLE is {limit('max_nsample')}")
    return nsample


def _scratch(B: int, rows: int, dev) -> torch.Tensor:
    return torch.empty(int(lib().lc_pn2_scratch_elems(B, rows)), device=dev, dtype=_I32)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None or t.numel() == 0 else t.data_ptr()


@_entry
def ball_query(radius: float, nsample: int, xyz: torch.Tensor, xyz_batch_cnt: torch.Tensor, new_xyz: torch.Tensor,
               new_xyz_batch_cnt: torch.Tensor) -> torch.Tensor:
    """int32 [M, nsample]: the kernel's rows -- local indices, the row pre-filled with the first hit, [-1, 0, ...] for an
    empty ball."""
    N, M = _f(xyz, "xyz", 3), _f(new_xyz, "new_xyz", 3)
    B = _counts(xyz_batch_cnt, new_xyz_batch_cnt, "xyz_batch_cnt", "new_xyz_batch_cnt")
    nsample = _nsample(nsample, "ball_query")
    idx = torch.empty((M, nsample), device=xyz.device, dtype=_I32)
    check(lib().lc_pn2_ball_query_fwd(_ptr(xyz), xyz_batch_cnt.data_ptr(), _ptr(new_xyz), new_xyz_batch_cnt.data_ptr(),
                                      _ptr(idx), _scratch(B, M, xyz.device).data_ptr(), B, N, M, float(radius), nsample,
                                      _stream()), "lc_pn2_ball_query_fwd")
    return idx


@_entry
def group(features: torch.Tensor, features_batch_cnt: torch.Tensor, idx: torch.Tensor,
          idx_batch_cnt: torch.Tensor) -> torch.Tensor:
    """[M, C, nsample]: out[m, c, s] = features[start + idx[m, s], c]; 0 for an index outside its cloud."""
    N = _f(features, "features", None)
    C = features.shape[1]
    B = _counts(features_batch_cnt, idx_batch_cnt, "features_batch_cnt", "idx_batch_cnt")
    _i(idx, "idx")
    if idx.dim() != 2 or idx.shape[1] < 1 or C < 1:
        raise ValueError(f"group: `idx` must be [M, nsample >= 1] and C >= 1, got {tuple(idx.shape)}, C = {C}")
    M, ns = idx.shape
    out = torch.empty((M, C, ns), device=features.device, dtype=_F32)
    check(lib().lc_pn2_group_fwd(_ptr(features), features_batch_cnt.data_ptr(), _ptr(idx), idx_batch_cnt.data_ptr(), _ptr(out),
                                 _scratch(B, M, features.device).data_ptr(), B, N, C, M, ns, _stream()), "lc_pn2_group_fwd")
    return out


def _inverse(key: torch.Tensor, rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(order, seg) int32: the stable sort of `key` (values 0..rows, `rows` = reads nothing) and the first position of every
    row 0..rows in it."""
    skey, order = torch.sort(key.long(), stable=True)
    seg = torch.searchsorted(skey, torch.arange(rows + 1, device=key.device, dtype=torch.long))
    return order.to(_I32).contiguous(), seg.to(_I32).contiguous()


@_entry
def three_nn(unknown: torch.Tensor, unknown_batch_cnt: torch.Tensor, known: torch.Tensor,
             known_batch_cnt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dist2 float32 [N, 3], idx int32 [N, 3] global rows of `known`), ascending (distance, index); a slot never filled
    holds +inf and the cloud's start row."""
    N, M = _f(unknown, "unknown", 3), _f(known, "known", 3)
    B = _counts(unknown_batch_cnt, known_batch_cnt, "unknown_batch_cnt", "known_batch_cnt")
    dist2 = torch.empty((N, 3), device=unknown.device, dtype=_F32)
    idx = torch.empty((N, 3), device=unknown.device, dtype=_I32)
    check(lib().lc_pn2_three_nn_fwd(_ptr(unknown), unknown_batch_cnt.data_ptr(), _ptr(known), known_batch_cnt.data_ptr(),
                                    _ptr(dist2), _ptr(idx), _scratch(B, N, unknown.device).data_ptr(), B, N, M, _stream()),
          "lc_pn2_three_nn_fwd")
    return dist2, idx


def _interp_args(idx, weight, who):
    _i(idx, "idx")
    _req(weight, "weight")
    if idx.dim() != 2 or idx.shape[1] != 3 or tuple(weight.shape) != tuple(idx.shape) or not weight.is_contiguous():
        raise ValueError(f"{who}: `idx` and `weight` must be contiguous [N, 3], got {tuple(idx.shape)} and {tuple(weight.shape)}")
    return idx.shape[0]


@_entry
def three_interpolate(features: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """[N, C] = (w0 f0 + w1 f1) + w2 f2 over rows idx [N, 3] of `features` [M, C]; an index outside [0, M) adds 0."""
    M = _f(features, "features", None)
    C = features.shape[1]
    N = _interp_args(idx, weight, "three_interpolate")
    if C < 1:
        raise ValueError("three_interpolate: C = 0")
    out = torch.empty((N, C), device=features.device, dtype=_F32)
    check(lib().lc_pn2_three_interpolate_fwd(_ptr(features), _ptr(idx), _ptr(weight), _ptr(out), N, C, M, _stream()),
          "lc_pn2_three_interpolate_fwd")
    return out


@_entry
def three_interpolate_bwd(grad_out: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor, M: int) -> torch.Tensor:
    """[M, C]: every row the sum of grad_out[n, c] weight[n, j] over its entries in ascending (n, j) order."""
    N = _f(grad_out, "grad_out", None)
    C, M = grad_out.shape[1], int(M)
    if _interp_args(idx, weight, "three_interpolate_bwd") != N or C < 1:
        raise ValueError(f"three_interpolate_bwd: `grad_out` {tuple(grad_out.shape)} over `idx` {tuple(idx.shape)}")
    flat = idx.reshape(-1)
    key = torch.where((flat >= 0) & (flat < M), flat, torch.full_like(flat, M))
    order, seg = _inverse(key, M)
    grad = torch.empty((M, C), device=grad_out.device, dtype=_F32)
    check(lib().lc_pn2_three_interpolate_bwd(_ptr(grad_out), _ptr(order), seg.data_ptr(), _ptr(weight), _ptr(grad), N, C, M,
                                             _stream()), "lc_pn2_three_interpolate_bwd")
    return grad


@_entry
def voxel_query(max_range, radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor, new_coords: torch.Tensor,
                point_indices: torch.Tensor) -> torch.Tensor:
    """int32 [M, nsample]: global rows of `xyz`, the kernel's rows ([-1, 0, ...] when nothing is found)."""
    N, M = _f(xyz, "xyz", 3), _f(new_xyz, "new_xyz", 3)
    _i(new_coords, "new_coords", (M, 4))
    _i(point_indices, "point_indices")
    if point_indices.dim() != 4 or point_indices.numel() == 0:
        raise ValueError(f"voxel_query: `point_indices` must be non-empty [B, Z, Y, X], got {tuple(point_indices.shape)}")
    B, Z, Y, X = point_indices.shape
    zr, yr, xr = (int(v) for v in max_range)
    nsample = _nsample(nsample, "voxel_query")
    idx = torch.empty((M, nsample), device=xyz.device, dtype=_I32)
    check(lib().lc_pn2_voxel_query_fwd(_ptr(new_xyz), _ptr(xyz), _ptr(new_coords), point_indices.data_ptr(), _ptr(idx), M, N,
                                       B, Z, Y, X, nsample, float(radius), zr, yr, xr, _stream()), "lc_pn2_voxel_query_fwd")
    return idx


@_entry
def fps_stack(xyz: torch.Tensor, counts, npoints) -> torch.Tensor:
    """int32 [sum(npoints)]: the farthest-point sequence of every cloud (global rows) under the tie rule of a 1024-thread
    block.  `counts`, `npoints`: HOST lists."""
    N = _f(xyz, "xyz", 3)
    counts, npoints = [int(v) for v in counts], [int(v) for v in npoints]
    if len(counts) != len(npoints) or min(counts + [0]) < 0 or min(npoints + [0]) < 0 or sum(counts) != N:
        raise ValueError(f"fps_stack: counts {counts} / npoints {npoints} over {N} rows")
    from .ops_pointmlp import limit as pm_limit

    if max(counts + [0]) > pm_limit("fps_max_n"):
        raise NotImplementedError(f"stack_farthest_point_sample: a cloud of {max(counts)} points is not built -- "
                                  f"LC_FPS_MAX_N is {pm_limit('fps_max_n')}")
    out = torch.empty(sum(npoints), device=xyz.device, dtype=_I32)
    start = o = 0
    for n, m in zip(counts, npoints):
        if m and not n:
            raise ValueError("fps_stack: samples asked from an empty cloud")
        if m:
            check(lib().lc_fps_stack_fwd(xyz.data_ptr() + 12 * start, out.data_ptr() + 4 * o, n, m, start, _stream()),
                  "lc_fps_stack_fwd")
        start, o = start + n, o + m
    return out


@_entry
def sa_first(xyz: torch.Tensor, xyz_batch_cnt: torch.Tensor, new_xyz: torch.Tensor, new_xyz_batch_cnt: torch.Tensor,
             features: Optional[torch.Tensor], idx: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, Co: int,
             use_xyz: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[1, Co, M nsample] = relu(W G + bias) with G the grouped operand of QueryAndGroup over the ball query's rows `idx`
    (never written to memory); `wpk` the device copy of ops_pointmlp.pack_weight(W [Co, C + 3 use_xyz])."""
    from .ops_pointmlp import packed_weight_elems

    N, M = _f(xyz, "xyz", 3), _f(new_xyz, "new_xyz", 3)
    B = _counts(xyz_batch_cnt, new_xyz_batch_cnt, "xyz_batch_cnt", "new_xyz_batch_cnt")
    C = 0
    if features is not None:
        if _f(features, "features", None) != N:
            raise ValueError(f"sa_first: `features` has {features.shape[0]} rows, `xyz` {N}")
        C = features.shape[1]
    _i(idx, "idx")
    if idx.dim() != 2 or idx.shape[0] != M or idx.shape[1] < 1:
        raise ValueError(f"sa_first: `idx` must be [{M}, nsample], got {tuple(idx.shape)}")
    ns = _nsample(idx.shape[1], "sa_first")
    Ci, Co = C + (3 if use_xyz else 0), int(Co)
    if Ci < 1 or Co < 1:
        raise ValueError("sa_first: no input rows (features is None and use_xyz is off) or Co < 1")
    _req(wpk, "wpk")
    _req(bias, "bias")
    if wpk.numel() != packed_weight_elems(Ci, Co) or not wpk.is_contiguous():
        raise ValueError(f"sa_first: `wpk` has {wpk.numel()} elements, {Ci} -> {Co} packs to {packed_weight_elems(Ci, Co)}")
    if tuple(bias.shape) != (Co,) or not bias.is_contiguous():
        raise ValueError(f"sa_first: `bias` must be contiguous [{Co}]")
    shape = (1, Co, M * ns)
    if out is None:
        out = torch.empty(shape, device=xyz.device, dtype=_F32)
    _req(out, "out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"sa_first: `out` must be contiguous {shape}, got {tuple(out.shape)}")
    check(lib().lc_pn2_sa_first_fwd(_ptr(xyz), xyz_batch_cnt.data_ptr(), _ptr(new_xyz), new_xyz_batch_cnt.data_ptr(),
                                    _ptr(features), _ptr(idx), wpk.data_ptr(), bias.data_ptr(), _ptr(out),
                                    _scratch(B, M, xyz.device).data_ptr(), B, N, M, C, Co, ns, 1 if use_xyz else 0, _stream()),
          "lc_pn2_sa_first_fwd")
    return out


@_entry
def groupmax_into(x: torch.Tensor, K: int, out: torch.Tensor, col: int) -> torch.Tensor:
    """out[m, col + c] = the maximum over the K consecutive columns m K .. m K + K - 1 of `x` [1, C, M K]; `out` contiguous
    [M, W] with col + C <= W (lc_pointmlp_groupmax_fwd with the result's strides)."""
    _req(x, "x")
    _req(out, "out")
    K, col = int(K), int(col)
    if x.dim() != 3 or x.shape[0] != 1 or not x.is_contiguous() or x.numel() == 0 or K < 1 or x.shape[2] % K:
        raise ValueError(f"groupmax_into: `x` must be contiguous non-empty [1, C, M*{K}], got {tuple(x.shape)}")
    C, M = x.shape[1], x.shape[2] // K
    if out.dim() != 2 or out.shape[0] != M or not out.is_contiguous() or col < 0 or col + C > out.shape[1]:
        raise ValueError(f"groupmax_into: `out` must be contiguous [{M}, >= {col + C}], got {tuple(out.shape)}")
    check(lib().lc_pointmlp_groupmax_fwd(x.data_ptr(), out.data_ptr() + 4 * col, 1, C, M, K, 0, 1, out.shape[1], _stream()),
          "lc_pointmlp_groupmax_fwd")
    return out
