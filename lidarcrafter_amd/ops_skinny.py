"""Tensor-level wrappers over the skinny dense-layer family of csrc/layout_gen.hip (include/lidarcrafter_hip.h:
lc_skinny_*, lc_rowprep_fwd, lc_graph_pool_fwd, lc_time_embed_fwd).  Like ops.py: CUDA(HIP) float32 tensors only, no
CPU / eager-PyTorch fallback.

A *segment* is `(tensor [R, >= c0 + width], c0, width, idx | None)`: `width` columns of a row-major matrix starting at
column c0, row m of the operand being row idx[m] of the tensor (row m without idx).  `idx` is an int32 CUDA tensor whose
values the CALLER has checked against R (the kernels do not)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from ._lib import RowSegment, check, lib
from .ops import _F32, _req, _stream

ACT = {None: 0, "none": 0, "relu": 1, "geglu": 2}


def _rows(t: torch.Tensor, name: str) -> None:
    _req(t, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"`{name}` must be a row-major 2-D tensor, got shape {tuple(t.shape)} strides {t.stride()}")


def _idx(t: Optional[torch.Tensor], name: str, M: int) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != M:
        raise ValueError(f"`{name}` must be a contiguous int32 CUDA tensor of {M} rows")
    return t.data_ptr()


def segments(segs: Sequence, M: int):
    """-> (ctypes array of lc_row_segment, K).  Keeps nothing alive: the caller holds the tensors."""
    if not 1 <= len(segs) <= 3:
        raise ValueError("an operand has one to three row segments")
    arr = (RowSegment * len(segs))()
    K = 0
    for j, (t, c0, w, idx) in enumerate(segs):
        _rows(t, f"segment {j}")
        if c0 < 0 or w < 1 or c0 + w > t.shape[1]:
            raise ValueError(f"segment {j}: columns [{c0}, {c0 + w}) outside a tensor of {t.shape[1]} columns")
        if idx is None and t.shape[0] < M:
            raise ValueError(f"segment {j}: {t.shape[0]} rows for an operand of {M}")
        arr[j].p = t.data_ptr() + 4 * c0
        arr[j].idx = _idx(idx, f"segment {j} idx", M)
        arr[j].ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
        arr[j].width = w
        K += w
    return arr, K


def skinny_parts(M: int, N: int, K: int) -> int:
    return int(lib().lc_skinny_parts(M, N, K))


def skinny_linear(segs: Sequence, M: int, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
                  vec=None, res=None, out: Optional[torch.Tensor] = None, parts: Optional[torch.Tensor] = None,
                  nparts: Optional[int] = None) -> torch.Tensor:
    """out[M, N'] = act(X . w^T + bias) + vec_tensor[vec_idx[m], c0:c0+N'] + res_tensor[m, c0:c0+N'] with X the gathered
    concatenation of `segs`; w [N, K] contiguous (nn.Linear layout); act None | 'relu' | 'geglu' (N' = N / 2);
    vec = (tensor, c0, idx | None), res = (tensor, c0); `parts`: workspace of >= nparts * M * N floats."""
    arr, K = segments(segs, M)
    _req(w, "w")
    if w.dim() != 2 or not w.is_contiguous() or w.shape[1] != K:
        raise ValueError(f"skinny_linear: w must be contiguous [N, {K}], got {tuple(w.shape)}")
    N = w.shape[0]
    a = ACT[act]
    No = N // 2 if a == 2 else N
    if nparts is None:
        nparts = skinny_parts(M, N, K)
    if parts is None:
        parts = torch.empty(nparts * M * N, device=w.device, dtype=_F32)
    _req(parts, "parts")
    if parts.numel() < nparts * M * N or not parts.is_contiguous():
        raise ValueError("skinny_linear: workspace too small")
    if out is None:
        out = torch.empty((M, No), device=w.device, dtype=_F32)
    _rows(out, "out")
    if out.shape[0] < M or out.shape[1] < No:
        raise ValueError("skinny_linear: out too small")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError("skinny_linear: bias must be contiguous [N]")
    vp = vix = rp = None
    vld = rld = 0
    if vec is not None:
        vt, vc0, vidx = vec
        _rows(vt, "vec")
        if vc0 < 0 or vc0 + No > vt.shape[1]:
            raise ValueError("skinny_linear: vec columns out of range")
        vp, vld, vix = vt.data_ptr() + 4 * vc0, vt.stride(0), _idx(vidx, "vec idx", M)
    if res is not None:
        rt, rc0 = res
        _rows(rt, "res")
        if rc0 < 0 or rc0 + No > rt.shape[1] or rt.shape[0] < M:
            raise ValueError("skinny_linear: res out of range")
        rp, rld = rt.data_ptr() + 4 * rc0, rt.stride(0)
    s = _stream()
    L = lib()
    check(L.lc_skinny_gemm_fwd(arr, len(segs), w.data_ptr(), parts.data_ptr(), M, N, K, nparts, s), "lc_skinny_gemm_fwd")
    check(L.lc_skinny_combine_fwd(parts.data_ptr(), nparts, None if bias is None else bias.data_ptr(), a, vp, vld,
                                  vix, rp, rld, out.data_ptr(), out.stride(0), M, N, s), "lc_skinny_combine_fwd")
    return out


def rowprep(segs: Sequence, M: int, groups: int = 0, eps: float = 1e-5, gamma=None, beta=None, silu: bool = False,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row GroupNorm over `groups` groups (1: LayerNorm; 0: none) [+ SiLU] of the gathered concatenation of `segs`."""
    arr, Cn = segments(segs, M)
    if beta is not None and gamma is None:
        raise ValueError("rowprep: beta without gamma (the kernel applies beta only next to gamma)")
    dev = segs[0][0].device
    if out is None:
        out = torch.empty((M, Cn), device=dev, dtype=_F32)
    _rows(out, "out")
    if out.shape[0] < M or out.shape[1] < Cn:
        raise ValueError("rowprep: out too small")
    for t, n in ((gamma, "gamma"), (beta, "beta")):
        if t is not None:
            _req(t, n)
            if t.numel() != Cn or not t.is_contiguous():
                raise ValueError(f"rowprep: {n} must be contiguous [{Cn}]")
    check(lib().lc_rowprep_fwd(arr, len(segs), out.data_ptr(), out.stride(0), M, Cn, groups, float(eps),
                               None if gamma is None else gamma.data_ptr(), None if beta is None else beta.data_ptr(),
                               1 if silu else 0, _stream()), "lc_rowprep_fwd")
    return out


def graph_pool(t: torch.Tensor, s_col: int, o_col: int, H: int, row_ptr: torch.Tensor, slots: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Scatter-mean of triple rows onto object rows through the CSR of graph.edge_csr (count clamped at 1).  The caller
    has checked that every slot names a row of `t`."""
    _rows(t, "t")
    O = row_ptr.numel() - 1
    for x, n in ((row_ptr, "row_ptr"), (slots, "slots")):
        if not x.is_cuda or x.dtype != torch.int32 or not x.is_contiguous():
            raise ValueError(f"graph_pool: `{n}` must be a contiguous int32 CUDA tensor")
    if slots.numel() > 2 * t.shape[0]:
        raise ValueError("graph_pool: more slots than two per triple row")
    if out is None:
        out = torch.empty((O, H), device=t.device, dtype=_F32)
    _rows(out, "out")
    if out.shape[0] < O or out.shape[1] < H:
        raise ValueError("graph_pool: out too small")
    check(lib().lc_graph_pool_fwd(t.data_ptr(), t.stride(0), s_col, o_col, row_ptr.data_ptr(), slots.data_ptr(),
                                  out.data_ptr(), out.stride(0), O, H, _stream()), "lc_graph_pool_fwd")
    return out


def time_embed(t: torch.Tensor, freqs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(t, "t"), _req(freqs, "freqs")
    U, half = t.numel(), freqs.numel()
    if not t.is_contiguous() or not freqs.is_contiguous():
        raise ValueError("time_embed: contiguous operands")
    if out is None:
        out = torch.empty((U, 2 * half), device=t.device, dtype=_F32)
    _rows(out, "out")
    if not out.is_contiguous() or tuple(out.shape) != (U, 2 * half):
        raise ValueError("time_embed: out must be contiguous [U, 2 * half]")
    check(lib().lc_time_embed_fwd(t.data_ptr(), freqs.data_ptr(), out.data_ptr(), U, half, _stream()), "lc_time_embed_fwd")
    return out
