"""Tensor-level wrapper over the fused PointNet trunk of csrc/pointnet.hip (include/lidarcrafter_hip.h:
lc_pointnet_trunk_*).  Like ops.py: CUDA(HIP) float32 tensors only, no CPU / eager-PyTorch fallback."""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream

TILE = 128        # points per block of the trunk kernel (csrc/pointnet.hip PN_T; tests/test_pointnet_host.py compares)
WIDTHS = (3, 64, 128, 1024)


def trunk_scratch_elems(B: int, N: int) -> int:
    return int(lib().lc_pointnet_trunk_scratch_elems(B, N))


@_entry
def pointnet_trunk(x: torch.Tensor, trans: Optional[torch.Tensor], w1, b1, w2, b2, w3, b3, relu3: bool,
                   out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, :1024] = [relu](max over the points of W3 relu(W2 relu(W1 p' + b1) + b2) + b3), p' = p^T trans[b] (p without
    `trans`).  x [B,3,N] with a contiguous [3,N] block per cloud; trans [B,3,3] contiguous; the weights [64,3], [128,64],
    [1024,128] and biases contiguous, BatchNorm already folded in; `out` [B, >= 1024] row-major (columns 0:1024 are
    written); `scratch` >= trunk_scratch_elems(B, N) floats."""
    _req(x, "x")
    if x.dim() != 3 or x.shape[1] != 3:
        raise ValueError(f"pointnet_trunk: `x` must be [B,3,N], got {tuple(x.shape)}")
    B, _, N = x.shape
    if B < 1 or N < 1:
        raise ValueError("pointnet_trunk: empty batch or empty clouds")
    if (N > 1 and x.stride(2) != 1) or x.stride(1) != N:
        raise ValueError(f"pointnet_trunk: the [3,N] block of a cloud must be contiguous, strides={x.stride()}")
    x_bs = x.stride(0) if B > 1 else 3 * N
    for t, n, shape in ((w1, "w1", (64, 3)), (b1, "b1", (64,)), (w2, "w2", (128, 64)), (b2, "b2", (128,)),
                        (w3, "w3", (1024, 128)), (b3, "b3", (1024,))):
        _req(t, n)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"pointnet_trunk: `{n}` must be contiguous {shape}, got {tuple(t.shape)}")
    if trans is not None:
        _req(trans, "trans")
        if tuple(trans.shape) != (B, 3, 3) or not trans.is_contiguous():
            raise ValueError(f"pointnet_trunk: `trans` must be contiguous [{B},3,3], got {tuple(trans.shape)}")
    if out is None:
        out = torch.empty((B, 1024), device=x.device, dtype=_F32)
    _req(out, "out")
    if out.dim() != 2 or out.shape[0] != B or out.shape[1] < 1024 or out.stride(1) != 1:
        raise ValueError(f"pointnet_trunk: `out` must be row-major [{B}, >= 1024], got {tuple(out.shape)}")
    y_bs = out.stride(0) if B > 1 else out.shape[1]
    need = trunk_scratch_elems(B, N)
    if scratch is None:
        scratch = torch.empty(need, device=x.device, dtype=_F32)
    _req(scratch, "scratch")
    if scratch.numel() < need or not scratch.is_contiguous():
        raise ValueError("pointnet_trunk: workspace too small")
    check(lib().lc_pointnet_trunk_fwd(x.data_ptr(), x_bs, None if trans is None else trans.data_ptr(), w1.data_ptr(),
                                      b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(),
                                      1 if relu3 else 0, out.data_ptr(), y_bs, B, N, scratch.data_ptr(), _stream()),
          "lc_pointnet_trunk_fwd")
    return out
