"""Earth Mover's Distance (auction approximation) -- mirror of the reference's
`lidargen/metrics/modules/emd/emd_module.py` (`emdFunction`, `emdModule` :46-95) and of `compute_pairwise_emd`
(`lidargen/metrics/metric_utils.py:447-458`), on the HIP kernels of csrc/emd.hip (ops.emd_forward).
`compute_pairwise_emd_batch` is this project's own: the pairs of a list that share a truncated length go through one launch."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.autograd import Function

from lidarcrafter_amd import ops as K

EPS, ITERS = 0.005, 50   # metric_utils.py:456


class emdFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters):
        assert xyz1.dim() == 3 and xyz2.dim() == 3, "expected [B, n, 3] clouds"
        assert xyz1.size(1) == xyz2.size(1), "the two clouds must have the same number of points"
        assert xyz1.size(0) == xyz2.size(0), "the two clouds must have the same batch size"
        xyz1 = xyz1.contiguous().float()
        xyz2 = xyz2.contiguous().float()
        dist, assignment = K.emd_forward(xyz1, xyz2, eps, iters)
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, gradidx):
        # emd_cuda.cu NmDistanceGradKernel: 2 g (xyz1 - xyz2[assignment]) for xyz1, nothing for xyz2
        xyz1, xyz2, assignment = ctx.saved_tensors
        matched = torch.gather(xyz2, 1, assignment.long().unsqueeze(-1).expand(-1, -1, 3))
        g = (graddist.contiguous() * 2).unsqueeze(-1)
        return g * (xyz1 - matched), torch.zeros_like(xyz2), None, None


class emdModule(nn.Module):
    def forward(self, input1, input2, eps, iters):
        return emdFunction.apply(input1, input2, eps, iters)


def _truncate(x, y):
    """The pair cut to its common length rounded down to a multiple of 1024 (metric_utils.py:450-452)."""
    for name, a in (("x", x), ("y", y)):
        if not isinstance(a, (np.ndarray, torch.Tensor)) or a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"compute_pairwise_emd: `{name}` must be an [N, 3] cloud")
    n = min(x.shape[0], y.shape[0])
    n -= n % 1024
    if n == 0:
        raise ValueError("compute_pairwise_emd: fewer than 1024 points in common")
    return x[:n], y[:n]


def _dev(a):
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("compute_pairwise_emd needs the MI355X: no CPU fallback on the hot path")
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    if not a.is_cuda:
        raise RuntimeError("compute_pairwise_emd: tensors must be CUDA(HIP) tensors -- no CPU fallback on the hot path")
    return a.float().contiguous()


def compute_pairwise_emd(x, y, module=None):
    module = emdModule() if module is None else module
    x, y = _truncate(x, y)
    dist, _ = module(_dev(x)[None], _dev(y)[None], EPS, ITERS)
    return torch.sqrt(dist).mean().item()


def compute_pairwise_emd_batch(reference, samples):
    """[compute_pairwise_emd(r, s) for r, s in zip(reference, samples)], one launch per truncated length."""
    if len(reference) != len(samples):
        raise ValueError("compute_pairwise_emd_batch: as many reference clouds as samples")
    pairs = [_truncate(r, s) for r, s in zip(reference, samples)]
    by_len = {}
    for i, (r, _) in enumerate(pairs):
        by_len.setdefault(r.shape[0], []).append(i)
    out = [None] * len(pairs)
    for idx in by_len.values():
        a = torch.stack([_dev(pairs[i][0]) for i in idx])
        b = torch.stack([_dev(pairs[i][1]) for i in idx])
        dist, _ = emdModule()(a, b, EPS, ITERS)
        for row, i in enumerate(idx):
            out[i] = torch.sqrt(dist[row:row + 1]).mean().item()   # the reduction of the one-pair call, bit for bit
    return out
