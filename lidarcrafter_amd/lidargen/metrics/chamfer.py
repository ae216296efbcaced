"""Chamfer distance -- mirror of the reference's `lidargen/metrics/modules/chamfer3D/
dist_chamfer_3D.py` (`chamfer_3DDist`), `modules/chamfer2D/dist_chamfer_2D.py` (`chamfer_2DDist`) and of
`compute_pairwise_cd` / `compute_pairwise_cd_batch` (`lidargen/metrics/metric_utils.py:415-444`).  Both modules are
differentiable, as in the reference: `chamfer_3DFunction` / `chamfer_2DFunction` are its `torch.autograd.Function`s
(dist_chamfer_3D.py:28-66), the forward ops.chamfer3d / chamfer2d, the backward ops.chamfer3d_backward /
chamfer2d_backward -- the reference's gradient terms summed in a fixed order instead of its float atomicAdd, so a loss
through them has the same gradient bits alone, in any batch and from run to run (csrc/chamfer_bwd.hip).  idx1 / idx2
are not differentiable, and the backward is differentiable once.  The evaluation callers below pass tensors that need
no gradient and get the forward's values unchanged.  `bev_min_matching` is this project's own: the row minima that
compute_mmd averages, on the grid route (ops.bev_chamfer_min) or, for a grid that route does not take, on the literal
one."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from lidarcrafter_amd import ops as K


def _chamfer_function(name, fwd, bwd):
    class _Fn(Function):
        @staticmethod
        def forward(ctx, xyz1, xyz2):
            xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
            dist1, dist2, idx1, idx2 = fwd(xyz1, xyz2)
            ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
            ctx.mark_non_differentiable(idx1, idx2)
            return dist1, dist2, idx1, idx2

        @staticmethod
        @once_differentiable
        def backward(ctx, graddist1, graddist2, gradidx1, gradidx2):
            xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
            return bwd(xyz1, xyz2, graddist1.float().contiguous(), graddist2.float().contiguous(), idx1, idx2)

    _Fn.__name__ = _Fn.__qualname__ = name
    return _Fn


chamfer_3DFunction = _chamfer_function("chamfer_3DFunction", K.chamfer3d, K.chamfer3d_backward)
chamfer_2DFunction = _chamfer_function("chamfer_2DFunction", K.chamfer2d, K.chamfer2d_backward)


class chamfer_3DDist(nn.Module):
    def forward(self, input1, input2):
        return chamfer_3DFunction.apply(input1.float(), input2.float())


class chamfer_2DDist(nn.Module):
    def forward(self, input1, input2):
        return chamfer_2DFunction.apply(input1.float(), input2.float())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() if isinstance(a, np.ndarray) else a


def compute_pairwise_cd(x, y, module=None):
    module = chamfer_3DDist() if module is None else module
    x, y = _dev(x), _dev(y)
    if x.ndim == 2 and y.ndim == 2:
        x, y = x[None], y[None]
    dist1, dist2, _, _ = module(x, y)
    return ((dist1.mean() + dist2.mean()) / 2).item()


def compute_pairwise_cd_batch(reference, samples):
    """One reference cloud against a list of clouds: shorter clouds are padded with points at 1e6
    (as the reference does) and the padded tail is excluded from the means.  [n, 3] clouds go through
    chamfer_3DDist, [n, 2] clouds (pcd2bev_bin's cells) through chamfer_2DDist."""
    assert reference.ndim == 2 and reference.shape[1] in (2, 3), "[n, 3] or [n, 2] clouds"
    dim = reference.shape[1]
    module = chamfer_3DDist() if dim == 3 else chamfer_2DDist()
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    reference, samples = host(reference), [host(s) for s in samples]
    len_r, len_s = reference.shape[0], [s.shape[0] for s in samples]
    max_len = max([len_r] + len_s)
    padv = lambda a: np.vstack([a, np.ones((max_len - a.shape[0], dim), dtype=np.float32) * 1e6])
    ref = _dev(padv(np.asarray(reference, np.float32)))
    smp = _dev(np.stack([padv(np.asarray(s, np.float32)) for s in samples]))
    dist_r, dist_s, _, _ = module(ref[None].expand_as(smp).contiguous(), smp)
    return [((dist_r[i, :len_r].mean() + dist_s[i, :len_s[i]].mean()) / 2.).item()
            for i in range(smp.shape[0])]


def bev_min_matching(reference, samples, x_range, y_range, voxel_size=0.5, route="auto"):
    """For every reference cloud: (min over the samples of the 2-D chamfer distance of their BEV cell sets, its index),
    two float64 / int64 numpy arrays.  route 'grid': ops.bev_chamfer_min (exact); 'literal': pcd2bev_bin's cells through
    compute_pairwise_cd_batch per reference, as the reference's compute_mmd does; 'auto': the grid route, the literal
    one where the grid is outside what the distance transform takes."""
    from . import metric_utils

    assert route in ("auto", "grid", "literal")
    ref, smp = [_dev(c).float() for c in reference], [_dev(c).float() for c in samples]
    if route != "literal":
        try:
            mn, arg = K.bev_chamfer_min(ref, smp, x_range, y_range, voxel_size)
            return mn.cpu().numpy(), arg.cpu().numpy()
        except K.BevGridUnsupported:
            if route == "grid":
                raise
    r_cells, s_cells = ([c.cpu().numpy() for c in sets]
                        for sets in metric_utils.bev_bin(x_range, y_range, voxel_size, ref, smp))
    for name, sets in (("reference", r_cells), ("sample", s_cells)):
        for k, c in enumerate(sets):
            if c.shape[0] == 0:
                raise ValueError(f"bev_min_matching: {name} cloud {k} has no point inside the BEV range")
    mins, args = [], []
    for r in r_cells:
        d = compute_pairwise_cd_batch(r, s_cells)
        args.append(int(np.argmin(d)))
        mins.append(d[args[-1]])
    return np.asarray(mins, np.float64), np.asarray(args, np.int64)
