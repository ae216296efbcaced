"""Shared inputs and CPU restatements of the pointnet2_stack module tests (tests/test_pointnet2_stack.py) and of the timing
script (devtools/pointnet2_stack_time.py): seeded clouds, the voxel scene, the test modules and their float64 / float32
restatements from torch layers over the oracle's indices."""
import copy

import numpy as np
import torch
import torch.nn as nn

import _pointnet2_stack_oracle as O
from lidargen.ops.pointnet2.pointnet2_stack import pointnet2_modules as PM
from lidargen.ops.pointnet2.pointnet2_stack import voxel_pool_modules as VM

LAYOUTS = {"base": ([300, 1, 67], [40, 3, 24]),
           "gaps": ([120, 0, 30, 67], [20, 5, 0, 24])}     # a cloud without points, a cloud without centres


FEW_KNOWN = ([5, 2, 1, 0], [4, 2, 1, 2])           # `known` clouds of two and of one point

_CLOUDS = {}


def clouds(layout, kind, seed=0):
    """(xyz [N,3], xyz_cnt, new_xyz [M,3], new_cnt) float32 numpy: 'grid' = integers(0, 17) / 4, 'uniform' = [0, 4)^3."""
    key = (repr(layout), kind, seed)
    if key not in _CLOUDS:
        pc, cc = LAYOUTS[layout] if isinstance(layout, str) else layout
        rng = np.random.default_rng(seed)
        if kind == "grid":
            draw = lambda n: (rng.integers(0, 17, (n, 3)) / 4).astype(np.float32)  # noqa: E731
        else:
            draw = lambda n: (rng.random((n, 3)) * 4).astype(np.float32)  # noqa: E731
        xyz = draw(sum(pc))
        new = draw(sum(cc))
        for a in (xyz, new):
            a.setflags(write=False)
        _CLOUDS[key] = (xyz, list(pc), new, list(cc))
    return _CLOUDS[key]


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).to(dev)                # (a copy: the cached inputs stay read-only)
    return t if dtype is None else t.to(dtype)


def I(a, dev):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)


def voxel_scene(layout, seed=0):
    """Quarter-grid points in voxels of edge 1/4: point_indices [B,17,17,17] holds the last point of every voxel."""
    xyz, pc, new, cc = clouds(layout, "grid", seed)
    B = len(pc)
    pi = np.full((B, 17, 17, 17), -1, np.int32)
    cell = np.rint(xyz * 4).astype(np.int64)
    for k, b in enumerate(O.batch_of(pc)):
        pi[b, cell[k, 2], cell[k, 1], cell[k, 0]] = k
    nc = np.rint(new * 4).astype(np.int64)
    coords = np.stack([O.batch_of(cc), nc[:, 2], nc[:, 1], nc[:, 0]], axis=1).astype(np.int32)     # (batch, z, y, x)
    return xyz, pc, new, cc, coords, pi


def randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
            m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=g)
            m.bias.data = 0.2 * torch.randn(m.bias.shape, generator=g)
            m.running_mean.data = 0.2 * torch.randn(m.running_mean.shape, generator=g)
            m.running_var.data = 0.5 + torch.rand(m.running_var.shape, generator=g)
    return module


def sa_module(seed=0, C=6):
    torch.manual_seed(seed)
    m = PM.StackSAModuleMSG(radii=[0.7, 1.25], nsamples=[8, 16], mlps=[[C, 16, 33], [C, 24, 16, 40]], use_xyz=True)
    return randomise(m, seed + 1)


def sa_inputs(layout="base", C=6, seed=0):
    xyz, pc, new, cc = clouds(layout, "grid", seed)
    feats = np.random.default_rng(50 + seed).standard_normal((len(xyz), C)).astype(np.float32)
    return xyz, pc, new, cc, feats


def sa_cpu(module, inputs, dtype, pool="max"):
    """The module from torch layers on the CPU in `dtype` over the oracle's indices."""
    xyz, pc, new, cc, feats = inputs
    m = copy.deepcopy(module).cpu().to(dtype)
    outs = []
    for k, g in enumerate(m.groupers):
        raw = O.ball_query(xyz, pc, new, cc, g.radius, g.nsample)
        nd = np.float64 if dtype == torch.float64 else np.float32
        x = O.grouped_operand(xyz.astype(nd), pc, new, cc, feats.astype(nd), raw)
        x = torch.from_numpy(x).permute(1, 0, 2).unsqueeze(0)
        y = m.mlps[k](x)
        y = y.max(dim=3)[0] if pool == "max" else y.mean(dim=3)
        outs.append(y.squeeze(0).permute(1, 0))
    return m, torch.cat(outs, dim=1)


def sa_dev_args(inputs, dev):
    xyz, pc, new, cc, feats = inputs
    return T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev), T(feats, dev)


def fp_module_errors(dev):
    """(output, its largest per-row relative L2 error against float64, the float32 torch module's)."""
    unknown, uc, known, kc = clouds("base", "grid")
    rng = np.random.default_rng(21)
    uf, kf = rng.standard_normal((len(unknown), 5)).astype(np.float32), rng.standard_normal((len(known), 9)).astype(np.float32)
    torch.manual_seed(2)
    module = randomise(PM.StackPointnetFPModule(mlp=[14, 24, 17]), 4).eval()
    with torch.no_grad():
        got = module.to(dev)(T(unknown, dev), I(uc, dev), T(known, dev), I(kc, dev), T(uf, dev), T(kf, dev)).cpu().numpy()
        res = {}
        for dtype, nd in ((torch.float64, np.float64), (torch.float32, np.float32)):
            d2, idx = O.three_nn(unknown, uc, known, kc, dtype=nd)
            dist = torch.sqrt(torch.from_numpy(d2))
            recip = 1.0 / (dist + 1e-8)
            w = (recip / torch.sum(recip, dim=-1, keepdim=True)).numpy()
            x = np.concatenate([O.three_interpolate(kf.astype(nd), idx, w), uf.astype(nd)], axis=1)
            m = copy.deepcopy(module).cpu().to(dtype)
            res[dtype] = m.mlp(torch.from_numpy(x).permute(1, 0)[None, :, :, None])[0, :, :, 0].permute(1, 0).numpy()
    e_hip = O.rel_l2_rows(got, res[torch.float64]).max()
    e_torch = O.rel_l2_rows(res[torch.float32], res[torch.float64]).max()
    return got, float(e_hip), float(e_torch)


def neighbor_voxel_module_errors(dev):
    """(output, its largest per-row relative L2 error against float64, the float32 torch module's)."""
    layout = ([150, 90], [20, 20])                                  # the reference's view needs equal centres per cloud
    xyz, pc, new, cc, coords, pi = voxel_scene(layout, seed=2)
    C = 6
    feats = np.random.default_rng(31).standard_normal((len(xyz), C)).astype(np.float32)
    torch.manual_seed(6)
    module = randomise(VM.NeighborVoxelSAModuleMSG(query_ranges=[[1, 1, 1], [2, 2, 2]], radii=[0.4, 0.75], nsamples=[4, 16],
                                                    mlps=[[C, 16, 20], [C, 24, 12]]), 7).eval()
    xyz_order = coords[:, [0, 3, 2, 1]]                             # the module takes [batch, x, y, z]
    with torch.no_grad():
        got = module.to(dev)(T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev), T(xyz_order, dev), T(feats, dev),
                             T(pi, dev)).cpu().numpy()
        res = {}
        po = O.offsets(pc)
        for dtype, nd in ((torch.float64, np.float64), (torch.float32, np.float32)):
            m = copy.deepcopy(module).cpu().to(dtype)
            outs = []
            for k, g in enumerate(m.groupers):
                fin = m.mlps_in[k](torch.from_numpy(feats.astype(nd)).permute(1, 0).unsqueeze(0))[0].permute(1, 0).numpy()
                raw = O.voxel_query(g.max_range, g.radius, g.nsample, xyz, new, coords, pi)
                idx, mask = O.finish_query(raw)
                idx = idx - po[:-1][O.batch_of(cc)][:, None]
                idx[mask] = 0
                gf = O.group(fin, pc, idx, cc)
                gx = O.group(xyz.astype(nd), pc, idx, cc) - new.astype(nd)[:, :, None]
                gf[mask], gx[mask] = 0, 0
                pos = m.mlps_pos[k](torch.from_numpy(gx).permute(1, 0, 2).unsqueeze(0))
                y = torch.relu(torch.from_numpy(gf).permute(1, 0, 2).unsqueeze(0) + pos).max(dim=3)[0]
                outs.append(m.mlps_out[k](y)[0].permute(1, 0))
            res[dtype] = torch.cat(outs, dim=1).numpy()
    e_hip = O.rel_l2_rows(got, res[torch.float64]).max()
    e_torch = O.rel_l2_rows(res[torch.float32], res[torch.float64]).max()
    return got, float(e_hip), float(e_torch)
