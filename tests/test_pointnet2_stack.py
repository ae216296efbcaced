"""GPU tests of lidargen.ops.pointnet2.pointnet2_stack (csrc/pointnet2_stack.hip, lidarcrafter_amd.ops_pointnet2) against
the numpy oracle of tests/_pointnet2_stack_oracle.py.

Index kernels: equality.  On the quarter grid (coordinates k / 4, k = 0..16) every distance is exact in float32, so the
strict < of the ball query and the inclusive <= of the voxel query are decided on pairs that lie exactly on the sphere.  On
random clouds the test first asserts, on its own inputs, that no decision depends on the precision, then asks for equality.
Sums (interpolation backward): bit-equal to the oracle's ascending order.  The gathered first layer and the fused
route: bit-equal to the materialised formulation through lc_pointmlp_conv_fwd.  Modules against float64 on the CPU: the
largest per-row relative L2 error is at most twice that of the float32 torch module on the same inputs (both are float32
sums of equal length in different orders)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnet2_stack_oracle as O  # noqa: E402
from _pointnet2_stack_cases import (FEW_KNOWN, I, T, clouds, fp_module_errors, neighbor_voxel_module_errors,  # noqa: E402
                                    sa_cpu, sa_dev_args, sa_inputs, sa_module, voxel_scene)

from lidarcrafter_amd import ops_pointmlp as KM  # noqa: E402
from lidarcrafter_amd import ops_pointnet2 as KP  # noqa: E402
from lidargen.ops.pointnet2.pointnet2_stack import pointnet2_utils as PU  # noqa: E402
from lidargen.ops.pointnet2.pointnet2_stack import voxel_query_utils as VQ  # noqa: E402

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def same_bits(got, want):
    want = np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(bits(got.contiguous()), want.view(np.int32))


# ---- ball query ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [1, 16, 32])
@pytest.mark.parametrize("radius", [1.25, 0.2])
@pytest.mark.parametrize("layout", ["base", "gaps"])
def test_ball_query_quarter_grid(dev, layout, radius, nsample):
    xyz, pc, new, cc = clouds(layout, "grid")
    sizes = []
    want = O.ball_query(xyz, pc, new, cc, radius, nsample, sizes=sizes)
    if layout == "base":
        o, c = O.offsets(pc), O.offsets(cc)
        on = sum(int((O.sqdist(xyz[o[b]:o[b + 1]], q, np.float64) == O.radius2(radius, np.float64)).sum())
                 for b in range(3) for q in new[c[b]:c[b + 1]])
        if radius == 1.25:
            assert on > 10, "no pair on the sphere: the strict < is not exercised"
        else:
            assert sum(s == 0 for s in sizes) > len(sizes) // 2, "few empty balls"
    raw = KP.ball_query(radius, nsample, T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev))
    assert np.array_equal(raw.cpu().numpy(), want)
    idx, mask = PU.ball_query(radius, nsample, T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev))
    widx, wmask = O.finish_query(want)
    assert idx.dtype == torch.int32 and mask.dtype == torch.bool and not idx.requires_grad
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(mask.cpu().numpy(), wmask)


def test_ball_query_limits(dev):
    xyz, pc, new, cc = clouds("base", "grid")
    big = KP.limit("max_nsample")
    assert big >= 128
    raw = KP.ball_query(8.0, big, T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev))
    assert np.array_equal(raw.cpu().numpy(), O.ball_query(xyz, pc, new, cc, 8.0, big))
    with pytest.raises(NotImplementedError, match="LC_PN2_MAX_NSAMPLE"):
        KP.ball_query(1.0, big + 1, T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev))


# ---- voxel query ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [1, 8])
@pytest.mark.parametrize("layout", ["base", "gaps"])
def test_voxel_query_quarter_grid(dev, layout, nsample):
    xyz, pc, new, cc, coords, pi = voxel_scene(layout)
    rng_, radius = (1, 2, 1), 0.5
    want = O.voxel_query(rng_, radius, nsample, xyz, new, coords, pi)
    on = sum(int((O.sqdist(xyz, q, np.float64) == 0.25).sum()) for q in new)
    assert on > 0 and (want[:, 0] == -1).any() and (want[:, 0] >= 0).any()
    raw = KP.voxel_query(rng_, radius, nsample, T(xyz, dev), T(new, dev), T(coords, dev), T(pi, dev))
    assert np.array_equal(raw.cpu().numpy(), want)
    idx, mask = VQ.voxel_query(rng_, radius, nsample, T(xyz, dev), T(new, dev), T(coords, dev), T(pi, dev))
    widx, wmask = O.finish_query(want)
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(mask.cpu().numpy(), wmask)
    # the strict comparison would lose pairs that lie on the sphere inside the walked cells
    if layout == "base":
        assert not np.array_equal(want, O.voxel_query(rng_, radius, nsample, xyz, new, coords, pi, inclusive=False))


# ---- three nearest neighbours --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["base", "gaps", FEW_KNOWN])
def test_three_nn_quarter_grid(dev, layout):
    """`known` = the layout's centres, `unknown` = its points: FEW_KNOWN has clouds of two and of one known point, 'gaps'
    a cloud without any."""
    unknown, uc, known, kc = clouds(layout, "grid")
    wd2, widx = O.three_nn(unknown, uc, known, kc)
    d2, idx = KP.three_nn(T(unknown, dev), I(uc, dev), T(known, dev), I(kc, dev))
    assert np.array_equal(idx.cpu().numpy(), widx) and same_bits(d2, wd2)
    dist, idx2 = PU.three_nn(T(unknown, dev), I(uc, dev), T(known, dev), I(kc, dev))
    assert torch.equal(idx2, idx) and torch.equal(dist, torch.sqrt(T(wd2, dev)))
    if layout != "base":
        assert np.isinf(wd2).any()


# ---- random clouds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_clouds_indices(dev, seed):
    layout = ([300], [67])
    xyz, pc, new, cc = clouds(layout, "uniform", seed)
    radius, nsample = 0.8, 16
    r2 = O.radius2(radius, np.float64)
    excluded = 0
    for q in new:
        d64 = O.sqdist(xyz, q, np.float64)
        excluded += int((np.abs(d64 - r2) <= 1e-5 * r2).any())
    assert excluded == 0                                          # the cap on excluded centres is 0
    sizes = []
    O.ball_query(xyz, pc, new, cc, radius, nsample, sizes=sizes)
    # balls smaller than nsample and balls that fill the row: at 16 in the draws of seeds 0 - 2 (the largest ball of seed 3
    # holds 15 points), and in every draw at the median ball size
    assert min(sizes) < nsample and (seed == 3 or max(sizes) >= nsample)
    median = sorted(sizes)[len(sizes) // 2]
    assert min(sizes) < median <= max(sizes)
    for ns in (nsample, median):
        want = O.ball_query(xyz, pc, new, cc, radius, ns)
        assert np.array_equal(want, O.ball_query(xyz, pc, new, cc, radius, ns, dtype=np.float64))
        raw = KP.ball_query(radius, ns, T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev))
        assert np.array_equal(raw.cpu().numpy(), want)
    # three-NN of the centres among the points
    wd2, widx = O.three_nn(new, cc, xyz, pc)
    d64, i64 = O.three_nn(new, cc, xyz, pc, dtype=np.float64)
    assert np.array_equal(widx, i64)
    d2, idx = KP.three_nn(T(new, dev), I(cc, dev), T(xyz, dev), I(pc, dev))
    assert np.array_equal(idx.cpu().numpy(), widx) and same_bits(d2, wd2)


# ---- grouping ------------------------------------------------------------------------------------------------------------
def _group_case(layout, C=5, nsample=16, seed=0):
    xyz, pc, new, cc = clouds(layout, "grid", seed)
    idx, _ = O.finish_query(O.ball_query(xyz, pc, new, cc, 1.25, nsample))
    rng = np.random.default_rng(100 + seed)
    feats = rng.standard_normal((len(xyz), C)).astype(np.float32)
    return feats, pc, idx, cc, rng


@pytest.mark.parametrize("layout", ["base", "gaps"])
def test_grouping_forward(dev, layout):
    feats, pc, idx, cc, _ = _group_case(layout)
    f, i = T(feats, dev), T(idx, dev)
    out = PU.grouping_operation(f, I(pc, dev), i, I(cc, dev))
    start = T(O.offsets(pc)[:-1][O.batch_of(cc)], dev)[:, None]                     # [M, 1]
    inside = i.long() < T(np.asarray(pc)[O.batch_of(cc)], dev)[:, None]             # (row 0 of an empty ball in an empty cloud)
    rows = torch.where(inside, start + i.long(), torch.zeros_like(start)).reshape(-1)
    want = f.index_select(0, rows).view(idx.shape[0], idx.shape[1], -1) * inside[:, :, None]
    want = want.permute(0, 2, 1)
    assert torch.equal(out, want) and same_bits(out, O.group(feats, pc, idx, cc))


def test_grouping_out_of_range_indices(dev):
    feats, pc, idx, cc, rng = _group_case("base", nsample=4)
    idx = idx.copy()
    idx[0, 1], idx[5, 0], idx[41, 0], idx[50, 2] = -1, 300, 1, 67     # below 0 / one past the end of clouds 0, 1 and 2
    want = O.group(feats, pc, idx, cc)
    assert (want[0, :, 1] == 0).all() and (want[41, :, 0] == 0).all() and (want[50, :, 2] == 0).all()
    out = PU.grouping_operation(T(feats, dev), I(pc, dev), T(idx, dev), I(cc, dev))
    assert same_bits(out, want)


# ---- interpolation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["base", FEW_KNOWN])
def test_three_interpolate(dev, layout):
    unknown, uc, known, kc = clouds(layout, "grid")
    C, M, N = 7, len(known), len(unknown)
    rng = np.random.default_rng(7)
    kf = rng.standard_normal((M, C)).astype(np.float32)
    dist, idx = PU.three_nn(T(unknown, dev), I(uc, dev), T(known, dev), I(kc, dev))
    recip = 1.0 / (dist + 1e-8)
    weight = recip / torch.sum(recip, dim=-1, keepdim=True)
    if layout != "base":
        assert bool((weight == 0).any()) and bool(torch.isinf(dist).any())       # fewer than three known points
    w, i = weight.cpu().numpy(), idx.cpu().numpy()
    f = T(kf, dev).requires_grad_(True)
    out = PU.three_interpolate(f, idx, weight)
    assert same_bits(out, O.three_interpolate(kf, i, w))
    gi = rng.integers(-8, 9, (N, C)).astype(np.float32)
    wi = T(np.ones_like(w), dev)
    out_i = PU.three_interpolate(f, idx, wi)
    (g,) = torch.autograd.grad(out_i, f, T(gi, dev))
    assert same_bits(g, O.three_interpolate_bwd(gi, i, np.ones_like(w), M))      # integer terms: the indices
    gr = rng.standard_normal((N, C)).astype(np.float32)
    (g1,) = torch.autograd.grad(out, f, T(gr, dev), retain_graph=True)
    (g2,) = torch.autograd.grad(out, f, T(gr, dev))
    assert same_bits(g1, O.three_interpolate_bwd(gr, i, w, M)) and torch.equal(g1, g2)


def test_three_interpolate_out_of_range(dev):
    kf = np.arange(12, dtype=np.float32).reshape(4, 3)
    idx = np.array([[0, 4, -1], [3, 3, 9]], np.int32)
    w = np.array([[0.5, 0.25, 0.25], [0.5, 0.5, 1.0]], np.float32)
    out = PU.three_interpolate(T(kf, dev), T(idx, dev), T(w, dev))
    assert same_bits(out, O.three_interpolate(kf, idx, w))
    g = KP.three_interpolate_bwd(torch.ones(2, 3, device=dev), T(idx, dev), T(w, dev), 4)
    assert same_bits(g, O.three_interpolate_bwd(np.ones((2, 3), np.float32), idx, w, 4))


# ---- stacked farthest point sampling -------------------------------------------------------------------------------------
_FPS = {}


def _fps_case():
    if not _FPS:
        rng = np.random.default_rng(11)
        counts = [1, 7, 300, 1025, 2500]
        parts = [rng.random((n, 3)).astype(np.float32) * 4 for n in counts]
        parts[1] = parts[1][np.arange(7) % 3]                       # 3 distinct points, 6 picks
        parts[2] = (rng.integers(0, 5, (300, 3)) / 4).astype(np.float32)   # ties at every pick
        xyz = np.concatenate(parts)
        npoints = [1, 6, 40, 33, 20]
        _FPS.update(xyz=xyz, counts=counts, npoints=npoints, want=O.fps_stack(xyz, counts, npoints))
    return _FPS


@pytest.mark.parametrize("as_tensor", [False, True], ids=["list", "tensor"])
def test_stack_fps(dev, as_tensor):
    c = _fps_case()
    npoint = torch.tensor(c["npoints"], device=dev).int() if as_tensor else list(c["npoints"])
    got = PU.stack_farthest_point_sample(T(c["xyz"], dev), I(c["counts"], dev), npoint)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), c["want"])


def test_stack_fps_int_count_and_limit(dev):
    rng = np.random.default_rng(12)
    xyz = rng.random((90, 3)).astype(np.float32)
    got = PU.stack_farthest_point_sample(T(xyz, dev), I([40, 50], dev), 9)
    assert np.array_equal(got.cpu().numpy(), O.fps_stack(xyz, [40, 50], [9, 9]))
    n = KM.limit("fps_max_n") + 1
    with pytest.raises(NotImplementedError, match="LC_FPS_MAX_N"):
        PU.stack_farthest_point_sample(torch.zeros(n, 3, device=dev), I([n], dev), 4)


# ---- the gathered first layer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [1, 16])
@pytest.mark.parametrize("Co", [16, 33, 64])
@pytest.mark.parametrize("C", [0, 1, 29, 32, 61])
def test_gathered_first_layer(dev, C, Co, nsample):
    xyz, pc, new, cc = clouds("base", "grid")
    radius = 0.6
    rng = np.random.default_rng(1000 * C + 10 * Co + nsample)
    feats = None if C == 0 else T(rng.standard_normal((len(xyz), C)).astype(np.float32), dev)
    w = torch.from_numpy(rng.standard_normal((Co, C + 3)).astype(np.float32))
    bias = T(rng.standard_normal(Co).astype(np.float32), dev)
    wpk = KM.pack_weight(w).to(dev)
    args = (T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev))
    raw = KP.ball_query(radius, nsample, *args)
    empty = raw[:, 0] == -1
    assert bool(empty.any()) and not bool(empty.all())
    L = raw.shape[0] * nsample
    assert L % KM.conv_block_cols(Co) != 0
    got = KP.sa_first(*args, feats, raw, wpk, bias, Co)
    grouped, idx = PU.QueryAndGroup(radius, nsample, use_xyz=True)(*args, feats)    # [M, C + 3, nsample]
    assert grouped.shape[1] == C + 3 and bool((grouped[empty] == 0).all())
    x = grouped.permute(1, 0, 2).reshape(1, C + 3, L).contiguous()
    assert torch.equal(got, KM.conv(x, wpk, bias, Co, True))


@pytest.mark.parametrize("Co", [65, 128])
def test_gathered_first_layer_four_channel_blocks(dev, Co):
    """Co > 64: the geometry with four channel blocks per block (64 columns per block)."""
    test_gathered_first_layer(dev, 29, Co, 16)


def test_gathered_first_layer_without_xyz_and_bad_indices(dev):
    xyz, pc, new, cc = clouds("gaps", "grid")
    C, Co, ns = 8, 40, 4
    rng = np.random.default_rng(3)
    feats = T(rng.standard_normal((len(xyz), C)).astype(np.float32), dev)
    w = torch.from_numpy(rng.standard_normal((Co, C)).astype(np.float32))
    bias, wpk = T(rng.standard_normal(Co).astype(np.float32), dev), KM.pack_weight(w).to(dev)
    args = (T(xyz, dev), I(pc, dev), T(new, dev), I(cc, dev))
    raw = KP.ball_query(1.25, ns, *args)
    got = KP.sa_first(*args, feats, raw, wpk, bias, Co, use_xyz=False)
    grouped, _ = PU.QueryAndGroup(1.25, ns, use_xyz=False)(*args, feats)
    x = grouped.permute(1, 0, 2).reshape(1, C, -1).contiguous()
    assert torch.equal(got, KM.conv(x, wpk, bias, Co, True))
    # an index outside its cloud reads nothing: zero features, 0 - centre for the coordinates
    w3 = torch.from_numpy(rng.standard_normal((Co, C + 3)).astype(np.float32))
    wpk3 = KM.pack_weight(w3).to(dev)
    bad = raw.clone()
    live = torch.nonzero(bad[:, 0] >= 0).reshape(-1)
    bad[live[0], 1], bad[live[1], 2] = 100000, -5
    got = KP.sa_first(*args, feats, bad, wpk3, bias, Co)
    idx, mask = bad.clone(), bad[:, 0] == -1
    idx[mask] = 0
    gx = PU.grouping_operation(args[0], args[1], idx, args[3]) - args[2].unsqueeze(-1)
    gf = PU.grouping_operation(feats, args[1], idx, args[3])
    gx[mask], gf[mask] = 0, 0
    x = torch.cat([gx, gf], dim=1).permute(1, 0, 2).reshape(1, C + 3, -1).contiguous()
    assert torch.equal(got, KM.conv(x, wpk3, bias, Co, True))


# ---- modules -------------------------------------------------------------------------------------------------------------
SANE = 3 * 64 * 2.0 ** -24
"""A sanity bound where the exact statement is made elsewhere (bit equality with the materialised route): three layers of
float32 sums of at most 64 terms, each within terms x 2^-24 of its exact value relative to sum|ab|."""


def _sa_materialised(module, args):
    """The operator route with the layers run through lc_pointmlp_conv_fwd and the maximum in torch."""
    outs = []
    for grouper, layers in zip(module.groupers, module.packed(args[0].device)):
        grouped, _ = grouper(*args)
        M, Ci, ns = grouped.shape
        y = grouped.permute(1, 0, 2).reshape(1, Ci, M * ns).contiguous()
        for wpk, b, Co in layers:
            y = KM.conv(y, wpk, b, Co, True)
        outs.append(y.view(y.shape[1], M, ns).max(dim=2)[0].permute(1, 0))
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("layout", ["base", "gaps"])
def test_sa_module_fused_equals_materialised(dev, layout, monkeypatch):
    module, inputs = sa_module().to(dev).eval(), sa_inputs(layout)
    args = sa_dev_args(inputs, dev)
    with torch.no_grad():
        new_xyz, fused = module(*args)
        assert new_xyz is args[2] and fused.shape == (len(inputs[2]), 73)
        assert torch.equal(fused, _sa_materialised(module, args))
        monkeypatch.setenv("LC_PN2_FUSED", "0")
        _, oper = module(*args)                                   # the operator route: torch's layers round differently
        ref = sa_cpu(module, inputs, torch.float64)[1].numpy()
    assert O.rel_l2_rows(oper.cpu().numpy(), ref).max() < SANE


def test_sa_module_against_float64(dev):
    module, inputs = sa_module().to(dev).eval(), sa_inputs("base")
    with torch.no_grad():
        _, fused = module(*sa_dev_args(inputs, dev))
        ref = sa_cpu(module, inputs, torch.float64)[1].numpy()
        f32 = sa_cpu(module, inputs, torch.float32)[1].numpy()
    e_hip, e_torch = O.rel_l2_rows(fused.cpu().numpy(), ref).max(), O.rel_l2_rows(f32, ref).max()
    print(f"StackSAModuleMSG eval, max per-row rel L2 vs float64: fused HIP {e_hip:.3e}, float32 torch {e_torch:.3e}")
    assert e_hip <= 2 * e_torch


def test_sa_module_cloud_alone_and_in_batch(dev):
    module, inputs = sa_module().to(dev).eval(), sa_inputs("base")
    xyz, pc, new, cc, feats = inputs
    with torch.no_grad():
        _, both = module(*sa_dev_args(inputs, dev))
        po, co = O.offsets(pc), O.offsets(cc)
        for b in (0, 2):
            alone = (xyz[po[b]:po[b + 1]], [pc[b]], new[co[b]:co[b + 1]], [cc[b]], feats[po[b]:po[b + 1]])
            _, one = module(*sa_dev_args(alone, dev))
            assert torch.equal(one, both[co[b]:co[b + 1]])


def test_sa_module_repacks_after_optimizer_step(dev):
    module, inputs = sa_module(seed=5).to(dev), sa_inputs("base")
    args = sa_dev_args(inputs, dev)
    module.eval()
    with torch.no_grad():
        _, before = module(*args)
    packed = module.packed(dev)
    assert module.packed(dev) is packed                          # unchanged parameters: the cached pack
    opt = torch.optim.SGD(module.parameters(), lr=0.05)
    g = torch.Generator().manual_seed(8)
    for p in module.parameters():                                # (gradients set by hand: any step must re-pack)
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt.step()
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.add_(0.1)
    with torch.no_grad():
        _, after = module(*args)
        assert module.packed(dev) is not packed and not torch.equal(after, before)
        assert torch.equal(after, _sa_materialised(module, args))
        ref = sa_cpu(module, inputs, torch.float64)[1].numpy()
    assert O.rel_l2_rows(after.cpu().numpy(), ref).max() < SANE


def test_fp_module_against_float64(dev):
    got, e_hip, e_torch = fp_module_errors(dev)
    print(f"StackPointnetFPModule, max per-row rel L2 vs float64: HIP route {e_hip:.3e}, float32 torch {e_torch:.3e}")
    assert got.shape == (368, 17) and e_hip <= 2 * e_torch


def test_neighbor_voxel_module_against_float64(dev):
    got, e_hip, e_torch = neighbor_voxel_module_errors(dev)
    print(f"NeighborVoxelSAModuleMSG, max per-row rel L2 vs float64: HIP route {e_hip:.3e}, float32 torch {e_torch:.3e}")
    assert got.shape == (40, 32) and e_hip <= 2 * e_torch
