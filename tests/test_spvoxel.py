"""GPU tests of the point <-> voxel exchanges (csrc/spvoxel.hip), the SPVCNN extractor built on them and the Frechet
Point-Voxel Distance front-end, against the float64 restatement of tests/_spvcnn_oracle.py (itself pinned on grid_sample by
tests/test_spvcnn_host.py).  `pytest -m gpu`.

Tolerances, as in tests/test_spconv.py: the oracle runs the same arithmetic in float32; the row-wise rel-L2 of that against
float64 is measured at run time and the kernel may be 4 x as far off, never less than TOL_CONV.  Integer results (the
neighbour rows) and the scatter-mean's bits (against a float32 loop in the documented order) are compared exactly."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spconv_hash as H  # noqa: E402
import _spconv_oracle as O  # noqa: E402
import _spvcnn_oracle as PV  # noqa: E402

from lidarcrafter_amd import ops_spconv as KS  # noqa: E402
from lidarcrafter_amd import ops_spvoxel as KV  # noqa: E402
from lidarcrafter_amd.testing import seeded_randn, synth_points  # noqa: E402
from tests._profile_cases import TOL_CONV  # noqa: E402   2e-6: the project's tolerance for its fp32-accurate kernels

pytestmark = pytest.mark.gpu
DEPTH_RANGE = [1.0, 45.0]            # nuScenes ('32')


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _limit(ref32, ref64):
    base = float(O.rel_l2_rows(ref32, ref64).max())
    return max(4.0 * base, TOL_CONV), base


def _check_rows(got, ref32, ref64, what):
    limit, base = _limit(ref32, ref64)
    err = float(O.rel_l2_rows(got, ref64).max())
    print(f"{what}: worst row rel-L2 {err:.2e}; float32 oracle {base:.2e}; ratio {err / max(base, 1e-30):.2f}; "
          f"limit {limit:.2e}")
    assert bool(torch.isfinite(got).all()) and err < limit, (what, err, limit)


# ---- the float coordinate ---------------------------------------------------------------------------------------------
def test_float_coordinate_on_the_device_is_the_restatement(dev):
    """(c * 0.05) / 0.05 by torch's own expression on the device, bit for bit the numpy restatement (a multiplication by
    the float32 reciprocal), for every c in [0, 4096); the model's helper is that expression."""
    from lidargen.metrics.models.spvcnn.model import float_coords

    c = torch.arange(4096, dtype=torch.float32, device=dev)
    got = ((c * 0.05) / 0.05).cpu().numpy()
    want = PV.float_coord(np.arange(4096))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert int((got != np.arange(4096)).sum()) > 0
    ci = torch.stack([torch.arange(4096), torch.arange(4096).flip(0), torch.arange(4096) // 3, torch.arange(4096) % 5], 1)
    pts = float_coords(ci.to(torch.int32).to(dev), 0.05, 0.05).cpu()
    assert torch.equal(pts, PV.point_coords(ci))


# ---- query ------------------------------------------------------------------------------------------------------------
def _map_scene(s):
    """The three-cloud scene of tests/test_spconv.py `_map_scene`, restated: coordinates at stride s, rows shuffled.
    Cloud 0: a solid 4 x 4 x 4 block at the origin, an isolated voxel, a pair along x and two voxels at the largest
    supported x.  Clouds 1 and 2: the same coordinates as each other, among them (0, 0, 0) -- where a probe of cloud 0 at
    the largest x + s would land if it wrapped out of its field of the key."""
    top = KS.MAX_COORD // s
    block = [(x, y, z) for x in range(4) for y in range(4) for z in range(4)]
    c0 = block + [(20, 21, 22), (30, 30, 30), (31, 30, 30), (top, 0, 0), (top - 1, 0, 0)]
    c12 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (5, 5, 5), (6, 5, 5), (6, 6, 6), (9, 0, 3)]
    rows = [(x * s, y * s, z * s, 0) for x, y, z in c0] + [(x * s, y * s, z * s, b) for b in (1, 2) for x, y, z in c12]
    c = torch.tensor(rows, dtype=torch.int64)
    return c[torch.randperm(len(c), generator=torch.Generator().manual_seed(s))]


def _scene_points(c, s):
    """Points on every voxel, at random fractions inside every voxel's cell and inside the cell before it (so that the
    voxel is the far corner), and four points with no voxel around them."""
    g = torch.Generator().manual_seed(100 + s)
    v = c[:, :3].float()
    inside = v + torch.rand((len(c), 3), generator=g) * s
    before = (v - torch.rand((len(c), 3), generator=g) * s).clamp_min(0)
    xyz = torch.cat([v, inside, before])
    b = c[:, 3].float().repeat(3)
    far = torch.tensor([[1000.0 * s, 1000.0 * s, 1000.0 * s, 0.0], [20.5 * s, 21.0 * s, 22.0 * s, 2.0],
                        [float(KS.MAX_COORD), float(KS.MAX_COORD), 0.5, 1.0], [9.25 * s, 1.5 * s, 3.0 * s, 0.0]])
    return torch.cat([torch.cat([xyz, b[:, None]], 1), far]).contiguous()


@pytest.mark.parametrize("s", [1, 4, 16])
def test_query_equals_the_oracle(dev, s):
    c = _map_scene(s)
    pts = _scene_points(c, s)
    want_idx, w64 = PV.point_maps(pts, c, s, torch.float64)
    _, w32 = PV.point_maps(pts, c, s, torch.float32)
    n_nbr = (want_idx >= 0).sum(1)
    assert int(n_nbr.max()) == 8 and int(n_nbr.min()) == 0 and sorted(set(n_nbr.tolist()))[:3] == [0, 1, 2]
    cd = c.to(torch.int32).to(dev)
    table = KS.hash_build(cd, int(c[:, :3].max()), 3)
    idx, w = KV.query(pts.to(dev), s, table, len(c))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (len(pts), 8) and tuple(w.shape) == (len(pts), 8)
    assert torch.equal(idx.cpu().long(), want_idx)
    # the same rows as the convolution's own table of the children of the point's cell
    base = torch.cat([(torch.floor(pts[:, :3] / s) * s), pts[:, 3:]], 1).to(torch.int32).to(dev)
    assert torch.equal(idx, KS.kernel_map(base, KS.KIND_DOWN, s, table, len(c)))
    _check_rows(w, w32, w64, f"trilinear weights, stride {s}")
    none = n_nbr == 0
    assert int(none.sum()) >= 3 and bool((w.cpu()[none] == 0).all()) and bool(torch.isfinite(w).all())
    # the voxel at the largest x: the probes at x + s are absent, not cloud 1's voxel at x = 0
    i = int((pts[:len(c), 0] == (KS.MAX_COORD // s) * s).nonzero()[0])
    assert int(idx[i, 0]) >= 0 and bool((idx[i, 4:] == -1).all())
    only_idx, no_w = KV.query(pts.to(dev), s, table, len(c), weights=False)
    assert no_w is None and torch.equal(only_idx, idx)
    again, w_again = KV.query(pts.to(dev), s, table, len(c))
    assert torch.equal(again, idx) and torch.equal(w_again, w)


def _hash_scenes():
    c, _ = H.clustered_scene()
    nb = KS.MAX_BATCH + 1
    return {"clustered": (c, 1, 3), "top-1": (H.top_scene(1), 1, nb), "top-4": (H.top_scene(4), 4, nb)}


@pytest.mark.parametrize("scene", ["clustered", "top-1", "top-4"])
def test_query_on_the_hash_scenes(dev, scene):
    """The query's own probe loop on the tables of tests/_spconv_hash.py: a chain of 300 keys that wraps the end of the
    table, and voxels at the largest coordinate of every axis and in the largest batch (the probes at + s beyond them
    are absent, not the voxel a carry into the next field of the key would name).  Points as in `_scene_points`."""
    c, s, n_batch = _hash_scenes()[scene]
    pts = _scene_points(c, s)
    want_idx, w64 = PV.point_maps(pts, c, s, torch.float64)
    _, w32 = PV.point_maps(pts, c, s, torch.float32)
    n_nbr = (want_idx >= 0).sum(1)
    assert int(n_nbr.max()) >= 2 and int(n_nbr.min()) == 0 and int((n_nbr > 0).sum()) >= 2 * len(c)
    cd = c.to(torch.int32).to(dev)
    table = KS.hash_build(cd, int(c[:, :3].max()), n_batch)
    keys, vals, disp, slots = H.table_invariants(table, c)
    if scene == "clustered":
        assert int((slots < H.sp_slot(keys[slots], H.CLUSTER_CAP)).sum()) >= 250 and int(disp.max()) >= 250
    idx, w = KV.query(pts.to(dev), s, table, len(c))
    assert torch.equal(idx.cpu().long(), want_idx)
    base = torch.cat([(torch.floor(pts[:, :3] / s) * s), pts[:, 3:]], 1).to(torch.int32).to(dev)
    assert torch.equal(idx, KS.kernel_map(base, KS.KIND_DOWN, s, table, len(c)))
    _check_rows(w, w32, w64, f"trilinear weights on the {scene} table")
    assert bool((w.cpu()[n_nbr == 0] == 0).all()) and bool(torch.isfinite(w).all())
    if scene != "clustered":                                         # on a top voxel: no probe beyond it finds anything
        top = KS.MAX_COORD // s * s
        on = pts[:len(c)]
        for axis, ks in ((0, [4, 5, 6, 7]), (1, [2, 3, 6, 7]), (2, [1, 3, 5, 7])):
            at = (on[:, axis] == top).nonzero()[:, 0]
            got = idx.cpu()[at]
            assert len(at) >= 5 and bool((got[:, ks] == -1).all()) and bool((got[:, 0] == at).all())


# ---- devoxelize -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 131])
@pytest.mark.parametrize("C", [16, 48, 64, 128])
def test_devoxelize_vs_float64(dev, C, N):
    n_rows = N + 5
    g = torch.Generator().manual_seed(7 * N + C)
    F = seeded_randn(n_rows, C, seed=3 * N + C)
    F[0] = float("nan")                                              # rows no entry names
    F[-1] = float("nan")
    idx = torch.randint(1, n_rows - 1, (N, 8), generator=g)
    idx = torch.where(torch.rand((N, 8), generator=g) < 0.6, idx, torch.full_like(idx, -1))
    w = torch.rand((N, 8), generator=g)
    w = w / w.sum(1, keepdim=True)
    add = seeded_randn(N, C, seed=N + C)
    raw = idx.clone()                                                # entries outside [0, n_rows): absent as well
    raw[0, 0], raw[N // 2, 7], raw[N - 1, 3] = n_rows, -5, n_rows + 7
    idx[0, 0] = idx[N // 2, 7] = idx[N - 1, 3] = -1
    Fd, wd, addd, rawd = F.to(dev), w.to(dev), add.to(dev), raw.to(torch.int32).to(dev)
    r32, r64 = PV.devoxelize(F, idx, w), PV.devoxelize(F.double(), idx, w.double())
    a32, a64 = r32 + add, r64 + add.double()
    what = f"devoxelize C={C} N={N}"
    plain = KV.devoxelize(Fd, rawd, wd)
    _check_rows(plain, r32, r64, what)
    assert torch.equal(plain, KV.devoxelize(Fd, idx.to(torch.int32).to(dev), wd))
    with_add = KV.devoxelize(Fd, rawd, wd, addend=addd)
    _check_rows(with_add, a32, a64, what + " + addend")
    inplace = addd.clone()
    assert KV.devoxelize(Fd, rawd, wd, addend=inplace, out=inplace) is inplace
    assert torch.equal(inplace, with_add)                            # the addend may be the output
    # F and out as column slices of wider buffers: the slack keeps its sentinel
    Fw = torch.full((n_rows, C + 8), float("nan"), device=dev)
    Fw[:, 4:4 + C] = Fd
    out = torch.full((N, C + 12), -7.25, device=dev)
    KV.devoxelize(Fw[:, 4:4 + C], rawd, wd, addend=addd, out=out[:, 8:8 + C])
    assert bool((out[:, :8] == -7.25).all()) and bool((out[:, 8 + C:] == -7.25).all())
    assert torch.equal(out[:, 8:8 + C], with_add)


# ---- voxelize ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 64, 128])
def test_voxelize_bits_and_float64(dev, C):
    """Voxels of 1, 2, 17 and 300 points and one of none, among others, the points in shuffled order and a few in no
    voxel: bit-equal to a float32 loop that adds F[p] / count in ascending point order, the same bits twice."""
    counts = [1, 2, 17, 300, 0, 3, 1, 64, 65, 1, 1, 5, 0, 2, 9, 1]
    g = torch.Generator().manual_seed(C)
    idx0 = torch.cat([torch.full((n,), v) for v, n in enumerate(counts)] + [torch.full((6,), -1)])
    idx0 = idx0[torch.randperm(len(idx0), generator=g)]
    N, V = len(idx0), len(counts)
    F = seeded_randn(N, C, seed=C + 1) * torch.exp(seeded_randn(N, 1, seed=C + 2))
    loop = torch.zeros((V, C))
    for p in range(N):
        v = int(idx0[p])
        if v >= 0:
            loop[v] = loop[v] + F[p] / torch.tensor(float(counts[v]))
    r64 = PV.voxelize(F.double(), idx0, V)
    perm, offsets = KV.voxel_order(idx0.to(torch.int32).to(dev), V)
    order = torch.sort(idx0, stable=True).indices
    assert torch.equal(perm.cpu().long(), order) and offsets.cpu().tolist() == np.cumsum([6] + counts).tolist()
    Fd = F.to(dev)
    got = KV.voxelize(Fd, perm, offsets)
    assert tuple(got.shape) == (V, C) and torch.equal(got.cpu(), loop)
    assert bool((got[4] == 0).all()) and bool((got[12] == 0).all())
    _check_rows(got, loop, r64, f"voxelize C={C}")
    assert torch.equal(KV.voxelize(Fd, perm, offsets), got)
    # rows of a wider buffer in, a column slice out
    Fw = torch.full((N, C + 4), float("nan"), device=dev)
    Fw[:, :C] = Fd
    out = torch.full((V, C + 8), -7.25, device=dev)
    KV.voxelize(Fw[:, :C], perm, offsets, out=out[:, 4:4 + C])
    assert bool((out[:, :4] == -7.25).all()) and bool((out[:, 4 + C:] == -7.25).all()) and torch.equal(out[:, 4:4 + C], got)


# ---- the network ------------------------------------------------------------------------------------------------------
def _cloud(seed, n=2000, lo=1.0, hi=3.2, scale=0.25):
    """About 1 500 voxels: a shell of a synthetic sweep, shrunk so that voxels have neighbours (test_spconv's `_cloud`)."""
    p = synth_points(20000, seed)[:, :3]
    d = np.linalg.norm(p, axis=1)
    return (p[(d > lo) & (d < hi)][:n] * np.float32(scale)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _state(seed):
    from lidargen.metrics.models.spvcnn.model import Model

    return PV.seeded_state(Model(O.CONFIG), seed)


def _model(dev, seed):
    from lidargen.metrics.models.spvcnn.model import Model

    m = Model(O.CONFIG)
    m.load_state_dict(_state(seed))
    return m.eval().to(dev)


@functools.lru_cache(maxsize=None)
def _net_case(weights_seed, cloud_seeds):
    """(feats, coords, logits float32 mode, logits float64) of the oracle, computed once."""
    feats, coords = O.collate([O.pcd2voxel(_cloud(s)) for s in cloud_seeds])
    sd = _state(weights_seed)
    return feats, coords, PV.network(sd, feats, coords, torch.float32), PV.network(sd, feats, coords, torch.float64)


def test_network_vs_float64(dev):
    feats, coords, ref32, ref64 = _net_case(1, (11, 12))
    assert 2400 < len(coords) < 4000
    assert float(_state(1)["point_transforms.0.0.bias"].abs().min()) > 1e-4      # the Linear biases are away from zero
    m = _model(dev, 1)
    out = m(feats.to(dev), coords.to(torch.int32).to(dev))
    assert out["logits"].shape == (len(coords), 48) and out["logits"].dtype == torch.float32
    assert torch.equal(out["coords"].cpu(), PV.point_coords(coords)[:, :3])
    assert out["batch_indices"].dtype == torch.int64 and torch.equal(out["batch_indices"].cpu(), coords[:, 3])
    assert float(ref64.abs().max()) > 1e-3 and float((ref64 == 0).double().mean()) < 0.9     # a live output
    _check_rows(out["logits"], ref32, ref64, "SPVCNN logits")
    deep = m(feats.to(dev), coords.to(torch.int32).to(dev), return_logits=True)
    sd = _state(1)
    d32, lv4 = PV.network(sd, feats, coords, torch.float32, deep=True)
    d64, _ = PV.network(sd, feats, coords, torch.float64, deep=True)
    assert deep["logits"].shape == (len(lv4), 128) and torch.equal(deep["batch_indices"].cpu().long(), lv4[:, 3])
    _check_rows(deep["logits"], d32, d64, "SPVCNN bottleneck after the second exchange")


def test_batch_independence_through_the_network(dev):
    """Cloud A alone and as the middle one of three: the same bits in every row, twice."""
    m = _model(dev, 1)
    items = [O.pcd2voxel(_cloud(s)) for s in (21, 11, 22)]
    fa, ca = O.collate(items[1:2])
    f3, c3 = O.collate(items)
    ya = m(fa.to(dev), ca.to(torch.int32).to(dev))["logits"]
    y3 = m(f3.to(dev), c3.to(torch.int32).to(dev))["logits"]
    lo = len(items[0][1])
    assert torch.equal(y3[lo:lo + len(ca)], ya)
    assert torch.equal(m(f3.to(dev), c3.to(torch.int32).to(dev))["logits"], y3)


def test_call_sequence_tables_orders_and_weights_belong_to_their_call(dev):
    """A second cloud with the SAME number of points at other places must get its own tables, point orders and trilinear
    weights; load_state_dict between calls folds the transforms again; nothing of an earlier call stays."""
    feats, coords, ref32, ref64 = _net_case(1, (11,))
    mirrored = coords.clone()
    mirrored[:, 0] = coords[:, 0].max() - coords[:, 0]               # the same count, other neighbours
    sd = _state(1)
    m = _model(dev, 1)
    run = lambda c: m(feats.to(dev), c.to(torch.int32).to(dev))["logits"]
    first = run(coords)
    _check_rows(first, ref32, ref64, "first cloud")
    r32, r64 = PV.network(sd, feats, mirrored, torch.float32), PV.network(sd, feats, mirrored, torch.float64)
    assert float(O.rel_l2_rows(r64, ref64).median()) > 1e-3           # the other places are visible at all
    _check_rows(run(mirrored), r32, r64, "same point count, other coordinates")
    m.load_state_dict(_state(2))
    _, _, s32, s64 = _net_case(2, (11,))
    assert float(O.rel_l2_rows(s64, ref64).median()) > 1e-3
    _check_rows(run(coords), s32, s64, "after load_state_dict")
    with torch.no_grad():
        m.point_transforms[2][0].bias.add_(0.3)
    sd2 = dict(_state(2))
    sd2["point_transforms.2.0.bias"] = sd2["point_transforms.2.0.bias"] + 0.3
    e32, e64 = PV.network(sd2, feats, coords, torch.float32), PV.network(sd2, feats, coords, torch.float64)
    assert float(O.rel_l2_rows(e64, s64).median()) > 1e-3
    _check_rows(run(coords), e32, e64, "after an in-place edit of a Linear bias")
    m.load_state_dict(_state(1))
    assert torch.equal(run(coords), first)


# ---- compute_point_voxel_logits, compute_fpvd -------------------------------------------------------------------------
def _metre_cloud(seed, n=600, hi=14.0):
    """A sweep cropped to 14 m: nothing beyond, so its far depth sectors are empty (test_spconv's `_metre_cloud`)."""
    p = synth_points(8000, seed)[:, :3]
    d = np.linalg.norm(p, axis=1)
    return p[(d > 1.0) & (d < hi)][:n]


def _edge_clearance(clouds):
    """The smallest distance in metres of any row's depth from a sector edge, by the oracle's depths."""
    edges = O.sector_edges(DEPTH_RANGE)
    gap = float("inf")
    for c in clouds:
        _, vc = O.pcd2voxel(O.preprocess_pcd(c, DEPTH_RANGE))
        vc = vc.float()
        d = torch.norm(vc - vc.mean(0), dim=-1) * O.VOXEL_SIZE
        gap = min(gap, float((d[:, None] - edges[None]).abs().min()))
    return gap


def _oracle_features(sd, clouds, dtype):
    items = [O.pcd2voxel(O.preprocess_pcd(c, DEPTH_RANGE)) for c in clouds]
    feats, coords = O.collate(items)
    return O.sector_means(PV.network(sd, feats, coords, dtype), coords, DEPTH_RANGE, len(clouds))


def test_compute_point_voxel_logits(dev):
    from lidargen.metrics import metric_utils as MU

    clouds = [_metre_cloud(31), _metre_cloud(32, n=450), _metre_cloud(33, hi=40.0)]
    assert _edge_clearance(clouds) > 1e-3         # the integer and the float coordinate decide every row's sector alike
    sd = _state(1)
    ref32, ref64 = _oracle_features(sd, clouds, torch.float32), _oracle_features(sd, clouds, torch.float64)
    (got,) = MU.compute_point_voxel_logits("32", clouds, model=_model(dev, 1))
    assert got.shape == (3, 768) and got.dtype == np.float32
    got = torch.from_numpy(got)
    empty = ref64.reshape(3, 16, 48).abs().sum(2) == 0
    assert bool(empty[0, 6:].all()) and not bool(empty[0, :3].any()) and not bool(empty[2, :12].any())
    assert bool((got.reshape(3, 16, 48)[empty] == 0).all())          # an empty sector is exact zeros
    _check_rows(got, ref32, ref64, "depth-sector features of the SPVCNN")
    two, one = MU.compute_point_voxel_logits("32", clouds[:2], clouds[2:], model=_model(dev, 1))
    assert torch.equal(torch.from_numpy(np.concatenate([two, one])), got)


def test_compute_fpvd_vs_float64_features(dev, capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils

    real = [_metre_cloud(40 + i, n=300) for i in range(6)]
    fake = [_metre_cloud(60 + i, n=300) * np.float32(0.8) for i in range(6)]
    assert _edge_clearance(real + fake) > 1e-3
    sd = _state(1)
    f64 = [_oracle_features(sd, s, torch.float64).numpy() for s in (real, fake)]
    f32 = [_oracle_features(sd, s, torch.float32).numpy() for s in (real, fake)]
    want, want32 = O.compute_fd(*f64), O.compute_fd(*f32)
    limit = 4.0 * abs(want32 - want) / abs(want)
    m = _model(dev, 1)
    score = eval_utils.compute_fpvd(real, fake, "32", model=m)
    out = capsys.readouterr().out
    rel = abs(score - want) / abs(want)
    print(f"FPVD {score!r} against {want!r}: relative {rel:.2e}; float32 oracle {limit / 4:.2e}; limit {limit:.2e}")
    assert "Evaluating (FPVD) ..." in out and OUTPUT_TEMPLATE.format("FPVD", score) in out
    assert rel < limit
    same = eval_utils.compute_fpvd(real, real, "32", model=m)
    assert abs(same) < 1e-6 * float(np.trace(np.cov(f64[0], rowvar=False)))
