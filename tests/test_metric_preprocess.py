"""GPU tests of the batched device front-end of FRID / FSVD / FPVD (csrc/metric_preprocess.hip, lidarcrafter_amd/
ops_metric_pre.py, metric_utils.preprocess_range_batch / pcd2voxel_batch, the `preprocess_device='cuda'` keyword; DESIGN.md
section 5u).  Everything is compared BIT FOR BIT with the host route (preprocess_range, preprocess_pcd + pcd2voxel +
sparse_collate), never with the code under test.  The one tolerance of the file is the rule of tests/
_metric_preprocess_cases.py that drops, before both routes run, the points within 1e-6 px of a pixel boundary (two correctly
working double-precision atan2 / asin differ by about 1e-12 px); it may drop at most 1e-4 of the points, which is asserted."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metric_preprocess_cases as cases  # noqa: E402
import _rangenet_oracle as RO  # noqa: E402
import _spconv_oracle as SO  # noqa: E402
import _spvcnn_oracle as PV  # noqa: E402

from lidarcrafter_amd import ops_metric_pre as KP  # noqa: E402
from lidarcrafter_amd.testing import seeded_fill_rangenet  # noqa: E402
from lidargen.metrics import metric_utils as MU  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _host_range(clouds, cfg):
    """The tensor compute_range_logits builds on the host, of the clouds widened to float64 (the device route's contract;
    for float64 clouds the host route itself)."""
    return torch.from_numpy(np.stack([MU.preprocess_range(np.asarray(c, np.float64), **cfg) for c in clouds])).float()


def _same_bits(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.shape)
    diff = got.view(torch.int32) != want.view(torch.int32) if got.dtype == torch.float32 else got != want
    assert not bool(diff.any()), (what, int(diff.sum()), diff.nonzero()[:5].tolist())


# ---- the range route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_key,nclouds,dtype", cases.RANGE_CASES)
def test_range_images_equal_the_host_route(dev, size_key, nclouds, dtype):
    """float64 clouds: the host route; float32 clouds: the host route on the widened cloud.  All four channels."""
    cfg = cases.CFG[size_key]
    clouds, total, _ = cases.range_batch(size_key, nclouds, dtype)
    share = sum(cases.range_batch(*c)[2] for c in cases.RANGE_CASES) / sum(cases.range_batch(*c)[1] for c in cases.RANGE_CASES)
    print(f"[metric_preprocess] dropped share of the range inputs {share:.2e}")
    assert share <= cases.DROP_CAP
    assert all(c.dtype == np.dtype(dtype) for c in clouds)
    got = MU.preprocess_range_batch(clouds, dev, **cfg)
    assert got.is_cuda and got.dtype == torch.float32
    want = _host_range(clouds, cfg)
    assert int((want[:, 0] > 0).sum()) > 0 and int((want[:, 1:] != -1).sum()) > 0          # (the case shows something)
    _same_bits(got, want, (size_key, nclouds, dtype))
    if dtype == "float64":                                                               # the host route as it stands
        as_is = torch.from_numpy(np.stack([MU.preprocess_range(c, **cfg) for c in clouds])).float()
        assert torch.equal(as_is, want)


def _placed(dtype):
    """Clouds of placed points for the 4x16 image, one list per purpose."""
    cfg = cases.CFG["4x16"]
    t = np.dtype(dtype).type
    seam = np.array([[-5.0, 0.0, 0.5], [-7.0, -0.0, 0.5],                 # yaw = -pi: column 0; yaw = +pi: column W -> W - 1
                     [3.0, 4.0, 30.0], [3.0, -4.0, -30.0],               # above fov_up: row 0; below fov_down: row H - 1
                     [0.0, 0.0, 9.0], [0.0, 0.0, -11.0]], dtype=t)       # z / depth = +1 and -1
    lo, hi = t(cases.DEPTH_RANGE[0]), t(cases.DEPTH_RANGE[1])
    # the first mask compares the depth in the cloud's dtype widened: on the bound (out), one ulp either side of it
    probes = [lo, np.nextafter(lo, t(2)), np.nextafter(lo, t(0)), hi, np.nextafter(hi, t(0)), np.nextafter(hi, t(100))]
    if t is np.float64:
        # the second mask is range2xyz's on the float32 image: depths inside the first mask that ROUND onto a bound in
        # float32 (a depth and no back-projection), and one float32 ulp inside the bounds (both)
        probes += [1.0 + 1e-9, 45.0 - 1e-9, float(np.nextafter(np.float32(1), np.float32(2))),
                   float(np.nextafter(np.float32(45), np.float32(0)))]
    bounds = [np.array([[d, 0.0, 0.0]], dtype=t) for d in probes]        # depth = sqrt(d^2) = d exactly; one cloud each
    ray = cases.ray(cfg, 2, 5)
    g = np.random.default_rng(5)
    distinct = (ray[None] * g.permutation(np.linspace(5.0, 30.0, 500))[:, None]).astype(t)
    same = np.repeat((ray * 12.5).astype(t)[None], 250, 0)
    jitter = np.stack([(cases.ray(cfg, 2, 5, (0.3 + 0.4 * a, 0.3 + 0.4 * b)) * 12.5).astype(t) for a, b in g.uniform(0, 1, (250, 2))])
    pile = np.concatenate([same, jitter])[g.permutation(500)]
    a, b = (cases.ray(cfg, 1, 3) * 8.0).astype(t), (cases.ray(cfg, 3, 12) * 20.0).astype(t)
    leak = [a[None], b[None], a[None]]
    return cfg, seam, bounds, distinct, pile, leak


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_placed_points(dev, dtype):
    cfg, seam, bounds, distinct, pile, leak = _placed(dtype)
    H, W = cfg["size"]
    for what, clouds in (("seam, row clamps, poles", [seam]), ("both masks at both bounds", bounds),
                         ("500 distinct depths in one pixel", [distinct]), ("500 nearly equal depths in one pixel", [pile]),
                         ("a pixel of cloud b alone", leak)):
        want = _host_range(clouds, cfg)
        got = MU.preprocess_range_batch(clouds, dev, **cfg)
        _same_bits(got, want, what)
    want = _host_range([seam], cfg)[0, 0]
    assert want[:, 0].max() > 0 and want[:, W - 1].max() > 0 and want[0].max() > 0 and want[H - 1].max() > 0
    d = _host_range(bounds, cfg)
    seen = (d[:, 0] > 0).flatten(1).any(1).tolist()
    assert seen[:6] == [False, True, False, False, True, False]                       # the first mask, pinned by the host
    if dtype == "float64":
        shown = (d[:, 1:] != -1).flatten(1).any(1).tolist()
        assert seen[6:] == [True] * 4 and shown[6:] == [False, False, True, True]      # the second mask
    one = _host_range([distinct], cfg)[0, 0]
    assert int((one > 0).sum()) == 1 and float(one.max()) == float(np.float32(np.linalg.norm(distinct.astype(np.float64), axis=1).min()))
    lk = MU.preprocess_range_batch(leak, dev, **cfg).cpu()
    assert lk[0, 0, 1, 3] > 0 and lk[1, 0, 1, 3] == -1 and lk[2, 0, 1, 3] > 0 and lk[1, 0, 3, 12] > 0 and lk[0, 0, 3, 12] == -1


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_range_alone_and_at_any_position(dev, dtype):
    cfg = cases.CFG["32x1024"]
    clouds, _, _ = cases.range_batch("32x1024", 5, dtype)
    probe = cases.range_batch("32x1024", 1, dtype)[0][0]
    alone = MU.preprocess_range_batch([probe], dev, **cfg)
    for pos in (0, 2, 5):
        batch = clouds[:pos] + [probe] + clouds[pos:]
        got = MU.preprocess_range_batch(batch, dev, **cfg)
        assert torch.equal(got[pos:pos + 1].view(torch.int32), alone.view(torch.int32)), pos
    again = MU.preprocess_range_batch(clouds, dev, **cfg)
    assert torch.equal(again.view(torch.int32), MU.preprocess_range_batch(clouds, dev, **cfg).view(torch.int32))   # run to run


def test_range_cuda_tensors_in(dev):
    """CUDA tensors are concatenated on the device: the same bits as the numpy clouds."""
    cfg = cases.CFG["4x16"]
    clouds, _, _ = cases.range_batch("4x16", 3, "float64")
    got = MU.preprocess_range_batch([torch.from_numpy(c).to(dev) for c in clouds], dev, **cfg)
    _same_bits(got, _host_range(clouds, cfg), "cuda tensors")


def test_direction_table_call_sequence(dev):
    """The table outlives a call: sizes and fovs alternate A, B, A; A's second result is its first, and no third table is
    built.  The host-side table is range2xyz of an all-ones image."""
    A = dict(cases.CFG["4x16"])
    B = {"size": [32, 1024], "fov": [3, -25], "depth_range": [1.0, 45.0]}
    for cfg in (A, B):
        H, W = cfg["size"]
        table = KP.ray_directions_host(H, W, cfg["fov"])
        ones = MU.range2xyz(np.ones((H, W), np.float32), log_scale=False, fov=cfg["fov"], depth_range=[0.0, 2.0])
        assert table.dtype == np.float64 and np.array_equal(table, ones)
    ca = cases.range_batch("4x16", 3, "float64")[0]
    cb = [cases.drop_near_boundaries(cases.sweep(900 + k, n, np.float64), B)[0] for k, n in enumerate((64, 0, 700))]
    first = MU.preprocess_range_batch(ca, dev, **A)
    built = KP.DIRS_BUILT
    second = MU.preprocess_range_batch(cb, dev, **B)
    third = MU.preprocess_range_batch(ca, dev, **A)
    assert KP.DIRS_BUILT <= built + 1
    assert torch.equal(first.view(torch.int32), third.view(torch.int32))
    _same_bits(first, _host_range(ca, A), "A")
    _same_bits(second, _host_range(cb, B), "B")
    assert torch.equal(KP.ray_directions(4, 16, A["fov"], dev).cpu(), torch.from_numpy(KP.ray_directions_host(4, 16, A["fov"])))


def test_compute_range_logits_on_the_device_route(dev):
    """Equal inputs, and the network's bits do not depend on the batch: the host route's rows bit for bit."""
    from lidargen.metrics.models.rangenet.model import Model

    m = seeded_fill_rangenet(Model(RO.config(21)), 1).eval().requires_grad_(False).to(dev)
    cfg = dict(cases.CFG["4x16"], size=[16, 64])
    clouds = [cases.drop_near_boundaries(c, cfg)[0] for c in
              [cases.sweep(950 + k, n, np.float64) for k, n in enumerate((300, 0, 65, 1, 700))] + [RO.metre_cloud(71).astype(np.float64)]]
    (host,) = MU.compute_range_logits("32", clouds, model=m, size=(16, 64))
    (got,) = MU.compute_range_logits("32", clouds, model=m, size=(16, 64), preprocess_device="cuda")
    assert got.shape == (6, 512) and got.dtype == np.float32 and float(np.abs(host).max()) > 0
    assert np.array_equal(got.view(np.int32), host.view(np.int32))


# ---- the voxel route ----------------------------------------------------------------------------------------------------
def _host_voxels(clouds):
    return MU.sparse_collate([MU.pcd2voxel(MU.preprocess_pcd(c, depth_range=cases.DEPTH_RANGE)) for c in clouds])


def _same_triple(got, want, what):
    for name, g, w in zip(("feats", "coords", "offsets"), got, want):
        _same_bits(g, w.cpu(), (what, name))


@pytest.mark.parametrize("nclouds,dtype", cases.VOXEL_CASES)
def test_voxels_equal_the_host_route(dev, nclouds, dtype):
    clouds = cases.voxel_batch(nclouds, dtype)
    want = _host_voxels(clouds)
    got = MU.pcd2voxel_batch(clouds, dev, depth_range=cases.DEPTH_RANGE)
    assert all(t.is_cuda for t in got) and want[0].shape[0] > 0
    _same_triple(got, want, (nclouds, dtype))
    if nclouds == 3:
        assert want[0].shape[0] < sum(c.shape[0] for c in clouds) // 4            # many points per voxel
        assert int(want[2][1]) == int(want[2][2])                                  # the empty cloud inside the batch
    if nclouds == 5:
        assert int(want[2][2]) == int(want[2][3]) and clouds[2].shape[0] > 0       # the cloud the filter empties
        kept = MU.preprocess_pcd(clouds[0], depth_range=cases.DEPTH_RANGE)
        assert 0 < kept.shape[0] < clouds[0].shape[0] - 6                          # the bounds cut on both sides


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_voxels_of_cuda_tensors_equal_the_per_cloud_cuda_route(dev, dtype):
    clouds = [cases.dyadic_sweep(41, 2000, dtype), np.zeros((0, 3), dtype), cases.dyadic_sweep(42, 65, dtype),
              (cases.dyadic_sweep(43, 64, dtype) / 64).astype(dtype)]
    on_dev = [torch.from_numpy(c).to(dev) for c in clouds]
    want = MU.sparse_collate([MU.pcd2voxel(MU.preprocess_pcd(c, depth_range=cases.DEPTH_RANGE)) for c in on_dev])
    got = MU.pcd2voxel_batch(on_dev, dev, depth_range=cases.DEPTH_RANGE)
    _same_triple(got, want, ("cuda", dtype))
    _same_triple(got, _host_voxels(clouds), ("cuda against the host", dtype))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_voxels_alone_and_at_any_position(dev, dtype):
    clouds = cases.voxel_batch(5, dtype)
    probe = cases.voxel_batch(3, dtype)[0]
    f0, c0, o0 = MU.pcd2voxel_batch([probe], dev, depth_range=cases.DEPTH_RANGE)
    for pos in (0, 2, 5):
        f, c, o = MU.pcd2voxel_batch(clouds[:pos] + [probe] + clouds[pos:], dev, depth_range=cases.DEPTH_RANGE)
        a, b = int(o[pos]), int(o[pos + 1])
        assert b - a == int(o0[1]) and torch.equal(f[a:b].view(torch.int32), f0.view(torch.int32)), pos
        assert torch.equal(c[a:b, :3], c0[:, :3]) and bool((c[a:b, 3] == pos).all()), pos
    one, two = (MU.pcd2voxel_batch(clouds, dev, depth_range=cases.DEPTH_RANGE) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(one, two))                        # run to run


def _metre_clouds():
    from lidarcrafter_amd.testing import synth_points

    out = []
    for seed, n, hi in ((31, 600, 14.0), (32, 450, 14.0), (33, 600, 40.0)):
        p = synth_points(8000, seed)[:, :3]
        d = np.linalg.norm(p, axis=1)
        out.append(p[(d > 1.0) & (d < hi)][:n])
    return out


@functools.lru_cache(maxsize=None)
def _sparse_model(kind):
    if kind == "voxel":
        from lidargen.metrics.models.minkowskinet.model import Model
        m = Model(SO.CONFIG)
        m.load_state_dict(SO.seeded_state(Model(SO.CONFIG), 1))
    else:
        from lidargen.metrics.models.spvcnn.model import Model
        m = Model(SO.CONFIG)
        m.load_state_dict(PV.seeded_state(Model(SO.CONFIG), 1))
    return m.eval().to("cuda:0")


def test_compute_logits_on_the_device_route(dev):
    clouds = _metre_clouds()
    m = _sparse_model("voxel")
    (host,) = MU.compute_logits("32", "voxel", clouds, model=m)
    (got,) = MU.compute_logits("32", "voxel", clouds, model=m, preprocess_device="cuda")
    assert got.shape == host.shape == (3, 768) and float(np.abs(host).max()) > 0
    assert np.array_equal(got.view(np.int32), host.view(np.int32))


def test_compute_point_voxel_logits_on_the_device_route(dev):
    clouds = _metre_clouds()
    m = _sparse_model("point_voxel")
    (host,) = MU.compute_point_voxel_logits("32", clouds, model=m)
    (got,) = MU.compute_point_voxel_logits("32", clouds, model=m, preprocess_device="cuda")
    assert got.shape == host.shape == (3, 768) and float(np.abs(host).max()) > 0
    assert np.array_equal(got.view(np.int32), host.view(np.int32))
