"""GPU tests of the PointMLP kernels (csrc/pointmlp.hip), of the network under the reference's module tree and of the object
front-end, against the CPU oracle of tests/_pointmlp_oracle.py and the reference's recorded run (tests/golden/pointmlp.npz).

Index kernels: equality with the restatement.  Grouping and dense layers: per-sample relative L2 below TOL_CONV against
float64.  Whole network: 3 x the reference float32 module's own error on that cloud, read from the fixture.  Outputs sit
between guard bands, scratch starts as NaN."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointmlp_oracle as O  # noqa: E402
from test_pointmlp_host import CASES, fixture_tables, make, oracle64  # noqa: E402

from lidarcrafter_amd import ops_pointmlp as KM  # noqa: E402
from lidarcrafter_amd._lib import HipError  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = O.TOL_CONV
GUARD = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def guarded(dev, shape, dtype, fill):
    """(view of `shape`, check): the view lies between two guard bands that check() finds untouched."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device=dev, dtype=dtype)

    def check():
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), "a write outside the output"

    return buf[GUARD:GUARD + n].view(shape), check


# ---- farthest point sampling -------------------------------------------------------------------------------------------
def _fps_clouds(N):
    """[B,N,3]: uniform, zero-padded, all-equal, a far point last, fewer distinct points than picks."""
    c = O.clouds(5, N, 1000 + N, real=[N, max(1, N // 3), N, N, N])
    c[2] = c[2, 0]
    c[3] = 0.25 * c[3]
    c[3, -1] = (50.0, -40.0, 30.0)
    c[4] = c[4, np.arange(N) % 3]
    return c


_FPS_WANT = {}


def _fps_case(N, M):
    if (N, M) not in _FPS_WANT:
        c = _fps_clouds(N)
        _FPS_WANT[N, M] = (c, O.fps_batch(c, M))
    return _FPS_WANT[N, M]


@pytest.mark.parametrize("N,M", [(1, 1), (2, 2), (63, 32), (64, 64), (65, 33), (1000, 512), (1024, 512), (1025, 7), (2500, 64)])
def test_fps_equals_the_restatement(dev, N, M):
    """N = 1000: bs = 512 < N, the tie key's k / bs part decides; 1024: four points per thread; 2500: the strided case."""
    c, want = _fps_case(N, M)
    out, check = guarded(dev, (c.shape[0], M), torch.int32, -7)
    got = KM.fps(torch.from_numpy(c).to(dev), M, out=out)
    check()
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want), (N, M)
    if M > 3:
        assert want[2].tolist() == [0] * M and want[4][3:].tolist() == [0] * (M - 3)        # index 0 repeats
    if N > 1 and M > 1:
        assert want[3][1] == N - 1                                                          # the far point is the first pick
    alone = KM.fps(torch.from_numpy(c[1:2].copy()).to(dev), M)                              # a cloud alone: the same bits
    assert torch.equal(alone, got[1:2])


def test_fps_above_lds_and_refusals(dev):
    N = KM.limit("fps_max_n")
    assert N >= 8192
    c = O.clouds(1, N, 77, real=[N - 1000])
    assert np.array_equal(KM.fps(torch.from_numpy(c).to(dev), 6).cpu().numpy(), O.fps_batch(c, 6))
    mid = O.clouds(1, 4097, 78)
    assert np.array_equal(KM.fps(torch.from_numpy(mid).to(dev), 5).cpu().numpy(), O.fps_batch(mid, 5))
    with pytest.raises(HipError, match="unsupported shape"):
        KM.fps(torch.zeros(1, N + 1, 3, device=dev), 4)
    with pytest.raises(ValueError, match="npoint"):
        KM.fps(torch.zeros(1, 8, 3, device=dev), 0)
    with pytest.raises(RuntimeError, match="CUDA"):
        KM.fps(torch.zeros(1, 8, 3), 4)


# ---- k nearest neighbours ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,K", [(24, 5, 24), (25, 5, 24), (63, 7, 1), (64, 9, 24), (65, 1, 32), (1024, 33, 24), (1024, 4, 32),
                                   (1025, 3, 24), (3, 3, 1)])
def test_knn_equals_the_restatement(dev, N, S, K):
    """N = K, K + 1, 63 / 64 / 65, 1024 (registers) and 1025 (streamed); S = 1; K = 1 / 24 / 32; duplicated and padded points."""
    c = O.clouds(3, N, 2000 + N + K, real=[N, max(1, N // 3), N])
    c[2] = c[2, np.arange(N) % max(1, N // 2)]                                              # every point twice
    q = np.stack([np.random.default_rng(b).permutation(N)[np.arange(S) % N] for b in range(3)]).astype(np.int32)
    out, check = guarded(dev, (3, S, K), torch.int32, -7)
    got = KM.knn(torch.from_numpy(c).to(dev), torch.from_numpy(q).to(dev), K, out=out)
    check()
    assert np.array_equal(got.cpu().numpy(), O.knn_batch(c, q, K)), (N, S, K)
    alone = KM.knn(torch.from_numpy(c[1:2].copy()).to(dev), torch.from_numpy(q[1:2].copy()).to(dev), K)
    assert torch.equal(alone, got[1:2])


def test_knn_refusals(dev):
    xyz = torch.zeros(1, 8, 3, device=dev)
    q = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    with pytest.raises(HipError, match="invalid argument"):
        KM.knn(xyz, q, 9)                                                                    # N < K
    with pytest.raises(HipError, match="unsupported shape"):
        KM.knn(torch.zeros(1, 40, 3, device=dev), q, 33)
    with pytest.raises(TypeError, match="int32"):
        KM.knn(xyz, q.long(), 2)
    bad = torch.tensor([[8, -1]], dtype=torch.int32, device=dev)                            # outside the cloud: a row of -1
    assert KM.knn(xyz, bad, 3).cpu().tolist() == [[[-1] * 3] * 2]


# ---- grouping ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,S,K", [(16, 64, 32, 5), (64, 300, 150, 24), (17, 40, 7, 3)])
def test_group_against_float64(dev, d, N, S, K):
    """S K = 160, 3600, 21: none a multiple of the 256-column block; d = 17: a partial channel block."""
    B = 3
    c = O.clouds(B, N, 3000 + d)
    (f, k), = O.geometry(c, [S], [K])
    g = torch.Generator().manual_seed(d)
    x = torch.randn(B, d, N, generator=g) + 0.5
    al, be = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    want, std = O.group(x.double(), f, k, al.double(), be.double())
    out, check = guarded(dev, (B, 2 * d, S * K), torch.float32, -7.5)
    scratch = torch.full((KM.group_scratch_elems(B, S, K),), float("nan"), device=dev, dtype=torch.float64)
    sigma = torch.full((B,), float("nan"), device=dev)
    args = (x.to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(k).to(dev), al.to(dev), be.to(dev))
    got = KM.group(*args, out=out, scratch=scratch, sigma=sigma)
    check()
    errs = O.rel_l2_per_sample(got, want)
    serr = float(((sigma.cpu().double() - std) / std).abs().max())
    print(f"d {d} S K {S * K}: worst sample {max(errs):.2e}, sigma {serr:.2e}")
    assert max(errs) < TOL and serr < 2e-7 and not bool((out == -7.5).any())
    assert torch.equal(KM.group(*args), got)
    alone = KM.group(*[a[1:2].contiguous() if a.dim() > 1 else a for a in args])
    assert torch.equal(alone, got[1:2])


def test_group_zero_deviation_is_finite(dev):
    """Every neighbour equals its anchor: sigma = 0, the result is beta through the + 1e-5."""
    B, d, N, S, K = 2, 16, 32, 8, 4
    x = torch.randn(B, d, N)
    f = torch.arange(S, dtype=torch.int32).repeat(B, 1)
    k = f[:, :, None].repeat(1, 1, K).contiguous()
    al, be = torch.full((d,), 2.0), torch.arange(d, dtype=torch.float32)
    sigma = torch.empty(B, device=dev)
    got = KM.group(x.to(dev), f.to(dev), k.to(dev), al.to(dev), be.to(dev), sigma=sigma).cpu()
    assert bool(torch.isfinite(got).all()) and sigma.cpu().tolist() == [0.0, 0.0]
    assert torch.equal(got[:, :d], be[None, :, None].expand(B, d, S * K))
    assert torch.equal(got[:, d:], x[:, :, :S].repeat_interleave(K, dim=2))


# ---- dense layers ------------------------------------------------------------------------------------------------------
def _dense_case(B, Ci, Co, L, seed, res):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, L, generator=g)
    w = torch.randn(Co, Ci, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g)
    r = torch.randn(B, Co, L, generator=g) if res else None
    return x, w, b, r


def _assert_dense(dev, B, Ci, Co, L, seed, act, res):
    x, w, b, r = _dense_case(B, Ci, Co, L, seed, res)
    out, check = guarded(dev, (B, Co, L), torch.float32, -7.5)
    got = KM.conv(x.to(dev), KM.pack_weight(w).to(dev), b.to(dev), Co, act, res=None if r is None else r.to(dev), out=out)
    check()
    want = O.dense(x.double(), w.double(), b.double(), act, None if r is None else r.double())
    errs = O.rel_l2_per_sample(got, want)
    assert max(errs) < TOL, (B, Ci, Co, L, act, res, errs)
    assert not bool((out == -7.5).any())
    return max(errs)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("Ci,Co", [(16, 16), (32, 48), (48, 32), (16, 1024), (1024, 16), (3, 64), (33, 65)])
def test_conv_widths_and_lengths(dev, Ci, Co, res):
    """Ci / Co among 16, 32, 48, 1024 (and 3, 33, 65: partial chunks and channel blocks) at L = 1, 31, 32, 33 and at one
    column past the layer's block."""
    worst = 0.0
    for i, L in enumerate((1, 31, 32, 33, KM.conv_block_cols(Co) + 1)):
        worst = max(worst, _assert_dense(dev, 2, Ci, Co, L, 100 * Ci + Co + i, i % 2 == 0, res))
    print(f"{Ci} -> {Co} residual {res}: worst sample {worst:.2e}")


def test_conv_deepest_layer(dev):
    print(f"1024 -> 1024, L = 70: worst sample {_assert_dense(dev, 2, 1024, 1024, 70, 5, True, True):.2e}")


def test_conv_residual_is_added_before_the_activation(dev):
    x, w, b, r = _dense_case(1, 8, 8, 5, 9, True)
    r = r - 3.0
    got = KM.conv(x.to(dev), KM.pack_weight(w).to(dev), b.to(dev), 8, True, res=r.to(dev)).cpu()
    assert float(got.min()) == 0.0 and max(O.rel_l2_per_sample(got, O.dense(x.double(), w.double(), b.double(), True, r.double()))) < TOL


def test_conv_bits_and_aliasing(dev):
    x, w, b, r = _dense_case(4, 48, 80, 70, 11, True)
    args = (KM.pack_weight(w).to(dev), b.to(dev), 80, True)
    full = KM.conv(x.to(dev), *args, res=r.to(dev))
    assert torch.equal(full, KM.conv(x.to(dev), *args, res=r.to(dev)))
    assert torch.equal(full[2:3], KM.conv(x[2:3].contiguous().to(dev), *args, res=r[2:3].contiguous().to(dev)))
    sq = torch.randn(1, 80, 9, device=dev)
    w2 = KM.pack_weight(torch.randn(80, 80)).to(dev)
    with pytest.raises(HipError, match="invalid argument"):
        KM.conv(sq, w2, b.to(dev), 80, True, out=sq)                                         # y aliasing x
    with pytest.raises(HipError, match="invalid argument"):
        KM.conv(torch.randn(1, 80, 9, device=dev), w2, b.to(dev), 80, True, res=sq, out=sq)   # y aliasing res
    with pytest.raises(ValueError, match="packs to"):
        KM.conv(sq, w2[:-4], b.to(dev), 80, True)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("Ci,Co", [(3, 20), (33, 65), (64, 32)])
def test_conv_bits_equal_rangenet_1x1(dev, Ci, Co, res):
    """The pointwise layer and RangeNet's 1x1 mode are two geometries of one engine (csrc/dense_f32.h): the same packed
    weights, the same chunks, the same k order; without an activation the epilogues are the same arithmetic (+ bias, + one
    addend).  So the bits are equal, whatever the tile: L = 1, 33, 257 as one image row, and L = 66 as two rows of 33."""
    from lidarcrafter_amd import ops_rangenet as KR

    for i, (L, H) in enumerate(((1, 1), (33, 1), (257, 1), (66, 2))):
        x, w, b, r = _dense_case(2, Ci, Co, L, 7 * Ci + Co + i, res)
        x, b, r = x.to(dev), b.to(dev), None if r is None else r.to(dev)
        got = KM.conv(x, KM.pack_weight(w).to(dev), b, Co, False, res=r)
        want = KR.conv(x.view(2, Ci, H, L // H), KR.pack_weight(w[:, :, None, None].contiguous(), 0).to(dev), b, 0, Co, False,
                       res1=None if r is None else r.view(2, Co, H, L // H))
        assert torch.equal(got, want.view(2, Co, L)), (Ci, Co, L, H, res)


@pytest.mark.parametrize("C,G,K", [(7, 5, 24), (33, 11, 24), (4, 1, 64), (3, 300, 4)])
def test_groupmax(dev, C, G, K):
    """G K = 120, 264, 64, 1200: the last group ends inside a dense tile; G = 1: the global pool."""
    t = torch.randn(3, C, G * K, generator=torch.Generator().manual_seed(C))
    out, check = guarded(dev, (3, C, G), torch.float32, -7.5)
    got = KM.groupmax(t.to(dev), K, out=out)
    check()
    assert torch.equal(got.cpu(), t.reshape(3, C, G, K).amax(3))
    if G == 1:
        assert torch.equal(KM.groupmax(t.to(dev), K, channel_major=True).cpu()[0].t(), t.amax(2))
    with pytest.raises(ValueError, match="groupmax"):
        KM.groupmax(t.to(dev), G * K + 1)                                   # no whole number of groups


def test_linear_layers_run_with_the_batch_as_columns(dev):
    g = torch.Generator().manual_seed(3)
    f, w, b = torch.randn(5, 1024, generator=g), torch.randn(512, 1024, generator=g) / 32.0, torch.randn(512, generator=g)
    got = KM.conv(f.t().contiguous()[None].to(dev), KM.pack_weight(w).to(dev), b.to(dev), 512, True)[0].t()
    assert max(O.rel_l2_per_sample(got, torch.relu(f.double() @ w.double().t() + b.double()))) < TOL


# ---- whole network -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_network_against_the_fixture(dev, golden, name):
    gold = golden("pointmlp")
    cpu_model, cfg, f64, l64 = oracle64(gold, name)
    x = torch.from_numpy(gold[f"{name}_x"])
    xyz = np.ascontiguousarray(gold[f"{name}_x"].transpose(0, 2, 1))
    m = make(name).to(dev)
    with torch.no_grad():
        tables = m.geometry(x.to(dev).permute(0, 2, 1))
        for i, ((f, k), (rf, rk), (of, ok)) in enumerate(zip(tables, fixture_tables(gold, name, len(cfg[0])),
                                                             O.geometry(xyz, cfg[0], cfg[1]))):
            f, k = f.cpu().numpy(), k.cpu().numpy()
            assert np.array_equal(f, rf), (name, i)                       # the reference run's picks, index for index
            assert np.array_equal(k, ok), (name, i)                       # the (distance, index) tables
            for b in range(2):                                            # the reference's tables but for equal coordinates
                assert O.same_neighbour_coordinates(xyz[b], k[b], rk[b]), (name, i, b)
            xyz = np.stack([c[j] for c, j in zip(xyz, f)])
        feat = m(x.to(dev), return_features=True)
        logits = m(x.to(dev))
        assert feat.is_cuda and tuple(feat.shape) == tuple(f64.shape) and tuple(logits.shape) == (2, 4)
        ef, el = np.array(O.rel_l2_per_sample(feat, f64)), np.array(O.rel_l2_per_sample(logits, l64))
        bf, bl = 3.0 * gold[f"{name}_feat_err"], 3.0 * gold[f"{name}_logit_err"]
        print(f"{name}: features HIP {ef} reference float32 {gold[f'{name}_feat_err']}; logits HIP {el} reference float32 "
              f"{gold[f'{name}_logit_err']}")
        assert np.all(ef < bf), (name, ef, bf)
        assert np.all(el < bl), (name, el, bl)
        assert torch.equal(m(x.to(dev)), logits)                          # two calls: the same bits
        assert torch.equal(m(x[1:2].to(dev)), logits[1:2])                # a cloud alone: the same bits
        assert torch.equal(m(x[1:2].to(dev), return_features=True), feat[1:2])


def test_buffer_edit_in_place_folds_again(dev, golden):
    gold = golden("pointmlp")
    m = make("tiny").to(dev)
    x = torch.from_numpy(gold["tiny_x"]).to(dev)
    with torch.no_grad():
        a = m(x)
        packed = m.packed(dev)[0]
        assert m.packed(dev)[0] is packed                                 # nothing changed: nothing packed again
        m.pre_blocks_list[1].operation[0].net2[1].running_var.add_(0.25)
        b = m(x)
        assert not torch.equal(a, b) and m.packed(dev)[0] is not packed
        m.local_grouper_list[0].affine_beta.add_(0.5)
        c = m(x)
        assert not torch.equal(b, c)
        cfg = O.config_of(m)
        sd = {k: v.cpu() for k, v in m.state_dict().items()}
        _, want = O.forward(sd, cfg, x.cpu(), fixture_tables(gold, "tiny", 2))
        assert np.all(np.array(O.rel_l2_per_sample(c, want)) < TOL)


def test_arbitrary_stage_list_runs(dev):
    """Three stages, widths 12 -> 24 -> 24 -> 72, 100 points (no power of two), K above and below the anchors left."""
    from lidargen.metrics.extractor.pointmlp import Model

    from lidarcrafter_amd.testing import seeded_fill_pointmlp

    m = seeded_fill_pointmlp(Model(points=100, class_num=3, embed_dim=12, res_expansion=0.5, bias=True, use_xyz=False,
                                   normalize="anchor", dim_expansion=[2, 1, 3], pre_blocks=[1, 0, 2], pos_blocks=[0, 1, 1],
                                   k_neighbors=[7, 20, 5], reducers=[2, 2, 5]), 9).eval().requires_grad_(False)
    c = O.clouds(2, 100, 8, real=[100, 37])
    x = torch.from_numpy(c).permute(0, 2, 1).contiguous()
    cfg = O.config_of(m)
    f64, l64 = O.forward(m.state_dict(), cfg, x, O.geometry(c, cfg[0], cfg[1]))
    m = m.to(dev)
    assert max(O.rel_l2_per_sample(m(x.to(dev), return_features=True), f64)) < TOL
    assert max(O.rel_l2_per_sample(m(x.to(dev)), l64)) < TOL


# ---- front-end ---------------------------------------------------------------------------------------------------------
def _loader(seed, n, N=64):
    g = np.random.default_rng(seed)
    batches = []
    for i in range(0, n, 4):
        b = min(4, n - i)
        real = g.integers(N // 3, N + 1, b)
        data = O.clouds(b, N, seed * 100 + i, real=list(real)) * np.float32(0.8 + 0.05 * seed)
        batches.append((torch.from_numpy(data), torch.from_numpy(g.integers(0, 3, b)), torch.from_numpy(real)))
    return batches


def test_get_fg_object_set_feature_and_obj_scores(dev, capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, bev, distribution, eval_utils
    from lidargen.metrics import fg_object as F

    m = make("tiny").to(dev)
    sets = []
    for seed in (1, 2):
        loader = _loader(seed, 40)
        s = F.get_fg_object_set_feature(loader, m, class_names=("car", "truck"))
        assert set(s) == {"unkonw", "car", "truck"}
        labels = np.concatenate([b[1].numpy() for b in loader])
        data = torch.cat([b[0] for b in loader])
        for ci, cname in ((1, "car"), (2, "truck")):
            n = int((labels == ci).sum())
            assert s[cname]["pts_feat"].shape == (n, 64) and s[cname]["bev_hists"].shape == (n, 100, 100)
        assert len(s["unkonw"]["pts_feat"]) == int((labels == 0).sum())
        cfg = O.config_of(m)
        cars = data[labels == 1]
        want, _ = O.forward({k: v.cpu() for k, v in m.state_dict().items()}, cfg, cars.permute(0, 2, 1),
                            O.geometry(cars.numpy(), cfg[0], cfg[1]))
        assert max(O.rel_l2_per_sample(s["car"]["pts_feat"], want)) < TOL
        hist = bev.point_cloud_to_histogram(cars[0].to(dev), min_depth=1e-6, max_depth=1e3, field_size=2.0).cpu().numpy()
        assert np.array_equal(s["car"]["bev_hists"][0], hist) and hist.sum() > 0
        sets.append(s)
    # a dozen objects cannot fill a 64 x 64 covariance: the scores are formed over the four widest-spread columns
    cols = np.argsort(np.concatenate([s["car"]["pts_feat"] for s in sets]).var(0))[-4:]
    for s in sets:
        s["car"]["pts_feat"] = s["car"]["pts_feat"][:, cols].astype(np.float64)
    capsys.readouterr()
    np.random.seed(0)
    out = eval_utils.compute_obj_scores(sets[0], sets[1], class_name="car")
    text = capsys.readouterr().out
    assert set(out) == {"frechet_distance", "squared_mmd", "jsd", "mmd"}
    fa, fb = sets[0]["car"]["pts_feat"], sets[1]["car"]["pts_feat"]
    assert out["frechet_distance"] == float(distribution.compute_frechet_distance(fa, fb)) and out["frechet_distance"] > 0
    np.random.seed(0)
    assert out["squared_mmd"] == float(distribution.compute_squared_mmd(fa, fb))
    ha, hb = (torch.from_numpy(s["car"]["bev_hists"]).to(dev).float() for s in sets)
    assert out["jsd"] == float(bev.compute_jsd_2d(ha, hb)) and out["mmd"] == float(bev.compute_mmd_2d(ha, hb))
    assert 0 < out["jsd"] < 1
    for name, key in (("OFD ", "frechet_distance"), ("OMMD", "squared_mmd"), ("OJSD", "jsd"), ("OBMD", "mmd")):
        assert OUTPUT_TEMPLATE.format(name, out[key]) in text
    same = eval_utils.compute_obj_scores(sets[0], sets[0])
    assert abs(same["jsd"]) < 1e-7 and abs(same["frechet_distance"]) < 1e-6 * float(np.trace(np.cov(fa, rowvar=False)))


def test_validate_classification(dev):
    from lidargen.metrics import fg_object as F

    m = make("tiny").to(dev)
    loader = _loader(3, 10)
    res = F.validate_classification(m, loader, class_names=["car", "truck", "bus"])
    assert res["class_names"] == ["unknow", "car", "truck", "bus"]
    data = torch.cat([b[0] for b in loader])
    cfg = O.config_of(m)
    _, logits = O.forward({k: v.cpu() for k, v in m.state_dict().items()}, cfg, data.permute(0, 2, 1),
                          O.geometry(data.numpy(), cfg[0], cfg[1]))
    assert np.array_equal(res["test_pred"], logits.argmax(1).numpy())
    assert np.array_equal(res["test_true"], np.concatenate([b[1].numpy() for b in loader]))
    assert np.array_equal(res["num_points_in_gt"], np.concatenate([b[2].numpy() for b in loader]))
    assert 0.0 <= F.compute_cgf_from_results(res)["overall"]["accuracy"] <= 1.0
