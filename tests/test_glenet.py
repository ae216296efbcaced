"""GPU tests of the GLENet / RGF kernels (csrc/glenet.hip) at the smallest shapes that can still go
wrong: objects around the 256-thread block of the centring kernel, rows around the 128-point tile of the trunk, a row index
past 65 535, pairs around the 64-thread block of the box kernels, draws around the 64-lane wave of the score kernel.
References: tests/_glenet_oracle.py (numpy / float64 restatements) and the reference's records in tests/golden/glenet.npz."""
import json

import numpy as np
import pytest
import torch

import _glenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx(golden):
    return golden("glenet")


@pytest.fixture(scope="module")
def net():
    from lidargen.metrics.models.glenet import DEFAULT_MODEL_CFG, Generator

    m = Generator(DEFAULT_MODEL_CFG, 3, 1)
    m.load_state_dict(O.seeded_state(7))
    return m.eval().requires_grad_(False).to(DEV)


@pytest.fixture(scope="module")
def e_ref(fx):
    """The reference's own error on the generic pairs, from the fixture."""
    return float(np.abs(fx["gen_iou"].astype(np.float64) - O.iou3d_f64(fx["gen_g"], fx["gen_q"])).max())


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _clouds(sizes, seed):
    r = np.random.default_rng(seed)
    pts = [(r.uniform(-0.5, 0.5, (n, 3)) * np.array([3.9, 1.6, 1.56]) + np.array([20.0, -8.0, 0.5])).astype(np.float32) for n in sizes]
    return pts, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- segment_center
def test_segment_center():
    from lidarcrafter_amd import ops_glenet as KG

    sizes = (1, 2, 255, 256, 257, 5000)
    pts, off = _clouds(sizes, 1)
    out, mean = KG.segment_center(_t(np.concatenate(pts)), _t(off))
    out, mean = out.cpu().numpy(), mean.cpu().numpy()
    for b, p in enumerate(pts):
        want = p.astype(np.float64).mean(axis=0).astype(np.float32)
        assert np.all(np.abs(mean[b].astype(np.float64) - want) <= np.spacing(np.abs(want))), (b, mean[b], want)
        assert np.array_equal(_bits(out[off[b]:off[b + 1]]), _bits(O.normalise(p, mean[b]))), b
        alone, mean1 = KG.segment_center(_t(p), _t(np.array([0, len(p)], np.int32)))
        assert np.array_equal(_bits(alone), _bits(out[off[b]:off[b + 1]])) and np.array_equal(_bits(mean1[0]), _bits(mean[b]))
    assert np.array_equal(out[0], np.zeros(3, np.float32))            # one point: it is its own mean


# ---------------------------------------------------------------------------------------------- trunk
def _norm_objects(sizes, seed):
    pts, off = _clouds(sizes, seed)
    norm = np.concatenate([O.normalise(p, p.astype(np.float64).mean(axis=0).astype(np.float32)) for p in pts])
    return norm, off


def _choice(sizes, D, K, seed):
    r = np.random.default_rng(seed)
    ch = np.stack([np.stack([r.integers(0, n, K) for n in sizes]) for _ in range(D)]).astype(np.int32)
    for b, n in enumerate(sizes):
        ch[:, b, 0] = 0                                             # index 0 ...
        ch[:, b, -1] = n - 1                                        # ... and n - 1
        if K >= 4:
            ch[:, b, 1] = ch[:, b, 2] = n // 2                      # a repeat
    return ch


def _gather(norm, off, ch):
    D, B, K = ch.shape
    return np.stack([norm[off[b] + ch[d, b]] for d in range(D) for b in range(B)]).astype(np.float32)          # [R, K, 3]


@pytest.mark.parametrize("K", [1, 127, 128, 129, 512])
@pytest.mark.parametrize("R", [1, 3])
def test_trunk(net, K, R):
    from lidarcrafter_amd import ops_glenet as KG
    from lidarcrafter_amd import ops_pointnet as KP

    f = net.folded()
    main, side = f["main"], f["side"]
    assert bool((net.x_encoder.fe.bn3.weight < 0).any()) and bool((net.obj_encoder.fe.bn3.weight < 0).any())
    sizes = (1,) if R == 1 and K == 1 else ((700,) if R == 1 else (1, 129, 700))      # an object of one point is in
    norm, off = _norm_objects(sizes, 2)
    ch = _choice(sizes, 1, K, 3 + K)
    fa, fs = KG.glenet_trunk(_t(norm), _t(off), _t(ch), main, side)
    assert tuple(fa.shape) == (512, R) and tuple(fs.shape) == (8, R)
    fa2, fs2 = KG.glenet_trunk(_t(norm), _t(off), _t(ch), main, side)
    assert torch.equal(fa, fa2) and torch.equal(fs, fs2)                                # two runs
    # the same kernel on a materialised copy of the gathered points with an identity index list
    g = _gather(norm, off, ch)
    ident = np.broadcast_to(np.arange(K, dtype=np.int32), (1, R, K)).copy()
    ga, gs = KG.glenet_trunk(_t(g.reshape(R * K, 3)), _t((np.arange(R + 1) * K).astype(np.int32)), _t(ident), main, side)
    assert torch.equal(fa, ga) and torch.equal(fs, gs)
    # a row alone
    for b in range(R):
        a1, s1 = KG.glenet_trunk(_t(norm[off[b]:off[b + 1]]), _t(np.array([0, sizes[b]], np.int32)), _t(ch[:, b:b + 1]), main, side)
        assert torch.equal(a1[:, 0], fa[:, b]) and torch.equal(s1[:, 0], fs[:, b])
    # featA: the bits of lc_pointnet_trunk_fwd on the same points, the third layer padded to its 1024 rows
    x = _t(np.ascontiguousarray(g.transpose(0, 2, 1)))
    w3 = torch.zeros((1024, 128), device=DEV)
    w3[:512] = main[4]
    b3 = torch.zeros(1024, device=DEV)
    b3[:512] = main[5]
    pn = KP.pointnet_trunk(x, None, main[0], main[1], main[2], main[3], w3, b3, False)
    assert torch.equal(pn[:, :512].t(), fa)
    # featS: float32 fma chains over ascending input channel from the bias
    layers = [(side[0].cpu().numpy(), side[1].cpu().numpy()), (side[2].cpu().numpy(), side[3].cpu().numpy()),
              (side[4].cpu().numpy(), side[5].cpu().numpy())]
    assert np.array_equal(_bits(fs.t()), _bits(O.side_trunk_f32(layers, g.transpose(0, 2, 1))))
    # float64: per row within 3 x m_ref, the error of a torch float32 evaluation of the same module layers (BatchNorm as its
    # own step) against the same float64 value, measured here
    sd = {k: torch.as_tensor(v) for k, v in O.seeded_state(7).items()}
    xg = g.transpose(0, 2, 1)
    for got, prefix in ((fa, "x_encoder.fe."), (fs, "obj_encoder.fe.")):
        want = O.trunk_max_f64(sd, prefix, xg)
        err = (got.t().cpu().double() - want).norm(dim=1) / want.norm(dim=1)
        m_ref = (O.trunk_max_f32(sd, prefix, xg).double() - want).norm(dim=1) / want.norm(dim=1)
        print(f"K={K} R={R} {prefix} rel-L2 per row: HIP {err.tolist()} torch float32 {m_ref.tolist()}")
        assert bool((err <= 3 * m_ref).all()), (prefix, err.tolist(), m_ref.tolist())


def test_trunk_rows_past_65535(net):
    """R = 65 537 rows of K = 2: the row is the block index.  One object of 5 points has 25 index pairs; every row must
    carry the bits of its pair from a 25-row call."""
    from lidarcrafter_amd import ops_glenet as KG

    f = net.folded()
    norm, off = _norm_objects((5,), 4)
    R = 65537
    r = np.random.default_rng(6)
    ch = r.integers(0, 5, (R, 1, 2)).astype(np.int32)
    ch[-1, 0] = (4, 0)
    fa, fs = KG.glenet_trunk(_t(norm), _t(off), _t(ch), f["main"], f["side"])
    combos = np.array([[i, j] for i in range(5) for j in range(5)], np.int32).reshape(25, 1, 2)
    ca, cs = KG.glenet_trunk(_t(norm), _t(off), _t(combos), f["main"], f["side"])
    pick = _t(ch[:, 0, 0] * 5 + ch[:, 0, 1], torch.int64)
    assert torch.equal(fa, ca[:, pick]) and torch.equal(fs, cs[:, pick])
    assert torch.isfinite(fa).all() and torch.isfinite(fs).all()


def test_trunk_draw_grid_and_clamped_indices(net):
    """[D, B] rows: row d B + b reads object b.  An index outside the object is clamped into it."""
    from lidarcrafter_amd import ops_glenet as KG

    f = net.folded()
    sizes = (3, 130)
    norm, off = _norm_objects(sizes, 8)
    ch = _choice(sizes, 3, 130, 9)
    fa, fs = KG.glenet_trunk(_t(norm), _t(off), _t(ch), f["main"], f["side"])
    for d in range(3):
        a, s = KG.glenet_trunk(_t(norm), _t(off), _t(ch[d:d + 1]), f["main"], f["side"])
        assert torch.equal(a, fa[:, 2 * d:2 * d + 2]) and torch.equal(s, fs[:, 2 * d:2 * d + 2])
    wild = ch.copy()
    wild[:, 0, 5], wild[:, 1, 7] = 1000, -4
    want = ch.copy()
    want[:, 0, 5], want[:, 1, 7] = 2, 0
    a, s = KG.glenet_trunk(_t(norm), _t(off), _t(wild), f["main"], f["side"])
    b, t = KG.glenet_trunk(_t(norm), _t(off), _t(want), f["main"], f["side"])
    assert torch.equal(a, b) and torch.equal(s, t)


# ---------------------------------------------------------------------------------------------- rotated boxes
def test_rbox_intersection_reproduces_the_reference(fx):
    from lidarcrafter_amd import ops_glenet as KG

    names = json.loads(str(fx["named"]))
    for tag in ("gen", "nam"):
        pts, cnt, area = KG.rbox_intersection(_t(fx[tag + "_cg"]), _t(fx[tag + "_cq"]))
        assert np.array_equal(cnt.cpu().numpy(), fx[tag + "_cnt"])
        assert np.array_equal(_bits(pts), _bits(fx[tag + "_pts"]))
        sep = O.angles_separated(O.rinter(fx[tag + "_cg"], fx[tag + "_cq"])[3], fx[tag + "_cnt"])
        same = _bits(area) == _bits(fx[tag + "_area"])
        print(f"{tag}: {int((~sep).sum())} of {len(sep)} pairs set aside, {int((~same).sum())} areas differ in their bits")
        assert np.all(same[sep])
        if tag == "gen":
            assert (~sep).mean() <= 0.02
        else:
            for n in ("identical", "turned_by_pi", "negative_size"):
                i = names.index(n)
                assert same[i] if sep[i] else cnt[i].item() == fx["nam_cnt"][i], n


@pytest.mark.parametrize("N", [1, 63, 64, 65, 2000])
def test_riou3d_paired_against_the_exact_clip(fx, e_ref, N):
    from lidarcrafter_amd import ops_glenet as KG

    g, q = fx["gen_g"][:N], fx["gen_q"][:N]
    got = KG.riou3d_paired(_t(g), _t(q)).cpu().numpy()
    err = np.abs(got.astype(np.float64) - O.iou3d_f64(g, q))
    print(f"N={N}: max error {err.max():.3e}, e_ref {e_ref:.3e}")
    assert err.max() <= 3 * e_ref
    wide = np.concatenate([q, np.full((N, 2), 7.0, np.float32)], axis=1)                  # [N, 9]: the first seven columns count
    assert np.array_equal(_bits(KG.riou3d_paired(_t(g), _t(wide))), _bits(got))


def test_riou3d_named_cases(fx, e_ref):
    from lidargen.metrics.models.glenet.eval_utils import iou3d

    names = json.loads(str(fx["named"]))
    g, q = fx["nam_g"], fx["nam_q"]
    got = iou3d(_t(g), _t(q)).cpu().numpy()
    assert not np.isnan(got).any()
    positive = (g[:, 3:6] > 0).all(axis=1) & (q[:, 3:6] > 0).all(axis=1)
    exact = O.iou3d_f64(g[positive], q[positive])
    agree = np.zeros(len(names), bool)
    agree[positive] = np.abs(fx["nam_iou"][positive].astype(np.float64) - exact) <= e_ref
    for n, a, b, ok in zip(names, got, fx["nam_iou"], agree):
        print(f"{n:22s} kernel {a:.7g} reference {b:.7g} {'checked' if ok else 'reference and exact value differ'}")
    checked = {n for n, ok in zip(names, agree) if ok}
    assert checked == set(names) - {"identical", "turned_by_pi", "negative_size"}, checked       # 11 of the 14
    assert np.all(np.abs(got[agree].astype(np.float64) - fx["nam_iou"][agree]) <= e_ref)


# ---------------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", [1, 2, 30, 64, 65])
def test_glenet_score(D, B):
    from lidarcrafter_amd import ops_glenet as KG

    r = np.random.default_rng(100 * D + B)
    gt = np.concatenate([r.normal(0, 0.1, (B, 3)), r.normal(0, 0.1, (B, 3)), r.uniform(-3, 3, (B, 1))], axis=1).astype(np.float32)
    gt[0, 6] = 2.5                                                   # w = angle - 2.5 is negative for most draws
    box = np.tile(np.concatenate([gt, np.zeros((B, 2), np.float32)], axis=1), (D, 1, 1))
    box = (box + r.normal(0, 0.05, box.shape)).astype(np.float32)
    box[..., 6] += r.normal(0, 0.3, (D, B)).astype(np.float32)
    box[0, 0, 6] = 2.0                                               # ... and for this one by construction
    pred, overlap, variance, mean_overlap = KG.glenet_score(_t(box), _t(gt))
    assert np.array_equal(_bits(pred[..., 7:]), _bits(box[..., 7:])) and np.array_equal(_bits(pred[..., 6]), _bits(box[..., 6]))
    want = O.decode(box[..., :7])
    assert np.allclose(pred[..., :7].cpu().numpy(), want, rtol=2e-6, atol=0)             # exp differs in its last bit
    gt_dec = KG.glenet_score(_t(np.concatenate([gt, np.zeros((B, 2), np.float32)], axis=1)[None]), _t(gt))[0][0]   # [B, 9]
    pair = KG.riou3d_paired(gt_dec.repeat(D, 1), pred.reshape(D * B, 9).contiguous())
    assert np.array_equal(_bits(pair.reshape(D, B)), _bits(overlap))
    p, ov = pred.cpu().numpy(), overlap.cpu().numpy().astype(np.float64)
    assert (p[:, 0, 6] - 2.5 < 0).any()
    for b in range(B):
        v = O.score(p[:, b], gt[b, 6])
        assert np.allclose(variance[b].cpu().numpy(), v, rtol=1e-12, atol=0), (b, variance[b], v)
        assert np.isclose(mean_overlap[b].item(), ov[:, b].mean(), rtol=1e-12, atol=0)
    if D == 1:
        assert torch.count_nonzero(variance) == 0
    else:
        assert float(overlap.max()) > 0.2 and float(variance.min()) > 0


# ---------------------------------------------------------------------------------------------- end to end
def _rows_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)


def test_sample_boxes_against_the_reference(fx, net):
    x, text, eps, _, off = O.gathered(fx)
    D, B, K = fx["obj_choice"].shape
    args = (_t(fx["obj_points"]), _t(fx["obj_offsets"]), _t(fx["obj_text"][fx["obj_class"]]), _t(fx["obj_choice"]), _t(fx["obj_eps"]))
    raw = net.sample_boxes(*args, postprocess=False)
    assert tuple(raw.shape) == (D, B, 9)
    raw = raw.reshape(D * B, 9).cpu().numpy()
    f64 = O.generator_f64(O.seeded_state(7), x, text, eps)[2].numpy()
    m_ref = _rows_err(fx["ref_box"], f64)                              # the reference float32 module's own error, per row
    err = _rows_err(raw, f64)
    print(f"rel-L2 per row against float64: HIP {err}\nreference float32 {m_ref}")
    assert np.all(err <= 3 * m_ref)
    assert np.all(_rows_err(raw, fx["ref_box"]) <= 4 * m_ref)
    # the heading post-process: the reference's angle up to the half turns a logit tie or a floor edge can move
    post = net.sample_boxes(*args).reshape(D * B, 9).cpu().numpy()
    keep = [0, 1, 2, 3, 4, 5, 7, 8]
    assert np.array_equal(_bits(post[:, keep]), _bits(raw[:, keep]))
    d = post[:, 6].astype(np.float64) - fx["ref_box_post"][:, 6]
    turns = np.round(d / np.pi)
    assert np.all(np.abs(d - turns * np.pi) <= 1e-5)
    v = fx["ref_box"][:, 6].astype(np.float64) - 0.78539
    edge = np.abs(v / np.pi - np.round(v / np.pi)) < 1e-5
    tie = np.abs(fx["ref_box"][:, 7] - fx["ref_box"][:, 8]) < 1e-5
    assert np.all((turns == 0) | edge | tie)
    # forward(batch_dict) on the gathered, normalised points of draw 0: the same rows
    batch = {"points": _t(x[:B]), "text_feat": _t(text[:B]), "eps": _t(fx["obj_eps"][0])}
    assert np.array_equal(_bits(net(batch)), _bits(post[:B]))
    g = torch.Generator().manual_seed(3)
    batch = {"points": _t(x[:B]), "text_feat": _t(text[:B]), "generator": g}
    first = net(batch).clone()
    g.manual_seed(3)
    assert torch.equal(net(batch), first) and not torch.equal(first, _t(post[:B]))
    # an object without points
    off0 = fx["obj_offsets"].copy()
    off0[1] = 0
    with pytest.raises(ValueError, match="without points"):
        net.sample_boxes(args[0], _t(off0), *args[2:])


def _synthetic_dataset(seed):
    from lidargen.metrics.datasets.object_uncertainty_dataset import NuscObjUncertainty

    r = np.random.default_rng(seed)
    sizes = (1, 5, 40, 140, 150, 151, 200, 300, 301, 400, 700, 2000)
    infos = []
    for i, n in enumerate(sizes):
        size = np.array([3.9, 1.6, 1.56]) * np.exp(r.normal(0, 0.1, 3))
        centre = np.array([r.uniform(-30, 30), r.uniform(-30, 30), r.uniform(-1, 1)])
        yaw = r.uniform(-np.pi, np.pi)
        p = r.uniform(-0.5, 0.5, (n, 3)) * size
        c, s = np.cos(yaw), np.sin(yaw)
        p = np.stack([p[:, 0] * c - p[:, 1] * s, p[:, 0] * s + p[:, 1] * c, p[:, 2]], axis=1) + centre
        infos.append({"points": p.astype(np.float32), "name": ("car", "truck", "bus")[i % 3], "num_points_in_gt": n,
                      "box3d_lidar": [*centre, *size, yaw]})
    text = {k: v for k, v in zip(("car", "truck", "bus"), r.normal(0, 0.05, (3, 1, 512)).astype(np.float32))}
    return NuscObjUncertainty(infos, text, generator=np.random.default_rng(seed + 1))


def test_compute_rgf_fold_and_table(net, capsys):
    from lidarcrafter_amd import ops_glenet as KG
    from lidargen.metrics import fg_object

    a = fg_object.compute_rgf_fold(_synthetic_dataset(5), net, draws=4, generator=torch.Generator().manual_seed(9))
    b = fg_object.compute_rgf_fold(_synthetic_dataset(5), net, draws=4, generator=torch.Generator().manual_seed(9))
    assert list(a) == list(b) == [f"{i}_{i}" for i in range(12)]
    for k in a:
        assert np.array_equal(a[k]["variance"], b[k]["variance"]) and a[k]["overlap"] == b[k]["overlap"]
        assert a[k]["variance"].shape == (7,) and np.isfinite(a[k]["variance"]).all() and np.isfinite(a[k]["overlap"])
    # the host route from the read-back of the same draws
    ds = _synthetic_dataset(5)
    batch = next(ds.batches(2048))
    choice = _t(ds.choice(np.diff(batch["offsets"]), 4))
    eps = torch.randn((4, 12, 8), generator=torch.Generator().manual_seed(9)).to(DEV)
    box = net.sample_boxes(_t(batch["points"]), _t(batch["offsets"]), _t(batch["text_feat"]), choice, eps)
    pred, overlap, _, _ = KG.glenet_score(box, _t(batch["gt_boxes"]))
    pred, overlap = pred.cpu().numpy(), overlap.cpu().numpy().astype(np.float64)
    host = {k: {"variance": O.score(pred[:, i], batch["gt_boxes"][i, 6]), "overlap": overlap[:, i].mean(),
                "pointnum": batch["num_points_in_gt"][i]} for i, k in enumerate(batch["key"])}
    want = fg_object.compute_rgf_from_results(host)
    got = fg_object.compute_rgf([_synthetic_dataset(5)], net, draws=4, generator=torch.Generator().manual_seed(9))
    with pytest.raises(ValueError, match="two datasets"):            # two unfolded lists number their objects alike
        fg_object.compute_rgf([_synthetic_dataset(5), _synthetic_dataset(5)], net, draws=1)
    capsys.readouterr()
    assert list(got["partitions"]) == list(want["partitions"]) == ["<150", "150-300", ">300"]
    for x, y in [(got["overall"], want["overall"])] + [(got["partitions"][k], want["partitions"][k]) for k in want["partitions"]]:
        assert np.allclose(x["variance"], y["variance"], rtol=1e-12, atol=0) and np.isclose(x["overlap"], y["overlap"], rtol=1e-12, atol=0)
