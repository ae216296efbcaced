"""CPU tests of the Frechet Range Image Distance: the float64 oracle (tests/_rangenet_oracle.py) against the reference's
recorded outputs for both module trees (tests/golden/rangenet.npz), the state-dict contract, the key translation, the
BatchNorm fold, the weight packing, the range-image projection, the subsample, every refusal, the loaders (which never
fetch), the argument checks of the C entries, and the refusals of compute_logits / evaluate that other tests pin."""
import ctypes
import inspect
import io
import os
import random
import re
import sys
import tarfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rangenet_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_CFG = {"size": [8, 64], "fov": [10, -30], "depth_range": [1.0, 45.0]}
INPUTS5 = {"range": True, "xyz": True, "remission": True}


@pytest.fixture(scope="module")
def gold(golden):
    return golden("rangenet")


@pytest.fixture(scope="module")
def trees():
    """(Model darknet-53 filled with salt 1, RangeNet darknet-21 filled with salt 2): the fixture's two modules."""
    from lidarcrafter_amd.testing import seeded_fill_rangenet
    from lidargen.metrics.extractor.rangenet import RangeNet
    from lidargen.metrics.models.rangenet.model import Model

    m = seeded_fill_rangenet(Model(O.config(53)), 1).eval().requires_grad_(False)
    e = seeded_fill_rangenet(RangeNet(inputs=INPUTS5, num_classes=20, backbone=21), 2).eval().requires_grad_(False)
    return m, e


def _check(name, got, want):
    errs = O.rel_l2_per_sample(got, want)
    print(f"{name}: per-sample rel-L2 {['%.2e' % e for e in errs]} (limit {O.TOL_CONV:.0e})")
    assert max(errs) < O.TOL_CONV, (name, errs)


@pytest.mark.parametrize("prefix", ["m", "e"])
def test_state_dict_contract(gold, trees, prefix):
    sd = trees[0 if prefix == "m" else 1].state_dict()
    assert list(sd.keys()) == list(gold[f"{prefix}_names"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(gold[f"{prefix}_shapes"])
    sums = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])
    np.testing.assert_allclose(sums, gold[f"{prefix}_checksums"], rtol=1e-12, atol=1e-12)
    assert "backbone.enc3.residual_5.conv2.weight" in trees[0].state_dict()
    assert "decoder.dec5.upconv.bias" in trees[0].state_dict()
    assert "backbone.bn1.num_batches_tracked" in trees[0].state_dict()


def test_oracle_vs_reference_model(gold, trees):
    sd = trees[0].state_dict()
    x = torch.from_numpy(gold["m_x"])
    enc, dec = O.model_forward(sd, O.config(53), x, torch.float64)
    _check("decoder", dec, gold["m_decoder"])
    for agg in ("all", "sector", "depth"):
        _check(agg, O.aggregate(dec, agg), gold[f"m_{agg}"])
    _check("return_logits", enc.mean([2, 3]), gold["m_logits"])
    # the fill keeps the 53-layer network in range and every feature column alive
    peak = float(np.abs(gold["m_decoder"]).max())
    assert 10.0 < peak < 1e3, peak
    assert float(np.abs(gold["m_depth"][0] - gold["m_depth"][1]).min()) > 0.0
    assert float(np.abs(gold["m_depth"]).min()) > 0.0


def test_oracle_vs_reference_extractor(gold, trees):
    sd = trees[1].state_dict()
    x = torch.from_numpy(gold["e_x"])
    dec, logits = O.extractor_forward(sd, 21, x, torch.float64)
    _check("decoder", dec, gold["e_decoder"])
    _check("lidargen", O.subsample(dec), gold["e_lidargen"])
    _check("head", logits, gold["e_head"])
    assert gold["e_head"].shape == (1, 20, 16, 64) and gold["e_lidargen"].shape == (1, 4096)


def test_key_translation(gold):
    from lidargen.metrics.extractor.rangenet import RangeNet, _translate_param_name

    src, dst = list(gold["translate_src"]), list(gold["translate_dst"])
    assert [_translate_param_name(k) for k in src] == dst
    own = RangeNet(inputs={"range": True, "xyz": True, "remission": False}, num_classes=20, backbone=53).state_dict()
    assert sorted(own) == sorted(dst)


def test_fold_against_float64_formula():
    from lidarcrafter_amd import ops_rangenet as KR

    g = torch.Generator().manual_seed(3)
    for mode, Ci, Co in ((0, 8, 6), (1, 5, 7), (2, 4, 3), (3, 6, 5)):
        w = torch.randn(KR.weight_shape(mode, Ci, Co), generator=g)
        cb = torch.randn(Co, generator=g) if mode == 3 else None
        gamma, beta, mean = (torch.randn(Co, generator=g) for _ in range(3))
        var = 0.5 + torch.rand(Co, generator=g)
        w32, b32 = KR.fold_bn(w, cb, (gamma, beta, mean, var, 1e-5), mode)
        w64, b64 = O.fold64(w, cb, gamma, beta, mean, var, 1e-5, mode)
        assert w32.dtype == torch.float32 and torch.equal(w32, w64.float()) and torch.equal(b32, b64.float())
        # folded conv == conv + BatchNorm, in float64
        x = torch.randn(2, Ci, 3, 5, generator=g, dtype=torch.float64)
        y = O.raw_conv(x, w.double(), mode) + (0 if cb is None else cb.double().view(1, -1, 1, 1))
        y = torch.nn.functional.batch_norm(y, mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
        z = O.raw_conv(x, w64, mode) + b64.view(1, -1, 1, 1)
        assert float((y - z).abs().max()) < 1e-12 * float(y.abs().max())
    w32, b32 = KR.fold_bn(w, cb, None, 3)                      # the head: nothing to fold
    assert torch.equal(w32, w) and torch.equal(b32, cb)


def test_pack_layout_and_tile_extents():
    from lidarcrafter_amd import _lib
    from lidarcrafter_amd import ops_rangenet as KR

    h = _lib.lib()
    assert [h.lc_rangenet_tile_extent(i) for i in range(5)] == [KR.TILE_W, KR.TILE_H, KR.TILE_CO, KR.TILE_W_MAX, 0]
    g = torch.Generator().manual_seed(4)
    for mode, Ci, Co in ((0, 33, 20), (1, 5, 32), (2, 17, 40), (3, 18, 33)):
        w = torch.randn(KR.weight_shape(mode, Ci, Co), generator=g)
        p = KR.pack_weight(w, mode)
        KC, T = KR.K_CHUNK[mode], KR.TAPS[mode]
        nch, ncb = -(-Ci // KC), -(-Co // 32)
        assert p.numel() == KR.packed_weight_elems(mode, Ci, Co) == ncb * nch * T * KC * 32
        p = p.view(ncb, nch, T, KC // 8, 64, 4)
        taps = [1, 3, 2, 0] if mode == 3 else list(range(T))
        for cb, ch, t, q, lane, e in ((0, 0, 0, 0, 0, 0), (ncb - 1, nch - 1, T - 1, KC // 8 - 1, 63, 3), (0, nch - 1, T // 2, 1, 37, 2)):
            co, ci = cb * 32 + (lane & 31), ch * KC + 2 * (4 * q + e) + (lane >> 5)
            if co < Co and ci < Ci:
                want = w[ci, co, 0, taps[t]] if mode == 3 else w.reshape(Co, Ci, T)[co, ci, taps[t]]
            else:
                want = torch.tensor(0.0)
            assert p[cb, ch, t, q, lane, e] == want, (mode, cb, ch, t, q, lane, e)
        assert float(p.double().pow(2).sum()) == pytest.approx(float(w.double().pow(2).sum()), rel=1e-12)
    assert h.lc_rangenet_packed_weight_elems(4, 8, 8) == 0 and h.lc_rangenet_packed_weight_elems(1, 0, 8) == 0
    with pytest.raises(ValueError):
        KR.pack_weight(torch.zeros(4, 4, 3, 3), 0)


def test_flop_formula_counts_the_plan(trees):
    from lidargen.metrics.models.rangenet.plan import flops_per_pixel

    for tree, layers, in_ch, head in ((trees[0], 53, 4, 0), (trees[1], 21, 5, 20)):
        macs, px = 0.0, 1.0
        for L in tree.plan().layers:
            w = L.conv.weight
            if L.mode == 2:
                px /= 2
            if L.mode == 3:
                px *= 2
                macs += px * w.shape[0] * w.shape[1] * 2           # two of the four taps per output pixel
            else:
                macs += px * w[0].numel() * w.shape[0]
        assert macs == flops_per_pixel(layers, in_ch, head)
    assert flops_per_pixel(53, 4) == 2738304.0                      # 2.7 M multiply-adds per full-resolution pixel


def test_range_projection_matches_reference(gold):
    from lidargen.metrics import metric_utils as MU

    cloud = gold["cloud"]
    rng_img, feat = MU.pcd2range(cloud, **RANGE_CFG)
    assert feat is None and rng_img.dtype == np.float32
    assert np.array_equal(rng_img, gold["proj_range"])
    assert np.array_equal(MU.range2xyz(rng_img, log_scale=False, **RANGE_CFG), gold["proj_xyz"])
    prep = MU.preprocess_range(cloud, **RANGE_CFG)
    assert prep.shape == (4, 8, 64) and np.array_equal(prep, gold["prep"])
    # the cases the cloud was built for
    depth = np.linalg.norm(cloud, 2, axis=1)
    assert (depth <= 1.0).any() and (depth >= 45.0).any()
    assert rng_img[:, 63].max() > 0 and rng_img[0].max() > 0 and rng_img[7].max() > 0
    assert 0 < (rng_img > 0).sum() < ((depth > 1.0) & (depth < 45.0)).sum()      # pixels were contended
    near = np.linalg.norm(np.array([10.0, 0.5, -0.5], np.float32))
    assert np.isclose(rng_img, near).any() and not np.isclose(rng_img, 2 * near).any()
    rem = np.arange(len(cloud), dtype=np.float32)
    assert MU.pcd2range(cloud, remission=rem, **RANGE_CFG)[1].max() > 0
    assert MU.pcd2range(cloud, labels=rem, **RANGE_CFG)[1].min() == 0


def test_subsample_indices_and_global_rng(gold, trees):
    from lidargen.metrics.extractor import rangenet as R

    random.seed(123)
    state = random.getstate()
    idx = R.subsample_indices(32 * 16 * 64)
    assert random.getstate() == state
    assert idx == list(gold["subsample_idx"])
    y = torch.arange(2 * 32 * 16 * 64, dtype=torch.float32).view(2, 32, 16, 64)
    f = trees[1].flatten_and_subsample(y)
    assert random.getstate() == state
    assert torch.equal(f[1], y[1].reshape(-1)[torch.tensor(idx)])


def test_refusals(trees):
    from lidargen.metrics.extractor import rangenet as R
    from lidargen.metrics.extractor.rangenet import Preprocess, RangeNet
    from lidargen.metrics.models.rangenet.model import Backbone, Decoder, Model

    m, e = trees
    x = torch.zeros(1, 5, 16, 64)
    with pytest.raises(NotImplementedError, match="OS"):
        Model(O.config(53, OS=16))
    with pytest.raises(NotImplementedError, match="OS"):
        Backbone(O.config(21, OS=8)["backbone"])
    with pytest.raises(NotImplementedError, match="OS"):
        Decoder(O.CONFIG["decoder"], OS=16)
    with pytest.raises(NotImplementedError, match="return_list"):
        m(x, return_list=["enc_0"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e(x)
    with pytest.raises(NotImplementedError, match="Model.forward"):
        m.backbone(x)
    fresh = Model(O.config(21))
    with pytest.raises(NotImplementedError, match="training mode"):
        fresh(x)
    with pytest.raises(NotImplementedError, match="grad mode"):
        fresh.eval()(x)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        fresh.eval()(x)
    fe = RangeNet(inputs=INPUTS5, num_classes=3, backbone=21)
    with pytest.raises(NotImplementedError, match="training mode"):
        fe(x)
    with pytest.raises(NotImplementedError, match="grad mode"):
        fe.eval()(x)
    for layers, flags in ((21, (True, False, False)), (53, (False, True, True)), (21, (False, False, True))):
        b = Backbone(O.config(layers, *flags)["backbone"])
        assert b.conv1.weight.shape[1] == b.get_input_depth() == len(b.input_idxs) == flags[0] + 3 * flags[1] + flags[2]
    for name in ("kNN", "knn", "CRFRNN", "crf_rnn", "make_semantickitti_cmap"):
        with pytest.raises(NotImplementedError, match="not built"):
            getattr(R, name)(20)
    p = Preprocess()
    img = torch.tensor([2.0, -1.0]).view(1, 1, 1, 2).repeat(1, 5, 1, 1)
    assert torch.equal(p(img), torch.tensor([2.0, 0.0]).view(1, 1, 1, 2).repeat(1, 5, 1, 1))
    assert torch.equal(p(img, torch.zeros(1, 1, 1, 2)), torch.zeros_like(img))
    with pytest.raises(AssertionError):
        p(img[:, :4])
    assert len(p.state_dict()) == 0


def _write_archive(path, model, head, arch="2025-7-17-06:41"):
    cfg = ("backbone:\n  input_depth: {range: true, xyz: true, remission: false}\n  extra: {layers: 21}\n"
           "dataset:\n  sensor:\n    img_means: [1.0, 2.0, 3.0, 4.0, 5.0]\n    img_stds: [6.0, 7.0, 8.0, 9.0, 10.0]\n")
    with tarfile.open(path, "w:gz") as tar:
        for name, sd in (("backbone", model.backbone.state_dict()), ("segmentation_decoder", model.decoder.state_dict()),
                         ("segmentation_head", head.state_dict())):
            buf = io.BytesIO()
            torch.save(sd, buf)
            info = tarfile.TarInfo(f"{arch}/{name}")
            info.size = buf.tell()
            buf.seek(0)
            tar.addfile(info, buf)
        info = tarfile.TarInfo(f"{arch}/arch_cfg.yaml")
        info.size = len(cfg)
        tar.addfile(info, io.BytesIO(cfg.encode()))


def test_loaders_read_local_files_and_fetch_nothing(tmp_path, monkeypatch):
    import yaml

    from lidarcrafter_amd.testing import seeded_fill_rangenet
    from lidargen import metrics
    from lidargen.metrics.extractor import rangenet as R
    from lidargen.metrics.models.rangenet.model import Model

    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    url = "http://www.ipb.uni-bonn.de/html/projects/bonnetal/lidar/semantic/models/darknet53-1024.tar.gz"
    cached = os.path.join(str(tmp_path / "hub"), "checkpoints", "darknet53-1024.tar.gz")
    with pytest.raises(FileNotFoundError, match=re.escape(cached)):
        R.rangenet53(url_or_file=url)
    with pytest.raises(FileNotFoundError, match=re.escape(cached)):
        R.rangenet53(weights="SemanticKITTI_64x1024")
    with pytest.raises(FileNotFoundError, match="darknet21.tar.gz"):
        R.rangenet21(weights="SemanticKITTI_64x2048")
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "none.tar.gz"))):
        R.build_rangenet(str(tmp_path / "none.tar.gz"))
    assert not os.path.exists(tmp_path / "hub")                       # not even the cache directory is made
    src = inspect.getsource(R) + inspect.getsource(metrics) + inspect.getsource(sys.modules[Model.__module__])
    for word in ("download_url", "urlopen", "urlretrieve", "requests", "load_state_dict_from_url"):
        assert word not in src, word

    # a local archive: the folder name of the reference's own file, or any other
    model = seeded_fill_rangenet(Model(O.config(21)), 5)
    head = seeded_fill_rangenet(torch.nn.Sequential(torch.nn.Dropout2d(0.1), torch.nn.Conv2d(32, 7, 3, 1, 1)), 5)
    for arch in ("2025-7-17-06:41", "darknet21"):
        path = str(tmp_path / f"{arch.replace(':', '_')}.tar.gz")
        _write_archive(path, model, head, arch)
        net, pre = R.rangenet53(url_or_file=path, compile=True)
        assert net.backbone == 21 and net.num_classes == 7 and net.in_ch == 4 and not net.training
        assert pre.num_channels == 4 and pre.mean == [1.0, 2.0, 3.0, 4.0]
        assert torch.equal(net.enc3.residual_blocks[1].residual[1][0].weight, model.backbone.enc3.residual_1.conv2.weight)
        assert torch.equal(net.dec5.conv[0].bias, model.decoder.dec5.upconv.bias)
        assert torch.equal(net.head[1].bias, head[1].bias)
    fresh, none = R.rangenet21(inputs=INPUTS5, num_classes=4)
    assert none is None and fresh.backbone == 21 and fresh.training

    # build_model('rangenet'): config.yaml + backbone + segmentation_decoder of <root>/<dataset>/rangenet
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "w"))):
        metrics.build_model("nuscenes", "rangenet", root=tmp_path / "w")
    folder = tmp_path / "w" / "nuscenes" / "rangenet"
    folder.mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="config.yaml"):
        metrics.build_model("nuscenes", "rangenet", root=tmp_path / "w")
    (folder / "config.yaml").write_text(yaml.safe_dump(O.config(21)))
    torch.save(model.backbone.state_dict(), folder / "backbone")
    with pytest.raises(FileNotFoundError, match="segmentation_decoder"):
        metrics.build_model("nuscenes", "rangenet", root=tmp_path / "w")
    torch.save(model.decoder.state_dict(), folder / "segmentation_decoder")
    got = metrics.build_model("nuscenes", "rangenet", root=tmp_path / "w")
    assert not got.training and not any(p.requires_grad for p in got.parameters())
    for (k, a), b in zip(got.state_dict().items(), model.state_dict().values()):
        assert torch.equal(a, b), k
    with pytest.raises(FileNotFoundError, match="backbone"):
        Model(O.config(21)).load_pretrained_weights(str(tmp_path / "nowhere"))


def test_c_entry_argument_checks():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    src = open(os.path.join(ROOT, "include", "lidarcrafter_hip.h")).read()
    codes = dict(re.findall(r"#define\s+(LC_E[A-Z]+)\s+\(?(-?\d+)\)?", src))
    EINVAL, EUNSUP = int(codes["LC_EINVAL"]), int(codes["LC_EUNSUP"])
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    al = p + (-p) % 16
    other = al + 64

    def conv(x=al, w=al, b=al, y=other, B=1, Ci=4, Co=4, H=2, W=2, mode=1, r1=None, r2=None):
        return h.lc_rangenet_conv_fwd(x, w, b, r1, r2, y, B, Ci, Co, H, W, mode, 1, None)

    assert conv(x=None) == EINVAL and conv(w=None) == EINVAL and conv(b=None) == EINVAL and conv(y=None) == EINVAL
    for kw in (dict(B=0), dict(Ci=0), dict(Co=0), dict(H=0), dict(W=0), dict(mode=4), dict(mode=-1)):
        assert conv(**kw) == EINVAL, kw
    assert conv(y=al) == EINVAL and conv(r1=other) == EINVAL and conv(r2=other) == EINVAL      # in place
    assert conv(w=al + 4) == EUNSUP                                                            # packed weights unaligned
    assert conv(B=70000) == EUNSUP and conv(B=600, Co=128 * 128) == EUNSUP                      # grid limits
    assert conv(H=140000) == EUNSUP
    red = h.lc_rangenet_reduce_fwd
    assert red(None, al, 1, 1, 16, 16, 0, None) == EINVAL and red(al, None, 1, 1, 16, 16, 0, None) == EINVAL
    assert red(al, other, 1, 1, 16, 16, 3, None) == EINVAL and red(al, other, 0, 1, 16, 16, 0, None) == EINVAL
    assert red(al, other, 1, 1, 8, 16, 2, None) == EUNSUP and red(al, other, 1, 1, 16, 8, 1, None) == EUNSUP
    assert h.lc_rangenet_pack_weight(None, 1, 4, 4, al) == EINVAL and h.lc_rangenet_pack_weight(al, 5, 4, 4, al) == EINVAL
    assert h.lc_abi_version() == 6


def test_pinned_refusals_name_the_new_calls():
    from lidargen.metrics import eval_utils, metric_utils

    with pytest.raises(NotImplementedError, match="'range'.*compute_range_logits"):
        metric_utils.compute_logits("32", "range", [])
    with pytest.raises(NotImplementedError, match="'frid'.*compute_frid"):
        eval_utils.evaluate([], [], ["frid"], "32")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            metric_utils.compute_range_logits("32", [O.metre_cloud(1)])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            eval_utils.extract_range_features(None, None, np.zeros((1, 5, 16, 64), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_utils.extract_range_features(None, None, torch.zeros(1, 5, 16, 64))


def test_compute_frd_on_feature_matrices(capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils
    from lidargen.metrics.distribution import compute_frechet_distance

    g = np.random.default_rng(5)
    a, b = g.normal(0.0, 1.0, (40, 12)), g.normal(0.3, 1.2, (50, 12))
    score = eval_utils.compute_frd(a, b, model=None)
    out = capsys.readouterr().out
    assert score == compute_frechet_distance(a, b)
    assert "Evaluating (FRD) ..." in out and OUTPUT_TEMPLATE.format("FRD ", score) in out
