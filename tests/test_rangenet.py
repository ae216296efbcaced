"""GPU tests of the dense RangeNet convolutions (csrc/rangenet.hip), of the network under both module trees and of the
FRID / FRD front-ends, against the float64 CPU oracle of tests/_rangenet_oracle.py.  Per-sample relative L2 below
TOL_CONV (derived in the oracle file); the float32 CPU oracle's own error is printed next to every whole-network figure.
T = the exported tile extents: a block row is 32 pixels for Co > 64, 64 for Co <= 64, 128 for Co <= 32 (64 in mode 2)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rangenet_oracle as O  # noqa: E402

from lidarcrafter_amd import ops_rangenet as KR  # noqa: E402
from lidarcrafter_amd.testing import error_profiles, rangenet_images, seeded_fill_rangenet  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = O.TOL_CONV
INPUTS5 = {"range": True, "xyz": True, "remission": True}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _block_row(mode, Co):
    """Pixels per block row of rn_conv_kernel for this layer (mode 3: input pixels)."""
    cw = 1 if (Co <= 32 and mode != 2) else (2 if Co <= 64 else 4)
    return KR.TILE_W * 4 // cw


def _case(mode, B, Ci, Co, H, W, seed, nres):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=g)
    x[torch.rand(x.shape, generator=g) < 0.1] = -1.0                      # holes, as range images have them
    w = torch.randn(KR.weight_shape(mode, Ci, Co), generator=g) / (Ci * KR.TAPS[mode]) ** 0.5
    b = torch.randn(Co, generator=g)
    res = [torch.randn(B, Co, H, KR.out_width(mode, W), generator=g) for _ in range(nres)]
    return x, w, b, res


def _run(dev, mode, x, w, b, act, res, out=None):
    wpk = KR.pack_weight(w.contiguous(), mode).to(dev)
    r = [t.to(dev) for t in res] + [None, None]
    return KR.conv(x.to(dev), wpk, b.to(dev), mode, b.numel(), act, res1=r[0], res2=r[1], out=out)


def _assert_conv(dev, mode, B, Ci, Co, H, W, seed, act=True, nres=1):
    x, w, b, res = _case(mode, B, Ci, Co, H, W, seed, nres)
    got = _run(dev, mode, x, w, b, act, res)
    r = res + [None, None]
    want = O.conv_layer(x, w, b, mode, act, r[0], r[1])
    assert tuple(got.shape) == tuple(want.shape) == (B, Co, H, KR.out_width(mode, W))
    errs = O.rel_l2_per_sample(got, want)
    assert max(errs) < TOL, (mode, B, Ci, Co, H, W, act, nres, errs)
    return max(errs)


@pytest.mark.parametrize("nres", [0, 1, 2])
@pytest.mark.parametrize("act", [False, True], ids=["linear", "lrelu"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_conv_epilogue(dev, mode, act, nres):
    worst = _assert_conv(dev, mode, 2, 5, 20, 3, KR.TILE_W + 1, 100 + mode, act, nres)
    print(f"mode {mode} act {act} addends {nres}: worst sample {worst:.2e}")


@pytest.mark.parametrize("Co", [20, 32, 40, 72])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_conv_edges(dev, mode, Co):
    """Both sides of every tile edge: W in {1, 2, 3, T-1, T, T+1, 2T+5} for the layer's block row T, H in {1, 2, 3} around
    the two-row block, Ci in {1, 4, 5} (a partly filled channel chunk); odd widths in mode 2, W = 1 in mode 3."""
    T = _block_row(mode, Co)
    Tp = 2 * T if mode == 2 else T                                        # mode 2 tiles OUTPUT pixels: two inputs each
    worst = 0.0
    for i, W in enumerate((1, 2, 3, Tp - 1, Tp, Tp + 1, 2 * Tp + 5)):
        worst = max(worst, _assert_conv(dev, mode, 2, (1, 4, 5)[i % 3], Co, (3, 1, 2)[i % 3], W, 200 + 10 * mode + i, True,
                                        i % 3))
    print(f"mode {mode} Co {Co} block row {T}: worst sample {worst:.2e}")


@pytest.mark.parametrize("mode,Ci,Co,H,W", [(0, 33, 65, 5, 70), (1, 17, 129, 4, 40), (2, 48, 64, 5, 131), (3, 40, 20, 3, 70),
                                            (3, 64, 96, 2, 33), (1, 32, 32, 33, 9), (0, 64, 32, 2, 300)])
def test_conv_more_chunks_and_blocks(dev, mode, Ci, Co, H, W):
    """Several channel chunks with a partial last one, several channel groups with a partial last one, several row and
    column blocks."""
    print(f"worst sample {_assert_conv(dev, mode, 2, Ci, Co, H, W, 300 + mode, True, 2):.2e}")


def test_conv_deepest_layer(dev):
    """K = 9 * 512 = 4608, the longest sum of the network (3x3, 512 -> 1024), at H = 3, W = 5."""
    print(f"K = 4608: worst sample {_assert_conv(dev, 1, 1, 512, 1024, 3, 5, 400, True, 1):.2e}")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_conv_writes_only_its_output(dev, mode):
    B, Ci, Co, H, W = 2, 5, 20, 3, 37
    x, w, b, res = _case(mode, B, Ci, Co, H, W, 500 + mode, 1)
    n = B * Co * H * KR.out_width(mode, W)
    pad = 256
    buf = torch.full((n + 2 * pad,), -7.5, device=dev)
    out = buf[pad:pad + n].view(B, Co, H, KR.out_width(mode, W))
    got = _run(dev, mode, x, w, b, True, res, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:pad] == -7.5).all()) and bool((buf[pad + n:] == -7.5).all())
    assert max(O.rel_l2_per_sample(out, O.conv_layer(x, w, b, mode, True, res[0]))) < TOL
    assert not bool((out == -7.5).any())


@pytest.mark.parametrize("mode,Co", [(0, 72), (1, 20), (2, 40), (3, 32)])
def test_conv_bits_do_not_depend_on_the_batch(dev, mode, Co):
    x, w, b, res = _case(mode, 4, 5, Co, 3, 70, 600 + mode, 1)
    full = _run(dev, mode, x, w, b, True, res)
    again = _run(dev, mode, x, w, b, True, res)
    alone = _run(dev, mode, x[2:3].contiguous(), w, b, True, [res[0][2:3].contiguous()])
    assert torch.equal(full, again)
    assert torch.equal(full[2:3], alone)


def test_aggregations(dev):
    g = torch.Generator().manual_seed(7)
    y = torch.randn(3, 5, 32, 96, generator=g) + 0.5
    for kind in ("all", "sector", "depth"):
        got = KR.reduce(y.to(dev), kind)
        want = O.aggregate(y.double(), kind)
        assert got.shape == want.shape
        assert max(O.rel_l2_per_sample(got, want)) < 1e-6, kind
        assert torch.equal(got, KR.reduce(y.to(dev), kind))
    assert torch.equal(KR.reduce(y[1:2].contiguous().to(dev), "depth"), KR.reduce(y.to(dev), "depth")[1:2])
    with pytest.raises(ValueError, match="% 16"):
        KR.reduce(y[:, :, :24].contiguous().to(dev), "depth")
    with pytest.raises(ValueError, match="% 16"):
        KR.reduce(y[:, :, :, :40].contiguous().to(dev), "sector")
    assert KR.reduce(y[:, :, :24].contiguous().to(dev), "sector").shape == (3, 80)


# ---- whole network -------------------------------------------------------------------------------------------------
def _model(layers, salt):
    from lidargen.metrics.models.rangenet.model import Model

    return seeded_fill_rangenet(Model(O.config(layers)), salt).eval().requires_grad_(False)


_ORACLE = {}


def _model_oracle(layers, salt, B, H, W, seed):
    """(input, float64 (encoder, decoder), float32 (encoder, decoder)) of the CPU oracle, computed once per case."""
    key = ("m", layers, salt, B, H, W, seed)
    if key not in _ORACLE:
        sd = _model(layers, salt).state_dict()
        x = rangenet_images(B, H, W, seed)
        _ORACLE[key] = (x, O.model_forward(sd, O.config(layers), x, torch.float64),
                        O.model_forward(sd, O.config(layers), x, torch.float32))
    return _ORACLE[key]


def _report(name, got, want64, want32):
    errs = O.rel_l2_per_sample(got, want64)
    base = O.rel_l2_per_sample(want32, want64)
    line = f"{name}: HIP {max(errs):.2e} per-sample worst; float32 CPU oracle {max(base):.2e}; limit {TOL:.0e}"
    if want64.dim() == 4:
        prof = error_profiles(torch.as_tensor(got), want64, ((1,),))["profiles"][(1,)]
        line += f"; worst channel {prof['index']} {prof['worst']:.2e} (median {prof['median']:.2e})"
    print(line)
    assert max(errs) < TOL, (name, errs, base)


@pytest.mark.parametrize("layers,B,H,W", [(21, 3, 16, 64), (53, 2, 16, 64), (53, 2, 32, 96)])
def test_model_tree_against_float64(dev, layers, B, H, W):
    """Decoder map, the three aggregations and the pooled encoder logits of models.rangenet.Model.  At W = 64 and 96 the
    deepest level is 2 and 3 pixels wide."""
    x, (enc64, dec64), (enc32, dec32) = _model_oracle(layers, 1, B, H, W, 31)
    m = _model(layers, 1).to(dev)
    with torch.no_grad():
        dec = m(x.to(dev))
        assert dec.is_cuda and tuple(dec.shape) == (B, 32, H, W)
        _report(f"darknet-{layers} {B}x{H}x{W} decoder", dec.cpu(), dec64, dec32)
        for agg in ("all", "sector", "depth"):
            got = m(x.to(dev), return_final_logits=True, agg_type=agg)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32
            _report(f"  {agg}", got, O.aggregate(dec64, agg), O.aggregate(dec32, agg))
        pooled = m(x.to(dev), return_logits=True)
        assert isinstance(pooled, np.ndarray) and pooled.shape == (B, 1024)
        _report("  return_logits", pooled, enc64.mean([2, 3]), enc32.mean([2, 3]))
        assert torch.equal(m(x.to(dev)), dec)                             # a repeat gives the same bits
        assert torch.equal(m(x[1:2].to(dev)), dec[1:2])                   # and so does the sample alone


def test_extractor_tree_against_float64(dev):
    """extractor.rangenet.RangeNet (darknet-21, 5 inputs): decoder map, 'lidargen' subsample, head logits (Co = 20)."""
    from lidargen.metrics.extractor.rangenet import RangeNet

    e = seeded_fill_rangenet(RangeNet(inputs=INPUTS5, num_classes=20, backbone=21), 2).eval().requires_grad_(False)
    x = rangenet_images(3, 16, 64, 32)
    sd = e.state_dict()
    dec64, log64 = O.extractor_forward(sd, 21, x, torch.float64)
    dec32, log32 = O.extractor_forward(sd, 21, x, torch.float32)
    e = e.to(dev)
    with torch.no_grad():
        _report("extractor decoder", e(x.to(dev), feature="decoder").cpu(), dec64, dec32)
        feats = e(x.to(dev), feature="lidargen")
        assert tuple(feats.shape) == (3, 4096)
        _report("extractor lidargen", feats.cpu(), O.subsample(dec64), O.subsample(dec32))
        logits = e(x.to(dev))
        assert tuple(logits.shape) == (3, 20, 16, 64)
        _report("extractor head", logits.cpu(), log64, log32)


def test_fixture_inputs_on_the_device(dev, golden):
    """The reference's recorded float32 outputs (tests/golden/rangenet.npz) against the HIP path, both trees."""
    from lidargen.metrics.extractor.rangenet import RangeNet

    gold = golden("rangenet")
    m = _model(53, 1).to(dev)
    e = seeded_fill_rangenet(RangeNet(inputs=INPUTS5, num_classes=20, backbone=21), 2).eval().requires_grad_(False).to(dev)
    with torch.no_grad():
        x = torch.from_numpy(gold["m_x"]).to(dev)
        assert max(O.rel_l2_per_sample(m(x).cpu(), gold["m_decoder"])) < TOL
        assert max(O.rel_l2_per_sample(m(x, return_final_logits=True), gold["m_depth"])) < TOL
        assert max(O.rel_l2_per_sample(m(x, return_logits=True), gold["m_logits"])) < TOL
        xe = torch.from_numpy(gold["e_x"]).to(dev)
        assert max(O.rel_l2_per_sample(e(xe, feature="lidargen").cpu(), gold["e_lidargen"])) < TOL
        assert max(O.rel_l2_per_sample(e(xe).cpu(), gold["e_head"])) < TOL


def test_weight_change_in_place_is_seen(dev):
    m = _model(21, 3).to(dev)
    x = rangenet_images(1, 16, 64, 33).to(dev)
    with torch.no_grad():
        a = m(x)
        packed = m.plan()._packed
        assert m.plan().packed(dev) is packed                             # nothing changed: nothing packed again
        m.backbone.enc2.residual_0.conv2.weight.mul_(0.5)
        b = m(x)
        assert not torch.equal(a, b)
        m.decoder.dec3.bn.running_var.add_(0.25)
        c = m(x)
        assert not torch.equal(b, c)
        sd = {k: v.cpu() for k, v in m.state_dict().items()}
        _, want = O.model_forward(sd, O.config(21), x.cpu(), torch.float64)
        assert max(O.rel_l2_per_sample(c.cpu(), want)) < TOL


# ---- front-ends ----------------------------------------------------------------------------------------------------
def _oracle_features(sd, clouds, dtype, size=(16, 64)):
    from lidargen.metrics import DATASET_CONFIG
    from lidargen.metrics import metric_utils as MU

    cfg = dict(DATASET_CONFIG["nuscenes"], size=list(size))
    x = torch.from_numpy(np.stack([MU.preprocess_range(c, **cfg) for c in clouds])).float()
    _, dec = O.model_forward(sd, O.config(21), x, dtype)
    return O.aggregate(dec, "depth").numpy()


def test_compute_range_logits_batches(dev, monkeypatch):
    from lidargen import metrics
    from lidargen.metrics import metric_utils as MU

    m = _model(21, 1).to(dev)
    clouds = [O.metre_cloud(70 + i) for i in range(5)]
    (whole,) = MU.compute_range_logits("32", clouds, model=m, size=(16, 64))
    assert whole.shape == (5, 512) and whole.dtype == np.float32
    monkeypatch.setitem(metrics.MODAL2BATCHSIZE, "range", 2)
    parts, empty = MU.compute_range_logits("32", clouds, [], model=m, size=(16, 64))
    assert np.array_equal(whole, parts) and empty.shape[0] == 0
    want = _oracle_features(m.state_dict(), clouds, torch.float64)
    assert max(O.rel_l2_per_sample(whole, want)) < TOL


def test_compute_frid_vs_float64_features(dev, capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils

    real = [O.metre_cloud(40 + i) for i in range(6)]
    fake = [O.metre_cloud(60 + i) * np.float32(0.8) for i in range(6)]
    m = _model(21, 1)
    sd = m.state_dict()
    f64 = [_oracle_features(sd, s, torch.float64) for s in (real, fake)]
    f32 = [_oracle_features(sd, s, torch.float32) for s in (real, fake)]
    want, want32 = O.compute_fd(*f64), O.compute_fd(*f32)
    limit = 4.0 * abs(want32 - want) / abs(want)
    m = m.to(dev)
    score = eval_utils.compute_frid(real, fake, "32", model=m, size=(16, 64))
    out = capsys.readouterr().out
    rel = abs(score - want) / abs(want)
    print(f"FRID {score!r} against {want!r}: relative {rel:.2e}; float32 oracle {limit / 4:.2e}; limit {limit:.2e}")
    assert "Evaluating (FRID) ..." in out and OUTPUT_TEMPLATE.format("FRID", score) in out
    assert rel < limit
    same = eval_utils.compute_frid(real, real, "32", model=m, size=(16, 64))
    assert abs(same) < 1e-6 * float(np.trace(np.cov(f64[0], rowvar=False)))


def test_compute_frd_vs_float64_features(dev, capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils
    from lidargen.metrics.distribution import compute_frechet_distance
    from lidargen.metrics.extractor.rangenet import Preprocess, RangeNet

    e = seeded_fill_rangenet(RangeNet(inputs=INPUTS5, num_classes=20, backbone=21), 2).eval().requires_grad_(False)
    pre, cols = Preprocess(), slice(0, 4096, 16)          # 256 of the 4096 columns: the matrix square root stays quick
    real, fake = rangenet_images(6, 16, 64, 81), rangenet_images(6, 16, 64, 82) * 0.8
    sd = e.state_dict()
    f64 = [O.subsample(O.extractor_forward(sd, 21, pre(s), torch.float64)[0]).numpy() for s in (real, fake)]
    f32 = [O.subsample(O.extractor_forward(sd, 21, pre(s), torch.float32)[0]).double().numpy() for s in (real, fake)]
    want = compute_frechet_distance(f64[0][:, cols], f64[1][:, cols])
    want32 = compute_frechet_distance(f32[0][:, cols], f32[1][:, cols])
    limit = 4.0 * abs(want32 - want) / abs(want)
    e = e.to(dev)
    feats = eval_utils.extract_range_features(e, pre, real.numpy(), batch_size=4)
    assert feats.shape == (6, 4096) and feats.dtype == np.float64
    assert max(O.rel_l2_per_sample(feats, f64[0])) < TOL
    score = eval_utils.compute_frd(real.to(dev), fake.to(dev), e, pre, batch_size=4, columns=cols)
    out = capsys.readouterr().out
    rel = abs(score - want) / abs(want)
    print(f"FRD {score!r} against {want!r}: relative {rel:.2e}; float32 oracle {limit / 4:.2e}; limit {limit:.2e}")
    assert "Evaluating (FRD) ..." in out and OUTPUT_TEMPLATE.format("FRD ", score) in out
    assert rel < limit
    assert eval_utils.compute_frd(feats, fake.to(dev), e, pre, columns=cols) == score       # a set may already be a feature matrix
    same = eval_utils.compute_frd(real.to(dev), real.to(dev), e, pre, columns=cols)
    assert abs(same) < 1e-6 * float(np.trace(np.cov(f64[0][:, cols], rowvar=False)))
