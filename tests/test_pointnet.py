"""GPU tests of the fused PointNet trunk (csrc/pointnet.hip), the PointNet1 extractor built on it and the Frechet Point
Distance front-end, against the float64 restatement of tests/_pointnet_oracle.py (itself pinned on the reference's
recorded features by tests/test_pointnet_host.py).  `pytest -m gpu`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnet_oracle as O  # noqa: E402

from lidarcrafter_amd import ops_pointnet as KP  # noqa: E402
from lidarcrafter_amd.testing import pointnet_clouds, seeded_randn, synth_points  # noqa: E402
from tests._profile_cases import TOL_CONV  # noqa: E402   2e-6: the project's tolerance for its fp32-accurate convolutions

pytestmark = pytest.mark.gpu
T = KP.TILE
SHAPES = [(1, 1), (2, 37), (3, T - 1), (3, T), (3, T + 1), (2, 1000), (1, 4 * T + 3)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _trunk_weights(seed=0):
    """Folded weights of one trunk as a checkpoint may leave them: mixed signs, rows of W3 of very different scale."""
    w1, b1 = seeded_randn(64, 3, seed=seed + 1) / 3 ** 0.5, 0.3 * seeded_randn(64, seed=seed + 2)
    w2, b2 = seeded_randn(128, 64, seed=seed + 3) / 8.0, 0.3 * seeded_randn(128, seed=seed + 4)
    w3 = seeded_randn(1024, 128, seed=seed + 5) / 128 ** 0.5 * torch.exp(seeded_randn(1024, 1, seed=seed + 6))
    b3 = 0.3 * seeded_randn(1024, seed=seed + 7)
    return [t.contiguous() for t in (w1, b1, w2, b2, w3, b3)]


def _trans(B, seed):
    return (torch.eye(3)[None] + 0.3 * seeded_randn(B, 3, 3, seed=seed)).contiguous()


def _run_trunk(dev, x, trans, ws, relu3, **kw):
    y = KP.pointnet_trunk(x.to(dev), None if trans is None else trans.to(dev), *[w.to(dev) for w in ws], relu3, **kw)
    torch.cuda.synchronize()
    return y


def _check_rows(got, ref, what, tol=TOL_CONV):
    err = O.rel_l2_rows(got, ref)
    print(f"{what}: rel-L2 per cloud {[f'{e:.2e}' for e in err.tolist()]}")
    assert float(err.max()) < tol, (what, err.tolist())


@pytest.mark.parametrize("relu3", [0, 1])
@pytest.mark.parametrize("with_trans", [False, True], ids=["plain", "trans"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_trunk_vs_float64(dev, B, N, with_trans, relu3):
    ws = _trunk_weights()
    x = pointnet_clouds(B, N, seed=7 * B + N)
    trans = _trans(B, 99 + N) if with_trans else None
    y = _run_trunk(dev, x, trans, ws, bool(relu3))
    assert y.shape == (B, 1024) and bool(torch.isfinite(y).all())
    _check_rows(y, O.trunk(x, trans, *ws, bool(relu3)), f"trunk B={B} N={N} trans={with_trans} relu3={relu3}")


def test_trunk_maximum_in_the_partial_last_tile(dev):
    """The last point, alone in a partial tile, is far from the others: most channel maxima sit there."""
    ws = _trunk_weights(10)
    B, N = 2, 2 * T + 1
    x = pointnet_clouds(B, N, seed=3)
    x[:, :, -1] = torch.tensor([[4.0, -3.0, 5.0], [-6.0, 2.0, 3.0]])
    ref = O.trunk(x, None, *ws, False)
    alone = O.trunk(x[:, :, -1:], None, *ws, False)
    assert int((ref == alone).sum()) > B * 256                       # those maxima are the last point's
    assert int((ref != alone).sum()) > B * 64                        # and the others are not
    _check_rows(_run_trunk(dev, x, None, ws, False), ref, "maximum in the last, partial tile")
    # a lane past N must not count: the same clouds without that point
    _check_rows(_run_trunk(dev, x[:, :, :-1].contiguous(), None, ws, False), O.trunk(x[:, :, :-1], None, *ws, False),
                "last tile dropped")


def test_trunk_all_zero_cloud(dev):
    """(0,0,0) is a point: a cloud of nothing else gives the network's response to the origin, not -inf or 0."""
    ws = _trunk_weights(20)
    x = pointnet_clouds(3, T + 9, seed=5)
    x[1] = 0.0
    for trans in (None, _trans(3, 6)):
        ref = O.trunk(x, trans, *ws, False)
        assert float(ref[1].abs().min()) > 0.0
        y = _run_trunk(dev, x, trans, ws, False)
        _check_rows(y, ref, "all-zero cloud")
        one = _run_trunk(dev, torch.zeros(1, 3, 1), None, ws, False)   # N does not matter for such a cloud
        if trans is None:
            assert torch.equal(one[0], y[1])


@pytest.mark.parametrize("N", [37, 4 * T + 3])
def test_scratch_content_does_not_matter(dev, N):
    ws = _trunk_weights(30)
    x = pointnet_clouds(2, N, seed=8)
    n = KP.trunk_scratch_elems(2, N)
    base = _run_trunk(dev, x, None, ws, True)
    for fill in (float("inf"), float("nan")):
        scratch = torch.full((n,), fill, device=dev)
        y = _run_trunk(dev, x, None, ws, True, scratch=scratch)
        assert torch.equal(y, base), fill
        assert bool(torch.isfinite(scratch).all())                    # every word of it was written
    with pytest.raises(ValueError, match="workspace"):
        KP.pointnet_trunk(x.to(dev), None, *[w.to(dev) for w in ws], True, scratch=torch.empty(n - 1, device=dev))


def test_output_stride_leaves_other_columns(dev):
    ws = _trunk_weights(40)
    x = pointnet_clouds(3, 200, seed=9)
    out = torch.full((3, 1808), -7.25, device=dev)
    y = _run_trunk(dev, x, None, ws, False, out=out)
    assert y is out and bool((out[:, 1024:] == -7.25).all())
    assert torch.equal(out[:, :1024], _run_trunk(dev, x, None, ws, False))


def test_batch_independence_and_repeatability(dev):
    """Cloud c alone and as member 3 of a batch of 5: identical bits, on the trunk and on the full features."""
    from lidargen.metrics.extractor import PointNet1

    ws = _trunk_weights(50)
    x = pointnet_clouds(5, 3 * T + 17, seed=10)
    trans = _trans(5, 11)
    y5 = _run_trunk(dev, x, trans, ws, False)
    y1 = _run_trunk(dev, x[3:4].contiguous(), trans[3:4].contiguous(), ws, False)
    assert torch.equal(y5[3], y1[0])
    assert torch.equal(y5, _run_trunk(dev, x, trans, ws, False))
    m = PointNet1(k=16)
    m.load_state_dict(O.seeded_state(1))
    m = m.eval().to(dev)
    f5, f1 = m(x.to(dev)), m(x[3:4].to(dev))
    assert torch.equal(f5[3], f1[0])
    assert torch.equal(f5, m(x.to(dev)))
    t5, t1 = m.feat.stn(x.to(dev)), m.feat.stn(x[3:4].to(dev))
    assert torch.equal(t5[3], t1[0])


def _check_features(got, ref, what):
    assert got.shape == ref.shape
    for lo, hi in O.SEGMENTS:
        _check_rows(got[:, lo:hi], ref[:, lo:hi], f"{what} columns {lo}:{hi}")


@pytest.mark.parametrize("B,N,seed", [(2, 37, 11), (3, 1000, 12)])
def test_pointnet1_vs_float64(dev, B, N, seed):
    from lidargen.metrics.extractor import PointNet1

    x, ref, ref_trans = O.case(1, B, N, seed)
    m = PointNet1(k=16)
    m.load_state_dict(O.seeded_state(1))
    m = m.eval().to(dev)
    f = m(x.to(dev))
    assert f.shape == (B, 1808) and f.dtype == torch.float32
    _check_features(f, ref, f"PointNet1 B={B} N={N}")
    x1, trans = m.feat(x.to(dev))
    assert torch.equal(x1, f[:, :1024]) and trans.shape == (B, 3, 3)
    _check_rows(trans, ref_trans, "trans")
    _check_rows(m.feat.stn(x.to(dev)), ref_trans, "STN3d")


def test_call_sequence_follows_the_weights(dev):
    """A result depends on the weights and the input of its own call only: load_state_dict, an in-place edit of a
    BatchNorm buffer and a change of shape in between all show, and nothing of an earlier call stays."""
    from lidargen.metrics.extractor import PointNet1

    a = (2, 37, 11)
    b = (3, 300, 14)
    m = PointNet1(k=16)
    m.load_state_dict(O.seeded_state(1))
    m = m.eval().to(dev)
    xa, ref, _ = O.case(1, *a)
    _check_features(m(xa.to(dev)), ref, "first weights")
    m.load_state_dict(O.seeded_state(2))
    _check_features(m(xa.to(dev)), O.case(2, *a)[1], "after load_state_dict")
    with torch.no_grad():
        m.feat.bn2.running_var.mul_(1.7)
        m.feat.stn.bn4.running_mean.add_(0.2)
    sd = dict(O.seeded_state(2))
    sd["feat.bn2.running_var"] = sd["feat.bn2.running_var"] * 1.7
    sd["feat.stn.bn4.running_mean"] = sd["feat.stn.bn4.running_mean"] + 0.2
    ref_a = O.pointnet1(sd, xa)[0]
    assert float(O.rel_l2_rows(ref_a, O.case(2, *a)[1]).min()) > 1e-3          # the edit is visible at all
    fa = m(xa.to(dev))
    _check_features(fa, ref_a, "after in-place edits")
    xb = pointnet_clouds(*b)
    _check_features(m(xb.to(dev)), O.pointnet1(sd, xb)[0], "another shape")
    fa2 = m(xa.to(dev))
    _check_features(fa2, ref_a, "the first shape again")
    assert torch.equal(fa, fa2)


def _metre_clouds(n, N, seed, stretch=1.0):
    return [synth_points(N, seed + i)[:, :3] * np.float32(stretch) for i in range(n)]


def test_extract_point_features_keeps_input_order(dev):
    from lidargen.metrics import eval_utils
    from lidargen.metrics.extractor import PointNet1

    m = PointNet1(k=16)
    m.load_state_dict(O.seeded_state(1))
    m = m.eval().to(dev)
    lens = [100, 137, 100, 100, 137, 100, 137]
    clouds = [synth_points(n, 40 + i)[:, :3] for i, n in enumerate(lens)]
    clouds[2] = torch.from_numpy(clouds[2]).to(dev)                   # tensors and arrays mix
    feats = eval_utils.extract_point_features(m, clouds, batch_size=2)
    assert feats.shape == (7, 1808) and feats.dtype == np.float64
    for i, c in enumerate(clouds):
        c = torch.as_tensor(c).to(dev)
        one = m((c.float() * (1 / 80.0)).t()[None].contiguous())[0].double().cpu().numpy()
        assert np.array_equal(feats[i], one), i                       # batch-independent bits make this exact
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_utils.extract_point_features(m, [torch.zeros(5, 3)])


def test_compute_fpd_vs_float64_features(dev, capsys):
    """48 + 48 clouds of 512 points; the distance on the first 32 feature columns (fewer samples than the 1808 columns
    would leave the matrix square root of a rank-deficient product in charge)."""
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils
    from lidargen.metrics.distribution import compute_frechet_distance
    from lidargen.metrics.extractor import PointNet1

    m = PointNet1(k=16)
    m.load_state_dict(O.seeded_state(1))
    m = m.eval().to(dev)
    real, fake = _metre_clouds(48, 512, 100), _metre_clouds(48, 512, 200, stretch=0.8)
    sd = O.seeded_state(1)

    def oracle(clouds):
        x = torch.from_numpy(np.stack([c.T for c in clouds])) * (1 / 80.0)     # float32, as the front-end scales
        return torch.cat([O.pointnet1(sd, x[i:i + 16])[0] for i in range(0, len(clouds), 16)]).numpy()

    want = compute_frechet_distance(oracle(real)[:, :32], oracle(fake)[:, :32])
    cols = slice(0, 32)
    score = eval_utils.compute_fpd(real, fake, m, batch_size=16, columns=cols)
    out = capsys.readouterr().out
    print(f"FPD {score!r} against {want!r}: relative {abs(score - want) / abs(want):.2e}")
    assert "Evaluating (FPD) ..." in out and OUTPUT_TEMPLATE.format("FPD ", score) in out
    assert abs(score - want) <= 1e-4 * abs(want)
    # the real set's features may be passed in their place (the evaluator caches them)
    fr = eval_utils.extract_point_features(m, real)
    assert eval_utils.compute_fpd(fr, fake, m, columns=cols) == score
