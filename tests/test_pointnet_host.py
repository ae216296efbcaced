"""CPU checks of the Frechet Point Distance pieces: the float64 restatement the GPU tests compare against
(tests/_pointnet_oracle.py) is itself pinned on the reference's recorded features (tests/golden/pointnet.npz), the module
surface (state-dict names, BatchNorm folding, refusals, checkpoint lookup), the host distances of distribution.py, and
the argument checks of the two new entry points (callable without a GPU)."""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnet_oracle as O  # noqa: E402

from lidarcrafter_amd.testing import pointnet_clouds, seeded_fill_pointnet  # noqa: E402

TOL = 2e-6          # relative L2 per cloud and per segment; the reference's own float32 run sits at 1.0e-7 ... 1.5e-7
LC_EINVAL, LC_EUNSUP = -1, -2


@pytest.fixture(scope="module")
def gold(golden):
    return golden("pointnet")


def _cases(gold):
    return [(i, tuple(int(v) for v in c)) for i, c in enumerate(gold["cases"])]


def test_oracle_matches_reference_features(gold):
    sd = O.seeded_state(int(gold["salt"]))
    for i, (B, N, seed) in _cases(gold):
        x = torch.from_numpy(gold[f"x_{i}"])
        assert x.shape == (B, 3, N)
        assert torch.equal(x, pointnet_clouds(B, N, seed))            # the generator the GPU tests draw from
        assert float((x == 0).all(dim=1).float().mean()) > 0.3        # a third of the points are (0,0,0)
        f, t = O.pointnet1(sd, x)
        ref = torch.from_numpy(gold[f"feat_{i}"]).double()
        assert f.shape == ref.shape == (B, 1808)
        for lo, hi in O.SEGMENTS:
            err = O.rel_l2_rows(f[:, lo:hi], ref[:, lo:hi])
            print(f"case {i} columns {lo}:{hi} rel-L2 per cloud {err.tolist()}")
            assert float(err.max()) < TOL, (i, lo, hi, err)
        assert float(O.rel_l2_rows(t, torch.from_numpy(gold[f"trans_{i}"]).double()).max()) < TOL


def test_trunk_oracle_is_the_modules_trunk(gold):
    """O.trunk on folded weights == the unfolded conv/bn chain of O._points_mlp (float64, both ReLU settings)."""
    from lidargen.metrics.extractor import PointNet1
    from lidargen.metrics.extractor.pointnet import fold_bn

    m = seeded_fill_pointnet(PointNet1(k=16), 1).eval()
    sd = m.state_dict()
    x = pointnet_clouds(2, 37, 11).double()
    for mod, prefix, relu3 in ((m.feat.stn, "feat.stn.", True), (m.feat, "feat.", False)):
        ws = [fold_bn(c.weight, c.bias, b, torch.float64) for c, b in mod._pairs()[:3]]
        got = O.trunk(x, None, *ws[0], *ws[1], *ws[2], relu3)
        want = O._points_mlp(sd, prefix, x, relu3)
        assert float(O.rel_l2_rows(got, want).max()) < 1e-13


def test_state_dict_names_shapes_and_checksums(gold):
    from lidargen.metrics.extractor import PointNet1

    m = seeded_fill_pointnet(PointNet1(k=16), int(gold["salt"]))
    sd = m.state_dict()
    assert len(sd) == 74
    assert list(sd.keys()) == [str(n) for n in gold["names"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in gold["shapes"]]
    mine = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])
    assert np.array_equal(mine, gold["checksums"])                    # both ends drew the same numbers
    for p in ("feat.stn.bn3.weight", "feat.bn3.weight"):
        neg = int((sd[p] < 0).sum())
        assert 100 < neg < 500, (p, neg)                              # a negative BatchNorm scale in front of each max
    assert float(sd["feat.bn1.running_mean"].abs().max()) > 0.1
    v = torch.cat([t.flatten() for k, t in sd.items() if k.endswith("running_var")])
    assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5


def test_fold_bn_matches_unfolded_modules():
    from lidargen.metrics.extractor import PointNet1
    from lidargen.metrics.extractor.pointnet import fold_bn

    m = seeded_fill_pointnet(PointNet1(k=16), 3).eval().double()
    g = torch.Generator().manual_seed(4)
    for mod in (m.feat.stn, m.feat, m):
        for lin, bn in mod._pairs():
            if bn is None:
                continue
            conv = isinstance(lin, torch.nn.Conv1d)
            x = torch.randn((5, lin.weight.shape[1], 7) if conv else (5, lin.weight.shape[1]), generator=g,
                            dtype=torch.float64)
            with torch.no_grad():
                want = bn(lin(x))
            w, b = fold_bn(lin.weight, lin.bias, bn, torch.float64)
            got = torch.einsum("oc,bcn->bon", w, x) + b[None, :, None] if conv else x @ w.T + b
            assert float((got - want).norm() / want.norm()) < 1e-14
            assert w.shape == (lin.weight.shape[0], lin.weight.shape[1])
    assert int((m.feat.bn3.weight < 0).sum()) > 0                    # negative scales were part of that
    w32, b32 = fold_bn(m.feat.conv3.weight, m.feat.conv3.bias, m.feat.bn3)
    assert w32.dtype == b32.dtype == torch.float32 and w32.is_contiguous()


def test_folded_cache_follows_the_weights():
    """The fold is kept under every tensor's (address, _version): load_state_dict and in-place edits fold again."""
    from lidargen.metrics.extractor import PointNet1

    m = seeded_fill_pointnet(PointNet1(k=16), 1).eval()
    a = m.feat.folded()
    assert m.feat.folded() is a
    with torch.no_grad():
        m.feat.bn2.running_var.mul_(2.0)
    b = m.feat.folded()
    assert b is not a and not torch.equal(a[1][0], b[1][0]) and torch.equal(a[0][0], b[0][0])
    m.load_state_dict(O.seeded_state(2))
    c = m.feat.folded()
    assert c is not b and not torch.equal(c[2][0], b[2][0])
    s = m.feat.stn.folded()
    with torch.no_grad():
        m.feat.stn.fc3.bias.add_(1.0)
    assert m.feat.stn.folded() is not s


def test_refusals():
    from lidargen.metrics.extractor import PointNet1, PointNetfeat, STN3d

    m = seeded_fill_pointnet(PointNet1(k=16), 1)
    x = torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(x)
    m.eval()
    for mod in (m, m.feat, m.feat.stn, STN3d().eval()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(x)
    with pytest.raises(NotImplementedError):
        PointNetfeat(global_feat=False)
    m.feat.global_feat = False
    with pytest.raises(NotImplementedError):
        m(x)
    with pytest.raises(NotImplementedError):
        m.feat(x)


def test_pretrained_pointnet_reads_a_local_file_only(tmp_path, monkeypatch):
    from lidargen.metrics.extractor import pointnet as P

    missing = tmp_path / "nothing" / "cls_model_39.pth"
    with pytest.raises(FileNotFoundError) as e:
        P.pretrained_pointnet(checkpoint=missing)
    assert str(missing) in str(e.value)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    want = os.path.join(str(tmp_path / "hub"), "checkpoints", "cls_model_39.pth")
    with pytest.raises(FileNotFoundError) as e:
        P.pretrained_pointnet()
    assert want in str(e.value)
    with pytest.raises(ValueError):
        P.pretrained_pointnet(dataset="modelnet")
    sd = O.seeded_state(1)
    os.makedirs(os.path.dirname(want))
    torch.save(sd, want)
    for kw in ({}, {"checkpoint": want, "compile": False}):
        m = P.pretrained_pointnet(**kw)
        assert not m.training and not any(p.requires_grad for p in m.parameters())
        got = m.state_dict()
        assert all(torch.equal(got[k], sd[k]) for k in sd) and len(got) == len(sd)


def test_module_names_no_downloader():
    """Nothing in the extractor imports or calls anything that fetches: no url / download / request name in its code
    (docstrings and comments are not code)."""
    from lidargen.metrics.extractor import pointnet as P

    tree = ast.parse(open(P.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module or "")
            names.update(a.name for a in node.names)
        elif isinstance(node, ast.Name):
            names.add(node.id)
        elif isinstance(node, ast.Attribute):
            names.add(node.attr)
    bad = [n for n in names if any(w in n.lower() for w in ("url", "download", "request", "http", "socket"))]
    assert not bad, bad


def test_distribution_matches_reference_numbers(gold):
    from lidargen.metrics import distribution as D

    a, b = gold["dist_a"], gold["dist_b"]
    assert a.shape == (40, 24) and b.shape == (50, 24)
    fd = D.compute_frechet_distance(a, b)
    assert abs(fd - float(gold["frechet"])) <= 1e-10 * abs(float(gold["frechet"]))
    np.random.seed(0)
    mmd = D.compute_squared_mmd(a, b, num_subsets=5, max_subset_size=30)
    assert abs(mmd - float(gold["squared_mmd"])) <= 1e-12 * abs(float(gold["squared_mmd"]))
    assert D.compute_frechet_distance(a, a) < 1e-8 * fd               # a set against itself
    with pytest.raises(AssertionError):
        D.compute_frechet_distance(a, b[:, :20])


def test_compute_fpd_on_feature_matrices(gold, capsys):
    """Both arguments already feature matrices: no model, no GPU; the line is the template's."""
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils

    a, b = gold["dist_a"], gold["dist_b"]
    score = eval_utils.compute_fpd(a, b, model=None)
    assert abs(score - float(gold["frechet"])) <= 1e-10 * abs(float(gold["frechet"]))
    assert OUTPUT_TEMPLATE.format("FPD ", score) in capsys.readouterr().out
    sub = eval_utils.compute_fpd(a, b, model=None, columns=slice(0, 8))
    from lidargen.metrics.distribution import compute_frechet_distance
    assert sub == compute_frechet_distance(a[:, :8], b[:, :8])
    with pytest.raises(NotImplementedError):
        eval_utils.evaluate([], [], ["frid"], "nuscenes")             # FRD stays refused
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_utils.extract_point_features(None, [torch.zeros(5, 3)])


def test_entry_points_refuse_bad_arguments():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(x=p, x_bs=3 * 8, trans=None, w1=p, b1=p, w2=p, b2=p, w3=p, b3=p, y=p, y_bs=1024, B=1, N=8, scratch=p):
        return h.lc_pointnet_trunk_fwd(x, x_bs, trans, w1, b1, w2, b2, w3, b3, 0, y, y_bs, B, N, scratch, None)

    for name in ("x", "w1", "b1", "w2", "b2", "w3", "b3", "y", "scratch"):
        assert call(**{name: None}) == LC_EINVAL, name
    assert call(B=0) == LC_EINVAL and call(N=0) == LC_EINVAL and call(B=-3) == LC_EINVAL
    assert call(B=65536, x_bs=24) == LC_EUNSUP
    assert call(N=1 << 24, x_bs=3 << 24) == LC_EUNSUP
    assert call(x_bs=3 * 8 - 1) == LC_EUNSUP                          # clouds overlap
    assert call(y_bs=1023) == LC_EUNSUP                               # rows of y overlap
    off = ctypes.c_void_p(p.value + 4)
    assert call(w2=off) == LC_EUNSUP and call(w3=off) == LC_EUNSUP    # rows read as 128-bit quads


def test_scratch_elems_positive_and_monotone():
    from lidarcrafter_amd import ops_pointnet as KP

    T = KP.TILE
    assert KP.trunk_scratch_elems(1, 1) == 1024 and KP.trunk_scratch_elems(1, T) == 1024
    assert KP.trunk_scratch_elems(1, T + 1) == 2048                   # ops_pointnet.TILE is the kernel's tile
    prev = 0
    for N in sorted((1, 37, T - 1, T, T + 1, 1000, 4 * T + 3, 32768, (1 << 24) - 1)):
        cur = KP.trunk_scratch_elems(1, N)
        assert cur > 0 and cur >= prev
        assert [KP.trunk_scratch_elems(B, N) for B in (1, 2, 5, 16)] == [cur * B for B in (1, 2, 5, 16)]
        prev = cur
    assert KP.trunk_scratch_elems(65535, (1 << 24) - 1) == 65535 * (1 << 17) * 1024   # no 32-bit overflow
    assert KP.trunk_scratch_elems(0, 5) == 0 and KP.trunk_scratch_elems(5, 0) == 0
