"""CPU tests of the PointMLP object extractor's host side: the import line, the state-dict tables, the oracle of
tests/_pointmlp_oracle.py against the reference's recorded run (tests/golden/pointmlp.npz), the refusals, the dataset and
the CGF / DCF host code, and the mutation check that sizes the GPU tests' bound."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointmlp_oracle as O  # noqa: E402

from lidarcrafter_amd.testing import seeded_fill_pointmlp  # noqa: E402

TINY = dict(points=64, class_num=4, embed_dim=16, k_neighbors=[4, 4], reducers=[2, 2], pre_blocks=[1, 1], pos_blocks=[1, 1],
            dim_expansion=[2, 2], bias=False, use_xyz=False, normalize="anchor")
CASES = {"full": 1, "elite": 2, "tiny": 3}      # case -> salt of the seeded fill


def make(name):
    from lidargen.metrics.extractor import pointmlp as P

    m = {"full": lambda: P.pointMLP(4), "elite": lambda: P.pointMLPElite(4), "tiny": lambda: P.Model(**TINY)}[name]()
    return seeded_fill_pointmlp(m, CASES[name]).eval().requires_grad_(False)


def fixture_tables(gold, name, stages):
    return [(gold[f"{name}_fps{i}"], gold[f"{name}_knn{i}"]) for i in range(stages)]


_F64 = {}


def oracle64(gold, name):
    """(model, cfg, float64 features, float64 logits) on the fixture's clouds and tables, computed once per case."""
    if name not in _F64:
        m = make(name)
        cfg = O.config_of(m)
        f, l = O.forward(m.state_dict(), cfg, torch.from_numpy(gold[f"{name}_x"]), fixture_tables(gold, name, len(cfg[0])))
        _F64[name] = (m, cfg, f, l)
    return _F64[name]


def test_reference_import_line_resolves():
    from lidargen.ops.pointnet2.pointnet2_batch import pointnet2_utils
    from lidargen.metrics.extractor import pointmlp as P
    from lidargen.metrics.extractor.pointmlp import pointMLP  # noqa: F401  (fg_object.py's import)
    from lidargen.metrics.datasets.nuscenes_object_dataset import NuscObject  # noqa: F401

    assert pointnet2_utils.furthest_point_sample is pointnet2_utils.farthest_point_sample
    for n in ("get_activation", "LocalGrouper", "ConvBNReLU1D", "ConvBNReLURes1D", "PreExtraction", "PosExtraction", "Model",
              "pointMLP", "pointMLPElite"):
        assert hasattr(P, n), n
    assert P.pointnet2_utils is pointnet2_utils


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_tables_equal_the_reference(golden, name):
    gold = golden("pointmlp")
    sd = make(name).state_dict()
    assert list(sd.keys()) == gold[f"{name}_names"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == gold[f"{name}_shapes"].tolist()
    sums = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])
    assert np.array_equal(sums, gold[f"{name}_checksums"])             # the same draw as the generator's
    if name == "full":
        assert len(sd) == 246 and sum(p.numel() for p in make(name).parameters()) == 13229252


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_geometry_against_the_reference_run(golden, name):
    gold = golden("pointmlp")
    m = make(name)
    groups, kn, _, _ = O.config_of(m)
    xyz = np.ascontiguousarray(gold[f"{name}_x"].transpose(0, 2, 1))
    for i, (f, k) in enumerate(O.geometry(xyz, groups, kn)):
        assert np.array_equal(f, gold[f"{name}_fps{i}"]), (name, i)     # picks: index for index
        for b in range(xyz.shape[0]):
            assert O.same_neighbour_coordinates(xyz[b], k[b], gold[f"{name}_knn{i}"][b]), (name, i, b)
        xyz = np.stack([c[j] for c, j in zip(xyz, f)])


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_network_against_the_reference_run(golden, name):
    """The float64 oracle is the reference's float64 copy: the recorded float32 outputs lie at the recorded distance."""
    gold = golden("pointmlp")
    _, _, f64, l64 = oracle64(gold, name)
    ef, el = O.rel_l2_per_sample(gold[f"{name}_feat"], f64), O.rel_l2_per_sample(gold[f"{name}_logits"], l64)
    print(name, "features", ef, "recorded", gold[f"{name}_feat_err"], "logits", el, "recorded", gold[f"{name}_logit_err"])
    assert np.allclose(ef, gold[f"{name}_feat_err"], rtol=1e-3, atol=1e-12)
    assert np.allclose(el, gold[f"{name}_logit_err"], rtol=1e-3, atol=1e-12)
    assert max(ef) < 2e-6 and max(el) < 2e-6


def test_oracle_with_its_own_tables_gives_the_same_features(golden):
    """Tied points carry equal coordinates and equal features: the (distance, index) tables change nothing."""
    gold = golden("pointmlp")
    m, cfg, f64, _ = oracle64(gold, "tiny")
    x = gold["tiny_x"]
    own = O.geometry(np.ascontiguousarray(x.transpose(0, 2, 1)), cfg[0], cfg[1])
    f, _ = O.forward(m.state_dict(), cfg, torch.from_numpy(x), own)
    assert max(O.rel_l2_per_sample(f, f64)) < 1e-14


def test_fps_restatement_tie_rule():
    """Among equal maxima the reference's tree prefers the smallest bit-reversed thread index, then the smallest k."""
    def rev(v, bits):
        return int(format(v, f"0{bits}b")[::-1], 2) if bits else 0

    for N, M, real in ((64, 20, 21), (1000, 40, 333), (1025, 7, 400), (7, 7, 2), (2500, 12, 700)):
        c = O.clouds(1, N, N, real=[real])[0]
        bs = O.block_size(N)
        bits = bs.bit_length() - 1
        temp, old, want = np.full(N, 1e10, np.float32), 0, [0]
        for _ in range(1, M):
            temp = np.minimum(O.sqdist(c, c[old]), temp)
            cand = np.flatnonzero(temp == temp.max())
            old = int(min(cand, key=lambda k: (rev(int(k) % bs, bits), int(k))))
            want.append(old)
        assert O.fps(c, M).tolist() == want, N
    assert O.fps(np.zeros((5, 3), np.float32), 4).tolist() == [0, 0, 0, 0]        # no distinct point left: index 0 repeats


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    from lidargen.metrics.extractor import pointmlp as P
    from lidargen.ops.pointnet2.pointnet2_batch import pointnet2_utils as U

    ok = dict(TINY)
    with pytest.raises(NotImplementedError, match="groups = 2"):
        P.Model(**dict(ok, groups=2))
    with pytest.raises(NotImplementedError, match="groups = 2"):
        P.ConvBNReLURes1D(16, groups=2)
    for act in ("gelu", "rrelu", "selu", "silu", "hardswish", "leakyrelu", "GELU"):
        with pytest.raises(NotImplementedError, match=f"'{act}' is not built"):
            P.Model(**dict(ok, activation=act))
    with pytest.raises(NotImplementedError, match="use_xyz=True"):
        P.Model(**dict(ok, use_xyz=True))
    for norm in ("center", None, "batch"):
        with pytest.raises(NotImplementedError, match="normalize"):
            P.Model(**dict(ok, normalize=norm))
    with pytest.raises(NotImplementedError, match="kernel_size = 3"):
        P.ConvBNReLU1D(3, 8, kernel_size=3)
    assert isinstance(P.get_activation("relu"), torch.nn.ReLU)
    m = P.Model(**ok)
    x = torch.zeros(1, 3, 64)
    with pytest.raises(NotImplementedError, match="training mode"):
        m(x)
    m.eval()
    with pytest.raises(NotImplementedError, match="grad mode"):
        m(x)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="CPU tensors"):
            m(x)
    m.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        m(x)
    for sub in (m.embedding, m.local_grouper_list[0], m.pre_blocks_list[0], m.pos_blocks_list[0],
                m.pre_blocks_list[0].operation[0]):
        with pytest.raises(NotImplementedError, match="forward is not built on its own"):
            sub(x)
    for name, word in (("ball_query", "ball query"), ("grouping_operation", "grouping"), ("three_nn", "three-NN"),
                       ("three_interpolate", "interpolate"), ("gather_operation", "gather")):
        with pytest.raises(NotImplementedError, match=f"{name}: {word}"):
            getattr(U, name)(x)
    with pytest.raises(NotImplementedError, match="QueryAndGroup"):
        U.QueryAndGroup(0.1, 4)
    with pytest.raises(NotImplementedError, match="GroupAll"):
        U.GroupAll()
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        U.furthest_point_sample(torch.zeros(1, 8, 3), 4)


def test_bias_is_folded_not_refused():
    from lidargen.metrics.extractor import pointmlp as P

    m = seeded_fill_pointmlp(P.Model(**dict(TINY, bias=True)), 4).eval()
    assert "embedding.net.0.bias" in m.state_dict()
    (w, b), = m.folded()[:1]
    ow, ob = O.fold(m.state_dict(), "embedding.net.0", "embedding.net.1", torch.float32)
    assert torch.equal(w, ow) and torch.equal(b, ob) and float(m.embedding.net[0].bias.detach().abs().max()) > 0
    n = len(m.folded())
    assert m.folded() is m.folded()
    first = m.folded()
    with torch.no_grad():
        m.embedding.net[1].running_var.add_(0.5)                          # an in-place edit of a buffer folds again
    again = m.folded()
    assert again is not first and len(again) == n and not torch.equal(again[0][0], first[0][0])
    with torch.no_grad():
        m.local_grouper_list[1].affine_alpha.mul_(2.0)
    assert m.folded() is not again


def test_pretrained_pointmlp_reads_net_and_never_fetches(tmp_path):
    from lidargen.metrics import fg_object as F

    missing = tmp_path / "none.pth"
    with pytest.raises(FileNotFoundError, match=str(missing)):
        F.pretrained_pointmlp(missing, device="cpu")
    sd = make("full").state_dict()
    path = tmp_path / "nusc_object_classification_model.pth"
    torch.save({"net": {"module." + k: v for k, v in sd.items()}, "epoch": 3}, path)
    net = F.pretrained_pointmlp(path, device="cpu")
    assert not net.training and all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    assert not any(p.requires_grad for p in net.parameters())


# ---- host pieces -------------------------------------------------------------------------------------------------------
def _write_objects(tmp_path, width):
    g = np.random.default_rng(3)
    infos = []
    for i, (n, name) in enumerate(((30, "car"), (80, "bus"), (50, "bicycle"))):
        pts = g.normal(size=(n, width)).astype(np.float32)
        p = tmp_path / f"obj{i}_{width}.bin"
        pts.tofile(p)
        infos.append({"path": str(p) if width == 4 else p.name, "name": name, "num_points_in_gt": n,
                      "box3d_lidar": [0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.3 * i, 0.0, 0.0], "_pts": pts})
    return infos


def test_norm_fg_points_against_the_reference(golden):
    from lidargen.metrics.datasets.nuscenes_object_dataset import NuscObject

    gold = golden("pointmlp")
    ds = NuscObject.__new__(NuscObject)
    got = ds.norm_fg_points(gold["norm_points"].copy(), gold["norm_box"])
    assert got.dtype == np.float32 and np.abs(got - gold["norm_out"]).max() < 1e-6


@pytest.mark.parametrize("form", ["pkl_path", "ori"])
def test_nusc_object_forms_pad_and_truncate(tmp_path, form):
    from lidargen.metrics.datasets.nuscenes_object_dataset import NuscObject

    infos = _write_objects(tmp_path, 4 if form == "pkl_path" else 5)
    stored = [{k: v for k, v in i.items() if k != "_pts"} for i in infos]
    pkl = tmp_path / "infos.pkl"
    if form == "pkl_path":
        with open(pkl, "wb") as f:
            pickle.dump({"car": [stored[0]], "bus": [stored[1]], "bicycle": [stored[2]]}, f)
        mk = lambda **kw: NuscObject(num_points=40, partition="val", pkl_path=str(pkl), **kw)  # noqa: E731
        n = 2                                                             # 'bicycle' is not among the class names
    else:
        with open(pkl, "wb") as f:
            pickle.dump(stored, f)
        mk = lambda **kw: NuscObject(num_points=40, partition="val", info_path=str(pkl), data_root=str(tmp_path), **kw)  # noqa: E731
        n = 3
    ds = mk(generator=np.random.default_rng(7))
    assert len(ds) == n and ds.dataset_type == ("custom" if form == "pkl_path" else "ori")
    pts, label, count = ds[0]
    assert pts.shape == (40, 3) and pts.dtype == np.float32 and int(label) == 1 and int(count) == 30
    assert np.all(pts[30:] == 0.0) and np.all(np.abs(pts[:30]).sum(1) > 0)        # padded behind the shuffled points
    want = ds.norm_fg_points(infos[0]["_pts"][:, :3].copy(), infos[0]["box3d_lidar"][:7])
    assert np.array_equal(np.sort(pts[:30], axis=0), np.sort(want, axis=0))
    pts1, label1, _ = ds[1]
    assert pts1.shape == (40, 3) and int(label1) == 3 and np.all(np.abs(pts1).sum(1) > 0)   # 80 points truncated to 40
    if form == "ori":
        assert int(ds[2][1]) == 0                                         # a class outside the names: background
    again = mk(generator=np.random.default_rng(7))
    assert np.array_equal(again[0][0], pts) and np.array_equal(again[1][0], pts1)  # the shuffle is the generator's
    with pytest.raises(FileNotFoundError, match="no info file"):
        NuscObject(pkl_path=str(tmp_path / "absent.pkl"))


def test_cgf_and_dcf_against_the_fixture(golden, capsys):
    from lidargen.metrics import fg_object as F

    gold = golden("pointmlp")
    res = {"class_names": ["unknow", "car", "truck", "bus"], "test_true": gold["cgf_true"], "test_pred": gold["cgf_pred"],
           "num_points_in_gt": gold["cgf_pts"]}
    out = F.compute_cgf_from_results(res)
    assert out["overall"]["accuracy"] == float(gold["cgf_overall"])
    for lbl, acc in zip(F.FIXED_LABELS, gold["cgf_bins"]):
        if np.isnan(acc):
            assert lbl not in out["partitions"]
        else:
            assert out["partitions"][lbl]["accuracy"] == float(acc)
    assert sum(p["count"] for p in out["partitions"].values()) == len(gold["cgf_true"])
    dcf = F.compute_dcf(json.loads(str(gold["dcf_input"])))
    assert dcf == dict(zip(gold["dcf_names"].tolist(), gold["dcf_scores"].tolist()))
    assert "Average confidence per class:" in capsys.readouterr().out


@pytest.mark.parametrize("Co,Ci", [(1, 1), (20, 3), (32, 32), (33, 65), (65, 33)])
def test_packed_weights_are_rangenet_1x1s(Co, Ci):
    """One packed-weight layout (csrc/dense_f32.h): the pointwise packer is RangeNet's at one tap and chunks of 32."""
    from lidarcrafter_amd import ops_pointmlp as KM, ops_rangenet as KR

    w = torch.randn(Co, Ci, generator=torch.Generator().manual_seed(100 * Co + Ci))
    assert KM.packed_weight_elems(Ci, Co) == KR.packed_weight_elems(0, Ci, Co)
    assert torch.equal(KM.pack_weight(w), KR.pack_weight(w[:, :, None, None], 0))


# ---- what the GPU bound can see ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "elite"])
def test_mutations_move_the_features_by_16_bounds(golden, name):
    """The GPU tests hold the HIP path to 3 x the reference float32 module's own error.  One replaced neighbour index, or the
    + 1e-5 dropped from the normalisation, moves the float64 features by at least 16 such bounds."""
    gold = golden("pointmlp")
    m, cfg, f64, _ = oracle64(gold, name)
    x = torch.from_numpy(gold[f"{name}_x"])
    tables = fixture_tables(gold, name, len(cfg[0]))
    bound = 3.0 * gold[f"{name}_feat_err"]
    f_eps, _ = O.forward(m.state_dict(), cfg, x, tables, mutate="eps")
    moved = np.array(O.rel_l2_per_sample(f_eps, f64)) / bound
    print(name, "eps dropped:", moved, "bounds")
    assert moved.min() >= 16.0
    swapped = [(f.copy(), k.copy()) for f, k in tables]
    swapped[0][1][0, 3, 1] = (swapped[0][1][0, 3, 1] + 17) % x.shape[2]
    swapped[0][1][1, 3, 1] = 2
    f_idx, _ = O.forward(m.state_dict(), cfg, x, swapped)
    moved = np.array(O.rel_l2_per_sample(f_idx, f64)) / bound
    print(name, "one index replaced:", moved, "bounds")
    assert moved.min() >= 16.0
