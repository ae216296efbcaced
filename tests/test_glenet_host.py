"""CPU-side tests of the GLENet / RGF feature: the numpy restatement of the reference's polygon
intersection against the reference's records (tests/golden/glenet.npz, written by tests/golden/make_glenet_fixtures.py),
the reference's own error against an exact clip, the fold and bin helpers against sklearn / pandas, the module tree's
state dict, a float64 evaluation of the module against the reference's float32 outputs, the refusals and the C entry
points' argument checks."""
import json
import os

import numpy as np
import pytest
import torch

import _glenet_oracle as O


@pytest.fixture(scope="module")
def fx(golden):
    return golden("glenet")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("tag", ["gen", "nam"])
def test_oracle_reproduces_the_reference_records(fx, tag):
    """Vertices, counts and areas of the restatement are bit-equal to the reference's on every generic pair and every named
    case, the quirks included (two identical boxes: area 0)."""
    pts, cnt, area, _ = O.rinter(fx[tag + "_cg"], fx[tag + "_cq"])
    assert np.array_equal(cnt, fx[tag + "_cnt"])
    assert np.array_equal(_bits(pts), _bits(fx[tag + "_pts"]))
    assert np.array_equal(_bits(area), _bits(fx[tag + "_area"]))
    iou = O.iou3d(fx[tag + "_g"], fx[tag + "_q"], area=area)
    assert np.array_equal(_bits(iou), _bits(fx[tag + "_iou"]))
    if tag == "nam":
        names = json.loads(str(fx["named"]))
        assert fx["nam_iou"][names.index("identical")] == 0.0                     # the reference's quirk
        assert abs(fx["nam_iou"][names.index("turned_by_pi")]) < 1e-6            # about 4e-8 where the exact value is 1
        assert fx["nam_iou"][names.index("negative_size")] < 0                    # not special-cased


def test_reference_error_against_the_exact_clip(fx):
    """e_ref, the reference's own float32 error on the generic pairs, from the fixture: small against the IoU scale, and the
    float64 clip agrees with the reference wherever nothing is degenerate."""
    exact = O.iou3d_f64(fx["gen_g"], fx["gen_q"])
    e_ref = float(np.abs(fx["gen_iou"].astype(np.float64) - exact).max())
    print(f"e_ref = {e_ref:.3e} over {len(exact)} pairs, IoU in [{exact.min():.3f}, {exact.max():.3f}]")
    assert 0 < e_ref < 1e-3
    assert exact.min() >= 0 and exact.max() <= 1 and exact.mean() > 0.3             # the pairs do overlap
    sep = O.angles_separated(O.rinter(fx["gen_cg"], fx["gen_cq"])[3], fx["gen_cnt"])
    assert (~sep).mean() <= 0.02


# ---------------------------------------------------------------------------------------------- folds and bins
def test_kfold_indices_equal_sklearn():
    model_selection = pytest.importorskip("sklearn.model_selection")
    from lidargen.metrics.datasets.object_uncertainty_dataset import kfold_indices

    for n in (10, 23, 1000):
        want = list(model_selection.KFold(n_splits=10, shuffle=True, random_state=42).split(np.arange(n)))
        got = kfold_indices(n)
        assert len(got) == 10
        for (tr, va), (wtr, wva) in zip(got, want):
            assert np.array_equal(tr, wtr) and np.array_equal(va, wva)


def _seeded_table(n=57):
    r = np.random.default_rng(3)
    pts = r.integers(0, 150, n)                    # nothing above 300: the last bin stays empty
    pts[:4] = (0, 150, 300, 151)                   # values exactly on the edges
    return {f"{i}_{i}": {"variance": r.random(7), "overlap": float(r.random()), "pointnum": int(pts[i])} for i in range(n)}


def _pandas_route(result_json, bins):
    pd = pytest.importorskip("pandas")
    labels = ["<150", "150-300", ">300"]
    df = pd.DataFrame.from_dict(result_json, orient="index")
    out = {"overall": {"variance": df["variance"].mean().tolist(), "overlap": df["overlap"].mean()}, "partitions": {}}
    df["bin"] = pd.cut(df["pointnum"], bins=bins, labels=labels, include_lowest=True)
    for lbl in labels:
        sub = df[df["bin"] == lbl]
        if not sub.empty:
            out["partitions"][lbl] = {"variance": sub["variance"].mean().tolist(), "overlap": sub["overlap"].mean()}
    return out


def test_rgf_table_equals_the_pandas_route(capsys):
    from lidargen.metrics.fg_object import compute_rgf_from_results

    table = _seeded_table()
    table["x"] = {"variance": np.full(7, 0.5), "overlap": 0.25, "pointnum": 299}
    got = compute_rgf_from_results(table)
    want = _pandas_route(table, [0, 150, 300, np.inf])
    assert list(got["partitions"]) == list(want["partitions"]) == ["<150", "150-300"]       # the empty bin is skipped
    for a, b in [(got["overall"], want["overall"])] + [(got["partitions"][k], want["partitions"][k]) for k in want["partitions"]]:
        assert a["variance"] == b["variance"] and a["overlap"] == b["overlap"]
    assert "整体 variance" in capsys.readouterr().out
    # 150 falls into the first bin, 300 into the second, 0 into the first (include_lowest)
    one = {k: {"variance": np.zeros(7), "overlap": float(i), "pointnum": p} for i, (k, p) in enumerate((("a", 0), ("b", 150), ("c", 300)))}
    got = compute_rgf_from_results(one)
    assert got["partitions"]["<150"]["overlap"] == 0.5 and got["partitions"]["150-300"]["overlap"] == 2.0


# ---------------------------------------------------------------------------------------------- state dict
def test_state_dict_keys_and_shapes(fx):
    from lidargen.metrics.models.glenet import DEFAULT_MODEL_CFG, Generator

    net = Generator(DEFAULT_MODEL_CFG, 3, 1)
    sd = net.state_dict()
    assert list(sd) == json.loads(str(fx["names"])) and len(sd) == 110
    assert [list(v.shape) for v in sd.values()] == json.loads(str(fx["shapes"]))
    seeded = O.seeded_state(7)
    missing = Generator(DEFAULT_MODEL_CFG, 3, 1).load_state_dict(seeded, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert "global_step" in sd and any(k.startswith("xy_encoder.") for k in sd)
    # the seeded fill leaves no BatchNorm statistic trivial and makes some bn3 gains negative; global_step stays 0
    for k, v in seeded.items():
        if k.endswith("running_mean"):
            assert float(v.abs().max()) > 0.05, k
        elif k.endswith("running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5 and float(v.std()) > 0.05, k
        elif k.endswith("bn3.weight"):
            assert bool((v < 0).any()) and bool((v > 0).any()), k
    assert int(seeded["global_step"]) == 0


# ---------------------------------------------------------------------------------------------- module against float64
def _row_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)


def test_float64_module_reproduces_the_reference(fx):
    """The float64 evaluation of the project's seeded state dict gives the reference's recorded float32 outputs to the
    reference's own float32 error m_ref, measured here per row; m_ref has the size of float32 rounding through ~10 layers."""
    x, text, eps, _, _ = O.gathered(fx)
    mu, logvar, box = O.generator_f64(O.seeded_state(7), x, text, eps)
    m_mu, m_lv, m_box = _row_err(fx["ref_mu"], mu), _row_err(fx["ref_logvar"], logvar), _row_err(fx["ref_box"], box)
    print(f"m_ref: mu {m_mu.max():.2e} logvar {m_lv.max():.2e} box {m_box.max():.2e}")
    assert max(m_mu.max(), m_lv.max(), m_box.max()) < 1e-4            # a wrong key, fold or layer order is O(1)
    assert min(m_mu.max(), m_box.max()) > 0                           # the records are float32, not a copy of this evaluation
    post = O.heading(box.float())
    assert np.allclose(post[:, :6].numpy(), fx["ref_box_post"][:, :6], rtol=0, atol=1e-4)


def test_heading_and_decode_match_the_restated_formulas():
    from lidargen.metrics.models.glenet.model import heading_postprocess

    g = torch.Generator().manual_seed(0)
    box = torch.randn((64, 9), generator=g) * 2
    box[0, 7] = box[0, 8] = 0.25                                     # dir[0] == dir[1]: label 0
    box[1, 6] = 0.78539 + np.pi                                     # v exactly a multiple of pi (in float32: as computed)
    box[2, 6] = 0.78539
    box[3, 6] = 0.78539 - 2 * np.pi
    want = O.heading(box)
    got = heading_postprocess(box.clone(), 0.78539, 0.0, 2)
    assert torch.equal(got, want)
    assert got[0, 6] == want[0, 6] and float(got[0, 6]) < 0.78539 + np.pi          # label 0: no half turn added
    v = box[:, 6] - 0.78539
    lab = (box[:, 8] > box[:, 7]).float()
    assert torch.equal(got[:, 6], (v - torch.floor(v / np.pi) * np.pi) + 0.78539 + np.pi * lab)
    assert torch.all((got[:, 6] - 0.78539 - np.pi * lab >= -1e-6) & (got[:, 6] - 0.78539 - np.pi * lab < np.pi + 1e-6))
    # decode: centres by the float64 diagonal, rounded once; sizes exp times the anchor in float32
    b = box.numpy()[:, :7].astype(np.float32)
    d = O.decode(b)
    diag = np.sqrt(3.9 ** 2 + 1.6 ** 2)
    assert np.array_equal(d[:, 0], (b[:, 0].astype(np.float64) * diag).astype(np.float32))
    assert np.array_equal(d[:, 2], b[:, 2] * np.float32(1.56))
    assert np.allclose(d[:, 3], np.exp(b[:, 3].astype(np.float64)) * 3.9, rtol=1e-6)
    assert np.array_equal(d[:, 6], b[:, 6])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path):
    from lidargen.metrics import fg_object
    from lidargen.metrics.models.glenet import DEFAULT_MODEL_CFG, Generator
    from lidargen.metrics.models.glenet import eval_utils, model
    from lidarcrafter_amd import ops_glenet as KG

    net = Generator(DEFAULT_MODEL_CFG, 3, 1).eval()
    batch = {"points": torch.zeros(2, 3, 16), "text_feat": torch.zeros(2, 512), "eps": torch.zeros(2, 8)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.sample_boxes(torch.zeros(4, 3), torch.tensor([0, 4], dtype=torch.int32), torch.zeros(1, 512),
                         torch.zeros((1, 1, 8), dtype=torch.int32), torch.zeros(1, 1, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KG.riou3d_paired(torch.zeros(1, 7), torch.zeros(1, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_utils.iou3d(torch.zeros(1, 7), torch.zeros(1, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KG.segment_center(torch.zeros(4, 3), torch.tensor([0, 4], dtype=torch.int32))
    from lidarcrafter_amd import ops
    for name in ("segment_center", "glenet_trunk", "rbox_intersection", "riou3d_paired", "glenet_score"):
        assert getattr(ops, name) is getattr(KG, name)                # ops.<name> resolves to the same entry
    with pytest.raises(AttributeError):
        ops.no_such_op
    net.train()
    with pytest.raises(NotImplementedError, match="training mode"):
        net(batch)
    with pytest.raises(NotImplementedError, match="training mode"):
        net.sample_boxes(None, None, None, None, None)
    for fn in (net.reg_loss, net.get_training_loss, net.kl_divergence, model.l2_regularisation, net.reg_loss_func,
               net.dir_loss_func):
        with pytest.raises(NotImplementedError, match="not built"):
            fn(torch.zeros(1), torch.zeros(1))
    with pytest.raises(NotImplementedError, match="not built"):
        net.x_encoder({"x": batch["points"], "text_feat": batch["text_feat"]})
    missing = tmp_path / "nusc_object_uncertainty_model.pth"
    with pytest.raises(FileNotFoundError, match=str(missing)):
        fg_object.pretrained_glenet(missing)
    torch.save({"model_state": O.seeded_state(7)}, missing)
    loaded = fg_object.pretrained_glenet(missing, device="cpu")
    assert not loaded.training and torch.equal(loaded.state_dict()["x_encoder.fc1.weight"], O.seeded_state(7)["x_encoder.fc1.weight"])


def test_dataset_is_ragged_and_normalises_the_box():
    from lidargen.metrics.datasets.object_uncertainty_dataset import NuscObjUncertainty, kfold_indices

    r = np.random.default_rng(0)
    infos = [{"points": r.normal(0, 1, (n, 4)).astype(np.float32) + 5, "name": ("car", "truck", "bus", "pedestrian")[i % 4],
              "box3d_lidar": [5.0, 5.1, 4.9, 4.0, 1.7, 1.5, 0.3 * i, 0.0, 0.0], "num_points_in_gt": n}
             for i, n in enumerate(r.integers(1, 40, 27))]
    text = {k: r.normal(0, 1, (1, 512)).astype(np.float32) for k in ("car", "truck", "bus")}
    kept = [x for x in infos if x["name"] != "pedestrian"]
    ds = NuscObjUncertainty(infos, text, fold_idx=2, generator=np.random.default_rng(5))
    val = kfold_indices(len(kept))[2][1]
    assert len(ds) == len(val)
    item = ds[0]
    src = kept[val[0]]
    assert item["key"] == f"{val[0]}_{val[0]}" and item["points"].shape == (src["num_points_in_gt"], 3)
    mean = src["points"][:, :3].astype(np.float64).mean(axis=0).astype(np.float32)
    diag = np.sqrt(3.9 ** 2 + 1.6 ** 2)
    want = np.array([-mean[0] / diag, -mean[1] / diag, -mean[2] / 1.56, np.log(4.0 / 3.9), np.log(1.7 / 1.6), np.log(1.5 / 1.56),
                     src["box3d_lidar"][6]], np.float32)
    assert np.array_equal(item["gt_boxes"], want)
    batch = next(ds.batches(8))
    counts = np.diff(batch["offsets"])
    assert batch["points"].shape[0] == counts.sum() and batch["gt_boxes"].shape == (len(counts), 7)
    ch = ds.choice(counts, 4)
    assert ch.shape == (4, len(counts), 512) and ch.dtype == np.int32
    assert (ch >= 0).all() and (ch < counts[None, :, None]).all()
    again = NuscObjUncertainty(infos, text, fold_idx=2, generator=np.random.default_rng(5)).choice(counts, 4)
    assert np.array_equal(ch, again)
    infos[int(val[0])]  # (the source list is not modified)
    empty = [dict(kept[0], points=np.zeros((0, 4), np.float32))]
    with pytest.raises(ValueError, match="no points"):
        NuscObjUncertainty(empty, text)[0]


# ---------------------------------------------------------------------------------------------- ABI
def test_entry_points_refuse_before_any_launch():
    """Null pointers and sizes < 1 return LC_EINVAL before anything is dereferenced or launched (callable without a GPU)."""
    import ctypes

    from lidarcrafter_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = -1
    assert h.lc_segment_center_fwd(None, p, 1, 4, 1.0, 1.0, 1.0, p, p, None) == EINVAL
    assert h.lc_segment_center_fwd(p, None, 1, 4, 1.0, 1.0, 1.0, p, p, None) == EINVAL
    assert h.lc_segment_center_fwd(p, p, 0, 4, 1.0, 1.0, 1.0, p, p, None) == EINVAL
    assert h.lc_segment_center_fwd(p, p, 1, 0, 1.0, 1.0, 1.0, p, p, None) == EINVAL
    assert h.lc_segment_center_fwd(p, p, 1, 4, 0.0, 1.0, 1.0, p, p, None) == EINVAL
    w = [p] * 12

    def trunk(norm=p, total=4, off=p, ch=p, B=1, K=4, R=1, weights=w, fa=p, fs=p):
        return h.lc_glenet_trunk_fwd(norm, total, off, ch, B, K, R, *weights, fa, fs, None)

    assert trunk(norm=None) == EINVAL and trunk(off=None) == EINVAL and trunk(ch=None) == EINVAL
    assert trunk(fa=None) == EINVAL and trunk(fs=None) == EINVAL
    for i in range(12):
        assert trunk(weights=w[:i] + [None] + w[i + 1:]) == EINVAL
    assert trunk(B=0) == EINVAL and trunk(K=0) == EINVAL and trunk(R=0) == EINVAL and trunk(total=0) == EINVAL
    assert h.lc_rbox_inter_fwd(None, p, 1, p, p, p, None) == EINVAL
    assert h.lc_rbox_inter_fwd(p, p, 0, p, p, p, None) == EINVAL
    assert h.lc_rbox_inter_fwd(p, p, 1, p, None, p, None) == EINVAL
    assert h.lc_riou3d_paired_fwd(None, 7, p, 7, 1, p, None) == EINVAL
    assert h.lc_riou3d_paired_fwd(p, 7, p, 7, 0, p, None) == EINVAL
    assert h.lc_riou3d_paired_fwd(p, 6, p, 7, 1, p, None) == EINVAL
    assert h.lc_glenet_score_fwd(None, p, 1, 1, 4.2, 3.9, 1.6, 1.56, p, p, p, p, None) == EINVAL
    assert h.lc_glenet_score_fwd(p, p, 0, 1, 4.2, 3.9, 1.6, 1.56, p, p, p, p, None) == EINVAL
    assert h.lc_glenet_score_fwd(p, p, 1, 0, 4.2, 3.9, 1.6, 1.56, p, p, p, p, None) == EINVAL
    assert h.lc_glenet_score_fwd(p, p, 1, 1, 4.2, 3.9, 1.6, 1.56, p, p, None, p, None) == EINVAL
    assert h.lc_glenet_score_fwd(p, p, 1, 1, 0.0, 3.9, 1.6, 1.56, p, p, p, p, None) == EINVAL
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB), "csrc", "glenet.hip"))
