"""CPU tests of the Frechet Point-Voxel Distance: the float64 oracle of tests/_spvcnn_oracle.py pinned on
torch.nn.functional.grid_sample (the neighbour order and the trilinear weights of voxel_to_point), its renormalisation and
scatter-mean on direct restatements, the float coordinate of initial_voxelize, and the host side of the SPVCNN extractor
(state-dict keys, the Linear + BatchNorm1d fold, the loader, the refusals)."""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spconv_oracle as O  # noqa: E402
import _spvcnn_oracle as PV  # noqa: E402

from lidarcrafter_amd import ops_spvoxel as KV  # noqa: E402


def _model():
    from lidargen.metrics.models.spvcnn.model import Model

    return Model(O.CONFIG)


# ---- the oracle -------------------------------------------------------------------------------------------------------
def _block(s, n=5):
    """A fully populated n x n x n block at stride s, rows shuffled, batch 0."""
    rows = [(x * s, y * s, z * s, 0) for x in range(n) for y in range(n) for z in range(n)]
    c = torch.tensor(rows, dtype=torch.int64)
    return c[torch.randperm(len(c), generator=torch.Generator().manual_seed(s))]


@pytest.mark.parametrize("s", [1, 4])
def test_voxel_to_point_is_grid_sample(s):
    """On a full block every interior point has its eight neighbours and their weights sum to 1, so voxel_to_point is
    trilinear interpolation: torch.nn.functional.grid_sample (5-D, bilinear, align_corners=True, float64) of the dense
    volume.  The oracle divides the weights by (their sum + 1e-8): the one known factor (1 + 1e-8) is multiplied back, and
    the two then agree to 1e-10."""
    n, C = 5, 6
    vox = _block(s, n)
    g = torch.Generator().manual_seed(10 + s)
    F = torch.randn((len(vox), C), generator=g, dtype=torch.float64)
    p = torch.rand((200, 3), generator=g, dtype=torch.float64) * (n - 1) * s
    on = torch.randint(0, n - 1, (40, 3), generator=g).double() * s               # exactly on voxels
    mixed = p[:40].clone()
    mixed[:, 1] = torch.floor(mixed[:, 1] / s) * s                                # on a voxel plane along y only
    p = torch.cat([p, on, mixed]).float()                                         # the coordinate is a float32
    pts = torch.cat([p, torch.zeros(len(p), 1)], 1)
    idx, w = PV.point_maps(pts, vox, s, torch.float64)
    assert bool((idx >= 0).all())
    got = PV.devoxelize(F, idx, w) * (1.0 + 1e-8)
    vol = torch.zeros((C, n, n, n), dtype=torch.float64)
    vol[:, vox[:, 0] // s, vox[:, 1] // s, vox[:, 2] // s] = F.t()
    grid = (p.double() / ((n - 1) * s) * 2 - 1)[:, [2, 1, 0]].reshape(1, 1, 1, -1, 3)   # grid_sample's x is the last axis
    want = torch.nn.functional.grid_sample(vol[None], grid, mode="bilinear", align_corners=True)[0, :, 0, 0].t()
    assert float((got - want).abs().max()) < 1e-10
    # the first neighbour is the point's own cell, the last the opposite corner
    cell = (torch.floor(p / s) * s).long()
    assert torch.equal(vox[idx[:, 0], :3], cell) and torch.equal(vox[idx[:, 7], :3], cell + s)
    assert torch.equal(vox[idx[:, 1], :3], cell + torch.tensor([0, 0, s]))        # z fastest


def test_renormalisation_with_absent_neighbours_and_none():
    """Weights of absent neighbours are zeroed before the division by (sum + 1e-8); a point without any neighbour gets
    zeros, not NaN; another batch's voxel at the same place is not a neighbour."""
    s = 2
    vox = torch.tensor([[0, 0, 0, 0], [2, 0, 0, 0], [0, 2, 2, 0], [2, 2, 2, 0], [40, 40, 40, 1], [0, 0, 2, 1]])
    pts = torch.tensor([[0.5, 1.25, 0.75, 0.0], [1.0, 1.0, 1.0, 0.0], [41.0, 40.5, 40.0, 0.0], [41.0, 40.5, 40.0, 1.0],
                        [100.0, 3.0, 3.0, 0.0]])
    idx, w = PV.point_maps(pts, vox, s, torch.float64)
    assert idx.tolist() == [[0, -1, -1, 2, 1, -1, -1, 3], [0, -1, -1, 2, 1, -1, -1, 3], [-1] * 8, [4] + [-1] * 7, [-1] * 8]
    for i, (x, y, z, b) in enumerate(pts.double().tolist()):
        raw = []
        for k in range(8):
            ax = (x - np.floor(x / s) * s) if k & 4 else (np.floor(x / s) * s + s - x)
            ay = (y - np.floor(y / s) * s) if k & 2 else (np.floor(y / s) * s + s - y)
            az = (z - np.floor(z / s) * s) if k & 1 else (np.floor(z / s) * s + s - z)
            raw.append(ax * ay * az / s ** 3 if idx[i, k] >= 0 else 0.0)
        want = [r / (sum(raw) + 1e-8) for r in raw]
        assert np.abs(np.array(want) - w[i].numpy()).max() < 1e-15
    assert bool((w[2] == 0).all()) and bool((w[4] == 0).all()) and bool(torch.isfinite(w).all())
    assert abs(float(w[0].sum()) - 1.0) < 1e-7 and float(w[3, 0]) > 0.99           # renormalised over what is present
    F = torch.randn((len(vox), 3), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out = PV.devoxelize(F, idx, w)
    assert bool((out[2] == 0).all()) and torch.allclose(out[3], F[4] * w[3, 0])


def test_point_to_voxel_is_index_add_of_the_quotients():
    g = torch.Generator().manual_seed(3)
    idx0 = torch.randint(0, 9, (200,), generator=g)
    idx0[idx0 == 4] = 5                                              # voxel 4 has no point
    F = torch.randn((200, 5), generator=g, dtype=torch.float64)
    count = torch.bincount(idx0, minlength=9).double()
    want = torch.zeros((9, 5), dtype=torch.float64).index_add_(0, idx0, F / count[idx0][:, None])
    got = PV.voxelize(F, idx0, 9)
    assert float((got - want).abs().max()) < 1e-14 and bool((got[4] == 0).all())
    assert torch.allclose(got[7], F[idx0 == 7].mean(0))


def test_float_coordinate_floors_to_the_integer():
    """(c * 0.05) / 0.05 in float32 is not the identity, by either route (the device multiplies by the reciprocal, the
    host divides), but it is never below c: its floor is c; both routes leave the same c one ulp above."""
    c = np.arange(4096)
    mul, div = PV.float_coord(c), PV.float_coord_div(c)
    assert mul.dtype == np.float32 and div.dtype == np.float32
    for v in (mul, div):
        assert np.array_equal(np.floor(v).astype(np.int64), c)
    off = np.nonzero(mul != c)[0]
    assert len(off) > 0 and np.array_equal(off, np.nonzero(div != c)[0])
    assert np.array_equal(mul[off], np.nextafter(c[off].astype(np.float32), np.float32(np.inf)))
    t = torch.arange(4096, dtype=torch.float32)
    assert np.array_equal(((t * 0.05) / 0.05).numpy(), div)          # torch on the host: the plain route
    from lidargen.metrics.models.spvcnn.model import float_coords

    ci = torch.stack([torch.arange(4096)] * 3 + [torch.arange(4096) % 7], 1)
    assert torch.equal(float_coords(ci, 0.05, 0.05), PV.point_coords(ci))          # the model's expression, on the host
    vox, row = PV.initial_voxels(PV.point_coords(torch.tensor([[7, 3, 11, 1], [7, 3, 11, 0], [7, 3, 11, 1], [0, 0, 0, 0]])))
    assert vox.tolist() == [[0, 0, 0, 0], [7, 3, 11, 0], [7, 3, 11, 1]] and row.tolist() == [2, 1, 2, 0]


# ---- plumbing ---------------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_references():
    from lidargen.metrics.models.minkowskinet.model import Model as MinkUNet

    m = _model()
    sd = m.state_dict()
    base = list(MinkUNet(O.CONFIG).state_dict())
    assert base[-2:] == ["classifier.0.weight", "classifier.0.bias"]
    want = []
    for i in range(3):
        want += [f"point_transforms.{i}.0.weight", f"point_transforms.{i}.0.bias", f"point_transforms.{i}.1.weight",
                 f"point_transforms.{i}.1.bias", f"point_transforms.{i}.1.running_mean", f"point_transforms.{i}.1.running_var",
                 f"point_transforms.{i}.1.num_batches_tracked"]
    assert list(sd) == base + want
    assert [tuple(sd[f"point_transforms.{i}.0.weight"].shape) for i in range(3)] == [(128, 16), (64, 128), (48, 64)]
    assert len(m._pairs()) == 52 and all(bn is not None for _, bn in m._pairs())
    state = PV.seeded_state(m, 4)
    assert float(state["point_transforms.1.0.bias"].abs().min()) > 0
    m2 = _model()
    m2.load_state_dict(state)
    assert all(torch.equal(v, state[k]) for k, v in m2.state_dict().items())


def test_linear_batchnorm_fold_matches_the_modules():
    m = _model()
    sd = PV.seeded_state(m, 1)
    m.load_state_dict(sd)
    m.eval()
    names = {id(mod): n for n, mod in m.named_modules()}
    first = m.folded()
    g = torch.Generator().manual_seed(2)
    for (layer, bn), (w, b) in zip(m._pairs()[49:], first[49:]):
        wo, bo = PV.fold_linear(sd, names[id(layer)], names[id(bn)], torch.float32)
        assert torch.equal(w, wo) and torch.equal(b, bo) and tuple(w.shape) == (1, layer.in_features, layer.out_features)
        x = torch.randn((7, layer.in_features), generator=g, dtype=torch.float64)
        seq = copy.deepcopy(torch.nn.Sequential(layer, bn)).double().eval()
        w64, b64 = PV.fold_linear(sd, names[id(layer)], names[id(bn)], torch.float64)
        with torch.no_grad():
            assert float((seq(x) - (x @ w64[0] + b64)).abs().max()) < 1e-12
    for (conv, bn), (w, b) in zip(m._pairs()[:49], first[:49]):       # the convolutions fold as in the MinkUNet
        wo, bo = O.fold(sd, names[id(conv)], names[id(bn)], torch.float32)
        assert torch.equal(w, wo) and torch.equal(b, bo)
    assert m.folded() is first
    with torch.no_grad():
        m.point_transforms[2][1].running_var.mul_(2.0)
    again = m.folded()
    assert again is not first and not torch.equal(again[51][0], first[51][0]) and torch.equal(again[50][0], first[50][0])


def test_pretrained_reads_the_folder_and_fetches_nothing(tmp_path):
    import yaml

    from lidargen.metrics import models

    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path))):
        models.spvcnn.pretrained("nuscenes", device="cpu", root=tmp_path)
    folder = tmp_path / "nuscenes" / "spvcnn"
    folder.mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="config.yaml"):
        models.spvcnn.pretrained("nuscenes", device="cpu", root=tmp_path)
    (folder / "config.yaml").write_text(yaml.safe_dump(O.CONFIG))
    with pytest.raises(FileNotFoundError, match="model.ckpt"):
        models.spvcnn.pretrained("nuscenes", device="cpu", root=tmp_path)
    sd = PV.seeded_state(_model(), 3)
    torch.save({"state_dict": dict(sd, **{"criterion.weight": torch.zeros(3)})}, folder / "model.ckpt")
    m = models.spvcnn.pretrained("nuscenes", device="cpu", root=tmp_path)
    assert type(m).__module__.endswith("spvcnn.model") and not m.training
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    short = {k: v for k, v in sd.items() if k != "point_transforms.1.1.running_mean"}
    torch.save({"state_dict": short}, folder / "model.ckpt")
    with pytest.raises(KeyError, match="point_transforms.1.1.running_mean"):
        models.spvcnn.pretrained("nuscenes", device="cpu", root=tmp_path)


def test_model_refuses_train_mode_and_cpu_tensors():
    from lidargen.metrics.models.spvcnn.model import Model

    m = _model()
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="not a width"):
        Model({"model_params": dict(O.CONFIG["model_params"], cr=0.75)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KV.query(torch.zeros(4, 4), 1, torch.zeros(8, dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KV.devoxelize(torch.zeros(4, 16), torch.zeros(4, 8, dtype=torch.int32), torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KV.voxelize(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))


def _defines():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "lidarcrafter_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(LC_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}


def test_exchange_entries_refuse_before_any_launch():
    """The C entries check their arguments on the host: nothing is dereferenced or launched (callable without a GPU)."""
    from lidarcrafter_amd import _lib

    d = _defines()
    EINVAL, EUNSUP = d["LC_EINVAL"], d["LC_EUNSUP"]
    h = _lib.lib()
    p = 4096
    assert h.lc_spvox_query(p, 10, 3, p, 10, p, p, None) == EUNSUP                         # not a power of two
    assert h.lc_spvox_query(p, 10, 2 * d["LC_SPCONV_MAX_STRIDE"], p, 10, p, p, None) == EUNSUP
    assert h.lc_spvox_query(p, d["LC_SPCONV_MAX_ROWS"] + 1, 1, p, 10, p, p, None) == EUNSUP
    assert h.lc_spvox_query(p + 4, 10, 1, p, 10, p, p, None) == EUNSUP                     # quads
    assert h.lc_spvox_query(p, 0, 1, p, 10, p, p, None) == EINVAL and h.lc_spvox_query(p, 10, 1, None, 10, p, p, None) == EINVAL

    def devox(C=16, ldf=None, lda=0, ldo=None, addend=None, f=p, N=10):
        return h.lc_spvox_devoxelize(f, C if ldf is None else ldf, 10, p, p, addend, lda, p, C if ldo is None else ldo, N,
                                     C, None)

    for C in (4, 8, 32, 96, 256):
        assert devox(C=C) == EUNSUP, C
    assert devox(ldf=18) == EUNSUP and devox(ldo=18) == EUNSUP and devox(addend=p, lda=18) == EUNSUP and devox(f=p + 4) == EUNSUP
    assert devox(ldf=8) == EINVAL and devox(addend=p, lda=8) == EINVAL and devox(N=0) == EINVAL
    vox = lambda C=16, ldf=16, ldo=16, V=10: h.lc_spvox_voxelize(p, ldf, 10, p, 10, p, V, p, ldo, C, None)
    for C in (8, 32, 48, 96, 256):
        assert vox(C=C) == EUNSUP, C
    assert vox(ldf=8) == EINVAL and vox(ldo=8) == EINVAL and vox(V=0) == EINVAL
    assert vox(V=d["LC_SPCONV_MAX_ROWS"] + 1) == EUNSUP
    for c in (16, 128, 64, 48):
        assert c in KV.WIDTHS_DEVOX
    for c in (4, 16, 128, 64):
        assert c in KV.WIDTHS_VOX


# ---- refusals that stay, and where they point ---------------------------------------------------------------------------
def test_refusals_name_the_new_entry_points(tmp_path):
    from lidargen import metrics
    from lidargen.metrics import eval_utils, metric_utils

    with pytest.raises(NotImplementedError, match="'point_voxel'.*metric_utils.compute_point_voxel_logits"):
        metric_utils.compute_logits("32", "point_voxel", [])
    with pytest.raises(NotImplementedError, match="spvcnn.*models.spvcnn.pretrained"):
        metrics.build_model("nuscenes", "spvcnn", root=tmp_path)
    with pytest.raises(NotImplementedError, match="'fpvd'.*eval_utils.compute_fpvd"):
        eval_utils.evaluate([], [], ["fpvd"], "32")
    assert callable(metric_utils.compute_point_voxel_logits) and callable(eval_utils.compute_fpvd)
    assert callable(metrics.models.spvcnn.pretrained)
