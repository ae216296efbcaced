"""CPU tests of the Frechet Sparse Volume Distance: the float64 oracle (tests/_spconv_oracle.py) pinned on
torch.nn.functional.conv3d / conv_transpose3d, the host-side pieces of the product (pcd2voxel, the model's state-dict
names, the BatchNorm fold, build_model, the Frechet formula), the argument checks of the C entry points, and the host
side of the GPU tests of the coordinate hash and the convolution widths (tests/_spconv_hash.py: the restated capacity, the
scenes exist and are what they claim, the vectorised neighbour oracle is the dictionary's; CONV_CASES covers both models)."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spconv_hash as H  # noqa: E402
import _spconv_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(s, seed, B=2, dims=(6, 4, 8), Ci=3, fill=0.4):
    """Random active sites of a dense grid, coordinates multiples of s; -> (feats float64, coords int64, dense, dims)."""
    g = torch.Generator().manual_seed(seed)
    occ = torch.rand((B,) + dims, generator=g) < fill
    b, x, y, z = occ.nonzero(as_tuple=True)
    perm = torch.randperm(len(b), generator=g)                       # the rows are in no particular order
    b, x, y, z = b[perm], x[perm], y[perm], z[perm]
    coords = torch.stack([x * s, y * s, z * s, b], 1)
    feats = torch.randn((len(b), Ci), generator=g, dtype=torch.float64)
    dense = torch.zeros((B, Ci) + dims, dtype=torch.float64)
    dense[b, :, x, y, z] = feats
    return feats, coords, dense


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), float((a - b).abs().max())


@pytest.mark.parametrize("s", [1, 2])
def test_oracle_stride1_conv_is_conv3d(s):
    feats, coords, dense = _scene(s, 1)
    Ci, Co = 3, 5
    w = torch.randn((27, Ci, Co), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    got = O.conv(feats, O.nbr_same(coords, s), w)
    wd = w.reshape(3, 3, 3, Ci, Co).permute(4, 3, 2, 1, 0)          # k = ix + 3 iy + 9 iz -> [Co, Ci, kx, ky, kz]
    ref = F.conv3d(dense, wd, padding=1)
    _close(got, ref[coords[:, 3], :, coords[:, 0] // s, coords[:, 1] // s, coords[:, 2] // s])
    assert int((O.nbr_same(coords, s) >= 0).sum()) > 3 * len(coords)   # the scene has neighbours at all


@pytest.mark.parametrize("s", [1, 2])
def test_oracle_down_conv_is_strided_conv3d(s):
    feats, coords, dense = _scene(s, 3)
    Ci, Co = 3, 4
    w = torch.randn((8, Ci, Co), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    coarse = O.down_coords(coords, s)
    got = O.conv(feats, O.nbr_down(coords, coarse, s), w)
    wd = w.reshape(2, 2, 2, Ci, Co).permute(4, 3, 0, 1, 2)          # k = 4 ix + 2 iy + iz
    ref = F.conv3d(dense, wd, stride=2)
    q = coarse[:, :3] // (2 * s)
    _close(got, ref[coarse[:, 3], :, q[:, 0], q[:, 1], q[:, 2]])
    # every coarse site that has a child is there, once, and no other
    occ = F.max_pool3d((dense.abs().sum(1, keepdim=True) > 0).double(), 2)[:, 0]
    assert len(coarse) == int(occ.sum()) and bool((occ[coarse[:, 3], q[:, 0], q[:, 1], q[:, 2]] == 1).all())
    key = coarse[:, 3] * 10 ** 9 + coarse[:, 0] * 10 ** 6 + coarse[:, 1] * 10 ** 3 + coarse[:, 2]
    assert bool((key[1:] > key[:-1]).all())                          # ascending (batch, x, y, z)


@pytest.mark.parametrize("s", [1, 2])
def test_oracle_transposed_conv_is_conv_transpose3d(s):
    _, coords, dense = _scene(s, 5)
    Ci, Co = 4, 3
    g = torch.Generator().manual_seed(6)
    coarse = O.down_coords(coords, s)
    fc = torch.randn((len(coarse), Ci), generator=g, dtype=torch.float64)
    w = torch.randn((8, Ci, Co), generator=g, dtype=torch.float64)
    nbr = O.nbr_up(coords, coarse, s)
    assert bool(((nbr >= 0).sum(1) == 1).all())                      # one (j, k) per fine voxel
    got = O.conv(fc, nbr, w)
    B, _, X, Y, Z = dense.shape
    dc = torch.zeros((B, Ci, X // 2, Y // 2, Z // 2), dtype=torch.float64)
    q = coarse[:, :3] // (2 * s)
    dc[coarse[:, 3], :, q[:, 0], q[:, 1], q[:, 2]] = fc
    ref = F.conv_transpose3d(dc, w.reshape(2, 2, 2, Ci, Co).permute(3, 4, 0, 1, 2), stride=2)
    _close(got, ref[coords[:, 3], :, coords[:, 0] // s, coords[:, 1] // s, coords[:, 2] // s])


def test_downsampled_coordinate_order():
    from lidarcrafter_amd import ops_spconv as KS

    c = torch.tensor([[3, 0, 0, 1], [0, 0, 0, 1], [2, 5, 1, 0]])
    want = [[2, 4, 0, 0], [0, 0, 0, 1], [2, 0, 0, 1]]
    assert O.down_coords(c, 1).tolist() == want
    got = KS.downsample_coords(c.to(torch.int32), 1)                 # torch plumbing: runs on the CPU too
    assert got.dtype == torch.int32 and got.tolist() == want
    c2 = torch.tensor([[6, 0, 4, 1], [0, 0, 0, 1], [4, 10, 2, 0], [4, 8, 2, 0]])
    assert KS.downsample_coords(c2.to(torch.int32), 2).tolist() == O.down_coords(c2, 2).tolist() == \
        [[4, 8, 0, 0], [0, 0, 0, 1], [4, 0, 4, 1]]
    top = torch.tensor([[KS.MAX_COORD, 1, 0, KS.MAX_BATCH], [0, 0, 0, 0]], dtype=torch.int32)
    assert KS.unpack_keys(KS.pack_keys(top)).tolist() == top.tolist()


def _pcd2voxel_transcribed(pcd):
    """The reference's lines (metric_utils.py:28-66, 157-165) in numpy, as they stand there."""
    pcd_voxel = np.round(pcd / 0.05)
    pcd_voxel = pcd_voxel - pcd_voxel.min(0, keepdims=1)
    feat = np.concatenate((pcd, -np.ones((pcd.shape[0], 1))), axis=1)
    coords = np.floor(pcd_voxel / np.array((1, 1, 1))).astype(np.int32)
    x = coords - np.min(coords, axis=0)
    x = x.astype(np.uint64, copy=False)
    xmax = np.max(x, axis=0).astype(np.uint64) + 1
    h = np.zeros(x.shape[0], dtype=np.uint64)
    for k in range(x.shape[1] - 1):
        h += x[:, k]
        h *= xmax[k + 1]
    h += x[:, -1]
    _, inds, _ = np.unique(h, return_index=True, return_inverse=True)
    return torch.FloatTensor(feat[inds]), torch.LongTensor(pcd_voxel[inds])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pcd2voxel_against_the_reference_lines(dtype):
    from lidargen.metrics import metric_utils as MU

    g = np.random.default_rng(3)
    pcd = g.uniform(-2, 2, (400, 3))
    pcd[10] = pcd[3] + 0.004                                         # the same voxel: the first point keeps it
    pcd[200] = pcd[3] - 0.003
    pcd[5] = (0.125, 0.375, -0.125)                                  # 2.5, 7.5, -2.5 voxels: half-way, rounds to even
    pcd[6] = (0.075, 0.025, 0.225)                                   # 1.5, 0.5, 4.5 in exact arithmetic
    pcd = pcd.astype(dtype)
    feat, vox = _pcd2voxel_transcribed(pcd)
    out = MU.pcd2voxel(pcd)["lidar"]
    assert out.F.dtype == torch.float32 and out.C.dtype == torch.int64
    assert torch.equal(out.F, feat) and torch.equal(out.C, vox)
    assert len(vox) < 400 and bool((out.F[:, 3] == -1).all())
    fo, co = O.pcd2voxel(pcd)
    assert torch.equal(fo, feat) and torch.equal(co, vox)
    r = np.round(np.asarray([0.125], dtype) / 0.05)
    assert r[0] == 2.0                                               # the half-way case is one
    kept = MU.preprocess_pcd(pcd * 20, depth_range=[1.0, 45.0])
    d = np.linalg.norm(pcd * 20, 2, axis=1)
    assert np.array_equal(kept, (pcd * 20)[(d > 1.0) & (d < 45.0)]) and 0 < len(kept) < 400
    feats, coords, offsets = MU.sparse_collate([MU.pcd2voxel(pcd), MU.pcd2voxel(pcd[:50])])
    assert coords.dtype == torch.int32 and coords.shape == (len(vox) + offsets[2] - offsets[1], 4)
    assert offsets.tolist()[:2] == [0, len(vox)] and bool((coords[len(vox):, 3] == 1).all())
    assert torch.equal(coords[:len(vox), :3].long(), vox) and torch.equal(feats[:len(vox)], feat)


_CONV_BN = """stem.0 stem.1 | stem.3 stem.4
stage1.0.net.0 stage1.0.net.1 | stage1.1.net.0 stage1.1.net.1 | stage1.1.net.3 stage1.1.net.4
stage1.2.net.0 stage1.2.net.1 | stage1.2.net.3 stage1.2.net.4
stage2.0.net.0 stage2.0.net.1 | stage2.1.net.0 stage2.1.net.1 | stage2.1.net.3 stage2.1.net.4
stage2.1.downsample.0 stage2.1.downsample.1 | stage2.2.net.0 stage2.2.net.1 | stage2.2.net.3 stage2.2.net.4
stage3.0.net.0 stage3.0.net.1 | stage3.1.net.0 stage3.1.net.1 | stage3.1.net.3 stage3.1.net.4
stage3.1.downsample.0 stage3.1.downsample.1 | stage3.2.net.0 stage3.2.net.1 | stage3.2.net.3 stage3.2.net.4
stage4.0.net.0 stage4.0.net.1 | stage4.1.net.0 stage4.1.net.1 | stage4.1.net.3 stage4.1.net.4
stage4.1.downsample.0 stage4.1.downsample.1 | stage4.2.net.0 stage4.2.net.1 | stage4.2.net.3 stage4.2.net.4
up1.0.net.0 up1.0.net.1 | up1.1.0.net.0 up1.1.0.net.1 | up1.1.0.net.3 up1.1.0.net.4
up1.1.0.downsample.0 up1.1.0.downsample.1 | up1.1.1.net.0 up1.1.1.net.1 | up1.1.1.net.3 up1.1.1.net.4
up2.0.net.0 up2.0.net.1 | up2.1.0.net.0 up2.1.0.net.1 | up2.1.0.net.3 up2.1.0.net.4
up2.1.0.downsample.0 up2.1.0.downsample.1 | up2.1.1.net.0 up2.1.1.net.1 | up2.1.1.net.3 up2.1.1.net.4
up3.0.net.0 up3.0.net.1 | up3.1.0.net.0 up3.1.0.net.1 | up3.1.0.net.3 up3.1.0.net.4
up3.1.0.downsample.0 up3.1.0.downsample.1 | up3.1.1.net.0 up3.1.1.net.1 | up3.1.1.net.3 up3.1.1.net.4
up4.0.net.0 up4.0.net.1 | up4.1.0.net.0 up4.1.0.net.1 | up4.1.0.net.3 up4.1.0.net.4
up4.1.0.downsample.0 up4.1.0.downsample.1 | up4.1.1.net.0 up4.1.1.net.1 | up4.1.1.net.3 up4.1.1.net.4"""


def _model():
    from lidargen.metrics.models.minkowskinet.model import Model

    return Model(O.CONFIG)


def test_state_dict_keys_are_the_references():
    """layer_num [32, 32, 64, 128, 256, 256, 128, 96, 96] at cr 0.5: widths 16 16 32 64 128 128 64 48 48; a residual block
    has a `downsample` where its widths differ (stage1.1 keeps 16: none)."""
    want = []
    for pair in re.split(r"\||\n", _CONV_BN):
        conv, bn = pair.split()
        want.append(conv + ".kernel")
        want += [f"{bn}.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    want += ["classifier.0.weight", "classifier.0.bias"]
    m = _model()
    sd = m.state_dict()
    assert list(sd) == want
    assert tuple(sd["stem.0.kernel"].shape) == (27, 4, 16) and tuple(sd["stage1.0.net.0.kernel"].shape) == (8, 16, 16)
    assert tuple(sd["stage2.1.downsample.0.kernel"].shape) == (16, 32)            # ks = 1: no offset axis
    assert tuple(sd["up1.0.net.0.kernel"].shape) == (8, 128, 128)
    assert tuple(sd["up1.1.0.net.0.kernel"].shape) == (27, 192, 128)              # 128 up-sampled + 64 skipped
    assert tuple(sd["up2.1.0.net.0.kernel"].shape) == (27, 96, 64) and tuple(sd["up4.1.0.net.0.kernel"].shape) == (27, 64, 48)
    assert tuple(sd["classifier.0.weight"].shape) == (20, 48)
    assert len(m._pairs()) == 49 and all(bn is not None for _, bn in m._pairs())


def test_fold_matches_the_oracle_and_follows_the_weights():
    m = _model()
    sd = O.seeded_state(m, 1)
    m.load_state_dict(sd)
    m.eval()
    names = {id(mod): n for n, mod in m.named_modules()}
    first = m.folded()
    for (conv, bn), (w, b) in zip(m._pairs(), first):
        wo, bo = O.fold(sd, names[id(conv)], names[id(bn)], torch.float32)
        assert torch.equal(w, wo) and torch.equal(b, bo) and w.dim() == 3
    assert m.folded() is first                                       # nothing changed: nothing is folded again
    with torch.no_grad():
        m.stage3[1].downsample[1].running_var.mul_(2.0)
    again = m.folded()
    assert again is not first
    i = [names[id(c)] for c, _ in m._pairs()].index("stage3.1.downsample.0")
    assert not torch.equal(again[i][0], first[i][0]) and torch.equal(again[0][0], first[0][0])
    m.load_state_dict(O.seeded_state(m, 2))
    assert not torch.equal(m.folded()[0][0], first[0][0])


def test_model_refusals():
    from lidargen.metrics import eval_utils, metric_utils
    from lidargen.metrics.models.minkowskinet.model import Model
    from lidargen.metrics.models.ts.basic_blocks import Conv3d

    m = _model()
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="not a width"):
        Model({"model_params": dict(O.CONFIG["model_params"], cr=0.75)})
    with pytest.raises(ValueError, match="nine"):
        Model({"model_params": dict(O.CONFIG["model_params"], layer_num=[32] * 8)})
    with pytest.raises(NotImplementedError):
        Conv3d(8, 8, kernel_size=3, stride=2)
    with pytest.raises(RuntimeError, match="parameters only"):
        Conv3d(16, 16)(torch.zeros(1, 16))
    for modality in ("range", "point_voxel"):
        with pytest.raises(NotImplementedError, match=f"'{modality}'"):
            metric_utils.compute_logits("32", modality, [])
    with pytest.raises(NotImplementedError, match="compute_fsvd"):
        eval_utils.evaluate([], [], ["fsvd"], "32")


def test_build_model_reads_the_folder_and_fetches_nothing(tmp_path):
    import yaml

    from lidargen import metrics

    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path))):
        metrics.build_model("nuscenes", "minkowskinet", root=tmp_path)
    folder = tmp_path / "nuscenes" / "minkowskinet"
    folder.mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="config.yaml"):
        metrics.build_model("nuscenes", "minkowskinet", root=tmp_path)
    (folder / "config.yaml").write_text(yaml.safe_dump(O.CONFIG))
    with pytest.raises(FileNotFoundError, match="model.ckpt"):
        metrics.build_model("nuscenes", "minkowskinet", root=tmp_path)
    sd = O.seeded_state(_model(), 3)
    torch.save({"state_dict": dict(sd, **{"criterion.weight": torch.zeros(3)})}, folder / "model.ckpt")
    m = metrics.build_model("nuscenes", "minkowskinet", root=tmp_path)
    assert not m.training and all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    short = {k: v for k, v in sd.items() if k != "up3.0.net.1.running_mean"}
    torch.save({"state_dict": short}, folder / "model.ckpt")
    with pytest.raises(KeyError, match="up3.0.net.1.running_mean"):
        metrics.build_model("nuscenes", "minkowskinet", root=tmp_path)
    with pytest.raises(NotImplementedError, match="spvcnn"):
        metrics.build_model("nuscenes", "spvcnn", root=tmp_path)


def _batch2list_transcribed(batch_dict, depth_range):
    """The 'depth' branch of the reference's batch2list (metric_utils.py:329-331, 351-365, 370) as it stands there."""
    output_list = []
    batch_indices = batch_dict["batch_indices"]
    for b_idx in range(batch_indices.max() + 1):
        logits = batch_dict["logits"][batch_indices == b_idx]
        coords = batch_dict["coords"][batch_indices == b_idx].float()
        coords = coords - coords.mean(0)
        bev_depth = torch.norm(coords, dim=-1) * 0.05
        sector_range = torch.linspace(depth_range[0] + 3, depth_range[1], 16 + 1)
        sector_range[0] = 0.
        logits_list = []
        for i in range(16):
            sector_indices = torch.where((bev_depth >= sector_range[i]) & (bev_depth < sector_range[i + 1]))[0]
            sector_logits = logits[sector_indices].mean(0)
            sector_logits = torch.nan_to_num(sector_logits, 0.)
            logits_list.append(sector_logits)
        output_list.append(torch.cat(logits_list).detach().cpu().numpy())
    return output_list


def test_sector_means_against_the_reference_lines():
    from lidargen.metrics import metric_utils as MU

    dr = [1.0, 45.0]
    g = torch.Generator().manual_seed(8)
    # cloud 0: voxels out to 300 (15 m): its far sectors are empty.  cloud 1: three rows at x = 0 and one at x = 525:
    # the mean is 131.25, the three sit at 131.25 voxels = 6.5625 m, exactly the second edge (4 + 41 / 16)
    c0 = torch.cat([torch.randint(0, 300, (500, 3), generator=g), torch.zeros(500, 1, dtype=torch.int64)], 1)
    c1 = torch.tensor([[0, 7, 3, 1], [0, 7, 3, 1], [0, 7, 3, 1], [525, 7, 3, 1]])
    coords = torch.cat([c0, c1])
    logits = torch.randn((len(coords), 6), generator=g, dtype=torch.float64)
    edges = O.sector_edges(dr)
    assert torch.equal(edges, MU.sector_edges(dr)) and float(edges[0]) == 0.0 and float(edges[1]) == 6.5625
    d1 = torch.norm(c1[:, :3].float() - c1[:, :3].float().mean(0), dim=-1) * 0.05
    assert float(d1[0]) == float(edges[1])                           # on the edge: it belongs to sector 1, not 0
    want = np.stack(_batch2list_transcribed({"logits": logits, "coords": coords[:, :3], "batch_indices": coords[:, 3]}, dr))
    got = O.sector_means(logits, coords, dr)
    assert got.shape == (2, 96)
    assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    assert bool((got[0, 6 * 8:] == 0).all()) and bool((got[0, :6 * 4] != 0).all())          # empty far sectors: zeros
    assert bool((got[1, :6] == 0).all()) and torch.allclose(got[1, 6:12], logits[500:503].mean(0))


def test_frechet_formula_is_the_evaluators():
    from lidargen.metrics import eval_utils
    from lidargen.metrics.distribution import compute_frechet_distance

    g = np.random.default_rng(5)
    a, b = g.normal(size=(40, 6)), g.normal(size=(50, 6)) * 1.3 + 0.2
    got = eval_utils.compute_fd(a, b)
    assert abs(got - O.compute_fd(a, b)) <= 1e-12 * abs(got)
    assert abs(got - compute_frechet_distance(a, b)) <= 1e-9 * abs(got)      # the same quantity by other operations
    assert abs(eval_utils.compute_fd(a, a)) < 1e-6 * np.trace(np.cov(a, rowvar=False))


def _defines():
    src = open(os.path.join(ROOT, "include", "lidarcrafter_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(LC_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}


def test_limits_and_widths_refuse_before_any_launch():
    """The C entries check their arguments on the host: nothing is dereferenced or launched (callable without a GPU)."""
    from lidarcrafter_amd import _lib
    from lidarcrafter_amd import ops_spconv as KS

    d = _defines()
    EINVAL, EUNSUP = d["LC_EINVAL"], d["LC_EUNSUP"]
    assert (KS.TILE, KS.MAX_COORD, KS.MAX_BATCH) == (d["LC_SPCONV_TILE"], d["LC_SPCONV_MAX_COORD"], d["LC_SPCONV_MAX_BATCH"])
    assert d["LC_SPCONV_MAX_COORD"] == (1 << 18) - 1 and d["LC_SPCONV_MAX_BATCH"] < (1 << 9) - 1   # the key's fields, sign bit free
    h = _lib.lib()
    p = 4096
    nb = h.lc_spconv_hash_bytes(1000)
    assert nb == 2048 * 12 and h.lc_spconv_hash_bytes(0) == 0 and h.lc_spconv_hash_bytes(d["LC_SPCONV_MAX_ROWS"] + 1) == 0
    build = lambda n=1000, mc=100, nbatch=2, bytes_=nb: h.lc_spconv_hash_build(p, n, mc, nbatch, p, bytes_, None)
    assert build(mc=d["LC_SPCONV_MAX_COORD"] + 1) == EUNSUP
    assert build(nbatch=d["LC_SPCONV_MAX_BATCH"] + 2) == EUNSUP
    assert build(n=d["LC_SPCONV_MAX_ROWS"] + 1) == EUNSUP
    assert build(bytes_=nb - 1) == EINVAL and build(n=0) == EINVAL and build(mc=-1) == EINVAL
    assert h.lc_spconv_map(p, 10, 0, d["LC_SPCONV_MAX_STRIDE"] + 1, p, 10, p, None) == EUNSUP
    assert h.lc_spconv_map(p, 10, 3, 1, p, 10, p, None) == EINVAL
    assert h.lc_spconv_map(p, 10, 0, 1, None, 10, p, None) == EINVAL

    def fwd(Ci=16, Co=16, K=27, ldx=None, ldy=None, col=0, nbr=p, x=p, res=None, ldr=0, M=100):
        return h.lc_spconv_fwd(x, Ci if ldx is None else ldx, nbr, 100, p, p, res, ldr, p, Co + col if ldy is None else ldy,
                               col, M, Ci, Co, K, 1, None)

    for Ci, Co in ((24, 16), (8, 16), (16, 24), (16, 256), (256, 128), (3, 16)):
        assert fwd(Ci=Ci, Co=Co) == EUNSUP, (Ci, Co)
    assert fwd(K=9) == EUNSUP and fwd(K=2) == EUNSUP
    assert fwd(ldx=18) == EUNSUP and fwd(col=2) == EUNSUP and fwd(x=p + 4) == EUNSUP      # quads
    assert fwd(res=p, ldr=18) == EUNSUP
    assert fwd(nbr=None) == EINVAL and fwd(ldx=8) == EINVAL and fwd(ldy=8) == EINVAL and fwd(M=0) == EINVAL
    assert fwd(nbr=None, K=1, M=101) == EINVAL                       # the dense form reads row j of x for output row j
    assert h.lc_spconv_sector_means(p, 300, p, p, 2, 300, p, 0.05, p, None) == EUNSUP
    assert h.lc_spconv_sector_means(p, 8, p, p, 2, 16, p, 0.05, p, None) == EINVAL
    # the Python wrappers refuse CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KS.sparse_conv(torch.zeros(4, 16), None, torch.zeros(1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KS.hash_build(torch.zeros(4, 4, dtype=torch.int32), 1, 1)
    for c in O.CONFIG["model_params"]["layer_num"]:
        assert int(0.5 * c) in KS.WIDTHS_OUT
    assert all(c in KS.WIDTHS_IN for c in (4, 192, 96, 64))


# ---- the host side of the hash and width tests of tests/test_spconv.py ---------------------------------------------------
def test_restated_capacity_is_the_librarys():
    from lidarcrafter_amd import _lib

    assert tuple(H.sp_capacity(n) for n in H.CAPACITY_NS) == H.CAPACITIES == (1024, 1024, 1024, 2048, 2048, 4096)
    h = _lib.lib()
    for n in H.CAPACITY_NS + (400, 30000, 32768, 32769):
        assert h.lc_spconv_hash_bytes(n) == 12 * H.sp_capacity(n), n
    assert H.sp_capacity(30000) == 65536
    d = _defines()
    assert (H.MAX_COORD, H.MAX_BATCH) == (d["LC_SPCONV_MAX_COORD"], d["LC_SPCONV_MAX_BATCH"])
    # the largest key of all is not the empty marker, and every key is a non-negative int64
    top = H.sp_key(np.array([[H.MAX_COORD, H.MAX_COORD, H.MAX_COORD, H.MAX_BATCH]]))
    assert top[0] != H.EMPTY and int(top[0]) == (H.MAX_BATCH << 54) | ((1 << 54) - 1) and int(top[0]) >> 62 == 1
    for n in H.CAPACITY_NS:
        c = H.capacity_scene(n)
        assert c.shape == (n, 4) and len({tuple(r) for r in c.tolist()}) == n and sorted(set(c[:, 3].tolist())) <= [0, 1, 2]
    assert sorted(set(H.capacity_scene(513)[:, 3].tolist())) == [0, 1, 2]


def test_clustered_scene_exists():
    """300 keys of cloud 0 whose home slot is one of the last 8 of 1024, 100 ordinary rows, 50 absent coordinates whose
    home slot lies in the chain those 300 must form."""
    c, absent = H.clustered_scene()
    assert c.shape == (400, 4) and absent.shape == (50, 4) and H.sp_capacity(len(c)) == H.CLUSTER_CAP
    rows = {tuple(r) for r in c.tolist()}
    assert len(rows) == 400 and not rows & {tuple(r) for r in absent.tolist()}
    home = H.sp_slot(H.sp_key(c), H.CLUSTER_CAP)
    assert int((home >= H.CLUSTER_CAP - 8).sum()) >= 300
    ah = H.sp_slot(H.sp_key(absent), H.CLUSTER_CAP)
    assert bool(((ah >= H.CLUSTER_CAP - 8) | (ah < 200)).all())
    # a sequential insertion into 1024 slots: at least 292 of the 300 cannot stay in the last 8 slots
    want = O.nbr_same(c, 1)
    assert int(((want >= 0).sum(1) >= 2).sum()) >= 80                # the scene has neighbours
    assert bool((O._lookup(O._index(c), absent, O.offsets3(1))[:, 13] == -1).all())


def test_ordered_table_is_one_arrangement():
    """What invariant (iv) of H.table_invariants compares a built table with: the same slots whatever the order of the
    rows, every key behind smaller keys only, and the clustered keys wrapped over the end of the table."""
    c, _ = H.clustered_scene()
    keys, vals = H.ordered_table(c)
    for seed in (1, 2):
        perm = torch.randperm(len(c), generator=torch.Generator().manual_seed(seed))
        k2, v2 = H.ordered_table(c[perm])
        assert np.array_equal(k2, keys) and np.array_equal(perm.numpy()[v2[v2 >= 0]], vals[vals >= 0])
    disp, slots = H.displacements(keys, H.CLUSTER_CAP)
    assert len(slots) == 400 and int((slots < H.sp_slot(keys[slots], H.CLUSTER_CAP)).sum()) >= 250 and int(disp.max()) >= 250
    for h, d in zip(slots.tolist(), disp.tolist()):
        between = keys[(h - np.arange(1, d + 1)) % H.CLUSTER_CAP]
        assert bool((between < keys[h]).all())
    d = H.duplicate_scene()
    kd, vd = H.ordered_table(d)
    last = {tuple(r): i for i, r in enumerate(d.tolist())}
    assert int((kd != H.EMPTY).sum()) == 104 and sorted(vd[vd >= 0].tolist()) == sorted(last.values())


def test_scenes_are_what_they_claim():
    d = H.duplicate_scene()
    rows = {}
    for r in map(tuple, d.tolist()):
        rows[r] = rows.get(r, 0) + 1
    times = sorted(rows.values())
    assert len(rows) == 104 and times.count(1) == 40 and sorted(set(times)) == [1, 2, 3, 4, 5] and len(d) == 40 + 16 * 14
    for s in (1, 4):
        t = H.top_scene(s)
        top = H.MAX_COORD // s * s
        assert len({tuple(r) for r in t.tolist()}) == len(t) and int(t[:, :3].max()) == top and top + s == 1 << 18
        assert [top, top, top, H.MAX_BATCH] in t.tolist() and [top, top, top, H.MAX_BATCH - 1] in t.tolist()
        for axis in range(3):
            assert int((t[:, axis] == top).sum()) >= 5
        for x, y, z, b in t.tolist():                                # behind every top voxel: the origin of the next cloud
            if top in (x, y, z) and b < H.MAX_BATCH:
                assert [0, 0, 0, b + 1] in t.tolist()
    w = H.sweep_scene()
    assert w.shape == (30000, 4) and len(np.unique(H.sp_key(w))) == 30000 and H.sp_capacity(len(w)) == 65536
    assert sorted(set(w[:, 3].tolist())) == [0, 1]


@pytest.mark.parametrize("s", [1, 2, 4])
def test_sorted_oracle_is_the_dictionary_oracle(s):
    """The searchsorted oracle the 30 000-row scene is checked by, against O.nbr_* at 500 rows, on the rows at the top of
    every field and on rows that repeat (the last one wins in both)."""
    scenes = [H.capacity_scene(500) * torch.tensor([s, s, s, 1]), H.duplicate_scene() * torch.tensor([s, s, s, 1])]
    if s in (1, 4):
        scenes.append(H.top_scene(s))
    for c in scenes:
        coarse = O.down_coords(c, s)
        assert torch.equal(H.SortedOracle.nbr_same(c, s), O.nbr_same(c, s))
        assert torch.equal(H.SortedOracle.nbr_down(c, coarse, s), O.nbr_down(c, coarse, s))
        assert torch.equal(H.SortedOracle.nbr_up(c, coarse, s), O.nbr_up(c, coarse, s))
    assert int((O.nbr_same(scenes[0], s) >= 0).sum()) > 3 * 500


def _kernel_shapes(model):
    """{(Ci, Co, K, transposed)} of every `.kernel` of the model: ks 1 kernels have no offset axis; the transposed
    convolutions are the first of every up stage."""
    out = set()
    for k, v in model.state_dict().items():
        if k.endswith(".kernel"):
            transposed = bool(re.fullmatch(r"up\d\.0\.net\.0\.kernel", k))
            out.add((v.shape[-2], v.shape[-1], v.shape[0] if v.dim() == 3 else 1, transposed))
    return out


def test_conv_cases_cover_every_width_of_both_models():
    import test_spconv as TS
    from lidargen.metrics.models.spvcnn.model import Model as SPVCNN

    used = _kernel_shapes(_model()) | _kernel_shapes(SPVCNN(O.CONFIG))
    assert len(used) == 25 and (96, 64, 27, False) in used and (128, 64, 8, True) in used
    cases = set(TS.CONV_CASES)
    assert len(cases) == len(TS.CONV_CASES)
    for Ci, Co, K, transposed in sorted(used):
        assert (Ci, Co, K, transposed) in cases, (Ci, Co, K, transposed)
    assert any(K == 27 and Co == 64 for _, Co, K, _ in cases) and any(K == 27 and Ci == 96 for Ci, _, K, _ in cases)
    assert {Co // 16 for _, Co, _, _ in cases} == {1, 2, 3, 4, 8}    # every instance of the kernel
