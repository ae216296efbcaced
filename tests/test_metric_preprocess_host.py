"""CPU tests of the batched device front-end of FRID / FSVD / FPVD (lidarcrafter_amd/ops_metric_pre.py, metric_utils.
preprocess_range_batch / pcd2voxel_batch, the `preprocess_device` keyword): the keyword exists everywhere and None is the
unchanged path, the refusals, the key width, the header, and the cap of the drop rule on the GPU tests' own inputs."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metric_preprocess_cases as cases  # noqa: E402

from lidarcrafter_amd import ops_metric_pre as KP  # noqa: E402
from lidargen.metrics import eval_utils  # noqa: E402
from lidargen.metrics import metric_utils as MU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = (MU.compute_range_logits, MU.compute_logits, MU.compute_point_voxel_logits, eval_utils.compute_frid,
       eval_utils.compute_fsvd, eval_utils.compute_fpvd)


def test_the_keyword_is_accepted_by_all_six_functions_and_defaults_to_none():
    for fn in SIX + (MU._sector_features,):
        p = inspect.signature(fn).parameters["preprocess_device"]
        assert p.default is None, fn.__name__
    for fn in (MU.preprocess_range_batch, MU.pcd2voxel_batch):
        assert inspect.signature(fn).parameters["device"].default == "cuda"


class _Stop(Exception):
    pass


class _Net(torch.nn.Module):
    """Stands in for an extractor: it has a parameter (the front-ends ask for its device) and stops the call."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, *a, **k):
        raise _Stop()


def test_none_calls_the_unchanged_path(monkeypatch):
    """With the keyword left out or None the three front-ends prepare their input cloud by cloud on the host, through
    preprocess_range / preprocess_pcd + pcd2voxel + sparse_collate, and never touch the batched functions."""
    calls = []

    def spy(name):
        real = getattr(MU, name)

        def f(*a, **k):
            calls.append(name)
            return real(*a, **k)

        monkeypatch.setattr(MU, name, f)

    def never(*a, **k):
        raise AssertionError("the batched route was taken")

    for name in ("preprocess_range", "preprocess_pcd", "pcd2voxel", "sparse_collate"):
        spy(name)
    monkeypatch.setattr(MU, "preprocess_range_batch", never)
    monkeypatch.setattr(MU, "pcd2voxel_batch", never)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)           # (nothing below reaches the GPU)
    clouds = [cases.sweep(1, 40, np.float64), cases.sweep(2, 30, np.float64)]
    for kw in ({}, {"preprocess_device": None}):
        calls.clear()
        with pytest.raises(_Stop):
            MU.compute_range_logits("32", clouds, model=_Net(), size=(4, 16), **kw)
        assert calls == ["preprocess_range"] * 2
        for fn, args in ((MU.compute_logits, ("32", "voxel", clouds)), (MU.compute_point_voxel_logits, ("32", clouds))):
            calls.clear()
            with pytest.raises(_Stop):
                fn(*args, model=_Net(), **kw)
            assert calls == ["preprocess_pcd", "pcd2voxel"] * 2 + ["sparse_collate"]


def test_cuda_takes_the_batched_route(monkeypatch):
    seen = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(MU, "check_preprocess_device", lambda d, need_gpu=True: torch.device("cuda", 0))
    monkeypatch.setattr(MU, "preprocess_range_batch", lambda clouds, device, **cfg: seen.append(("range", len(clouds), cfg["size"])) or torch.zeros(1))
    monkeypatch.setattr(MU, "pcd2voxel_batch", lambda clouds, device, depth_range: seen.append(("voxel", len(clouds), depth_range)) or (torch.zeros(1),) * 3)
    monkeypatch.setattr(MU, "preprocess_range", lambda *a, **k: pytest.fail("the host route was taken"))
    monkeypatch.setattr(MU, "pcd2voxel", lambda *a, **k: pytest.fail("the host route was taken"))
    clouds = [cases.sweep(1, 40, np.float64)] * 3
    with pytest.raises(_Stop):
        MU.compute_range_logits("32", clouds, model=_Net(), size=(4, 16), preprocess_device="cuda")
    with pytest.raises(_Stop):
        MU.compute_logits("32", "voxel", clouds, model=_Net(), preprocess_device="cuda")
    with pytest.raises(_Stop):
        MU.compute_point_voxel_logits("32", clouds, model=_Net(), preprocess_device="cuda")
    assert seen == [("range", 3, [4, 16]), ("voxel", 3, [1.0, 45.0]), ("voxel", 3, [1.0, 45.0])]


def test_an_unknown_value_and_a_missing_gpu_raise(monkeypatch):
    clouds = [cases.sweep(1, 40, np.float64)]
    for bad in ("cpu", "hip", 3.5, torch.device("cpu")):
        with pytest.raises(ValueError, match="not a"):
            MU.compute_range_logits("32", clouds, model=_Net(), preprocess_device=bad)
        with pytest.raises(ValueError, match="not a"):
            MU.compute_logits("32", "voxel", clouds, model=_Net(), preprocess_device=bad)
        with pytest.raises(ValueError, match="not a"):
            MU.compute_point_voxel_logits("32", clouds, model=_Net(), preprocess_device=bad)
        with pytest.raises(ValueError, match="not a"):
            MU.preprocess_range_batch(clouds, bad, **cases.CFG["4x16"])
        with pytest.raises(ValueError, match="not a"):
            MU.pcd2voxel_batch(clouds, bad, depth_range=cases.DEPTH_RANGE)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for call in (lambda: MU.preprocess_range_batch(clouds, "cuda", **cases.CFG["4x16"]),
                 lambda: MU.pcd2voxel_batch(clouds, "cuda", depth_range=cases.DEPTH_RANGE),
                 lambda: MU.compute_range_logits("32", clouds, model=_Net(), preprocess_device="cuda"),
                 lambda: MU.compute_logits("32", "voxel", clouds, model=_Net(), preprocess_device="cuda"),
                 lambda: MU.compute_point_voxel_logits("32", clouds, model=_Net(), preprocess_device="cuda"),
                 lambda: eval_utils.compute_frid(clouds, clouds, "32", model=_Net(), preprocess_device="cuda"),
                 lambda: eval_utils.compute_fsvd(clouds, clouds, "32", model=_Net(), preprocess_device="cuda"),
                 lambda: eval_utils.compute_fpvd(clouds, clouds, "32", model=_Net(), preprocess_device="cuda")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # CPU tensors and mixtures are no input of the device route, whatever the machine
    monkeypatch.setattr(KP, "_device", lambda d, need_gpu=True: torch.device("cpu"))
    with pytest.raises(TypeError, match="CUDA"):
        KP.ragged([torch.zeros(3, 3)], "cuda")
    with pytest.raises(TypeError, match="one dtype"):
        KP.ragged([np.zeros((3, 3), np.float32), np.zeros((3, 3))], "cuda")
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        KP.ragged([np.zeros((3, 4))], "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KP.range_images(torch.zeros(3, 3), torch.zeros(2, dtype=torch.int32), [4, 16], [10, -30], [1.0, 45.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KP.voxelize(torch.zeros(3, 3), torch.zeros(2, dtype=torch.int32), [1.0, 45.0], 0.05)


def test_remission_labels_and_an_empty_batch_are_refused_by_name():
    clouds = [cases.sweep(1, 40, np.float64)]
    with pytest.raises(NotImplementedError, match="`remission=`"):
        MU.preprocess_range_batch(clouds, "cuda", remission=np.zeros(40), **cases.CFG["4x16"])
    with pytest.raises(NotImplementedError, match="`labels=`"):
        MU.preprocess_range_batch(clouds, "cuda", labels=np.zeros(40), **cases.CFG["4x16"])
    with pytest.raises(ValueError, match="an empty batch"):
        MU.preprocess_range_batch([], "cuda", **cases.CFG["4x16"])
    with pytest.raises(ValueError, match="an empty batch"):
        MU.pcd2voxel_batch([], "cuda", depth_range=cases.DEPTH_RANGE)
    with pytest.raises(ValueError, match="an empty batch"):
        MU.sparse_collate([])                                                   # ... as the host route does


def test_key_width_refusal():
    """The sort key is (cloud, x, y, z) in bit fields: the cloud field holds 0 ... B, an axis field q + R with R =
    ceil(hi / voxel) + 2.  More than 64 bits together are refused by name, on the host, before any upload."""
    assert KP.voxel_key_bits(50, 45.0, 0.05) == (6, 33)            # 2 * 902 + 1 = 1805 < 2^11
    assert KP.voxel_key_bits(25, 56.0, 0.05) == (5, 36)            # KITTI: 2 * 1122 + 1 = 2245 < 2^12
    assert KP.voxel_key_bits(1, 45.0, 0.05)[0] == 1 and KP.voxel_key_bits(63, 45.0, 0.05)[0] == 6
    assert KP.voxel_key_bits(64, 45.0, 0.05)[0] == 7
    assert KP.voxel_key_bits(127, 13000.0, 0.05) == (7, 57)        # 2 * 260002 + 1 < 2^19: 64 bits, the last that fit
    with pytest.raises(NotImplementedError, match="8 cloud-index bits .* 57 key bits .* exceed 64"):
        KP.voxel_key_bits(128, 13000.0, 0.05)
    with pytest.raises(NotImplementedError, match="exceed 64"):
        MU.pcd2voxel_batch([np.zeros((1, 3))] * 2, "cuda", depth_range=[1.0, 1.0e6])
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    p = 4096
    assert h.lc_voxel_batch_fwd(p, 0, p, 2, 8, 1.0, 1.0e6, 0.05, p, p, p, p, None) == -2       # LC_EUNSUP, nothing launched
    assert h.lc_voxel_batch_fwd(None, 0, p, 2, 8, 1.0, 45.0, 0.05, p, p, p, p, None) == -1
    assert h.lc_voxel_batch_fwd(p, 0, p, 2, 0, 1.0, 45.0, 0.05, p, p, p, p, None) == -1
    assert h.lc_voxel_batch_fwd(p, 0, p, 2, 8, 45.0, 1.0, 0.05, p, p, p, p, None) == -1
    assert h.lc_voxel_batch_scratch_bytes(0, 1) == 0
    assert h.lc_range_batch_fwd(p, 2, p, 1, 8, 4, 16, 1.0, 45.0, 1.0, 45.0, 0.5, 0.7, p, p, p, None) == -1
    assert h.lc_range_batch_fwd(p, 0, p, 0, 8, 4, 16, 1.0, 45.0, 1.0, 45.0, 0.5, 0.7, p, p, p, None) == -1
    assert h.lc_range_batch_fwd(p, 0, p, 1, 8, 4, 16, 1.0, 45.0, 1.0, 45.0, 0.5, 0.7, None, p, p, None) == -1


def test_the_drop_rule_cap_holds_on_the_test_inputs():
    total = sum(cases.range_batch(*c)[1] for c in cases.RANGE_CASES)
    dropped = sum(cases.range_batch(*c)[2] for c in cases.RANGE_CASES)
    assert total == 4 * sum(sum(b) for b in cases.BATCHES.values()) > 20000
    print(f"[metric_preprocess] the drop rule takes {dropped} of {total} points")
    assert dropped / total <= cases.DROP_CAP, (dropped, total)
    for c in cases.RANGE_CASES:                                       # what is left is clear of every boundary
        cfg = cases.CFG[c[0]]
        for cloud in cases.range_batch(*c)[0]:
            assert cloud.dtype == np.dtype(c[2])
            if cloud.shape[0]:
                px, py = cases.pixel_coordinates(cloud, cfg)
                assert float(np.abs(px - np.rint(px)).min()) >= cases.DROP_TOL and float(np.abs(py - np.rint(py)).min()) >= cases.DROP_TOL
    sizes = sorted(n for b in cases.BATCHES.values() for n in b)
    assert sizes[:5] == [0, 0, 1, 63, 64] and 65 in sizes and sizes[-1] > 1900 and sorted(cases.BATCHES) == [1, 3, 5]


def test_the_direction_table_is_range2xyz_of_an_all_ones_image():
    for H, W, fov in ((4, 16, [10, -30]), (32, 1024, [10, -30]), (64, 1024, [3, -25])):
        ones = MU.range2xyz(np.ones((H, W), np.float32), log_scale=False, fov=fov, depth_range=[0.0, 2.0])
        table = KP.ray_directions_host(H, W, fov)
        assert table.dtype == np.float64 and table.shape == (3, H, W) and np.array_equal(table, ones)


def test_the_header_declares_the_new_symbols():
    from lidarcrafter_amd import _lib, build

    src = open(os.path.join(ROOT, "include", "lidarcrafter_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("lc_range_batch_fwd", "lc_voxel_batch_fwd", "lc_voxel_batch_scratch_bytes", "lc_voxel_batch_key_bits"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert "metric_preprocess.hip" in build.SOURCES
