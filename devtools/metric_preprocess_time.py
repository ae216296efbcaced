"""Host against device preprocessing of the three learned scores, one process, JSON lines (profiles/metric_preprocess.txt).
Synthetic nuScenes-sized float32 sweeps (testing.synth_points, `points` each) at the three workload shapes of the front-ends:
100 clouds (FRID, compute_range_logits), 50 (FSVD, compute_logits 'voxel'), 25 (FPVD, compute_point_voxel_logits); seeded
extractors (RangeNet-53, the MinkUNet and the SPVCNN of the shipped configuration).  Per shape, same process, same inputs,
after a warm-up pass of each, `rounds` alternating wall-clock passes with a device synchronisation at both ends, medians:
  * the preprocessing alone up to the network's input on the device -- host: per-cloud numpy, stack / collate, upload;
    device: preprocess_range_batch / pcd2voxel_batch (one upload, the kernels, for voxels the one read-back);
  * the whole compute_*_logits call, preprocess_device=None against 'cuda'.
And what the contract on float32 clouds costs the range route: the share of points whose pixel differs between the host's
float32 evaluation and the float64 evaluation of the widened cloud (the device route's definition, which the tests pin bit
for bit), the share of image pixels whose depth differs between the two routes' images, and the largest difference of the
seeded RangeNet's feature rows.  The voxel triples of the two routes are compared for equality.
python devtools/metric_preprocess_time.py [out_path points rounds]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import _rangenet_oracle as RO  # noqa: E402
from fpvd_time import seeded_model  # noqa: E402
from lidarcrafter_amd.testing import seeded_fill_rangenet, synth_points  # noqa: E402
from lidargen.metrics import DATASET_CONFIG, metric_utils as MU  # noqa: E402
from lidargen.metrics.models.minkowskinet.model import Model as MinkUNet  # noqa: E402
from lidargen.metrics.models.rangenet.model import Model as RangeNet  # noqa: E402
from lidargen.metrics.models.spvcnn.model import Model as SPVCNN  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(fns, rounds):
    """{name: {'median_ms', 'min_ms', 'max_ms'}} of `rounds` alternating passes after one warm-up pass of each."""
    for fn in fns.values():
        wall_ms(fn)
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(wall_ms(fn)[0])
    return {k: {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}
            for k, v in ts.items()}


def pixels(cloud, size, fov, depth_range, **_):
    """(mask, column, row) per point by pcd2range's lines in the dtype of `cloud`."""
    fov_up, fov_down = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
    fov_range = abs(fov_down) + abs(fov_up)
    depth = np.linalg.norm(cloud, 2, axis=1)
    mask = np.logical_and(depth > depth_range[0], depth < depth_range[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        yaw = -np.arctan2(cloud[:, 1], cloud[:, 0])
        pitch = np.arcsin(cloud[:, 2] / depth)
    proj_x = 0.5 * (yaw / np.pi + 1.0)
    proj_y = 1.0 - (pitch + abs(fov_down)) / fov_range
    proj_x *= size[1]
    proj_y *= size[0]
    col = np.maximum(0, np.minimum(size[1] - 1, np.floor(proj_x))).astype(np.int32)
    row = np.maximum(0, np.minimum(size[0] - 1, np.floor(proj_y))).astype(np.int32)
    return mask, col, row


def main():
    args = sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "metric_preprocess.txt")
    points, rounds = (int(v) for v in (args[1:3] + ["30000", "5"][len(args[1:3]):]))
    assert torch.cuda.is_available(), "metric_preprocess_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    cfg = DATASET_CONFIG["nuscenes"]
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    emit({"box": {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
                  "numpy": np.__version__}, "points_per_cloud": points, "rounds": rounds, "cloud_dtype": "float32"})
    clouds = [np.ascontiguousarray(synth_points(points, 100 + i)[:, :3]) for i in range(100)]

    with torch.no_grad():
        # ---- FRID: 100 clouds ------------------------------------------------------------------------------------------
        net = seeded_fill_rangenet(RangeNet(RO.config(53)), 1).eval().requires_grad_(False).to(dev)
        pre = alternate({"host": lambda: torch.from_numpy(np.stack([MU.preprocess_range(c, **cfg) for c in clouds])).float().to(dev),
                         "device": lambda: MU.preprocess_range_batch(clouds, dev, **cfg)}, rounds)
        whole = alternate({"host": lambda: MU.compute_range_logits("32", clouds, model=net),
                           "device": lambda: MU.compute_range_logits("32", clouds, model=net, preprocess_device="cuda")}, rounds)
        emit({"compute_range_logits": {"clouds": 100, "preprocessing": pre, "whole_call": whole}})
        moved = kept = 0
        for c in clouds:
            m32, c32, r32 = pixels(c, **cfg)
            m64, c64, r64 = pixels(c.astype(np.float64), **cfg)
            both = m32 & m64
            kept += int((m32 | m64).sum())
            moved += int(((c32 != c64) | (r32 != r64))[both].sum()) + int((m32 != m64).sum())
        img_h = torch.from_numpy(np.stack([MU.preprocess_range(c, **cfg) for c in clouds])).float()
        img_d = MU.preprocess_range_batch(clouds, dev, **cfg).cpu()
        (rows_h,) = MU.compute_range_logits("32", clouds, model=net)
        (rows_d,) = MU.compute_range_logits("32", clouds, model=net, preprocess_device="cuda")
        emit({"float32_contract": {"points_in_range": kept, "points_in_another_pixel": moved,
                                   "share_of_points": moved / max(kept, 1),
                                   "depth_pixels_that_differ": int((img_h[:, 0] != img_d[:, 0]).sum()),
                                   "share_of_depth_pixels": float((img_h[:, 0] != img_d[:, 0]).float().mean()),
                                   "rangenet53_feature_rows": {"max_abs_difference": float(np.abs(rows_h - rows_d).max()),
                                                               "max_abs_feature": float(np.abs(rows_h).max()),
                                                               "worst_row_rel_l2": float(max(np.linalg.norm(a - b) / np.linalg.norm(a)
                                                                                             for a, b in zip(rows_h, rows_d)))}}})
        del net

        # ---- FSVD: 50 clouds, FPVD: 25 clouds --------------------------------------------------------------------------
        for name, cls, n, call in (("compute_logits_voxel", MinkUNet, 50, lambda cl, m, **k: MU.compute_logits("32", "voxel", cl, model=m, **k)),
                                   ("compute_point_voxel_logits", SPVCNN, 25, lambda cl, m, **k: MU.compute_point_voxel_logits("32", cl, model=m, **k))):
            net = seeded_model(cls, dev)
            sub = clouds[:n]
            pre = alternate({"host": lambda: MU.sparse_collate([MU.pcd2voxel(MU.preprocess_pcd(c, **cfg)) for c in sub], dev),
                             "device": lambda: MU.pcd2voxel_batch(sub, dev, depth_range=cfg["depth_range"])}, rounds)
            whole = alternate({"host": lambda: call(sub, net), "device": lambda: call(sub, net, preprocess_device="cuda")}, rounds)
            th = MU.sparse_collate([MU.pcd2voxel(MU.preprocess_pcd(c, **cfg)) for c in sub], dev)
            td = MU.pcd2voxel_batch(sub, dev, depth_range=cfg["depth_range"])
            (rows_h,), (rows_d,) = call(sub, net), call(sub, net, preprocess_device="cuda")
            emit({name: {"clouds": n, "voxels": int(th[1].shape[0]), "preprocessing": pre, "whole_call": whole,
                         "triples_equal": bool(all(torch.equal(a, b) for a, b in zip(th, td))),
                         "feature_rows_equal": bool(np.array_equal(rows_h, rows_d))}})
            del net
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
