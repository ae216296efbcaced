"""MMD timing, one process, one JSON line per case (profiles/mmd.txt): eval_utils.compute_mmd's work on synthetic sweeps for
R = S = 64 and 256 at '32' (120 x 120 cells) and '64' (200 x 200), on two routes over the SAME inputs:
  * grid:    chamfer.bev_min_matching(route='grid')    -- bitmaps, integer distance transforms, pair sums (csrc/bev_chamfer.hip);
  * literal: chamfer.bev_min_matching(route='literal') -- pcd2bev_bin, then compute_pairwise_cd_batch per reference cloud
             (padding to the longest set with points at 1e6, chamfer_2DDist), as the reference's compute_mmd does.
Sweeps: 30 000 points, polar, radius |N(0, sigma)| with sigma in [8, 25] m (a nuScenes-sized sweep fills a few thousand cells).
The two routes alternate inside one process after a warm-up call of each; times are host clocks around a call that ends
with its result on the host, median / min / max.  The literal route's score must agree with the grid route's within the
float32 tolerance 2^-21 max(nx, ny) + 1e-5.
python devtools/mmd_time.py [out_file] [reps]"""
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidargen.metrics import chamfer, metric_utils  # noqa: E402


def sweeps(seed, count, points=30000):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        r = np.abs(rng.normal(0.0, rng.uniform(8.0, 25.0), points))
        th = rng.uniform(0.0, 2.0 * np.pi, points)
        out.append(torch.from_numpy(np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-3, 1, points)], 1)
                                    .astype(np.float32)).cuda())
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    out_file = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mmd.txt")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    assert torch.cuda.is_available(), "mmd_time.py measures on the GPU only"
    lines = [json.dumps({"box": {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
                                 "torch": torch.__version__, "host": platform.node()}, "reps": reps})]
    print(lines[-1], flush=True)
    for data in ("32", "64"):
        cfg = metric_utils.DATA_CONFIG[data]
        for n in (64, 256):
            ref, smp = sweeps(n, n), sweeps(n + 1, n)
            run = {r: (lambda r=r: chamfer.bev_min_matching(ref, smp, cfg["x"], cfg["y"], 0.5, route=r))
                   for r in ("grid", "literal")}
            first = {r: clock(run[r]) for r in ("grid", "literal")}       # warm-up (code objects, allocator), kept
            ts = {"grid": [], "literal": []}
            for _ in range(reps):
                for r in ("grid", "literal"):
                    ts[r].append(clock(run[r])[0])
            g, l = first["grid"][1][0], first["literal"][1][0]
            cells = [c.shape[0] for c in metric_utils.pcd2bev_bin(data, ref)[0]]
            side = 120 if data == "32" else 200
            row = {"data": data, "R": n, "S": n, "cells_per_set_mean": round(float(np.mean(cells)), 1),
                   "cells_per_set_max": int(max(cells)), "mmd_grid": float(g.mean()), "mmd_literal": float(l.mean()),
                   "worst_pair_rel_diff": float(np.max(np.abs(g - l) / g)), "tolerance": 2.0 ** -21 * side + 1e-5,
                   "first_call_ms": {r: round(first[r][0], 3) for r in first},
                   "grid": stats(ts["grid"]), "literal": stats(ts["literal"])}
            row["literal_over_grid"] = round(row["literal"]["median_ms"] / row["grid"]["median_ms"], 2)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
