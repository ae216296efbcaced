"""EMD timing, one process, one JSON line per shape (profiles/emd.txt):
  * ops.emd_forward at eps = 0.005, 50 iterations (what compute_pairwise_emd runs) on uniform random clouds in [0, 1)^3:
    B = 1, n = 32768 (the shape eval_utils.compute_emd produces for a nuScenes frame) and B = 8, n = 8192;
  * the same call at 1 iteration: the first bid pass (every point bids: n x n values) plus the fixed passes;
  * the yardstick: ops.chamfer3d at the same B, n -- TWO directions of n x n squared distances, the first bid pass is the
    pair work of one of them (with a square root and two float64 subtractions per pair on top);
  * launches per call (counted from the call's structure: init + 3 per iteration + dist) and the scratch size.
Times are host clocks around a call that ends in a device synchronise, median / min / max over `reps` calls after warm-up.
python devtools/emd_time.py [reps]"""
import json
import os
import platform
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidarcrafter_amd import ops  # noqa: E402
from lidarcrafter_amd._lib import lib  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    assert torch.cuda.is_available(), "emd_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    box = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "host": platform.node()}
    print(json.dumps({"box": box, "reps": reps}), flush=True)
    for B, n in ((1, 32768), (8, 8192), (1, 8192), (1, 2048)):
        g = torch.Generator().manual_seed(n + B)
        a = torch.rand((B, n, 3), generator=g).to(dev)
        b = torch.rand((B, n, 3), generator=g).to(dev)
        out = {"B": B, "n": n, "eps": 0.005, "iters": 50}
        d, asg = ops.emd_forward(a, b, 0.005, 50)
        out["emd_mean_sqrt_dist"] = round(float(d.sqrt().mean()), 6)
        out["distinct_objects_frac"] = round(sum(int(r.unique().numel()) for r in asg) / (B * n), 4)
        d2, asg2 = ops.emd_forward(a, b, 0.005, 50)
        out["repeatable"] = bool(torch.equal(d, d2) and torch.equal(asg, asg2))
        out["emd_50_iters"] = timed(lambda: ops.emd_forward(a, b, 0.005, 50), reps)
        out["emd_1_iter"] = timed(lambda: ops.emd_forward(a, b, 0.005, 1), reps)
        out["chamfer3d_both_directions"] = timed(lambda: ops.chamfer3d(a, b), reps)
        out["launches_per_call_50_iters"] = 1 + 3 * 50 + 1
        out["scratch_mb"] = round(lib().lc_emd_scratch_bytes(B, n) / 2 ** 20, 2)
        per_iter = (out["emd_50_iters"]["median_ms"] - out["emd_1_iter"]["median_ms"]) / 49
        out["later_iterations_mean_ms"] = round(per_iter, 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
