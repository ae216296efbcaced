"""Device against host route of lidargen/metrics/distribution.py, one process, the same inputs, JSON lines
(profiles/stats_f64.txt).  Synthetic ReLU features in float64 (tests/_stats_oracle.py features) at the three shapes of the
evaluator:
  * compute_frechet_distance, 2 x 1000 x 1808 (PointNet's width) and 2 x 2000 x 4096 (RangeNet's 'lidargen' width);
  * compute_squared_mmd, 100 subsets x 1000 rows x 1024 (PointMLP's width; 2 x 1200 objects), after the same seed.
Per call: a host clock around the call, which ends in a device synchronise (the result is a Python float) and includes the
upload of the numpy features -- END-TO-END call times, not kernel times; no kernel trace is taken here.  The device route is
warmed once and then timed `rounds` times (median, min ... max); the host route is timed once (it takes seconds).  Both
values and their difference are recorded, with the route, k and the Jacobi sweeps of the device.
The tile engine alone: device events around `reps` back-to-back products at the shapes those calls multiply, as a rate and
as a share of the float64 matrix peak (78.6 TFLOP/s, the data sheet's figure for the MI355X; a per-CALL rate that includes
the launch gap and the allocation of the result).
python devtools/stats_time.py [out_path rounds reps]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _stats_oracle as O  # noqa: E402
from lidarcrafter_amd import ops_stats as S  # noqa: E402
from lidargen.metrics import distribution as D  # noqa: E402

F64_MATRIX_PEAK_TFLOPS = 78.6


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def per_call_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stats_f64.txt")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    assert torch.cuda.is_available(), "the timing needs the GPU; nothing is measured without it"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").close()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        with open(out_path, "a") as f:              # line by line: a later failure keeps what was measured
            f.write(line + "\n")

    emit({"device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
          "host_threads": torch.get_num_threads(), "torch": torch.__version__, "rounds": rounds, "reps": reps,
          "times": "end-to-end call times (host clock, upload included); no kernel trace taken"})

    for n, d in ((1000, 1808), (2000, 4096)):
        x1, x2 = O.features(n, d, 1), O.features(n, d, 2, shift=0.1)
        info = {}
        t1, t2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
        S.frechet_distance(t1, t2, info=info)                                   # warm-up, and the route's record
        dev_t = []
        for _ in range(rounds):
            ms, dev = wall_ms(lambda: D.compute_frechet_distance(x1, x2, device="cuda"))
            dev_t.append(ms)
        host_ms, host = wall_ms(lambda: D.compute_frechet_distance(x1, x2))
        emit({"call": "compute_frechet_distance", "shape": [2, n, d], **info, "device": stats(dev_t),
              "host_ms": round(host_ms, 1), "host_over_device": round(host_ms / statistics.median(dev_t), 1),
              "device_value": dev, "host_value": host, "relative_difference": abs(dev - host) / abs(host)})
        del t1, t2

    n, width, subsets, m = 1200, 1024, 100, 1000
    f1, f2 = O.features(n, width, 3), O.features(n, width, 4, shift=0.1)
    np.random.seed(0)
    D.compute_squared_mmd(f1, f2, num_subsets=2, device="cuda")                 # warm-up
    dev_t = []
    for _ in range(rounds):
        np.random.seed(1)
        ms, dev = wall_ms(lambda: D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=m, device="cuda"))
        dev_t.append(ms)
    np.random.seed(1)
    host_ms, host = wall_ms(lambda: D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=m))
    flop = subsets * 3 * 2.0 * m * m * width
    emit({"call": "compute_squared_mmd", "shape": [subsets, m, width], "sets": [n, n], "device": stats(dev_t),
          "host_ms": round(host_ms, 1), "host_over_device": round(host_ms / statistics.median(dev_t), 1),
          "device_value": dev, "host_value": host, "relative_difference": abs(dev - host) / abs(host),
          "gram_tflop": round(flop / 1e12, 3),
          "call_tflops": round(flop / (statistics.median(dev_t) * 1e-3) / 1e12, 2),
          "call_share_of_f64_matrix_peak": round(flop / (statistics.median(dev_t) * 1e-3) / 1e12 / F64_MATRIX_PEAK_TFLOPS, 3)})

    # the engine alone, at the products of the calls above
    for name, form, ps, qs in (("B A^T 2000 x 4096", "nt", (2000, 4096), (2000, 4096)),
                               ("M^T M 2000 x 2000", "tn", (2000, 2000), (2000, 2000)),
                               ("A^T A 4096 x 2000", "tn", (2000, 4096), (2000, 4096)),
                               ("B A^T 1000 x 1808", "nt", (1000, 1808), (1000, 1808))):
        rng = np.random.RandomState(0)
        p, q = torch.from_numpy(rng.randn(*ps)).cuda(), torch.from_numpy(rng.randn(*qs)).cuda()
        out = S.matmul(p, q, form)
        M, N = out.shape
        K = ps[1] if form == "nt" else ps[0]
        t = [per_call_ms(lambda: S.matmul(p, q, form), reps) for _ in range(rounds)]
        tf = 2.0 * M * N * K / (statistics.median(t) * 1e-3) / 1e12
        emit({"engine": name, "form": form, "M_N_K": [M, N, K], **stats(t), "tflops": round(tf, 2),
              "share_of_f64_matrix_peak": round(tf / F64_MATRIX_PEAK_TFLOPS, 3)})


if __name__ == "__main__":
    main()
