"""Chamfer backward timing, one process, one JSON line per shape (profiles/chamfer_bwd.txt), D = 3:
  * ops.chamfer3d_backward: the inverse table built on the device (key kernel, one rocPRIM radix sort, binary search) and
    the two gather launches of csrc/chamfer_bwd.hip, all inside lc_chamfer3d_bwd; the kernel trace in profiles/ splits it;
  * the baseline: the same gradient written in torch ops -- gather, multiply, and index_add_ for the scattered terms
    (float atomics) -- on the same inputs in the same process;
  * shapes: B = 8, N = M = 1024 (objects), B = 1, N = M = 30000 (a sweep), and the funnel at N = M = 30000: every point
    of the first cloud within 1e-3 of ONE point of the second (a collapsed cloud), so one row of grad_xyz2 sums 30000
    scattered terms;
  * whether each formulation repeats its bits over 5 calls, and the largest difference between the two.
idx1 / idx2 come from ops.chamfer3d.  Times are host clocks around a call that ends in a device synchronise, median / min /
max over `reps` calls after 3 warm-up calls.
python devtools/chamfer_bwd_time.py [reps]
python devtools/chamfer_bwd_time.py trace CASE    3 + 10 calls of ops.chamfer3d_backward on one case and nothing else: the
                                                  program of a `rocprofv3 --kernel-trace --stats` run of its own"""
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
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def torch_backward(x, y, g1, g2, i1, i2):
    B, N, _ = x.shape
    M = y.shape[1]
    l1, l2 = i1.long(), i2.long()
    t1 = (g1 * 2)[..., None] * (x - torch.gather(y, 1, l1[..., None].expand(-1, -1, 3)))
    t2 = (g2 * 2)[..., None] * (y - torch.gather(x, 1, l2[..., None].expand(-1, -1, 3)))
    batch = torch.arange(B, device=x.device)[:, None]
    ga, gb = t1.clone(), t2.clone()
    ga.view(-1, 3).index_add_(0, (l2 + batch * N).view(-1), -t2.view(-1, 3))
    gb.view(-1, 3).index_add_(0, (l1 + batch * M).view(-1), -t1.view(-1, 3))
    return ga, gb


def main():
    trace = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "trace" else None
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 50
    assert torch.cuda.is_available(), "chamfer_bwd_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    box = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "host": platform.node()}
    print(json.dumps({"box": box, "reps": reps, "trace": trace}), flush=True)
    for name, B, n in (("objects", 8, 1024), ("sweep", 1, 30000), ("funnel", 1, 30000)):
        if trace and name != trace:
            continue
        g = torch.Generator().manual_seed(n + B)
        y = (torch.rand((B, n, 3), generator=g) * 50).to(dev)
        x = (torch.rand((B, n, 3), generator=g) * 50).to(dev)
        if name == "funnel":
            x = (y[:, n // 2:n // 2 + 1] + (torch.rand((B, n, 3), generator=g) - 0.5).to(dev) * 2e-3).contiguous()
        g1, g2 = torch.randn((B, n), generator=g).to(dev), torch.randn((B, n), generator=g).to(dev)
        _, _, i1, i2 = ops.chamfer3d(x, y)
        if trace:
            for _ in range(13):
                ops.chamfer3d_backward(x, y, g1, g2, i1, i2)
            torch.cuda.synchronize()
            continue
        seg_len = torch.bincount((i1.long() + torch.arange(B, device=dev)[:, None] * n).view(-1), minlength=B * n)
        out = {"case": name, "B": B, "N": n, "M": n, "scratch_kb": round(lib().lc_chamfer_bwd_scratch_bytes(B, n, n) / 1024, 1),
               "longest_segment_into_xyz2": int(seg_len.max()),
               "rows_of_xyz2_with_more_than_32_sources": int((seg_len > 32).sum())}
        ours = ops.chamfer3d_backward(x, y, g1, g2, i1, i2)
        base = torch_backward(x, y, g1, g2, i1, i2)
        out["max_abs_diff_ours_vs_torch"] = max(float((a - b).abs().max()) for a, b in zip(ours, base))
        out["max_abs_gradient"] = max(float(a.abs().max()) for a in ours)
        out["ours_repeats_bits"] = all(all(torch.equal(a, b) for a, b in zip(ours, ops.chamfer3d_backward(x, y, g1, g2, i1, i2)))
                                      for _ in range(5))
        out["torch_repeats_bits"] = all(all(torch.equal(a, b) for a, b in zip(base, torch_backward(x, y, g1, g2, i1, i2)))
                                       for _ in range(5))
        out["ours_whole_call"] = timed(lambda: ops.chamfer3d_backward(x, y, g1, g2, i1, i2), reps)
        out["torch_ops_index_add"] = timed(lambda: torch_backward(x, y, g1, g2, i1, i2), reps)
        out["forward_chamfer3d"] = timed(lambda: ops.chamfer3d(x, y), reps)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
