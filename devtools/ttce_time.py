"""TTCE timing, one process, one JSON line per measurement (profiles/temporal_metrics.txt):
  * synthetic sweeps of ~30 000 points (tests/_icp_oracle.py: ring pattern on a ground plane inside walls), a 10-frame
    sequence whose poses are 0.4 m and 0.4 degrees apart, so the pairs 3 and 4 frames apart differ by 1.2 - 1.7 m;
  * ops.icp_point_to_point at radius 2.0 on ONE pair (frames 0 -> 3) and on the 13 pairs of the sequence (what
    calculate_single_sequence_TTCE sends), grid build included; the grid build alone; one correspondence pass alone;
  * the same over the cell edge h / radius of the grid;
  * two yardsticks in the same process on the same pair:
      parent route  the same loop with every pass done by the brute-force ops.chamfer3d on float32 copies plus torch ops
                    for the masked sums and the SVD (what this repository could do before csrc/icp.hip),
      CPU route     the numpy / scipy cKDTree restatement (tests/_icp_oracle.py icp), one thread;
  * launches per call, counted from the call's structure: 4 for the grids + init + (max_iteration + 1) x (pass, update).
Times are host clocks around calls that end in a device synchronise, median / min / max over `reps` calls after warm-up.
python devtools/ttce_time.py [reps]"""
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
import _icp_oracle as O  # noqa: E402
from lidarcrafter_amd import ops  # noqa: E402

RADIUS = 2.0
N = 30000


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def parent_route(src, tgt, radius, max_iteration=30, rel=1e-6):
    """The ICP loop on what the parent commit offers: brute-force float32 chamfer for the correspondences, torch for the
    rest; float64 transform and sums, one host read-back per iteration for the stopping rule."""
    T = torch.eye(4, dtype=torch.float64, device=src.device)
    tgt32 = tgt.float()[None]
    r2 = radius * radius

    def one_pass(T):
        p = src @ T[:3, :3].T + T[:3, 3]
        d1, _, i1, _ = ops.chamfer3d(p.float()[None], tgt32)
        q = tgt[i1[0].long()]
        d2 = ((p - q) ** 2).sum(dim=1)
        m = d2 <= r2
        n = m.sum()
        return p, q, m, n, (n / len(src)).item(), (torch.sqrt((d2 * m).sum() / n).item() if n > 0 else 0.0)

    p, q, m, n, fit, rmse = one_pass(T)
    it = 0
    for it in range(1, max_iteration + 1):
        if n > 0:
            w = m.to(torch.float64)[:, None]
            mp, mq = (p * w).sum(0) / n, (q * w).sum(0) / n
            H = ((q - mq) * w).T @ (p - mp) / n
            U, S, Vt = torch.linalg.svd(H)
            D = torch.eye(3, dtype=torch.float64, device=src.device)
            D[2, 2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
            R = U @ D @ Vt
            upd = torch.eye(4, dtype=torch.float64, device=src.device)
            upd[:3, :3], upd[:3, 3] = R, mq - R @ mp
            T = upd @ T
        prev = (fit, rmse)
        p, q, m, n, fit, rmse = one_pass(T)
        if abs(prev[0] - fit) < rel and abs(prev[1] - rmse) < rel:
            break
    return T, fit, rmse, it


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    assert torch.cuda.is_available(), "ttce_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    box = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "host": platform.node()}
    print(json.dumps({"box": box, "reps": reps, "points_per_sweep": N, "radius": RADIUS}), flush=True)
    frames = [O.sweep(N, 100 + k, (0.4 * k, 0.1 * k), 0.4 * k, rings=32) for k in range(10)]
    seq_pairs = [(i, i + s) for s in (3, 4) for i in range(10 - s)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    pts = torch.from_numpy(np.concatenate(frames)).to(dev)
    one_pts = torch.from_numpy(np.concatenate([frames[0], frames[3]])).to(dev)
    one_off = [0, N, 2 * N]
    eye = torch.eye(4, dtype=torch.float64, device=dev)[None]

    # results first: the three routes on the one pair
    T, fit, rmse, iters = ops.icp_point_to_point(one_pts, one_off, [[0, 1]], RADIUS)
    t0 = time.perf_counter()
    cpu = O.icp(frames[0], frames[3], RADIUS)
    cpu_s = time.perf_counter() - t0
    Tp, fitp, rmsep, itp = parent_route(one_pts[:N], one_pts[N:], RADIUS)
    print(json.dumps({"one_pair_results": {
        "hip": {"iterations": int(iters[0]), "fitness": float(fit[0]), "rmse": float(rmse[0]),
                "t": [round(v, 6) for v in T[0, :3, 3].tolist()]},
        "cpu": {"iterations": cpu.iterations, "fitness": cpu.fitness, "rmse": cpu.inlier_rmse,
                "margins_tie_radius_sratio": [float(v) for v in cpu.margins()]},
        "parent": {"iterations": itp, "fitness": fitp, "rmse": rmsep},
        "max_abs_T_hip_minus_cpu": float(np.abs(T[0].cpu().numpy() - cpu.T).max()),
        "max_abs_T_parent_minus_cpu": float(np.abs(Tp.cpu().numpy() - cpu.T).max())}}), flush=True)
    Ts, _, _, its = ops.icp_point_to_point(pts, off, seq_pairs, RADIUS)
    print(json.dumps({"sequence_iterations": its.tolist(),
                      "launches_per_call_30_iterations": {"grids": 4, "loop": 1 + 2 * 31}}), flush=True)

    for ratio in (ops.NN_CELL_RATIO, 0.125, 0.25, 0.5, 1.0, 2.0):
        out = {"cell_over_radius": ratio, "default": ratio == ops.NN_CELL_RATIO}
        g1 = ops.nn_grid(one_pts, one_off, RADIUS, cell_ratio=ratio)
        gs = ops.nn_grid(pts, off, RADIUS, cell_ratio=ratio)
        out["grid_build_2_clouds"] = timed(lambda: ops.nn_grid(one_pts, one_off, RADIUS, cell_ratio=ratio), reps)
        out["grid_build_10_clouds"] = timed(lambda: ops.nn_grid(pts, off, RADIUS, cell_ratio=ratio), reps)
        out["one_pass_identity"] = timed(lambda: ops.nn_radius(one_pts, one_off, [[0, 1]], eye, RADIUS, grid=g1), reps)
        out["one_pass_final_T"] = timed(lambda: ops.nn_radius(one_pts, one_off, [[0, 1]], T, RADIUS, grid=g1), reps)
        out["icp_one_pair_given_grid"] = timed(lambda: ops.icp_point_to_point(one_pts, one_off, [[0, 1]], RADIUS, grid=g1),
                                               reps)
        out["icp_13_pairs_given_grid"] = timed(lambda: ops.icp_point_to_point(pts, off, seq_pairs, RADIUS, grid=gs), reps)
        print(json.dumps(out), flush=True)

    out = {"icp_one_pair_with_grid_build": timed(lambda: ops.icp_point_to_point(one_pts, one_off, [[0, 1]], RADIUS), reps),
           "icp_13_pairs_with_grid_build": timed(lambda: ops.icp_point_to_point(pts, off, seq_pairs, RADIUS), reps),
           "parent_route_one_pair": timed(lambda: parent_route(one_pts[:N], one_pts[N:], RADIUS), max(3, reps // 3), warm=1),
           "cpu_route_one_pair_s": round(cpu_s, 3)}
    a, b = out["icp_one_pair_with_grid_build"]["median_ms"], out["icp_13_pairs_with_grid_build"]["median_ms"]
    out["parent_over_hip_one_pair"] = round(out["parent_route_one_pair"]["median_ms"] / a, 2)
    out["cpu_over_hip_one_pair"] = round(cpu_s * 1e3 / a, 2)
    out["cpu_13_pairs_extrapolated_over_hip"] = round(13 * cpu_s * 1e3 / b, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
