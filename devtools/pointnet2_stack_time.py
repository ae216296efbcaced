"""lidargen.ops.pointnet2.pointnet2_stack timing and errors, JSON lines (profiles/pointnet2_stack.txt).

Without --worker this starts ONE fresh child process under `timeout` (the measurement runs in that one process, on the
same operands for every route) and passes its exit status on.  The worker:
  * errors: StackSAModuleMSG (fused eval route), StackPointnetFPModule and NeighborVoxelSAModuleMSG against the float64
    CPU restatement over the float32 torch module's own error, on the inputs of tests/test_pointnet2_stack.py;
  * timings at 2 clouds x 16 384 points (uniform in 33 x 33 x 2, about 7.5 points per unit volume), 2 x 2 048 centres (a
    seeded subset of the points), 16 feature channels: the PV-RCNN scale radii [0.4, 0.8], nsamples [16, 16],
    mlps [[16, 16], [16, 16]], and one wide scale radius 0.8, nsample 16, mlp [64, 64, 128]:
      ball_query      the ball query alone (radius 0.8, nsample 16)
      fused           StackSAModuleMSG eval forward under no_grad: ball query, gathered first layer, dense layers, maximum
      operator        the same module with LC_PN2_FUSED=0: this package's operators + torch layers
      plain_torch     the same formulation in torch ops only: cdist, the nsample smallest hit indices by topk, gather,
                      the module's own Conv2d / BatchNorm2d / ReLU, max
    device events around `reps` back-to-back calls, so PER-CALL times with their launch gaps and allocations; `rounds` rounds
    after a warm-up, the routes alternating inside every round; median (min ... max).
python devtools/pointnet2_stack_time.py [out_path reps rounds]"""
import json
import os
import platform
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420


def per_call_ms(fn, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def plain_torch_sa(module, xyz, counts, new_xyz, new_counts, feats):
    """StackSAModuleMSG's formulation in torch ops only; counts are HOST lists."""
    import torch

    outs = []
    for k, g in enumerate(module.groupers):
        cols = []
        ps = cs = 0
        for n, m in zip(counts, new_counts):
            p, c, f = xyz[ps:ps + n], new_xyz[cs:cs + m], feats[ps:ps + n]
            hit = torch.cdist(c, p) < g.radius                                       # [m, n]
            key = torch.where(hit, torch.arange(n, device=p.device)[None, :], torch.full((1, 1), n, device=p.device))
            key = torch.cat([key, torch.full((m, g.nsample), n, device=p.device)], dim=1)    # (clouds below nsample points)
            idx = torch.topk(key, g.nsample, dim=1, largest=False, sorted=True)[0]   # the first nsample hits, ascending
            empty = idx[:, 0] == n
            idx = torch.where(idx == n, idx[:, :1], idx)
            idx = torch.where(empty[:, None], torch.zeros_like(idx), idx)
            flat = idx.reshape(-1)
            gx = p.index_select(0, flat).view(m, g.nsample, 3) - c[:, None, :]
            gf = f.index_select(0, flat).view(m, g.nsample, -1)
            x = torch.cat([gx, gf], dim=2) * (~empty)[:, None, None]
            cols.append(x)
            ps, cs = ps + n, cs + m
        x = torch.cat(cols, dim=0).permute(2, 0, 1).unsqueeze(0)                     # [1, C + 3, M, nsample]
        outs.append(module.mlps[k](x).max(dim=3)[0].squeeze(0).permute(1, 0))
    return torch.cat(outs, dim=1)


def worker(out_path, reps, rounds):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _pointnet2_stack_cases as TS
    from lidarcrafter_amd import ops_pointnet2 as KP
    from lidargen.ops.pointnet2.pointnet2_stack import pointnet2_modules as PM

    assert torch.cuda.is_available(), "the timing needs the GPU; nothing is measured without it"
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    emit({"device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
          "torch": torch.__version__, "reps": reps, "rounds": rounds})

    # ---- errors on the tests' inputs ---------------------------------------------------------------------------------
    O = TS.O
    module, inputs = TS.sa_module().to(dev).eval(), TS.sa_inputs("base")
    with torch.no_grad():
        fused = module(*TS.sa_dev_args(inputs, dev))[1].cpu().numpy()
        ref = TS.sa_cpu(module, inputs, torch.float64)[1].numpy()
        f32 = TS.sa_cpu(module, inputs, torch.float32)[1].numpy()
    e_hip, e_torch = float(O.rel_l2_rows(fused, ref).max()), float(O.rel_l2_rows(f32, ref).max())
    emit({"StackSAModuleMSG_eval_max_row_rel_l2_vs_float64": {"fused_hip": e_hip, "float32_torch_cpu": e_torch,
                                                               "ratio": round(e_hip / e_torch, 3)}})
    for name, fn in (("StackPointnetFPModule", TS.fp_module_errors), ("NeighborVoxelSAModuleMSG", TS.neighbor_voxel_module_errors)):
        _, e_hip, e_torch = fn(dev)
        emit({name + "_max_row_rel_l2_vs_float64": {"hip_route": e_hip, "float32_torch_cpu": e_torch,
                                                    "ratio": round(e_hip / e_torch, 3)}})

    # ---- timings -----------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(0)
    counts, new_counts, C = [16384, 16384], [2048, 2048], 16
    pts = (rng.random((sum(counts), 3)) * np.array([33.0, 33.0, 2.0])).astype(np.float32)
    pick = np.concatenate([np.sort(rng.choice(16384, 2048, replace=False)) + 16384 * b for b in range(2)])
    xyz, new_xyz = torch.from_numpy(pts).to(dev), torch.from_numpy(pts[pick]).to(dev)
    feats = torch.from_numpy(rng.standard_normal((sum(counts), C)).astype(np.float32)).to(dev)
    xc, nc = TS.I(counts, dev), TS.I(new_counts, dev)
    sizes = (torch.cdist(new_xyz[:2048], xyz[:16384]) < 0.8).sum(dim=1).float()
    emit({"clouds": counts, "centres": new_counts, "channels": C, "points_in_ball_r0.8": {
        "mean": round(float(sizes.mean()), 2), "min": int(sizes.min()), "max": int(sizes.max())}})

    torch.manual_seed(0)
    setups = {"pvrcnn_2x[16,16]": PM.StackSAModuleMSG(radii=[0.4, 0.8], nsamples=[16, 16], mlps=[[C, 16, 16], [C, 16, 16]]),
              "wide_[64,64,128]": PM.StackSAModuleMSG(radii=[0.8], nsamples=[16], mlps=[[C, 64, 64, 128]])}
    for name, module in setups.items():
        module = TS.randomise(module, 1).to(dev).eval()

        def fused():
            os.environ["LC_PN2_FUSED"] = "1"
            return module(xyz, xc, new_xyz, nc, feats)[1]

        def operator():
            os.environ["LC_PN2_FUSED"] = "0"
            return module(xyz, xc, new_xyz, nc, feats)[1]

        def plain():
            return plain_torch_sa(module, xyz, counts, new_xyz, new_counts, feats)

        def query():
            return KP.ball_query(0.8, 16, xyz, xc, new_xyz, nc)

        fns = {"ball_query": query, "fused": fused, "operator": operator, "plain_torch": plain}
        times = {k: [] for k in fns}
        with torch.no_grad():
            outs = {k: fn() for k, fn in fns.items()}                                # warm-up, and the results compared
            for _ in range(2):
                for fn in fns.values():
                    fn()
            for _ in range(rounds):
                for k, fn in fns.items():
                    times[k].append(per_call_ms(fn, reps))
        os.environ.pop("LC_PN2_FUSED", None)

        def rel(a, b):
            return float((a - b).norm() / b.norm())

        med = {k: statistics.median(v) for k, v in times.items()}
        emit({"setup": name, **{k: stats(v) for k, v in times.items()},
              "operator_over_fused": round(med["operator"] / med["fused"], 3),
              "plain_torch_over_fused": round(med["plain_torch"] / med["fused"], 3),
              "rel_l2_fused_vs_operator": rel(outs["fused"], outs["operator"]),
              "rel_l2_fused_vs_plain_torch": rel(outs["fused"], outs["plain_torch"])})

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    args = [a for a in sys.argv[1:] if a != "--worker"]
    out_path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "pointnet2_stack.txt")
    reps = int(args[1]) if len(args) > 1 else 10
    rounds = int(args[2]) if len(args) > 2 else 7
    if "--worker" in sys.argv:
        worker(out_path, reps, rounds)
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker", out_path, str(reps),
           str(rounds)]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
