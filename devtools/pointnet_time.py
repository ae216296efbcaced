"""PointNet extractor timing, one process, JSON lines (profiles/pointnet.txt).  At B clouds of N points (16 x 32768: one
evaluator batch of 32 x 1024 range images), seeded weights (testing.seeded_fill_pointnet), seeded clouds:
  * extractor.PointNet1 (two fused trunks + the six dense heads) per batch;
  * ops_pointnet.pointnet_trunk alone (one trunk launch pair: the fused kernel and the tile reduction);
  * the identical layers in eager torch on the same device, in the same process, on the same inputs (conv1d /
    batch_norm / relu / amax / linear from the same state dict), whole model and one trunk;
  * the agreement of the two feature matrices (relative L2 per segment), so the times compare equal work;
  * the arithmetic floor: 2 trunks x B x N x 2 (3 x 64 + 64 x 128 + 128 x 1024) flop at the f32-input MFMA peak.
Device events around `reps` back-to-back calls after warm-up, repeated `rounds` times, alternating the two
implementations; median (min ... max) of the per-call means.
python devtools/pointnet_time.py [B N reps rounds]"""
import json
import os
import platform
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidarcrafter_amd import ops_pointnet as KP  # noqa: E402
from lidarcrafter_amd.testing import pointnet_clouds, seeded_fill_pointnet  # noqa: E402
from lidargen.metrics.extractor import PointNet1  # noqa: E402

PEAK_F32_MATRIX = 155e12     # measured v_mfma_f32_32x32x2_f32 rate of the chip, flop/s
TRUNK_FLOP_PER_POINT = 2 * (3 * 64 + 64 * 128 + 128 * 1024)


def eager_trunk(sd, p, x, relu3):
    def bn(h, n):
        return F.batch_norm(h, sd[n + ".running_mean"], sd[n + ".running_var"], sd[n + ".weight"], sd[n + ".bias"], False)
    h = F.relu(bn(F.conv1d(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"]), p + "bn1"))
    h = F.relu(bn(F.conv1d(h, sd[p + "conv2.weight"], sd[p + "conv2.bias"]), p + "bn2"))
    h = bn(F.conv1d(h, sd[p + "conv3.weight"], sd[p + "conv3.bias"]), p + "bn3")
    return (F.relu(h) if relu3 else h).amax(dim=2)


def eager_model(sd, x):
    def bn(h, n):
        return F.batch_norm(h, sd[n + ".running_mean"], sd[n + ".running_var"], sd[n + ".weight"], sd[n + ".bias"], False)

    def fc(h, n):
        return F.linear(h, sd[n + ".weight"], sd[n + ".bias"])
    p = "feat.stn."
    g = eager_trunk(sd, p, x, True)
    g = F.relu(bn(fc(g, p + "fc1"), p + "bn4"))
    g = F.relu(bn(fc(g, p + "fc2"), p + "bn5"))
    trans = fc(g, p + "fc3").view(-1, 3, 3) + torch.eye(3, device=x.device)
    xt = torch.bmm(x.transpose(2, 1), trans).transpose(2, 1)
    x1 = eager_trunk(sd, "feat.", xt, False)
    x2 = F.relu(bn(fc(x1, "fc1"), "bn1"))
    x3 = F.relu(bn(fc(x2, "fc2"), "bn2"))
    return torch.cat((x1, x2, x3, fc(x3, "fc3")), dim=1)


def per_call_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    B, N, reps, rounds = (int(v) for v in (sys.argv[1:5] + ["16", "32768", "10", "7"][len(sys.argv) - 1:]))
    assert torch.cuda.is_available(), "pointnet_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    print(json.dumps({"box": {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
                              "torch": torch.__version__, "host": platform.node()},
                      "B": B, "N": N, "reps": reps, "rounds": rounds}), flush=True)
    m = seeded_fill_pointnet(PointNet1(k=16), 1).eval().to(dev)
    sd = {k: v for k, v in m.state_dict().items()}
    x = pointnet_clouds(B, N, seed=1).to(dev)
    (w1, b1), (w2, b2), (w3, b3) = m.feat.folded()
    scratch = torch.empty(KP.trunk_scratch_elems(B, N), device=dev)
    y = torch.empty((B, 1024), device=dev)
    with torch.no_grad():
        fns = {
            "hip_model": lambda: m(x),
            "eager_model": lambda: eager_model(sd, x),
            "hip_trunk": lambda: KP.pointnet_trunk(x, None, w1, b1, w2, b2, w3, b3, False, out=y, scratch=scratch),
            "eager_trunk": lambda: eager_trunk(sd, "feat.", x, False),
        }
        f_hip, f_eager = m(x).double(), eager_model(sd, x).double()
        agree = {f"{lo}:{hi}": float(((f_hip[:, lo:hi] - f_eager[:, lo:hi]).norm(dim=1) / f_eager[:, lo:hi].norm(dim=1)).max())
                 for lo, hi in ((0, 1024), (1024, 1536), (1536, 1792), (1792, 1808))}
        print(json.dumps({"hip_vs_eager_rel_l2_worst_cloud": agree}), flush=True)
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                ts[k].append(per_call_ms(fn, reps))
    out = {k: stats(v) for k, v in ts.items()}
    trunk_floor = B * N * TRUNK_FLOP_PER_POINT / PEAK_F32_MATRIX * 1e3
    out["trunk_floor_ms"] = round(trunk_floor, 3)
    out["model_floor_ms"] = round(2 * trunk_floor, 3)
    out["hip_trunk_fraction_of_floor"] = round(trunk_floor / out["hip_trunk"]["median_ms"], 3)
    out["hip_model_fraction_of_floor"] = round(2 * trunk_floor / out["hip_model"]["median_ms"], 3)
    out["hip_trunk_tflops"] = round(B * N * TRUNK_FLOP_PER_POINT / out["hip_trunk"]["median_ms"] / 1e9, 1)
    out["eager_over_hip_model"] = round(out["eager_model"]["median_ms"] / out["hip_model"]["median_ms"], 2)
    out["eager_over_hip_trunk"] = round(out["eager_trunk"]["median_ms"] / out["hip_trunk"]["median_ms"], 2)
    out["scratch_mb"] = round(scratch.numel() * 4 / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
