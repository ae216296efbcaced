"""FSVD extractor timing, one process, JSON lines (profiles/fsvd.txt).  `n` synthetic nuScenes-sized sweeps
(testing.synth_points, `points` each) through the MinkUNet of the shipped configuration (cr 0.5, layer_num 32 32 64 128 256
256 128 96 96), seeded weights:
  * metric_utils.compute_logits('32', 'voxel', clouds) whole: host quantization, collate, maps, network, sector means;
  * the network forward alone on the collated batch (coordinate levels, hashes, maps and the 49 convolutions);
  * the 49 convolution launches alone, replayed on the recorded operands (ops_spconv.sparse_conv);
  * torchsparse 1.4.0's algorithm written in torch ops on the same device, in the same process, over the SAME maps and
    folded weights and the same operands: per offset index_select of the input rows, mm, index_add_ into the output,
    then bias, residual and ReLU.  Its (input row, output row) lists per offset are built outside the timed region, as
    torchsparse builds its kernel map once; the channel concatenations cost it nothing here (it reads the recorded operands);
  * the agreement of the two (relative L2 per layer, worst), so the times compare equal work.
Device events around `reps` back-to-back passes after warm-up, `rounds` times, alternating; median (min ... max).
python devtools/fsvd_time.py [out_path n points reps rounds]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidarcrafter_amd import ops_spconv as KS  # noqa: E402
from lidarcrafter_amd.testing import synth_points  # noqa: E402
from lidargen.metrics import DATASET_CONFIG, metric_utils as MU  # noqa: E402
from lidargen.metrics.models.minkowskinet.model import Model  # noqa: E402

CONFIG = {"model_params": dict(cr=0.5, layer_num=[32, 32, 64, 128, 256, 256, 128, 96, 96], voxel_size=0.05, num_class=20,
                               input_dims=4)}


def seeded_model(dev):
    m = Model(CONFIG)
    g = torch.Generator().manual_seed(1)
    sd = {}
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith(".kernel"):
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (v.shape[-2] * (v.shape[0] if v.dim() == 3 else 1))) ** 0.5
        elif k.endswith(".weight") and v.dim() == 1:
            sd[k] = 0.7 + 0.6 * torch.rand(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.2
    m.load_state_dict(sd)
    return m.eval().to(dev)


def per_pass_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}


def main():
    args = sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "fsvd.txt")
    n, points, reps, rounds = (int(v) for v in (args[1:5] + ["50", "30000", "3", "5"][len(args[1:5]):]))
    assert torch.cuda.is_available(), "fsvd_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    emit({"box": {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
          "clouds": n, "points_per_cloud": points, "reps": reps, "rounds": rounds, "config": CONFIG["model_params"]})
    model = seeded_model(dev)
    clouds = [synth_points(points, 100 + i)[:, :3] for i in range(n)]
    cfg = DATASET_CONFIG["nuscenes"]
    t0 = time.perf_counter()
    batch = [MU.pcd2voxel(MU.preprocess_pcd(p, **cfg)) for p in clouds]
    host_ms = (time.perf_counter() - t0) * 1e3
    feats, coords, offsets = MU.sparse_collate(batch, dev)
    emit({"voxels": int(coords.shape[0]), "host_quantize_ms": round(host_ms, 1)})

    # one forward with every convolution's operands recorded
    calls, real = [], KS.sparse_conv

    def recording(x, nbr, w, b=None, residual=None, relu=False, out=None, out_col=0):
        y = real(x, nbr, w, b, residual=residual, relu=relu, out=out, out_col=out_col)
        calls.append((x, nbr, w, b, residual, relu, y, out_col))
        return y

    KS.sparse_conv = recording
    try:
        model(feats, coords)
    finally:
        KS.sparse_conv = real
    torch.cuda.synchronize()
    emit({"conv_launches": len(calls), "rows_per_level": sorted({c[6].shape[0] for c in calls}, reverse=True),
          "gathered_flop": int(sum(2 * (int((c[1] >= 0).sum()) if c[1] is not None else c[0].shape[0]) * c[2].shape[1]
                                   * c[2].shape[2] for c in calls))})

    # torchsparse 1.4.0's convolution in torch ops: the per-offset row lists (its kernel map), built once
    lists = []
    for x, nbr, w, b, res, relu, y, col in calls:
        if nbr is None:
            lists.append(None)
            continue
        per = []
        for k in range(nbr.shape[1]):
            o = (nbr[:, k] >= 0).nonzero(as_tuple=True)[0]
            per.append((nbr[o, k].long(), o) if o.numel() else None)
        lists.append(per)

    def torch_conv(i):
        x, nbr, w, b, res, relu, y, col = calls[i]
        if nbr is None:
            out = x @ w[0]
        else:
            out = torch.zeros((nbr.shape[0], w.shape[2]), device=dev)
            for k, io in enumerate(lists[i]):
                if io is not None:
                    out.index_add_(0, io[1], x.index_select(0, io[0]) @ w[k])
        if b is not None:
            out = out + b
        if res is not None:
            out = out + res
        return torch.relu(out) if relu else out

    def hip_convs():
        for x, nbr, w, b, res, relu, y, col in calls:
            real(x, nbr, w, b, residual=res, relu=relu, out=y, out_col=col)

    def torch_convs():
        for i in range(len(calls)):
            torch_conv(i)

    worst = 0.0
    for i, c in enumerate(calls):
        want = torch_conv(i).double()
        got = c[6][:, c[7]:c[7] + c[2].shape[2]].double()
        worst = max(worst, float((got - want).norm() / want.norm().clamp_min(1e-30)))
    emit({"hip_vs_torch_ops_rel_l2_worst_layer": worst})

    with torch.no_grad():
        fns = {"hip_forward": lambda: model(feats, coords), "hip_convs": hip_convs, "torch_ops_convs": torch_convs}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                ts[k].append(per_pass_ms(fn, reps))
        whole = []
        for _ in range(max(2, rounds // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            MU.compute_logits("32", "voxel", clouds, model=model)
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
    out = {k: stats(v) for k, v in ts.items()}
    out["compute_logits_wall"] = stats(whole)
    out["torch_ops_over_hip_convs"] = round(out["torch_ops_convs"]["median_ms"] / out["hip_convs"]["median_ms"], 2)
    emit(out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
