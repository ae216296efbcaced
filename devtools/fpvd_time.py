"""FPVD extractor timing, one process, JSON lines (profiles/fpvd.txt).  `n` synthetic nuScenes-sized sweeps
(testing.synth_points, `points` each, the generator of devtools/fsvd_time.py) through the SPVCNN of the shipped
configuration (cr 0.5, layer_num 32 32 64 128 256 256 128 96 96), seeded weights:
  * metric_utils.compute_point_voxel_logits('32', clouds) whole: host quantization, collate, maps, network, sector means;
  * the network forward alone on the collated batch, next to the MinkUNet forward (the FSVD extractor) on the same voxels;
  * the seven point <-> voxel exchanges alone, replayed on the recorded operands (ops_spvoxel.devoxelize / voxelize), and
    each of them on its own;
  * the same seven passes in torch ops on the same device, in the same process, over the SAME maps and operands:
    devoxelize as the sum over the 8 neighbours of index_select(F, idx_k) * w_k (+ addend), voxelize as index_add_ of
    F / count into zeros.  The clamped indices, the per-point counts and idx0 are built outside the timed region;
  * the three point transforms alone (the dense form of ops_spconv.sparse_conv);
  * the three query passes with their point orders (ops_spvoxel.query + voxel_order);
  * the agreement of the two routes (relative L2 per exchange, worst), so the times compare equal work.
Device events around back-to-back passes after warm-up (`reps` of them, more for a short pass: a window lasts 20 ms at
least), `rounds` times, alternating; median (min ... max).
python devtools/fpvd_time.py [out_path n points reps rounds]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidarcrafter_amd import ops_spconv as KS  # noqa: E402
from lidarcrafter_amd import ops_spvoxel as KV  # noqa: E402
from lidarcrafter_amd.testing import synth_points  # noqa: E402
from lidargen.metrics import DATASET_CONFIG, metric_utils as MU  # noqa: E402
from lidargen.metrics.models.minkowskinet.model import Model as MinkUNet  # noqa: E402
from lidargen.metrics.models.spvcnn.model import Model  # noqa: E402

CONFIG = {"model_params": dict(cr=0.5, layer_num=[32, 32, 64, 128, 256, 256, 128, 96, 96], voxel_size=0.05, num_class=20,
                               input_dims=4)}


def seeded_model(cls, dev):
    m = cls(CONFIG)
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
        elif k.endswith(".weight") and k.startswith("point_transforms"):
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / v.shape[1]) ** 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.2
    m.load_state_dict(sd)
    return m.eval().to(dev)


WINDOW_MS = 20.0                     # a timed window is at least this long: the short passes are repeated more often


def per_pass_ms(fn, reps):
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
    args = sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "fpvd.txt")
    n, points, reps, rounds = (int(v) for v in (args[1:5] + ["25", "30000", "3", "5"][len(args[1:5]):]))
    assert torch.cuda.is_available(), "fpvd_time.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    emit({"box": {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
          "clouds": n, "points_per_cloud": points, "reps": reps, "rounds": rounds, "config": CONFIG["model_params"]})
    model, mink = seeded_model(Model, dev), seeded_model(MinkUNet, dev)
    clouds = [synth_points(points, 100 + i)[:, :3] for i in range(n)]
    cfg = DATASET_CONFIG["nuscenes"]
    t0 = time.perf_counter()
    batch = [MU.pcd2voxel(MU.preprocess_pcd(p, **cfg)) for p in clouds]
    host_ms = (time.perf_counter() - t0) * 1e3
    feats, coords, offsets = MU.sparse_collate(batch, dev)
    emit({"points": int(coords.shape[0]), "host_quantize_ms": round(host_ms, 1)})

    # one forward with every exchange's, transform's and query's operands recorded
    devox, vox, dense, queries = [], [], [], []
    real = dict(devoxelize=KV.devoxelize, voxelize=KV.voxelize, query=KV.query, sparse_conv=KS.sparse_conv)

    def rec_devox(f, idx, w, addend=None, out=None):
        keep = None if addend is None else addend.clone()
        y = real["devoxelize"](f, idx, w, addend=addend, out=out)
        devox.append((f, idx, w, keep, y))
        return y

    def rec_vox(f, perm, offs, out=None):
        y = real["voxelize"](f, perm, offs, out=out)
        vox.append((f, perm, offs, y))
        return y

    def rec_query(pts, stride, table, n_table, weights=True):
        queries.append((pts, stride, table, n_table))
        return real["query"](pts, stride, table, n_table, weights=weights)

    def rec_conv(x, nbr, w, b=None, residual=None, relu=False, out=None, out_col=0):
        y = real["sparse_conv"](x, nbr, w, b, residual=residual, relu=relu, out=out, out_col=out_col)
        if nbr is None and residual is None and relu and x.shape[0] == coords.shape[0]:
            dense.append((x, w, b, y))
        return y

    KV.devoxelize, KV.voxelize, KV.query, KS.sparse_conv = rec_devox, rec_vox, rec_query, rec_conv
    try:
        model(feats, coords)
    finally:
        KV.devoxelize, KV.voxelize, KV.query, KS.sparse_conv = (real[k] for k in ("devoxelize", "voxelize", "query",
                                                                                    "sparse_conv"))
    torch.cuda.synchronize()
    vox = [v for v in vox if v[0].shape[1] != 4]                     # initial_voxelize's scatter of the inputs is not an exchange
    assert len(devox) == 4 and len(vox) == 3 and len(dense) == 3 and len(queries) == 3
    emit({"exchanges": [{"kind": "voxel_to_point", "C": d[0].shape[1], "voxels": d[0].shape[0], "addend": d[3] is not None}
                        for d in devox] + [{"kind": "point_to_voxel", "C": v[0].shape[1], "voxels": v[3].shape[0],
                                            "largest_voxel": int((v[2][1:] - v[2][:-1]).max())} for v in vox]})

    # the torch-ops route: its index tensors, built once
    t_devox = [(d[1].clamp_min(0).long(), d[2]) for d in devox]
    t_vox = []
    for f, perm, offs, y in vox:
        cnt = (offs[1:] - offs[:-1]).float()
        idx0 = torch.empty(perm.shape[0], dtype=torch.long, device=dev)
        idx0[perm.long()] = torch.repeat_interleave(torch.arange(cnt.shape[0], device=dev), (offs[1:] - offs[:-1]).long())
        t_vox.append((idx0, cnt[idx0][:, None]))

    def hip_devox(i):
        f, idx, w, add, y = devox[i]
        return real["devoxelize"](f, idx, w, addend=add, out=None)

    def hip_vox(i):
        f, perm, offs, y = vox[i]
        return real["voxelize"](f, perm, offs, out=y)

    def torch_devox(i):
        f, _, _, add, _ = devox[i]
        idx, w = t_devox[i]
        out = f.index_select(0, idx[:, 0]) * w[:, 0:1]
        for k in range(1, 8):
            out += f.index_select(0, idx[:, k]) * w[:, k:k + 1]
        return out if add is None else out + add

    def torch_vox(i):
        f, _, _, y = vox[i]
        idx0, cnt = t_vox[i]
        return torch.zeros_like(y).index_add_(0, idx0, f / cnt)

    worst = 0.0
    for i in range(4):
        want, got = torch_devox(i).double(), hip_devox(i).double()
        worst = max(worst, float((got - want).norm() / want.norm().clamp_min(1e-30)))
    for i in range(3):
        want, got = torch_vox(i).double(), hip_vox(i).double()
        worst = max(worst, float((got - want).norm() / want.norm().clamp_min(1e-30)))
    emit({"hip_vs_torch_ops_rel_l2_worst_exchange": worst})

    def hip_queries():
        for pts, stride, table, n_table in queries:
            idx, _ = real["query"](pts, stride, table, n_table)
            KV.voxel_order(idx[:, 0].contiguous(), n_table)

    def hip_dense():
        for x, w, b, y in dense:
            real["sparse_conv"](x, None, w, b, relu=True, out=y)

    with torch.no_grad():
        fns = {"spvcnn_forward": lambda: model(feats, coords), "minkunet_forward": lambda: mink(feats, coords),
               "hip_exchanges": lambda: [hip_devox(i) for i in range(4)] + [hip_vox(i) for i in range(3)],
               "torch_ops_exchanges": lambda: [torch_devox(i) for i in range(4)] + [torch_vox(i) for i in range(3)],
               "point_transforms": hip_dense, "queries_and_orders": hip_queries}
        for i in range(4):
            fns[f"hip_devox_{i}"] = lambda i=i: hip_devox(i)
            fns[f"torch_devox_{i}"] = lambda i=i: torch_devox(i)
        for i in range(3):
            fns[f"hip_vox_{i}"] = lambda i=i: hip_vox(i)
            fns[f"torch_vox_{i}"] = lambda i=i: torch_vox(i)
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        n_reps = {k: max(reps, min(2000, int(WINDOW_MS / max(per_pass_ms(fn, reps), 1e-3)) + 1)) for k, fn in fns.items()}
        ts = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                ts[k].append(per_pass_ms(fn, n_reps[k]))
        whole = []
        for _ in range(max(2, rounds // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            MU.compute_point_voxel_logits("32", clouds, model=model)
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
    out = {k: dict(stats(v), reps=n_reps[k]) for k, v in ts.items()}
    out["compute_point_voxel_logits_wall"] = stats(whole)
    out["torch_ops_over_hip_exchanges"] = round(out["torch_ops_exchanges"]["median_ms"] / out["hip_exchanges"]["median_ms"], 2)
    out["spvcnn_over_minkunet_forward"] = round(out["spvcnn_forward"]["median_ms"] / out["minkunet_forward"]["median_ms"], 2)
    emit(out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
