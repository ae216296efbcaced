"""GLENet / RGF timing, one process, JSON lines (profiles/glenet.txt).  A Generator with seeded weights
(testing.seeded_fill_glenet) at the RGF shape: 30 draws x 2048 synthetic objects of 50-2000 points, K = 512, same process
and operands, alternating:
  * the gathered trunk kernel (ops_glenet.glenet_trunk: both trunks and their max, R = 61 440 rows);
  * the identical layers (same folded weights) in eager torch float32 on a materialised [R, 3, 512], in row chunks (the
    512-channel activation of all rows at once would be 64 GB);
  * lc_pointnet_trunk_fwd (3 -> 64 -> 128 -> 1024) on the same materialised points: the ratio to the gathered trunk against
    the flop ratio (192 + 8192 + 65536) / (192 + 8192 + 131072) = 0.53;
  * the score kernel (decode, paired IoU, variance) per pair, against the CPU oracle's polygon loop per pair;
  * the whole compute_rgf_fold (host dataset, index lists, upload, sampler, score, read-back).
Device events around `reps` back-to-back calls after warm-up, repeated `rounds` times, alternating; median (min ... max).
python devtools/glenet_time.py [reps rounds draws objects]"""
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _glenet_oracle as O  # noqa: E402
from lidarcrafter_amd import ops_glenet as KG  # noqa: E402
from lidarcrafter_amd import ops_pointnet as KP  # noqa: E402
from lidarcrafter_amd.testing import seeded_fill_glenet  # noqa: E402
from lidargen.metrics import fg_object  # noqa: E402
from lidargen.metrics.datasets.object_uncertainty_dataset import NuscObjUncertainty  # noqa: E402
from lidargen.metrics.models.glenet import DEFAULT_MODEL_CFG, Generator  # noqa: E402

PEAK_F32_MATRIX = 155e12     # measured v_mfma_f32_32x32x2_f32 rate of the chip, flop/s
FLOP_PER_POINT = 2 * (3 * 64 + 64 * 128 + 128 * 512) + 2 * (3 * 8 + 8 * 8 + 8 * 8)
FLOP_PER_POINT_1024 = 2 * (3 * 64 + 64 * 128 + 128 * 1024)


def synthetic_infos(n_objects, seed):
    r = np.random.default_rng(seed)
    infos = []
    for i in range(n_objects):
        n = int(r.integers(50, 2001))
        size = np.array([3.9, 1.6, 1.56]) * np.exp(r.normal(0, 0.1, 3))
        centre = np.array([r.uniform(-40, 40), r.uniform(-40, 40), r.uniform(-1, 1)])
        p = r.uniform(-0.5, 0.5, (n, 3)) * size + centre
        infos.append({"points": p.astype(np.float32), "name": ("car", "truck", "bus")[i % 3], "num_points_in_gt": n,
                      "box3d_lidar": [*centre, *size, float(r.uniform(-np.pi, np.pi))]})
    text = r.normal(0, 1, (3, 512))
    text = (text / np.linalg.norm(text, axis=1, keepdims=True)).astype(np.float32)
    return infos, dict(zip(("car", "truck", "bus"), text))


def eager_trunks(main, side, x, rows=2048):
    """Both trunks and their max in eager torch float32 on x [R, 3, K], `rows` rows at a time."""
    outs = []
    for r0 in range(0, x.shape[0], rows):
        xs = x[r0:r0 + rows]
        pair = []
        for w in (main, side):
            h = torch.relu(F.conv1d(xs, w[0][:, :, None], w[1]))
            h = torch.relu(F.conv1d(h, w[2][:, :, None], w[3]))
            pair.append(F.conv1d(h, w[4][:, :, None], w[5]).amax(dim=2))
        outs.append(pair)
    return torch.cat([p[0] for p in outs]), torch.cat([p[1] for p in outs])


def per_call_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    D = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    n_objects = int(sys.argv[4]) if len(sys.argv) > 4 else 2048
    K = 512
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    print(json.dumps({"device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
                      "torch": torch.__version__, "reps": reps, "rounds": rounds, "draws": D, "objects": n_objects}), flush=True)
    dev = torch.device("cuda:0")
    infos, text = synthetic_infos(n_objects, 1)
    with torch.no_grad():
        net = seeded_fill_glenet(Generator(DEFAULT_MODEL_CFG, 3, 1), 7).eval().requires_grad_(False).to(dev)
        f = net.folded()
        main_w, side_w = f["main"], f["side"]
        ds = NuscObjUncertainty(infos, text, generator=np.random.default_rng(2))
        batch = next(ds.batches(n_objects))
        B = len(batch["key"])
        R = D * B
        points, offsets = torch.from_numpy(batch["points"]).to(dev), torch.from_numpy(batch["offsets"]).to(dev)
        choice = torch.from_numpy(ds.choice(np.diff(batch["offsets"]), D, K)).to(dev)
        norm, _ = KG.segment_center(points, offsets)
        rows = (offsets[:-1].long()[None, :, None] + choice.long()).reshape(R, K)
        x = norm[rows].permute(0, 2, 1).contiguous()                                   # [R, 3, K] materialised
        w3 = torch.zeros((1024, 128), device=dev)
        w3[:512] = main_w[4]
        b3 = torch.zeros(1024, device=dev)
        b3[:512] = main_w[5]
        out = (torch.empty((512, R), device=dev), torch.empty((8, R), device=dev))
        pn_out = torch.empty((R, 1024), device=dev)
        pn_scratch = torch.empty(KP.trunk_scratch_elems(R, K), device=dev)
        fns = {
            "segment_center": lambda: KG.segment_center(points, offsets),
            "trunk_gathered": lambda: KG.glenet_trunk(norm, offsets, choice, main_w, side_w, out=out),
            "eager_torch_f32": lambda: eager_trunks(main_w, side_w, x),
            "pointnet_trunk_1024": lambda: KP.pointnet_trunk(x, None, *main_w[:4], w3, b3, False, out=pn_out, scratch=pn_scratch),
        }
        fa, fs = fns["trunk_gathered"]()
        ea, es = fns["eager_torch_f32"]()
        agree = (float((fa.t() - ea).double().norm() / ea.double().norm()), float((fs.t() - es).double().norm() / es.double().norm()))
        same_bits = bool(torch.equal(fns["pointnet_trunk_1024"]()[:, :512].t(), fa))
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(per_call_ms(fn, reps))
        mt, mp = statistics.median(times["trunk_gathered"]), statistics.median(times["pointnet_trunk_1024"])
        ratios = [a / b for a, b in zip(times["trunk_gathered"], times["pointnet_trunk_1024"])]
        flop = float(FLOP_PER_POINT) * R * K
        print(json.dumps({"rows": R, "K": K, "total_points": int(points.shape[0]), **{k: stats(v) for k, v in times.items()},
                          "trunk_over_eager": round(mt / statistics.median(times["eager_torch_f32"]), 4),
                          "rel_l2_hip_vs_eager_main_side": agree, "featA_bits_equal_pointnet_trunk": same_bits,
                          "trunk_tflops": round(flop / mt / 1e9, 1),
                          "trunk_frac_of_f32_matrix_peak": round(flop / (mt * 1e-3) / PEAK_F32_MATRIX, 3),
                          "pointnet_trunk_tflops": round(float(FLOP_PER_POINT_1024) * R * K / mp / 1e9, 1),
                          "trunk_over_pointnet_trunk": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                                                        "max": round(max(ratios), 4)},
                          "flop_ratio": round((192 + 8192 + 65536) / (192 + 8192 + 131072), 4)}), flush=True)
        del x, pn_out, pn_scratch, ea, es
        torch.cuda.empty_cache()

        # the whole sampler and the score kernel
        eps = torch.randn((D, B, 8), generator=torch.Generator().manual_seed(0)).to(dev)
        text_feat, gt = torch.from_numpy(batch["text_feat"]).to(dev), torch.from_numpy(batch["gt_boxes"]).to(dev)
        box = net.sample_boxes(points, offsets, text_feat, choice, eps)
        t_sample = [per_call_ms(lambda: net.sample_boxes(points, offsets, text_feat, choice, eps), 1) for _ in range(rounds)]
        KG.glenet_score(box, gt)
        t_score = [per_call_ms(lambda: KG.glenet_score(box, gt), max(reps, 10)) for _ in range(rounds)]
        pred, _, _, _ = KG.glenet_score(box, gt)
        n_cpu = 500
        gdec = KG.glenet_score(torch.cat([gt, torch.zeros((B, 2), device=dev)], 1)[None].contiguous(), gt)[0][0]
        g5 = gdec[:n_cpu, [0, 1, 3, 4, 6]].cpu().numpy()
        q5 = pred[0, :n_cpu][:, [0, 1, 3, 4, 6]].cpu().numpy()
        cg, cq = O.rbbox_to_corners(g5).numpy(), O.rbbox_to_corners(q5).numpy()
        t0 = time.perf_counter()
        O.rinter(cg, cq)
        cpu_us = (time.perf_counter() - t0) / n_cpu * 1e6
        ms = statistics.median(t_score)
        print(json.dumps({"sample_boxes": stats(t_sample), "sample_boxes_rows": R, "glenet_score": stats(t_score), "pairs": R,
                          "score_ns_per_pair": round(ms * 1e6 / R, 2), "cpu_oracle_us_per_pair": round(cpu_us, 1),
                          "cpu_oracle_pairs_timed": n_cpu}), flush=True)

        # the whole fold, host side included (wall clock around a synchronise)
        walls = []
        for _ in range(max(2, rounds // 2)):
            fold = NuscObjUncertainty(infos, text, generator=np.random.default_rng(2))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fg_object.compute_rgf_fold(fold, net, draws=D, generator=torch.Generator().manual_seed(0))
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"compute_rgf_fold_wall": stats(walls), "objects": len(res), "draws": D,
                          "pairs_per_s": round(len(res) * D / (statistics.median(walls) * 1e-3))}), flush=True)


if __name__ == "__main__":
    main()
