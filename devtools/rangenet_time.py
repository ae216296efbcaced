"""RangeNet-53 timing, one process, JSON lines (profiles/rangenet.txt).  Seeded weights (testing.seeded_fill_rangenet),
seeded range images (testing.rangenet_images); per shape [B, C, H, W]:
  * models.rangenet.Model forward (the plan over csrc/rangenet.hip) per batch;
  * the identical layers in eager torch float32 on the same device and operands: F.conv2d / conv_transpose2d over the
    SAME folded weights and biases, leaky_relu, the same addends;
  * the agreement of the two decoder maps (relative L2), so the times compare equal work;
  * per layer kind (stem, down, 1x1, 3x3, up): device-event time of each launch summed over the kind, counted flops
    (2 x multiply-adds of plan.flops_per_pixel's terms), fraction of the 155 TFLOP/s f32-matrix peak;
  * the split of one metric_utils.compute_range_logits call into host projection (numpy) and network;
  * the parity of the whole-network test cases against the float64 CPU oracle (tests/_rangenet_oracle.py), next to the
    float32 CPU oracle's own error.
Device events around `reps` back-to-back calls after warm-up, repeated `rounds` times, alternating the two
implementations; median (min ... max) of the per-call means.
python devtools/rangenet_time.py [reps rounds]"""
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
import _rangenet_oracle as O  # noqa: E402
from lidarcrafter_amd import ops_rangenet as KR  # noqa: E402
from lidarcrafter_amd.testing import rangenet_images, seeded_fill_rangenet  # noqa: E402
from lidargen.metrics import metric_utils as MU  # noqa: E402
from lidargen.metrics.models.rangenet.model import Model  # noqa: E402
from lidargen.metrics.models.rangenet.plan import flops_per_pixel  # noqa: E402

PEAK_F32_MATRIX = 155e12     # measured v_mfma_f32_32x32x2_f32 rate of the chip, flop/s
KIND = {"stem": "stem 3x3", "down": "down 3x3 s(1,2)", "c1": "block 1x1", "c2": "block 3x3", "up": "up 1x4^T", "head": "head"}


def folded(model):
    out = []
    for L in model.plan().layers:
        bn = None if L.bn is None else (L.bn.weight, L.bn.bias, L.bn.running_mean, L.bn.running_var, L.bn.eps)
        w, b = KR.fold_bn(L.conv.weight, L.conv.bias, bn, L.mode)
        out.append((L, w.cuda(), b.cuda()))
    return out


def eager_forward(layers, x):
    skips, h, blk_in, skip = [], x, None, None
    for L, w, b in layers:
        if L.tag == "down":
            skips.append(h)
        if L.tag == "c1":
            blk_in = h
        if L.mode == 3:
            y = F.conv_transpose2d(h, w, b, stride=(1, 2), padding=(0, 1))
        else:
            y = F.conv2d(h, w, b, stride=(1, 2) if L.mode == 2 else 1, padding=0 if L.mode == 0 else 1)
        y = F.leaky_relu(y, 0.1) if L.act else y
        if L.tag == "c2":
            y = y + blk_in
            if skip is not None:
                y = y + skip
            blk_in = skip = None
        if L.tag == "up":
            skip = skips.pop()
        h = y
    return h


def per_layer(model, x):
    """{kind: (ms, flop)} of one forward: events around every launch."""
    plan = model.plan()
    packed = plan.packed(x.device)
    ev, skips, h, blk_in, skip = [], [], x, None, None
    for L, (wpk, bias, Co) in zip(plan.layers, packed):
        if L.tag == "down":
            skips.append(h)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if L.tag == "c1":
            blk_in, y = h, KR.conv(h, wpk, bias, L.mode, Co, L.act)
        elif L.tag == "c2":
            y = KR.conv(h, wpk, bias, L.mode, Co, L.act, res1=blk_in, res2=skip)
            blk_in = skip = None
        else:
            y = KR.conv(h, wpk, bias, L.mode, Co, L.act)
            if L.tag == "up":
                skip = skips.pop()
        b.record()
        taps = 2 if L.mode == 3 else KR.TAPS[L.mode]
        ev.append((L.tag, a, b, 2.0 * y.numel() * h.shape[1] * taps))
        h = y
    torch.cuda.synchronize()
    out = {}
    for tag, a, b, flop in ev:
        ms, fl, n = out.get(tag, (0.0, 0.0, 0))
        out[tag] = (ms + a.elapsed_time(b), fl + flop, n + 1)
    return out


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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    print(json.dumps({"device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
                      "torch": torch.__version__, "reps": reps, "rounds": rounds}), flush=True)
    with torch.no_grad():
        for B, C, H, W in ((100, 4, 32, 1024), (8, 5, 64, 1024)):
            cfg = O.config(53, remission=(C == 5))
            model = seeded_fill_rangenet(Model(cfg), 1).eval().requires_grad_(False).cuda()
            x5 = rangenet_images(B, H, W, 9).cuda()
            x = x5[:, model.backbone.input_idxs].contiguous()
            layers = folded(model)
            hip = lambda: model(x5)  # noqa: E731
            eager = lambda: eager_forward(layers, x)  # noqa: E731
            a, b = hip(), eager()
            agree = float((a - b).double().norm() / b.double().norm())
            hip(), eager()
            th, te = [], []
            for _ in range(rounds):
                th.append(per_call_ms(hip, reps))
                te.append(per_call_ms(eager, reps))
            flop = 2.0 * flops_per_pixel(53, C) * B * H * W
            mh = statistics.median(th)
            print(json.dumps({"shape": [B, C, H, W], "layers": 53, "hip": stats(th), "eager_torch_f32": stats(te),
                              "hip_over_eager": round(mh / statistics.median(te), 3), "decoder_rel_l2_hip_vs_eager": agree,
                              "gflop": round(flop / 1e9, 1), "hip_tflops": round(flop / mh / 1e9, 1),
                              "frac_of_f32_matrix_peak": round(flop / (mh * 1e-3) / PEAK_F32_MATRIX, 3)}), flush=True)
            per_layer(model, x)
            kinds = per_layer(model, x)
            for tag, (ms, fl, n) in kinds.items():
                print(json.dumps({"shape": [B, C, H, W], "kind": KIND[tag], "launches": n, "ms": round(ms, 3),
                                  "gflop": round(fl / 1e9, 1), "tflops": round(fl / ms / 1e9, 1),
                                  "frac_of_f32_matrix_peak": round(fl / (ms * 1e-3) / PEAK_F32_MATRIX, 3)}), flush=True)
            del model, layers, a, b, x, x5
            torch.cuda.empty_cache()

        # one compute_range_logits call: 100 clouds of 30000 points at nuScenes' 32 x 1024
        model = seeded_fill_rangenet(Model(O.config(53)), 1).eval().requires_grad_(False).cuda()
        clouds = [O.metre_cloud(i, n=30000) for i in range(100)]
        MU.compute_range_logits("32", clouds[:4], model=model)
        from lidargen.metrics import DATASET_CONFIG
        t0 = time.perf_counter()
        imgs = np.stack([MU.preprocess_range(c, **DATASET_CONFIG["nuscenes"]) for c in clouds])
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        MU.compute_range_logits("32", clouds, model=model)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        print(json.dumps({"compute_range_logits": {"clouds": 100, "points": 30000, "whole_call_ms": round((t3 - t2) * 1e3, 1),
                                                   "host_projection_ms": round((t1 - t0) * 1e3, 1),
                                                   "network_and_copies_ms": round((t3 - t2 - (t1 - t0)) * 1e3, 1)},
                          "image_shape": list(imgs.shape)}), flush=True)

        # parity of the whole-network test cases
        for layers_n, B, H, W in ((21, 3, 16, 64), (53, 2, 16, 64), (53, 2, 32, 96)):
            m = seeded_fill_rangenet(Model(O.config(layers_n)), 1).eval().requires_grad_(False)
            xi = rangenet_images(B, H, W, 31)
            sd = m.state_dict()
            enc64, dec64 = O.model_forward(sd, O.config(layers_n), xi, torch.float64)
            enc32, dec32 = O.model_forward(sd, O.config(layers_n), xi, torch.float32)
            m = m.cuda()
            got = m(xi.cuda()).cpu()
            depth = m(xi.cuda(), return_final_logits=True)
            pooled = m(xi.cuda(), return_logits=True)
            print(json.dumps({"parity": f"darknet-{layers_n} {B}x{H}x{W}", "per_sample_rel_l2_vs_float64": {
                "decoder_hip": max(O.rel_l2_per_sample(got, dec64)), "decoder_float32_cpu": max(O.rel_l2_per_sample(dec32, dec64)),
                "depth_hip": max(O.rel_l2_per_sample(depth, O.aggregate(dec64, "depth"))),
                "depth_float32_cpu": max(O.rel_l2_per_sample(O.aggregate(dec32, "depth"), O.aggregate(dec64, "depth"))),
                "return_logits_hip": max(O.rel_l2_per_sample(pooled, enc64.mean([2, 3]))),
                "return_logits_float32_cpu": max(O.rel_l2_per_sample(enc32.mean([2, 3]), enc64.mean([2, 3])))},
                "limit": O.TOL_CONV}), flush=True)


if __name__ == "__main__":
    main()
