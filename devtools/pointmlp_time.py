"""PointMLP timing, one process, JSON lines (profiles/pointmlp.txt).  pointMLP(4) with seeded weights
(testing.seeded_fill_pointmlp) on 8 clouds of 1024 points (half of them zero-padded objects), alternating:
  * the whole forward (Model.forward: geometry + dense chain);
  * the geometry alone (Model.geometry: four FPS and four kNN launches), and each FPS call alone with its time per pick;
  * the dense chain alone (Model.dense on index tables computed before);
  * the identical layers in eager torch float32 on the same device, fed the SAME index tables and the SAME folded weights
    (gather, torch.std, conv1d as a batched matmul, relu, amax);
  * the agreement of the two feature matrices (relative L2), so the times compare equal work;
  * the counted multiply-adds of the dense chain and the fraction of the 155 TFLOP/s f32-matrix peak;
  * the parity of the three fixture cases (tests/golden/pointmlp.npz) against the float64 oracle, next to the reference
    float32 module's own recorded error.
Device events around `reps` back-to-back calls after warm-up, repeated `rounds` times, alternating; median (min ... max).
python devtools/pointmlp_time.py [reps rounds]"""
import json
import os
import platform
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pointmlp_oracle as O  # noqa: E402
from test_pointmlp_host import CASES, make, oracle64  # noqa: E402
from lidarcrafter_amd import ops_pointmlp as KM  # noqa: E402
from lidarcrafter_amd.testing import seeded_fill_pointmlp  # noqa: E402
from lidargen.metrics.extractor.pointmlp import pointMLP  # noqa: E402

PEAK_F32_MATRIX = 155e12     # measured v_mfma_f32_32x32x2_f32 rate of the chip, flop/s


def eager_dense(model, x, tables, return_features=True):
    """Model.dense in eager torch float32 over the same folded weights and index tables."""
    ws = iter([(w.to(x.device), b.to(x.device)) for w, b in model.folded()])

    def layer(t, act, res=None):
        w, b = next(ws)
        y = torch.matmul(w, t) + b[None, :, None]
        if res is not None:
            y = y + res
        return torch.relu(y) if act else y

    def block(t):
        return layer(layer(t, True), True, res=t)

    feat = layer(x, True)
    for i, (f, k) in enumerate(tables):
        B, d, _ = feat.shape
        S, K = k.shape[1], k.shape[2]
        g = model.local_grouper_list[i]
        anchor = torch.gather(feat, 2, f.long()[:, None, :].expand(B, d, S))
        nb = torch.gather(feat, 2, k.long().reshape(B, 1, S * K).expand(B, d, S * K)).reshape(B, d, S, K)
        diff = nb - anchor[..., None]
        std = diff.reshape(B, -1).std(dim=1).reshape(B, 1, 1, 1)
        norm = g.affine_alpha.reshape(1, d, 1, 1) * (diff / (std + 1e-5)) + g.affine_beta.reshape(1, d, 1, 1)
        t = layer(torch.cat([norm, anchor[..., None].expand(B, d, S, K)], 1).reshape(B, 2 * d, S * K), True)
        for _ in model.pre_blocks_list[i].operation:
            t = block(t)
        feat = t.reshape(B, t.shape[1], S, K).amax(3)
        for _ in model.pos_blocks_list[i].operation:
            feat = block(feat)
    f = feat.amax(2)
    if return_features:
        return f
    h = layer(layer(f.t()[None], True), True)
    return layer(h, False)[0].t()


def dense_macs(model, N):
    """Multiply-adds of the dense chain per cloud of N points, per stage (the embedding counted with stage 0)."""
    out = []
    pairs = iter(model._pairs())
    lin, _ = next(pairs)
    emb = lin.weight.shape[0] * lin.weight.shape[1] * N
    for i, g in enumerate(model.local_grouper_list):
        cols, total = g.groups * g.kneighbors, emb if i == 0 else 0
        lin, _ = next(pairs)
        total += lin.weight.shape[0] * lin.weight.shape[1] * cols
        for _ in model.pre_blocks_list[i].operation:
            for _ in range(2):
                lin, _ = next(pairs)
                total += lin.weight.shape[0] * lin.weight.shape[1] * cols
        for _ in model.pos_blocks_list[i].operation:
            for _ in range(2):
                lin, _ = next(pairs)
                total += lin.weight.shape[0] * lin.weight.shape[1] * g.groups
        out.append(total)
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
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    print(json.dumps({"device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
                      "torch": torch.__version__, "reps": reps, "rounds": rounds}), flush=True)
    dev = torch.device("cuda:0")
    B, N = 8, 1024
    with torch.no_grad():
        model = seeded_fill_pointmlp(pointMLP(4), 1).eval().requires_grad_(False).to(dev)
        c = O.clouds(B, N, 9, real=[N, 90, N, 341, N, 853, N, 500])
        x = torch.from_numpy(c).permute(0, 2, 1).contiguous().to(dev)
        xyz = torch.from_numpy(c).to(dev)
        tables = model.geometry(xyz)
        fns = {"forward": lambda: model(x, return_features=True), "geometry": lambda: model.geometry(xyz),
               "dense_chain": lambda: model.dense(x, tables, True), "eager_torch_f32": lambda: eager_dense(model, x, tables)}
        a, b = fns["dense_chain"](), fns["eager_torch_f32"]()
        agree = float((a - b).double().norm() / b.double().norm())
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(per_call_ms(fn, reps))
        macs = dense_macs(model, N)
        md = statistics.median(times["dense_chain"])
        flop = 2.0 * sum(macs) * B
        print(json.dumps({"shape": [B, 3, N], **{k: stats(v) for k, v in times.items()},
                          "dense_over_eager": round(md / statistics.median(times["eager_torch_f32"]), 3),
                          "geometry_share_of_forward": round(statistics.median(times["geometry"]) /
                                                             statistics.median(times["forward"]), 3),
                          "features_rel_l2_hip_vs_eager": agree, "gmac_per_cloud_by_stage": [round(m / 1e9, 2) for m in macs],
                          "dense_tflops": round(flop / md / 1e9, 1),
                          "frac_of_f32_matrix_peak": round(flop / (md * 1e-3) / PEAK_F32_MATRIX, 3)}), flush=True)
        pts, cur = N, xyz
        for i, g in enumerate(model.local_grouper_list):
            f = tables[i][0]
            tf = [per_call_ms(lambda: KM.fps(cur, g.groups), reps) for _ in range(rounds)]
            tk = [per_call_ms(lambda: KM.knn(cur, f, g.kneighbors), reps) for _ in range(rounds)]
            print(json.dumps({"stage": i, "points": pts, "anchors": g.groups, "fps": stats(tf),
                              "fps_ns_per_pick": round(statistics.median(tf) * 1e6 / max(1, g.groups - 1), 1), "knn": stats(tk)}),
                  flush=True)
            cur = torch.gather(cur, 1, f.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
            pts = g.groups
        del model
        gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "pointmlp.npz")))
        for name in CASES:
            _, _, f64, l64 = oracle64(gold, name)
            m = make(name).to(dev)
            xg = torch.from_numpy(gold[f"{name}_x"]).to(dev)
            print(json.dumps({"parity": name, "per_cloud_rel_l2_vs_float64": {
                "features_hip": O.rel_l2_per_sample(m(xg, return_features=True), f64),
                "features_reference_float32": gold[f"{name}_feat_err"].tolist(),
                "logits_hip": O.rel_l2_per_sample(m(xg), l64),
                "logits_reference_float32": gold[f"{name}_logit_err"].tolist()}, "limit": "3 x the reference's"}), flush=True)


if __name__ == "__main__":
    main()
