"""MeanFlow generator timing, one process, one JSON line (profiles/meanflow.txt):
  * one-step `flow.sample()` wall time at batch 1 and 8 (32 x 1024, the meanflow-nusc params, seeded weights);
  * the MFEfficientUNet forward against an EfficientUNet forward of the same shape and params at batch 8, alternated
    call by call (same box, same clocks): the cost of what the MF model adds (q / k normalisation, two time MLPs).
  * --train (profiles/meanflow_train.txt): a MeanFlow training step (flow.loss + backward) against an EfficientUNet
    training step (ddpm loss + backward) at batch 8, alternated step by step, their peak memory, and kernel times of
    lc_attention_jvp_fwd against lc_attention_train_fwd and of the fused GroupNorm jvp pair against
    lc_groupnorm_stats + lc_groupnorm_apply_train on the same shapes.
python devtools/meanflow_time.py [reps] [--train]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidarcrafter_amd.testing import seeded_fill, seeded_fill_qk_gains, seeded_randn  # noqa: E402
from lidargen.utils import inference  # noqa: E402
from lidargen.utils.configs import __all__ as CONFIGS  # noqa: E402


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 30
    dev = torch.device("cuda:0")
    flow, mf, _ = inference.load_model_flow_training(CONFIGS["meanflow-nusc"]())
    seeded_fill(flow, salt=100)
    seeded_fill_qk_gains(flow, salt=100)
    flow = flow.eval().to(dev)
    ddpm, eu, _ = inference.load_model_duffusion_training(CONFIGS["nuscenes-unet-uncond"]())
    seeded_fill(eu, salt=100)
    eu = eu.eval().to(dev)
    from lidarcrafter_amd import ops as K
    K.prepare_model(flow), K.prepare_model(eu)
    out = {"shape": [2, 32, 1024], "reps": reps}

    for B in (1, 8):
        rng = lambda: [torch.Generator().manual_seed(i) for i in range(B)]  # noqa: E731
        for _ in range(3):
            flow.sample(batch_size=B, rng=rng())
        ts = [_ms(lambda: flow.sample(batch_size=B, rng=rng())) for _ in range(reps)]
        out[f"sample_1step_b{B}_ms"] = round(statistics.median(ts), 3)
        out[f"sample_1step_b{B}_min_ms"] = round(min(ts), 3)

    B = 8
    x = seeded_randn(B, 2, 32, 1024, seed=5).to(dev)
    t, r = torch.ones(B, device=dev), torch.zeros(B, device=dev)
    lam = torch.zeros(B, device=dev)
    with torch.inference_mode(), K.defer_range_checks():
        tf_mf, tf_eu = mf.time_features(t, r), eu.time_features(lam)
        for _ in range(3):
            mf(x, t, r, time_features=tf_mf), eu(x, lam, time_features=tf_eu)
        a, b = [], []
        for _ in range(reps):
            a.append(_ms(lambda: mf(x, t, r, time_features=tf_mf)))
            b.append(_ms(lambda: eu(x, lam, time_features=tf_eu)))
    K.range_poll(dev)
    out["mf_forward_b8_ms"] = round(statistics.median(a), 3)
    out["eu_forward_b8_ms"] = round(statistics.median(b), 3)
    out["mf_over_eu"] = round(statistics.median(a) / statistics.median(b), 4)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def _ev_us(fn, reps):
    """median device time of fn() in microseconds (events around each call)."""
    ts = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(ts[3:]), 2)


def train_main(reps):
    import numpy as np

    from lidarcrafter_amd import autograd as AG

    dev = torch.device("cuda:0")
    flow, mf, _ = inference.load_model_flow_training(CONFIGS["meanflow-nusc"]())
    seeded_fill(flow, salt=100)
    seeded_fill_qk_gains(flow, salt=100)
    flow = flow.train().to(dev)
    ddpm, eu, _ = inference.load_model_duffusion_training(CONFIGS["nuscenes-unet-uncond"]())
    seeded_fill(eu, salt=100)
    ddpm = ddpm.train().to(dev)
    B = 8
    x = seeded_randn(B, 2, 32, 1024, seed=5).clamp(-1, 1).to(dev)
    np.random.seed(0)
    torch.manual_seed(0)

    def mf_step():
        flow.zero_grad(set_to_none=True)
        flow({"x_0": x})[0].backward()

    def eu_step():
        ddpm.zero_grad(set_to_none=True)
        ddpm(x).backward()

    out = {"shape": [B, 2, 32, 1024], "reps": reps}
    peaks = {}
    for name, fn in (("mf", mf_step), ("eu", eu_step)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    a, b = [], []
    for _ in range(reps):
        a.append(_ms(mf_step))
        b.append(_ms(eu_step))
    out["mf_train_step_b8_ms"] = round(statistics.median(a), 2)
    out["eu_train_step_b8_ms"] = round(statistics.median(b), 2)
    out["mf_over_eu_train"] = round(statistics.median(a) / statistics.median(b), 3)
    out["mf_peak_mib"], out["eu_peak_mib"] = round(peaks["mf"], 1), round(peaks["eu"], 1)
    out["peak_ratio"] = round(peaks["mf"] / peaks["eu"], 3)

    # kernels at the model's level-4 attention shape: B * 8 heads, 64 channels, 512 tokens
    q, k, v, dq, dk, dv = (seeded_randn(B, 8, 64, 512, seed=10 + i).to(dev) for i in range(6))
    o = torch.empty_like(q)
    lse = torch.empty(B * 8, 512, device=dev)
    amax = torch.empty(3, device=dev)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    lib = AG.lib()
    out["attn_jvp_fwd_us"] = _ev_us(lambda: AG.attention_jvp_launch(q, k, v, dq, dk, dv, 0.125), reps)
    for prec, flag in (("f16x2", 1), ("f32", 0)):
        out[f"attn_train_fwd_{prec}_us"] = _ev_us(lambda: lib.lc_attention_train_fwd(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B * 8, 512, 512, 64, 64, 0.125, flag,
            amax.data_ptr() if flag else None, st()), reps)
    # GroupNorm: the first level's AdaGN + SiLU, [8, 64, 32, 1024]
    for shape in ((B, 64, 32, 1024), (B, 512, 4, 128)):
        xg, dxg = seeded_randn(*shape, seed=20).to(dev), seeded_randn(*shape, seed=21).to(dev)
        sc, sh = (seeded_randn(B, shape[1], seed=22 + i).to(dev) * 0.1 for i in range(2))
        tag = "x".join(map(str, shape))
        out[f"gn_jvp_pair_{tag}_us"] = _ev_us(lambda: AG.GroupNormActJvp.apply(xg, None, None, sc, sh, 8, 1e-6, True, dxg,
                                                                                sc, sh), reps)
        out[f"gn_stats_apply_{tag}_us"] = _ev_us(lambda: AG.GroupNormAct.apply(xg, None, None, sc, sh, 8, 1e-6, True),
                                                 reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--train" in sys.argv:
        train_main(int(args[0]) if args else 20)
    else:
        main()
