"""HDiT training timing, one process, one JSON line (profiles/hdit_train.txt):
  * a training step (ddpm(x0) in train mode, backward, AdamW) of nuscenes-hdit-uncond (32 x 1024, seeded weights) against
    an EfficientUNet training step (nuscenes-unet-uncond) at batch 2 (the config's) and 8, alternated step by step;
  * the peak memory of each step;
  * the neighbourhood kernels at level 0 (batch 8, 2 heads x 64 channels, 32 x 256 tokens, 3 x 9 window): the inference
    forward, the training forward (+ log-sum-exp) and the backward (dq, dk, dv).
python devtools/hdit_train_time.py [reps] [--hdit-only]
(--hdit-only: batch-8 HDiT steps alone, for rocprofv3 --kernel-trace --stats -- python devtools/hdit_train_time.py 3 --hdit-only)"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidarcrafter_amd.testing import seeded_fill, seeded_fill_hdit, seeded_randn  # noqa: E402
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
    reps = int(args[0]) if args else 10
    hdit_only = "--hdit-only" in sys.argv
    dev = torch.device("cuda:0")
    hd, _, _ = inference.load_model_duffusion_training(CONFIGS["nuscenes-hdit-uncond"]())
    seeded_fill(hd, salt=100)
    seeded_fill_hdit(hd, salt=100)
    hd = hd.train().to(dev)
    eu, _, _ = inference.load_model_duffusion_training(CONFIGS["nuscenes-unet-uncond"]())
    seeded_fill(eu, salt=100)
    eu = eu.train().to(dev)
    opts = {id(m): torch.optim.AdamW(m.parameters(), lr=1e-6) for m in (hd, eu)}
    out = {"shape": [2, 32, 1024], "reps": reps}
    torch.manual_seed(0)

    for B in ((8,) if hdit_only else (2, 8)):
        x = seeded_randn(B, 2, 32, 1024, seed=5).clamp(-1, 1).to(dev)

        def step(m):
            opt = opts[id(m)]
            opt.zero_grad(set_to_none=True)
            m(x).backward()
            opt.step()

        if hdit_only:
            for _ in range(reps):
                step(hd)
            torch.cuda.synchronize()
            print(json.dumps({"hdit_only_steps_b8": reps}))
            return
        peaks = {}
        for name, m in (("hdit", hd), ("eu", eu)):
            for _ in range(2):
                step(m)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            step(m)
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        a, b = [], []
        for _ in range(reps):
            a.append(_ms(lambda: step(hd)))
            b.append(_ms(lambda: step(eu)))
        out[f"hdit_train_step_b{B}_ms"] = round(statistics.median(a), 2)
        out[f"eu_train_step_b{B}_ms"] = round(statistics.median(b), 2)
        out[f"hdit_over_eu_train_b{B}"] = round(statistics.median(a) / statistics.median(b), 3)
        out[f"hdit_peak_b{B}_mib"], out[f"eu_peak_b{B}_mib"] = round(peaks["hdit"], 1), round(peaks["eu"], 1)

    from lidarcrafter_amd import ops as K

    B, heads, d, h, w = 8, 2, 64, 32, 256
    C = heads * d
    qkv = seeded_randn(B, 3 * C, h * w, seed=9).to(dev)
    q, k, v = qkv[:, :C].contiguous(), qkv[:, C:2 * C].contiguous(), qkv[:, 2 * C:]
    do = seeded_randn(B, C, h * w, seed=10).to(dev)
    o, lse = K.hdit_na_train(q, k, v, heads, h, w, (3, 9))
    n = 50
    for name, fn in (("na_fwd", lambda: K.hdit_na(q, k, v, heads, h, w, (3, 9))),
                     ("na_train_fwd", lambda: K.hdit_na_train(q, k, v, heads, h, w, (3, 9))),
                     ("na_bwd", lambda: K.hdit_na_bwd(q, k, v, o, do, lse, heads, h, w, (3, 9)))):
        for _ in range(3):
            fn()
        out[f"{name}_level0_b8_us"] = round(_ms(lambda: [fn() for _ in range(n)]) / n * 1e3, 2)
    out["na_bwd_over_fwd"] = round(out["na_bwd_level0_b8_us"] / out["na_fwd_level0_b8_us"], 2)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
