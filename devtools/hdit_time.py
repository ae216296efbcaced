"""HDiT timing, one process, one JSON line (profiles/hdit.txt):
  * the HDiT forward (nuscenes-hdit-uncond params, 32 x 1024, seeded weights, time features precomputed) against the
    EfficientUNet forward (nuscenes-unet-uncond) of the same batch, at batch 1 and 8, alternated call by call (same box,
    same clocks);
  * a 50-step DDIM `sample()` at batch 8 (first call: eager step + graph capture; then replays of the cached graph);
  * the neighbourhood-attention kernel alone at level 0 (batch 8, 2 heads x 64 channels, 32 x 256 tokens) and its
    effective bandwidth on q + k + v + o (each read / written once).
python devtools/hdit_time.py [reps]"""
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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    dev = torch.device("cuda:0")
    ddpm, hd, _ = inference.load_model_duffusion_training(CONFIGS["nuscenes-hdit-uncond"]())
    seeded_fill(ddpm, salt=100)
    seeded_fill_hdit(ddpm, salt=100)
    ddpm = ddpm.eval().to(dev)
    _, eu, _ = inference.load_model_duffusion_training(CONFIGS["nuscenes-unet-uncond"]())
    seeded_fill(eu, salt=100)
    eu = eu.eval().to(dev)
    from lidarcrafter_amd import ops as K
    K.prepare_model(ddpm), K.prepare_model(eu)
    out = {"shape": [2, 32, 1024], "reps": reps}

    for B in (1, 8):
        x = seeded_randn(B, 2, 32, 1024, seed=5).to(dev)
        lam = torch.linspace(-10, 10, B, device=dev)
        with torch.inference_mode(), K.defer_range_checks():
            tf_hd, tf_eu = hd.time_features(lam), eu.time_features(lam)
            for _ in range(3):
                hd(x, lam, time_features=tf_hd), eu(x, lam, time_features=tf_eu)
            a, b = [], []
            for _ in range(reps):
                a.append(_ms(lambda: hd(x, lam, time_features=tf_hd)))
                b.append(_ms(lambda: eu(x, lam, time_features=tf_eu)))
        K.range_poll(dev)
        out[f"hdit_forward_b{B}_ms"] = round(statistics.median(a), 3)
        out[f"eu_forward_b{B}_ms"] = round(statistics.median(b), 3)
        out[f"hdit_over_eu_b{B}"] = round(statistics.median(a) / statistics.median(b), 4)

    rng = lambda: [torch.Generator().manual_seed(i) for i in range(8)]  # noqa: E731
    out["ddim50_b8_first_ms"] = round(_ms(lambda: ddpm.sample(8, 50, progress=False, rng=rng(), mode="ddim")), 2)
    ts = [_ms(lambda: ddpm.sample(8, 50, progress=False, rng=rng(), mode="ddim")) for _ in range(3)]
    out["ddim50_b8_ms"] = round(statistics.median(ts), 2)

    B, heads, d, h, w = 8, 2, 64, 32, 256
    qkv = seeded_randn(B, 3 * heads * d, h * w, seed=9).to(dev)
    C = heads * d
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    o = torch.empty(B, C, h * w, device=dev)
    for _ in range(5):
        K.hdit_na(q, k, v, heads, h, w, (3, 9), out=o)
    n = 200
    ms = _ms(lambda: [K.hdit_na(q, k, v, heads, h, w, (3, 9), out=o) for _ in range(n)]) / n
    out["na_level0_b8_us"] = round(ms * 1e3, 2)
    out["na_level0_b8_gbps"] = round(4 * 4 * B * C * h * w / (ms * 1e-3) / 1e9, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
