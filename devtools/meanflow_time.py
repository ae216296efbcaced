"""MeanFlow generator timing, one process, one JSON line (profiles/meanflow.txt):
  * one-step `flow.sample()` wall time at batch 1 and 8 (32 x 1024, the meanflow-nusc params, seeded weights);
  * the MFEfficientUNet forward against an EfficientUNet forward of the same shape and params at batch 8, alternated
    call by call (same box, same clocks): the cost of what the MF model adds (q / k normalisation, two time MLPs).
python devtools/meanflow_time.py [reps]"""
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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
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


if __name__ == "__main__":
    main()
