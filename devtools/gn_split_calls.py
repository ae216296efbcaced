"""What every pre-split GroupNorm apply pass of one C2 sampling step is called with: shape, batch stride of the input,
statistics segments (channels, slots, unit), entries one block folds (n_ent), AdaGN scale / shift present.
    python devtools/gn_split_calls.py        (one eager step of bench.py's model; needs the GPU)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from lidarcrafter_amd import ops as K  # noqa: E402

dev = torch.device("cuda:0")
ddpm, _ = bench.build_ddpm(dev)
orig, n = K._groupnorm_split, [0]


def logged(x, x_bs, G, eps, gamma, beta, scale, shift, act_silu, packed):
    B, C, H, W = x.shape
    hs = K._find_stats(x, G, octet_groups=True)
    segs = [(h.channels, h.slots, h.unit) for h in hs] if hs else None
    n_ent = [(C // G // u) * s for _, s, u in segs] if segs else None
    print(f"{n[0]:3d} x {B}x{C}x{H}x{W} x_bs {x_bs} (C*HW {C * H * W}) G {G} segments {segs} n_ent {n_ent} "
          f"adagn {scale is not None} silu {act_silu} ptr%4096 {x.data_ptr() % 4096} consumer {packed.name}", flush=True)
    n[0] += 1
    return orig(x, x_bs, G, eps, gamma, beta, scale, shift, act_silu, packed)


K._groupnorm_split = logged
x_T = bench.x_T_for(0, ddpm.sampling_shape, 1).to(dev)
state = ddpm.begin_sampling(8, 4, rng=None, mode="ddim", ddim_eta=0.0, x_T=x_T)
ddpm.sampling_step(state)          # step 0 runs eagerly
torch.cuda.synchronize()
