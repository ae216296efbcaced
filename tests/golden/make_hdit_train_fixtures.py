"""Golden vectors of HDiT training (reference lidargen/models/dits/hdit.py under ContinuousTimeGaussianDiffusion.p_loss,
base.py:124-141), run on the CPU from the read-only reference tree in train mode.

Run in the build container only:   python tests/golden/make_hdit_train_fixtures.py
Output: tests/golden/hdit_train.npz (committed).  The reference model, the natten restatement and the weights
(seeded_fill + seeded_fill_hdit, salt 100) come from make_hdit_fixtures.py, imported, not edited.

The noise of q_step_from_x_0 is pinned: `randn_like` returns seeded_randn(seed=N_SEED) and the steps are fixed, so the
loss is a function of the weights alone.  Each model runs once in float32 and once in float64 (the same weights): the
float64 run is the yardstick, the float32 run the reference's own rounding of this ill-conditioned model.

  * small model (base 64, 32 x 256, B = 2): loss, and a digest of every parameter gradient (name, norm, first 8 entries),
    with the clamped heads (prefix s, logits up to 100: ill-conditioned) and without them (prefix u: the logit scales
    near ln 10, where float32 rounding stays small and a gradient error cannot hide behind it);
  * full nuscenes-hdit-uncond model (base 128, 32 x 1024, B = 2, ray-angle coords): loss and every gradient norm.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_hdit_fixtures as MH  # noqa: E402

from lidarcrafter_amd.testing import seeded_randn  # noqa: E402

STEPS = [0.3, 0.8]
X_SEED_SMALL, N_SEED_SMALL = 641, 642
X_SEED_FULL, N_SEED_FULL = 651, 652


def grad_digest(named_params, heads=True):
    names, norms, hs = [], [], []
    for k, p_ in named_params:
        if p_.grad is None:
            continue
        g = p_.grad.detach().double().flatten()
        names.append(k)
        norms.append(float(g.norm()))
        h = torch.zeros(8, dtype=torch.float64)
        h[: min(8, g.numel())] = g[:8]
        hs.append(h)
    return np.array(names), np.array(norms), torch.stack(hs).numpy()


def pinned_loss(m, x, noise, dtype):
    """The reference's p_loss at STEPS with the noise pinned, in `dtype`; returns the loss (gradients left in m)."""
    m = m.to(dtype).train()
    ddpm = MH.DF.ContinuousTimeGaussianDiffusion(m, torch.nn.Identity()).train()
    n = noise.to(dtype)
    ddpm.randn_like = lambda x_, rng=None: n
    m.zero_grad(set_to_none=True)
    loss = ddpm.p_loss(x.to(dtype), torch.tensor(STEPS, dtype=dtype))
    loss.backward()
    return loss.detach().double()


def main():
    out = {"steps": np.array(STEPS, np.float32)}
    for prefix, base, res, ray, clamped, xs, ns in (
            ("s", 64, (32, 256), False, True, X_SEED_SMALL, N_SEED_SMALL),
            ("u", 64, (32, 256), False, False, X_SEED_SMALL, N_SEED_SMALL),
            ("f", 128, (32, 1024), True, True, X_SEED_FULL, N_SEED_FULL)):
        m = MH.build(base, res, ray_angles=ray, clamped_heads=clamped)
        x = seeded_randn(2, 2, *res, seed=xs)
        noise = seeded_randn(2, 2, *res, seed=ns)
        out[f"{prefix}_x_seed"], out[f"{prefix}_n_seed"] = np.int64(xs), np.int64(ns)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            loss = pinned_loss(m, x, noise, dtype)
            names, norms, heads = grad_digest(m.named_parameters())
            out[f"{prefix}_loss{tag}"] = loss.numpy()
            out[f"{prefix}_norms{tag}"] = norms
            if prefix != "f":
                out[f"{prefix}_heads{tag}"] = heads
            out[f"{prefix}_names"] = names
            print(prefix, tag, float(loss), flush=True)
        m.float()

    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "hdit_train.npz")
    MH.save_npz(path, arrays)
    assert os.path.getsize(path) < 600 * 1024, "hdit_train.npz grew"
    dev = np.abs(arrays["s_norms32"] - arrays["s_norms64"]) / np.maximum(arrays["s_norms64"], 1e-30)
    print(f"hdit_train.npz  {os.path.getsize(path) / 1024:.1f} KiB  small loss {float(arrays['s_loss64']):.6f}  full "
          f"loss {float(arrays['f_loss64']):.6f}  worst float32 gradient-norm deviation (small) {dev.max():.2e}")


if __name__ == "__main__":
    main()
