"""Golden vectors of MeanFlow training (reference lidargen/models/flows/mean_flow.py MeanFlow.loss, :128-160), run on the
CPU from the read-only reference tree with jvp_api="autograd" (torch.autograd.functional.jvp with create_graph=True).

Run in the build container only:   python tests/golden/make_meanflow_train_fixtures.py
Output: tests/golden/meanflow_train.npz (committed).  The reference model, its timm Attention restatement and the weights
(seeded_fill + seeded_fill_qk_gains, salt 100) come from make_meanflow_fixtures.py, imported, not edited.

  * small model (base 16, 8 x 64, B = 4) at fixed t, r (two rows r < t, one r = t, one t = 1, r = 0): x from
    seeded_randn, e = torch.randn after torch.manual_seed(E_SEED) (what the reference's randn_like draws); u, dudt,
    loss, mse and a digest of every parameter gradient (name, norm, first 8 entries);
  * one seeded end-to-end flow.loss(x) of the small model: np.random.seed / torch.manual_seed, the drawn t and r, loss;
  * full meanflow-nusc model (32 x 1024, B = 2): u and dudt summaries, loss, mse and every parameter's gradient norm.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_meanflow_fixtures as MM  # noqa: E402

from lidarcrafter_amd.testing import seeded_randn  # noqa: E402

T_SMALL, R_SMALL = [0.9, 0.7, 0.5, 1.0], [0.2, 0.3, 0.5, 0.0]
T_FULL, R_FULL = [0.8, 1.0], [0.3, 0.0]
X_SEED_SMALL, E_SEED_SMALL = 611, 612
X_SEED_FULL, E_SEED_FULL = 621, 622
E2E_NP_SEED, E2E_TORCH_SEED, E2E_X_SEED = 5, 6, 613


def make_flow(m, res):
    return MM.MEAN_FLOW.MeanFlow(m, channels=2, image_size=res, normalizer=["minmax", None, None],
                                 time_dist=["lognorm", -0.4, 1], flow_ratio=0.5, cfg_ratio=0.1, cfg_scale=None,
                                 jvp_api="autograd")


def grad_digest(named_params):
    names, norms, heads = [], [], []
    for k, p_ in named_params:
        if p_.grad is None:
            continue
        g = p_.grad.detach().double().flatten()
        names.append(k)
        norms.append(float(g.norm()))
        h = torch.zeros(8, dtype=torch.float64)
        h[: min(8, g.numel())] = g[:8]
        heads.append(h)
    return np.array(names), np.array(norms), torch.stack(heads).numpy()


def fixed_loss(flow, x, t, r, e_seed):
    """The reference's own flow.loss(x) with sample_t_r pinned to (t, r) and e = randn_like(x) after manual_seed(e_seed);
    u and dudt from the same jvp call the reference makes."""
    t, r = torch.tensor(t), torch.tensor(r)
    flow.sample_t_r = lambda B, device: (t, r)
    flow.model.zero_grad(set_to_none=True)
    torch.manual_seed(e_seed)
    loss, mse = flow.loss(x)
    loss.backward()
    torch.manual_seed(e_seed)
    e = torch.randn_like(x)
    t_, r_ = t[:, None, None, None], r[:, None, None, None]
    z = (1 - t_) * x + t_ * e
    v = e - x
    u, dudt = torch.autograd.functional.jvp(lambda z_, t__, r__: flow.model(z_, t__, r__, condition=None), (z, t, r),
                                            (v, torch.ones_like(t), torch.zeros_like(r)))
    del flow.sample_t_r
    return loss.detach(), mse.detach(), e, u.detach(), dudt.detach()


def main():
    out = {}
    ms = MM.build(16, (8, 64))
    flow = make_flow(ms, (8, 64))
    x = seeded_randn(4, 2, 8, 64, seed=X_SEED_SMALL)
    loss, mse, e, u, dudt = fixed_loss(flow, x, T_SMALL, R_SMALL, E_SEED_SMALL)
    out.update(s_t=np.array(T_SMALL, np.float32), s_r=np.array(R_SMALL, np.float32), s_x=x, s_e=e, s_u=u, s_dudt=dudt,
               s_loss=loss, s_mse=mse, s_x_seed=np.int64(X_SEED_SMALL), s_e_seed=np.int64(E_SEED_SMALL))
    out["s_names"], out["s_norms"], out["s_heads"] = grad_digest(ms.named_parameters())

    # end to end: the reference's draws under np.random.seed / torch.manual_seed
    x2 = seeded_randn(4, 2, 8, 64, seed=E2E_X_SEED)
    np.random.seed(E2E_NP_SEED)
    t2, r2 = flow.sample_t_r(4, "cpu")
    np.random.seed(E2E_NP_SEED)
    torch.manual_seed(E2E_TORCH_SEED)
    loss2, mse2 = flow.loss(x2)
    out.update(e2e_np_seed=np.int64(E2E_NP_SEED), e2e_torch_seed=np.int64(E2E_TORCH_SEED),
               e2e_x_seed=np.int64(E2E_X_SEED), e2e_t=t2, e2e_r=r2, e2e_loss=loss2.detach(), e2e_mse=mse2.detach())

    # full size
    m = MM.build(64, (32, 1024))
    flow = make_flow(m, (32, 1024))
    x = seeded_randn(2, 2, 32, 1024, seed=X_SEED_FULL)
    loss, mse, e, u, dudt = fixed_loss(flow, x, T_FULL, R_FULL, E_SEED_FULL)
    out.update(MM.summary("f_u", u, MM.COL_STEP_FULL))
    out.update(MM.summary("f_dudt", dudt, MM.COL_STEP_FULL))
    out.update(f_t=np.array(T_FULL, np.float32), f_r=np.array(R_FULL, np.float32), f_loss=loss, f_mse=mse,
               f_x_seed=np.int64(X_SEED_FULL), f_e_seed=np.int64(E_SEED_FULL))
    names, norms, _ = grad_digest(m.named_parameters())
    out["f_names"], out["f_norms"] = names, norms

    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "meanflow_train.npz")
    MM.save_npz(path, arrays)
    assert os.path.getsize(path) < 600 * 1024, "meanflow_train.npz grew: store fewer columns"
    print(f"meanflow_train.npz  {os.path.getsize(path) / 1024:.1f} KiB  small loss {float(out['s_loss']):.6f}  "
          f"full loss {float(out['f_loss']):.6f}  e2e t {t2.tolist()} r {r2.tolist()}")


if __name__ == "__main__":
    main()
