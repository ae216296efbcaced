"""HDiT training, host side (CPU suite): the train-mode refusals, the argument checks of the new C entry points and the
training fixture (tests/golden/hdit_train.npz, make_hdit_train_fixtures.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC_EINVAL, LC_EUNSUP = -1, -2


@pytest.fixture(autouse=True)
def _private_rng():
    with torch.random.fork_rng(devices=[]):
        yield


def _small(**kw):
    from lidargen.models.dits.hdit import HDiT

    return HDiT((32, 256), 2, base_channels=64, depths=(1, 1, 1, 1), **kw)


def test_train_mode_cpu_forward_has_no_cpu_path():
    m = _small().train()
    x = torch.zeros(1, 2, 32, 256)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m(x, torch.zeros(1))
    m.eval()
    with pytest.raises(NotImplementedError, match="HDiT training is not built for eval-mode forwards: call .train()"):
        m(x, torch.zeros(1))


def test_training_graph_refuses_dropout():
    from lidarcrafter_amd.autograd_hdit import hdit_forward

    m = _small(dropout=0.1).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        hdit_forward(m, torch.zeros(1, 2, 32, 256), torch.zeros(1))


def test_eval_mode_loss_stays_value_only():
    """p_loss builds no graph for an eval-mode HDiT: the forward runs under no_grad (here it reaches the CPU refusal of
    the inference path, not the training one)."""
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion

    ddpm = ContinuousTimeGaussianDiffusion(_small(), torch.nn.Identity()).eval()
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ddpm(torch.zeros(1, 2, 32, 256))


def test_training_entry_points_refuse_bad_arguments_before_any_launch():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    p = 4096                                   # never dereferenced: every call below must be refused first
    op = _lib.CmOperand(p, 0, 0, 8)
    nul = _lib.CmOperand(None, 0, 0, 8)
    r = ctypes.byref
    # rmsnorm backward: (x, x_bs, x_cs, f, f_bs, mode, dy, dy_bs, dy_cs, dx, dx_bs, dx_cs, rs, df, df_bs, B, C, L, eps)
    a = [p, 0, 8, p, 0, 1, p, 0, 8, p, 0, 8, p, p, 8, 1, 8, 8, 1e-6, None]
    bad = lambda i, v: h.lc_hdit_rmsnorm_bwd(*(a[:i] + [v] + a[i + 1:]))  # noqa: E731
    assert bad(0, None) == LC_EINVAL                      # no x
    assert bad(9, None) == LC_EINVAL                      # no dx
    assert bad(5, 3) == LC_EINVAL                         # mode
    assert bad(3, None) == LC_EINVAL                      # mode 1 without f
    assert bad(12, None) == LC_EINVAL                     # df without rs scratch
    assert bad(16, 0) == LC_EINVAL                        # C = 0
    assert bad(18, 0.0) == LC_EINVAL                      # eps
    assert bad(15, 70000) == LC_EUNSUP                    # B > 65535
    # geglu backward
    assert h.lc_hdit_geglu_bwd(None, 0, p, 0, p, 0, 1, 8, 8, None) == LC_EINVAL
    assert h.lc_hdit_geglu_bwd(p, 0, p, 0, p, 0, 1, 0, 8, None) == LC_EINVAL
    assert h.lc_hdit_geglu_bwd(p, 0, p, 0, p, 0, 70000, 8, 8, None) == LC_EUNSUP
    # q / k preparation backward
    q = [p, 0, 8] * 6 + [p, p, p, p, p]
    assert h.lc_hdit_qk_prep_bwd(*q, 1, 2, 48, 8, None) == LC_EUNSUP         # d = 48
    assert h.lc_hdit_qk_prep_bwd(*q, 40000, 2, 32, 8, None) == LC_EUNSUP     # B * heads > 65535
    q2 = list(q)
    q2[21] = None                                                             # no scratch
    assert h.lc_hdit_qk_prep_bwd(*q2, 1, 2, 32, 8, None) == LC_EINVAL
    q3 = list(q)
    q3[14] = 0                                                                # dq channel stride
    assert h.lc_hdit_qk_prep_bwd(*q3, 1, 2, 32, 8, None) == LC_EINVAL
    # neighbourhood attention: train forward and backward share the forward's limits
    ops5 = [r(op)] * 5
    assert h.lc_hdit_na_train_fwd(r(op), r(op), r(op), p, 0, 0, 8, None, 1, 2, 32, 8, 16, 3, 9, 1.0, None) == \
        LC_EINVAL                                                             # no lse
    assert h.lc_hdit_na_train_fwd(r(op), r(op), r(op), p, 0, 0, 8, p, 1, 2, 32, 8, 16, 3, 8, 1.0, None) == LC_EUNSUP
    assert h.lc_hdit_na_bwd(*ops5, p, p, p, p, p, 1, 2, 32, 2, 16, 3, 9, 1.0, None) == LC_EUNSUP   # kh > h
    assert h.lc_hdit_na_bwd(*ops5, p, p, p, p, p, 1, 2, 32, 8, 16, 4, 9, 1.0, None) == LC_EUNSUP   # even kh
    assert h.lc_hdit_na_bwd(*ops5, p, p, p, p, p, 1, 2, 32, 16, 16, 9, 11, 1.0, None) == LC_EUNSUP  # kh * kw > 81
    assert h.lc_hdit_na_bwd(*ops5, p, p, p, p, p, 1, 2, 96, 8, 16, 3, 9, 1.0, None) == LC_EUNSUP   # d = 96
    assert h.lc_hdit_na_bwd(*ops5, p, p, p, p, p, 1, 2, 32, 8, 2, 3, 9, 1.0, None) == LC_EUNSUP    # kw / 2 > w
    assert h.lc_hdit_na_bwd(*ops5, p, None, p, p, p, 1, 2, 32, 8, 16, 3, 9, 1.0, None) == LC_EINVAL  # no scratch
    assert h.lc_hdit_na_bwd(r(nul), *ops5[1:], p, p, p, p, p, 1, 2, 32, 8, 16, 3, 9, 1.0, None) == LC_EINVAL
    assert h.lc_hdit_na_bwd(*ops5, p, p, p, p, p, 0, 2, 32, 8, 16, 3, 9, 1.0, None) == LC_EINVAL
    # lerp backward
    la = [p, 0, p, 0, p, 0, p, p, 0, p, 0, p, 1, 8, 4, 4, 2, 2, None]
    assert h.lc_hdit_lerp_bwd(*(la[:6] + [None] + la[7:])) == LC_EINVAL      # no alpha
    assert h.lc_hdit_lerp_bwd(*(la[:12] + [0] + la[13:])) == LC_EINVAL       # B = 0
    assert h.lc_hdit_lerp_bwd(*(la[:12] + [70000] + la[13:])) == LC_EUNSUP   # B > 65535


def test_training_fixture_keys_and_size():
    path = os.path.join(ROOT, "tests", "golden", "hdit_train.npz")
    assert os.path.getsize(path) < 600 * 1024
    g = dict(np.load(path))
    for k in ("steps", "s_x_seed", "s_n_seed", "s_loss32", "s_loss64", "s_names", "s_norms32", "s_norms64", "s_heads32",
              "s_heads64", "u_loss32", "u_loss64", "u_names", "u_norms32", "u_norms64", "u_heads32", "u_heads64",
              "f_x_seed", "f_n_seed", "f_loss32", "f_loss64", "f_names", "f_norms32", "f_norms64"):
        assert k in g, k
    assert len(g["s_names"]) == len(g["s_norms64"]) == len(g["s_heads64"]) and len(g["f_names"]) == len(g["f_norms64"])
    # every parameter of the full model has a gradient in the reference, under this project's parameter names
    from lidargen.models.dits import __all__ as D
    from lidargen.utils.configs import __all__ as C

    cfg = C["nuscenes-hdit-uncond"]()
    m = D["hdit"](in_channels=2, resolution=cfg.data.resolution, **cfg.model.params)
    assert [str(n) for n in g["f_names"]] == [n for n, _ in m.named_parameters()]
    assert any(str(n).endswith("residual_attn.scale") for n in g["s_names"])
