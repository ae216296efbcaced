"""MeanFlow training on the CPU side: the new C entry points refuse bad arguments before any launch, and the training
fixture (tests/golden/meanflow_train.npz) is self-consistent under the host formula of MeanFlow.loss."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC_EINVAL, LC_EUNSUP = -1, -2


def test_jvp_entry_points_refuse_bad_arguments_before_any_launch():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    p = 4096                                   # never dereferenced: every call below must be refused first
    # GroupNorm jvp
    assert h.lc_groupnorm_jvp_partials_elems(2, 64, 8, 64, 8) == 2 * 8 * 1 * 4       # one 4096-element chunk per group
    assert h.lc_groupnorm_jvp_partials_elems(2, 60, 8, 64, 8) == 0                    # C % G
    assert h.lc_groupnorm_jvp_stats(None, 0, p, 0, p, 1, 64, 8, 64, 8, None) == LC_EINVAL
    assert h.lc_groupnorm_jvp_stats(p, 0, None, 0, p, 1, 64, 8, 64, 8, None) == LC_EINVAL
    assert h.lc_groupnorm_jvp_stats(p, 0, p, 0, p, 1, 60, 8, 64, 8, None) == LC_EINVAL
    args = [p, 0, p, 0, p, None, None, None, None, None, None, 0, p, 0, p, 0, 1, 64, 8, 64, 8, 1e-6, 1, None, None, None,
            None]

    def apply(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return h.lc_groupnorm_jvp_apply_train(*a)

    assert apply(a14=None) == LC_EINVAL                   # no dy
    assert apply(a5=p) == LC_EINVAL                       # gamma without beta
    assert apply(a9=p) == LC_EINVAL                       # dscale without scale
    assert apply(a10=p, a8=None) == LC_EINVAL             # dshift without shift
    assert apply(a17=0) == LC_EINVAL                      # C = 0
    # qk norm
    assert h.lc_qk_norm_cm_jvp(None, 0, 8, p, 0, 8, p, p, 0, 8, p, 0, 8, 1, 2, 4, 8, None) == LC_EINVAL
    assert h.lc_qk_norm_cm_jvp(p, 0, 8, p, 0, 8, p, p, 0, 8, None, 0, 8, 1, 2, 4, 8, None) == LC_EINVAL   # dx w/o dy
    assert h.lc_qk_norm_cm_jvp(p, 0, 8, None, 0, 8, p, None, 0, 8, None, 0, 8, 1, 2, 4, 8, None) == LC_EINVAL
    assert h.lc_qk_norm_cm_jvp(p, 0, 0, None, 0, 0, p, p, 0, 8, None, 0, 0, 1, 2, 4, 8, None) == LC_EINVAL  # x_cs
    assert h.lc_qk_norm_cm_jvp(p, 0, 8, p, 0, 8, p, p, 0, 8, p, 0, 8, 1, 2, 96, 8, None) == LC_EUNSUP    # d > 64
    assert h.lc_qk_norm_cm_bwd_partials(2, 8, 512) == 2 * 8 * 2
    assert h.lc_qk_norm_cm_bwd(p, 0, 8, p, 0, 8, p, None, 0, 8, None, None, 1, 2, 4, 8, None) == LC_EINVAL  # no gx
    assert h.lc_qk_norm_cm_bwd(p, 0, 8, p, 0, 8, p, p, 0, 8, p, None, 1, 2, 4, 8, None) == LC_EINVAL       # half dg
    assert h.lc_qk_norm_cm_bwd(p, 0, 8, p, 0, -8, p, p, 0, 8, None, None, 1, 2, 4, 8, None) == LC_EINVAL   # gy_cs
    assert h.lc_qk_norm_cm_bwd(p, 0, 8, p, 0, 8, p, p, 0, 8, None, None, 1, 2, 65, 8, None) == LC_EUNSUP
    assert h.lc_qk_norm_cm_bwd(p, 0, 8, p, 0, 8, p, p, 0, 8, None, None, 70000, 1, 4, 8, None) == LC_EUNSUP
    # attention jvp
    a = [p] * 9
    assert h.lc_attention_jvp_fwd(*a, 1, 32, 32, 96, 32, 1.0, None) == LC_EUNSUP          # dqk > 64
    assert h.lc_attention_jvp_fwd(*a, 1, 32, 32, 32, 65, 1.0, None) == LC_EUNSUP          # dv > 64
    assert h.lc_attention_jvp_fwd(*a, 0, 32, 32, 32, 32, 1.0, None) == LC_EINVAL
    assert h.lc_attention_jvp_fwd(*a, 1, 32, 0, 32, 32, 1.0, None) == LC_EINVAL
    assert h.lc_attention_jvp_fwd(*([p] * 5 + [None] + [p] * 3), 1, 32, 32, 32, 32, 1.0, None) == LC_EINVAL


def test_training_forward_refuses_cpu():
    import pytest

    from lidarcrafter_amd.lidargen.models.unets.efficient_mf_unet import MFEfficientUNet
    from lidargen.models.flows import MeanFlow

    m = MFEfficientUNet(2, (8, 64), base_channels=16, coords_encoding="fourier_features")
    x = torch.zeros(2, 2, 8, 64)
    o = torch.ones(2)
    with pytest.raises(NotImplementedError, match="jvp"):
        m.forward_jvp(x, o, o * 0, x, o, o * 0)
    flow = MeanFlow(m, channels=2, image_size=(8, 64))
    with pytest.raises(NotImplementedError, match="JVP"):
        flow.loss_terms(x, o, o * 0, x)


def test_fixture_reproduces_its_loss_in_float64():
    """u, dudt, t, r, x, e of the fixture give its loss and mse through the host formula (float64): pins the target
    u_tgt = v - (t - r) dudt, the stop-gradient error and adaptive_l2_loss."""
    from lidargen.models.flows.mean_flow import adaptive_l2_loss

    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "meanflow_train.npz")))
    d = {k: torch.from_numpy(g["s_" + k]).double() for k in ("x", "e", "u", "dudt", "t", "r")}
    t_, r_ = d["t"][:, None, None, None], d["r"][:, None, None, None]
    v = d["e"] - d["x"]
    err = d["u"] - (v - (t_ - r_) * d["dudt"])
    loss, mse = adaptive_l2_loss(err), (err ** 2).mean()
    assert abs(float(loss) - float(g["s_loss"])) <= 1e-5 * float(g["s_loss"])
    assert abs(float(mse) - float(g["s_mse"])) <= 1e-5 * float(g["s_mse"])
    assert bool((d["r"] <= d["t"]).all()) and int((d["r"] == d["t"]).sum()) == 1
    # the end-to-end draws respect r <= t and flow_ratio 0.5 (two of four rows r = t)
    assert bool((g["e2e_r"] <= g["e2e_t"]).all()) and int((g["e2e_r"] == g["e2e_t"]).sum()) >= 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "meanflow_train.npz")) < 600 * 1024
