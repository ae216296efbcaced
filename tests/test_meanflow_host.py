"""MeanFlow generator, host side (CPU suite): registry, checkpoint keys against the reference's (tests/golden/meanflow.npz,
tests/golden/make_meanflow_fixtures.py), the config against option_meanflow_nusc.py, the factories, the refusals."""
import ctypes

import numpy as np
import pytest
import torch


def _keys(module):
    return sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())


def _full_model():
    from lidargen.models.unets import __all__ as U
    from lidargen.utils.configs import __all__ as C

    cfg = C["meanflow-nusc"]()
    return U["mf_efficient_unet"](in_channels=2, resolution=cfg.data.resolution, **cfg.model.params)


def test_registry_resolves_the_generator():
    from lidargen.models.flows import __all__ as F
    from lidargen.models.flows import MeanFlow
    from lidargen.models.unets import __all__ as U
    from lidargen.models.unets.efficient_mf_unet import MFEfficientUNet

    assert U["mf_efficient_unet"] is MFEfficientUNet
    assert F == {"mean": MeanFlow}
    m = _full_model()
    assert sum(p.numel() for p in m.parameters()) == 31_180_934


def test_state_dict_keys_match_the_reference(golden):
    from lidargen.models.flows import MeanFlow

    g = golden("meanflow")
    m = _full_model()
    assert _keys(m) == list(g["keys_model"])
    flow = MeanFlow(m, channels=2, image_size=(32, 1024))
    assert _keys(flow) == list(g["keys_flow"])
    assert all(k.startswith("model.") for k in flow.state_dict())


def test_efficient_unet_keys_unchanged(golden):
    """The attention class became a Block argument: EfficientUNet's checkpoint keys are still the reference's."""
    from lidargen.models.unets import EfficientUNet

    m = EfficientUNet(2, (32, 1024), base_channels=64, coords_encoding="fourier_features")
    assert _keys(m) == list(golden("unet_full")["keys"])


def test_config_matches_the_reference_option_file():
    from lidargen.utils.configs import __all__ as C

    cfg = C["meanflow-nusc"]()
    # option_meanflow_nusc.py, written out as data
    assert cfg.model.architecture == "mf_efficient_unet"
    assert cfg.model.params == {"base_channels": 64, "temb_channels": None, "channel_multiplier": (1, 2, 4, 8),
                                "num_residual_blocks": (3, 3, 3, 3), "gn_num_groups": 8, "gn_eps": 1e-6,
                                "attn_num_heads": 8, "coords_encoding": "fourier_features", "ring": True}
    f = cfg.flow
    assert (f.flow_type, f.channels, tuple(f.image_size), f.flow_ratio) == ("mean", 2, (32, 1024), 0.5)
    assert f.normalizer == ["minmax", None, None] and f.time_dist == ["lognorm", -0.4, 1]
    assert (f.cfg_ratio, f.cfg_scale, f.cfg_unconditional, f.jvp_api) == (0.1, None, "u", "autograd")
    t = cfg.training
    assert (t.batch_size_train, t.batch_size_eval, t.num_workers, t.num_steps, t.steps_save_image,
            t.steps_save_model, t.gradient_accumulation_steps) == (2, 8, 4, 300_000, 5_000, 10_000, 1)
    assert (t.lr, t.lr_warmup_steps, t.adam_beta1, t.adam_beta2, t.adam_weight_decay, t.adam_epsilon) == \
        (1e-4, 10_000, 0.9, 0.99, 0.0, 1e-8)
    assert (t.ema_decay, t.ema_update_every, t.mixed_precision, t.dynamo_backend, t.output_dir, t.seed) == \
        (0.995, 10, "fp16", "inductor", "logs/diffusion", 0)
    d = cfg.data
    assert (d.dataset, d.depth_format, d.scan_unfolding, d.projection, d.train_depth, d.train_reflectance) == \
        ("nuscenes", "log_depth", False, "spherical-1024", True, True)
    assert (tuple(d.resolution), d.min_depth, d.max_depth, d.fov_up, d.fov_down) == ((32, 1024), 1.45, 80.0, 10.0, -30.0)
    assert not hasattr(cfg, "diffusion") and cfg.resume is None


def _synthetic_ckpt():
    from lidargen.utils import inference
    from lidargen.utils.configs import __all__ as C

    from lidarcrafter_amd.testing import seeded_fill, seeded_fill_qk_gains

    cfg = C["meanflow-nusc"]()
    flow, model, lu = inference.load_model_flow_training(cfg)
    seeded_fill(flow, salt=3)
    seeded_fill_qk_gains(flow, salt=3)
    sd = {k: v.clone() for k, v in flow.state_dict().items()}
    import dataclasses

    return {"cfg": dataclasses.asdict(cfg), "ema_weights": sd, "weights": sd, "global_step": 12}, sd


def test_setup_model_flow_on_cpu(capsys):
    from lidargen.utils import inference
    from lidargen.utils.lidar import get_linear_ray_angles

    ckpt, sd = _synthetic_ckpt()
    flow, lidar_utils, cfg = inference.setup_model_flow("meanflow-nusc", ckpt, device="cpu")
    assert "#params: 31,180,934" in capsys.readouterr().out
    assert type(flow).__name__ == "MeanFlow" and type(flow.model).__name__ == "MFEfficientUNet"
    assert all(torch.equal(flow.state_dict()[k], v) for k, v in sd.items())
    assert torch.equal(flow.model.coords, get_linear_ray_angles(32, 1024, 10.0, -30.0))
    assert torch.equal(lidar_utils.ray_angles, flow.model.coords)
    assert flow.image_size == (32, 1024) and flow.channels == 2
    with pytest.raises(RuntimeError):
        flow.sample()                          # no CPU path
    with pytest.raises(NotImplementedError, match="JVP"):
        flow.loss(torch.zeros(1, 2, 32, 1024))
    with pytest.raises(NotImplementedError, match="JVP"):
        flow({"x_0": torch.zeros(1, 2, 32, 1024)})


def test_load_model_flow_training_resume(tmp_path):
    from lidargen.utils import inference
    from lidargen.utils.configs import __all__ as C

    ckpt, sd = _synthetic_ckpt()
    ckpt.update(optimizer={"o": 1}, lr_scheduler={"s": 2})
    path = tmp_path / "ckpt.pt"
    torch.save(ckpt, path)
    cfg = C["meanflow-nusc"]()
    assert len(inference.load_model_flow_training(cfg)) == 3
    cfg.resume = str(path)
    flow, model, lu, step, opt, sched = inference.load_model_flow_training(cfg)
    assert (step, opt, sched) == (12, {"o": 1}, {"s": 2}) and flow.model is model
    assert all(torch.equal(flow.state_dict()[k], v) for k, v in sd.items())


def test_host_helpers_match_the_reference_formulas():
    from lidargen.models.flows.mean_flow import MeanFlow, Normalizer, adaptive_l2_loss

    e = torch.linspace(-1, 1, 2 * 3 * 4 * 5).reshape(2, 3, 4, 5)
    d = (e ** 2).mean(dim=(1, 2, 3))
    assert torch.allclose(adaptive_l2_loss(e), (d / (d + 1e-3) ** 0.5).mean())
    n = Normalizer.from_list(["minmax", None, None])
    assert torch.equal(n.unnorm(n.norm(torch.tensor([0.25]))), torch.tensor([0.25]))
    flow = MeanFlow(torch.nn.Linear(1, 1), channels=2, image_size=(8, 64))
    np.random.seed(0)
    t, r = flow.sample_t_r(64, "cpu")
    assert bool((r <= t).all()) and int((r == t).sum()) >= 32
    assert torch.equal(MeanFlow.time_grid(2), torch.tensor([1.0, 0.5, 0.0]))


def test_model_refuses_cpu_and_grad_mode():
    from lidarcrafter_amd.lidargen.models.unets.efficient_mf_unet import MFEfficientUNet

    m = MFEfficientUNet(2, (8, 64), base_channels=16, coords_encoding="fourier_features")
    x = torch.zeros(1, 2, 8, 64)
    with pytest.raises(NotImplementedError, match="jvp"):
        m(x, torch.tensor(1.0), torch.tensor(0.0))
    with torch.no_grad(), pytest.raises(RuntimeError, match="CUDA"):
        m(x, torch.tensor(1.0), torch.tensor(0.0))


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    LC_EINVAL, LC_EUNSUP = -1, -2
    qk = h.lc_qk_norm_cm_fwd
    assert qk(p, 0, 16, p, 0, 16, p, p, 1, 1, 128, 16, None) == LC_EUNSUP       # d = 128 > 64
    assert qk(p, 0, 16, p, 0, 16, p, p, 1, 70000, 8, 16, None) == LC_EUNSUP     # B * heads > 65535
    assert qk(p, 0, 16, p, 0, 16, p, p, 0, 1, 8, 16, None) == LC_EINVAL         # B = 0
    assert qk(p, 0, 16, p, 0, 16, p, p, 1, 1, 0, 16, None) == LC_EINVAL         # d = 0
    assert qk(p, 0, 16, p, 0, 16, p, p, 1, 1, 8, 0, None) == LC_EINVAL          # L = 0
    assert qk(p, 0, 16, p, 0, 16, None, p, 1, 1, 8, 16, None) == LC_EINVAL      # no gain
    fs = h.lc_flow_step_fwd
    assert fs(p, 8, p, 8, p, p, 8, 0, 8, None) == LC_EINVAL                      # B = 0
    assert fs(p, 8, p, 8, p, p, 8, 1, 0, None) == LC_EINVAL                      # n = 0
    assert fs(p, 8, p, 8, None, p, 8, 1, 8, None) == LC_EINVAL                   # no dt
    assert fs(p, 8, p, 8, p, p, 8, 70000, 8, None) == LC_EUNSUP                  # B > 65535


def test_fixture_summaries_are_consistent(golden):
    """The full-size outputs are stored as columns + row norms + sample norms: the stored columns of a row never hold
    more energy than the whole row, and the row norms make up the sample norms."""
    g = golden("meanflow")
    for prefix in ("y_full0", "y_full1", "ref_sample", "b8_s1", "b8_s2"):
        cols, rows, norm = (g[f"{prefix}_{k}"].astype(np.float64) for k in ("cols", "rownorm", "norm"))
        assert cols.shape[:-1] == rows.shape and rows.shape[0] == norm.shape[0]
        assert (np.linalg.norm(cols, axis=-1) <= rows * (1 + 1e-6)).all()
        assert np.allclose(np.sqrt((rows.reshape(rows.shape[0], -1) ** 2).sum(1)), norm, rtol=1e-5)
