"""HDiT, host side (CPU suite): registry, parameter count and checkpoint keys against the reference's
(tests/golden/hdit.npz, tests/golden/make_hdit_fixtures.py), the config against option_dit_nusc.py, the factories,
the refusals."""
import pytest
import torch


def _keys(module):
    return sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())


@pytest.fixture(autouse=True)
def _private_rng():
    """The constructors draw their initial weights from torch's global generator: every test here runs on a fork of
    it, so the tests that run after this file see the global stream as they would without it."""
    with torch.random.fork_rng(devices=[]):
        yield


def _full_model(**over):
    from lidargen.models.dits import __all__ as D
    from lidargen.utils.configs import __all__ as C

    cfg = C["nuscenes-hdit-uncond"]()
    params = dict(cfg.model.params, **over)
    return D["hdit"](in_channels=2, resolution=cfg.data.resolution, **params)


def test_registry_resolves_hdit():
    from lidargen.models.dits import __all__ as D
    from lidargen.models.dits.hdit import HDiT

    assert D == {"hdit": HDiT}
    m = _full_model()
    assert sum(p.numel() for p in m.parameters()) == 79_859_844
    assert len(m.state_dict()) == 213


def test_state_dict_keys_match_the_reference(golden):
    m = _full_model()
    keys = _keys(m)
    assert keys == list(golden("hdit")["keys_model"])
    for k in ("coords:(1, 2, 32, 1024)", "timestep_pe.0.freqs:(128,)",
              "down_levels.level_0.0.residual_attn.rope.freqs_h:(2, 16)",
              "mid_levels.2.residual_attn.rope.freqs_w:(16, 16)"):
        assert k in keys, k


def test_config_matches_the_reference_option_file():
    from lidargen.utils.configs import __all__ as C

    cfg = C["nuscenes-hdit-uncond"]()
    # option_dit_nusc.py, written out as data
    assert cfg.model.architecture == "hdit"
    assert cfg.model.params == {"base_channels": 128, "time_embed_channels": 256, "depths": (3, 3, 3, 3),
                                "dilation": (1, 1, 1, 1), "positional_embedding": "learnable_embedding", "ring": True}
    d = cfg.diffusion
    assert (d.num_training_steps, d.num_sampling_steps, d.prediction_type, d.loss_type, d.noise_schedule,
            d.timestep_type) == (None, 1024, "eps", "l2", "cosine", "continuous")
    t = cfg.training
    assert (t.batch_size_train, t.batch_size_eval, t.num_workers, t.num_steps, t.steps_save_image, t.steps_save_model,
            t.gradient_accumulation_steps, t.lr, t.lr_warmup_steps, t.adam_beta1, t.adam_beta2, t.adam_weight_decay,
            t.adam_epsilon, t.ema_decay, t.ema_update_every, t.mixed_precision, t.dynamo_backend, t.output_dir,
            t.seed) == (2, 8, 4, 2_560_000, 5_000, 100_000, 1, 1e-4, 80_000, 0.9, 0.99, 0.0, 1e-8, 0.995, 10, "fp16",
                        "inductor", "logs/diffusion", 0)
    a = cfg.data
    assert (a.dataset, a.depth_format, a.scan_unfolding, a.projection, a.train_depth, a.train_reflectance,
            tuple(a.resolution), a.min_depth, a.max_depth, a.fov_up, a.fov_down) == \
        ("nuscenes", "log_depth", False, "spherical-1024", True, True, (32, 1024), 1.45, 80.0, 10.0, -30.0)


def test_factories_build_hdit(tmp_path):
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion
    from lidargen.models.dits.hdit import HDiT
    from lidargen.utils import inference
    from lidargen.utils.configs import __all__ as C
    from lidargen.utils.lidar import get_linear_ray_angles

    cfg = C["nuscenes-hdit-uncond"]()
    ddpm, model, lidar_utils = inference.load_model_duffusion_training(cfg)
    assert isinstance(model, HDiT) and isinstance(ddpm, ContinuousTimeGaussianDiffusion)
    # spherical projection: the coords buffer holds the ray angles, as the reference's setup functions leave it
    assert torch.equal(model.coords, get_linear_ray_angles(32, 1024, 10.0, -30.0))
    ckpt = {"cfg": {}, "ema_weights": ddpm.state_dict(), "global_step": 0}
    path = tmp_path / "hdit.pth"
    torch.save(ckpt, path)
    ddpm2, lu, cfg2 = inference.setup_model("nuscenes-hdit-uncond", str(path), device="cpu", show_info=False)
    assert isinstance(ddpm2.model, HDiT)


def test_constructor_refuses_unbuilt_options():
    with pytest.raises(NotImplementedError, match="dilation"):
        _full_model(dilation=(1, 2, 1, 1))
    for pe in ("spherical_harmonics", "polar_coordinates", "fourier_features", None):
        with pytest.raises(NotImplementedError, match="positional_embedding"):
            _full_model(positional_embedding=pe)


def test_cpu_forward_raises():
    from lidargen.models.dits.hdit import HDiT

    m = HDiT((32, 256), 2, base_channels=64, depths=(1, 1, 1, 1)).eval()
    x = torch.zeros(1, 2, 32, 256)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="no CPU path"):
        m(x, torch.zeros(1))
    with pytest.raises(NotImplementedError, match="HDiT training is not built"):
        m(x, torch.zeros(1))
