"""MeanFlow sampler -- API / state_dict mirror of the reference's lidargen/models/flows/mean_flow.py.

The network predicts the average velocity u(z, t, r) between times r <= t, so one network call moves a sample from
noise (t = 1) to data (r = 0): `z - model(z, 1, 0)` (MeanFlow.sample, mean_flow.py:186-199).  Sampling runs on the HIP
path (MFEfficientUNet, ops.flow_step).  Training (`loss`, mean_flow.py:128-160 of the reference):

    u, dudt = jvp(model, (z, t, r), (v, 1, 0));   loss = adaptive_l2_loss(u - sg(v - (t - r) dudt))

The target is stop-gradient, so the parameter gradients flow through the primal u only: no double backward is needed.
The reference's `create_graph=True` (jvp_api "autograd") exists only because torch.autograd.functional.jvp computes a
JVP by the double-vjp trick; "autograd" and "funtorch" give the same loss and the same gradients, and both run
MFEfficientUNet.forward_jvp here (the differentiable forward with its tangent computed alongside, csrc/flow_jvp.hip).
`Normalizer`, `adaptive_l2_loss` and `sample_t_r` are the reference's host code."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from lidarcrafter_amd import ops as K


class Normalizer:
    # minmax for raw image, mean_std for vae latent
    def __init__(self, mode="minmax", mean=None, std=None):
        assert mode in ["minmax", "mean_std"], "mode must be 'minmax' or 'mean_std'"
        self.mode = mode
        if mode == "mean_std":
            if mean is None or std is None:
                raise ValueError("mean and std must be provided for 'mean_std' mode")
            self.mean = torch.tensor(mean).view(-1, 1, 1)
            self.std = torch.tensor(std).view(-1, 1, 1)

    @classmethod
    def from_list(cls, config):
        """config: [mode, mean, std]"""
        mode, mean, std = config
        return cls(mode, mean, std)

    def norm(self, x):
        if self.mode == "minmax":
            return x * 2 - 1
        return (x - self.mean.to(x.device)) / self.std.to(x.device)

    def unnorm(self, x):
        if self.mode == "minmax":
            return (x + 1) * 0.5
        return x * self.std.to(x.device) + self.mean.to(x.device)


def stopgrad(x):
    return x.detach()


def adaptive_l2_loss(error, gamma=0.5, c=1e-3):
    """sg(w) * ||delta||_2^2 with w = 1 / (||delta||^2 + c)^p, p = 1 - gamma (error [B, C, H, W] -> scalar)."""
    delta_sq = torch.mean(error ** 2, dim=(1, 2, 3), keepdim=False)
    p = 1.0 - gamma
    w = 1.0 / (delta_sq + c).pow(p)
    return (stopgrad(w) * delta_sq).mean()


def _hw(image_size):
    return tuple(image_size) if isinstance(image_size, (tuple, list)) else (image_size, image_size)


class MeanFlow(nn.Module):
    def __init__(self, model, channels=1, image_size=32, num_classes=None, normalizer=["minmax", None, None],
                 flow_ratio=0.50, time_dist=["lognorm", -0.4, 1.0], cfg_ratio=0.10, cfg_scale=2.0,
                 cfg_uncond="u", jvp_api="autograd"):
        super().__init__()
        self.model = model
        self.channels = channels
        self.image_size = image_size
        self.num_classes = num_classes
        self.use_cond = num_classes is not None
        self.normer = Normalizer.from_list(normalizer)
        self.flow_ratio = flow_ratio
        self.time_dist = time_dist
        self.cfg_ratio = cfg_ratio
        self.w = cfg_scale
        self.cfg_uncond = cfg_uncond
        self.jvp_api = jvp_api
        assert jvp_api in ["funtorch", "autograd"], "jvp_api must be 'funtorch' or 'autograd'"
        self.create_graph = jvp_api == "autograd"

    @property
    def device(self):
        return next(self.model.parameters()).device

    # r is never larger than t (reference mean_flow.py:108-132)
    def sample_t_r(self, batch_size, device):
        if self.time_dist[0] == "uniform":
            samples = np.random.rand(batch_size, 2).astype(np.float32)
        elif self.time_dist[0] == "lognorm":
            mu, sigma = self.time_dist[-2], self.time_dist[-1]
            normal_samples = np.random.randn(batch_size, 2).astype(np.float32) * sigma + mu
            samples = 1 / (1 + np.exp(-normal_samples))
        t_np = np.maximum(samples[:, 0], samples[:, 1])
        r_np = np.minimum(samples[:, 0], samples[:, 1])
        num_selected = int(self.flow_ratio * batch_size)
        indices = np.random.permutation(batch_size)[:num_selected]
        r_np[indices] = t_np[indices]
        return torch.tensor(t_np, device=device), torch.tensor(r_np, device=device)

    def loss(self, x, c=None):
        """(loss, mse_val) of the reference's MeanFlow.loss; `c` is ignored, as there.  Draws as the reference does:
        t, r from np.random (sample_t_r), then e from torch's global CPU generator with x's shape, copied to x's device --
        so `np.random.seed(a); torch.manual_seed(b); flow.loss(x_gpu)` draws what the reference's `flow.loss(x_cpu)`
        draws under the same seeds."""
        if not x.is_cuda:
            raise NotImplementedError("MeanFlow.loss: the JVP of the network runs on the GPU kernels only "
                                      "(MFEfficientUNet.forward_jvp); there is no CPU path")
        t, r = self.sample_t_r(x.shape[0], x.device)
        e = torch.randn(x.shape, dtype=x.dtype).to(x.device)
        loss, mse_val, _, _ = self.loss_terms(x, t, r, e)
        return loss, mse_val

    def loss_terms(self, x, t, r, e):
        """(loss, mse_val, u, dudt) for given times t, r [B] and noise e (the seam of the tests).  The tangent direction
        is (v, 1, 0); u carries the training graph, dudt none."""
        if not x.is_cuda:
            raise NotImplementedError("MeanFlow.loss: the JVP of the network runs on the GPU kernels only "
                                      "(MFEfficientUNet.forward_jvp); there is no CPU path")
        t, r, e = t.to(x.device).float(), r.to(x.device).float(), e.to(x.device)
        t_, r_ = t[:, None, None, None], r[:, None, None, None]
        z = (1 - t_) * x + t_ * e
        v = e - x
        u, dudt = self.model.forward_jvp(z, t, r, v, torch.ones_like(t), torch.zeros_like(r))
        u_tgt = v - (t_ - r_) * dudt
        error = u - stopgrad(u_tgt)
        loss = adaptive_l2_loss(error)
        mse_val = (stopgrad(error) ** 2).mean()
        return loss, mse_val, u, dudt

    def forward(self, batch):
        return self.loss(batch["x_0"], batch.get("y", None))

    # ---- sampling -----------------------------------------------------------------------------------------------------
    def _noise(self, batch_size, rng, device):
        """[B, channels, H, W] standard normal, drawn on the host and copied to `device` (the contract of
        models/diffusion/base.py randn): rng None -> torch's global CPU generator; one Generator; or a list of
        per-sample generators, sample i drawn from generator i alone."""
        shape = (batch_size, self.channels, *_hw(self.image_size))
        if rng is None or isinstance(rng, torch.Generator):
            dev = "cpu" if rng is None else rng.device
            return torch.randn(shape, generator=rng, device=dev).to(device)
        if isinstance(rng, list):
            assert len(rng) == batch_size
            return torch.stack([torch.randn(shape[1:], generator=g, device=g.device).to(device) for g in rng])
        raise ValueError(f"invalid rng: {rng}")

    @staticmethod
    def time_grid(num_steps: int) -> torch.Tensor:
        """float32 [S + 1]: t_i = 1 - i / S (t_0 = 1 noise, t_S = 0 data)."""
        return (1.0 - torch.arange(num_steps + 1, dtype=torch.float64) / num_steps).float()

    @torch.compiler.disable
    @torch.inference_mode()
    def sample(self, device=None, *, batch_size: int = 1, num_steps: int = 1, rng=None, return_all: bool = False):
        """`sample()` is the reference's formula: z ~ N(0, I) of batch 1, `z - model(z, 1, 0)`.  With the default
        rng (None) the noise comes from torch's global CPU generator, so `torch.manual_seed(s); flow.sample()` gives
        the noise of the reference's `torch.manual_seed(s); flow.sample(device="cpu")` (not that of its CUDA stream).
        num_steps = S > 1 (an extension): z <- z - (t_i - t_{i+1}) * model(z, t_i, t_{i+1}) on t_i = 1 - i / S.
        Returns [B, channels, H, W] (unclipped, as the reference), or [S + 1, B, ...] of every state with return_all."""
        if num_steps < 1 or batch_size < 1:
            raise ValueError("sample: num_steps and batch_size must be >= 1")
        device = self.device if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("MeanFlow.sample: the MFEfficientUNet forward runs on the GPU kernels only "
                               f"(device {device}); there is no CPU path")
        B, S = batch_size, num_steps
        tg = self.time_grid(S)
        dts = (tg[:-1] - tg[1:])[:, None].expand(S, B).contiguous().to(device)        # [S, B]
        t_rows = tg[:-1, None].expand(S, B).reshape(-1).to(device)
        r_rows = tg[1:, None].expand(S, B).reshape(-1).to(device)
        tf_all = self.model.time_features(t_rows, r_rows)                             # every step's, once

        def run():
            z = self._noise(B, rng, device)
            states = [z.clone()] if return_all else None
            for i in range(S):
                tf = tuple(a[i * B:(i + 1) * B] for a in tf_all)
                u = self.model(z, tg[i], tg[i + 1], time_features=tf)
                z = K.flow_step(z, u, dts[i], out=None if return_all else z)
                if return_all:
                    states.append(z)
            return torch.stack(states) if return_all else z

        # the conv range records are polled once, after the run (ops.run_range_safe)
        return K.run_range_safe(run, rng, device, "MeanFlow.sample")
