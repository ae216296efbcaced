"""Diffusion over per-object layout vectors -- API mirror of the reference's
lidargen/models/diffusion/continuous_layout_cond.py:9-191 (`CondContinuousLayoutGaussianDiffusion`): the first stage of
the LiDARCrafter pipeline, scene graph -> one 20-vector (box + trajectory code) per object.  x is [O, 20] with O the
objects of all scenes of the batch; denoiser `UNet1DModel`, condition model `SceneGraph`.

Differences from the reference, all on purpose:
  * `sample()` and `forward()` work on a shallow copy of the caller's dict (the reference overwrites
    `batch_dict['scenegraph_input']` with a tuple, so a second call on the same dict fails there);
  * the sampling loop keeps everything on the device: the schedule is tabulated once on the host, the denoiser runs on
    one plan of preallocated buffers (`UNet1DModel.make_plan`), step 1 is captured into a HIP graph that the remaining
    steps replay, the update is the fused lc_pstep_fwd; the graph lives for ONE call (O, T and the edge lists change with
    every batch).  The replayed step allocates nothing.  What the host does around it per step is not allocation-free:
    the DDPM noise goes through base.randn like in the other samplers (with per-object CPU generators: O draws of 20
    numbers into a pinned ring, one upload into a caching-allocator tensor, one copy into the graph's static buffer) --
    drawing all S x O x 20 values before the loop would put S x O tiny host draws in front of the first step instead of
    next to the running GPU, and one randn of [S, 20] per generator is not the same numbers as S draws of 20 -- and two
    small device copies move the step's log-SNR and coefficient row into the static buffers the graph reads;
  * the reference's `torch.isnan(...).any()` probes (a host synchronisation per attention layer) are not reproduced;
  * training is not built: a grad-mode forward raises NotImplementedError."""
from __future__ import annotations

from typing import Literal

import torch
from tqdm.auto import tqdm

from lidarcrafter_amd import ops as K

from . import schedules
from .continuous_time_cond import CondContinuousTimeGaussianDiffusion


class CondContinuousLayoutGaussianDiffusion(CondContinuousTimeGaussianDiffusion):
    @torch.no_grad()
    def get_scenegraph_input(self, batch):
        """The collated `scenegraph_input` dict -> the 13-tuple `SceneGraph.forward` takes, on this sampler's device."""
        dev = self.device
        enc, dec = batch["encoder"], batch["decoder"]
        return (enc["objs"].to(dev), enc["tripltes"].to(dev), enc["text_feats"].to(dev), enc["rel_feats"].to(dev),
                dec["objs"].to(dev), dec["tripltes"].to(dev), dec["boxes"].to(dev), dec["text_feats"].to(dev),
                dec["rel_feats"].to(dev), dec["obj_to_scene"], dec["triple_to_scene"], batch["missing_nodes"],
                batch["manipulated_subs"] + batch["manipulated_objs"])

    def q_step_from_x_0(self, x_0, step_t, rng=None):
        noise = self.randn_like(x_0, rng=rng)
        alpha, sigma = schedules.alpha_sigma(self.log_snr(step_t))
        return x_0 * alpha[:, :, 0, 0] + noise * sigma[:, :, 0, 0], noise

    def sample_timesteps(self, batch_size: int, sample_ids, device) -> torch.Tensor:
        """One t per scene, shared by its objects."""
        scenes, inv = torch.unique(torch.as_tensor(sample_ids), return_inverse=True)
        t = torch.rand(scenes.shape[0], device=device, dtype=torch.float32)
        return t[inv.to(device)]

    def prepare_df_input(self, triples, obj_embed, relation_cond, scene_ids=None, obj_boxes=None):
        return {"preds": triples, "box": obj_boxes, "uc_b": obj_embed, "c_b": relation_cond,
                "obj_id_to_scene": scene_ids}

    def get_network_condition(self, steps=None, input_dict=None, only_custom_condition=False):
        sg = input_dict["scenegraph_input"]
        latent_obj_vecs, obj_embed_ = self.condition_model(*sg)
        other = self.prepare_df_input(sg[5], obj_embed_, obj_boxes=input_dict["x_0"], relation_cond=latent_obj_vecs,
                                      scene_ids=sg[9])
        if only_custom_condition:
            return dict(other_condition=other)
        return dict(time_condition=self.log_snr(steps)[:, 0, 0, 0], other_condition=other)

    def _training_refused(self):
        from lidargen.models.unets.unet_1d import TRAINING_MSG

        mods = [m for m in (self.model, self.condition_model) if isinstance(m, torch.nn.Module)]
        if torch.is_grad_enabled() and any(p.requires_grad for m in mods for p in m.parameters()):
            raise NotImplementedError(TRAINING_MSG)

    def p_loss(self, input_dict: dict, steps, loss_mask=None):
        self._training_refused()
        x_0 = input_dict["x_0"]
        loss_mask = torch.ones_like(x_0) if loss_mask is None else loss_mask
        x_t, noise = self.q_step_from_x_0(x_0, steps)
        with torch.no_grad():
            condition = self.get_network_condition(steps, input_dict)
            prediction = self.model(x_t, condition)
        return self._masked_loss(prediction, self.get_target(x_0, steps, noise), loss_mask, steps)

    def forward(self, input_dict: dict, loss_mask=None):
        self._training_refused()
        sg = self.get_scenegraph_input(input_dict["scenegraph_input"])
        x_0, loss_mask = sg[6][:, :20], sg[6][:, 20:]
        work = dict(input_dict, x_0=x_0, scenegraph_input=sg)          # the caller's dict stays as it was
        steps = self.sample_timesteps(x_0.shape[0], sg[9], x_0.device)
        return self.p_loss(work, steps, loss_mask)

    @staticmethod
    def _rows4(x):
        return x.reshape(x.shape[0], 1, 1, x.shape[-1])

    @torch.compiler.disable
    @torch.inference_mode()
    def p_step(self, x_t, condition_dict: dict, step_t, step_s, rng=None, mode: Literal["ddpm", "ddim"] = "ddpm",
               ddim_eta: float = 0.0):
        if mode not in schedules.MODES:
            raise ValueError(f"invalid mode {mode}")
        lam_t = self._schedule(step_t.float().cpu())
        lam_s = self._schedule(step_s.float().cpu())
        coef = schedules.step_coefficients(lam_t, lam_s, mode, ddim_eta, self._clip())
        condition_dict.update(dict(time_condition=lam_t.to(x_t.device)))      # mutates, like the reference
        pred = self.model(x_t, condition_dict)
        noise = self._noise_for(x_t, rng, mode, ddim_eta)
        y = K.pstep(self._rows4(x_t.float().contiguous()), self._rows4(pred),
                    None if noise is None else self._rows4(noise.contiguous()), coef.to(x_t.device),
                    self._objective_id(), schedules.MODES[mode])
        return y.reshape(x_t.shape)

    @torch.inference_mode()
    def sample(self, batch_dict: dict, num_steps: int, progress: bool = True, rng=None, return_all: bool = False,
               mode: Literal["ddpm", "ddim"] = "ddpm", ddim_eta: float = 0.0):
        if mode not in schedules.MODES:
            raise ValueError(f"invalid mode {mode}")
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("CondContinuousLayoutGaussianDiffusion.sample: the sampler must live on a CUDA(HIP) "
                               "device -- the hot path has no CPU fallback")
        sg = self.get_scenegraph_input(batch_dict["scenegraph_input"])
        x_0 = sg[6][:, :20]
        work = dict(batch_dict, x_0=x_0, scenegraph_input=sg)           # the caller's dict stays as it was
        O = x_0.shape[0]
        x_T = self.randn(O, *self.sampling_shape, rng=rng, device=dev).squeeze(-1)
        cond = self.get_network_condition(input_dict=work, only_custom_condition=True)
        other = cond["other_condition"]
        self.model._guard(x_T)
        with torch.cuda.device(dev):
            plan = self.model.make_plan(other["uc_b"].float(), other["preds"], 1, None)
            lam = self._schedule(torch.linspace(1.0, 0.0, num_steps + 1))
            coef = schedules.step_coefficients(lam[:-1], lam[1:], mode, ddim_eta, self._clip()).to(dev)   # [S, 8]
            lam_d = lam[:-1].contiguous().to(dev)
            coef_rows = torch.empty((O, 8), device=dev, dtype=torch.float32)
            needs_noise = mode == "ddpm" or ddim_eta != 0.0
            noise_buf = torch.empty((O, 20), device=dev, dtype=torch.float32) if needs_noise else None
            plan.x.copy_(x_T)
            x4 = self._rows4(plan.x)
            obj, mid = self._objective_id(), schedules.MODES[mode]
            st = {"x": plan.x, "rng": rng}

            def body():
                plan.run()
                K.pstep(x4, self._rows4(plan.y), None if noise_buf is None else self._rows4(noise_buf), coef_rows, obj,
                        mid, out=x4)

            graph = None
            out = [x_T.clone()] if return_all else None
            for i in tqdm(range(num_steps), desc="sampling", leave=False, disable=not progress):
                noise = self._noise_for(plan.x, rng, mode, ddim_eta, st)
                plan.t.copy_(lam_d[i:i + 1])
                coef_rows.copy_(coef[i].expand(O, 8))
                if noise_buf is not None:
                    noise_buf.copy_(noise)
                if graph is None and i == 1 and self.use_hip_graph and K.PROFILE is None and num_steps > 2:
                    graph = torch.cuda.CUDAGraph()         # step 0 ran eagerly: code objects loaded, weights packed
                    with torch.cuda.graph(graph):
                        body()
                    graph.replay()
                elif graph is not None:
                    graph.replay()
                else:
                    body()
                if return_all:
                    out.append(plan.x.clone())
            self.finish_sampling(st)
            return torch.stack(out) if return_all else plan.x.clone()
