"""Generate tests/golden/layout_gen.npz from the reference's scene-graph layout generator (CPU, this container only).

    python tests/golden/make_layout_gen_fixtures.py

The reference modules are imported through the namespace stubs of _ref_import.py plus two shims of this file: a stub
`omegaconf.listconfig` (UNet1DModel.__init__ imports it only to test a type) and `Tensor.cuda -> self` (SceneGraph
hard-codes `.cuda()`; _ref_import installs it).  Weights come from lidarcrafter_amd.testing.seeded_fill +
seeded_fill_layout_gen, inputs from synth_scene_graph_batch, so the file holds OUTPUTS and key lists only.  Every float32
output has a float64 twin (`*_f64`, the same modules after `.double()`) and `ref_err_*`, the relative L2 deviation of
the float32 output from it.  The float64 run keeps the reference's float32 sinusoidal embedding (nn.py casts the time to
float32 on purpose); only what follows it is double."""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import as R  # noqa: E402
from lidarcrafter_amd.testing import (LAYOUT_GEN_VOCAB, rel_l2, seeded_fill, seeded_fill_layout_gen,  # noqa: E402
                                      seeded_randn, synth_scene_graph_batch)

SALT = 11
UNET = dict(dims=1, in_channels=20, out_channels=20, model_channels=512, channel_mult=[1, 1, 1, 1], num_res_blocks=2,
            attention_resolutions=[4, 2], num_heads=8, use_spatial_transformer=True, transformer_depth=1,
            conditioning_key="crossattn", concat_dim=1280, crossattn_dim=1280, use_checkpoint=True, enable_t_emb=True)
COND = dict(embedding_dim=64, gconv_pooling="avg", gconv_num_layers=5, mlp_normalization="batch", separated=True,
            replace_latent=True, residual=True, use_angles=True, use_clip=True, vocab=LAYOUT_GEN_VOCAB)


def main():
    torch.set_grad_enabled(False)
    R.install()
    R._PKGS.append("lidargen.models.diffusion")
    m = types.ModuleType("lidargen.models.diffusion")
    m.__path__ = [R.REF + "/lidargen/models/diffusion"]
    sys.modules["lidargen.models.diffusion"] = m
    oc, lc = types.ModuleType("omegaconf"), types.ModuleType("omegaconf.listconfig")
    lc.ListConfig = type("ListConfig", (), {})
    oc.listconfig = lc
    sys.modules["omegaconf"], sys.modules["omegaconf.listconfig"] = oc, lc

    U = R.ref("models.unets.unet_1d")
    SG = R.ref("models.unets.scene_graph")
    DF = R.ref("models.diffusion.continuous_layout_cond")
    GN32 = R.ref("models.unets.ldm_diffusion_util").GroupNorm32
    gn32_forward = GN32.forward

    model = U.UNet1DModel(**UNET)
    cond = SG.SceneGraph(**COND)
    ddpm = DF.CondContinuousLayoutGaussianDiffusion(model=model, condition_model=cond, loss_type="l2",
                                                    prediction_type="eps", noise_schedule="cosine", clip_sample=False)
    seeded_fill(ddpm, salt=SALT)
    seeded_fill_layout_gen(ddpm, salt=SALT)
    ddpm.eval()
    ddpm64 = copy.deepcopy(ddpm).double().eval()
    orig_te = U.timestep_embedding

    out = {"state_dict_keys": np.array(sorted(f"{k}:{tuple(v.shape)}" for k, v in ddpm.state_dict().items()))}

    def both(name, fn):
        """fn(ddpm, cast) -> tensor; run in float32 and float64."""
        a = fn(ddpm, lambda t: t)
        U.timestep_embedding = lambda *x, **k: orig_te(*x, **k).double()
        GN32.forward = torch.nn.GroupNorm.forward          # (GroupNorm32 casts its input to float32)
        try:
            b = fn(ddpm64, lambda t: t.double() if t.is_floating_point() else t)
        finally:
            U.timestep_embedding, GN32.forward = orig_te, gn32_forward
        out[name] = a.float().numpy()
        out[name + "_f64"] = b.numpy()
        out["ref_err_" + name] = np.float64(rel_l2(a, b))
        print(f"ref_err_{name} = {rel_l2(a, b):.3e}   |y| = {float(b.abs().mean()):.3e}")

    def sg_tuple(d, batch, cast):
        t = d.get_scenegraph_input(copy.deepcopy(batch["scenegraph_input"]))
        return tuple(cast(x) if isinstance(x, torch.Tensor) else x for x in t)

    plain = synth_scene_graph_batch(3, seed=1)
    manip = synth_scene_graph_batch(3, seed=2, manipulate=True)

    def scene_graph(batch, which, seed=None):
        def fn(d, cast):
            if seed is not None:
                np.random.seed(seed)
            return d.condition_model(*sg_tuple(d, batch, cast))[which]
        return fn

    both("sg_plain_latent", scene_graph(plain, 0))
    both("sg_plain_embed", scene_graph(plain, 1))
    both("sg_manip_latent", scene_graph(manip, 0, seed=5))
    both("sg_manip_embed", scene_graph(manip, 1, seed=5))

    def unet_forward(batch, times_of_scene, x_seed):
        def fn(d, cast):
            sg = sg_tuple(d, batch, cast)
            np.random.seed(5)
            lat, emb = d.condition_model(*sg)
            O = emb.shape[0]
            x = cast(seeded_randn(O, 20, seed=x_seed))
            t = cast(torch.tensor(times_of_scene, dtype=torch.float32)[sg[9]])
            other = d.prepare_df_input(sg[5], emb, relation_cond=lat, scene_ids=sg[9], obj_boxes=None)
            return d.model(x, dict(time_condition=t, other_condition=other))
        return fn

    both("unet_uniform", unet_forward(plain, [0.7, 0.7, 0.7], 31))
    both("unet_per_scene", unet_forward(manip, [-3.0, 0.4, 5.5], 32))

    # (c) a single object with its self-loop triple only
    def single(d, cast):
        emb = cast(seeded_randn(1, 640, seed=33))
        other = d.prepare_df_input(torch.tensor([[0, 3, 0]]), emb, relation_cond=None)
        return d.model(cast(seeded_randn(1, 20, seed=34)), dict(time_condition=cast(torch.tensor([1.25])),
                                                                 other_condition=other))

    both("unet_single", single)

    # the graph network alone (box_graph_cov shapes)
    def gcn(d, cast):
        sg = sg_tuple(d, plain, cast)
        O, T = sg[4].shape[0], sg[5].shape[0]
        obj, pred = cast(seeded_randn(O, 768, seed=35)), cast(seeded_randn(T, 128, seed=36))
        return d.model.box_graph_cov(obj, pred, torch.stack([sg[5][:, 0], sg[5][:, 2]], dim=1))[0]

    both("gcn", gcn)

    # single torso modules at the shipped widths, O = 7 rows (the keys name the module in the state_dict):
    # a ResBlock with a 1x1 skip conv on the 1024-channel [h | skip] concatenation, a SpatialTransformer1D, the stride-2
    # Downsample conv and the Upsample (interpolate(scale_factor=1) + conv)
    MO = 7

    def module(path, args):
        def fn(d, cast):
            mod = d.model.get_submodule(path)
            return mod(*[cast(a) for a in args])[:, :, 0]
        return fn

    both("mod_resblock", module("output_blocks.0.0", [seeded_randn(MO, 1024, 1, seed=51), seeded_randn(MO, 2048, seed=52)]))
    both("mod_transformer", module("input_blocks.4.1", [seeded_randn(MO, 512, 1, seed=53), seeded_randn(MO, 1, 1280, seed=54)]))
    both("mod_downsample", module("input_blocks.3.0", [seeded_randn(MO, 512, 1, seed=55)]))
    both("mod_upsample", module("output_blocks.2.1", [seeded_randn(MO, 512, 1, seed=56)]))

    # p_step, trajectory and loss.  The float64 twin keeps every random draw and the schedule in float32 (the sampler
    # draws float32 noise and float32 log-SNR values; a float64 draw would be other numbers), the network is double.
    def cond_of(d, cast):
        b = copy.deepcopy(manip)
        sg = tuple(cast(x) if isinstance(x, torch.Tensor) else x for x in d.get_scenegraph_input(b["scenegraph_input"]))
        b["x_0"], b["scenegraph_input"] = sg[6][:, :20], sg
        np.random.seed(5)
        return d.get_network_condition(input_dict=b, only_custom_condition=True), b

    O = manip["scenegraph_input"]["decoder"]["objs"].numel()
    x_t = seeded_randn(O, 20, seed=41)
    f32_randn, f32_randn_like = ddpm.randn, ddpm.randn_like
    ddpm64.randn = lambda *a, **k: f32_randn(*a, **k).double()
    ddpm64.randn_like = lambda x, rng=None: f32_randn_like(x.float(), rng=rng).double()
    for mode in ("ddpm", "ddim"):
        def pstep(d, cast, mode=mode):
            cd, _ = cond_of(d, cast)
            rng = [torch.Generator().manual_seed(500 + i) for i in range(O)]
            return d.p_step(cast(x_t.clone()), cd, torch.full((O,), 0.6), torch.full((O,), 0.5), rng=rng, mode=mode)

        def traj(d, cast, mode=mode):
            rng = [torch.Generator().manual_seed(700 + i) for i in range(O)]
            b = copy.deepcopy(manip)
            for side in ("encoder", "decoder"):
                b["scenegraph_input"][side] = {k: cast(v) for k, v in b["scenegraph_input"][side].items()}
            np.random.seed(5)
            return d.sample(b, 8, progress=False, rng=rng, return_all=True, mode=mode)

        both(f"pstep_{mode}", pstep)
        both(f"traj_{mode}", traj)
    # eval-mode loss with fixed t per scene and fixed noise
    noise = seeded_randn(O, 20, seed=42)

    def loss(d, cast):
        _, b = cond_of(d, cast)
        steps = torch.tensor([0.2, 0.55, 0.9])[b["scenegraph_input"][9]]
        d.randn_like = lambda x, rng=None: cast(noise.clone())
        np.random.seed(5)
        return d.p_loss(b, steps, b["scenegraph_input"][6][:, 20:])

    both("loss", loss)
    np.savez_compressed(os.path.join(HERE, "layout_gen.npz"), **out)
    print("wrote layout_gen.npz", os.path.getsize(os.path.join(HERE, "layout_gen.npz")), "bytes")


if __name__ == "__main__":
    main()
