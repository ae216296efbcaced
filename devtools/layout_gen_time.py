"""Layout generator timing, one process, one JSON line per batch size (profiles/layout_gen.txt):
  * one denoiser step of the HIP path as a replayed HIP graph, and its sections (time path, graph network, ResBlocks,
    transformer blocks) as graphs of their own;
  * the yardstick: the SAME module tree evaluated module by module with plain torch ops on the same device (full
    3-tap convolutions, attention with its softmax, BatchNorm, index_add pooling -- what running the reference's
    arithmetic through PyTorch costs), eager and under torch.cuda.graph;
  * a whole 256-step DDPM `sample()`;
  * one alternative of the decomposition: the step with `to_out . to_v` of the attention folded at pack time
    (unet_1d.FOLD_ATTENTION_VALUE), its launch count and its deviation from the default step.
python devtools/layout_gen_time.py [reps]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidarcrafter_amd.testing import (LAYOUT_GEN_VOCAB, rel_l2, seeded_fill, seeded_fill_layout_gen,  # noqa: E402
                                      seeded_randn, synth_scene_graph_batch)
from lidargen.models.unets.unet_1d import (Downsample, ResBlock, SpatialTransformer1D, Upsample,  # noqa: E402
                                           timestep_freqs)
from lidargen.utils import inference  # noqa: E402
from lidargen.utils.configs import __all__ as CONFIGS  # noqa: E402

F = torch.nn.functional


def torch_forward(m, x, t, uc_b, triples, freqs):
    """UNet1DModel module by module with torch ops (nothing packed, nothing skipped); freqs: timestep_freqs on the device."""
    a = t[:, None] * freqs[None]
    emb = m.time_embed(torch.cat([a.cos(), a.sin()], -1))
    s, p, o = triples[:, 0], triples[:, 1], triples[:, 2]
    obj = torch.cat([uc_b, m.box_embeddings(x), m.box_time_emb(emb)], 1)
    ctx = m.box_graph_cov(obj, m.pred_embeddings(p), torch.stack([s, o], 1))[0][:, None]

    def attn(ca, q_in, c):
        B, h = q_in.shape[0], ca.heads
        q, k, v = [z.reshape(B, z.shape[1], h, -1).transpose(1, 2) for z in (ca.to_q(q_in), ca.to_k(c), ca.to_v(c))]
        w = (q @ k.transpose(-1, -2) * ca.scale).softmax(-1)
        return ca.to_out((w @ v).transpose(1, 2).reshape(B, q_in.shape[1], -1))

    def res(b, h):
        y = b.in_layers(h) + b.emb_layers(emb)[..., None]
        return b.skip_connection(h) + b.out_layers(y)

    def st(sp, h):
        z = sp.proj_in(sp.norm(h)).transpose(1, 2)
        for blk in sp.transformer_blocks:
            n = blk.norm1(z)
            z = attn(blk.attn1, n, n) + z
            z = attn(blk.attn2, blk.norm2(z), ctx) + z
            a_, g_ = blk.ff.net[0].proj(blk.norm3(z)).chunk(2, -1)
            z = blk.ff.net[2](a_ * F.gelu(g_)) + z
        return sp.proj_out(z.transpose(1, 2)) + h

    def run(seq, h):
        for layer in seq:
            if isinstance(layer, ResBlock):
                h = res(layer, h)
            elif isinstance(layer, SpatialTransformer1D):
                h = st(layer, h)
            elif isinstance(layer, Downsample):
                h = layer.op(h)
            elif isinstance(layer, Upsample):
                h = layer.conv(h)
            else:
                h = layer(h)
        return h

    hs, h = [], x[:, :, None]
    for seq in m.input_blocks:
        h = run(seq, h)
        hs.append(h)
    h = run(m.middle_block, h)
    for seq in m.output_blocks:
        h = run(seq, torch.cat([h, hs.pop()], 1))
    return m.out(h)[:, :, 0]


def timed(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    dev = torch.device("cuda:0")
    cfg = CONFIGS["nuscenes-layout"]()
    cfg.condition_model.params["vocab"] = LAYOUT_GEN_VOCAB
    ddpm, model = inference.load_model_layout_duffusion_training(cfg)
    seeded_fill(ddpm, salt=100)
    seeded_fill_layout_gen(ddpm, salt=100)
    ddpm = ddpm.eval().to(dev)
    for n_scenes in (1, 8, 32):
        batch = synth_scene_graph_batch(n_scenes, seed=0, manipulate=True)
        with torch.inference_mode():
            sg = ddpm.get_scenegraph_input(batch["scenegraph_input"])
            np.random.seed(5)
            _, uc_b = ddpm.condition_model(*sg)
            O, T = uc_b.shape[0], sg[5].shape[0]
            x, t = seeded_randn(O, 20, seed=1).to(dev), torch.full((O,), 0.7, device=dev)
            plan = model.make_plan(uc_b, sg[5])
            P = plan.P
            plan.x.copy_(x), plan.t.copy_(t[:1])
            out = {"scenes": n_scenes, "O": O, "T": T, "reps": reps}
            g = capture(plan.run)
            out["hip_step_graph_ms"] = round(timed(g.replay, reps), 4)
            out["hip_step_eager_ms"] = round(timed(plan.run, reps), 4)
            y_hip = plan.y.clone()
            freqs = timestep_freqs(model.model_channels).to(dev)
            ref = lambda: torch_forward(model, x, t, uc_b, sg[5], freqs)  # noqa: E731
            out["hip_vs_torch_rel_l2"] = float(f"{rel_l2(y_hip, ref()):.3e}")
            out["torch_step_eager_ms"] = round(timed(ref, reps), 4)
            try:
                gt = capture(ref)
                out["torch_step_graph_ms"] = round(timed(gt.replay, reps), 4)
            except Exception as e:  # noqa: BLE001
                out["torch_step_graph_ms"] = None
                out["torch_graph_error"] = repr(e)[:200]
            kinds = [op[0] for op in P.ops]
            out["hip_launches_per_step"] = 2 * kinds.count("gemm") + len(kinds) - kinds.count("gemm")
            full = plan.P
            for sec in ("time", "gcn", "res", "attn", "io"):
                sub = type(full)()
                sub.ops, sub.bufs, sub.w = [op for op, tg in zip(full.ops, full.tags) if tg == sec], full.bufs, full.w
                plan.P = sub
                gs = capture(plan.run)
                out[f"hip_{sec}_ms"] = round(timed(gs.replay, reps), 4)
                out[f"hip_{sec}_ops"] = len(sub.ops)
            plan.P = full
            from lidargen.models.unets import unet_1d as U1
            U1.FOLD_ATTENTION_VALUE = True
            try:
                plan2 = model.make_plan(uc_b, sg[5])
                plan2.x.copy_(x), plan2.t.copy_(t[:1])
                g2 = capture(plan2.run)
                out["hip_step_folded_attn_graph_ms"] = round(timed(g2.replay, reps), 4)
                k2 = [op[0] for op in plan2.P.ops]
                out["hip_folded_attn_launches"] = len(k2) + k2.count("gemm")
                out["folded_vs_default_rel_l2"] = float(f"{rel_l2(plan2.y, y_hip):.3e}")
                del plan2, g2
            finally:
                U1.FOLD_ATTENTION_VALUE = False
            model.packed()
            live = sum(w.numel() for k, w in P.w.items() if k not in ("pred_embeddings", "freqs")) * 4
            out["live_weight_mb"] = round(live / 1e6, 1)
            out["weight_stream_gbps"] = round(live / (out["hip_step_graph_ms"] * 1e-3) / 1e9, 1)
        rng = lambda: [torch.Generator().manual_seed(i) for i in range(O)]  # noqa: E731
        ddpm.sample(batch, 8, progress=False, rng=rng())
        ts = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ddpm.sample(batch, 256, progress=False, rng=rng())
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["sample_256_ddpm_ms"] = round(min(ts), 1)
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
