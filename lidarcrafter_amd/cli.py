"""Sampling harness with the reference CLI's flags (tools/generate/generate.py:92-102 and the bulk
sampler tools/evaluation/sample_and_save_cond.py): `--cfg --ckpt --device --mode --batch_size
--sampling_steps`.

  python -m lidarcrafter_amd.cli --cfg nuscenes-unet-uncond --batch_size 8 --sampling_steps 50 \
         --mode ddim --out samples/
  torchrun --nproc-per-node 8 -m lidarcrafter_amd.cli --cfg nuscenes-box-layout-v6 ...

Without --ckpt (no checkpoints ship with the reference, README.md:62) the weights are the seeded
random initialisation used by the tests.  Layout-conditioned configs take a synthetic layout batch
(lidarcrafter_amd.testing.synth_layout_batch) unless --batch_pt points to a saved batch dict.
`--cfg meanflow-nusc` samples the MeanFlow generator (inference.setup_model_flow's model) in `--flow_steps` network
calls (default 1: the reference's one-step `z - model(z, 1, 0)`); `--mode` / `--sampling_steps` do not apply to it, and
it runs on rank 0 alone (the data-parallel helper drives the diffusion samplers' interface).
`--cfg nuscenes-layout` samples the scene-graph layout generator on `--batch_size` synthetic scenes
(lidarcrafter_amd.testing.synth_scene_graph_batch with its synthetic vocabulary and stand-in CLIP features, or the
collated batch dict of --batch_pt, whose `vocab` entry is then required) on rank 0 and writes `<out>/layout_boxes.pt` =
{"boxes": float32 [O, 20], "obj_to_scene": int64 [O]}.
Output per rank-0: `<out>/samples.pt` = float32 [N,5,H,W] (metric depth, x, y, z, reflectance), the
tensor sample_and_save_cond.py:119-124,157-159 saves per sample."""
from __future__ import annotations

import argparse
import os
import time

import torch


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfg", default="nuscenes-unet-uncond")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--mode", choices=["ddpm", "ddim"], default="ddim")
    ap.add_argument("--batch_size", type=int, default=8, help="GLOBAL batch (sharded over ranks)")
    ap.add_argument("--sampling_steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch_pt", default=None, help="torch-saved layout batch dict (cond configs)")
    ap.add_argument("--out", default="samples")
    ap.add_argument("--flow_steps", type=int, default=1, help="network calls of a flow generator (meanflow-nusc)")
    args = ap.parse_args(argv)

    import torch.distributed as dist

    from lidarcrafter_amd import parallel
    from lidarcrafter_amd.testing import seeded_fill, seeded_fill_qk_gains, synth_layout_batch
    from lidargen.utils import inference
    from lidargen.utils.configs import __all__ as CONFIGS

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    # under torchrun (RANK / WORLD_SIZE exported) the process group is created for ONE rank too: the same RCCL
    # init / all-gather path runs on a single-GPU box as on the 8-GPU node (tests/test_rccl_single_gpu.py)
    dist_on = world > 1 or ("RANK" in os.environ and "WORLD_SIZE" in os.environ and args.device == "cuda")
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    device = torch.device(args.device, torch.cuda.current_device()) if args.device == "cuda" \
        else torch.device(args.device)

    cfg = CONFIGS[args.cfg]()
    cfg.resume = args.ckpt
    if cfg.model.architecture == "unet_1d":
        _sample_layout_gen(args, cfg, inference, device, rank)
        if dist_on:
            dist.destroy_process_group()
        return
    if hasattr(cfg, "flow"):
        _sample_flow(args, cfg, inference, device, rank, world, seeded_fill, seeded_fill_qk_gains)
        if dist_on:
            dist.destroy_process_group()
        return
    built = inference.load_model_duffusion_training(cfg)
    ddpm, model, lidar_utils = built[:3]
    if args.ckpt is None:
        seeded_fill(ddpm, salt=100)
    ddpm, lidar_utils = ddpm.eval().to(device), lidar_utils.to(device)

    shard = parallel.shard_range(args.batch_size, rank, world)
    batch = None
    if hasattr(cfg, "condition_model"):
        H, W = cfg.data.resolution
        if args.batch_pt:
            full = torch.load(args.batch_pt, map_location="cpu")
        else:
            extra = cfg.condition_model.params["out_channels"] - 10
            full = synth_layout_batch(args.batch_size, H, W, seed=args.seed, n_extra=extra)
        batch = {k: v[shard.start:shard.stop].to(device) for k, v in full.items()}
    t0 = time.perf_counter()
    frames = parallel.sample_data_parallel(ddpm, args.batch_size, args.sampling_steps,
                                           batch_dict=batch, mode=args.mode, base_seed=args.seed,
                                           gather=False)
    out = lidar_utils.postprocess(frames.clamp(-1, 1))          # [b,5,H,W] fused epilogue
    out = parallel.gather_frames(out, args.batch_size)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rank == 0:
        os.makedirs(args.out, exist_ok=True)
        torch.save(out.cpu(), os.path.join(args.out, "samples.pt"))
        print(f"{args.cfg}: {out.shape[0]} frames, {args.sampling_steps} {args.mode} steps, "
              f"{dt:.2f} s ({args.sampling_steps / dt:.1f} denoising-steps/s) -> {args.out}/samples.pt")
    if dist_on:
        dist.destroy_process_group()


def _sample_layout_gen(args, cfg, inference, device, rank):
    """Scene-graph layout generator: one `sample()` over all scenes of the batch on rank 0."""
    if rank != 0:
        return
    from lidarcrafter_amd.testing import LAYOUT_GEN_VOCAB, seeded_fill, seeded_fill_layout_gen, synth_scene_graph_batch

    if args.batch_pt:
        batch = torch.load(args.batch_pt, map_location="cpu")
        if "vocab" not in batch:
            raise SystemExit("--batch_pt for nuscenes-layout must hold the dataset's `vocab` next to `scenegraph_input`")
        cfg.condition_model.params["vocab"] = batch["vocab"]
    else:
        batch = synth_scene_graph_batch(args.batch_size, seed=args.seed, manipulate=True)
        cfg.condition_model.params["vocab"] = LAYOUT_GEN_VOCAB
    ddpm = inference.load_model_layout_duffusion_training(cfg)[0]
    if args.ckpt is None:
        seeded_fill(ddpm, salt=100)
        seeded_fill_layout_gen(ddpm, salt=100)
    ddpm = ddpm.eval().to(device)
    dec = batch["scenegraph_input"]["decoder"]
    rng = [torch.Generator().manual_seed(args.seed + i) for i in range(dec["objs"].numel())]
    t0 = time.perf_counter()
    boxes = ddpm.sample({"scenegraph_input": batch["scenegraph_input"]}, args.sampling_steps, progress=False, rng=rng,
                        mode=args.mode)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    os.makedirs(args.out, exist_ok=True)
    torch.save({"boxes": boxes.cpu(), "obj_to_scene": dec["obj_to_scene"].cpu()}, os.path.join(args.out, "layout_boxes.pt"))
    print(f"{args.cfg}: {boxes.shape[0]} objects / {dec['tripltes'].shape[0]} triples in {args.batch_size} scenes, "
          f"{args.sampling_steps} {args.mode} steps, {dt:.2f} s ({args.sampling_steps / dt:.1f} denoising-steps/s) -> "
          f"{args.out}/layout_boxes.pt")


def _sample_flow(args, cfg, inference, device, rank, world, seeded_fill, seeded_fill_qk_gains):
    """Flow generators (MeanFlow): `flow_steps` network calls on rank 0, the same samples.pt layout."""
    if rank != 0:
        return
    if world > 1:
        print(f"{args.cfg}: the flow generator samples on rank 0 only ({world} ranks launched)")
    flow, model, lidar_utils = inference.load_model_flow_training(cfg)[:3]
    if args.ckpt is None:
        seeded_fill(flow, salt=100)
        seeded_fill_qk_gains(flow, salt=100)
    flow, lidar_utils = flow.eval().to(device), lidar_utils.to(device)
    rng = [torch.Generator().manual_seed(args.seed + i) for i in range(args.batch_size)]
    t0 = time.perf_counter()
    frames = flow.sample(device, batch_size=args.batch_size, num_steps=args.flow_steps, rng=rng)
    out = lidar_utils.postprocess(frames.clamp(-1, 1))          # [B,5,H,W] fused epilogue
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    os.makedirs(args.out, exist_ok=True)
    torch.save(out.cpu(), os.path.join(args.out, "samples.pt"))
    print(f"{args.cfg}: {out.shape[0]} frames, {args.flow_steps} flow step(s), {dt * 1e3:.1f} ms -> "
          f"{args.out}/samples.pt")


if __name__ == "__main__":
    main()
