"""Deterministic synthetic weights / inputs shared by tests, bench and the fixture generator.

There are no pretrained checkpoints in this environment, and a freshly
constructed denoiser has 82 zero-initialised tensors (reference `ops.zero_out`
lidargen/models/unets/ops.py:9-11, `zero_module` nn.py:79-85) so it would output exactly 0.
`seeded_fill` therefore overwrites EVERY parameter with values that depend only on the
parameter's state_dict key and shape -- not on construction order or torch's global RNG --
so the reference modules (fixture generator) and this repo's modules get bit-identical
weights as long as their state_dict keys/shapes agree (which is itself the checkpoint contract).
"""
from __future__ import annotations

import zlib

import torch


def _gen_for(key: str, salt: int) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed((zlib.crc32(key.encode()) ^ (salt * 2654435761)) & 0x7FFFFFFF)
    return g


@torch.no_grad()
def seeded_fill(module: torch.nn.Module, salt: int = 0) -> torch.nn.Module:
    """Fill all parameters of `module` in place, keyed by their state_dict name."""
    for key, p in module.named_parameters():
        g = _gen_for(key, salt)
        r = torch.randn(p.shape, generator=g, dtype=torch.float32)
        if p.ndim >= 2:
            fan_in = max(1, p.numel() // p.shape[0])
            v = r / fan_in ** 0.5
        elif key.endswith("weight"):  # norm gains
            v = 1.0 + 0.1 * r
        else:  # biases
            v = 0.1 * r
        p.copy_(v.to(device=p.device, dtype=p.dtype))
    return module


@torch.no_grad()
def seeded_fill_qk_gains(module: torch.nn.Module, salt: int = 0) -> torch.nn.Module:
    """Give the q / k RMSNorm gains of MFEfficientUNet (`...q_norm.g`, `...k_norm.g`) magnitudes in [1.5, 2.5] with
    mixed signs, keyed by their state_dict name; call after `seeded_fill`.  `seeded_fill` leaves them at about +-0.1
    (one-element parameters not named `weight`), where the attention scores are nearly flat and a wrong eps, scale or
    normalisation axis of the q / k normalisation barely shows in the output."""
    for key, p in module.named_parameters():
        if not key.endswith(("q_norm.g", "k_norm.g")):
            continue
        u = torch.rand(p.shape, generator=_gen_for(key, salt), dtype=torch.float32)
        sign = 1.0 if zlib.crc32(key.encode()) % 2 == 0 else -1.0
        p.copy_((sign * (1.5 + u)).to(device=p.device, dtype=p.dtype))
    return module


@torch.no_grad()
def seeded_fill_hdit(module: torch.nn.Module, salt: int = 0, clamped_heads: bool = True) -> torch.nn.Module:
    """The HDiT tensors `seeded_fill` leaves degenerate, keyed by their state_dict name; call after `seeded_fill`:
      * the attention logit scales (`...residual_attn.scale`, [heads, 1]) near ln 10, the reference's init, and the first
        head of every other block at 5.0 > ln 100, so the clamp at ln 100 matters (`clamped_heads=False`: not those);
      * the RMSNorm gains (1-D `...scale`) at 1 + 0.1 r;
      * the Fourier frequencies (buffer `timestep_pe.0.freqs`) a standard normal draw, as the reference's init;
      * the positional embedding at 0.1 r (seeded_fill's fan-in scaling would leave it at ~1e-3)."""
    for key, p in list(module.named_parameters()) + list(module.named_buffers()):
        r = torch.randn(p.shape, generator=_gen_for(key, salt), dtype=torch.float32)
        if key.endswith("residual_attn.scale"):
            v = 2.302585092994046 + 0.3 * r
            if clamped_heads and zlib.crc32(key.encode()) % 2 == 0:
                v[0] = 5.0
        elif key.endswith(".scale") and p.ndim == 1:
            v = 1.0 + 0.1 * r
        elif key.endswith("timestep_pe.0.freqs"):
            v = r
        elif key.endswith("spatial_pe.embedding"):
            v = 0.1 * r
        else:
            continue
        p.copy_(v.to(device=p.device, dtype=p.dtype))
    return module


def seeded_randn(*shape: int, seed: int) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def error_profiles(got: torch.Tensor, ref: torch.Tensor, keeps, min_elems: int = 64) -> dict:
    """Relative-L2 error of `got` against the float64 `ref`, resolved by slice.  A fault confined to n of N outputs is
    diluted by sqrt(n / N) in the whole-tensor figure; a profile along the axis that isolates it shows it undiluted.

    keeps: tuples of kept axes, e.g. ((0,), (1,), (2,), (3,), (2, 3)) = sample, channel, row, column, pixel map of
    [B, C, H, W].  For each, sqrt(sum err^2 / sum ref^2) with both sums over all OTHER axes: one figure per slice.
    Returns {"whole": float, "profiles": {keep: {"err": float64 tensor shaped like the kept axes, "worst": float,
    "index": index tuple of the worst slice, "median": float}}}.  A profile whose slices hold fewer than `min_elems`
    elements is refused (ValueError): below that the figure is noise, not a property of the kernel."""
    if ref.dtype != torch.float64:
        raise TypeError("error_profiles: the reference must be float64")
    ref = ref.detach().cpu()
    got = got.detach().double().cpu()
    if got.shape != ref.shape:
        raise ValueError(f"error_profiles: shapes differ, {tuple(got.shape)} against {tuple(ref.shape)}")
    e2, r2 = (got - ref) ** 2, ref ** 2
    out = {"whole": float((e2.sum() / r2.sum().clamp_min(1e-300)).sqrt()), "profiles": {}}
    for keep in keeps:
        keep = tuple(int(a) % ref.dim() for a in keep)
        if not keep or len(set(keep)) != len(keep) or list(keep) != sorted(keep):
            raise ValueError(f"error_profiles: kept axes {keep} must be distinct and ascending")
        n_slices = 1
        for a in keep:
            n_slices *= ref.shape[a]
        per = ref.numel() // max(1, n_slices)
        if per < min_elems:
            raise ValueError(f"error_profiles: slices of profile {keep} hold {per} < {min_elems} elements")
        rest = [a for a in range(ref.dim()) if a not in keep]
        num = e2.sum(rest) if rest else e2
        den = r2.sum(rest) if rest else r2
        err = (num / den).sqrt()                       # a zero-norm slice gives inf / nan: the caller's input is degenerate
        flat = torch.nan_to_num(err.reshape(-1), nan=float("inf"))
        i = int(flat.argmax())
        out["profiles"][keep] = {"err": err, "worst": float(flat[i]), "median": float(flat.median()),
                                 "index": tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))}
    return out


def synth_points(N: int, seed: int):
    """Synthetic LiDAR sweep: azimuth U(-pi,pi), elevation U(-30.5,10.5) deg,
    range log-U(0.8,95) m, intensity U(0,255) -> float32 [N,4]."""
    import numpy as np

    g = np.random.default_rng(seed)
    az = g.uniform(-np.pi, np.pi, N)
    el = np.deg2rad(g.uniform(-30.5, 10.5, N))
    r = np.exp(g.uniform(np.log(0.8), np.log(95.0), N))
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el),
                     g.uniform(0, 255, N)], axis=1).astype(np.float32)


def synth_layout_batch(B: int, H: int, W: int, seed: int, n_extra: int = 0) -> dict:
    """Synthetic layout-condition batch: 13 object slots,
    n_valid ~ U{1..12}; scaled 3-D boxes U(-1,1) with class id U{1..8} in the last column (0 for
    padding); sorted 2-D corners U(0,1); `concat_cond` [B,10,H,W] = one-hot(9) of a rasterised
    class map + one log-depth channel (the output of `preprocess_condition_mask`,
    tools/evaluation/sample_and_save_cond.py:106-117).  n_extra>0 adds `autoregressive_cond`."""
    import numpy as np

    g = np.random.default_rng(seed)
    boxes = np.zeros((B, 13, 9), np.float32)
    b2d = np.zeros((B, 13, 4), np.float32)
    valid = np.zeros((B, 13), np.float32)
    cls_map = np.zeros((B, H, W), np.int64)
    dep_map = np.zeros((B, H, W), np.float32)
    for b in range(B):
        n = int(g.integers(1, 13))
        valid[b, :n] = 1
        boxes[b, :n, :8] = g.uniform(-1, 1, (n, 8))
        boxes[b, :n, 8] = g.integers(1, 9, n)
        xs = np.sort(g.uniform(0, 1, (n, 2)), axis=1)
        ys = np.sort(g.uniform(0, 1, (n, 2)), axis=1)
        b2d[b, :n] = np.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], 1)
        for k in range(n):
            x0, x1 = int(xs[k, 0] * W), max(int(xs[k, 1] * W), int(xs[k, 0] * W) + 1)
            y0, y1 = int(ys[k, 0] * H), max(int(ys[k, 1] * H), int(ys[k, 0] * H) + 1)
            cls_map[b, y0:y1, x0:x1] = int(boxes[b, k, 8])
            dep_map[b, y0:y1, x0:x1] = g.uniform(2, 60)
    onehot = np.eye(9, dtype=np.float32)[cls_map].transpose(0, 3, 1, 2)
    logd = np.clip(np.log2(dep_map + 1) / np.log2(81.0), 0, 1) * ((dep_map > 1.45) & (dep_map < 80))
    out = {
        "scaled_gt_boxes": torch.from_numpy(boxes),
        "gt_boxes_2d": torch.from_numpy(b2d),
        "is_valid_obj": torch.from_numpy(valid),
        "concat_cond": torch.from_numpy(np.ascontiguousarray(
            np.concatenate([onehot, logd[:, None].astype(np.float32)], 1))),
    }
    if n_extra:
        out["autoregressive_cond"] = torch.from_numpy(
            g.uniform(0, 1, (B, n_extra, H, W)).astype(np.float32))
    return out


def synth_boxes(n: int, pts, seed: int):
    """n rotated boxes [x,y,z,dx,dy,dz,heading] centred on random points of `pts` (float32)."""
    import numpy as np

    g = np.random.default_rng(seed)
    bx = np.stack([np.zeros(n), np.zeros(n), np.zeros(n), g.uniform(1.5, 10, n),
                   g.uniform(1.5, 5, n), g.uniform(1.5, 4, n), g.uniform(-3.2, 3.2, n)],
                  1).astype(np.float32)
    bx[:, :3] = pts[g.integers(0, len(pts), n), :3]
    return bx


def synth_scene_boxes(n: int, seed: int):
    """n scene boxes float32 [n, 8] = (x, y, z, l, w, h, yaw, class 1..8) at 5-60 m range, one of
    them straddling the +-pi azimuth seam (exercises the wrap-around case of convert_boxes_to_2d)."""
    import numpy as np

    g = np.random.default_rng(seed)
    r = g.uniform(5, 60, n)
    az = g.uniform(-np.pi, np.pi, n)
    az[0] = np.pi - 0.01
    b = np.stack([r * np.cos(az), r * np.sin(az), g.uniform(-2.0, 0.5, n), g.uniform(1.5, 9, n),
                  g.uniform(1.2, 3, n), g.uniform(1.2, 3.5, n), g.uniform(-np.pi, np.pi, n),
                  g.integers(1, 9, n).astype(np.float64)], 1)
    return b.astype(np.float32)


def synth_temporal_inputs(seed=0, K=5, T=6):
    """Seeded inputs of the temporal glue: ego + K object per-step offsets, K boxes, a point set."""
    import numpy as np

    g = np.random.default_rng(seed)
    ego = np.stack([g.normal(0.05, 0.02, T), g.uniform(0.3, 1.2, T)], 1)      # mostly forward (+y)
    ego[2] = [0.01, 0.02]                                                      # a < 0.1 m step
    obj = g.normal(0.0, 0.6, (K, T, 2))
    obj[1] = 0.0                                                               # a standing object
    obj[2, 3] = 0.0                                                            # stops for one step
    trajs = np.concatenate([ego[None], obj], 0)                                # [1+K, T, 2] offsets
    r, az = g.uniform(6, 40, K), g.uniform(-np.pi, np.pi, K)
    boxes = np.stack([r * np.cos(az), r * np.sin(az), g.uniform(-1.5, 0.0, K), g.uniform(1.5, 6, K),
                      g.uniform(1.2, 2.5, K), g.uniform(1.2, 2.5, K), g.uniform(-np.pi, np.pi, K)], 1)
    return trajs, boxes


def synth_object_batch(B: int, seed: int) -> dict:
    """Synthetic foreground-object condition batch: box codes `fg_encoding_box`
    [B, 6] = (x, y, z, l, w, unique yaw) in the scaled ranges of nuscenes_dataset.encoding_boxes_3d
    and class ids `fg_class` [B] in 0..7."""
    g = torch.Generator().manual_seed(seed)
    box = torch.rand(B, 6, generator=g) * 2 - 1
    cls = torch.randint(0, 8, (B,), generator=g)
    return {"fg_encoding_box": box, "fg_class": cls}


def synth_text_features(seed: int = 77) -> dict:
    """Stand-in for the CLIP class-name features of obj_text_feat.pkl (8 x 512, unit norm)."""
    names = ["car", "truck", "construction_vehicle", "bus", "trailer", "motorcycle", "bicycle",
             "pedestrian"]
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(8, 512, generator=g)
    f = f / f.norm(dim=1, keepdim=True)
    return {n: f[i] for i, n in enumerate(names)}


@torch.no_grad()
def seeded_fill_layout_gen(module: torch.nn.Module, salt: int = 0) -> torch.nn.Module:
    """The layout generator's tensors `seeded_fill` leaves degenerate, keyed by their state_dict name; call after
    `seeded_fill`: BatchNorm running statistics (mean 0.1 r, variance in [0.5, 1.5]; a fresh module has 0 / 1, which
    hides a wrong fold) and the embedding tables at 0.5 r (`seeded_fill` scales them by 1 / sqrt(width))."""
    for key, p in list(module.named_parameters()) + list(module.named_buffers()):
        g = _gen_for(key, salt + 1)
        if key.endswith("running_mean"):
            v = 0.1 * torch.randn(p.shape, generator=g)
        elif key.endswith("running_var"):
            v = 0.5 + torch.rand(p.shape, generator=g)
        elif "embeddings" in key and key.endswith("weight") and "box_embeddings" not in key:
            v = 0.5 * torch.randn(p.shape, generator=g)
        else:
            continue
        p.copy_(v.to(device=p.device, dtype=p.dtype))
    return module


@torch.no_grad()
def seeded_fill_pointnet(module: torch.nn.Module, salt: int = 0) -> torch.nn.Module:
    """Seeded weights of the PointNet extractor (STN3d / PointNetfeat / PointNet1), keyed by state_dict name: `seeded_fill`,
    then what it leaves trivial -- BatchNorm running means at 0.3 r, running variances in [0.5, 1.5], and about a quarter
    of the entries of every `bn3.weight` (the BatchNorm in front of a max over the points) negative, so a scale applied
    behind the max instead of inside the product shows."""
    seeded_fill(module, salt)
    for key, p in list(module.named_parameters()) + list(module.named_buffers()):
        g = _gen_for(key, salt + 1)
        if key.endswith("running_mean"):
            v = 0.3 * torch.randn(p.shape, generator=g)
        elif key.endswith("running_var"):
            v = 0.5 + torch.rand(p.shape, generator=g)
        elif key.endswith("bn3.weight"):
            v = torch.where(torch.rand(p.shape, generator=g) < 0.25, -p.detach().cpu().float(), p.detach().cpu().float())
        else:
            continue
        p.copy_(v.to(device=p.device, dtype=p.dtype))
    return module


def pointnet_clouds(B: int, N: int, seed: int) -> torch.Tensor:
    """[B, 3, N] float32 clouds as the evaluator feeds them (xyz / 80 of a synthetic sweep, channel-major) with every
    third point zeroed, as a masked range image leaves it."""
    import numpy as np

    out = np.empty((B, 3, N), np.float32)
    for b in range(B):
        pts = synth_points(N, seed * 1000 + b)[:, :3] / np.float32(80.0)
        pts[b % 3::3] = 0.0
        out[b] = pts.T
    return torch.from_numpy(out)


LAYOUT_GEN_VOCAB = {
    "object_idx_to_name": ["__scene__", "car", "truck", "construction_vehicle", "bus", "trailer", "motorcycle", "bicycle",
                           "pedestrian"],
    "pred_idx_to_name": ["__in_scene__", "front", "behind", "left", "right", "close by", "bigger than", "smaller than"],
}


def synth_scene_graph_batch(n_scenes: int, seed: int, manipulate: bool = False) -> dict:
    """Synthetic collated batch of the scene-graph layout generator, with the key names of the reference's collate
    (nuscenes_dataset.py:520-631, `tripltes` included): {'scenegraph_input': {'encoder': {...}, 'decoder': {...},
    'missing_nodes', 'manipulated_subs', 'manipulated_objs'}}.  Scenes are ragged (3 + (seed + i) % 7 objects), the last
    object of every scene appears in no triple, text / relationship features are 512-d unit-norm stand-ins for the CLIP
    features (one per class / predicate of LAYOUT_GEN_VOCAB), boxes are [O, 40] = 20 values in (-1, 1) + their loss
    mask.  manipulate=True: scene 0's encoder graph lacks one node of the decoder graph (an added node); the encoder
    graph of the last scene carries another predicate on one triple (a manipulated relationship) -- with one scene both
    happen in it."""
    import numpy as np

    g = np.random.default_rng(seed)
    n_cls, n_pred = len(LAYOUT_GEN_VOCAB["object_idx_to_name"]), len(LAYOUT_GEN_VOCAB["pred_idx_to_name"])
    tg = torch.Generator().manual_seed(1000 + seed)
    cls_feat = torch.randn(n_cls, 512, generator=tg)
    cls_feat = cls_feat / cls_feat.norm(dim=1, keepdim=True)
    rel_feat = torch.randn(n_pred, 512, generator=tg)
    rel_feat = rel_feat / rel_feat.norm(dim=1, keepdim=True)
    enc = {k: [] for k in ("objs", "tripltes", "boxes", "obj_to_scene", "triple_to_scene")}
    dec = {k: [] for k in enc}
    missing, man_s, man_o = [], [], []
    enc_off = dec_off = 0
    for i in range(n_scenes):
        n = 3 + (seed + i) % 7
        objs = g.integers(1, n_cls, n)
        boxes = np.concatenate([g.uniform(-1, 1, (n, 20)), (g.uniform(0, 1, (n, 20)) < 0.8).astype(np.float64)], 1)
        pairs = [(a, b) for a in range(n - 1) for b in range(n - 1) if a != b]      # object n-1: in no triple
        pick = g.permutation(len(pairs))[:max(2, min(len(pairs), 2 * n))]
        tri = np.array([[pairs[j][0], g.integers(1, n_pred), pairs[j][1]] for j in sorted(pick)], np.int64)
        e_objs, e_boxes, e_tri = objs.copy(), boxes.copy(), tri.copy()
        if manipulate and i == 0:
            a = int(tri[0, 0])                                       # a node with at least one triple is "added"
            keep = np.array([j for j in range(n) if j != a])
            remap = {int(j): k for k, j in enumerate(keep)}
            e_objs, e_boxes = objs[keep], boxes[keep]
            e_tri = np.array([[remap[int(s)], p, remap[int(o)]] for s, p, o in tri if s != a and o != a], np.int64)
            if len(e_tri) == 0:
                e_tri = np.array([[0, 1, 1]], np.int64)
            missing.append(enc_off + a)
        if manipulate and i == n_scenes - 1:
            k = len(e_tri) - 1
            e_tri[k, 1] = 1 + (e_tri[k, 1] % (n_pred - 1))           # another predicate on the encoder side
            man_s.append(enc_off + int(e_tri[k, 0]))
            man_o.append(enc_off + int(e_tri[k, 2]))
        for d, (o_, t_, b_, off) in ((enc, (e_objs, e_tri, e_boxes, enc_off)), (dec, (objs, tri, boxes, dec_off))):
            t_ = t_.copy()
            t_[:, 0] += off
            t_[:, 2] += off
            d["objs"].append(torch.from_numpy(o_.astype(np.int64)))
            d["tripltes"].append(torch.from_numpy(t_))
            d["boxes"].append(torch.from_numpy(b_.astype(np.float32)))
            d["obj_to_scene"].append(torch.full((len(o_),), i, dtype=torch.int64))
            d["triple_to_scene"].append(torch.full((len(t_),), i, dtype=torch.int64))
        enc_off += len(e_objs)
        dec_off += n
    out = {}
    for name, d in (("encoder", enc), ("decoder", dec)):
        c = {k: torch.cat(v) for k, v in d.items()}
        c["text_feats"] = cls_feat[c["objs"]].clone()
        c["rel_feats"] = rel_feat[c["tripltes"][:, 1]].clone()
        out[name] = c
    out.update(missing_nodes=missing, manipulated_subs=man_s, manipulated_objs=man_o)
    return {"scenegraph_input": out}


@torch.no_grad()
def seeded_fill_rangenet(module: torch.nn.Module, salt: int = 0) -> torch.nn.Module:
    """Seeded weights that keep a 53-layer random RangeNet (either module tree) in range, keyed by state_dict name: conv
    weights N(0, 1 / fan_in), conv biases 0.1 N, BatchNorm gains in U(0.5, 1.5) -- times 0.35 on the second BatchNorm of
    every residual block (`...bn2.weight` / `...residual.1.1.weight`), whose output is added to the block's input --
    BatchNorm biases and running means 0.2 N, running variances in U(0.5, 1.5).  With `rangenet_images` the decoder map
    peaks near 1e2 and every feature column varies; a He gain reaches 1e8 over the 52 convolutions."""
    for key, p in list(module.named_parameters()) + list(module.named_buffers()):
        if key.endswith("num_batches_tracked"):
            continue
        g = _gen_for(key, salt)
        if p.ndim == 4:
            v = torch.randn(p.shape, generator=g) / max(1, p.numel() // p.shape[0]) ** 0.5
        elif key.endswith("running_var"):
            v = 0.5 + torch.rand(p.shape, generator=g)
        elif key.endswith("running_mean"):
            v = 0.2 * torch.randn(p.shape, generator=g)
        elif key.endswith("weight"):                       # BatchNorm gains
            v = 0.5 + torch.rand(p.shape, generator=g)
            if key.endswith("bn2.weight") or key.endswith("residual.1.1.weight"):
                v = 0.35 * v
        elif ".bn" in key or key.startswith("bn") or key.endswith(".1.bias") and "head" not in key:
            v = 0.2 * torch.randn(p.shape, generator=g)    # BatchNorm biases
        else:
            v = 0.1 * torch.randn(p.shape, generator=g)    # conv biases (up convs, head)
        p.copy_(v.to(device=p.device, dtype=p.dtype))
    return module


def rangenet_images(B: int, H: int, W: int, seed: int, holes: float = 0.15) -> torch.Tensor:
    """[B, 5, H, W] float32 range images as the evaluator feeds them: (depth, x, y, z, remission), depth in 8 .. 40 m along
    the pixel's ray (azimuth over the columns, +10 .. -30 degrees over the rows), remission in [0, 1), and -1 in every
    channel of the `holes` share of the pixels that saw nothing."""
    import math

    g = torch.Generator().manual_seed(seed)
    depth = 8.0 + 32.0 * torch.rand((B, 1, H, W), generator=g)
    yaw = math.pi * (2.0 * (torch.arange(W, dtype=torch.float32) + 0.5) / W - 1.0).view(1, 1, 1, W)
    pitch = math.radians(10.0) - math.radians(40.0) * ((torch.arange(H, dtype=torch.float32) + 0.5) / H).view(1, 1, H, 1)
    img = torch.cat([depth, depth * torch.cos(yaw) * torch.cos(pitch), -depth * torch.sin(yaw) * torch.cos(pitch),
                     depth * torch.sin(pitch).expand(1, 1, H, W), torch.rand((B, 1, H, W), generator=g)], dim=1)
    hole = torch.rand((B, 1, H, W), generator=g) < holes
    return torch.where(hole, torch.full_like(img, -1.0), img).contiguous()


@torch.no_grad()
def seeded_fill_pointmlp(module: torch.nn.Module, salt: int = 0) -> torch.nn.Module:
    """Seeded weights for a PointMLP `Model` of either module tree, keyed by state_dict name: conv / linear weights
    N(0, 2 / fan_in) (0.5 of that on the second layer of every residual block, whose output is added to the block's input),
    biases 0.1 N, BatchNorm gains in U(0.5, 1.5), BatchNorm biases and running means 0.2 N, running variances in
    U(0.5, 1.5), affine_alpha in U(0.5, 1.5) and affine_beta 0.2 N: nothing is left at its initial value."""
    bn_names = {n for n, m in module.named_modules() if isinstance(m, torch.nn.BatchNorm1d)}
    for key, p in list(module.named_parameters()) + list(module.named_buffers()):
        if key.endswith("num_batches_tracked"):
            continue
        g = _gen_for(key, salt)
        owner, leaf = key.rsplit(".", 1) if "." in key else ("", key)
        if leaf == "affine_alpha":
            v = 0.5 + torch.rand(p.shape, generator=g)
        elif leaf == "affine_beta":
            v = 0.2 * torch.randn(p.shape, generator=g)
        elif owner in bn_names:
            v = 0.5 + torch.rand(p.shape, generator=g) if leaf in ("weight", "running_var") else \
                0.2 * torch.randn(p.shape, generator=g)
        elif leaf == "weight":
            fan_in = max(1, p.numel() // p.shape[0])
            v = torch.randn(p.shape, generator=g) * ((0.5 if ".net2." in key else 2.0) / fan_in) ** 0.5
        else:
            v = 0.1 * torch.randn(p.shape, generator=g)
        p.copy_(v.to(device=p.device, dtype=p.dtype))
    return module


@torch.no_grad()
def seeded_fill_glenet(module: torch.nn.Module, salt: int = 0) -> torch.nn.Module:
    """Seeded weights for a GLENet `Generator` of either module tree: `seeded_fill_pointnet`, whose key suffixes
    (`running_mean`, `running_var`, `bn3.weight` -- here the BatchNorm in front of the max over an object's points) are
    GLENet's too.  `global_step` is left alone."""
    return seeded_fill_pointnet(module, salt)
