"""Float64 restatement of the sparse-volume extractor of the Frechet Sparse Volume Distance: every rule of DESIGN.md
section 5l in plain torch / numpy on the CPU -- the input (`preprocess_pcd`, `pcd2voxel`, `collate`), the coordinate levels
and the three neighbour tables (from a plain dictionary over the coordinates, never the product's hash), the convolution,
the BatchNorm fold, the MinkUNet forward, the depth-sector means and the Frechet distance.  `dtype=torch.float32` runs the
same arithmetic in float32: the error of that mode against float64 is what the GPU tests scale their tolerance by.

torchsparse 1.4.0 is CUDA-only and is not installed anywhere this suite runs: the semantics here are read from its sources
and the reference's Python.  tests/test_spconv_host.py pins the two offset orders and the transposed convolution on
torch.nn.functional.conv3d / conv_transpose3d, which are nobody's reading."""
import numpy as np
import torch

VOXEL_SIZE = 0.05
NUM_SECTORS = 16


def offsets3(s):
    """ks 3: {-s, 0, s}^3, x fastest: k = ix + 3 iy + 9 iz."""
    return [((k % 3 - 1) * s, (k // 3 % 3 - 1) * s, (k // 9 - 1) * s) for k in range(27)]


def offsets2(s):
    """ks 2: {0, s}^3, z fastest (an even kernel volume flips the order): k = 4 ix + 2 iy + iz."""
    return [((k >> 2) * s, ((k >> 1) & 1) * s, (k & 1) * s) for k in range(8)]


def _index(coords):
    return {tuple(int(v) for v in row): i for i, row in enumerate(coords.tolist())}


def _lookup(index, coords, offs):
    """[M, K] int64: row of coords + offset (same batch) in `index`, -1 when absent."""
    out = np.full((len(coords), len(offs)), -1, np.int64)
    for j, (x, y, z, b) in enumerate(coords.tolist()):
        for k, (dx, dy, dz) in enumerate(offs):
            out[j, k] = index.get((x + dx, y + dy, z + dz, b), -1)
    return torch.from_numpy(out)


def nbr_same(coords, s):
    return _lookup(_index(coords), coords, offsets3(s))


def down_coords(coords, s):
    """Unique rows of (xyz // 2s) * 2s with their batch, ascending by (batch, x, y, z)."""
    c = coords.clone().long()
    c[:, :3] = torch.div(c[:, :3], 2 * s, rounding_mode="floor") * (2 * s)
    rows = sorted({tuple(r) for r in c.tolist()}, key=lambda r: (r[3], r[0], r[1], r[2]))
    return torch.tensor(rows, dtype=coords.dtype).reshape(-1, 4)


def nbr_down(fine, coarse, s):
    """[M_coarse, 8]: the children coarse + offset_k among the fine rows."""
    return _lookup(_index(fine), coarse, offsets2(s))


def nbr_up(fine, coarse, s):
    """[M_fine, 8]: entry k = the coarse row j with fine = coarse[j] + offset_k (one k per row), -1 elsewhere."""
    index = _index(coarse)
    return _lookup(index, fine, [(-dx, -dy, -dz) for dx, dy, dz in offsets2(s)])


def conv(x, nbr, w, b=None, res=None, relu=False):
    """act(sum_k x[nbr[:, k]] @ w[k] + b + res) in the dtype of x; nbr None: w [1, Ci, Co], the dense product."""
    w = w.to(x.dtype)
    if nbr is None:
        y = x @ w[0]
    else:
        y = torch.zeros((nbr.shape[0], w.shape[2]), dtype=x.dtype)
        for k in range(w.shape[0]):
            has = nbr[:, k] >= 0
            if bool(has.any()):
                y[has] += x[nbr[has, k]] @ w[k]
    if b is not None:
        y = y + b.to(x.dtype)
    if res is not None:
        y = y + res.to(x.dtype)
    return torch.relu(y) if relu else y


def fold(sd, conv_key, bn_key, dtype):
    """(w [K, Ci, Co], b) of bn(conv(.)) in eval mode, folded in float64, then rounded to `dtype`."""
    k = sd[conv_key + ".kernel"].double()
    w = k.reshape(-1, k.shape[-2], k.shape[-1])
    s = sd[bn_key + ".weight"].double() / torch.sqrt(sd[bn_key + ".running_var"].double() + 1e-5)
    b = sd[bn_key + ".bias"].double() - sd[bn_key + ".running_mean"].double() * s
    return (w * s).to(dtype), b.to(dtype)


def levels(coords, n=5):
    cs = [coords]
    for l in range(1, n):
        cs.append(down_coords(cs[-1], 1 << (l - 1)))
    return cs


def network(sd, feats, coords, dtype=torch.float64, maps=None):
    """The MinkUNet forward with return_final_logits=True: y4.F [N, cs[8]] over the input voxels, in `dtype`."""
    cs = levels(coords)
    same = [nbr_same(c, 1 << l) for l, c in enumerate(cs)]
    down = [nbr_down(cs[l], cs[l + 1], 1 << l) for l in range(4)]
    up = [nbr_up(cs[l], cs[l + 1], 1 << l) for l in range(4)]
    if maps is not None:
        maps.update(coords=cs, same=same, down=down, up=up)

    def cb(x, nbr, pre_conv, pre_bn, relu, res=None):
        w, b = fold(sd, pre_conv, pre_bn, dtype)
        return conv(x, nbr, w, b, res, relu)

    def block(x, nbr, pre):
        h = cb(x, nbr, pre + ".net.0", pre + ".net.1", True)
        r = cb(x, None, pre + ".downsample.0", pre + ".downsample.1", False) if pre + ".downsample.0.kernel" in sd else x
        return cb(h, nbr, pre + ".net.3", pre + ".net.4", True, res=r)

    x = cb(feats.to(dtype), same[0], "stem.0", "stem.1", True)
    skips = [cb(x, same[0], "stem.3", "stem.4", True)]
    x = skips[0]
    for i in range(1, 5):
        x = cb(x, down[i - 1], f"stage{i}.0.net.0", f"stage{i}.0.net.1", True)
        x = block(x, same[i], f"stage{i}.1")
        x = block(x, same[i], f"stage{i}.2")
        skips.append(x)
    for i in range(1, 5):
        lvl = 4 - i
        y = cb(x, up[lvl], f"up{i}.0.net.0", f"up{i}.0.net.1", True)
        x = torch.cat([y, skips[lvl]], dim=1)
        x = block(x, same[lvl], f"up{i}.1.0")
        x = block(x, same[lvl], f"up{i}.1.1")
    return x


def preprocess_pcd(pcd, depth_range):
    d = np.linalg.norm(pcd, 2, axis=1)
    return pcd[(d > depth_range[0]) & (d < depth_range[1])]


def pcd2voxel(pcd):
    """(feats [n, 4] float32, coords [n, 3] int64): round half to even of p / 0.05 minus the minimum; unique voxels in
    lexicographic (x, y, z) order, each keeping its first point; feature (x, y, z, -1) of that point."""
    v = np.round(pcd / VOXEL_SIZE)
    v = (v - v.min(0)).astype(np.int64)
    first = {}
    for i, row in enumerate(map(tuple, v.tolist())):
        first.setdefault(row, i)
    rows = sorted(first)
    inds = np.array([first[r] for r in rows], np.int64)
    feats = np.concatenate([pcd[inds].astype(np.float64), -np.ones((len(inds), 1))], 1).astype(np.float32)
    return torch.from_numpy(feats), torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def collate(items):
    feats = torch.cat([f for f, _ in items])
    coords = torch.cat([torch.cat([c, torch.full((len(c), 1), i, dtype=torch.int64)], 1) for i, (_, c) in enumerate(items)])
    return feats, coords


def sector_edges(depth_range):
    e = torch.linspace(depth_range[0] + 3, depth_range[1], NUM_SECTORS + 1)
    e[0] = 0.0
    return e


def sector_means(logits, coords, depth_range, n_clouds=None):
    """[n_clouds, 16 C] in the dtype of logits: the sector of a row is decided in float32, as the reference does
    (c = xyz.float() - mean, d = |c| * 0.05 against float32 edges); the mean of a sector's rows is taken in that dtype."""
    edges = sector_edges(depth_range)
    n_clouds = int(coords[:, 3].max()) + 1 if n_clouds is None else n_clouds
    C = logits.shape[1]
    out = torch.zeros((n_clouds, NUM_SECTORS * C), dtype=logits.dtype)
    for b in range(n_clouds):
        m = coords[:, 3] == b
        if not bool(m.any()):
            continue
        c = coords[m][:, :3].float()
        d = torch.norm(c - c.mean(0), dim=-1) * VOXEL_SIZE
        f = logits[m]
        for i in range(NUM_SECTORS):
            sel = (d >= edges[i]) & (d < edges[i + 1])
            if bool(sel.any()):
                out[b, i * C:(i + 1) * C] = f[sel].mean(0)
    return out


def compute_fd(reference, samples):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2) of np.mean / np.cov(rowvar=False)."""
    from scipy import linalg

    mu1, mu2 = np.mean(reference, axis=0), np.mean(samples, axis=0)
    s1, s2 = np.cov(reference, rowvar=False), np.cov(samples, rowvar=False)
    root, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(root).all():                                  # the evaluator's retry on a singular product
        eye = np.eye(s1.shape[0]) * 1e-6
        root = linalg.sqrtm((s1 + eye).dot(s2 + eye))
    return float(np.real((mu1 - mu2).dot(mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(root)))


def rel_l2_rows(got, ref):
    """Relative L2 error per row against the float64 `ref`."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    return (got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)


CONFIG = {"model_params": dict(cr=0.5, layer_num=[32, 32, 64, 128, 256, 256, 128, 96, 96], voxel_size=0.05, num_class=20,
                               input_dims=4)}


def seeded_state(model, seed):
    """A state dict for `model` as a checkpoint may leave it: kernels of fan-in scale, BatchNorm buffers away from (0, 1),
    some negative BatchNorm weights."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(100)
        elif k.endswith(".kernel"):
            fan = v.shape[-2] * (v.shape[0] if v.dim() == 3 else 1)
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / fan) ** 0.5
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g) * 1.5
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.3
        elif k.endswith(".weight") and v.dim() == 1:
            w = 0.7 + 0.6 * torch.rand(v.shape, generator=g)
            sd[k] = torch.where(torch.rand(v.shape, generator=g) < 0.2, -w, w)
        elif k.endswith(".bias") and v.dim() == 1 and "classifier" not in k:
            sd[k] = torch.randn(v.shape, generator=g) * 0.2
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    return sd
