"""Float64 restatement of the point-voxel extractor of the Frechet Point-Voxel Distance: every rule of DESIGN.md section 5m
in plain torch / numpy on the CPU -- the points' float coordinate, `initial_voxelize`, the eight neighbours and trilinear
weights of `voxel_to_point` (from a plain dictionary over the coordinates, never the product's hash), the scatter-mean of
`point_to_voxel`, the Linear + BatchNorm1d fold and the SPVCNN forward.  Everything the sparse-volume extractor already
has (levels, neighbour tables, convolution, fold, sector means, Frechet distance) comes from _spconv_oracle.
`dtype=torch.float32` runs the same arithmetic in float32: the error of that mode against float64 is what the GPU tests
scale their tolerance by.

torchsparse 1.4.0 is CUDA-only and is not installed anywhere this suite runs: the semantics here are read from its sources
and the reference's Python.  tests/test_spvcnn_host.py pins the neighbour order and the weights on
torch.nn.functional.grid_sample, which is nobody's reading."""
import numpy as np
import torch

import _spconv_oracle as O

VOXEL_SIZE = O.VOXEL_SIZE
STRIDES = (1, 1, 16, 16, 4, 4, 1)            # of the seven exchanges, in the order of the forward


def float_coord(c, v=VOXEL_SIZE):
    """(c * v) / v as torch computes it on the device, in float32: a division by a Python scalar is a multiplication
    by its float32 reciprocal, (c * f32(v)) * (f32(1) / f32(v)).  c: integers."""
    c = np.asarray(c).astype(np.float32)
    v = np.float32(v)
    return (c * v) * (np.float32(1.0) / v)


def float_coord_div(c, v=VOXEL_SIZE):
    """The plain route (c * f32(v)) / f32(v), what the CPU computes."""
    c = np.asarray(c).astype(np.float32)
    return (c * np.float32(v)) / np.float32(v)


def point_coords(coords, v=VOXEL_SIZE):
    """[N, 4] float32 = (float_coord(xyz), batch) of integer coords [N, 4]."""
    c = coords.numpy()
    return torch.from_numpy(np.concatenate([float_coord(c[:, :3], v), c[:, 3:].astype(np.float32)], 1))


def initial_voxels(pts):
    """Level-0 voxels: the unique floors of the points' float coordinate, ascending by (batch, x, y, z); and for every
    point the row of its voxel."""
    cells = torch.floor(pts.double()).long()
    rows = sorted({tuple(r) for r in cells.tolist()}, key=lambda r: (r[3], r[0], r[1], r[2]))
    index = {r: i for i, r in enumerate(rows)}
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 4), torch.tensor([index[tuple(r)] for r in cells.tolist()])


def point_maps(pts, vox, s, dtype=torch.float64):
    """(idx [N, 8] int64, w [N, 8] `dtype`) of voxel_to_point at stride s: the rows of `vox` [M, 4] at floor(p / s) * s +
    {0, s}^3, z fastest (k = 4 ix + 2 iy + iz), in the point's batch, -1 when absent; w_k = (a_x a_y) a_z with a = pc - p
    on an axis whose offset is 0 and p - pf where it is s, pf = floor(p / s) * s, pc = pf + s; then w /= s^3,
    w[idx == -1] = 0, w /= sum_k w + 1e-8.  The base is taken from the float32 coordinate (s is a power of two: exact in
    either precision); the weights are computed in `dtype` from that coordinate."""
    index = O._index(vox)
    base = (torch.floor(pts[:, :3] / s) * s).long()
    q = torch.cat([base, pts[:, 3:].long()], 1)
    idx = O._lookup(index, q, O.offsets2(s))
    p = pts[:, :3].to(dtype)
    pf = torch.floor(p / s) * s
    pc = pf + s
    cols = []
    for k in range(8):
        a = [(p[:, d] - pf[:, d]) if (k >> (2 - d)) & 1 else (pc[:, d] - p[:, d]) for d in range(3)]
        cols.append((a[0] * a[1]) * a[2])
    w = torch.stack(cols, 1)
    w = w / float(s) ** 3
    w[idx == -1] = 0
    w = w / (w.sum(1, keepdim=True) + torch.tensor(1e-8, dtype=dtype))
    return idx, w


def devoxelize(F, idx, w):
    """out[i] = sum over ascending k with idx[i, k] >= 0 of w[i, k] F[idx[i, k]], in the dtype of F."""
    out = torch.zeros((idx.shape[0], F.shape[1]), dtype=F.dtype)
    for k in range(idx.shape[1]):
        has = idx[:, k] >= 0
        if bool(has.any()):
            out[has] += w[has, k:k + 1].to(F.dtype) * F[idx[has, k]]
    return out


def voxelize(F, idx0, n_voxels):
    """out[v] = sum over the points p with idx0[p] = v, ascending, of F[p] / count[v]; zeros for a voxel without points."""
    has = idx0 >= 0
    count = torch.bincount(idx0[has], minlength=n_voxels).to(F.dtype)
    out = torch.zeros((n_voxels, F.shape[1]), dtype=F.dtype)
    for p in has.nonzero()[:, 0].tolist():
        out[idx0[p]] += F[p] / count[idx0[p]]
    return out


def fold_linear(sd, lin_key, bn_key, dtype):
    """(w [1, Ci, Co], b) of bn(linear(.)) in eval mode, folded in float64: w = W^T s, b = (bias - mean) s + beta."""
    s = sd[bn_key + ".weight"].double() / torch.sqrt(sd[bn_key + ".running_var"].double() + 1e-5)
    w = sd[lin_key + ".weight"].double().t() * s
    b = (sd[lin_key + ".bias"].double() - sd[bn_key + ".running_mean"].double()) * s + sd[bn_key + ".bias"].double()
    return w[None].to(dtype), b.to(dtype)


def network(sd, feats, coords, dtype=torch.float64, deep=False, v=VOXEL_SIZE):
    """The SPVCNN forward with return_final_logits=True: z3.F [N, cs[8]] per input point, in `dtype`; `deep`: y1.F over
    the level-4 voxels after the second exchange (return_logits=True), with those voxels."""
    pts = point_coords(coords, v)
    vox, _ = initial_voxels(pts)
    cs = O.levels(vox)
    same = [O.nbr_same(c, 1 << l) for l, c in enumerate(cs)]
    down = [O.nbr_down(cs[l], cs[l + 1], 1 << l) for l in range(4)]
    up = [O.nbr_up(cs[l], cs[l + 1], 1 << l) for l in range(4)]
    maps = {l: point_maps(pts, cs[l], 1 << l, dtype) for l in (0, 2, 4)}

    def to_points(x, l):
        return devoxelize(x, *maps[l])

    def to_voxels(f, l):
        return voxelize(f, maps[l][0][:, 0], len(cs[l]))

    def cb(x, nbr, pre_conv, pre_bn, relu, res=None):
        w, b = O.fold(sd, pre_conv, pre_bn, dtype)
        return O.conv(x, nbr, w, b, res, relu)

    def block(x, nbr, pre):
        h = cb(x, nbr, pre + ".net.0", pre + ".net.1", True)
        r = cb(x, None, pre + ".downsample.0", pre + ".downsample.1", False) if pre + ".downsample.0.kernel" in sd else x
        return cb(h, nbr, pre + ".net.3", pre + ".net.4", True, res=r)

    def transform(i, f):
        w, b = fold_linear(sd, f"point_transforms.{i}.0", f"point_transforms.{i}.1", dtype)
        return O.conv(f, None, w, b, None, True)

    def upward(i, x, skip):
        lvl = 4 - i
        y = cb(x, up[lvl], f"up{i}.0.net.0", f"up{i}.0.net.1", True)
        x = torch.cat([y, skip], dim=1)
        x = block(x, same[lvl], f"up{i}.1.0")
        return block(x, same[lvl], f"up{i}.1.1")

    x = cb(to_voxels(feats.to(dtype), 0), same[0], "stem.0", "stem.1", True)
    x0 = cb(x, same[0], "stem.3", "stem.4", True)
    z0 = to_points(x0, 0)
    skips = [x0]
    x = to_voxels(z0, 0)
    for i in range(1, 5):
        x = cb(x, down[i - 1], f"stage{i}.0.net.0", f"stage{i}.0.net.1", True)
        x = block(x, same[i], f"stage{i}.1")
        x = block(x, same[i], f"stage{i}.2")
        skips.append(x)
    z1 = to_points(x, 4) + transform(0, z0)
    y = to_voxels(z1, 4)
    if deep:
        return y, cs[4]
    y = upward(1, y, skips[3])
    y = upward(2, y, skips[2])
    z2 = to_points(y, 2) + transform(1, z1)
    y = upward(3, to_voxels(z2, 2), skips[1])
    y = upward(4, y, skips[0])
    return to_points(y, 0) + transform(2, z2)


def seeded_state(model, seed):
    """O.seeded_state over the SPVCNN's keys: it draws the transforms' Linear weights at scale 0.1, their biases at 0.2
    (away from zero) and their BatchNorm buffers away from (0, 1), as it does for the convolutions'."""
    return O.seeded_state(model, seed)
