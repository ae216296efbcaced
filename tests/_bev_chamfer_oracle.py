"""numpy restatements for the Minimum Matching Distance tests (tests/test_bev_chamfer.py, tests/test_bev_chamfer_host.py):
the reference's `pcd2bev_bin` (lidargen/metrics/metric_utils.py:261-284), the float32 arithmetic of its 2-D chamfer kernel
(chamfer2D.cu NmDistanceKernel: d = dx*dx + dy*dy, first minimum wins), `compute_pairwise_cd_batch` on top of it
(metric_utils.py:425-444), the EXACT chamfer distance of two cell sets in integers, and seeded synthetic sweeps."""
import math

import numpy as np

DATA_CONFIG = {"64": {"x": [-50, 50], "y": [-50, 50]}, "32": {"x": [-30, 30], "y": [-30, 30]}}
CHUNK = 512


def grid(x_range, y_range, voxel):
    nx = math.ceil((x_range[1] - x_range[0]) / voxel)
    ny = math.ceil((y_range[1] - y_range[0]) / voxel)
    return nx, ny, (math.ceil(x_range[0] / voxel), math.ceil(y_range[0] / voxel))


def tolerance(nx, ny):
    """Relative, per pair, between the float32 arithmetic and the exact value: coordinates k / n rounded to float32 carry
    2^-24 each, a difference 2^-23 against a smallest non-zero difference of 1 / n, the square doubles it; 1e-5 for the
    float32 means."""
    return 2.0 ** -21 * max(nx, ny) + 1e-5


def bev_cells(pcd, x_range, y_range, voxel):
    """Unique integer cells [k, 2] of one cloud, sorted by (ix, iy): strict mask, floor of the float32 quotient."""
    nx, ny, mb = grid(x_range, y_range, voxel)
    p = np.asarray(pcd, np.float32)
    m = (p[:, 0] > x_range[0]) & (p[:, 0] < x_range[1]) & (p[:, 1] > y_range[0]) & (p[:, 1] < y_range[1])
    v = np.floor(p[m][:, :2] / np.float32(voxel)).astype(np.int64) - np.asarray(mb, np.int64)
    assert v.size == 0 or (v.min() >= 0 and (v < (nx, ny)).all())
    key = np.unique(v[:, 0] * ny + v[:, 1])
    return np.stack([key // ny, key % ny], axis=1).reshape(-1, 2)


def bev_bin(x_range, y_range, voxel, *args):
    nx, ny, _ = grid(x_range, y_range, voxel)
    shape = np.asarray([nx, ny], np.float64)
    return tuple([(bev_cells(p, x_range, y_range, voxel).astype(np.float64) / shape).astype(np.float32) for p in data]
                 for data in args)


def pcd2bev_bin(data_type, *args, voxel_size=0.5):
    cfg = DATA_CONFIG[data_type]
    return bev_bin(cfg["x"], cfg["y"], voxel_size, *args)


def nm_distance(a, b):
    """For every point of a [n, 2] its squared distance to and the index of the nearest point of b [m, 2], float32, in the
    order of the kernel: chunks of 512 targets, first minimum inside a chunk, an earlier chunk keeps a tie."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    best = np.zeros(a.shape[0], np.float32)
    besti = np.zeros(a.shape[0], np.int32)
    for k2 in range(0, b.shape[0], CHUNK):
        t = b[k2:k2 + CHUNK]
        x2 = t[None, :, 0] - a[:, None, 0]
        y2 = t[None, :, 1] - a[:, None, 1]
        d = x2 * x2 + y2 * y2
        assert d.dtype == np.float32
        ci = np.argmin(d, axis=1)
        cb = d[np.arange(a.shape[0]), ci]
        take = (best > cb) if k2 else np.ones(a.shape[0], bool)
        best = np.where(take, cb, best)
        besti = np.where(take, ci + k2, besti).astype(np.int32)
    return best, besti


def chamfer2d(x1, x2):
    """[B, N, 2], [B, M, 2] -> dist1, dist2, idx1, idx2 like chamfer_2DDist."""
    out = [[], [], [], []]
    for a, b in zip(x1, x2):
        d1, i1 = nm_distance(a, b)
        d2, i2 = nm_distance(b, a)
        for o, v in zip(out, (d1, d2, i1, i2)):
            o.append(v)
    return tuple(np.stack(o) for o in out)


def pairwise_cd_batch(reference, samples):
    """compute_pairwise_cd_batch: padding with points at 1e6, float32 means of the unpadded heads."""
    len_r, len_s = reference.shape[0], [s.shape[0] for s in samples]
    n = max([len_r] + len_s)
    pad = lambda a: np.vstack([a, np.ones((n - a.shape[0], 2), np.float32) * 1e6])
    r = pad(np.asarray(reference, np.float32))
    out = []
    for s, ls in zip(samples, len_s):
        d1, _ = nm_distance(r, pad(np.asarray(s, np.float32)))
        d2, _ = nm_distance(pad(np.asarray(s, np.float32)), r)
        out.append(float((d1[:len_r].mean(dtype=np.float32) + d2[:ls].mean(dtype=np.float32)) / np.float32(2.0)))
    return out


def exact_sums(cr, cs, nx, ny):
    """Integer sums over the cells of cr / cs of the weighted squared distance di^2 ny^2 + dj^2 nx^2 to the other set."""
    cr, cs = np.asarray(cr, np.int64), np.asarray(cs, np.int64)
    di = cr[:, None, 0] - cs[None, :, 0]
    dj = cr[:, None, 1] - cs[None, :, 1]
    d = di * di * (ny * ny) + dj * dj * (nx * nx)
    return int(d.min(axis=1).sum()), int(d.min(axis=0).sum())


def exact_cd(cr, cs, nx, ny):
    a, b = exact_sums(cr, cs, nx, ny)
    return (float(a) / len(cr) + float(b) / len(cs)) / float(2 * nx * nx * ny * ny)


def exact_matrix(ref_cells, smp_cells, nx, ny):
    return np.array([[exact_cd(r, s, nx, ny) for s in smp_cells] for r in ref_cells], np.float64)


def sweeps(seed, count, x_range, y_range, voxel=0.5, lo=50, hi=400):
    """`count` polar clouds [N, 3] float32: radius |N(0, sigma)|, sigma in [3, 25] m, 50 ... 400 points; the first points of
    every cloud lie exactly on a range bound, outside the range, on a cell edge, and twice in one cell."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(lo, hi + 1))
        sigma = rng.uniform(3.0, 25.0)
        r = np.abs(rng.normal(0.0, sigma, n))
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        p = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-3.0, 1.0, n)], axis=1).astype(np.float32)
        xm, ym = 0.5 * (x_range[0] + x_range[1]), 0.5 * (y_range[0] + y_range[1])
        special = np.array([[x_range[0], ym, 0.0], [xm, y_range[1], 0.0], [x_range[1] + 1.0, ym, 0.0],
                            [xm, y_range[0] - 7.5, 0.0], [xm + 2 * voxel, ym - 3 * voxel, 0.0],
                            [xm + 0.25 * voxel, ym + 0.25 * voxel, 0.0], [xm + 0.75 * voxel, ym + 0.5 * voxel, 1.0]],
                           np.float32)
        p[:len(special)] = special
        out.append(p)
    return out


def cloud_of_cells(cells, x_range, y_range, voxel=0.5, repeat=1):
    """A cloud with one point (or `repeat`) in the middle of each given cell."""
    _, _, mb = grid(x_range, y_range, voxel)
    c = np.repeat(np.asarray(cells, np.float64), repeat, axis=0)
    xy = (c + np.asarray(mb, np.float64) + 0.5) * voxel
    return np.concatenate([xy, np.zeros((len(xy), 1))], axis=1).astype(np.float32)
