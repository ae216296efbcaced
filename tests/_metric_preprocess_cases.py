"""Inputs of tests/test_metric_preprocess.py and tests/test_metric_preprocess_host.py: ragged batches of seeded clouds for
the range-image and the voxel front-end, the rule that drops points next to a pixel boundary, placed points.  Expected
values never come from here: the tests take them from the host route (preprocess_range, pcd2voxel + sparse_collate)."""
import functools
import math

import numpy as np

# the two image sizes of the tests under nuScenes' fov and depth range
CFG = {"4x16": {"size": [4, 16], "fov": [10, -30], "depth_range": [1.0, 45.0]},
       "32x1024": {"size": [32, 1024], "fov": [10, -30], "depth_range": [1.0, 45.0]}}
DEPTH_RANGE = [1.0, 45.0]
# batches of 1, 3 and 5 clouds with 0, 1, 63, 64, 65 and about 2 000 points (one wave is 64 points, a block 256)
BATCHES = {1: [2000], 3: [64, 0, 2003], 5: [1, 63, 0, 65, 1990]}
DROP_TOL = 1e-6          # px: the distance to a pixel boundary under which a point is dropped before both routes run
DROP_CAP = 1e-4          # the share of points the rule may drop


def sweep(seed, n, dtype):
    """n points at 0.5 ... 50 m (so both depth bounds cut), every azimuth, elevations from -40 to 20 degrees (so both row
    clamps are hit under a fov of 10 / -30)."""
    g = np.random.default_rng(seed)
    d = g.uniform(0.5, 50.0, n)
    yaw = g.uniform(-math.pi, math.pi, n)
    pitch = np.radians(g.uniform(-40.0, 20.0, n))
    p = np.stack([d * np.cos(pitch) * np.cos(yaw), d * np.cos(pitch) * np.sin(yaw), d * np.sin(pitch)], 1)
    return np.ascontiguousarray(p.astype(dtype))


def pixel_coordinates(cloud, cfg):
    """float64 (proj_x, proj_y) before the floor, by pcd2range's lines on the cloud widened to float64, for every point."""
    p = np.asarray(cloud, np.float64)
    fov_up, fov_down = cfg["fov"][0] / 180.0 * np.pi, cfg["fov"][1] / 180.0 * np.pi
    fov_range = abs(fov_down) + abs(fov_up)
    depth = np.linalg.norm(p, 2, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        yaw = -np.arctan2(p[:, 1], p[:, 0])
        pitch = np.arcsin(p[:, 2] / depth)
    px = 0.5 * (yaw / np.pi + 1.0) * cfg["size"][1]
    py = (1.0 - (pitch + abs(fov_down)) / fov_range) * cfg["size"][0]
    return px, py


def drop_near_boundaries(cloud, cfg):
    """(the cloud without the points whose float64 pixel coordinate is within DROP_TOL px of an integer, how many went):
    double-precision atan2 / asin differ between libraries by about 1e-12 px at this scale, which decides such a point."""
    if cloud.shape[0] == 0:
        return cloud, 0
    px, py = pixel_coordinates(cloud, cfg)
    near = (np.abs(px - np.rint(px)) < DROP_TOL) | (np.abs(py - np.rint(py)) < DROP_TOL)
    return np.ascontiguousarray(cloud[~near]), int(near.sum())


@functools.lru_cache(maxsize=None)
def range_batch(size_key, nclouds, dtype_name):
    """(clouds after the drop rule, points before it, points dropped) of one seeded batch."""
    dtype = np.dtype(dtype_name)
    cfg = CFG[size_key]
    clouds, total, dropped = [], 0, 0
    for k, n in enumerate(BATCHES[nclouds]):
        c, d = drop_near_boundaries(sweep(1000 * nclouds + 10 * k + (7 if dtype == np.float32 else 0), n, dtype), cfg)
        clouds.append(c)
        total += n
        dropped += d
    return clouds, total, dropped


RANGE_CASES = [(s, b, d) for s in CFG for b in BATCHES for d in ("float64", "float32")]


def ray(cfg, row, col, frac=(0.5, 0.5)):
    """The float64 unit vector through pixel (row, col) at the fraction `frac` of its height and width: a point on it lies
    in that pixel, far from its boundaries for the default."""
    H, W = cfg["size"]
    fov_up, fov_down = cfg["fov"][0] / 180.0 * np.pi, cfg["fov"][1] / 180.0 * np.pi
    fov_range = abs(fov_down) + abs(fov_up)
    proj_x, proj_y = (col + frac[1]) / W, (row + frac[0]) / H
    yaw = (2.0 * proj_x - 1.0) * np.pi                       # the host's yaw (= -atan2(y, x))
    pitch = (1.0 - proj_y) * fov_range - abs(fov_down)
    return np.array([np.cos(-yaw) * np.cos(pitch), np.sin(-yaw) * np.cos(pitch), np.sin(pitch)])


# ---- voxels --------------------------------------------------------------------------------------------------------------
def voxel_sweep(seed, n, dtype):
    """A metre-scale cloud on both sides of the origin, depths 0.3 ... 60 m: both filter bounds cut."""
    g = np.random.default_rng(seed)
    d = g.uniform(0.3, 60.0, n)
    v = g.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.ascontiguousarray((v * d[:, None]).astype(dtype))


def duplicates(seed, n, dtype):
    """n points in about n / 12 voxels: every voxel holds many, the first index must win."""
    g = np.random.default_rng(seed)
    centres = np.rint(g.uniform(-200, 200, (max(n // 12, 1), 3))) * 0.05
    p = centres[g.integers(0, centres.shape[0], n)] + g.uniform(-0.02, 0.02, (n, 3))
    return np.ascontiguousarray(p.astype(dtype))


def half_multiples(seed, n, dtype):
    """Coordinates on odd multiples of half the voxel size (k * 0.025, what a decimal file holds) and on dyadic ones
    (k / 8 = 2.5 k voxels: exact ties): round half to even decides, in the cloud's own dtype."""
    g = np.random.default_rng(seed)
    a = (2 * g.integers(-400, 400, (n // 2, 3)) + 1) * 0.025
    b = g.integers(-160, 160, (n - n // 2, 3)) / 8.0
    return np.ascontiguousarray(np.concatenate([a, b]).astype(dtype))


def at_filter_bounds(dtype):
    """Depths exactly on both bounds of the open interval (dropped) and one ulp inside and outside them, in the dtype."""
    one, far = dtype(DEPTH_RANGE[0]), dtype(DEPTH_RANGE[1])
    rows = []
    for v in (one, np.nextafter(one, dtype(2)), np.nextafter(one, dtype(0)), far, np.nextafter(far, dtype(0)),
              np.nextafter(far, dtype(100))):
        rows += [[v, 0, 0], [0, -v, 0], [0, 0, v]]
    rows += [[0.6, 0.8, 0.0], [27.0, 36.0, 0.0], [0, 0, 0]]          # 1 and 45 by Pythagoras, and the origin
    return np.ascontiguousarray(np.array(rows, dtype=dtype))


@functools.lru_cache(maxsize=None)
def voxel_batch(nclouds, dtype_name):
    """One seeded batch: random sweeps, a cloud of duplicates, one of ties, the bound cases, an empty cloud and one that the
    filter empties."""
    dtype = np.dtype(dtype_name).type
    if nclouds == 1:
        return [voxel_sweep(11, 2000, dtype)]
    if nclouds == 3:
        return [duplicates(21, 1990, dtype), np.zeros((0, 3), dtype), half_multiples(22, 65, dtype)]
    return [at_filter_bounds(dtype), voxel_sweep(31, 63, dtype), (voxel_sweep(32, 64, dtype) * dtype(1e-3)).astype(dtype),
            half_multiples(33, 2001, dtype), voxel_sweep(34, 1, dtype)]


VOXEL_CASES = [(b, d) for b in (1, 3, 5) for d in ("float32", "float64")]


def dyadic_sweep(seed, n, dtype):
    """Coordinates k / 64, |k| <= 1920 (30 m): p * 20 and the sum of squares are exact in float32, so torch's quotient (a
    product with 1 / 0.05) and its norm agree with the IEEE division and numpy's norm -- what the per-cloud route of a
    CUDA tensor needs to be a reference for the batched one."""
    g = np.random.default_rng(seed)
    return np.ascontiguousarray((g.integers(-1920, 1921, (n, 3)) / 64.0).astype(dtype))
