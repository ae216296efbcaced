"""GPU tests of the radius-limited nearest neighbour and the point-to-point ICP (csrc/icp.hip, ops.nn_radius,
ops.icp_point_to_point) and of the TTCE / TCD front-end (lidargen/metrics/temporal.py) against tests/_icp_oracle.py.

Sizes are the kernels' edges: one point, fewer points than a wave, one more than a 256-point block, several blocks with a
partial last one.  Parity with the oracle is claimed only where the oracle's own records say it is decidable: no
nearest-neighbour tie, no point on the radius, a well-conditioned covariance (otherwise: pick another seed)."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL = dict(shift=(0.15, 0.05), yaw_deg=0.3)
_cache = {}


def _ops():
    from lidarcrafter_amd import ops

    return ops


def _scene(n, m, seed, small=False):
    key = ("scene", n, m, seed, small)
    if key not in _cache:
        _cache[key] = O.scene_pair(n, m, seed, **(SMALL if small else {}))
    return _cache[key]


def _oracle(n, m, seed, radius, small=False):
    key = ("icp", n, m, seed, radius, small)
    if key not in _cache:
        src, tgt, _ = _scene(n, m, seed, small)
        _cache[key] = (O.icp(src, tgt, radius), O.icp(src, tgt, radius, extended=True))
    return _cache[key]


def _batch(clouds):
    """list of [n,3] arrays -> (points on the device, offsets)"""
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds, axis=0), dtype=np.float64)).to(DEV)
    return pts, torch.from_numpy(off)


def _T(*mats):
    return torch.from_numpy(np.stack(mats).astype(np.float64)).to(DEV)


def _motion():
    from scipy.spatial.transform import Rotation

    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("zyx", [2.0, -0.7, 0.4], degrees=True).as_matrix()
    T[:3, 3] = [0.6, -0.25, 0.05]
    return T


def _check_nn(src, tgt, radius, T=None, grid_ratio=None, exact=True):
    """One pair through ops.nn_radius against the brute force: indices everywhere; d2 bit-equal (exact) or within
    32 * 2^-52 * (|p| + |q|)^2 -- about ten float64 roundings on coordinates of that size."""
    ops = _ops()
    T = np.eye(4) if T is None else T
    pts, off = _batch([src, tgt])
    grid = None if grid_ratio is None else ops.nn_grid(pts, off, radius, cell_ratio=grid_ratio)
    idx, d2 = ops.nn_radius(pts, off, [[0, 1]], _T(T), radius, grid=grid)
    idx, d2 = idx[0].cpu().numpy(), d2[0].cpu().numpy()
    moved = O.apply_transform(T, src)
    want_idx, want_d2 = O.nn_brute(moved, tgt, radius)
    assert idx.shape == (len(src),)
    bad = np.nonzero(idx != want_idx)[0]
    assert bad.size == 0, (bad[:5], idx[bad[:5]], want_idx[bad[:5]], d2[bad[:5]], want_d2[bad[:5]])
    hit = want_idx >= 0
    assert np.isinf(d2[~hit]).all()
    if exact:
        assert np.array_equal(d2[hit], want_d2[hit])
    else:
        q = tgt[want_idx[hit]]
        bound = 32.0 * 2.0 ** -52 * (np.linalg.norm(moved[hit], axis=1) + np.linalg.norm(q, axis=1)) ** 2
        err = np.abs(d2[hit] - want_d2[hit])
        print("max |d d2| / bound", float((err / bound).max()) if hit.any() else 0.0)
        assert (err <= bound).all()
    return idx, d2


def _decidable(src, tgt, radius):
    """No tie and no point on the radius to 1e-9, by brute force (the tests under a non-identity T, where the device's
    transformed point may differ from numpy's in its last bit)."""
    D = O.sq_dist(src[:, None, :], tgt[None, :, :])
    part = np.sort(D, axis=1)[:, :2]
    if part.shape[1] == 2:
        near = part[:, 0] <= (radius + 1.0) ** 2
        assert ((part[near, 1] - part[near, 0]) / np.maximum(part[near, 1], 1e-300) >= 1e-9).all(), "pick another seed"
    assert (np.abs(part[:, 0] - radius * radius) / (radius * radius) >= 1e-9).all(), "pick another seed"


@pytest.mark.parametrize("radius", [2.0, 0.5])
@pytest.mark.parametrize("n,m", [(1, 1), (63, 1000), (257, 300), (2500, 2311)])
def test_nn_radius_matches_brute_force(n, m, radius):
    src, tgt, _ = _scene(n, m, 11)
    if n == 1:
        src, tgt = np.array([[3.0, -1.0, 0.5]]), np.array([[3.25, -1.25, 0.25]])   # d2 = 0.1875 <= 0.25
    idx, _ = _check_nn(src, tgt, radius)
    assert (idx >= 0).any()
    if (n, radius) != (63, 2.0):
        assert n == 1 or (idx < 0).any()               # both outcomes occur at this motion
    T = _motion()
    _decidable(O.apply_transform(T, src), tgt, radius)
    _check_nn(src, tgt, radius, T=T, exact=False)


def test_nn_radius_points_on_cell_faces_and_negative_coordinates():
    """Targets on a lattice of exactly the cell edge around the origin (floor, not truncation, must place the negative
    ones), queries on lattice points, on faces, on edges and beside them: every distance is tied several ways, the
    smallest index wins."""
    g = np.arange(-3.0, 4.0)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    tgt = tgt[np.random.default_rng(0).permutation(len(tgt))]
    rng = np.random.default_rng(1)
    q = np.concatenate([tgt[:40], tgt[40:80] + [0.5, 0.0, 0.0], tgt[80:120] + [0.5, 0.5, 0.0], tgt[120:160] + 0.5,
                        tgt[160:200] - [0.0, 0.25, 0.0], rng.uniform(-4.5, 4.5, (100, 3)),
                        np.array([[-3.0, -3.0, -3.0], [3.0, 3.0, 3.0], [-5.0, 0.0, 0.0], [0.0, 0.0, 5.0], [5.5, 0.0, 0.0]])])
    for ratio in (0.5, 1.0, 0.25):          # h = 1 (the lattice), 2 and 0.5 at radius 2
        _check_nn(q, tgt, 2.0, grid_ratio=ratio)
    _check_nn(q, tgt, 0.5, grid_ratio=2.0)   # h = 1 again; the half-lattice queries sit exactly on the radius


def test_nn_radius_queries_outside_the_bounding_box():
    _, tgt, _ = _scene(257, 300, 11)
    lo, hi = tgt.min(axis=0), tgt.max(axis=0)
    rows = []
    for k in range(3):
        for far in (0.5, 0.999, 1.001, 1.5, 40.0):
            for side, edge in ((-1.0, lo), (1.0, hi)):
                near = tgt[np.argmin(tgt[:, k]) if side < 0 else np.argmax(tgt[:, k])].copy()
                near[k] = edge[k] + side * far * 2.0
                rows.append(near)
    rows.append(hi + 1.0)
    rows.append(lo - 1.2)
    idx, _ = _check_nn(np.array(rows), tgt, 2.0)
    assert (idx >= 0).sum() >= 12 and (idx < 0).sum() >= 12


def test_nn_radius_one_crowded_cell_and_a_10_km_cloud():
    rng = np.random.default_rng(2)
    crowd = 10.0 + rng.uniform(0.0, 0.1, (700, 3))          # one cell, more than two blocks' worth of points
    src = 10.0 + rng.uniform(-1.5, 1.6, (300, 3))
    _check_nn(src, crowd, 2.0)
    _check_nn(src, crowd, 0.5)
    s2, tgt, _ = _scene(257, 300, 11)
    wide = np.concatenate([tgt, [[-5000.0, 0.0, 0.0], [5000.0, 0.0, 0.0]]])   # 10 km in x: the cell edge must be doubled
    q = np.concatenate([s2, [[-4999.0, 0.5, 0.0], [4999.5, 0.0, 0.2], [2500.0, 0.0, 0.0]]])
    idx, _ = _check_nn(q, wide, 2.0)
    assert idx[-3] == 300 and idx[-2] == 301 and idx[-1] == -1
    _check_nn(q, wide, 2.0, grid_ratio=1e-3)                 # a far too fine start is coarsened the same way


def test_nn_radius_duplicated_targets_smaller_index_wins():
    src, tgt, _ = _scene(257, 300, 11)
    perm = np.random.default_rng(3).permutation(len(tgt))
    idx, _ = _check_nn(src, np.concatenate([tgt, tgt[perm], tgt]), 2.0)
    assert idx.max() < len(tgt)


@pytest.mark.parametrize("n,m,radius", [(257, 300, 2.0), (2500, 2311, 0.5)])
def test_nn_radius_does_not_depend_on_target_order(n, m, radius):
    ops = _ops()
    src, tgt, _ = _scene(n, m, 11)
    perm = np.random.default_rng(4).permutation(m)
    T = _T(_motion())
    pts, off = _batch([src, tgt, tgt[perm]])
    idx, d2 = ops.nn_radius(pts, off, [[0, 1], [0, 2]], T.repeat(2, 1, 1), radius)
    idx = idx.cpu().numpy()
    hit = idx[0] >= 0
    assert hit.any() and np.array_equal(idx[1] >= 0, hit)
    assert np.array_equal(perm[idx[1][hit]], idx[0][hit])
    assert torch.equal(d2[0], d2[1])


ICP_CASES = [(257, 300, 1, 2.0, False), (63, 1000, 1, 2.0, False), (2500, 2311, 1, 2.0, False), (2500, 2311, 2, 0.5, True)]


@pytest.mark.parametrize("n,m,seed,radius,small", ICP_CASES)
def test_icp_matches_oracle(n, m, seed, radius, small):
    """Iterations, final correspondences and fitness equal the oracle's; T within 8 dev + 1e-13, dev = the distance
    between the float64 / incremental and the long double / composed runs of the oracle on this case (measured on an
    MI355X: profiles/temporal_metrics.txt)."""
    ops = _ops()
    src, tgt, _ = _scene(n, m, seed, small)
    a, b = _oracle(n, m, seed, radius, small)
    tie, rad, s_ratio = a.margins()
    assert tie >= 1e-9 and rad >= 1e-9 and s_ratio >= 1e-3, "pick another seed"
    assert b.iterations == a.iterations
    dev = float(np.abs(a.T - b.T).max())
    pts, off = _batch([src, tgt])
    T, fitness, rmse, iters = ops.icp_point_to_point(pts, off, [[0, 1]], radius)
    got = T[0].cpu().numpy()
    observed = float(np.abs(got - a.T).max())
    print(f"icp case N={n} M={m} r={radius}: iterations {a.iterations} dev {dev:.3e} observed {observed:.3e} "
          f"factor {observed / max(dev, 1e-300):.2f} rmse diff {abs(float(rmse[0]) - a.inlier_rmse):.3e}")
    assert int(iters[0]) == a.iterations
    idx, _ = ops.nn_radius(pts, off, [[0, 1]], T, radius)
    assert np.array_equal(idx[0].cpu().numpy(), a.records[-1]["idx"])
    assert float(fitness[0]) == a.fitness
    assert np.array_equal(got[3], [0.0, 0.0, 0.0, 1.0])
    assert observed <= 8.0 * dev + 1e-13
    # a transform off by e (max norm) moves a point p by at most 3 e (1 + |p|), and the rmse by no more than its points
    reach = 1.0 + float(np.linalg.norm(src, axis=1).max())
    assert abs(float(rmse[0]) - a.inlier_rmse) <= 3.0 * (8.0 * dev + 1e-13) * reach


def test_icp_stopping_flags_and_batch_independence():
    """Three pairs of different sizes in one batch: identical clouds (1 iteration), nothing within the radius (identity,
    fitness 0, 1 iteration), one that uses all 30 iterations.  Every output bit is the same for a pair alone, and in a
    second run."""
    ops = _ops()
    same, _, _ = _scene(257, 300, 1)
    lone, _, _ = _scene(63, 1000, 1)
    src, tgt, _ = _scene(2500, 2311, 2, True)
    a, _ = _oracle(2500, 2311, 2, 0.5, True)
    assert a.iterations == 30, "pick another seed"
    clouds = [same, same.copy(), lone + [500.0, 0.0, 0.0], same, src, tgt]
    pairs = [[0, 1], [2, 3], [4, 5]]
    pts, off = _batch(clouds)
    out = ops.icp_point_to_point(pts, off, pairs, 0.5)
    T, fitness, rmse, iters = out
    assert iters.tolist() == [1, 1, 30]
    assert fitness.tolist()[:2] == [1.0, 0.0] and rmse[1].item() == 0.0 and rmse[0].item() < 1e-13
    assert torch.equal(T[1], torch.eye(4, dtype=torch.float64, device=DEV))
    # identical clouds: the update is the identity up to the rounding of the means of ~10 m coordinates
    assert (T[0] - torch.eye(4, dtype=torch.float64, device=DEV)).abs().max().item() < 1e-13
    again = ops.icp_point_to_point(pts, off, pairs, 0.5)
    for x, y in zip(out, again):
        assert torch.equal(x, y)
    for k, (s, t) in enumerate(pairs):
        p1, o1 = _batch([clouds[s], clouds[t]])
        alone = ops.icp_point_to_point(p1, o1, [[0, 1]], 0.5)
        for x, y in zip(out, alone):
            assert torch.equal(x[k], y[0]), k
    # a different order and a repeated pair: still the same bits
    shuffled = ops.icp_point_to_point(pts, off, [[4, 5], [0, 1], [4, 5]], 0.5)
    for x, y in zip(out, shuffled):
        assert torch.equal(x[2], y[0]) and torch.equal(x[2], y[2]) and torch.equal(x[0], y[1])


def test_icp_iteration_limit_and_init():
    ops = _ops()
    src, tgt, _ = _scene(257, 300, 1)
    pts, off = _batch([src, tgt])
    a = O.icp(src, tgt, 2.0, max_iteration=3)
    assert a.iterations == 3 and min(a.margins()[:2]) >= 1e-9
    bound = 8.0 * float(np.abs(a.T - O.icp(src, tgt, 2.0, max_iteration=3, extended=True).T).max()) + 1e-13
    T, fitness, _, iters = ops.icp_point_to_point(pts, off, [[0, 1]], 2.0, max_iteration=3)
    assert int(iters[0]) == 3 and float(fitness[0]) == a.fitness
    assert np.abs(T[0].cpu().numpy() - a.T).max() <= bound
    T0, fitness0, _, iters0 = ops.icp_point_to_point(pts, off, [[0, 1]], 2.0, max_iteration=0)
    assert int(iters0[0]) == 0 and torch.equal(T0[0], torch.eye(4, dtype=torch.float64, device=DEV))
    assert float(fitness0[0]) == O.icp(src, tgt, 2.0, max_iteration=0).fitness
    init = _motion()
    b = O.icp(src, tgt, 2.0, init=init)
    assert min(b.margins()[:2]) >= 1e-9 and b.margins()[2] >= 1e-3
    bound = 8.0 * float(np.abs(b.T - O.icp(src, tgt, 2.0, init=init, extended=True).T).max()) + 1e-13
    T, fitness, _, iters = ops.icp_point_to_point(pts, off, [[0, 1]], 2.0, init=_T(init))
    assert int(iters[0]) == b.iterations and float(fitness[0]) == b.fitness
    assert np.abs(T[0].cpu().numpy() - b.T).max() <= bound


@pytest.mark.parametrize("case", ["one_target", "one_source", "collinear"])
def test_icp_degenerate_covariance_gives_a_rotation(case):
    """M = 1, N = 1, points on a line: the covariance has rank 0 or 1 and the optimal rotation is not unique (an SVD
    would return an arbitrary one), so no parity is claimed -- only that the result is finite and a proper rotation."""
    ops = _ops()
    rng = np.random.default_rng(5)
    if case == "one_target":
        src, tgt = rng.uniform(-0.5, 0.5, (50, 3)), np.array([[0.2, 0.1, -0.1]])
    elif case == "one_source":
        src, tgt = np.array([[0.2, 0.1, -0.1]]), rng.uniform(-0.5, 0.5, (50, 3))
    else:
        t = rng.uniform(-5.0, 5.0, (80, 1))
        src = t * np.array([[1.0, 2.0, -0.5]])
        tgt = src + [0.1, 0.0, 0.05]
    pts, off = _batch([src, tgt])
    T, fitness, rmse, iters = ops.icp_point_to_point(pts, off, [[0, 1]], 2.0)
    T = T[0].cpu().numpy()
    assert np.isfinite(T).all() and np.isfinite(float(rmse[0])) and float(fitness[0]) == 1.0
    assert 1 <= int(iters[0]) <= 30
    R = T[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])


def test_front_end_refuses_what_it_cannot_place_and_answers_empty_clouds():
    ops = _ops()
    src, tgt, _ = _scene(63, 1000, 1)
    bad = src.copy()
    bad[5, 1] = np.nan
    pts, off = _batch([bad, tgt])
    with pytest.raises(ValueError, match="non-finite"):
        ops.icp_point_to_point(pts, off, [[0, 1]], 2.0)
    bad[5, 1] = np.inf
    pts, off = _batch([bad, tgt])
    with pytest.raises(ValueError, match="non-finite"):
        ops.nn_radius(pts, off, [[0, 1]], _T(np.eye(4)), 2.0)
    pts, off = _batch([src, tgt])
    with pytest.raises(ValueError):
        ops.icp_point_to_point(pts, off, [[0, 2]], 2.0)
    with pytest.raises(TypeError):
        ops.icp_point_to_point(pts.float(), off, [[0, 1]], 2.0)
    # an empty cloud in the batch: its pairs keep the initial transform, the others are registered as if alone
    pts, off = _batch([src, np.zeros((0, 3)), tgt])
    init = _T(_motion(), _motion(), np.eye(4))
    T, fitness, rmse, iters = ops.icp_point_to_point(pts, off, [[0, 1], [1, 2], [0, 2]], 2.0, init=init)
    assert torch.equal(T[:2], init[:2]) and fitness[:2].tolist() == [0.0, 0.0] and iters[:2].tolist() == [0, 0]
    p1, o1 = _batch([src, tgt])
    alone = ops.icp_point_to_point(p1, o1, [[0, 1]], 2.0)
    assert torch.equal(T[2], alone[0][0]) and int(iters[2]) == int(alone[3][0])
    idx, d2 = ops.nn_radius(pts, off, [[0, 1], [1, 2]], init[:2], 2.0)
    assert (idx == -1).all() and torch.isinf(d2).all()


def test_ttce_and_tcd_front_end(tmp_path, capsys):
    """A four-frame sequence as the reference stores it (frame_<k>_<token>.txt, an infos pickle): TTCE is the oracle's
    translation against the pose difference, TCD the float32 chamfer kernel on the world points."""
    from lidargen.metrics import temporal as TM

    ops = _ops()
    rng = np.random.default_rng(6)
    seq = tmp_path / "m" / "temporal_points" / "scene_7"
    seq.mkdir(parents=True)
    infos = []
    for k in range(4):
        token = f"{k}c0ffee{k}"
        yaw = 0.4 * k
        pos = (0.35 * k, 0.1 * k)
        infos.append({"token": token, "lidar2ego_rotation": [1.0, 0.0, 0.0, 0.0], "lidar2ego_translation": [0.9, 0.0, 1.8],
                      "ego2global_rotation": [np.cos(np.radians(yaw) / 2), 0.0, 0.0, np.sin(np.radians(yaw) / 2)],
                      "ego2global_translation": [600.0 + pos[0], 1200.0 + pos[1], 0.0]})
        pts = O.sweep(400 + 7 * k, 20 + k, pos, yaw)
        pts[0] = [0.05, 0.05, 0.05]     # a return at the sensor: dropped by load_points
        np.savetxt(seq / f"frame_{k}_{token}.txt", np.concatenate([pts, rng.uniform(size=(len(pts), 1))], axis=1))
    pkl = tmp_path / "infos.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"infos": infos}, f)
    data = {i["token"]: i for i in infos}
    files = [str(seq / f) for f in TM.natural_sorted(os.listdir(seq))]
    local = [TM.load_points(f, data) for f in files]
    assert [len(c) for c in local] == [399 + 7 * k for k in range(4)]
    a, b = O.icp(local[0], local[3], 2.0), O.icp(local[0], local[3], 2.0, extended=True)
    tie, rad, s_ratio = a.margins()
    assert tie >= 1e-9 and rad >= 1e-9 and s_ratio >= 1e-3, "pick another seed"
    dev = float(np.abs(a.T - b.T).max())
    _, t_gt = TM.get_gt_transformation(os.path.basename(files[0]), os.path.basename(files[3]), data)
    want = np.mean(np.abs(a.T[:3, 3] - t_gt))
    got = TM.calculate_single_sequence_TTCE(str(seq), data)
    assert sorted(got) == [3] and len(got[3]) == 1
    assert abs(got[3][0] - want) <= 8.0 * dev + 1e-13
    T, R, t = TM.estimate_transform_icp(local[0], local[3], threshold=2.0)
    assert T.dtype == np.float64 and np.abs(T - a.T).max() <= 8.0 * dev + 1e-13
    assert np.array_equal(R, T[:3, :3]) and np.array_equal(t, T[:3, 3])
    world = [torch.from_numpy(TM.load_points(f, data, to_global=True)).to(DEV).float()[None] for f in files]
    tcd = TM.calculate_single_sequence_TCD(str(seq), data)
    assert sorted(tcd) == [1, 2, 3] and [len(tcd[s]) for s in (1, 2, 3)] == [3, 2, 1]
    for split in (1, 2, 3):
        for i in range(4 - split):
            d1, d2, _, _ = ops.chamfer3d(world[i], world[i + split])
            assert tcd[split][i] == ((d1.mean() + d2.mean()) / 2).item()
    capsys.readouterr()
    out = TM.calculate_TTCE("m", infos_path=str(pkl), results_root=str(tmp_path))
    assert sorted(out) == [3, 4] and out[3] == got[3][0] and np.isnan(out[4])
    out = TM.calculate_TCD("m", infos_path=str(pkl), results_root=str(tmp_path))
    assert sorted(out) == [1, 2, 3, 4] and out[1] == np.mean(tcd[1]) and np.isnan(out[4])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == f"Method: m, Split: 3, TTCE: {got[3][0]:.4f} m" and lines[1] == "Method: m, Split: 4, TTCE: nan m"
    assert lines[2] == f"Method: m, Split: 1, TTCE: {np.mean(tcd[1]):.4f} m" and len(lines) == 6
