"""CPU restatement of the registration behind TTCE, for tests/test_icp_host.py and tests/test_icp.py:
Open3D's registration_icp with TransformationEstimationPointToPoint and default criteria (restated from its sources,
DESIGN.md section 5p) in numpy float64 over scipy's cKDTree, a brute-force radius nearest neighbour with the
smallest-index tie rule, and the synthetic sweeps the tests and devtools/ttce_time.py register.

Per iteration the loop records what decides whether another implementation can be compared with it at all: the
correspondences, how close the nearest neighbour came to a tie or to the radius, and the conditioning of the covariance."""
import numpy as np
from scipy.spatial import cKDTree


def apply_transform(T, p):
    """[N,3] -> T p + t with the operations in the kernel's order: ((T0 x + T1 y) + T2 z) + T3, separately rounded."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def sq_dist(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nn_brute(src, tgt, radius):
    """O(N M): idx [N] (the smallest index among equal minima -- numpy's argmin; -1 when d2 > radius^2), d2 [N] (inf
    likewise)."""
    idx = np.empty(len(src), dtype=np.int64)
    d2 = np.empty(len(src))
    for a in range(0, len(src), 512):
        D = sq_dist(src[a:a + 512, None, :], tgt[None, :, :])
        j = D.argmin(axis=1)
        idx[a:a + 512] = j
        d2[a:a + 512] = D[np.arange(len(j)), j]
    out = d2 > radius * radius
    idx[out] = -1
    d2[out] = np.inf
    return idx, d2


def umeyama(p, q, dtype=np.float64):
    """The rigid update of Open3D's point-to-point estimator (Eigen::umeyama without scaling) -> (4x4, S[1] / S[0])."""
    if len(p) == 0:
        return np.eye(4), np.inf
    pl, ql = p.astype(dtype), q.astype(dtype)
    n = dtype(len(p))
    mp, mq = pl.sum(axis=0) / n, ql.sum(axis=0) / n
    H = ((ql - mq)[:, :, None] * (pl - mp)[:, None, :]).sum(axis=0) / n
    U, S, Vt = np.linalg.svd(H.astype(np.float64))
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0])
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (mq - (R.astype(dtype) @ mp)).astype(np.float64)
    return T, (S[1] / S[0] if S[0] > 0 else 0.0)


class IcpResult:
    def __init__(self):
        self.T = np.eye(4)
        self.fitness = 0.0
        self.inlier_rmse = 0.0
        self.iterations = 0
        self.records = []   # one dict per pass

    def margins(self):
        """(smallest nearest / second-nearest gap, smallest distance to the radius, smallest S[1] / S[0]) over all passes."""
        return (min(r["tie_gap"] for r in self.records), min(r["radius_gap"] for r in self.records),
                min(r["s_ratio"] for r in self.records))


def _pass(tree, tgt, pts, radius, dtype):
    N, M, k = len(pts), len(tgt), min(2, len(tgt))
    _, cand = tree.query(pts, k=k, distance_upper_bound=radius + 1.0)
    cand = cand.reshape(N, k)
    D = np.full((N, k), np.inf)
    for c in range(k):
        ok = cand[:, c] < M   # the tree answers M for "none within the bound"
        D[ok, c] = sq_dist(pts[ok], tgt[cand[ok, c]])
    tie_gap = np.inf
    if k == 2:
        # the tree orders by its own (square-rooted) distances: order by the exact d2, the smaller index on equality
        swap = (D[:, 1] < D[:, 0]) | ((D[:, 1] == D[:, 0]) & (cand[:, 1] < cand[:, 0]))
        cand[swap] = cand[swap][:, ::-1]
        D[swap] = D[swap][:, ::-1]
        two = np.isfinite(D[:, 1])
        if two.any():
            tie_gap = float(np.min((D[two, 1] - D[two, 0]) / np.maximum(D[two, 1], 1e-300)))
    d2 = D[:, 0]
    seen = np.isfinite(d2)
    r2 = radius * radius
    radius_gap = float(np.min(np.abs(d2[seen] - r2) / r2)) if seen.any() else np.inf
    inl = seen & (d2 <= r2)
    idx = np.where(inl, cand[:, 0], -1).astype(np.int64)
    n = int(inl.sum())
    fitness = n / N
    rmse = float(np.sqrt(d2[inl].astype(dtype).sum() / dtype(n))) if n else 0.0
    return idx, fitness, rmse, tie_gap, radius_gap


def icp(src, tgt, radius, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, init=None, extended=False):
    """The loop of Open3D's RegistrationICP.  extended=False: as Open3D runs it -- float64 sums, the source cloud
    transformed incrementally by every update.  extended=True: every sum in np.longdouble and the composed transform
    applied to the original source (what the HIP loop does, with better sums): the distance between the two is the
    measured sensitivity of the result to summation order and to the form of the transform."""
    dtype = np.longdouble if extended else np.float64
    src, tgt = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(tgt, dtype=np.float64)
    res = IcpResult()
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    tree = cKDTree(tgt)
    pts = apply_transform(T, src)

    def one_pass():
        idx, fit, rmse, tg, rg = _pass(tree, tgt, pts, radius, dtype)
        sel = idx >= 0
        upd, s_ratio = umeyama(pts[sel], tgt[idx[sel]], dtype)
        res.records.append({"idx": idx, "tie_gap": tg, "radius_gap": rg, "s_ratio": s_ratio, "fitness": fit, "rmse": rmse})
        return fit, rmse, upd

    fit, rmse, upd = one_pass()
    for i in range(max_iteration):
        T = upd @ T
        pts = apply_transform(T, src) if extended else apply_transform(upd, pts)
        prev = (fit, rmse)
        fit, rmse, upd = one_pass()
        res.iterations = i + 1
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    res.T, res.fitness, res.inlier_rmse = T, fit, rmse
    return res


def _yaw(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def sweep(n, seed, position=(0.0, 0.0), yaw_deg=0.0, rings=16, noise=0.01, half=(30.0, 18.0), height=1.8):
    """n points of a ring-pattern sweep in the SENSOR frame: a sensor `height` above the ground plane at `position` of a
    walled yard of half-extents `half`, heading `yaw_deg`; `rings` elevations from -25 to +8 degrees, jittered azimuths,
    every ray ends on the ground or a wall; Gaussian range noise."""
    rng = np.random.default_rng(seed)
    per = -(-n // rings)
    el = np.radians(np.linspace(-25.0, 8.0, rings))[:, None] + np.zeros((1, per))
    az = (np.arange(per)[None, :] + rng.uniform(0.0, 1.0, (rings, per))) * (2.0 * np.pi / per)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)
    d = d[rng.permutation(len(d))[:n]]
    R = _yaw(yaw_deg)
    dw = d @ R.T
    o = np.array([position[0], position[1], height])
    t = np.full(len(d), 80.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, planes in ((0, (-half[0], half[0])), (1, (-half[1], half[1])), (2, (0.0,))):
            for c in planes:
                tt = (c - o[axis]) / dw[:, axis]
                t = np.where((tt > 0) & (tt < t), tt, t)
    t = t + rng.normal(0.0, noise, len(t))
    return d * t[:, None]


def scene_pair(n, m, seed, shift=(1.2, 0.3), yaw_deg=1.5):
    """(source [n,3], target [m,3], T_gt): two sweeps of the same yard from poses `shift` and `yaw_deg` apart;
    T_gt maps source coordinates to target coordinates."""
    src = sweep(n, seed, (0.0, 0.0), 0.0)
    tgt = sweep(m, seed + 1000003, shift, yaw_deg)
    R = _yaw(yaw_deg).T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.array([shift[0], shift[1], 0.0])
    return src, tgt, T
