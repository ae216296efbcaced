"""Restatements for the tests of the float64 statistics (tests/test_stats_f64.py, tests/test_stats_f64_host.py): the exact
Frechet distance through the singular values of the unsquared B A^T, the squaring bound, an extended-precision squared MMD
with its forward error bound, test matrices with a prescribed spectrum, and the subset draws of the host route."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)

# (n1, n2, d) of the Frechet tests and the route each takes
FD_SHAPES = [((40, 37, 96), "gram"), ((37, 40, 96), "gram"), ((100, 90, 256), "gram"), ((200, 180, 64), "cov"),
             ((70, 66, 17), "cov"), ((64, 64, 64), "gram")]


def features(n, d, seed, shift=0.0):
    """ReLU features with correlated columns, like an extractor's."""
    rng = np.random.RandomState(seed)
    mix = rng.randn(d, d) / np.sqrt(d)
    return np.maximum(rng.randn(n, d) @ mix + 0.3 + shift, 0.0)


def centred(x):
    x = np.asarray(x, np.float64)
    return (x - x.mean(axis=0)) / np.sqrt(x.shape[0] - 1)


def exact_fd(x1, x2):
    """(E, sigma): |mu1 - mu2|^2 + |A|_F^2 + |B|_F^2 - 2 sum sigma_i(B A^T), the singular values from numpy's SVD of the
    unsquared product; sigma padded with zeros to k = min(n1, n2, d) entries (the product has that rank at most)."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    a, b = centred(x1), centred(x2)
    sig = np.linalg.svd(b @ a.T, compute_uv=False)
    k = min(x1.shape[0], x2.shape[0], x1.shape[1])
    sig = np.sort(sig)[::-1][:k]
    diff = x1.mean(axis=0) - x2.mean(axis=0)
    return float(diff @ diff + (a * a).sum() + (b * b).sum() - 2.0 * sig.sum()), sig


def squaring_floor(sig):
    """What forming the k x k Gram matrix costs: its eigenvalues sigma_i^2 are known to delta = k eps sigma_max^2, so each
    sigma_i to min(sqrt(delta), delta / (2 sigma_i)); the trace term enters the distance twice."""
    sig = np.asarray(sig, np.float64)
    k = len(sig)
    delta = k * EPS * float(sig.max()) ** 2
    with np.errstate(divide="ignore"):
        per = np.minimum(np.sqrt(delta), delta / (2.0 * sig))
    return float(2.0 * per.sum())


def replay_subsets(n1, n2, m, num_subsets):
    """The rows the host route draws, in its order: per subset first feats2's, then feats1's."""
    rows = []
    for _ in range(num_subsets):
        r2 = np.random.choice(n2, m, replace=False)
        r1 = np.random.choice(n1, m, replace=False)
        rows.append((r2, r1))
    return rows


def mmd_longdouble(feats1, feats2, rows):
    """(value, bound): the host route's expression over the given subsets in np.longdouble, and the forward bound
    (width + 8) eps (sum |within entries| / (m - 1) + 2 sum |cross entries| / m) / (num_subsets m), the entries formed
    from |x| |y| (the diagonal of the within blocks left out, as in the value)."""
    L = np.longdouble
    f1, f2 = np.asarray(feats1, np.float64).astype(L), np.asarray(feats2, np.float64).astype(L)
    width = f1.shape[1]
    total, mag = L(0), L(0)
    for r2, r1 in rows:
        m = len(r2)
        x, y = f2[r2], f1[r1]
        k = lambda u, v: (u @ v.T / L(width) + L(1)) ** 3          # noqa: E731
        within, across = k(x, x) + k(y, y), k(x, y)
        total += (within.sum() - np.diag(within).sum()) / L(m - 1) - across.sum() * L(2) / L(m)
        ax, ay = np.abs(x), np.abs(y)
        wa, ca = k(ax, ax) + k(ay, ay), k(ax, ay)
        mag += (wa.sum() - np.diag(wa).sum()) / L(m - 1) + L(2) * ca.sum() / L(m)
    S, m = len(rows), len(rows[0][0])
    return total / L(S) / L(m), float((width + 8) * EPS * mag / L(S) / L(m))


def householder_spd(k, lam, seed):
    """Q diag(lam) Q^T with Q the product of three Householder reflections."""
    rng = np.random.RandomState(seed)
    q = np.eye(k)
    for _ in range(3):
        v = rng.randn(k)
        v /= np.linalg.norm(v)
        q = q - 2.0 * np.outer(q @ v, v)
    s = (q * np.asarray(lam, np.float64)) @ q.T
    return (s + s.T) / 2.0


def spectrum(k):
    """1 down to 1e-12, geometrically."""
    return np.ones(1) if k == 1 else np.logspace(0.0, -12.0, k)
