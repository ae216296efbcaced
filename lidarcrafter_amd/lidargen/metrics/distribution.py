"""Distances between two sets of feature vectors: the two functions of the reference's `lidargen/metrics/distribution.py`
(`compute_frechet_distance`, `compute_squared_mmd`) with its arithmetic, on the host with numpy / scipy in the dtype of the
inputs (the evaluator passes float64).  These are [n, 1808] matrices once per evaluation, not a hot path: no kernel.
`calculate_frechet_distance` is the formula of the reference's `fid_score.py` (:116-167), which FSVD goes through
(eval_utils.compute_fd): the same quantity as `compute_frechet_distance` but not the same operations (a dot product for the
mean term, three separate traces, a regularised retry when the matrix square root is not finite), so it stands beside it.

`compute_squared_mmd` takes its subsets from numpy's global generator, per subset first the rows of `feats2`, then the
rows of `feats1` -- the reference's order, so a call after `np.random.seed(s)` gives the reference's number."""
import numpy as np
from scipy import linalg


def _moments(feats):
    """(mean [d], covariance [d, d]) over the rows."""
    return np.mean(feats, axis=0), np.cov(feats, rowvar=False)


def compute_frechet_distance(feats1, feats2):
    """|mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)) of the Gaussians fitted to the two sets (real part)."""
    (mu1, cov1), (mu2, cov2) = _moments(feats1), _moments(feats2)
    if mu1.shape != mu2.shape or cov1.shape != cov2.shape:
        raise AssertionError(f"feature widths differ: {mu1.shape} against {mu2.shape}")
    mean_term = np.square(mu1 - mu2).sum()
    root, _ = linalg.sqrtm(np.dot(cov1, cov2), disp=False)
    return float(np.real(mean_term + np.trace(cov1 + cov2 - root * 2)))


def _poly3(u, v, width):
    """Cubic polynomial kernel matrix (u v^T / width + 1)^3."""
    return (u @ v.T / width + 1) ** 3


def compute_squared_mmd(feats1, feats2, num_subsets=100, max_subset_size=1000):
    """Unbiased squared MMD under the cubic polynomial kernel, averaged over `num_subsets` random subsets of
    min(n1, n2, max_subset_size) rows of each set."""
    width = feats1.shape[1]
    n1, n2 = feats1.shape[0], feats2.shape[0]
    m = min(min(n1, n2), max_subset_size)
    total = 0
    for _ in range(num_subsets):
        x = feats2[np.random.choice(n2, m, replace=False)]
        y = feats1[np.random.choice(n1, m, replace=False)]
        within = _poly3(x, x, width) + _poly3(y, y, width)
        across = _poly3(x, y, width)
        total += (within.sum() - np.diag(within).sum()) / (m - 1) - across.sum() * 2 / m
    return float(total / num_subsets / m)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) from the moments.  A non-finite square root is retried with eps
    added to both diagonals; an imaginary part of the root beyond 1e-3 on its diagonal raises, a smaller one is dropped."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, "the two mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "the two covariances have different dimensions"
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)
