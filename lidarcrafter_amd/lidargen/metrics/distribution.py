"""Distances between two sets of feature vectors: the two functions of the reference's `lidargen/metrics/distribution.py`
(`compute_frechet_distance`, `compute_squared_mmd`) with its arithmetic, on the host with numpy / scipy in the dtype of the
inputs (the evaluator passes float64).  That host route is the default (`device=None`) and is what the reference computes.
`calculate_frechet_distance` is the formula of the reference's `fid_score.py` (:116-167), which FSVD goes through
(eval_utils.compute_fd): the same quantity as `compute_frechet_distance` but not the same operations (a dot product for the
mean term, three separate traces, a regularised retry when the matrix square root is not finite), so it stands beside it.

`compute_squared_mmd` takes its subsets from numpy's global generator, per subset first the rows of `feats2`, then the
rows of `feats1` -- the reference's order, so a call after `np.random.seed(s)` gives the reference's number.

With `device='cuda'` (or a torch device) the three functions run in float64 on the HIP kernels of csrc/stats_f64.hip
(lidarcrafter_amd/ops_stats.py) and return a Python float: now that the feature extractors are
kernels, these statistics are the longest step of a score (seconds on the host at 2 x 2000 x 4096).  The Frechet distance
there is |mu1 - mu2|^2 + |A|_F^2 + |B|_F^2 - 2 sum_i sigma_i(B A^T) with A, B the centred sets over sqrt(n - 1): the singular
values come from one symmetric positive semi-definite k x k eigenproblem, k = min(n1, n2, d) (no square root of the
non-symmetric S1 S2, which loses half the digits when a covariance is singular).  The squared MMD uses the same rows as the
host route after the same `np.random.seed`.  Inputs may be numpy arrays or CUDA tensors, float32 or float64.  There is no
fallback: a CPU tensor or a missing GPU raises."""
import numpy as np
from scipy import linalg


def _moments(feats):
    """(mean [d], covariance [d, d]) over the rows."""
    return np.mean(feats, axis=0), np.cov(feats, rowvar=False)


def _shape2(a, name):
    shape = tuple(getattr(a, "shape", ()))
    if len(shape) != 2:
        raise ValueError(f"{name}: expected a [rows, width] matrix, got shape {shape}")
    return shape


def _check_device(device):
    import torch

    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"distribution: device={device!r} -- the device route runs on the GPU only, there is no CPU "
                           "fallback (device=None is the host route)")
    return dev


def _on_device(arrays, names, dev):
    """The inputs as contiguous float64 tensors on `dev`.  Non-finite values raise ValueError; a CPU tensor or a missing
    GPU raises RuntimeError; nothing falls back to the host."""
    import torch

    for a, name in zip(arrays, names):
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise RuntimeError(f"distribution: `{name}` is a CPU tensor -- the device route takes numpy arrays or "
                                   "CUDA(HIP) tensors, there is no CPU fallback")
        elif not np.isfinite(np.asarray(a)).all():
            raise ValueError(f"distribution: non-finite values in `{name}`")
    if not torch.cuda.is_available():
        raise RuntimeError("distribution: the device route needs the MI355X -- no CPU fallback on the hot path")
    out = []
    for a, name in zip(arrays, names):
        if isinstance(a, torch.Tensor):
            t = a.detach().to(dev, torch.float64).contiguous()
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"distribution: non-finite values in `{name}`")
        else:
            t = torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        out.append(t)
    return out


def _device_frechet(feats1, feats2, device):
    dev = _check_device(device)
    (n1, d1), (n2, d2) = _shape2(feats1, "feats1"), _shape2(feats2, "feats2")
    if d1 != d2:
        raise AssertionError(f"feature widths differ: {(d1,)} against {(d2,)}")
    if min(n1, n2) < 2:
        raise ValueError(f"distribution: fewer than 2 rows in a feature set ({n1} and {n2}): no covariance")
    from lidarcrafter_amd import ops_stats

    ops_stats.frechet_route(n1, n2, d1)                       # refuses k > 4096 before anything is uploaded
    x1, x2 = _on_device((feats1, feats2), ("feats1", "feats2"), dev)
    return ops_stats.frechet_distance(x1, x2)


def compute_frechet_distance(feats1, feats2, device=None):
    """|mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)) of the Gaussians fitted to the two sets (real part).  `device`: None
    the host route; 'cuda' or a torch device the float64 kernels (module docstring), tr (S1 S2)^(1/2) as the sum of the
    singular values of B A^T."""
    if device is not None:
        return _device_frechet(feats1, feats2, device)
    (mu1, cov1), (mu2, cov2) = _moments(feats1), _moments(feats2)
    if mu1.shape != mu2.shape or cov1.shape != cov2.shape:
        raise AssertionError(f"feature widths differ: {mu1.shape} against {mu2.shape}")
    mean_term = np.square(mu1 - mu2).sum()
    root, _ = linalg.sqrtm(np.dot(cov1, cov2), disp=False)
    return float(np.real(mean_term + np.trace(cov1 + cov2 - root * 2)))


def _poly3(u, v, width):
    """Cubic polynomial kernel matrix (u v^T / width + 1)^3."""
    return (u @ v.T / width + 1) ** 3


def _device_squared_mmd(feats1, feats2, num_subsets, max_subset_size, device):
    dev = _check_device(device)
    (n1, d1), (n2, d2) = _shape2(feats1, "feats1"), _shape2(feats2, "feats2")
    if d1 != d2:
        raise AssertionError(f"feature widths differ: {(d1,)} against {(d2,)}")
    m = min(min(n1, n2), max_subset_size)
    if m < 2:
        raise ValueError(f"distribution: fewer than 2 rows in a subset (sets of {n1} and {n2} rows, max_subset_size "
                         f"{max_subset_size}): the within-set mean is over m - 1 = {m - 1} entries")
    if d1 < 1 or num_subsets < 1:
        raise ValueError(f"distribution: width {d1}, num_subsets {num_subsets}")
    from lidarcrafter_amd import ops_stats

    x1, x2 = _on_device((feats1, feats2), ("feats1", "feats2"), dev)
    return ops_stats.squared_mmd(x1, x2, ops_stats.draw_subsets(n1, n2, m, int(num_subsets)))


def compute_squared_mmd(feats1, feats2, num_subsets=100, max_subset_size=1000, device=None):
    """Unbiased squared MMD under the cubic polynomial kernel, averaged over `num_subsets` random subsets of
    min(n1, n2, max_subset_size) rows of each set.  `device`: None the host route; 'cuda' or a torch device the fused
    float64 kernel over the same subsets (drawn on the host, in the same order, from numpy's global generator)."""
    if device is not None:
        return _device_squared_mmd(feats1, feats2, num_subsets, max_subset_size, device)
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


def _device_frechet_moments(mu1, sigma1, mu2, sigma2, device):
    import torch

    dev = _check_device(device)
    args = []
    for a, dims in ((mu1, 1), (sigma1, 2), (mu2, 1), (sigma2, 2)):
        if not isinstance(a, torch.Tensor):
            a = np.atleast_1d(a) if dims == 1 else np.atleast_2d(a)
        args.append(a)
    mu1, sigma1, mu2, sigma2 = args
    assert tuple(mu1.shape) == tuple(mu2.shape), "the two mean vectors have different lengths"
    assert tuple(sigma1.shape) == tuple(sigma2.shape), "the two covariances have different dimensions"
    d = int(mu1.shape[0])
    if len(mu1.shape) != 1 or tuple(sigma1.shape) != (d, d):
        raise ValueError(f"distribution: moments of shapes {tuple(mu1.shape)} and {tuple(sigma1.shape)}")
    from lidarcrafter_amd import ops_stats

    ops_stats.check_eig_size(d, "frechet distance (device route)")
    t = _on_device(args, ("mu1", "sigma1", "mu2", "sigma2"), dev)
    return ops_stats.frechet_distance_moments(*t)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, device=None):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) from the moments.  A non-finite square root is retried with eps
    added to both diagonals; an imaginary part of the root beyond 1e-3 on its diagonal raises, a smaller one is dropped.
    `device`: None this host route; 'cuda' or a torch device the float64 kernels: with S1 = V Lambda V^T and
    L = V sqrt(max(Lambda, 0)) the trace term is the sum of the square roots of the eigenvalues of the symmetric L^T S2 L.
    That route forms no non-symmetric square root, so the regularised retry and the imaginary-part check have no
    counterpart on it and `eps` is not used; the covariances are taken as symmetric positive semi-definite."""
    if device is not None:
        return _device_frechet_moments(mu1, sigma1, mu2, sigma2, device)
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
