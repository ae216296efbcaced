"""Tensor-level wrappers over the float64 statistics kernels of csrc/stats_f64.hip (include/lidarcrafter_hip.h: lc_stats_*;
DESIGN.md section 5t): the tile engine on the f64 MFMA, the fused squared-MMD kernel, centring, fixed-order reductions and
the one-sided Jacobi eigen-solver, and on top of them the three device routes of lidargen/metrics/distribution.py.  Like
ops_pointnet2.py: CUDA(HIP) contiguous tensors only, no CPU / eager-PyTorch fallback; everything is computed in float64."""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import check, lib
from .ops import _entry, _stream

_F64 = torch.float64
_I32 = torch.int32
EPS = float(np.finfo(np.float64).eps)
# Cap of the Jacobi sweeps.  The rows of S are orthogonalised, which is Jacobi on S^2: its convergence is linear for a long
# while on the wide spectra of feature Gram matrices and the count grows with k -- a numpy prototype of the scheme took 12-17
# sweeps at k = 37 ... 90, 24 at k = 400, 27 at k = 1000, and 29 at k = 129 on a spectrum graded from 1 to 1e-12; the
# MI355X 28 at the Gram matrix of 2 x 1000 x 1808 features, 30 at that of 2 x 2000 x 4096 (profiles/stats_f64.txt).
MAX_SWEEPS = 60


def limit(which: str) -> int:
    """'max_eig' (the largest matrix the Jacobi solver takes), 'reduce_scratch'."""
    return int(lib().lc_stats_limit(("max_eig", "reduce_scratch").index(which)))


def _m(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ops_stats: `{name}` must be a CUDA(HIP) tensor -- the hot path has no CPU fallback")
    if t.dtype != _F64:
        raise TypeError(f"`{name}` must be float64, got {t.dtype}")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or not t.is_contiguous():
        raise ValueError(f"ops_stats: `{name}` must be contiguous non-empty [rows, cols], got {tuple(t.shape)} strides {t.stride()}")
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the tile engine

FORMS = ("nt", "tn", "nn")


@_entry
def matmul(p: torch.Tensor, q: torch.Tensor, form: str = "nt") -> torch.Tensor:
    """'nt': p q^T (p [M, K], q [N, K]); 'tn': p^T q (p [K, M], q [K, N]); 'nn': p q (p [M, K], q [K, N]) -> [M, N] float64."""
    _m(p, "p")
    _m(q, "q")
    if form not in FORMS:
        raise ValueError(f"ops_stats.matmul: form {form!r} is not one of {FORMS}")
    if form == "nt":
        (M, K), (N, K2) = p.shape, q.shape
        ps, qs = (K, 1), (K2, 1)
    elif form == "tn":
        (K, M), (K2, N) = p.shape, q.shape
        ps, qs = (1, M), (1, N)
    else:
        (M, K), (K2, N) = p.shape, q.shape
        ps, qs = (K, 1), (1, N)
    if K != K2:
        raise ValueError(f"ops_stats.matmul[{form}]: inner lengths differ, {tuple(p.shape)} against {tuple(q.shape)}")
    out = torch.empty((M, N), device=p.device, dtype=_F64)
    check(lib().lc_stats_gemm_f64(p.data_ptr(), ps[0], ps[1], q.data_ptr(), qs[0], qs[1], out.data_ptr(), N, M, N, K, _stream()),
          "lc_stats_gemm_f64")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# centring and reductions

@_entry
def center(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [n >= 2, d] -> (mean [d], (x - mean) / sqrt(n - 1))."""
    _m(x, "x")
    n, d = x.shape
    if n < 2:
        raise ValueError(f"ops_stats.center: fewer than 2 rows ({n})")
    mean = torch.empty(d, device=x.device, dtype=_F64)
    a = torch.empty_like(x)
    check(lib().lc_stats_center_f64(x.data_ptr(), n, d, mean.data_ptr(), a.data_ptr(), _stream()), "lc_stats_center_f64")
    return mean, a


_MODES = ("sum", "sumsq", "sumsq_diff", "sum_sqrt")


def _reduce(mode: str, a: torch.Tensor, n: int, sa: int = 1, b: Optional[torch.Tensor] = None, sb: int = 1) -> torch.Tensor:
    """[1] device float64: the fixed-order sum over i < n of the mode's term of a.flat[i sa] (and b.flat[i sb])."""
    dev = a.device
    scratch = torch.empty(limit("reduce_scratch"), device=dev, dtype=_F64)
    out = torch.empty(1, device=dev, dtype=_F64)
    check(lib().lc_stats_reduce_f64(a.data_ptr(), sa, None if b is None else b.data_ptr(), sb, n, _MODES.index(mode),
                                    scratch.data_ptr(), out.data_ptr(), _stream()), "lc_stats_reduce_f64")
    return out


def _vec(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ops_stats: `{name}` must be a CUDA(HIP) tensor -- the hot path has no CPU fallback")
    if t.dtype != _F64 or not t.is_contiguous() or t.numel() < 1:
        raise ValueError(f"ops_stats: `{name}` must be contiguous non-empty float64")
    return t


@_entry
def sumsq(a: torch.Tensor) -> torch.Tensor:
    """[1]: the sum of squares of every element."""
    return _reduce("sumsq", _vec(a, "a"), a.numel())


@_entry
def sumsq_diff(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[1]: |a - b|^2 of two equally long vectors."""
    _vec(a, "a")
    _vec(b, "b")
    if a.numel() != b.numel():
        raise ValueError("ops_stats.sumsq_diff: lengths differ")
    return _reduce("sumsq_diff", a, a.numel(), 1, b, 1)


@_entry
def trace(s: torch.Tensor) -> torch.Tensor:
    """[1]: the trace of a square matrix."""
    _m(s, "s")
    if s.shape[0] != s.shape[1]:
        raise ValueError(f"ops_stats.trace: not square, {tuple(s.shape)}")
    return _reduce("sum", s, s.shape[0], s.shape[0] + 1)


@_entry
def sum_sqrt(lam: torch.Tensor) -> torch.Tensor:
    """[1]: the sum of sqrt(max(lam_i, 0))."""
    return _reduce("sum_sqrt", _vec(lam, "lam"), lam.numel())


# ---------------------------------------------------------------------------------------------------------------------
# the eigen-solver

def check_eig_size(k: int, who: str = "ops_stats.jacobi") -> int:
    """Refuses, without touching the GPU, a matrix the solver is not built for."""
    k = int(k)
    if k > 4096:
        raise NotImplementedError(f"{who}: a symmetric eigenproblem of size k = {k} is not built -- LC_STATS_MAX_EIG is 4096")
    return k


def round_robin(k: int):
    """The sweep's schedule as the kernels compute it (lc_stats_jacobi_pair, host code): a list of steps, each a list of
    pairs (p, q), p < q; the idle slot of an odd k is left out.  k >= 2."""
    k = int(k)
    n = k + (k & 1)
    pq = (ctypes.c_int * 2)()
    steps = []
    for step in range(n - 1):
        pairs = []
        for slot in range(n // 2):
            check(lib().lc_stats_jacobi_pair(k, step, slot, pq), "lc_stats_jacobi_pair")
            if pq[1] >= 0:
                pairs.append((int(pq[0]), int(pq[1])))
        steps.append(pairs)
    return steps


def jacobi_tol(k: int) -> float:
    """A pair counts as orthogonal at |w_p . w_q| <= tol |w_p| |w_q|: the rounding of a length-k dot product, sqrt(k) eps
    (at least 4 eps)."""
    return max(math.sqrt(k), 4.0) * EPS


# The second criterion of a rotation (csrc/stats_f64.hip jacobi_step_kernel): the entry (p, q) of V S V^T above ATOL times
# the root-mean-square eigenvalue |S|_F / sqrt(k) (<= lambda_max) -- two-sided Jacobi's absolute stopping rule.
ATOL = EPS


def _jacobi_rows(w: torch.Tensor, vectors: bool, max_sweeps: int):
    """In place on w [k, k]: sweeps until one rotates nothing.  -> (lam [k] the row norms, v [k, k] rows = eigenvectors or
    None, the number of sweeps run)."""
    k = w.shape[0]
    L, s = lib(), _stream()
    v = None
    if vectors:
        v = torch.empty_like(w)
        check(L.lc_stats_jacobi_init(v.data_ptr(), k, s), "lc_stats_jacobi_init")
    flag = torch.empty(1, device=w.device, dtype=_I32)
    tol = jacobi_tol(k)
    fro2 = _reduce("sumsq", w, w.numel())                 # rotations keep it: computed once
    sweeps, done = 0, False
    while not done and sweeps < max_sweeps:
        check(L.lc_stats_jacobi_sweep(w.data_ptr(), None if v is None else v.data_ptr(), k, tol, ATOL, fro2.data_ptr(),
                                      flag.data_ptr(), s),
              "lc_stats_jacobi_sweep")
        sweeps += 1
        done = int(flag.item()) == 0          # the one read-back of the sweep
    if not done:
        raise RuntimeError(f"ops_stats.jacobi: no convergence in {max_sweeps} sweeps at k = {k}")
    lam = torch.empty(k, device=w.device, dtype=_F64)
    check(L.lc_stats_jacobi_values(w.data_ptr(), k, lam.data_ptr(), s), "lc_stats_jacobi_values")
    return lam, v, sweeps


@_entry
def jacobi_eigh(s: torch.Tensor, vectors: bool = False, max_sweeps: int = MAX_SWEEPS, info: Optional[dict] = None):
    """Eigenvalues (ascending) of a symmetric positive semi-definite [k, k] matrix by one-sided Jacobi, and with `vectors`
    the matrix whose COLUMNS are the eigenvectors in that order.  The eigenvalues are the norms of the rotated rows, so an
    indefinite matrix gives absolute values.  RuntimeError when `max_sweeps` sweeps do not converge; `info['sweeps']`
    receives the number run."""
    check_eig_size(s.shape[0] if isinstance(s, torch.Tensor) and s.dim() == 2 else 0)
    _m(s, "s")
    if s.shape[0] != s.shape[1]:
        raise ValueError(f"ops_stats.jacobi_eigh: not square, {tuple(s.shape)}")
    lam, v, sweeps = _jacobi_rows(s.clone(), vectors, int(max_sweeps))
    if info is not None:
        info["sweeps"] = sweeps
    lam, order = torch.sort(lam)
    if not vectors:
        return lam
    return lam, v[order].t().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the routes of lidargen/metrics/distribution.py

def frechet_route(n1: int, n2: int, d: int) -> Tuple[str, int]:
    """('gram' | 'cov', k): which symmetric k x k matrix carries the trace term; refuses k > 4096 by name."""
    if min(n1, n2) <= d:
        return "gram", check_eig_size(min(n1, n2), "frechet distance (device route)")
    return "cov", check_eig_size(d, "frechet distance (device route)")


def _note(info: Optional[dict], **kw) -> None:
    """Records into a caller's `info`: 'sweeps' collects one count per eigenproblem, the other keys are set."""
    if info is None:
        return
    for key, val in kw.items():
        if key == "sweeps":
            info.setdefault(key, []).append(val)
        else:
            info[key] = val


def _tau(g: torch.Tensor, max_sweeps: int, info: Optional[dict] = None) -> torch.Tensor:
    lam, _, sweeps = _jacobi_rows(g, False, max_sweeps)
    _note(info, sweeps=sweeps)
    return sum_sqrt(lam)


def _tau_cov(s1: torch.Tensor, s2: torch.Tensor, max_sweeps: int, info: Optional[dict] = None) -> torch.Tensor:
    """sum sqrt(lambda_i(L^T S2 L)), S1 = V Lambda V^T, L = V sqrt(Lambda) over the numerical rank of S1: an eigenvalue at
    or below k eps lambda_max is rounding noise of the largest (numpy.linalg.matrix_rank's tolerance) and counts as 0 --
    left in, every such direction of a singular covariance would add sqrt(noise) to the sum."""
    k = s1.shape[0]
    lam, v, sweeps = _jacobi_rows(s1.clone(), True, max_sweeps)
    _note(info, sweeps=sweeps)
    lt = torch.empty_like(v)                                  # rows sqrt(lambda_i) v_i: L^T
    check(lib().lc_stats_scale_rows_f64(v.data_ptr(), lam.data_ptr(), k, k * EPS, lt.data_ptr(), _stream()),
          "lc_stats_scale_rows_f64")
    u = matmul(lt, s2, "nn")                                  # L^T S2
    return _tau(matmul(u, lt, "nt"), max_sweeps, info)        # (L^T S2) L


@_entry
def frechet_distance(x1: torch.Tensor, x2: torch.Tensor, max_sweeps: int = MAX_SWEEPS, info: Optional[dict] = None) -> float:
    """The Frechet distance of the Gaussians fitted to the rows of x1 [n1, d] and x2 [n2, d] (float64 device tensors):
    |mu1 - mu2|^2 + |A|_F^2 + |B|_F^2 - 2 sum sigma_i(B A^T).  `info` receives 'route', 'k' and the 'sweeps' of each
    eigenproblem."""
    _m(x1, "feats1")
    _m(x2, "feats2")
    route, k = frechet_route(x1.shape[0], x2.shape[0], x1.shape[1])
    _note(info, route=route, k=k)
    mu1, a = center(x1)
    mu2, b = center(x2)
    head = torch.cat([sumsq_diff(mu1, mu2), sumsq(a), sumsq(b)])
    if route == "gram":
        m = matmul(b, a, "nt")                                                 # B A^T [n2, n1]
        g = matmul(m, m, "tn") if x1.shape[0] <= x2.shape[0] else matmul(m, m, "nt")
        tau = _tau(g, max_sweeps, info)
    else:
        tau = _tau_cov(matmul(a, a, "tn"), matmul(b, b, "tn"), max_sweeps, info)
    mean_term, fa, fb, t = (float(v) for v in torch.cat([head, tau]).cpu().numpy())
    return float(mean_term + fa + fb - 2.0 * t)


@_entry
def frechet_distance_moments(mu1: torch.Tensor, s1: torch.Tensor, mu2: torch.Tensor, s2: torch.Tensor,
                             max_sweeps: int = MAX_SWEEPS) -> float:
    """The same quantity from the moments (float64 device tensors, mu [d], S [d, d]): the covariance route."""
    _m(s1, "sigma1")
    _m(s2, "sigma2")
    check_eig_size(s1.shape[0], "frechet distance (device route)")
    head = torch.cat([sumsq_diff(mu1, mu2), trace(s1), trace(s2)])
    tau = _tau_cov(s1, s2, max_sweeps)
    mean_term, ta, tb, t = (float(v) for v in torch.cat([head, tau]).cpu().numpy())
    return float(mean_term + ta + tb - 2.0 * t)


def draw_subsets(n1: int, n2: int, m: int, num_subsets: int) -> np.ndarray:
    """int32 [num_subsets, 2, m] from numpy's global generator in the host route's order: per subset first m rows of
    feats2 ([s, 0]), then m rows of feats1 ([s, 1])."""
    table = np.empty((num_subsets, 2, m), np.int32)
    for s in range(num_subsets):
        table[s, 0] = np.random.choice(n2, m, replace=False)
        table[s, 1] = np.random.choice(n1, m, replace=False)
    return table


@_entry
def mmd_sums(fx: torch.Tensor, fy: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """[num_subsets, 2] float64: per subset x = fx[table[s, 0]], y = fy[table[s, 1]] the sum of the off-diagonal entries of
    k(x, x) and k(y, y) and the sum of all entries of k(x, y), k(u, v) = (u v^T / width + 1)^3."""
    _m(fx, "fx")
    _m(fy, "fy")
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        raise RuntimeError("ops_stats: `table` must be a CUDA(HIP) tensor -- the hot path has no CPU fallback")
    if table.dtype != _I32 or table.dim() != 3 or table.shape[1] != 2 or not table.is_contiguous() or table.numel() == 0:
        raise ValueError(f"ops_stats.mmd_sums: `table` must be contiguous non-empty int32 [num_subsets, 2, m], got "
                         f"{table.dtype} {tuple(table.shape)}")
    if fx.shape[1] != fy.shape[1]:
        raise ValueError("ops_stats.mmd_sums: feature widths differ")
    S, _, m = table.shape
    partial = torch.empty(int(lib().lc_stats_mmd_partials(S, m)), device=fx.device, dtype=_F64)
    out = torch.empty((S, 2), device=fx.device, dtype=_F64)
    check(lib().lc_stats_mmd_f64(fx.data_ptr(), fx.shape[0], fy.data_ptr(), fy.shape[0], fx.shape[1], table.data_ptr(), S, m,
                                 partial.data_ptr(), out.data_ptr(), _stream()), "lc_stats_mmd_f64")
    return out


def squared_mmd(feats1: torch.Tensor, feats2: torch.Tensor, table: np.ndarray) -> float:
    """The host route's expression over the device's two sums per subset."""
    S, _, m = table.shape
    sums = mmd_sums(feats2, feats1, torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(feats1.device)).cpu().numpy()
    total = 0
    for within, across in sums:
        total += within / (m - 1) - across * 2 / m
    return float(total / S / m)
