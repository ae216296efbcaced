"""GPU tests of the float64 statistics kernels (csrc/stats_f64.hip, lidarcrafter_amd/ops_stats.py) and of the device route
of lidargen/metrics/distribution.py, against tests/_stats_oracle.py.

The first test pins the fragment layout of v_mfma_f64_16x16x4_f64 on exact integer data; everything else is built on that
engine.  Sizes are the tile's edges (16, 64: one below, at, one above), more than one block, and K tails that are no
multiple of 4 or of the 16-deep LDS tile.  Every measured figure is printed before it is asserted (pytest -s shows them;
profiles/stats_f64.txt records them)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stats_oracle as O  # noqa: E402

from lidargen.metrics import distribution as D  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = O.EPS
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 130]
INNER = [1, 3, 4, 5, 31, 32, 33, 100]
_cache = {}


def _S():
    from lidarcrafter_amd import ops_stats

    return ops_stats


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the engine: fragment layout and tails, bit for bit

def _ints(shape, seed):
    return np.random.RandomState(seed).randint(-4, 5, size=shape).astype(np.float64)


def _operands(form, M, N, K, seed):
    """(p, q, the product numpy forms) for one product form."""
    if form == "nt":
        p, q = _ints((M, K), seed), _ints((N, K), seed + 1)
        return p, q, p @ q.T
    if form == "tn":
        p, q = _ints((K, M), seed), _ints((K, N), seed + 1)
        return p, q, p.T @ q
    p, q = _ints((M, K), seed), _ints((K, N), seed + 1)
    return p, q, p @ q


@pytest.mark.parametrize("K", INNER)
@pytest.mark.parametrize("form", ["nt", "tn", "nn"])
def test_engine_exact(form, K):
    """Small-integer operands: every product and sum is exact in float64, so the engine must return numpy's bits for every
    rows x columns pair of the list -- a wrong lane -> (row, column) map or a tail read past K cannot."""
    S = _S()
    for M in SIZES:
        for N in SIZES:
            p, q, want = _operands(form, M, N, K, 1000 * M + N)
            got = S.matmul(_dev(p), _dev(q), form).cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), (form, M, N, K)


@pytest.mark.parametrize("form", ["nt", "tn", "nn"])
def test_engine_row_permutation(form):
    """Permuting the rows of the result's row operand permutes the result's rows, and likewise for its columns."""
    S = _S()
    M, N, K = 130, 65, 33
    p, q, want = _operands(form, M, N, K, 7)
    rp, rq = np.random.RandomState(3).permutation(M), np.random.RandomState(4).permutation(N)
    pp = p[rp] if form != "tn" else p[:, rp]
    qq = q[rq] if form == "nt" else q[:, rq]
    assert np.array_equal(S.matmul(_dev(pp), _dev(q), form).cpu().numpy(), want[rp])
    assert np.array_equal(S.matmul(_dev(p), _dev(qq), form).cpu().numpy(), want[:, rq])


def test_engine_refusals():
    S = _S()
    a = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.matmul(a, a)
    with pytest.raises(TypeError, match="float64"):
        S.matmul(a.to(DEV).float(), a.to(DEV).float())
    with pytest.raises(ValueError, match="inner lengths differ"):
        S.matmul(a.to(DEV), torch.zeros(4, 5, dtype=torch.float64, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the squared MMD

@pytest.mark.parametrize("subsets", [1, 3])
@pytest.mark.parametrize("m", [2, 15, 16, 17, 63, 64, 65, 130])
def test_mmd_exact_inputs_give_the_host_routes_bits(m, subsets):
    """Integer features in [-2, 2] of width 16: every kernel entry is a multiple of 1 / 4096 below 2^7 and every sum is
    exact, so after the same seed the device route must return the host route's bits.  Odd m: the subset size comes from
    max_subset_size (sets of m + 7 and m + 3 rows); even m: from the smaller set (m + 5 and m rows)."""
    if m % 2:
        n1, n2, cap = m + 7, m + 3, m
    else:
        n1, n2, cap = m + 5, m, 1000
    rng = np.random.RandomState(m)
    f1 = rng.randint(-2, 3, size=(n1, 16)).astype(np.float64)
    f2 = rng.randint(-2, 3, size=(n2, 16)).astype(np.float64)
    np.random.seed(m + subsets)
    host = D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=cap)
    np.random.seed(m + subsets)
    dev = D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=cap, device=DEV)
    assert isinstance(dev, float) and dev == host, (dev, host)
    np.random.seed(m + subsets)
    assert D.compute_squared_mmd(_dev(f1), _dev(f2).float(), num_subsets=subsets, max_subset_size=cap, device=DEV) == host


@pytest.mark.parametrize("width", [1, 3, 5, 33, 100])
def test_mmd_random_features(width):
    """Random features against the np.longdouble restatement over the same subsets, to the forward bound the oracle
    computes from the inputs (tests/_stats_oracle.py mmd_longdouble)."""
    n1, n2, m, subsets = 90, 75, 70, 2
    rng = np.random.RandomState(width)
    f1, f2 = rng.randn(n1, width), rng.randn(n2, width) + 0.25
    np.random.seed(width)
    rows = O.replay_subsets(n1, n2, m, subsets)
    want, bound = O.mmd_longdouble(f1, f2, rows)
    np.random.seed(width)
    host = D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=m)
    np.random.seed(width)
    dev = D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=m, device=DEV)
    e_dev, e_host = abs(float(np.longdouble(dev) - want)), abs(float(np.longdouble(host) - want))
    print(f"[stats_f64] mmd width {width:3d} m {m}: value {float(want):.6e} device error {e_dev:.2e} host error {e_host:.2e} "
          f"bound {bound:.2e}")
    assert e_dev <= bound
    np.random.seed(width)
    assert D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=m, device=DEV) == dev      # same bits again


def test_mmd_index_outside_the_matrix_reads_a_zero_row():
    """The kernel checks every gathered row against its matrix: an index outside adds a zero row, never a read outside."""
    S = _S()
    f = _dev(np.random.RandomState(0).randint(-2, 3, size=(6, 16)))
    z = torch.cat([f, torch.zeros(1, 16, dtype=torch.float64, device=DEV)])
    bad = torch.tensor([[[0, 9, 2, -1], [1, 3, 7, 5]]], dtype=torch.int32, device=DEV)
    good = torch.tensor([[[0, 6, 2, 6], [1, 3, 6, 5]]], dtype=torch.int32, device=DEV)
    assert torch.equal(S.mmd_sums(f, f, bad), S.mmd_sums(z, z, good))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the eigen-solver

KS = [1, 2, 3, 15, 16, 17, 33, 64, 65, 129]
# Eigenvalues and residuals are asked to C k eps lambda_max, orthogonality to C k eps, C = 8: an entry of V S V^T that the
# solver leaves is below eps times the root-mean-square eigenvalue, so by Gershgorin the eigenvalues move by at most
# k eps lambda_max (1 unit); numpy's eigvalsh carries an error of the same form (1 unit); a row of V goes through
# sweeps (k - 1) rotations of eps / 2 rounding each, a random walk of sqrt(30 k) eps / 2 <= 3 k eps per entry and its maximum
# over k^2 entries a few times that.  The numpy prototype of the scheme measured 0.8 / 0.8 / 3.1 units at these sizes.
C_EIG = 8.0


def _eig_case(kind, k):
    rng = np.random.RandomState(100 + k)
    if kind == "diagonal":
        return np.diag(rng.rand(k) + 0.5 * (np.arange(k) % 3 == 0))
    if kind == "identity":
        return 2.5 * np.eye(k)
    if kind == "rank_one":
        u = rng.randn(k)
        return np.outer(u, u)
    s = O.householder_spd(k, O.spectrum(k), k)
    if kind == "zero_rows":
        dead = np.arange(k) % 4 == 1
        s[dead, :] = 0.0
        s[:, dead] = 0.0
    return s


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["diagonal", "identity", "rank_one", "spectrum", "zero_rows"])
def test_jacobi_eigenvalues(kind, k):
    S = _S()
    s = _eig_case(kind, k)
    info = {}
    lam = S.jacobi_eigh(_dev(s), info=info).cpu().numpy()
    assert lam.shape == (k,) and np.isfinite(lam).all() and (np.diff(lam) >= 0).all()
    if kind in ("diagonal", "identity"):
        assert np.array_equal(lam, np.sort(np.diag(s))) and info["sweeps"] <= 1     # nothing to rotate: exact, one look
        return
    want = np.linalg.eigvalsh(s)
    unit = k * EPS * want.max()
    err = np.abs(lam - want).max() / unit
    print(f"[stats_f64] jacobi {kind:9s} k {k:3d}: sweeps {info['sweeps']:2d} max eigenvalue error {err:.2f} k eps lambda_max")
    assert err <= C_EIG


@pytest.mark.parametrize("k", KS)
def test_jacobi_vectors(k):
    S = _S()
    s = _eig_case("spectrum", k)
    info = {}
    lam, v = S.jacobi_eigh(_dev(s), vectors=True, info=info)
    lam, v = lam.cpu().numpy(), v.cpu().numpy()
    want = np.linalg.eigvalsh(s)
    unit = k * EPS * want.max()
    err = np.abs(lam - want).max() / unit
    resid = np.abs(s @ v - v * lam).max() / unit
    orth = np.abs(v.T @ v - np.eye(k)).max() / (k * EPS)
    print(f"[stats_f64] jacobi vectors   k {k:3d}: sweeps {info['sweeps']:2d} eigenvalues {err:.2f} residual {resid:.2f} "
          f"(k eps lambda_max) orthogonality {orth:.2f} (k eps)")
    assert err <= C_EIG and resid <= C_EIG and orth <= C_EIG
    assert np.array_equal(S.jacobi_eigh(_dev(s)).cpu().numpy(), lam)           # the vectors do not change the values


def test_jacobi_sweep_cap_raises():
    """A dense matrix cannot converge in two sweeps: the solver raises and returns, it does not loop."""
    S = _S()
    r = np.random.RandomState(5).randn(65, 65)
    with pytest.raises(RuntimeError, match="no convergence in 2 sweeps"):
        S.jacobi_eigh(_dev(r @ r.T), max_sweeps=2)
    assert S.jacobi_eigh(_dev(r @ r.T)).shape == (65,)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the Frechet distance

def _fd_case(shape):
    if shape not in _cache:
        n1, n2, d = shape
        x1, x2 = O.features(n1, d, 1), O.features(n2, d, 2, shift=0.1)
        exact, sig = O.exact_fd(x1, x2)
        _cache[shape] = dict(x1=x1, x2=x2, exact=exact, floor=O.squaring_floor(sig), host=D.compute_frechet_distance(x1, x2),
                             dev=D.compute_frechet_distance(x1, x2, device=DEV))
    return _cache[shape]


@pytest.mark.parametrize("shape,route", O.FD_SHAPES)
def test_frechet_distance_against_the_exact_value(shape, route):
    """|device - E| <= max(|host - E|, floor): E from the singular values of the unsquared B A^T, floor the squaring
    bound of the exact spectrum."""
    S = _S()
    assert S.frechet_route(*shape)[0] == route
    c = _fd_case(shape)
    e_dev, e_host = abs(c["dev"] - c["exact"]), abs(c["host"] - c["exact"])
    print(f"[stats_f64] fd {shape} {route}: E {c['exact']:.12g} device error {e_dev:.2e} host error {e_host:.2e} "
          f"floor {c['floor']:.2e}")
    assert isinstance(c["dev"], float)
    assert e_dev <= max(e_host, c["floor"])


@pytest.mark.parametrize("shape,route", O.FD_SHAPES)
def test_frechet_distance_properties(shape, route):
    c = _fd_case(shape)
    x1, x2 = c["x1"], c["x2"]
    # a set against itself
    _, sig = O.exact_fd(x1, x1)
    same = D.compute_frechet_distance(x1, x1, device=DEV)
    # the moments form on numpy's moments
    mom = D.calculate_frechet_distance(x1.mean(axis=0), np.cov(x1, rowvar=False), x2.mean(axis=0), np.cov(x2, rowvar=False),
                                       device=DEV)
    print(f"[stats_f64] fd {shape} {route}: self {same:.2e} (floor {O.squaring_floor(sig):.2e}) moments - features "
          f"{abs(mom - c['dev']):.2e} (floor {c['floor']:.2e})")
    assert abs(same) <= O.squaring_floor(sig)
    assert isinstance(mom, float) and abs(mom - c["dev"]) <= c["floor"]
    # the same bits from a second call, from CUDA tensors, and from float32 values passed as float32 or as float64
    assert D.compute_frechet_distance(x1, x2, device=DEV) == c["dev"]
    assert D.compute_frechet_distance(_dev(x1), _dev(x2), device=torch.device(DEV)) == c["dev"]
    y1, y2 = x1.astype(np.float32), x2.astype(np.float32)
    assert D.compute_frechet_distance(y1, y2, device=DEV) == D.compute_frechet_distance(y1.astype(np.float64),
                                                                                       y2.astype(np.float64), device=DEV)


def test_device_route_refusals_on_device_tensors():
    x = _dev(O.features(8, 6, 1))
    bad = x.clone()
    bad[2, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite values in `feats1`"):
        D.compute_frechet_distance(bad, x, device=DEV)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        D.compute_squared_mmd(x.cpu(), x, device=DEV)
    with pytest.raises(AssertionError, match="feature widths differ"):
        D.compute_frechet_distance(x, x[:, :5].contiguous(), device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the front-ends

def test_front_ends_pass_the_device_through(capsys):
    from lidargen.metrics import eval_utils as E
    from lidargen.metrics.eval_utils import OUTPUT_TEMPLATE

    f1, f2 = O.features(40, 24, 3), O.features(33, 24, 4, shift=0.2)
    want = D.compute_frechet_distance(f1, f2, device=DEV)
    host = D.compute_frechet_distance(f1, f2)
    capsys.readouterr()
    assert E.compute_fpd(f1, f2, None, stats_device=DEV) == want
    assert OUTPUT_TEMPLATE.format("FPD ", want) in capsys.readouterr().out
    assert E.compute_frd(f1, f2, None, stats_device=DEV) == want
    assert OUTPUT_TEMPLATE.format("FRD ", want) in capsys.readouterr().out
    assert E.compute_fd(f1, f2, stats_device=DEV) == want
    # without the keyword: what they return today
    assert E.compute_fpd(f1, f2, None) == host and E.compute_frd(f1, f2, None) == host
    assert OUTPUT_TEMPLATE.format("FRD ", host) in capsys.readouterr().out
    assert E.compute_fd(f1, f2) == D.calculate_frechet_distance(f1.mean(axis=0), np.cov(f1, rowvar=False), f2.mean(axis=0),
                                                                np.cov(f2, rowvar=False))


def test_obj_scores_on_the_device(capsys):
    from lidargen.metrics import eval_utils as E
    from lidargen.metrics.eval_utils import OUTPUT_TEMPLATE

    rng = np.random.RandomState(8)
    sets = []
    for n, shift in ((14, 0.0), (11, 0.3)):
        sets.append({"car": {"pts_feat": O.features(n, 4, n, shift=shift),
                             "bev_hists": rng.poisson(0.05, size=(n, 100, 100)).astype(np.float32)}})
    fa, fb = sets[0]["car"]["pts_feat"], sets[1]["car"]["pts_feat"]
    capsys.readouterr()
    np.random.seed(0)
    out = E.compute_obj_scores(sets[0], sets[1], class_name="car", stats_device=DEV)
    text = capsys.readouterr().out
    assert out["frechet_distance"] == D.compute_frechet_distance(fa, fb, device=DEV)
    np.random.seed(0)
    assert out["squared_mmd"] == D.compute_squared_mmd(fa, fb, device=DEV)
    for name, key in (("OFD ", "frechet_distance"), ("OMMD", "squared_mmd"), ("OJSD", "jsd"), ("OBMD", "mmd")):
        assert OUTPUT_TEMPLATE.format(name, out[key]) in text
    np.random.seed(0)
    plain = E.compute_obj_scores(sets[0], sets[1], class_name="car")
    np.random.seed(0)
    assert plain["frechet_distance"] == float(D.compute_frechet_distance(fa, fb))
    assert plain["squared_mmd"] == float(D.compute_squared_mmd(fa, fb)) and plain["jsd"] == out["jsd"]
    assert plain["mmd"] == out["mmd"]
