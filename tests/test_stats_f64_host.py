"""CPU tests of the device route of lidargen/metrics/distribution.py (lidarcrafter_amd/ops_stats.py, csrc/stats_f64.hip):
everything that is decided on the host -- the Jacobi schedule (the library's own host code), the route per shape, the subset
table, the unchanged host route behind `device=None`, and the refusals, none of which touches a GPU."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stats_oracle as O  # noqa: E402

from lidargen.metrics import distribution as D  # noqa: E402


def _S():
    from lidarcrafter_amd import ops_stats

    return ops_stats


@pytest.mark.parametrize("k", [2, 3, 4, 5, 16, 17, 129])
def test_round_robin_covers_every_pair_once(k):
    steps = _S().round_robin(k)
    assert len(steps) == k - 1 + (k & 1)
    seen = set()
    for pairs in steps:
        assert len(pairs) == k // 2                        # an odd k idles one row per step
        rows = [r for pq in pairs for r in pq]
        assert len(set(rows)) == len(rows), "pairs of one step share a row"
        for p, q in pairs:
            assert 0 <= p < q < k
            assert (p, q) not in seen
            seen.add((p, q))
    assert len(seen) == k * (k - 1) // 2


def test_round_robin_refuses_bad_arguments():
    import ctypes

    from lidarcrafter_amd import _lib

    h, pq = _lib.lib(), (ctypes.c_int * 2)()
    assert h.lc_stats_jacobi_pair(1, 0, 0, pq) == -1 and h.lc_stats_jacobi_pair(4, 3, 0, pq) == -1
    assert h.lc_stats_jacobi_pair(4, 0, 2, pq) == -1 and h.lc_stats_jacobi_pair(5, 4, 2, pq) == 0
    assert h.lc_stats_limit(0) == 4096 and h.lc_stats_mmd_partials(3, 130) == 3 * 3 * 9


@pytest.mark.parametrize("shape,route", O.FD_SHAPES)
def test_route_per_shape(shape, route):
    n1, n2, d = shape
    assert _S().frechet_route(n1, n2, d) == (route, min(n1, n2, d))


def test_subset_table_holds_the_host_routes_rows():
    S = _S()
    n1, n2, m, subsets = 23, 17, 9, 4
    np.random.seed(11)
    table = S.draw_subsets(n1, n2, m, subsets)
    np.random.seed(11)
    rows = O.replay_subsets(n1, n2, m, subsets)
    assert table.dtype == np.int32 and table.shape == (subsets, 2, m)
    for s, (r2, r1) in enumerate(rows):
        assert np.array_equal(table[s, 0], r2) and np.array_equal(table[s, 1], r1)
    # and those are the rows the host route multiplies: its value from the replayed rows, bit for bit
    f1, f2 = O.features(n1, 5, 1), O.features(n2, 5, 2)
    total = 0
    for r2, r1 in rows:
        x, y = f2[r2], f1[r1]
        within = D._poly3(x, x, 5) + D._poly3(y, y, 5)
        total += (within.sum() - np.diag(within).sum()) / (m - 1) - D._poly3(x, y, 5).sum() * 2 / m
    np.random.seed(11)
    assert D.compute_squared_mmd(f1, f2, num_subsets=subsets, max_subset_size=m) == float(total / subsets / m)


def test_device_none_is_the_host_route():
    f1, f2 = O.features(30, 12, 3), O.features(26, 12, 4, shift=0.2)
    assert D.compute_frechet_distance(f1, f2, device=None) == D.compute_frechet_distance(f1, f2)
    np.random.seed(5)
    a = D.compute_squared_mmd(f1, f2, num_subsets=3, max_subset_size=20)
    np.random.seed(5)
    assert D.compute_squared_mmd(f1, f2, num_subsets=3, max_subset_size=20, device=None) == a
    mom = (f1.mean(axis=0), np.cov(f1, rowvar=False), f2.mean(axis=0), np.cov(f2, rowvar=False))
    assert D.calculate_frechet_distance(*mom, device=None) == D.calculate_frechet_distance(*mom)
    for fn in (D.compute_frechet_distance, D.compute_squared_mmd, D.calculate_frechet_distance):
        assert inspect.signature(fn).parameters["device"].default is None


def test_front_ends_default_to_the_host_route(capsys):
    from lidargen.metrics import eval_utils as E

    f1, f2 = O.features(30, 12, 3), O.features(26, 12, 4, shift=0.2)
    for name in ("compute_fd", "compute_fpd", "compute_frd", "compute_fsvd", "compute_fpvd", "compute_frid",
                 "compute_obj_scores"):
        assert inspect.signature(getattr(E, name)).parameters["stats_device"].default is None
    assert E.compute_fd(f1, f2) == D.calculate_frechet_distance(f1.mean(axis=0), np.cov(f1, rowvar=False), f2.mean(axis=0),
                                                                np.cov(f2, rowvar=False))
    assert E.compute_fpd(f1, f2, None) == D.compute_frechet_distance(f1, f2)
    assert E.compute_frd(f1, f2, None) == D.compute_frechet_distance(f1, f2)


def test_refusals_by_message():
    f = O.features(8, 6, 1)
    with pytest.raises(AssertionError, match="feature widths differ"):
        D.compute_frechet_distance(f, f[:, :5], device="cuda")
    with pytest.raises(AssertionError, match="feature widths differ"):      # the host route's, unchanged
        D.compute_frechet_distance(f, f[:, :5])
    with pytest.raises(AssertionError, match="feature widths differ"):
        D.compute_squared_mmd(f, f[:, :5], device="cuda")
    bad = f.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite values in `feats2`"):
        D.compute_frechet_distance(f, bad, device="cuda")
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite values in `feats1`"):
        D.compute_squared_mmd(bad, f, device="cuda")
    with pytest.raises(ValueError, match="fewer than 2 rows"):
        D.compute_frechet_distance(f[:1], f, device="cuda")
    with pytest.raises(ValueError, match="fewer than 2 rows"):
        D.compute_squared_mmd(f, f, max_subset_size=1, device="cuda")
    with pytest.raises(RuntimeError, match="CPU tensor"):
        D.compute_frechet_distance(torch.from_numpy(f), f, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.compute_frechet_distance(f, f, device="cpu")
    cov = np.cov(f, rowvar=False)
    with pytest.raises(AssertionError, match="different lengths"):
        D.calculate_frechet_distance(f.mean(axis=0), cov, f.mean(axis=0)[:5], cov, device="cuda")
    with pytest.raises(ValueError, match="non-finite values in `sigma1`"):
        D.calculate_frechet_distance(f.mean(axis=0), cov * np.nan, f.mean(axis=0), cov, device="cuda")


def test_eigenproblem_above_4096_is_refused_by_name():
    S = _S()
    assert S.limit("max_eig") == 4096
    S.check_eig_size(4096)
    with pytest.raises(NotImplementedError, match="k = 4097 is not built"):
        S.frechet_route(5000, 4097, 4097)
    with pytest.raises(NotImplementedError, match="k = 4097 is not built"):
        S.frechet_route(4097, 5000, 8000)
    wide = np.broadcast_to(np.zeros((1, 1), np.float32), (4097, 4097))      # no memory behind it
    with pytest.raises(NotImplementedError, match="k = 4097 is not built"):
        D.compute_frechet_distance(wide, wide, device="cuda")
    with pytest.raises(NotImplementedError, match="k = 4097 is not built"):
        D.calculate_frechet_distance(wide[0], wide, wide[0], wide, device="cuda")
    with pytest.raises(NotImplementedError, match="k = 4097 is not built"):
        S.jacobi_eigh(torch.zeros(4097, 1).expand(4097, 4097))


def test_device_route_without_a_gpu_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    f = O.features(8, 6, 1)
    cov = np.cov(f, rowvar=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.compute_frechet_distance(f, f, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.compute_squared_mmd(f, f, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.calculate_frechet_distance(f.mean(axis=0), cov, f.mean(axis=0), cov, device="cuda")
