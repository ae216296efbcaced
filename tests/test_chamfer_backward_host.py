"""CPU checks around the chamfer backward: the properties of the float32 restatement the GPU test compares the device
with (tests/_chamfer_bwd_oracle.py), the refusal of CPU tensors, and the new names."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chamfer_bwd_oracle as O  # noqa: E402

F32 = np.float32
EPS = 2.0 ** -24


def _scene(kind, B, N, M, dim, seed):
    a, b = O.scene(B, N, M, kind, seed, dim)
    g1, g2 = O.grads(B, N, M, seed)
    return a, b, g1, g2, O.nearest(a, b), O.nearest(b, a)


def _reorder_bound(cnt, mag):
    """Two float32 summation orders of c terms t_i differ by at most 2 (c - 1) 2^-24 sum |t_i| to first order; 2 c covers
    the higher orders at these counts.  Per element, in float64."""
    return 2 * cnt * EPS * mag


@pytest.mark.parametrize("dim", [3, 2])
def test_restatement_matches_float64(dim):
    for kind, N, M in (("rand", 300, 70), ("dups", 64, 600), ("funnel", 700, 5), ("hubs", 300, 140), ("large", 90, 40)):
        a, b, g1, g2, i1, i2 = _scene(kind, 2, N, M, dim, 5)
        for got, (val, cnt, mag) in zip(O.backward(a, b, g1, g2, i1, i2), O.terms64(a, b, g1, g2, i1, i2)):
            assert got.dtype == F32
            assert np.all(np.abs(got.astype(np.float64) - val) <= (cnt + 1) * EPS * mag * (1 + 2.0 ** -20)), kind


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("N", [20, 33, 700])
def test_permuting_one_segment_moves_only_that_row(dim, N):
    """The sources of one segment in another order: only the row they point at may change, within the reorder bound; a
    short segment (20 serial terms), the first on the tree (33) and one of three rounds (700)."""
    a, b, g1, g2, i1, i2 = _scene("funnel", 1, N, 5, dim, 3)
    hub = 2
    assert np.all(i1 == hub)
    base = O.backward(a, b, g1, g2, i1, i2)
    perm = np.random.default_rng(1).permutation(N)
    assert not np.array_equal(perm, np.arange(N))
    # the same pairs under other source indices: rows of `a` (and what belongs to them) permuted, idx2 renamed
    inv = np.argsort(perm)
    pa, pg1, pi1, pi2 = a[:, perm], g1[:, perm], i1[:, perm], inv[i2].astype(np.int32)
    moved = O.backward(pa, b, pg1, g2, pi1, pi2)
    assert O.bits_equal(moved[0], base[0][:, perm]), "rows of grad_xyz1 carry their own terms only"
    rest = np.arange(5) != hub
    assert O.bits_equal(moved[1][:, rest], base[1][:, rest])
    _, cnt, mag = O.terms64(a, b, g1, g2, i1, i2)[1]
    err = np.abs(moved[1][:, hub].astype(np.float64) - base[1][:, hub])
    assert np.all(err <= _reorder_bound(cnt[:, hub], mag[:, hub]))
    assert cnt[0, hub, 0] == N + 1


@pytest.mark.parametrize("dim", [3, 2])
def test_same_clouds_give_zeros(dim):
    a, b, g1, g2, i1, i2 = _scene("same", 2, 300, 300, dim, 9)
    assert np.array_equal(i1, np.broadcast_to(np.arange(300), (2, 300)))
    ga, gb = O.backward(a, b, g1, g2, i1, i2)
    assert not ga.any() and not gb.any()


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("kind,N,M", [("rand", 300, 70), ("funnel", 700, 5), ("hubs", 300, 140)])
def test_gradients_sum_to_zero(dim, kind, N, M):
    """Every term enters once as t and once as -(t): the sum over all rows of both gradients is zero up to the order of
    the additions, i.e. within the sum of the elements' reorder bounds plus that of adding the rows up in float64."""
    a, b, g1, g2, i1, i2 = _scene(kind, 2, N, M, dim, 17)
    ga, gb = O.backward(a, b, g1, g2, i1, i2)
    (_, c1, m1), (_, c2, m2) = O.terms64(a, b, g1, g2, i1, i2)
    total = ga.astype(np.float64).sum(1) + gb.astype(np.float64).sum(1)
    bound = _reorder_bound(c1, m1).sum(1) + _reorder_bound(c2, m2).sum(1)
    assert total.shape == (2, dim) and np.all(np.abs(total) <= bound)
    assert np.all(bound < 1e-3 * (m1.sum(1) + m2.sum(1)))     # the bound says something


def test_documented_order_on_a_hand_example():
    """Three sources on target 0 and none on target 1, D = 2: ((+0 + d) + s_0) + s_1) + s_2 in ascending source index."""
    a = np.array([[[1.0, 2.0], [0.5, 0.25], [3.0, -1.0]]], F32)
    b = np.array([[[0.0, 0.0], [100.0, 100.0]]], F32)
    g1 = np.array([[0.1, 0.7, -0.3]], F32)
    g2 = np.array([[0.9, -0.2]], F32)
    i1 = np.zeros((1, 3), np.int32)
    i2 = np.array([[1, 2]], np.int32)
    ga, gb = O.backward(a, b, g1, g2, i1, i2)
    t = [(g1[0, k] * F32(2)) * (a[0, k] - b[0, 0]) for k in range(3)]
    want = F32(0) + (g2[0, 0] * F32(2)) * (b[0, 0] - a[0, 1])
    for k in range(3):
        want = want + -(t[k])
    assert O.bits_equal(gb[0, 0], want)
    assert O.bits_equal(gb[0, 1], F32(0) + (g2[0, 1] * F32(2)) * (b[0, 1] - a[0, 2]))
    assert O.bits_equal(ga[0, 0], F32(0) + t[0])                                         # receives nothing
    assert O.bits_equal(ga[0, 1], (F32(0) + t[1]) + -((g2[0, 0] * F32(2)) * (b[0, 0] - a[0, 1])))


def test_new_names_resolve_and_cpu_tensors_raise():
    import lidargen  # noqa: F401
    from lidarcrafter_amd import _lib, ops
    from lidargen.metrics import chamfer

    for name in ("lc_chamfer3d_bwd", "lc_chamfer2d_bwd"):
        assert name in _lib.SIGNATURES
    for fn in (chamfer.chamfer_3DFunction, chamfer.chamfer_2DFunction):
        assert issubclass(fn, torch.autograd.Function) and fn.__name__ in ("chamfer_3DFunction", "chamfer_2DFunction")
    for dim, bwd, fn, mod in ((3, ops.chamfer3d_backward, chamfer.chamfer_3DFunction, chamfer.chamfer_3DDist()),
                              (2, ops.chamfer2d_backward, chamfer.chamfer_2DFunction, chamfer.chamfer_2DDist())):
        x, y = torch.zeros(1, 4, dim), torch.zeros(1, 5, dim)
        g1, g2 = torch.zeros(1, 4), torch.zeros(1, 5)
        i1, i2 = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 5, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            bwd(x, y, g1, g2, i1, i2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn.apply(x.requires_grad_(), y)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(x, y)


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """The argument checks of the forward twins, and the int32 limit of the flat rows (callable without a GPU)."""
    import ctypes

    from lidarcrafter_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    LC_EINVAL, LC_EUNSUP = -1, -2
    for fn in (h.lc_chamfer3d_bwd, h.lc_chamfer2d_bwd):
        assert fn(p, p, p, p, p, p, 0, 4, 4, p, p, p, None) == LC_EINVAL
        assert fn(p, p, p, p, p, p, 1, 4, 0, p, p, p, None) == LC_EINVAL
        assert fn(p, p, p, p, p, None, 1, 4, 4, p, p, p, None) == LC_EINVAL
        assert fn(p, p, p, p, p, p, 1, 4, 4, None, p, p, None) == LC_EINVAL
        assert fn(p, p, p, p, p, p, 1, 4, 4, p, p, None, None) == LC_EINVAL          # no scratch
        assert fn(p, p, p, p, p, p, 65536, 40000, 4, p, p, p, None) == LC_EUNSUP     # B (N + M) >= 2^31 - 1
    # the scratch: host-only, 0 for what the entries refuse, five words per index and the sort's own storage otherwise
    size = h.lc_chamfer_bwd_scratch_bytes
    assert size(0, 4, 4) == 0 and size(1, 0, 4) == 0 and size(65536, 40000, 4) == 0
    assert size(1, 1, 1) >= 5 * 4 * 2 and size(8, 1024, 1024) >= 5 * 4 * 16384
    assert size(1, 30000, 30000) >= size(8, 1024, 1024) and size(1, 30000, 30000) < 16 << 20
