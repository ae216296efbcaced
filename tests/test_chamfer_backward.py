"""GPU checks of the chamfer backward (csrc/chamfer_bwd.hip, ops.chamfer3d_backward / chamfer2d_backward and the
autograd Functions of lidargen.metrics.chamfer), D = 3 and D = 2:

  (a) bit for bit the float32 restatement tests/_chamfer_bwd_oracle.py, which adds the terms in the documented order;
  (b) D = 3: the reference's own NmDistanceGradKernel (oracle/build_ref_gpu.py, both builds), called on zero-filled
      gradients with the product's idx: bit-equal where an element has one term, within the bound of two float32
      summation orders elsewhere;
  (c) the same formula in float64;
  (d) the same bits from call to call, and for a pair alone and anywhere in a batch of 40;
  (e) autograd through chamfer_3DDist / chamfer_2DDist.

Sizes sit on the kernel's edges: 256 rows per block (255 / 256 / 257, 513, 1025: one to five blocks), a segment of
32 / 33 sources (the last one a single thread adds / the first one the block's 256-lane tree takes), 255 / 256 / 257 and
513 / 1025 sources on that tree (idle lanes, one term per lane, a second, third and fifth round)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chamfer_bwd_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 2.0 ** -24

CASES = {
    # name: (B, N, M, kind, zero rows in grad_dist)
    "rand_B1_1x1": (1, 1, 1, "rand", False),
    "rand_B1_3x1": (1, 3, 1, "rand", False),
    "rand_B3_3x257": (3, 3, 257, "rand", False),
    "rand_B1_255x256_block_edge": (1, 255, 256, "rand", False),
    "rand_B1_256x255_block_edge": (1, 256, 255, "rand", False),
    "rand_B3_257x513": (3, 257, 513, "rand", False),
    "rand_B1_513x1025": (1, 513, 1025, "rand", False),
    "rand_B40_3x3": (40, 3, 3, "rand", False),
    "rand_B40_257x255": (40, 257, 255, "rand", False),
    "rand_B3_513x257_zero_rows": (3, 513, 257, "rand", True),
    "dups_B3_513x1025": (3, 513, 1025, "dups", False),
    "dups_B1_1025x513": (1, 1025, 513, "dups", False),
    "same_B1_257": (1, 257, 257, "same", False),
    "same_B3_1025": (3, 1025, 1025, "same", False),
    "large_B3_1025x513": (3, 1025, 513, "large", False),
    "large_B1_255x257": (1, 255, 257, "large", False),
    "funnel_B3_1025x257": (3, 1025, 257, "funnel", False),
    "funnel_B1_1025x1": (1, 1025, 1, "funnel", False),
    "funnel_B40_1025x3": (40, 1025, 3, "funnel", False),
    "funnel_B1_32x3_last_serial": (1, 32, 3, "funnel", False),
    "funnel_B3_33x3_first_tree": (3, 33, 3, "funnel", False),
    "funnel_B1_255x3_idle_lane": (1, 255, 3, "funnel", False),
    "funnel_B1_256x3_full_tree": (1, 256, 3, "funnel", False),
    "funnel_B1_257x3_second_round": (1, 257, 3, "funnel", False),
    "funnel_B3_513x255_third_round": (3, 513, 255, "funnel", False),
    "hubs_B3_1025x257_three_long_rows": (3, 1025, 257, "hubs", False),
    "hubs_B1_257x255": (1, 257, 255, "hubs", False),
}
DIMS = [3, 2]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(array, dev):
    return torch.from_numpy(np.array(array)).to(dev)      # (the shared cases are read-only arrays)


def _ops(dim):
    from lidarcrafter_amd import ops as K

    return (K.chamfer3d, K.chamfer3d_backward) if dim == 3 else (K.chamfer2d, K.chamfer2d_backward)


def _device_backward(dim, a, b, g1, g2, spoil=None):
    """(idx1, idx2, grad_xyz1, grad_xyz2) as numpy, forward and backward on the device; `spoil` rewrites the forward's
    (idx1, idx2) on the host before the backward sees them."""
    fwd, bwd = _ops(dim)
    dev = torch.device("cuda:0")
    x, y = _t(a, dev), _t(b, dev)
    _, _, i1, i2 = fwd(x, y)
    if spoil is not None:
        i1, i2 = (_t(i, dev) for i in spoil(i1.cpu().numpy(), i2.cpu().numpy()))
    ga, gb = bwd(x, y, _t(g1, dev), _t(g2, dev), i1, i2)
    return [t.cpu().numpy() for t in (i1, i2, ga, gb)]


@functools.lru_cache(maxsize=None)
def _case(name, dim):
    """Everything the tests share of one case, computed once and never written to."""
    B, N, M, kind, zero = CASES[name]
    seed = B * 100003 + N * 31 + M + dim
    a, b = O.scene(B, N, M, kind, seed, dim)
    g1, g2 = O.grads(B, N, M, seed, zero)
    i1, i2, ga, gb = _device_backward(dim, a, b, g1, g2)
    out = dict(a=a, b=b, g1=g1, g2=g2, i1=i1, i2=i2, ga=ga, gb=gb, kind=kind)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", list(CASES))
def test_bit_equal_to_the_restatement(dev, name, dim):
    c = _case(name, dim)
    B, N, M = c["a"].shape[0], c["a"].shape[1], c["b"].shape[1]
    assert c["i1"].dtype == np.int32 and c["i1"].min() >= 0 and c["i1"].max() < M
    assert c["i2"].dtype == np.int32 and c["i2"].min() >= 0 and c["i2"].max() < N
    wa, wb = O.backward(c["a"], c["b"], c["g1"], c["g2"], c["i1"], c["i2"])
    assert O.bits_equal(c["ga"], wa), f"grad_xyz1: {int((c['ga'] != wa).sum())} elements differ"
    assert O.bits_equal(c["gb"], wb), f"grad_xyz2: {int((c['gb'] != wb).sum())} elements differ"
    if c["kind"] == "same":
        assert np.array_equal(c["i1"], np.broadcast_to(np.arange(N, dtype=np.int32), (B, N)))
        assert not c["ga"].any() and not c["gb"].any()
    if c["kind"] == "funnel":
        hub = M // 2
        assert np.all(c["i1"] == hub), "the scene is no funnel"
        rest = np.arange(M) != hub
        assert O.bits_equal(c["gb"][:, rest], O.direct(c["b"], c["a"], c["g2"], c["i2"])[:, rest])
    if c["kind"] == "hubs":
        assert sorted(np.unique(c["i1"])) == [5, 6, 130], "the scene has other hubs"


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", list(CASES))
def test_within_float64(dev, name, dim):
    """Against the same formula in float64 on the float32 inputs, with the product's idx.  An element with c terms t_i
    (its direct term included) takes one rounding for the subtraction and one for the product of every term (g = grad * 2
    is exact), and c - 1 for the sum, whatever its order: to first order (c + 1) * 2^-24 * sum |t_i|; the factor
    (1 + 2^-20) is for the higher orders.  Every element is compared."""
    c = _case(name, dim)
    for got, (val, cnt, mag) in zip((c["ga"], c["gb"]), O.terms64(c["a"], c["b"], c["g1"], c["g2"], c["i1"], c["i2"])):
        tol = (cnt + 1) * EPS * mag * (1 + 2.0 ** -20)
        err = np.abs(got.astype(np.float64) - val)
        assert err.shape == got.shape and np.all(err <= tol), f"max excess {(err - tol).max()}"


@pytest.fixture(scope="module")
def ref():
    """{"off"|"fc": the reference's chamfer module}; skips only while nothing was built."""
    from oracle import build_ref_gpu as R

    if R.stamp() is None:
        pytest.skip("reference GPU kernels not built: oracle/_ref/gpu_ref_stamp.json is absent "
                    "(build() makes it where the reference sources exist)")
    return {"off": R.load_gpu_ref("chamfer_3d_ref"), "fc": R.load_gpu_ref("chamfer_3d_ref_fc")}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference_gradient_kernel(dev, ref, name):
    """The reference's backward adds into the tensors it is given with float atomicAdd: zero-filled here, as its
    chamfer_3DFunction allocates them.  It launches on the null stream, so the call is synchronised on both sides.  An
    element of c terms t_i: bit-equal for c <= 1, else within 2 * c * 2^-24 * sum |t_i| (two float32 summation orders),
    computed per element in float64."""
    c = _case(name, 3)
    x, y = _t(c["a"], dev), _t(c["b"], dev)
    g1, g2 = _t(c["g1"], dev), _t(c["g2"], dev)
    i1, i2 = _t(c["i1"], dev), _t(c["i2"], dev)
    bounds = O.terms64(c["a"], c["b"], c["g1"], c["g2"], c["i1"], c["i2"])
    for build, mod in ref.items():
        ra, rb = torch.zeros_like(x), torch.zeros_like(y)
        torch.cuda.synchronize()
        mod.backward(x, y, ra, rb, g1, g2, i1, i2)
        torch.cuda.synchronize()
        for which, got, want, (_, cnt, mag) in zip(("grad_xyz1", "grad_xyz2"), (c["ga"], c["gb"]),
                                                   (ra.cpu().numpy(), rb.cpu().numpy()), bounds):
            one = cnt <= 1
            assert O.bits_equal(got[one], want[one]), f"{build}/{which}: single-term elements differ"
            tol = 2 * cnt[~one] * EPS * mag[~one]
            err = np.abs(got[~one].astype(np.float64) - want[~one])
            assert np.all(err <= tol), f"{build}/{which}: beyond a float32 reorder, max excess {(err - tol).max()}"


@pytest.mark.parametrize("dim", DIMS)
def test_an_index_outside_its_cloud_adds_no_term(dev, dim):
    """The forward writes none; the backward's contract for one (a caller's own idx): neither its direct term nor its
    scattered term exists, every other term is where it was.  Negative, == the cloud's size, far beyond it; a row of a
    long segment's sources among them."""
    B, N, M = 2, 300, 5
    a, b = O.scene(B, N, M, "funnel", 23 + dim, dim)
    g1, g2 = O.grads(B, N, M, 29 + dim)

    def spoil(i1, i2):
        i1, i2 = i1.copy(), i2.copy()
        i1[0, 5], i1[0, 6], i1[1, 299], i1[1, 0] = -1, M, 2 ** 31 - 1, -2 ** 31
        i2[0, 1], i2[1, 4] = N, -7
        return i1, i2

    i1, i2, ga, gb = _device_backward(dim, a, b, g1, g2, spoil)
    assert i1[0, 5] == -1 and i2[1, 4] == -7
    wa, wb = O.backward(a, b, g1, g2, i1, i2)
    assert O.bits_equal(ga, wa) and O.bits_equal(gb, wb)
    clean = _device_backward(dim, a, b, g1, g2)
    assert not O.bits_equal(gb, clean[3]) and np.isfinite(ga).all() and np.isfinite(gb).all()
    (_, c1, _), (_, c2, _) = O.terms64(a, b, g1, g2, i1, i2)
    assert c1[0, 5, 0] == 0 and not ga[0, 5].any()           # no direct term, and no target points at this source
    assert c2[0, M // 2, 0] == 1 + 300 - 2                   # the hub of batch entry 0 lost two sources


@pytest.mark.parametrize("dim", DIMS)
def test_same_bits_from_call_to_call(dev, dim):
    c = _case("hubs_B3_1025x257_three_long_rows", dim)
    for _ in range(2):
        i1, i2, ga, gb = _device_backward(dim, c["a"], c["b"], c["g1"], c["g2"])
        assert np.array_equal(i1, c["i1"]) and np.array_equal(i2, c["i2"])
        assert O.bits_equal(ga, c["ga"]) and O.bits_equal(gb, c["gb"])


@pytest.mark.parametrize("dim", DIMS)
def test_a_pair_has_the_same_bits_anywhere_in_a_batch(dev, dim):
    """A funnel pair (a long segment) alone, and as the first, a middle and the last entry of a batch of 40."""
    N, M = 257, 255
    a1, b1 = O.scene(1, N, M, "funnel", 11 + dim, dim)
    g1, g2 = O.grads(1, N, M, 13 + dim)
    alone = _device_backward(dim, a1, b1, g1, g2)
    batch = _case("rand_B40_257x255", dim)
    for pos in (0, 20, 39):
        a, b, h1, h2 = (batch[k].copy() for k in ("a", "b", "g1", "g2"))
        a[pos], b[pos], h1[pos], h2[pos] = a1[0], b1[0], g1[0], g2[0]
        got = _device_backward(dim, a, b, h1, h2)
        for k, (one, many) in enumerate(zip(alone, got)):
            assert O.bits_equal(one[0].astype(F32), many[pos].astype(F32)), f"output {k} at batch position {pos}"
            others = np.arange(40) != pos
            assert O.bits_equal(many[others].astype(F32), batch[("i1", "i2", "ga", "gb")[k]][others].astype(F32))


@pytest.mark.parametrize("dim", DIMS)
def test_autograd_through_the_modules(dev, dim):
    import lidargen  # noqa: F401
    from lidargen.metrics import chamfer

    module = chamfer.chamfer_3DDist() if dim == 3 else chamfer.chamfer_2DDist()
    fwd, _ = _ops(dim)
    c = _case("rand_B3_257x513", dim)
    x = _t(c["a"], dev).requires_grad_()
    y = _t(c["b"], dev).requires_grad_()
    d1, d2, i1, i2 = module(x, y)
    for i in (i1, i2):
        assert i.dtype == torch.int32 and not i.requires_grad
    assert d1.requires_grad and d2.requires_grad
    d1.retain_grad(), d2.retain_grad()
    ((d1.mean() + d2.mean()) / 2).backward()
    wa, wb = O.backward(c["a"], c["b"], d1.grad.cpu().numpy(), d2.grad.cpu().numpy(), c["i1"], c["i2"])
    assert x.grad.dtype == torch.float32 and y.grad.dtype == torch.float32
    assert O.bits_equal(x.grad.cpu().numpy(), wa) and O.bits_equal(y.grad.cpu().numpy(), wb)
    assert np.abs(wa).max() > 0 and np.abs(wb).max() > 0

    # a float64 leaf receives a float64 gradient (the module's .float() cast, differentiated by torch)
    x64 = _t(c["a"], dev).double().requires_grad_()
    e1, e2, _, _ = module(x64, y.detach())
    ((e1.mean() + e2.mean()) / 2).backward()
    assert x64.grad.dtype == torch.float64 and O.bits_equal(x64.grad.float().cpu().numpy(), wa)

    # no graph: the forward's own outputs
    with torch.no_grad():
        got = module(x, y)
    for g, w in zip(got, fwd(x.detach(), y.detach())):
        assert not g.requires_grad and g.dtype == w.dtype and torch.equal(g, w)
    for g, w in zip((d1, d2, i1, i2), got):
        assert torch.equal(g.detach(), w)

    # differentiable once (a loss that is not linear in the distances, so that the first gradient has a graph at all)
    f1, f2, _, _ = module(x, y)
    gx, = torch.autograd.grad(((f1 ** 2).mean() + (f2 ** 2).mean()) / 2, x, create_graph=True)
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()
