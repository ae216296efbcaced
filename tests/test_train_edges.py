"""The UNet training kernels at their tile edges against float64.  `pytest -m gpu`.

csrc/conv_bwd.hip (weight / bias gradient of the ring convolution: exact fp32 and f16x2 split) and the GroupNorm backward
of csrc/norm.hip through the C ABI, row by row of the tables in tests/_train_edges.py; tests/test_train_edges_host.py
proves on the CPU that the tables reach every branch, that the bounds are reachable and that one missing term is
16 bounds.  Every operand is a view into a NaN-filled buffer in the row's layout, every output a view between guard
words, the scratch is NaN before every call, and every figure is printed before it is asserted
(profiles/train_edges.txt)."""
import pytest
import torch

from lidarcrafter_amd.testing import rel_l2, seeded_randn
from tests import _train_edges as TE

pytestmark = pytest.mark.gpu
NAN = float("nan")
ids = lambda c: c.name


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class WRun:
    """One row's operands on the device, and calls of either entry on them."""

    def __init__(self, dev, c, ks):
        from lidarcrafter_amd import ops as K
        from lidarcrafter_amd._lib import lib

        self.dev, self.c, self.ks, self.r = dev, c, ks, TE.wgrad_ref(c, ks)
        self.x, self.xbuf = TE.place(self.r.x, c.xl, dev)
        self.dy, self.dybuf = TE.place(self.r.dy, c.dyl, dev)
        HW = c.H * c.W
        assert self.x.data_ptr() % 16 == TE.addr_mod16(c.xl, c.Ci, HW) and self.dy.data_ptr() % 16 == TE.addr_mod16(c.dyl, c.Co, HW)
        assert self.x.stride(0) == TE.batch_stride(c.xl, c.Ci, HW) and self.dy.stride(0) == TE.batch_stride(c.dyl, c.Co, HW)
        self.n = c.Co * c.Ci * ks * ks
        self.nscratch = int(lib().lc_conv2d_ring_wgrad_scratch_elems(c.B, c.Ci, c.Co, c.H, c.W, ks))
        self.recs = None
        self.K = K

    def records(self):
        """Range records of exactly these tensors (split entry): measured, or from max|.| with the row's bound_mult."""
        if self.recs is None:
            K, c = self.K, self.c
            rx, rdy = K.PackedConv("t.x"), K.PackedConv("t.dy")
            for t, rec in ((self.x, rx), (self.dy, rdy)):
                if c.bound_mult != 1.0:
                    K.range_from_amax(t.abs().amax().reshape(1).float().contiguous(), rec, self.dev, c.bound_mult)
                else:
                    K.range_from_tensor(t, rec)
            self.recs = (rx, rdy)
        return self.recs

    def call(self, split, accumulate=0, dbias=True, prefill=None):
        """-> (rc, dw [Co, Ci, ks, ks], db [Co], guards intact).  dw / db start as NaN (accumulate = 0: the entry must
        overwrite) or as `prefill`."""
        from lidarcrafter_amd._lib import lib

        c, ks = self.c, self.ks
        scratch = torch.full((self.nscratch,), NAN, device=self.dev)
        dw, dwbuf = TE.guarded(self.n, self.dev, NAN)
        db, dbbuf = TE.guarded(c.Co, self.dev, NAN)
        if prefill is not None:
            dw.copy_(prefill[0].reshape(-1))
            db.copy_(prefill[1])
        args = (self.x.data_ptr(), self.x.stride(0), self.dy.data_ptr(), self.dy.stride(0))
        tail = (scratch.data_ptr(), dw.data_ptr(), db.data_ptr() if dbias else None, c.B, c.Ci, c.Co, c.H, c.W, ks, accumulate,
                _stream())
        if split:
            rx, rdy = self.records()
            rc = lib().lc_conv2d_ring_wgrad_f16x2(*args, rx.range_ptr(self.dev), rdy.range_ptr(self.dev), *tail)
        else:
            rc = lib().lc_conv2d_ring_wgrad(*args, *tail)
        torch.cuda.synchronize()
        G = TE.GUARD
        intact = bool(torch.isnan(dwbuf[:G]).all() and torch.isnan(dwbuf[G + self.n:]).all() and torch.isnan(dbbuf[:G]).all()
                      and torch.isnan(dbbuf[G + c.Co:]).all())
        return rc, dw.clone().reshape(c.Co, c.Ci, ks, ks), db.clone(), intact


def _check_row(dev, c, ks, split):
    run = WRun(dev, c, ks)
    r = run.r
    rc_route, route = TE.wgrad_route(c, ks, split)
    assert rc_route == 0
    bound = TE.SPLIT_BOUND if split else r.bound_f32
    bound_db = r.bound_f32                                   # the bias kernels are the same behind both entries
    rc, dw, db, intact = run.call(split)
    assert rc == 0, rc
    e_dw, z_dw, fin_dw = TE.rel_to_S(dw, r.dw, r.S_dw)
    e_db, z_db, fin_db = TE.rel_to_S(db, r.db, r.S_db)
    print(f"wgrad {c.name} ks={ks} {'split' if split else 'fp32'} route={route[:7]} e_dw={e_dw:.3e} (ref32 {r.e32_dw:.3e}, bound "
          f"{bound:.3e}) e_db={e_db:.3e} (ref32 {r.e32_db:.3e}, bound {bound_db:.3e}) nonzero-where-S=0: {z_dw}+{z_db} "
          f"signal/bound={r.signal / bound:.1f}")
    assert fin_dw and fin_db, "not finite (or not written: the outputs start as NaN)"
    assert intact, "a word next to dw / db was written"
    assert z_dw == 0 and z_db == 0, "an element whose every term is zero is not exactly 0"
    assert e_dw <= bound, (e_dw, bound)
    assert e_db <= bound_db, (e_db, bound_db)
    assert bool(torch.isnan(TE.outside(run.xbuf, run.x)).all()) and bool(torch.isnan(TE.outside(run.dybuf, run.dy)).all())
    # the same bits again (fresh NaN scratch: nothing is carried from call to call)
    rc, dw2, db2, intact = run.call(split)
    assert rc == 0 and intact and torch.equal(dw2, dw) and torch.equal(db2, db), "a second call gives other bits"
    # dbias = NULL: the same dW, db untouched
    rc, dw3, db3, intact = run.call(split, dbias=False)
    assert rc == 0 and intact and torch.equal(dw3, dw) and bool(torch.isnan(db3).all())
    # accumulate = 1: prefill + result, one float add per element
    pre = (seeded_randn(c.Co, c.Ci, ks, ks, seed=77).to(dev) * float(r.S_dw.max() ** 0.5 if float(r.S_dw.max()) > 0 else 1.0),
           seeded_randn(c.Co, seed=78).to(dev) * float(r.S_db.max() ** 0.5 if float(r.S_db.max()) > 0 else 1.0))
    rc, dw4, db4, intact = run.call(split, accumulate=1, prefill=pre)
    assert rc == 0 and intact
    assert torch.equal(dw4, pre[0] + dw), "accumulate: dW is not prefill + result"
    assert torch.equal(db4, pre[1] + db), "accumulate: db is not prefill + result"
    return run, dw, db


@pytest.mark.parametrize("ks", TE.KS)
@pytest.mark.parametrize("c", TE.WGRAD_F32 + TE.WGRAD_REFUSED, ids=ids)
def test_weight_gradient_fp32_row(dev, c, ks):
    run, _, _ = _check_row(dev, c, ks, 0)
    if c in TE.WGRAD_REFUSED:
        rc, dw, db, intact = run.call(1)
        assert rc == TE.LC_EUNSUP and intact and bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())


@pytest.mark.parametrize("ks", TE.KS)
@pytest.mark.parametrize("c", TE.WGRAD_SPLIT, ids=ids)
def test_weight_gradient_split_row(dev, c, ks):
    run, dw, db = _check_row(dev, c, ks, 1)
    r = run.r
    rc, dwf, dbf, _ = run.call(0)
    assert rc == 0
    d = TE.rel_to_S(dw, dwf.cpu().double(), r.S_dw)[0]
    print(f"wgrad {c.name} ks={ks} split against fp32: {d:.3e} (bound {TE.SPLIT_BOUND + r.bound_f32:.3e}); db bit-equal: "
          f"{torch.equal(db, dbf)}")
    assert d <= TE.SPLIT_BOUND + r.bound_f32
    assert torch.equal(db, dbf)
    assert TE.rel_to_S(dwf, r.dw, r.S_dw)[0] <= r.bound_f32


# ------------------------------------------------------------------------------------------------ GroupNorm backward
def _gn_run(dev, c, r):
    """stats + apply_train (the record) + bwd_train on the row's layouts -> dict of results (CPU) + flags."""
    from lidarcrafter_amd._lib import lib

    h = lib()
    t = r.t
    B, C, H, W, G = c.B, c.C, c.H, c.W, c.G
    HW = H * W
    x, xbuf = TE.place(t["x"], c.xl, dev)
    dy, dybuf = TE.place(t["dy"], c.dyl, dev)
    dx, dxbuf = TE.place(torch.full((B, C, H, W), NAN), c.dxl, dev)
    for v, kind in ((x, c.xl), (dy, c.dyl), (dx, c.dxl)):
        assert v.data_ptr() % 16 == TE.addr_mod16(kind, C, HW) and v.stride(0) == TE.batch_stride(kind, C, HW)
    par = {k: t[k].to(dev).contiguous() for k in TE.PARAMS if k in t}
    p = lambda k: par[k].data_ptr() if k in par else None
    part = torch.full((int(h.lc_groupnorm_partials_elems(B, C, H, W, G)),), NAN, device=dev, dtype=torch.float64)
    mr = torch.full((B, G, 2), NAN, device=dev)
    y = torch.full((B, C, H, W), NAN, device=dev)
    st = _stream()
    assert h.lc_groupnorm_stats(x.data_ptr(), x.stride(0), part.data_ptr(), B, C, H, W, G, st) == 0
    assert h.lc_groupnorm_apply_train(x.data_ptr(), x.stride(0), part.data_ptr(), p("gamma"), p("beta"), p("scale"), p("shift"), C,
                                      y.data_ptr(), C * HW, B, C, H, W, G, TE.EPS, int(c.act), mr.data_ptr(), None, st) == 0
    rows = torch.full((B, C, 2), NAN, device=dev, dtype=torch.float64)
    sizes = {"gamma": C, "beta": C, "scale": B * C, "shift": B * C}
    grads = {k: TE.guarded(sizes[k], dev, NAN) for k in par}
    gp = lambda k: grads[k][0].data_ptr() if k in grads else None
    sizes["amax"] = int(h.lc_groupnorm_amax_partials(B, C, H, W, G, 1))
    amax, amaxbuf = TE.guarded(sizes["amax"], dev, NAN)
    rc = h.lc_groupnorm_bwd_train(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), mr.data_ptr(), p("gamma"), p("beta"),
                                  p("scale"), p("shift"), C, rows.data_ptr(), dx.data_ptr(), dx.stride(0), gp("gamma"), gp("beta"),
                                  gp("scale"), gp("shift"), B, C, H, W, G, int(c.act), amax.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0, rc
    Gd = TE.GUARD
    intact = all(bool(torch.isnan(b[:Gd]).all() and torch.isnan(b[Gd + sizes[k]:]).all())
                 for k, b in [(k, b) for k, (_, b) in grads.items()] + [("amax", amaxbuf)])
    intact = intact and bool(torch.isnan(TE.outside(dxbuf, dx)).all()) and bool(torch.isnan(TE.outside(xbuf, x)).all()) and \
        bool(torch.isnan(TE.outside(dybuf, dy)).all())
    out = {k: v.clone().cpu() for k, (v, _) in grads.items()}
    out.update(x=dx.clone().cpu(), y=y.cpu(), amax=amax.clone().cpu(), intact=intact)
    return out


@pytest.mark.parametrize("c", TE.GN_CASES, ids=ids)
def test_groupnorm_backward_row(dev, c):
    r = TE.gn_ref(c)
    rc, route = TE.gn_route(c)
    assert rc == 0
    o = _gn_run(dev, c, r)
    e_dx = TE.gn_group_err(o["x"], r.ref64["x"], c.G, r.const)
    e_p = {k: TE.gn_param_err(o[k], r.ref64[k], r.S[k], k, c, r.const) for k in r.bound_p}
    e_y = rel_l2(o["y"], r.ref64["y"])
    amax_ok = bool(o["amax"].max() == o["x"].abs().max())
    print(f"gn-bwd {c.name} route={route} dx={float(e_dx.max()):.3e} (ref32 {r.e32_dx:.3e}, bound {r.bound_dx:.3e}) " +
          " ".join(f"d{k}={e_p[k]:.3e} (ref32 {r.e32_p[k]:.3e}, bound {r.bound_p[k]:.3e})" for k in e_p) +
          f" y={e_y:.3e} amax-exact: {amax_ok}")
    assert o["intact"], "a word outside dx / a parameter gradient was written, or an input changed"
    assert all(bool(torch.isfinite(o[k]).all()) for k in ("x", "amax", *e_p)), "not finite (or not written: the outputs start as NaN)"
    assert float(e_dx.max()) <= r.bound_dx, (e_dx, r.bound_dx)
    for k, e in e_p.items():
        assert e <= r.bound_p[k], (k, e, r.bound_p[k])
    assert amax_ok, (float(o["amax"].max()), float(o["x"].abs().max()))
    if c.data is None:
        assert e_y < 2e-6, e_y                       # the forward that left the record (test_groupnorm_gradients' tolerance)
    o2 = _gn_run(dev, c, r)
    for k in ("x", "amax", *e_p):
        assert torch.equal(o2[k], o[k]), f"a second call gives other bits in {k}"


# ------------------------------------------------------------------------------------------------ through autograd
class _Mod:
    def __init__(self, Co, Ci, ks, seed, dev):
        self.weight = (seeded_randn(Co, Ci, ks, ks, seed=seed) / (Ci * ks * ks) ** 0.5).to(dev).requires_grad_()
        self.bias = seeded_randn(Co, seed=seed + 1).to(dev).requires_grad_()


@pytest.mark.parametrize("H", [4, 3], ids=["H4", "H3-falls-back"])
@pytest.mark.parametrize("prec", ["f16x2", "f32"])
def test_concatenated_convs_through_autograd(dev, prec, H, monkeypatch):
    """Two AG.conv outputs concatenated into a third: the first two receive dy as channel slices of the concatenated
    gradient (uncopied: a batch stride larger than C H W).  dx, dW, db of all three against float64; H = 3: the split entry
    refuses, ConvRing.backward takes the fp32 kernel."""
    from lidarcrafter_amd import autograd as AG
    from lidarcrafter_amd._lib import lib
    from oracle import denoiser as D

    B, Ci, Ca, Cb, Co, W = 2, 5, 63, 66, 7, 64
    mods = [_Mod(Ca, Ci, 3, 301, dev), _Mod(Cb, Ci, 1, 303, dev), _Mod(Co, Ca + Cb, 3, 305, dev)]
    x = seeded_randn(B, Ci, H, W, seed=300)
    g = seeded_randn(B, Co, H, W, seed=307)
    calls = {"split": 0, "fp32": 0, "strided": 0}
    h = lib()
    f_split, f_f32 = h.lc_conv2d_ring_wgrad_f16x2, h.lc_conv2d_ring_wgrad

    def spy(name, fn):
        def wrapped(*a):
            calls[name] += 1
            co, hw = (a[11], a[12] * a[13]) if name == "split" else (a[9], a[10] * a[11])     # Co, H W of either signature
            calls["strided"] += int(a[3] > co * hw)
            return fn(*a)
        return wrapped

    monkeypatch.setattr(h, "lc_conv2d_ring_wgrad_f16x2", spy("split", f_split))
    monkeypatch.setattr(h, "lc_conv2d_ring_wgrad", spy("fp32", f_f32))
    xd = x.to(dev).requires_grad_()
    a = AG.conv(mods[0], xd, precision=prec)
    b = AG.conv(mods[1], xd, precision=prec)
    y = AG.conv(mods[2], torch.cat([a, b], dim=1), precision=prec)
    y.backward(g.to(dev))
    torch.cuda.synchronize()
    want_split = prec == "f16x2" and H % 2 == 0 and AG.TRAIN_WGRAD_PRECISION == "f16x2"
    assert (calls["split"], calls["fp32"]) == ((3, 0) if want_split else (0, 3)), calls
    assert calls["strided"] == 2, "the first two convs did not receive dy as a slice"
    # float64 reference
    ws = [(m.weight.detach().cpu().double().requires_grad_(), m.bias.detach().cpu().double().requires_grad_()) for m in mods]
    xr = x.double().requires_grad_()
    yr = D.conv_ring(torch.cat([D.conv_ring(xr, *ws[0]), D.conv_ring(xr, *ws[1])], 1), *ws[2])
    yr.backward(g.double())
    figs = {"y": rel_l2(y, yr), "dx": rel_l2(xd.grad, xr.grad)}
    for i, m in enumerate(mods):
        figs[f"dW{i}"] = rel_l2(m.weight.grad, ws[i][0].grad)
        figs[f"db{i}"] = rel_l2(m.bias.grad, ws[i][1].grad)
    print(f"autograd-cat {prec} H={H} calls={calls} " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()))
    for k, v in figs.items():
        assert v < TE.TOL_CONV_BWD, (k, v)


@pytest.mark.parametrize("sliced", [False, True], ids=["contig", "sliced"])
@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("shape", TE.RESAMPLE_SHAPES, ids=str)
def test_resample_backward_is_the_adjoint(dev, shape, up, sliced):
    """<resample(x), y> == <x, resample^T(y)> with resample^T = Resample2x.backward, the inner products in float64."""
    from lidarcrafter_amd import autograd as AG

    B, C, H, W = shape
    x = seeded_randn(B, C, H, W, seed=400 + W).to(dev).requires_grad_()
    rx = AG.resample(x, up=up)
    yv = seeded_randn(*rx.shape, seed=401 + W)
    if sliced:
        wide = torch.full((B, C + 3, *rx.shape[2:]), NAN, device=dev)
        wide[:, 1:1 + C] = yv.to(dev)
        y = wide[:, 1:1 + C]
        assert not y.is_contiguous() or B == 1
    else:
        y = yv.to(dev)
    rx.backward(y)
    lhs = float((rx.detach().double() * y.double()).sum())
    rhs = float((x.detach().double() * x.grad.double()).sum())
    scale = float(rx.detach().double().norm() * y.double().norm())
    print(f"resample-adjoint {shape} {'up' if up else 'down'} {'sliced' if sliced else 'contig'}: <Rx, y>={lhs:.9e} <x, R^T y>={rhs:.9e} "
          f"|diff| / (|Rx| |y|) = {abs(lhs - rhs) / scale:.3e}")
    assert torch.isfinite(x.grad).all()
    assert abs(lhs - rhs) <= TE.TOL_RESAMPLE * scale
