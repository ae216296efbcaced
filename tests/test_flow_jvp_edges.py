"""The MeanFlow tangent kernels at their tile edges, clamps and one-hot rows against float64.  `pytest -m gpu`.

csrc/flow_jvp.hip (GroupNorm JVP statistics and apply, q / k RMSNorm JVP and backward with its dg reduce, flash attention
with its tangent) through the C ABI, row by row of the tables in tests/_flow_jvp_edges.py; tests/test_flow_jvp_edges_host.py
proves on the CPU that the tables reach every branch, that the references are right and that a designed defect is 16
bounds.  Every operand is a view into a NaN-filled buffer in the row's layout, every output a NaN-filled view between
guard words (a sentinel that survives inside an output, or a word that changes outside one, fails the row), the scratch is
NaN before every call, and every figure is printed before it is asserted (profiles/flow_jvp_edges.txt)."""
import pytest
import torch

from lidarcrafter_amd.testing import rel_l2
from tests import _flow_jvp_edges as FE

pytestmark = pytest.mark.gpu
NAN = float("nan")
ids = lambda c: c.name


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, dev):
    """A NaN-filled n-float output between NaN guards -> (view, intact()): intact() after the call: the guards are NaN."""
    v, buf = FE.guarded(n, dev, NAN)
    G = FE.GUARD
    return v, lambda: bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all())


# ------------------------------------------------------------------------------------------------ q / k RMSNorm
def _place_cm(values, kind, dev):
    """[B, C, L] (CPU float32) inside a NaN-filled buffer -> (view, buffer): "contig"; "qkv": the middle third of a
    [B, 3 C, L] tensor; "cs": a channel stride of L + 3."""
    B, C, L = values.shape
    if kind == "contig":
        v, buf = FE.place(values[:, :, None, :], "contig", dev)
        return v[:, :, 0, :], buf
    G = FE.GUARD
    bs, cs, off = (3 * C * L, L, C * L) if kind == "qkv" else (C * (L + 3), L + 3, 0)
    buf = torch.full((2 * G + off + (B - 1) * bs + (C - 1) * cs + L,), NAN, dtype=torch.float32, device=dev)
    view = buf.as_strided((B, C, L), (bs, cs, 1), G + off)
    view.copy_(values)
    return view, buf


@pytest.mark.parametrize("c", FE.QK_CASES, ids=ids)
def test_qk_norm_row(dev, c):
    from lidarcrafter_amd._lib import lib

    h = lib()
    r = FE.qk_ref(c)
    rc, route = FE.qk_route(c)
    assert rc == 0
    B, C, L = c.B, c.heads * c.d, c.L
    x, xbuf = _place_cm(r.t["x"], c.xl, dev)
    dx, dxbuf = FE.place(r.t["dx"][:, :, None, :], "slice_lo", dev)          # a batch stride above C L
    gy, gybuf = FE.place(r.t["gy"][:, :, None, :], "off1", dev)              # one float into its buffer
    g = r.t["g"].to(dev)
    n = B * C * L
    st = _stream()

    def jvp(with_dx, with_y):
        y, y_ok = _out(n, dev)
        dy, dy_ok = _out(n, dev)
        rc = h.lc_qk_norm_cm_jvp(x.data_ptr(), x.stride(0), x.stride(1), dx.data_ptr() if with_dx else None, dx.stride(0), dx.stride(1),
                                 g.data_ptr(), y.data_ptr() if with_y else None, C * L, L, dy.data_ptr() if with_dx else None, C * L, L,
                                 B, c.heads, c.d, L, st)
        torch.cuda.synchronize()
        assert rc == 0 and y_ok() and dy_ok(), "refused, or a word next to y / dy was written"
        return y.clone().reshape(B, C, L), dy.clone().reshape(B, C, L)

    def bwd():
        gx, gx_ok = _out(n, dev)
        dg, dg_ok = _out(1, dev)
        part = torch.full((route[2],), NAN, dtype=torch.float64, device=dev)
        rc = h.lc_qk_norm_cm_bwd(x.data_ptr(), x.stride(0), x.stride(1), gy.data_ptr(), gy.stride(0), gy.stride(1), g.data_ptr(),
                                 gx.data_ptr(), C * L, L, part.data_ptr(), dg.data_ptr(), B, c.heads, c.d, L, st)
        torch.cuda.synchronize()
        assert rc == 0 and gx_ok() and dg_ok(), "refused, or a word next to gx / dg was written"
        assert bool(torch.isfinite(part).all()), "a partial of dg was not written"
        return gx.clone().reshape(B, C, L), float(dg[0])

    y, dy = jvp(True, True)
    gx, dg = bwd()
    e_y, z_y = FE.qk_token_err(y, r.y, c.heads)
    e_dy, z_dy = FE.qk_token_err(dy, r.dy, c.heads, r.scale_dy)
    e_gx, z_gx = FE.qk_token_err(gx, r.gx, c.heads, r.scale_gx)
    e_dg = abs(dg - r.dg) / r.S_dg
    print(f"flow-jvp-edges qk {c.name} route={route} y={float(e_y.max()):.3e} dy={float(e_dy.max()):.3e} gx={float(e_gx.max()):.3e} "
          f"(ref32 {r.e32:.3e}, bound {r.bound:.3e}) dg={e_dg:.3e} (ref32 {r.e32_dg:.3e}, bound {r.bound_dg:.3e}) "
          f"nonzero-where-ref=0: {z_y}+{z_dy}+{z_gx}")
    assert all(bool(torch.isfinite(a).all()) for a in (y, dy, gx)) and dg == dg, "not finite (or not written: the outputs start as NaN)"
    assert z_y == 0 and z_dy == 0 and z_gx == 0, "a token whose reference is all zero is not exactly zero"
    for e in (e_y, e_dy, e_gx):
        assert float(e.max()) <= r.bound, (float(e.max()), r.bound)
    assert e_dg <= r.bound_dg, (e_dg, r.bound_dg)
    # the primal-only form (dx == NULL) and the tangent-only form (y == NULL): the same bits, the other output untouched
    y2, dy2 = jvp(False, True)
    assert torch.equal(y2, y) and bool(torch.isnan(dy2).all())
    y3, dy3 = jvp(True, False)
    assert torch.equal(dy3, dy) and bool(torch.isnan(y3).all())
    gx2, dg2 = bwd()
    assert torch.equal(gx2, gx) and dg2 == dg, "a second call gives other bits"
    # the launcher of autograd.py in its want_y = False form, on the same strided views
    from lidarcrafter_amd import autograd as AG

    _, y_none, dy_py = AG._qk_norm_launch(x, g, c.heads, dx[:, :, 0, :], want_y=False)
    assert y_none is None and torch.equal(dy_py, dy)
    for buf, v in ((xbuf, x), (dxbuf, dx), (gybuf, gy)):
        assert bool(torch.isnan(FE.outside(buf, v)).all()), "an operand's surroundings changed"
    assert torch.equal(x.cpu(), r.t["x"]) and torch.equal(dx.cpu()[:, :, 0], r.t["dx"]) and torch.equal(gy.cpu()[:, :, 0], r.t["gy"])


# ------------------------------------------------------------------------------------------------ GroupNorm JVP
def _gn_run(dev, c, r):
    from lidarcrafter_amd._lib import lib

    h = lib()
    t = r.t
    B, C, H, W, G = c.B, c.C, c.H, c.W, c.G
    HW = H * W
    x, xbuf = FE.place(t["x"], c.xl, dev)
    dx, dxbuf = FE.place(t["dx"], c.dxl, dev)
    for v, kind in ((x, c.xl), (dx, c.dxl)):
        assert v.data_ptr() % 16 == FE.addr_mod16(kind, C, HW) and v.stride(0) == FE.batch_stride(kind, C, HW)
    par = {k: t[k].to(dev).contiguous() for k in ("gamma", "beta", "scale", "shift", "dscale", "dshift") if k in t}
    p = lambda k: par[k].data_ptr() if k in par else None
    rc, route = FE.gn_route(c)
    assert rc == 0
    nslots = int(h.lc_groupnorm_amax_partials(B, C, H, W, G, 0))
    assert nslots == route[7]
    part = torch.full((int(h.lc_groupnorm_jvp_partials_elems(B, C, H, W, G)),), NAN, device=dev, dtype=torch.float64)
    y, y_ok = _out(B * C * HW, dev)
    dy, dy_ok = _out(B * C * HW, dev)
    mr, mr_ok = _out(B * G * 2, dev)
    am, am_ok = _out(nslots, dev)
    dam, dam_ok = _out(nslots, dev)
    st = _stream()
    assert h.lc_groupnorm_jvp_stats(x.data_ptr(), x.stride(0), dx.data_ptr(), dx.stride(0), part.data_ptr(), B, C, H, W, G, st) == 0
    assert h.lc_groupnorm_jvp_apply_train(x.data_ptr(), x.stride(0), dx.data_ptr(), dx.stride(0), part.data_ptr(), p("gamma"), p("beta"),
                                          p("scale"), p("shift"), p("dscale"), p("dshift"), C, y.data_ptr(), C * HW, dy.data_ptr(),
                                          C * HW, B, C, H, W, G, FE.EPS, int(c.act), mr.data_ptr(), am.data_ptr(), dam.data_ptr(), st) == 0
    # GroupNormAct's statistics and apply on the same view
    part0 = torch.full((int(h.lc_groupnorm_partials_elems(B, C, H, W, G)),), NAN, device=dev, dtype=torch.float64)
    mr0 = torch.full((B * G * 2,), NAN, device=dev)
    y0 = torch.full((B * C * HW,), NAN, device=dev)
    assert h.lc_groupnorm_stats(x.data_ptr(), x.stride(0), part0.data_ptr(), B, C, H, W, G, st) == 0
    assert h.lc_groupnorm_apply_train(x.data_ptr(), x.stride(0), part0.data_ptr(), p("gamma"), p("beta"), p("scale"), p("shift"), C,
                                      y0.data_ptr(), C * HW, B, C, H, W, G, FE.EPS, int(c.act), mr0.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    intact = y_ok() and dy_ok() and mr_ok() and am_ok() and dam_ok() and bool(torch.isnan(FE.outside(xbuf, x)).all()) and \
        bool(torch.isnan(FE.outside(dxbuf, dx)).all()) and torch.equal(x.cpu(), t["x"]) and torch.equal(dx.cpu(), t["dx"])
    return dict(y=y.clone().reshape(B, C, H, W), dy=dy.clone().reshape(B, C, H, W), mr=mr.clone(), mr0=mr0, y0=y0.reshape(B, C, H, W),
                am=am.clone().reshape(B, -1), dam=dam.clone().reshape(B, -1), part=part, intact=intact, route=route)


@pytest.mark.parametrize("c", FE.GN_CASES, ids=ids)
def test_groupnorm_jvp_row(dev, c):
    r = FE.gn_ref(c)
    o = _gn_run(dev, c, r)
    y, dy = o["y"], o["dy"]
    e_y = FE.gn_group_err(y, r.y, c.G, r.skip_y)
    e_dy = FE.gn_group_err(dy, r.dy, c.G, r.skip_dy)
    amax_ok = torch.equal(o["am"].amax(1), y.abs().amax((1, 2, 3))) and torch.equal(o["dam"].amax(1), dy.abs().amax((1, 2, 3)))
    mr_ok = torch.equal(o["mr"], o["mr0"])
    line = (f"flow-jvp-edges gn {c.name} route={o['route']} y={float(e_y.max()):.3e} (ref32 {r.e32_y:.3e}, bound {r.bound_y:.3e}) "
            f"dy={float(e_dy.max()):.3e} (ref32 {r.e32_dy:.3e}, bound {r.bound_dy:.3e}) mean_rstd bit-equal: {mr_ok} "
            f"y against GroupNormAct: {rel_l2(y, o['y0']):.1e} amax slots {o['am'].numel()} exact: {amax_ok}")
    const = None
    if r.const is not None:
        cpg = c.C // c.G
        sl = slice(r.const * cpg, (r.const + 1) * cpg)
        cy, cdy = FE.gn_const_closed(r.t, c, r.const)
        by, bdy = FE.gn_const_bounds(r.t, c, r.const)
        dev_y = (y[:, sl].double().cpu() - cy[:, :, None, None]).abs().amax((2, 3))
        dev_dy = (dy[:, sl].double().cpu() - cdy[:, :, None, None]).abs().amax((2, 3))
        const = (dev_y, by, dev_dy, bdy)
        line += f" constant group: |y - closed| / bound {float((dev_y / by).max()):.2e}"
        if r.skip_dy is not None:
            line += f" |dy - closed| / bound {float((dev_dy / bdy).max()):.2e}"
    print(line)
    assert o["intact"], "a word outside an output was written, or an operand or its surroundings changed"
    for k in ("y", "dy", "mr", "am", "dam", "part"):
        assert bool(torch.isfinite(o[k]).all()), f"{k}: not finite (or not written: the outputs start as NaN)"
    assert float(e_y.max()) <= r.bound_y, (e_y, r.bound_y)
    assert float(e_dy.max()) <= r.bound_dy, (e_dy, r.bound_dy)
    assert mr_ok, "mean_rstd is not GroupNormAct's"
    assert bool((o["am"] >= 0).all()) and bool((o["dam"] >= 0).all())
    assert amax_ok, "the maximum over a sample's slots is not max|y[b]| / max|dy[b]| of the kernel's own outputs"
    if const is not None:
        assert bool((const[0] <= const[1]).all()), "the constant group's y is off its closed form"
        if r.skip_dy is not None:
            assert bool((const[2] <= const[3]).all()), "the constant group's dy is off its closed form"
    o2 = _gn_run(dev, c, r)
    for k in ("y", "dy", "mr", "am", "dam"):
        assert torch.equal(o2[k], o[k]), f"a second call gives other bits in {k}"


@pytest.mark.parametrize("name,f", FE.GN_CHAINED, ids=[n for n, _ in FE.GN_CHAINED])
def test_groupnorm_jvp_feeds_the_tangent_conv(dev, name, f):
    """group_norm_jvp -> conv_tangent: the f16x2 range of the tangent conv comes from the partial maxima of |dy| the apply
    pass left, at |dy| ~ 1e3 |y| and ~ 1e-3 |y|; against the float64 bias-free convolution of the float64 dy."""
    from lidarcrafter_amd import autograd as AG
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    assert AG.PRODUCER_AMAX and AG.TRAIN_CONV_PRECISION == "f16x2", "the range-from-maxima route is switched off"
    t, w = FE.gn_chained_operands(name, f)
    gn = torch.nn.GroupNorm(8, t["x"].shape[1], eps=FE.EPS).to(dev)
    with torch.no_grad():
        gn.weight.copy_(t["gamma"]), gn.bias.copy_(t["beta"])
    x = t["x"].to(dev).requires_grad_()
    y, dy = AG.group_norm_jvp(gn, x, t["dx"].to(dev), act=True)
    tag_y, tag_dy = AG._amax_of(y), AG._amax_of(dy)
    assert tag_y is not None and tag_dy is not None, "the partial maxima did not reach the tensors"
    assert torch.equal(tag_y[0].max(), y.detach().abs().max()) and torch.equal(tag_dy[0].max(), dy.abs().max())
    holder = K.PackedConv("t.jvp")
    dz = AG.conv_tangent(w.to(dev), holder, dy)
    y64, dy64 = FE.gn_closed(t, 8, True, torch.float64)
    ref = D.conv_ring(dy64, w.double(), None)
    e = rel_l2(dz, ref)
    print(f"flow-jvp-edges gn-chained {name}: max|dy| / max|y| = {float(dy.abs().max() / y.detach().abs().max()):.3e} "
          f"conv_tangent against float64: {e:.3e} (bound {FE.TOL_CONV:.1e}) y: {rel_l2(y, y64):.3e} dy: {rel_l2(dy, dy64):.3e}")
    assert bool(torch.isfinite(dz).all())
    assert e <= FE.TOL_CONV, e


# ------------------------------------------------------------------------------------------------ attention JVP
def _attn_run(dev, c, t):
    from lidarcrafter_amd._lib import lib

    ops, bufs = {}, {}
    for n in ("q", "k", "v", "dq", "dk", "dv"):
        ops[n], bufs[n] = FE.place(t[n][None], "contig", dev)
    o, o_ok = _out(FE.BH * c.dv * c.Lq, dev)
    do, do_ok = _out(FE.BH * c.dv * c.Lq, dev)
    lse, lse_ok = _out(FE.BH * c.Lq, dev)
    rc = lib().lc_attention_jvp_fwd(*(ops[n].data_ptr() for n in ("q", "k", "v", "dq", "dk", "dv")), o.data_ptr(), lse.data_ptr(),
                                    do.data_ptr(), FE.BH, c.Lq, c.Lk, c.dqk, c.dv, float(t["scale"]), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    intact = o_ok() and do_ok() and lse_ok() and all(bool(torch.isnan(FE.outside(bufs[n], ops[n])).all()) and
                                                     torch.equal(ops[n].cpu()[0], t[n]) for n in ops)
    return o.clone().reshape(FE.BH, c.dv, c.Lq), do.clone().reshape(FE.BH, c.dv, c.Lq), lse.clone().reshape(FE.BH, c.Lq), intact


@pytest.mark.parametrize("c", FE.ATTN_CASES, ids=ids)
def test_attention_jvp_row(dev, c):
    r = FE.attn_ref(c)
    rc, route = FE.attn_route(c)
    assert rc == 0
    o, do, lse, intact = _attn_run(dev, c, r.t)
    e_o, e_do = FE.attn_elem_err(o, r.r["o"], r.r["S_o"]), FE.attn_elem_err(do, r.r["do"], r.r["S_do"])
    e_lse = float(((lse.double().cpu() - r.r["lse"]).abs() / r.r["lse"].abs().clamp_min(1.0)).max())
    line = (f"flow-jvp-edges attn {c.name} route={route} o={e_o:.3e} (ref32 {r.e32_o:.3e}, bound {r.bound_o:.3e}) "
            f"do={e_do:.3e} (ref32 {r.e32_do:.3e}, bound {r.bound_do:.3e}) lse={e_lse:.3e} (ref32 {r.e32_lse:.3e}, bound {FE.LSE_TOL:.1e})")
    hot = None
    if FE.attn_win(c) is not None:
        w = FE.attn_win(c)
        hot = (FE.attn_elem_err(o, r.t["v"].double()[:, :, w, None].expand_as(r.r["o"]), r.r["S_o"]),
               FE.attn_elem_err(do, r.t["dv"].double()[:, :, w, None].expand_as(r.r["do"]), r.r["S_do"]))
        line += f" one-hot: o - v[{w}] = {hot[0]:.3e} do - dv[{w}] = {hot[1]:.3e}"
    print(line)
    assert intact, "a word outside an output was written, or an operand or its surroundings changed"
    assert all(bool(torch.isfinite(a).all()) for a in (o, do, lse)), "not finite (or not written: the outputs start as NaN)"
    assert e_o <= r.bound_o, (e_o, r.bound_o)
    assert e_do <= r.bound_do, (e_do, r.bound_do)
    assert e_lse <= FE.LSE_TOL, e_lse
    if hot is not None:
        assert hot[0] <= r.bound_o and hot[1] <= r.bound_do, hot
    o2, do2, lse2, _ = _attn_run(dev, c, r.t)
    assert torch.equal(o2, o) and torch.equal(do2, do) and torch.equal(lse2, lse), "a second call gives other bits"


def _by_position(got, ref32, ref64):
    """(whole rel-L2, worst rel-L2 by position of the last axis, its bound factor max(1, r_ref) from the float32 oracle):
    the by-query / by-key condition tests/test_attention_matrix.py holds the backward to, at TOL_ATTN_BWD."""
    g, r = got.detach().cpu().double(), ref64
    whole = float((g - r).norm() / r.norm())
    pos = lambda a: ((a - r).flatten(0, 1).norm(dim=0) / r.flatten(0, 1).norm(dim=0).clamp_min(1e-300))
    whole32 = float((ref32.double() - r).norm() / r.norm())
    r_ref = float(pos(ref32.double()).max()) / whole32 if whole32 > 0 else 1.0
    return whole, float(pos(g).max()), max(1.0, r_ref)


@pytest.mark.parametrize("c", FE.ATTN_BWD_CASES, ids=ids)
def test_attention_jvp_backward_row(dev, c):
    """FlashAttentionJvp's backward runs lc_attention_bwd* on the o and lse the JVP kernel saved: dq by query, dk and dv by
    key against float64 autograd under test_attention_matrix.py's tolerance for that backward."""
    from lidarcrafter_amd import autograd as AG

    t = FE.attn_operands(c)
    go, o64, *g64 = FE.attn_bwd_ref(c, torch.float64)
    _, o32, *g32 = FE.attn_bwd_ref(c, torch.float32)
    q, k, v = (t[n][None].to(dev).requires_grad_() for n in ("q", "k", "v"))
    z = lambda a: torch.zeros_like(a)
    o, _ = AG.FlashAttentionJvp.apply(q, k, v, z(q), z(k), z(v), t["scale"])
    o.backward(go[None].float().to(dev))
    torch.cuda.synchronize()
    figs = []
    for n, a, r32, r64 in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), g32, g64):
        assert a is not None and bool(torch.isfinite(a).all()), n
        if float(r64.norm()) == 0.0:
            # one key: p = 1, dq = dk = 0 in exact arithmetic; what is left is the rounding of go . v - go . o times k (or q)
            other = t["k"] if n == "dq" else t["q"]
            size = t["scale"] * float(go.norm()) * float(t["v"].double().norm()) * float(other.double().norm())
            figs.append((n, float(a.double().norm()) / size, 0.0, FE.TOL_ATTN_BWD, "|got| / (scale |go| |v| |k or q|), reference 0"))
        else:
            whole, worst, fac = _by_position(a[0], r32, r64)
            figs.append((n, whole, worst, FE.TOL_ATTN_BWD * fac, "whole, worst position"))
    print(f"flow-jvp-edges attn-bwd {c.name} ({AG.TRAIN_ATTN_BWD_PRECISION}) o={rel_l2(o[0], o64):.3e} " +
          " ".join(f"{n}={w:.3e}/{p:.3e} (tol {FE.TOL_ATTN_BWD:.1e}, by position {b:.2e}; {what})" for n, w, p, b, what in figs))
    for n, whole, worst, bound, _ in figs:
        assert whole <= FE.TOL_ATTN_BWD, (n, whole)
        assert worst <= bound, (n, worst, bound)
