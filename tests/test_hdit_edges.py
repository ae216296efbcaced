"""The HDiT kernels at their block edges, wraps and clamps against float64.  `pytest -m gpu`.

csrc/hdit.hip and csrc/hdit_bwd.hip through the C ABI, row by row of the tables in tests/_hdit_edges.py;
tests/test_hdit_edges_host.py proves on the CPU that the tables reach every edge, that the oracles are right, that the
bounds are reachable and that each subtly wrong oracle is 16 bounds away.  Every operand is a view into a NaN-filled buffer
in the row's layout, every output a view between NaN guard words, the scratch is NaN before every call, and every figure is
printed before it is asserted (profiles/hdit_edges.txt).  Every call is made twice (the same bits) and once more through
the ops wrapper on contiguous copies (the same bits again)."""
import ctypes

import pytest
import torch

from tests import _hdit_edges as E

pytestmark = pytest.mark.gpu
NAN = float("nan")
ids = lambda c: c.name
MODE = {"plain": 0, "mod": 1, "gain": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                    # a GPU fault: nothing more is launched in this session
        pytest.exit(f"the GPU reported an error, the run ends here: {e}", returncode=3)


def _lib():
    from lidarcrafter_amd._lib import lib

    return lib()


def _nan3(B, C, L):
    return torch.full((B, C, L), NAN)


def _untouched(*pairs):
    """Every (buffer, view): all that the view does not cover is still NaN."""
    return all(bool(torch.isnan(E.outside(buf, view)).all()) for buf, view in pairs)


def _guards(buf, n):
    return bool(torch.isnan(buf[:E.GUARD]).all() and torch.isnan(buf[E.GUARD + n:]).all())


def _fmt(tag, name, figs, e32, bnd):
    return f"hdit-edges {tag} {name}: " + " ".join(f"{k}={figs[k]:.3e} (ref32 {e32[k]:.3e}, bound {bnd[k]:.3e})" for k in figs)


def _assert_figs(figs, bnd):
    for k, v in figs.items():
        assert v <= bnd[k], (k, v, bnd[k])


def _same(a, b, what):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), f"{what}: other bits in {k}"


# ------------------------------------------------------------------------------------------------ RMSNorm
def _rms_run(dev, c, r, want_param=True):
    h = _lib()
    grid = c.form == "grid"
    x, xbuf = E.place3(r.x, c.xl, dev)
    dy, dybuf = E.place_pitch(r.dy, 3, dev) if grid else E.place3(r.dy, "contig", dev)
    y, ybuf = E.place3(_nan3(c.B, c.C, c.L), c.xl, dev)
    dx, dxbuf = E.place_pitch(_nan3(c.B, c.C, c.L), 5, dev) if grid else E.place3(_nan3(c.B, c.C, c.L), "slice_lo", dev)
    for v in (x, dy, y, dx):
        assert v.shape == (c.B, c.C, c.L) and v.stride(2) == 1 and (grid or v.stride(1) == 1)
    f, f_bs = None, 0
    if c.mode == "mod":
        wide = torch.full((c.B, 2 * c.C), NAN, device=dev)
        wide[:, c.C:] = r.f.to(dev)
        f, f_bs = wide[:, c.C:], 2 * c.C
    elif c.mode == "gain":
        f = r.f.to(dev).contiguous()
    fp = None if f is None else f.data_ptr()
    st = _stream()
    rc = h.lc_hdit_rmsnorm_fwd(x.data_ptr(), x.stride(0), x.stride(1), fp, f_bs, MODE[c.mode], y.data_ptr(), y.stride(0), y.stride(1),
                               c.B, c.C, c.L, E.EPS, st)
    _sync()
    assert rc == 0, rc
    param = want_param and c.mode != "plain"
    n_df = (c.B * c.C if c.mode == "mod" else c.C) if param else 1
    df, dfbuf = E.guarded(n_df, dev, NAN)
    rs = torch.full((c.B * c.L,), NAN, device=dev)
    rc = h.lc_hdit_rmsnorm_bwd(x.data_ptr(), x.stride(0), x.stride(1), fp, f_bs, MODE[c.mode], dy.data_ptr(), dy.stride(0), dy.stride(1),
                               dx.data_ptr(), dx.stride(0), dx.stride(1), rs.data_ptr() if param else None,
                               df.data_ptr() if param else None, c.C, c.B, c.C, c.L, E.EPS, st)
    _sync()
    assert rc == 0, rc
    intact = _untouched((xbuf, x), (dybuf, dy), (ybuf, y), (dxbuf, dx)) and _guards(dfbuf, n_df)
    if not param:
        intact = intact and bool(torch.isnan(df).all()) and bool(torch.isnan(rs).all())
    out = dict(y=y.clone().cpu(), dx=dx.clone().cpu(), intact=intact)
    if param:
        out.update(df=df.clone().cpu(), rs=rs.cpu())
    return out


@pytest.mark.parametrize("c", E.RMS, ids=ids)
def test_rmsnorm_row(dev, c):
    from lidarcrafter_amd import ops as K

    r = E.rms_ref(c)
    o = _rms_run(dev, c, r)
    figs = dict(y=E.token_err(o["y"], r.y), dx=E.token_err(o["dx"], r.dx))
    if r.df is not None:
        figs["df"] = E.elem_err(o["df"], r.df, r.S_df)
    print(_fmt("rmsnorm", c.name, figs, r.e32, r.bound))
    assert o["intact"], "a word outside an output was written, or an input changed"
    assert all(bool(torch.isfinite(o[k]).all()) for k in figs), "not finite (or not written: the outputs start as NaN)"
    _assert_figs(figs, r.bound)
    if c.zero_token:
        assert float(o["y"][c.B - 1, :, c.L - 1].abs().max()) == 0.0
    if "rs" in o:
        assert bool(torch.isfinite(o["rs"]).all()), "the r scratch has an unwritten token"
    _same(o, _rms_run(dev, c, r), "a second call")
    bare = _rms_run(dev, c, r, want_param=False)                      # df = rs = NULL: the same dx, nothing else written
    assert bare["intact"] and torch.equal(bare["dx"], o["dx"]) and torch.equal(bare["y"], o["y"])
    # the ops wrappers on contiguous copies
    shape = (c.B, c.C, 1, c.L) if c.form == "grid" else (c.B, c.C)
    xs, dys = r.x.reshape(shape).to(dev), r.dy.reshape(shape).to(dev)
    kw = {}
    if c.mode == "mod":
        kw["mod"] = r.f.to(dev)
    elif c.mode == "gain":
        kw["gain"] = r.f.to(dev).contiguous()
    assert torch.equal(K.hdit_rmsnorm(xs, **kw).cpu().reshape(o["y"].shape), o["y"])
    dxw, dfw = K.hdit_rmsnorm_bwd(xs, dys, **kw)
    assert torch.equal(dxw.cpu().reshape(o["dx"].shape), o["dx"])
    assert (dfw is None) == (r.df is None) and (dfw is None or torch.equal(dfw.cpu().reshape(-1), o["df"]))


# ------------------------------------------------------------------------------------------------ GEGLU
def _geglu_run(dev, c, r):
    h = _lib()
    x, xbuf = E.place3(r.x, c.xl, dev)
    dy, dybuf = E.place3(r.dy, "bs1", dev)
    y, ybuf = E.place3(_nan3(c.B, c.mid, c.L), "slice_lo", dev)
    dx, dxbuf = E.place3(_nan3(c.B, 2 * c.mid, c.L), "slice_hi", dev)
    for v, ch in ((x, 2 * c.mid), (dy, c.mid), (y, c.mid), (dx, 2 * c.mid)):
        assert v.shape == (c.B, ch, c.L) and v.stride(2) == 1 and v.stride(1) == c.L and v.stride(0) >= ch * c.L
    st = _stream()
    rc = h.lc_hdit_geglu_fwd(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), c.B, c.mid, c.L, st)
    _sync()
    assert rc == 0, rc
    rc = h.lc_hdit_geglu_bwd(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), dx.data_ptr(), dx.stride(0), c.B, c.mid, c.L, st)
    _sync()
    assert rc == 0, rc
    return dict(y=y.clone().cpu(), dx=dx.clone().cpu(), intact=_untouched((xbuf, x), (dybuf, dy), (ybuf, y), (dxbuf, dx)))


@pytest.mark.parametrize("c", E.GEGLU, ids=ids)
def test_geglu_row(dev, c):
    from lidarcrafter_amd import ops as K

    r = E.geglu_ref(c)
    o = _geglu_run(dev, c, r)
    figs = dict(y=E.elem_err(o["y"], r.y, r.S_y), dx=E.elem_err(o["dx"], r.dx, r.S_dx))
    print(_fmt("geglu", c.name, figs, r.e32, r.bound))
    assert o["intact"], "a word outside an output was written, or an input changed"
    assert bool(torch.isfinite(o["y"]).all()) and bool(torch.isfinite(o["dx"]).all()), "NaN or inf (the planted gates reach +-10 and 40)"
    _assert_figs(figs, r.bound)
    _same(o, _geglu_run(dev, c, r), "a second call")
    shape = (lambda ch: (c.B, ch, 1, c.L)) if c.form == "grid" else (lambda ch: (c.B, ch))
    xs, dys = r.x.reshape(shape(2 * c.mid)).to(dev), r.dy.reshape(shape(c.mid)).to(dev)
    assert torch.equal(K.hdit_geglu(xs).cpu().reshape(o["y"].shape), o["y"])
    assert torch.equal(K.hdit_geglu_bwd(xs, dys).cpu().reshape(o["dx"].shape), o["dx"])


# ------------------------------------------------------------------------------------------------ q / k preparation
def _qk_buffers(dev, c, t):
    """-> (q view, k view, [(flat buffer, its untouched copy, mask of what q / k cover)])."""
    C, L, B = E.QK_HEADS * c.d, c.L, E.QK_B
    if c.separate:
        q, qbuf = E.place_pitch(t["q"], 3, dev)
        k, kbuf = E.place_pitch(t["k"], 5, dev)
        bufs = [(qbuf, q), (kbuf, k)]
    else:
        ch = 3 * C + E.QK_PAD
        flat = torch.full((2 * E.GUARD + B * ch * L,), NAN, device=dev)
        whole = flat[E.GUARD:E.GUARD + B * ch * L].view(B, ch, L)
        q, k, v = whole[:, :C], whole[:, C + E.QK_PAD:2 * C + E.QK_PAD], whole[:, 2 * C + E.QK_PAD:]
        q.copy_(t["q"]), k.copy_(t["k"]), v.copy_(t["v"])
        bufs = [(flat, q), (flat, k)]
    checks = []
    for buf, view in bufs:
        mask = torch.ones(buf.numel(), dtype=torch.bool, device=dev)
        mask.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
        checks.append((buf, mask))
    if not c.separate:
        checks = [(flat, checks[0][1] & checks[1][1])]
    return q, k, [(buf, buf.clone(), mask) for buf, mask in checks]


def _bits_kept(checks):
    return all(torch.equal(buf.view(torch.int32)[mask], old.view(torch.int32)[mask]) for buf, old, mask in checks)


def _qk_run(dev, c, r, want_scale=True):
    h = _lib()
    t = r.t
    C, L, B, H = E.QK_HEADS * c.d, c.L, E.QK_B, E.QK_HEADS
    scale, cos_t, sin_t = (t[n].to(dev).contiguous() for n in ("scale", "cos_t", "sin_t"))
    st = _stream()
    q, k, checks = _qk_buffers(dev, c, t)
    for v in (q, k):
        assert v.shape == (B, C, L) and v.stride(2) == 1 and v.stride(1) >= L and v.stride(0) >= C * v.stride(1)
    rc = h.lc_hdit_qk_prep_fwd(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), scale.data_ptr(),
                               cos_t.data_ptr(), sin_t.data_ptr(), B, H, c.d, L, st)
    _sync()
    assert rc == 0, rc
    out = dict(q=q.clone().cpu(), k=k.clone().cpu(), intact=_bits_kept(checks))
    # the backward reads the raw slices
    q, k, checks = _qk_buffers(dev, c, t)
    gq, gqbuf = E.place_pitch(t["gq"], 3, dev)
    gk, gkbuf = E.place3(t["gk"], "slice_hi", dev)
    dq, dqbuf = E.place_pitch(_nan3(B, C, L), 5, dev)
    dk, dkbuf = E.place3(_nan3(B, C, L), "bs1", dev)
    part = torch.full((H * B * 2 * L,), NAN, device=dev, dtype=torch.float64)
    ds, dsbuf = E.guarded(H, dev, NAN)
    rc = h.lc_hdit_qk_prep_bwd(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1),
                               gq.data_ptr(), gq.stride(0), gq.stride(1), gk.data_ptr(), gk.stride(0), gk.stride(1),
                               dq.data_ptr(), dq.stride(0), dq.stride(1), dk.data_ptr(), dk.stride(0), dk.stride(1),
                               scale.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), part.data_ptr(),
                               ds.data_ptr() if want_scale else None, B, H, c.d, L, st)
    _sync()
    assert rc == 0, rc
    out["intact"] = out["intact"] and _bits_kept(checks) and torch.equal(q.cpu(), t["q"]) and torch.equal(k.cpu(), t["k"]) and \
        _untouched((gqbuf, gq), (gkbuf, gk), (dqbuf, dq), (dkbuf, dk)) and _guards(dsbuf, H) and \
        (want_scale or bool(torch.isnan(ds).all()))
    out.update(dq=dq.clone().cpu(), dk=dk.clone().cpu(), part_written=bool(torch.isfinite(part).all()))
    if want_scale:
        out["ds"] = ds.clone().cpu()
    return out


@pytest.mark.parametrize("c", E.QK, ids=ids)
def test_qk_prep_row(dev, c):
    from lidarcrafter_amd import ops as K

    r = E.qk_ref(c)
    o = _qk_run(dev, c, r)
    H = E.QK_HEADS
    figs = dict(q=E.token_err(o["q"], r.q, H), k=E.token_err(o["k"], r.k, H), dq=E.token_err(o["dq"], r.dq, H),
                dk=E.token_err(o["dk"], r.dk, H), ds=E.elem_err(o["ds"], r.ds, r.S_ds))
    print(_fmt("qk_prep", c.name, figs, r.e32, r.bound) + f" scales={c.scales}")
    assert o["intact"], "the v slice, a pad channel, a guard word or an input changed"
    assert all(bool(torch.isfinite(o[k]).all()) for k in figs) and o["part_written"]
    _assert_figs(figs, r.bound)
    for n, b, hd, tok, norm in E.qk_plants(c.L):
        if norm == 0:
            assert float(o[n][b, hd * c.d:(hd + 1) * c.d, tok].abs().max()) == 0.0, "the all-zero token is not exactly zero"
    assert bool((o["ds"][r.t["scale"] > E.LN100_F32] == 0).all())
    _same(o, _qk_run(dev, c, r), "a second call")
    bare = _qk_run(dev, c, r, want_scale=False)
    assert bare["intact"] and torch.equal(bare["dq"], o["dq"]) and torch.equal(bare["dk"], o["dk"])
    # the ops wrappers on contiguous copies
    t = {n: v.to(dev).contiguous() for n, v in r.t.items()}
    qc, kc = t["q"].clone(), t["k"].clone()
    K.hdit_qk_prep(qc, kc, H, t["scale"], t["cos_t"], t["sin_t"])
    assert torch.equal(qc.cpu(), o["q"]) and torch.equal(kc.cpu(), o["k"])
    dq, dk, ds = K.hdit_qk_prep_bwd(t["q"], t["k"], t["gq"], t["gk"], H, t["scale"], t["cos_t"], t["sin_t"])
    assert torch.equal(dq.cpu(), o["dq"]) and torch.equal(dk.cpu(), o["dk"]) and torch.equal(ds.cpu(), o["ds"])


# ------------------------------------------------------------------------------------------------ neighbourhood attention
def _cm(view, d):
    from lidarcrafter_amd._lib import CmOperand

    assert view.stride(2) == 1
    return CmOperand(view.data_ptr(), view.stride(0), d * view.stride(1), view.stride(1))


def _na_run(dev, c, r):
    h = _lib()
    t = r.t
    gh, gw, kh, kw = c.grid
    B, H, d = E.NA_B, E.NA_HEADS, c.d
    C, L = H * d, gh * gw
    ch = 3 * C + E.QK_PAD
    flat = torch.full((2 * E.GUARD + B * ch * L,), NAN, device=dev)
    whole = flat[E.GUARD:E.GUARD + B * ch * L].view(B, ch, L)
    q, k, v = whole[:, :C], whole[:, C + E.QK_PAD:2 * C + E.QK_PAD], whole[:, 2 * C + E.QK_PAD:]
    q.copy_(t["q"]), k.copy_(t["k"]), v.copy_(t["v"])
    before = flat.clone()
    do, dobuf = E.place_pitch(t["do"], 3, dev)
    st = _stream()
    ref = ctypes.byref
    res = {}
    for entry in ("fwd", "train"):
        if c.o_strided:
            o, obuf = E.place_pitch(_nan3(B, C, L), 3, dev)
        else:
            o, obuf = E.place3(_nan3(B, C, L), "contig", dev)
        assert o.shape == (B, C, L) and o.stride(2) == 1 and o.stride(1) >= L and o.stride(0) >= C * o.stride(1)
        lse, lsebuf = E.guarded(B * H * L, dev, NAN)
        ops3 = [_cm(x, d) for x in (q, k, v)]
        args = [ref(x) for x in ops3] + [o.data_ptr(), o.stride(0), d * o.stride(1), o.stride(1)]
        if entry == "fwd":
            rc = h.lc_hdit_na_fwd(*args, B, H, d, gh, gw, kh, kw, c.scale, st)
        else:
            rc = h.lc_hdit_na_train_fwd(*args, lse.data_ptr(), B, H, d, gh, gw, kh, kw, c.scale, st)
        _sync()
        assert rc == 0, rc
        ok = _untouched((obuf, o)) and _guards(lsebuf, B * H * L) and (entry == "train" or bool(torch.isnan(lse).all()))
        res[entry] = (o, lse, ok)
    o, lse, ok_t = res["train"]
    dsum = torch.full((B * H * L,), NAN, device=dev)
    grads = [E.guarded(B * C * L, dev, NAN) for _ in range(3)]
    ops5 = [_cm(x, d) for x in (q, k, v, o, do)]
    rc = h.lc_hdit_na_bwd(*(ref(x) for x in ops5), lse.data_ptr(), dsum.data_ptr(), *(g[0].data_ptr() for g in grads), B, H, d, gh, gw,
                          kh, kw, c.scale, st)
    _sync()
    assert rc == 0, rc
    intact = res["fwd"][2] and ok_t and torch.equal(flat.view(torch.int32), before.view(torch.int32)) and _untouched((dobuf, do)) and \
        all(_guards(g[1], B * C * L) for g in grads)
    out = dict(o_fwd=res["fwd"][0].clone().cpu(), o=o.clone().cpu(), lse=lse.clone().cpu().reshape(B * H, L), intact=intact,
               dsum_written=bool(torch.isfinite(dsum).all()))
    out.update({n: g[0].clone().cpu().reshape(B, C, L) for n, g in zip(("dq", "dk", "dv"), grads)})
    return out


@pytest.mark.parametrize("c", E.NA, ids=ids)
def test_neighbourhood_attention_row(dev, c):
    from lidarcrafter_amd import ops as K

    r = E.na_ref(c)
    o = _na_run(dev, c, r)
    figs = E.na_figures(o, r.ref)
    print(_fmt("na", c.name, figs, r.e32, r.bound))
    assert o["intact"], "a word outside an output was written, or an input changed"
    assert all(bool(torch.isfinite(o[k]).all()) for k in E.NA_OUT) and o["dsum_written"]
    assert torch.equal(o["o_fwd"], o["o"]), "hdit_na_train's o is not hdit_na's bit for bit"
    _assert_figs(figs, r.bound)
    if c.grid[2] * c.grid[3] == 1:
        assert torch.equal(o["o"], r.t["v"]), "a one-key window: o must be v bit for bit"
        assert torch.equal(o["dv"], r.t["do"]) and float(o["dq"].abs().max()) == 0.0 and float(o["dk"].abs().max()) == 0.0
    _same(o, _na_run(dev, c, r), "a second call")
    # the ops wrappers on contiguous copies
    gh, gw, kh, kw = c.grid
    t = {n: v.to(dev).contiguous() for n, v in r.t.items()}
    ow = K.hdit_na(t["q"], t["k"], t["v"], E.NA_HEADS, gh, gw, (kh, kw), scale=c.scale)
    ot, lse = K.hdit_na_train(t["q"], t["k"], t["v"], E.NA_HEADS, gh, gw, (kh, kw), scale=c.scale)
    assert torch.equal(ow.cpu(), o["o"]) and torch.equal(ot.cpu(), o["o"]) and torch.equal(lse.cpu(), o["lse"])
    grads = K.hdit_na_bwd(t["q"], t["k"], t["v"], ot, t["do"], lse, E.NA_HEADS, gh, gw, (kh, kw), scale=c.scale)
    for n, g in zip(("dq", "dk", "dv"), grads):
        assert torch.equal(g.cpu(), o[n]), n


# ------------------------------------------------------------------------------------------------ permutes
def _nan4(*shape):
    return torch.full(shape, NAN)


@pytest.mark.parametrize("c", E.PERMUTES, ids=ids)
def test_permute_row(dev, c):
    from lidarcrafter_amd import ops as K

    h = _lib()
    x = E.permute_operands(c)
    want = E.s2d_ref(x, c.P1, c.P2)
    st = _stream()
    for _ in range(2):
        xin, xbuf = E.place(x, c.il, dev)
        y, ybuf = E.place(_nan4(*want.shape), c.ol, dev)
        rc = h.lc_hdit_space_to_depth_fwd(xin.data_ptr(), xin.stride(0), y.data_ptr(), y.stride(0), c.B, c.C, c.H, c.W, c.P1, c.P2, st)
        _sync()
        assert rc == 0, rc
        s2d_ok = torch.equal(y.cpu(), want)
        zin, zbuf = E.place(want, c.il, dev)
        back, bbuf = E.place(_nan4(*x.shape), c.ol, dev)
        rc = h.lc_hdit_depth_to_space_fwd(zin.data_ptr(), zin.stride(0), back.data_ptr(), back.stride(0), None, 0, None, c.B, c.C,
                                          c.H // c.P1, c.W // c.P2, c.P1, c.P2, st)
        _sync()
        assert rc == 0, rc
        d2s_ok = torch.equal(back.cpu(), x)
        intact = _untouched((xbuf, xin), (ybuf, y), (zbuf, zin), (bbuf, back))
        print(f"hdit-edges permute {c.name}: n={c.C * c.H * c.W} space_to_depth equal: {s2d_ok} depth_to_space equal: {d2s_ok} "
              f"guards intact: {intact}")
        assert s2d_ok and d2s_ok and intact
    xd = x.to(dev)
    assert torch.equal(K.space_to_depth(xd, c.P1, c.P2).cpu(), want)
    assert torch.equal(K.depth_to_space(want.to(dev), c.P1, c.P2).cpu(), x)


# ------------------------------------------------------------------------------------------------ lerp
def _lerp_run(dev, c, r, want_alpha=True):
    h = _lib()
    t = r.t
    H, W = c.h * c.P1, c.w * c.P2
    ol = "contig" if c.sl == "contig" else "slice_hi"
    y, ybuf = E.place(t["y"], c.sl, dev)
    skip, sbuf = E.place(t["skip"], c.sl, dev)
    dout, gbuf = E.place(t["dout"], c.sl, dev)
    alpha = t["alpha"].to(dev)
    out, obuf = E.place(_nan4(c.B, c.C, H, W), ol, dev)
    dskip, dsbuf = E.place(_nan4(c.B, c.C, H, W), ol, dev)
    dy, dybuf = E.place(_nan4(*t["y"].shape), ol, dev)
    da, dabuf = E.guarded(c.C, dev, NAN)
    st = _stream()
    rc = h.lc_hdit_depth_to_space_fwd(y.data_ptr(), y.stride(0), out.data_ptr(), out.stride(0), skip.data_ptr(), skip.stride(0),
                                      alpha.data_ptr(), c.B, c.C, c.h, c.w, c.P1, c.P2, st)
    _sync()
    assert rc == 0, rc
    rc = h.lc_hdit_lerp_bwd(dout.data_ptr(), dout.stride(0), y.data_ptr(), y.stride(0), skip.data_ptr(), skip.stride(0), alpha.data_ptr(),
                            dskip.data_ptr(), dskip.stride(0), dy.data_ptr(), dy.stride(0), da.data_ptr() if want_alpha else None,
                            c.B, c.C, c.h, c.w, c.P1, c.P2, st)
    _sync()
    assert rc == 0, rc
    intact = _untouched((ybuf, y), (sbuf, skip), (gbuf, dout), (obuf, out), (dsbuf, dskip), (dybuf, dy)) and _guards(dabuf, c.C) and \
        (want_alpha or bool(torch.isnan(da).all()))
    res = dict(out=out.clone().cpu(), dskip=dskip.clone().cpu(), dy=dy.clone().cpu(), intact=intact)
    if want_alpha:
        res["dalpha"] = da.clone().cpu()
    return res


@pytest.mark.parametrize("c", E.LERP, ids=ids)
def test_lerp_row(dev, c):
    from lidarcrafter_amd import ops as K

    r = E.lerp_ref(c)
    o = _lerp_run(dev, c, r)
    figs = dict(out=E.elem_err(o["out"], r.out, r.S_out), **{n: E.elem_err(o[n], r.bwd[n], r.bwd["S_" + n]) for n in E.LERP_OUT})
    half = E.lerp_alpha(c) == 0.0
    differing = int((o["out"][:, half] != r.out32[:, half]).sum())
    print(_fmt("lerp", c.name, figs, r.e32, r.bound) + f" elements at weight 0.5 off the float32 restatement's bits: {differing} (bound 0)")
    assert o["intact"], "a word outside an output was written, or an input changed"
    assert all(bool(torch.isfinite(o[k]).all()) for k in figs)
    _assert_figs(figs, r.bound)
    # torch.lerp takes the high branch's formula from weight 0.5: the two differ by a rounding only, so by bits
    assert differing == 0
    _same(o, _lerp_run(dev, c, r), "a second call")
    bare = _lerp_run(dev, c, r, want_alpha=False)
    assert bare["intact"] and torch.equal(bare["dy"], o["dy"]) and torch.equal(bare["dskip"], o["dskip"])
    t = {n: v.to(dev) for n, v in r.t.items()}
    assert torch.equal(K.depth_to_space(t["y"], c.P1, c.P2, skip=t["skip"], alpha=t["alpha"]).cpu(), o["out"])
    dy, dskip, da = K.hdit_lerp_bwd(t["dout"], t["y"], t["skip"], t["alpha"], c.P1, c.P2)
    assert torch.equal(dy.cpu(), o["dy"]) and torch.equal(dskip.cpu(), o["dskip"]) and torch.equal(da.cpu(), o["dalpha"])


# ------------------------------------------------------------------------------------------------ tokenizer, Fourier
@pytest.mark.parametrize("c", E.TOKENIZE, ids=ids)
def test_tokenizer_row(dev, c):
    from lidarcrafter_amd import ops as K

    h = _lib()
    r = E.tokenize_ref(c)
    w, pe = r.t["w"].to(dev).contiguous(), r.t["pe"].to(dev).contiguous()
    got = []
    for _ in range(2):
        x, xbuf = E.place(r.t["x"], c.xl, dev)
        y, ybuf = E.place(_nan4(c.B, c.C, c.H, c.W // c.P), c.yl, dev)
        rc = h.lc_hdit_tokenize_fwd(x.data_ptr(), x.stride(0), w.data_ptr(), pe.data_ptr(), y.data_ptr(), y.stride(0), c.B, c.Cin, c.C,
                                    c.H, c.W, c.P, _stream())
        _sync()
        assert rc == 0, rc
        assert _untouched((xbuf, x), (ybuf, y)), "a word outside the output was written, or the input changed"
        got.append(y.clone().cpu())
    e = E.elem_err(got[0], r.y, r.S)
    print(f"hdit-edges tokenize {c.name}: y={e:.3e} (ref32 {r.e32:.3e}, bound {r.bound:.3e})")
    assert bool(torch.isfinite(got[0]).all())
    assert e <= r.bound, (e, r.bound)
    assert torch.equal(got[0], got[1]), "a second call gives other bits"
    assert torch.equal(K.hdit_tokenize(r.t["x"].to(dev), w, pe).cpu(), got[0])


@pytest.mark.parametrize("c", E.FOURIER, ids=ids)
def test_fourier_row(dev, c):
    from lidarcrafter_amd import ops as K

    h = _lib()
    r = E.fourier_ref(c)
    t, fr = r.t.to(dev), r.fr.to(dev)
    got = []
    for _ in range(2):
        y, ybuf = E.guarded(c.M * 2 * c.half, dev, NAN)
        rc = h.lc_hdit_fourier_fwd(t.data_ptr(), fr.data_ptr(), y.data_ptr(), c.M, c.half, _stream())
        _sync()
        assert rc == 0, rc
        assert _guards(ybuf, c.M * 2 * c.half)
        got.append(y.clone().cpu().reshape(c.M, 2 * c.half))
    e = E.elem_err(got[0], r.y, torch.ones_like(r.y))
    print(f"hdit-edges fourier {c.name}: y={e:.3e} (ref32 {r.e32:.3e}, bound {r.bound:.3e})")
    assert bool(torch.isfinite(got[0]).all())
    assert e <= r.bound, (e, r.bound)
    assert torch.equal(got[0], got[1]), "a second call gives other bits"
    assert torch.equal(K.hdit_fourier(t, fr).cpu(), got[0])
