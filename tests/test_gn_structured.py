"""GroupNorm from the producers' statistics entries on channel-structured activations (tests/_gn_structured.py has the
data and the bound; tests/test_gn_structured_host.py checks both on the CPU).  `pytest -m gpu`.

Recipe of every case: produce `y` through the producer with entries on, read it back, evaluate GroupNorm on the STORED
tensor in float64 and float32 on the CPU (the producer's own arithmetic drops out), run the consumer on `y` (entries) and
on `y.clone()` (statistics pass: the control, held to the same bound).

Conditions (per sample and group):
  1. rel-L2 against float64 <= max(tol, 4 x the largest per-group error of the float32 oracle on the same tensor);
     tol = 2e-6, 1e-4 in the common-level case.  The fused-input convolution mixes the groups: whole tensor there, against
     the float64 chain, floor 3e-6 (test_conv_fused_groupnorm's tolerance against the oracle).
  2. rows (lc_groupnorm_coeffs_os from the entries, groupnorm_coeffs from the statistics pass): |mean error| <=
     2^-23 max|group values|, rstd relative error within the bound of 1.
  3. an exactly constant group: everything finite, abs error <= S.constant_bound.
  4. the entry route gives the same bits twice.
Every case prints its figures (`GNS|route|data|consumer|R|entries|control|float32 oracle|bound`).

Measured on the MI355X (the table in DESIGN.md, "Error profiles"): every route at or below the float32 oracle's own error
(worst ratio 0.95 against the limit of 4), entries and control alike.  With the library of the commit before these tests 43
of the 234 cases fail: pair and quad entries shared their octet's pivot (per-group error up to 0.40 at R = 3070), and every
producer but the non-pipelined 1x1 kernel truncated its pivot to an integer (10 ... 33 x the oracle at step 2^-8)."""
import ctypes

import pytest
import torch

from lidarcrafter_amd.testing import rel_l2, seeded_randn
from tests import _gn_structured as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def decode(sa):
    """SplitAct -> fp64 [B, C, H, W] of (hi + lo) / x_scale (test_presplit.decode)."""
    B, C, H, W = sa.shape
    n = B * 2 * (C // 8) * H * W
    u = sa.buf[:n].view(B, 2, C // 8, H, W, 8).double()
    return ((u[:, 0] + u[:, 1]).permute(0, 1, 4, 2, 3).reshape(B, C, H, W) / sa.packed.x_scale).cpu()


def produce(K, dev, route, case):
    """The producer launch of `route` on the operands of `case` -> y (carrying the entries)."""
    B, Ci, Co, H, W = case["shape"]
    x = case["x"].to(dev)
    if route.entry == "resample2x":
        return K.resample2x(x, up=False)
    w, b = case["w"].to(dev), case["b"].to(dev)
    emit = True if route.unit == 8 else route.unit
    if route.entry == "conv2d_ring":
        return K.conv2d_ring(x, K.PackedConv(), w, b, tile_cfg=route.cfg, emit_stats=emit)
    pk = K.PackedConv("structured." + route.name)
    if route.entry == "_conv2d_ring_presplit":
        if route.name.startswith("splitk"):
            assert K.splitk_factor(B, Ci, Co, H, W) >= 2, "shape chosen to take the split-K route"
        # (the apply + split pass takes ragged planes; its normalised output is the conv's unit-variance input)
        sa = K.groupnorm(x, 8 if Ci % 64 == 0 else 2, S.EPS, split_for=pk)
        assert isinstance(sa, K.SplitAct)
        return K.conv2d_ring(sa, pk, w, b, tile_cfg=route.cfg, emit_stats=emit)
    if route.entry == "conv_down2":
        return K.conv_down2(x, pk, w, b, emit_stats=emit)
    assert route.entry == "conv_up2"
    return K.conv_up2(K.split_act(x, pk), pk, K.up9_weight(w), b, emit_stats=True)


def rows_from_entries(K, y, G):
    """(mean, rstd) [B, G] from the rows lc_groupnorm_coeffs_os derives from the entries `y` carries."""
    from lidarcrafter_amd._lib import OctStats

    B, C = y.shape[:2]
    hs = K._find_stats(y, G)
    cpad = (C + 15) // 16 * 16
    coef = torch.empty((B, cpad, 4), device=y.device, dtype=torch.float32)
    keep = [OctStats(h.buf.data_ptr(), h.channels, h.slots, h.unit) for h in hs]
    K.check(K.lib().lc_groupnorm_coeffs_os(ctypes.byref(keep[0]), ctypes.byref(keep[1]) if len(keep) > 1 else None, None,
                                           None, None, None, 0, coef.data_ptr(), B, C, cpad, G, float(S.EPS), K._stream()),
            "lc_groupnorm_coeffs_os")
    c = coef.cpu().double()[:, :C:C // G]
    return c[..., 0], c[..., 1]


def rows_from_pass(K, y, G):
    c = K.groupnorm_coeffs(y, G, S.EPS).cpu().double()[:, :y.shape[1]:y.shape[1] // G]
    return c[..., 0], c[..., 1]


def check_route(K, dev, route, data, y, const, fails, tag=""):
    """All consumers on `y` (entries) and `y.clone()` (statistics pass) under the conditions of the module docstring."""
    B, C, H, W = y.shape
    G, cpg = route.G, C // route.G
    name = f"{route.name}{tag}"
    hs = K._find_stats(y, G)
    assert hs is not None, "the producer left no entries a GroupNorm of this group count can fold"
    assert all(h.unit == route.unit for h in hs), [h.unit for h in hs]
    yc = y.clone()
    assert K._find_stats(yc, G) is None
    silu = data != "constant"
    tol = S.TOL_COMMON if data == "common" else S.TOL_ENTRY
    p = S.gn_params(B, C)
    pd = {k: v.to(dev) for k, v in p.items()}
    R = float(S.measure_R(y, G).max())
    bound, e32, ref64 = S.bound_for(y, G, p, silu, tol, const)
    worst32 = float(e32.max())
    keep = torch.ones(G, dtype=torch.bool)
    if const is not None:
        keep[const] = False

    def cond1(consumer, got_e, got_c):
        ee, ec = S.group_err(got_e, ref64, G)[:, keep], S.group_err(got_c, ref64, G)[:, keep]
        print(f"GNS|{name}|{data}|{consumer}|{R:.0f}|{float(ee.max()):.3e}|{float(ec.max()):.3e}|{worst32:.3e}|{bound:.3e}")
        for kind, t, e in (("entries", got_e, ee), ("statistics pass", got_c, ec)):
            if not bool(torch.isfinite(t).all()):
                fails.append(f"{name} {data} {consumer} {kind}: not finite")
            elif not float(e.max()) <= bound:
                b_, g_ = divmod(int(e.argmax()), e.shape[1])
                fails.append(f"{name} {data} {consumer} {kind}: group error {float(e.max()):.3e} > {bound:.3e} "
                             f"(sample {b_}, kept group {g_}; float32 oracle {worst32:.3e}, R {R:.0f})")
        if const is not None:                      # condition 3, channel by channel of the constant group
            for kind, t in (("entries", got_e), ("statistics pass", got_c)):
                t = t.detach().cpu().double()
                for b_ in range(B):
                    for c in range(const * cpg, (const + 1) * cpg):
                        level = float(y[b_, c, 0, 0])
                        lim = S.constant_bound(level, p["ga"], p["be"], p["ss"], c, b_, C)
                        err = float((t[b_, c] - S.constant_closed_form(p["be"], p["ss"], c, b_, C, silu)).abs().max())
                        if not err <= lim:
                            fails.append(f"{name} {consumer} {kind}: constant group, sample {b_} channel {c}: abs error "
                                         f"{err:.3e} > {lim:.3e}")

    ga, be, sc, sh = pd["ga"], pd["be"], pd["ss"][:, :C], pd["ss"][:, C:]
    # ---- apply (lc_groupnorm_apply_os against the statistics pass + apply)
    a1 = K.groupnorm(y, G, S.EPS, ga, be, sc, sh, act_silu=silu)
    a2 = K.groupnorm(yc, G, S.EPS, ga, be, sc, sh, act_silu=silu)
    cond1("apply", a1, a2)
    if not torch.equal(a1, K.groupnorm(y, G, S.EPS, ga, be, sc, sh, act_silu=silu)):        # condition 4
        fails.append(f"{name} {data} apply: the entry route is not deterministic")
    # ---- apply + split (lc_groupnorm_apply_os_split: whole octets, 2 or 4 per group), decoded from the fp16 planes
    if K.can_presplit(C, G) and K._find_stats(y, G, octet_groups=True) is not None:
        pk1, pk2 = K.PackedConv("structured.split"), K.PackedConv("structured.split.control")
        s1 = K.groupnorm(y, G, S.EPS, ga, be, sc, sh, act_silu=silu, split_for=pk1)
        s2 = K.groupnorm(yc, G, S.EPS, ga, be, sc, sh, act_silu=silu, split_for=pk2)
        assert isinstance(s1, K.SplitAct) and isinstance(s2, K.SplitAct)
        cond1("split", decode(s1), decode(s2))
        wc = (seeded_randn(64, C, 3, 3, seed=7400) / (C * 9) ** 0.5).to(dev)
        z1, z2 = K.conv2d_ring(s1, pk1, wc, None), K.conv2d_ring(s2, pk2, wc, None)   # ... and through the consuming conv
        if not rel_l2(z1, z2) <= max(tol, S.MARGIN * worst32):
            fails.append(f"{name} {data} split -> conv: {rel_l2(z1, z2):.3e} between the two routes")
    # ---- rows (condition 2)
    mean64, var64, rstd64 = S.group_stats64(y, G)
    amax = S.group_view(y, G).abs().amax(-1)
    for kind, (mu, rs) in (("entries", rows_from_entries(K, y, G)), ("statistics pass", rows_from_pass(K, yc, G))):
        em = ((mu - mean64).abs() / amax.clamp_min(1e-30))[:, keep]
        er = ((rs - rstd64).abs() / rstd64)[:, keep]
        print(f"GNS|{name}|{data}|rows {kind}|{R:.0f}|mean {float(em.max()) / S.F32_ULP:.2f} ulp|rstd {float(er.max()):.3e}|"
              f"{worst32:.3e}|{bound:.3e}")
        if not float(em.max()) <= S.F32_ULP:
            fails.append(f"{name} {data} rows, {kind}: mean off by {float(em.max()) / S.F32_ULP:.2f} x 2^-23 max|group|")
        if not float(er.max()) <= bound:
            fails.append(f"{name} {data} rows, {kind}: rstd relative error {float(er.max()):.3e} > {bound:.3e}")
        if not (bool(torch.isfinite(mu).all()) and bool(torch.isfinite(rs).all())):
            fails.append(f"{name} {data} rows, {kind}: not finite")
    # ---- groupnorm_stats -> convolution with fused rows (whole tensor: the convolution mixes the groups)
    from oracle import denoiser as D

    wc = seeded_randn(64, C, 3, 3, seed=7401) / (C * 9) ** 0.5
    st = K.groupnorm_stats(y, G, S.EPS, ga, be, sc, sh)
    assert st._struct.partials is None and st._struct.os0, "groupnorm_stats did not take the entries"
    stc = K.groupnorm_stats(yc, G, S.EPS, ga, be, sc, sh)
    assert stc._struct.partials is not None
    c1 = K.conv2d_ring(y, K.PackedConv(), wc.to(dev), None, gn_coeffs=st, gn_silu=silu)
    c2 = K.conv2d_ring(yc, K.PackedConv(), wc.to(dev), None, gn_coeffs=stc, gn_silu=silu)
    r64 = D.conv_ring(ref64, wc.double())
    r32 = D.conv_ring(S.gn_eval(y, G, p, silu, torch.float32), wc)
    cb = max(3e-6, S.MARGIN * rel_l2(r32, r64))
    e1, e2 = rel_l2(c1, r64), rel_l2(c2, r64)
    print(f"GNS|{name}|{data}|fused conv|{R:.0f}|{e1:.3e}|{e2:.3e}|{rel_l2(r32, r64):.3e}|{cb:.3e}")
    for kind, e in (("entries", e1), ("statistics pass", e2)):
        if not e <= cb:
            fails.append(f"{name} {data} fused conv, {kind}: {e:.3e} > {cb:.3e}")
    if not torch.equal(c1, K.conv2d_ring(y, K.PackedConv(), wc.to(dev), None, gn_coeffs=st, gn_silu=silu)):
        fails.append(f"{name} {data} fused conv: the entry route is not deterministic")
    return R


@pytest.mark.parametrize("data", S.DATA_NAMES)
@pytest.mark.parametrize("route", S.ROUTES, ids=repr)
def test_groupnorm_from_entries_on_structured_activations(dev, route, data, monkeypatch):
    from lidarcrafter_amd import ops as K

    monkeypatch.setattr(K, "FOLD_UP_MIN_CI", 32)
    case = S.make_case(route, data)
    y = produce(K, dev, route, case)
    assert tuple(y.shape) == route.out_shape(case["shape"])
    assert not K.range_poll(dev)
    h = y._lc_gnstats[(0, y.shape[1])]
    y_again = produce(K, dev, route, case)                                  # condition 4: the producer's entries
    assert torch.equal(y, y_again) and torch.equal(h.buf, y_again._lc_gnstats[(0, y.shape[1])].buf), \
        "the producer's output or its entries are not deterministic"
    assert bool(torch.isfinite(h.buf).all())
    fails = []
    R = check_route(K, dev, route, data, y, case["const"], fails)
    if route.sub_octet and data == "step8-a4":
        assert R >= S.R_MIN, f"R = {R:.1f}: the case does not reach the regime it is meant to test"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("data", S.DATA_NAMES)
def test_groupnorm_from_entries_of_two_concatenated_producers(dev, data):
    """Two producers with different tile shapes (different slot counts) write the halves of a concat buffer with pair
    entries; GroupNorm32 over the 128 channels (4 per group) folds both segments."""
    from lidarcrafter_amd import ops as K

    route = S.Route("concat-pair", "conv2d_ring", 2, (2, 32, 128, 8, 128), 32, sub_octet=True)
    B, Ci, C, H, W = route.shape
    w, b, const = S.conv_params(C, Ci, 3, route.G, data, seed=11)
    x = seeded_randn(B, Ci, H, W, seed=7311).to(dev)
    cat = torch.empty(B, C, H, W, device=dev)
    h = C // 2
    K.conv2d_ring(x, K.PackedConv(), w[:h].contiguous().to(dev), b[:h].contiguous().to(dev), out=cat[:, :h], tile_cfg=23,
                  emit_stats=2)
    K.conv2d_ring(x, K.PackedConv(), w[h:].contiguous().to(dev), b[h:].contiguous().to(dev), out=cat[:, h:], tile_cfg=13,
                  emit_stats=2)
    hs = K._find_stats(cat, route.G)
    assert hs is not None and len(hs) == 2 and hs[0].slots != hs[1].slots
    fails = []
    R = check_route(K, dev, route, data, cat, const, fails)
    if data == "step8-a4":
        assert R >= S.R_MIN, R
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("data", S.DATA_NAMES)
@pytest.mark.parametrize("route_name", ["def3x3-pair-c23", "ps-quad-c13", "def3x3-oct-c13", "def3x3-pair-c192"])
def test_training_forward_records_on_structured_activations(dev, route_name, data):
    """The training forward (lc_groupnorm_stats + lc_groupnorm_apply_train) leaves (mean, rstd) per group for its backward:
    conditions 1 - 3 on its output and on those records, on the structured tensor of the route's shape (the CPU evaluation of
    the producer: this forward reads no entries, only the tensor)."""
    from lidarcrafter_amd import autograd as AG

    route = S.ROUTE_BY_NAME[route_name]
    case = S.make_case(route, data)
    y = S.cpu_produce(route, case, torch.float64).float()
    B, C = y.shape[:2]
    G, cpg, const = route.G, C // route.G, case["const"]
    silu = data != "constant"
    p = S.gn_params(B, C)
    bound, e32, ref64 = S.bound_for(y, G, p, silu, S.TOL_COMMON if data == "common" else S.TOL_ENTRY, const)
    x = y.to(dev).requires_grad_()
    ss = p["ss"].to(dev)
    out = AG.GroupNormAct.apply(x, p["ga"].to(dev), p["be"].to(dev), ss[:, :C], ss[:, C:], G, S.EPS, silu)
    mr = out.grad_fn.saved_tensors[1].detach().cpu().double()
    assert tuple(mr.shape) == (B, G, 2) and bool(torch.isfinite(mr).all()) and bool(torch.isfinite(out).all())
    keep = torch.ones(G, dtype=torch.bool)
    if const is not None:
        keep[const] = False
    mean64, _, rstd64 = S.group_stats64(y, G)
    amax = S.group_view(y, G).abs().amax(-1)
    em = ((mr[..., 0] - mean64).abs() / amax.clamp_min(1e-30))[:, keep]
    er = ((mr[..., 1] - rstd64).abs() / rstd64)[:, keep]
    eo = S.group_err(out.detach(), ref64, G)[:, keep]
    print(f"GNS|train-{route_name}|{data}|records|{float(S.measure_R(y, G).max()):.0f}|mean {float(em.max()) / S.F32_ULP:.2f} ulp|"
          f"rstd {float(er.max()):.3e}|out {float(eo.max()):.3e}|{float(e32.max()):.3e}|{bound:.3e}")
    assert float(em.max()) <= S.F32_ULP, float(em.max()) / S.F32_ULP
    assert float(er.max()) <= bound, (float(er.max()), bound)
    assert float(eo.max()) <= bound, (float(eo.max()), bound)
    if const is not None:
        o = out.detach().cpu().double()
        for b_ in range(B):
            for c in range(const * cpg, (const + 1) * cpg):
                lim = S.constant_bound(float(y[b_, c, 0, 0]), p["ga"], p["be"], p["ss"], c, b_, C)
                err = float((o[b_, c] - S.constant_closed_form(p["be"], p["ss"], c, b_, C, silu)).abs().max())
                assert err <= lim, (b_, c, err, lim)
