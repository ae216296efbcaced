"""The case tables of tests/test_flow_jvp_edges.py, and the proof that they are complete (CPU only).

`lc_groupnorm_jvp_route`, `lc_qk_norm_cm_route` and `lc_attention_jvp_route` are the host functions the launchers and
kernels of csrc/flow_jvp.hip switch on (csrc/flow_jvp_route.h, csrc/gn_apply_route.h), so "which branch does this row
take" is asked of the library: every value of every field is hit, each cause of the scalar statistics branch occurs alone,
the closed-form float64 references agree with torch.func.jvp / autograd of the plain formulas, every designed defect moves
some element or token of every row it applies to by at least 16 bounds, and the float32 oracle stays under 8 floors on the
q / k and attention rows."""
import ctypes
import os
import re

import pytest
import torch

from tests import _flow_jvp_edges as FE
from tests.test_meanflow_training import _attn_ref, _gn_ref, _qk_ref

ids = lambda c: c.name
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_are_unique_and_every_row_names_its_edge():
    for table in (FE.QK_CASES, FE.GN_CASES, FE.ATTN_CASES, FE.ATTN_BWD_CASES):
        assert len({c.name for c in table}) == len(table)
        assert all(c.edge for c in table)


def test_the_apply_grid_rule_lives_in_one_header():
    src = {f: open(os.path.join(ROOT, "lidarcrafter_amd", "csrc", f)).read() for f in ("norm.hip", "flow_jvp.hip", "gn_apply_route.h")}
    assert "gnj_apply_grid" not in src["flow_jvp.hip"] and not re.search(r"\bgn_apply_grid\b", src["norm.hip"])
    for f in ("norm.hip", "flow_jvp.hip"):
        assert "lc_gn_apply_grid(" in src[f] and "HW * c * 2" not in src[f], f
    assert src["gn_apply_route.h"].count("inline void lc_gn_apply_grid") == 1


# ------------------------------------------------------------------------------------------------ routes
def test_every_qk_route_is_hit():
    dmax, blocks, trips, pad = set(), set(), set(), set()
    for c in FE.QK_CASES:
        rc, o = FE.qk_route(c)
        assert rc == 0, c.name
        from lidarcrafter_amd import _lib

        assert o[2] == _lib.lib().lc_qk_norm_cm_bwd_partials(c.B, c.heads, c.L) == o[1] * c.B * c.heads
        dmax.add(o[0]); blocks.add(o[1]); trips.add(o[3]); pad.add((o[0], o[0] - c.d > 0))
    assert dmax == {16, 32, 64} and blocks == {1, 2, 3} and trips == {1, 2}
    assert pad == {(m, p) for m in (16, 32, 64) for p in (False, True)}          # every DMAX exactly full and padded
    assert {c.d for c in FE.QK_CASES} >= {1, 5, 16, 17, 32, 33, 48, 64}
    assert {c.L for c in FE.QK_CASES} >= {1, 255, 256, 257, 513}
    assert {c.xl for c in FE.QK_CASES} >= {"contig", "qkv", "cs"}
    # the tiny tokens: every kind at a block's first and last token and at 255 / 256
    kinds = FE.qk_tiny_tokens(513)
    assert {0, 255, 256, 511, 512} <= set(kinds) and set(kinds.values()) == {0, 1, 2}
    for c in FE.QK_CASES:
        if c.tiny and c.L >= 257:
            got = {k for t, k in FE.qk_tiny_tokens(c.L).items()}
            assert got == {0, 1, 2}, c.name


def test_every_groupnorm_jvp_route_is_hit():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    seen = {k: set() for k in ("chunk", "chunks", "branch", "causes", "dvec", "slabs", "cpb", "last")}
    for c in FE.GN_CASES:
        rc, o = FE.gn_route(c)
        assert rc == 0, c.name
        n = (c.C // c.G) * c.H * c.W
        assert o[7] == h.lc_groupnorm_amax_partials(c.B, c.C, c.H, c.W, c.G, 0) == o[5] * (c.C // o[6]) * c.B, c.name
        assert h.lc_groupnorm_jvp_partials_elems(c.B, c.C, c.H, c.W, c.G) == 4 * c.B * c.G * o[1]
        assert h.lc_groupnorm_partials_elems(c.B, c.C, c.H, c.W, c.G) == 2 * c.B * c.G * o[1]       # the primal's chunks
        assert (o[1] - 1) * o[0] < n <= o[1] * o[0]
        seen["chunk"].add(o[0]); seen["chunks"].add(o[1]); seen["branch"].add(o[2]); seen["causes"].add(o[3])
        seen["dvec"].add((o[2], o[4])); seen["slabs"].add(o[5]); seen["cpb"].add(o[6])
        if o[1] > 1:
            seen["last"].add((o[0], n - (o[1] - 1) * o[0]))
    assert seen["chunk"] == {4096, 16384} and seen["chunks"] >= {1, 2, 3}
    assert seen["branch"] == {0, 1, 2}
    assert seen["slabs"] >= {1, 2, 3, 5} and seen["cpb"] == {1, 2, 4, 8}
    # a short last chunk: one element and one float4 after two whole chunks of 4096; a short one on the 16384 size
    assert {(4096, 1), (4096, 4)} <= seen["last"] and any(ce == 16384 and m < ce for ce, m in seen["last"])
    # the float4 loop with float4 / scalar / per-sample loads of dx
    assert {(1, 1), (1, 0), (1, 2)} <= seen["dvec"]
    # each cause ALONE, on the shape of the base row (which takes the float4 loop with float4 loads of dx)
    rows = {c.name: c for c in FE.GN_CASES}
    base = rows["base-vec"]
    assert FE.gn_route(base)[1][2:5] == [1, 0, 1]
    for name, cause, branch in (("x-off1", 2, 0), ("dx-off1", 4, 1), ("x-bs1", 2, 2), ("dx-bs1", 4, 1)):
        c = rows[name]
        assert c[2:7] == base[2:7] and FE.gn_route(c)[1][3] == cause and FE.gn_route(c)[1][2] == branch, name
    for name in ("x-slice-lo", "dx-slice-lo"):
        assert rows[name][2:7] == base[2:7] and FE.gn_route(rows[name])[1][2:5] == [1, 0, 1]
    # n % 4 alone: both operands contiguous and aligned
    c = rows["n-mod4-alone"]
    assert FE.gn_route(c)[1][2:4] == [0, 1] and c.xl == c.dxl == "contig"
    assert FE.gn_route(rows["n-mod4"])[1][2:4] == [0, 3]
    # x contiguous with dx slice_hi at H W % 4 != 0 and the reverse: n % 4 == 0, so the address alone decides
    a, b = rows["dx-slice-hi-odd"], rows["x-slice-hi-odd"]
    assert (a.H * a.W) % 4 and ((a.C // a.G) * a.H * a.W) % 4 == 0 and a[2:7] == b[2:7]
    assert FE.gn_route(a)[1][2] == 1 and FE.gn_route(a)[1][3] == 4 and FE.gn_route(a)[1][4] in (0, 2)
    assert FE.gn_route(b)[1][3] == 2 and FE.gn_route(b)[1][2] in (0, 2)
    assert {c.H * c.W for c in FE.GN_CASES} >= {4096, 4097} and any(c.C == c.G for c in FE.GN_CASES)
    combos = {(c.affine, c.ada, c.act) for c in FE.GN_CASES}
    assert combos >= {(False, True, True), (True, True, True), (True, False, False), (False, False, True), (True, True, False)}
    assert {(c.data, c.dxmode) for c in FE.GN_CASES if c.data} == {(d, m) for d in FE.GS.DATA_NAMES for m in ("rand", "prop")}
    assert max(c.B * c.C * c.H * c.W for c in FE.GN_CASES) * 4 <= 32 << 20            # the largest row: a few tens of MB


def test_every_attention_jvp_route_is_hit():
    seen = {k: set() for k in ("D", "last_rows", "tiles", "last", "qpad", "vpad", "qblocks")}
    for c in FE.ATTN_CASES + FE.ATTN_BWD_CASES:
        rc, o = FE.attn_route(c)
        assert rc == 0, c.name
        assert o[1] == {32: 64, 64: 32}[o[0]] and (o[2] - 1) * o[1] < c.Lq <= o[2] * o[1] and (o[3] - 1) * 16 + o[4] == c.Lk
        seen["D"].add(o[0]); seen["last_rows"].add((o[0], o[5])); seen["tiles"].add(o[3]); seen["last"].add(o[4])
        seen["qpad"].add(o[6]); seen["vpad"].add(o[7]); seen["qblocks"].add((o[0], o[2]))
    assert seen["D"] == {32, 64} and seen["tiles"] == {1, 2, 3} and seen["last"] >= {1, 15, 16}
    assert seen["last_rows"] >= {(32, 1), (32, 63), (32, 64), (64, 1), (64, 31), (64, 32)}
    assert seen["qblocks"] >= {(32, 1), (32, 2), (64, 1), (64, 2)}
    assert seen["qpad"] >= {0, 7, 4} and seen["vpad"] >= {0, 7, 4}                  # whole lanes, one channel, half a lane
    got = {(c.dqk, c.dv): FE.attn_route(c)[1][0] for c in FE.ATTN_CASES}
    assert set(got) >= set(FE.WIDTHS)
    assert got[(32, 32)] == 32 and got[(32, 33)] == 64 and got[(33, 32)] == 64 and got[(20, 40)] == 64 and got[(40, 8)] == 64
    for D, dq in ((32, 32), (64, 64)):
        assert {c.pattern for c in FE.ATTN_CASES if FE.attn_route(c)[1][0] == D} >= set(FE.PATTERNS) | {"random"}
    assert {c.Lk for c in FE.ATTN_CASES} >= {1, 15, 16, 17, 33}
    assert {c.Lq for c in FE.ATTN_CASES if FE.attn_route(c)[1][0] == 32} >= {1, 63, 64, 65}
    assert {c.Lq for c in FE.ATTN_CASES if FE.attn_route(c)[1][0] == 64} >= {1, 31, 32, 33}


def test_route_queries_refuse_as_their_entries():
    """Dummy pointers, no GPU: the refusals of the route queries are those of the entries, before any launch."""
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    out = (ctypes.c_int32 * 8)()
    E, U = -1, -2
    qk = lambda B=1, heads=1, d=4, L=4: (h.lc_qk_norm_cm_route(B, heads, d, L, out),
                                         h.lc_qk_norm_cm_jvp(p, d * L, L, p, d * L, L, p, p, d * L, L, p, d * L, L, B, heads, d, L, None))
    for kw, rc in ((dict(B=0), E), (dict(heads=0), E), (dict(d=0), E), (dict(L=0), E), (dict(d=65), U), (dict(B=256, heads=256), U)):
        assert qk(**kw) == (rc, rc), kw
    at = lambda BH=1, Lq=1, Lk=1, dqk=4, dv=4: (h.lc_attention_jvp_route(BH, Lq, Lk, dqk, dv, out),
                                                h.lc_attention_jvp_fwd(p, p, p, p, p, p, p, p, p, BH, Lq, Lk, dqk, dv, 1.0, None))
    for kw, rc in ((dict(BH=0), E), (dict(Lq=0), E), (dict(Lk=0), E), (dict(dqk=0), E), (dict(dv=0), E), (dict(dqk=65), U),
                   (dict(dv=65), U), (dict(BH=65536), U)):
        assert at(**kw) == (rc, rc), kw
    gn = lambda B=1, C=4, H=2, W=2, G=2: (h.lc_groupnorm_jvp_route(B, C, H, W, G, C * H * W, C * H * W, 0, 0, out),
                                          h.lc_groupnorm_jvp_stats(p, C * H * W, p, C * H * W, p, B, C, H, W, G, None))
    for kw, rc in ((dict(B=0), E), (dict(C=0), E), (dict(H=0), E), (dict(W=0), E), (dict(G=0), E), (dict(G=3), E), (dict(B=65536), U)):
        assert gn(**kw) == (rc, rc), kw
    assert h.lc_groupnorm_jvp_route(1, 4, 2, 2, 2, 16, 16, 0, 0, None) == E
    assert h.lc_qk_norm_cm_route(1, 1, 4, 4, None) == E and h.lc_attention_jvp_route(1, 1, 1, 4, 4, None) == E
    assert h.lc_groupnorm_jvp_route(1, 4, 2, 2, 2, 16, 16, 0, 0, out) == 0 and list(out) == [4096, 1, 1, 0, 1, 1, 1, 4]
    assert h.lc_qk_norm_cm_route(2, 65, 5, 257, out) == 0 and list(out)[:4] == [16, 2, 260, 2]
    assert h.lc_attention_jvp_route(3, 65, 33, 32, 33, out) == 0 and list(out) == [64, 32, 3, 3, 1, 1, 0, 7]


# ------------------------------------------------------------------------------------------------ q / k references
@pytest.mark.parametrize("c", FE.QK_CASES, ids=ids)
def test_qk_references_oracle_cap_and_defect(c):
    r = FE.qk_ref(c)
    x, dx, gy, g = (r.t[k].double() for k in ("x", "dx", "gy", "g"))
    # the closed forms against torch.func.jvp and autograd of the plain formula.  Exactly zero tokens are left out of the
    # tangent / gradient comparison: the derivative of |x| at 0 is torch's choice (its float64 result is finite: checked)
    y_t, dy_t = torch.func.jvp(lambda a: _qk_ref(a, g, c.heads), (x,), (dx,))
    xr, gr = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
    _qk_ref(xr, gr, c.heads).backward(gy)
    assert torch.isfinite(dy_t).all() and torch.isfinite(xr.grad).all() and torch.isfinite(gr.grad).all()
    nonzero = torch.ones(c.L, dtype=torch.bool)
    for t, kind in r.t["kinds"].items():
        nonzero[t] = kind != 0
    assert float(FE.qk_token_err(y_t, r.y, c.heads)[0].max()) <= 1e-13
    for got, ref, sc in ((dy_t, r.dy, r.scale_dy), (xr.grad, r.gx, r.scale_gx)):
        e, _ = FE.qk_token_err(got[..., nonzero], ref[..., nonzero], c.heads, None if sc is None else sc[..., nonzero])
        assert float(e.max()) <= 1e-12, (c.name, float(e.max()))
    assert abs(float(gr.grad) - r.dg) <= 1e-12 * r.S_dg
    # clamped tokens carry tangents near 1e12 |dx| (finite in float32), zero tokens come back as exactly zero in y
    if c.tiny:
        big = max(float(r.dy[..., t].abs().max()) for t, k in r.t["kinds"].items() if k != 2)
        assert 1e10 < big < 1e15
        assert all(float(r.y[..., t].abs().max()) == 0.0 for t, k in r.t["kinds"].items() if k == 0)
    # the float32 oracle: not exact, and under the cap
    assert 0 < r.e32 <= FE.ORACLE_CAP * FE.TOL_QK, (c.name, r.e32)
    assert r.e32_dg <= FE.ORACLE_CAP * FE.TOL_QK, (c.name, r.e32_dg)
    # the defect: the projection dropped at the clamp's neighbours (norm 3e-12) moves such a token by >= 16 bounds
    if c.tiny and c.d > 1:
        _, bad, _, _ = FE.qk_closed(x, dx, g, c.heads, defect="no-proj")
        e, _ = FE.qk_token_err(bad, r.dy, c.heads, r.scale_dy)
        nb = [t for t, k in r.t["kinds"].items() if k == 2]
        assert nb and float(e[..., nb].min()) >= FE.SIGNAL_OVER_BOUND * r.bound, (c.name, float(e[..., nb].min()), r.bound)
    if c.tiny and c.d == 1:
        # d = 1: the dropped projection leaves s w where 0 belongs: exactly one scale
        _, bad, _, _ = FE.qk_closed(x, dx, g, c.heads, defect="no-proj")
        e, _ = FE.qk_token_err(bad, r.dy, c.heads, r.scale_dy)
        assert float(e.max()) >= FE.SIGNAL_OVER_BOUND * r.bound


# ------------------------------------------------------------------------------------------------ GroupNorm references
@pytest.mark.parametrize("c", FE.GN_CASES, ids=ids)
def test_groupnorm_references_and_defects(c):
    r = FE.gn_ref(c)
    t = r.t
    d64 = lambda k: t[k].double() if k in t else None
    prim = (d64("x"),) + ((d64("scale"), d64("shift")) if c.ada else ())
    tang = (d64("dx"),) + ((d64("dscale"), d64("dshift")) if c.ada else ())
    f = lambda x_, *ss: _gn_ref(x_, c.G, FE.EPS, d64("gamma"), d64("beta"), ss[0] if c.ada else None, ss[1] if c.ada else None, c.act)
    y_t, dy_t = torch.func.jvp(f, prim, tang)
    assert float(FE.gn_group_err(y_t, r.y, c.G, r.skip_y).max()) <= 1e-9
    # (a tangent proportional to x cancels to rounding in dn: what is left of float64's own rounding is held against the
    #  float32 oracle's figure, six orders above it)
    assert float(FE.gn_group_err(dy_t, r.dy, c.G, r.skip_dy).max()) <= max(1e-9, 1e-6 * r.e32_dy), c.name
    assert (r.const is not None) == (c.data == "constant")
    assert r.e32_y > 0 and r.e32_dy > 0
    assert r.bound_y <= 1e-2 and r.bound_dy <= 1e-2, (r.bound_y, r.bound_dy)
    if r.const is not None:
        cy, cdy = FE.gn_const_closed(t, c, r.const)
        cpg = c.C // c.G
        sl = slice(r.const * cpg, (r.const + 1) * cpg)
        assert float((r.y[:, sl] - cy[:, :, None, None]).abs().max()) <= 1e-12
        if c.dxmode == "prop":
            assert float((r.dy[:, sl] - cdy[:, :, None, None]).abs().max()) <= 1e-9
        by, bdy = FE.gn_const_bounds(t, c, r.const)
        assert float(by.max()) <= 1e-2 and float(bdy.max()) <= 1e-1
    # the defect: the primal's maxima handed to the tangent -- per sample max|y| and max|dy| differ by far more than 16
    # bounds of either (the GPU test holds the slots to BIT equality with the kernel's own outputs)
    my, mdy = r.y.abs().amax((1, 2, 3)), r.dy.abs().amax((1, 2, 3))
    assert float(((my - mdy).abs() / torch.maximum(my, mdy)).min()) >= FE.SIGNAL_OVER_BOUND * max(r.bound_y, r.bound_dy), c.name
    # the defect: mean(n dx) left out of dn
    if c.dxmode == "rand" and c.data is None:
        _, bad = FE.gn_closed(t, c.G, c.act, torch.float64, defect="no-mndx")
        assert float(FE.gn_group_err(bad, r.dy, c.G).max()) >= FE.SIGNAL_OVER_BOUND * r.bound_dy, c.name


def test_structured_rows_reach_a_large_mean_and_a_cancelling_tangent():
    rows = {c.name: c for c in FE.GN_CASES if c.data}
    def ratio(c):
        mean, var, _ = FE.GS.group_stats64(FE.gn_operands(c)[0]["x"], c.G)
        live = var > 0
        return float((mean.abs()[live] / var[live].sqrt()).max())
    assert ratio(rows["step8-a4-rand"]) >= 1700 and ratio(rows["common-prop"]) >= 3000
    # a tangent proportional to x: dn = PROP n eps / (var + eps) cancels where var >> eps (the control's unit spread),
    # |dy| is carried by the AdaGN tangents
    c = rows["control-prop"]
    r = FE.gn_ref(c)
    t = dict(r.t)
    t.pop("dscale"), t.pop("dshift")
    t["dscale"], t["dshift"] = torch.zeros_like(r.t["dscale"]), torch.zeros_like(r.t["dshift"])
    _, dn_only = FE.gn_closed(t, c.G, c.act, torch.float64)
    assert float(dn_only.norm() / r.dy.norm()) < 1e-4


def test_chained_rows_have_the_stated_ratio():
    for name, f in FE.GN_CHAINED:
        t, w = FE.gn_chained_operands(name, f)
        y, dy = FE.gn_closed(t, 8, True, torch.float64)
        ratio = float(dy.abs().max() / y.abs().max())
        assert 0.1 * f <= ratio <= 10 * f, (name, ratio)


# ------------------------------------------------------------------------------------------------ attention references
def _defect_err(c, r, defect, drop=None):
    bad = FE.attn_closed(r.t, torch.float64, defect=defect, drop=drop)
    return max(FE.attn_elem_err(bad["o"], r.r["o"], r.r["S_o"]) / r.bound_o, FE.attn_elem_err(bad["do"], r.r["do"], r.r["S_do"]) / r.bound_do)


@pytest.mark.parametrize("c", FE.ATTN_CASES, ids=ids)
def test_attention_references_oracle_cap_and_defects(c):
    r = FE.attn_ref(c)
    t = r.t
    u = lambda n: t[n].double()[None]                                   # [1, BH, d, L]: _attn_ref's layout
    o_t, do_t = torch.func.jvp(lambda a, b, d: _attn_ref(a, b, d, t["scale"]), (u("q"), u("k"), u("v")), (u("dq"), u("dk"), u("dv")))
    assert FE.attn_elem_err(o_t[0], r.r["o"], r.r["S_o"]) <= 1e-13 and FE.attn_elem_err(do_t[0], r.r["do"], r.r["S_do"]) <= 1e-13
    S = torch.einsum("bct,bcs->bts", t["q"].double(), t["k"].double()) * t["scale"]
    assert float((torch.logsumexp(S, -1) * FE.LOG2E - r.r["lse"]).abs().max()) <= 1e-10
    # the float32 oracle: under the cap (the two-term bound is not vacuous)
    assert max(r.e32_o, r.e32_do) <= FE.ORACLE_CAP * FE.TOL_ATTN, (c.name, r.e32_o, r.e32_do)
    assert r.e32_lse <= FE.LSE_TOL
    # the pattern is what its name says, in float64 and in float32 alike
    S32 = torch.einsum("bct,bcs->bts", t["q"], t["k"]) * t["scale"]
    for s_ in (S, S32.double()):
        if c.pattern == "rising":
            assert bool((s_[..., 1:] > s_[..., :-1]).all())
        if c.pattern == "falling":
            assert bool((s_[..., 1:] < s_[..., :-1]).all()) and float((s_[..., 0] - s_[..., -1]).min()) * FE.LOG2E > 150
        if FE.attn_win(c) is not None:
            w = FE.attn_win(c)
            rest = torch.cat([s_[..., :w], s_[..., w + 1:]], -1)
            assert float((s_[..., w] - rest.amax(-1)).min()) * FE.LOG2E > 200
        if c.pattern == "equal":
            assert float(s_.abs().max()) == 0.0
        if c.pattern == "tied":
            assert bool((s_[..., 3] == s_[..., 20]).all()) and bool((s_.argmax(-1) == 3).all())
        if c.pattern == "offset500":
            assert 490 < float(s_.min()) * FE.LOG2E and float(s_.max()) * FE.LOG2E < 510
    if FE.attn_win(c) is not None:
        w = FE.attn_win(c)
        assert FE.attn_elem_err(t["v"].double()[:, :, w, None].expand_as(r.r["o"]), r.r["o"], r.r["S_o"]) <= 1e-14
        assert FE.attn_elem_err(t["dv"].double()[:, :, w, None].expand_as(r.r["do"]), r.r["do"], r.r["S_do"]) <= 1e-14
    # the defects, each at >= 16 bounds on every row it applies to
    if c.Lk > 1:
        heavy = int(r.r["p"].sum((0, 1)).argmax())                     # the key that carries the most weight
        assert _defect_err(c, r, "drop-key", heavy) >= FE.SIGNAL_OVER_BOUND, c.name
        assert _defect_err(c, r, "no-mu") >= FE.SIGNAL_OVER_BOUND, c.name
    if c.dqk > 1 and c.Lk > 1 and FE.attn_win(c) is None:               # (one key or one-hot: p is 0 / 1 whatever a channel adds)
        # the last live channel of q / k: the last channel of its lane when dqk % 8 == 0, a partly padded lane's otherwise
        assert _defect_err(c, r, "drop-channel", c.dqk - 1) >= FE.SIGNAL_OVER_BOUND, c.name


@pytest.mark.parametrize("c", FE.ATTN_BWD_CASES, ids=ids)
def test_attention_backward_reference_is_finite(c):
    ref = FE.attn_bwd_ref(c, torch.float64)
    assert all(bool(torch.isfinite(a).all()) for a in ref)
    assert all(float(a.abs().max()) > 0 for a in ref[2:]) or c.Lk == 1      # one key: p = 1, dq = dk = 0
