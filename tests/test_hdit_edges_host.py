"""The case tables of tests/test_hdit_edges.py, and the proof that they and their bounds mean something (CPU only).

Coverage is computed from the tables (block edges, grid-stride passes, channel quarters, key multiplicities, planted values
as they stand in the built operands); every float64 oracle equals torch autograd or an independent naive restatement on
its rows; the float32 oracle stays inside every bound on its own; and every mutant (a subtly wrong oracle, tests/_hdit_edges.py)
moves the worst figure of the rows it targets by at least SIGNAL_OVER_BOUND bounds.  The forward entries' refusals are
asked of the library with pointers that are never dereferenced."""
import ctypes
import math

import pytest
import torch

from tests import _hdit_edges as E

ids = lambda c: c.name
SIG = E.SIGNAL_OVER_BOUND
NA_FAST = [c for c in E.NA if c.d == 32] + [c for c in E.NA if c.d == 64 and c.scale == 2.5]    # the oracle checks' rows


def _close64(a, b, scale=None):
    scale = float(b.abs().max()) if scale is None else scale
    return float((a - b).abs().max()) <= 1e-11 * max(scale, 1e-300)


def test_names_are_unique_and_every_row_names_its_edge():
    for table in E.TABLES.values():
        assert len({c.name for c in table}) == len(table)
        assert all(c.edge for c in table)


# ------------------------------------------------------------------------------------------------ coverage
def _edge_kinds(ns, per):
    kinds = set()
    for n in ns:
        nb, last = E.blocks(n, per)
        kinds.add("one" if n == 1 else ("full" if last == per else "partial"))
        if nb > 1 and last < per:
            kinds.add("partial-after-full")
        if E.passes(n)[0] == 2 and E.passes(n)[1] % E.LANES:
            kinds.add("partial-second-pass")
    return kinds


def test_every_kernel_has_a_partial_a_full_and_a_single_block_row():
    need = {"one", "full", "partial", "partial-after-full"}
    stride = need | {"partial-second-pass"}
    assert _edge_kinds([c.L for c in E.RMS if c.form == "grid"], E.RMS_TOKENS) >= need
    assert _edge_kinds([c.mid * c.L for c in E.GEGLU], E.LANES) >= stride               # geglu_kernel, geglu_bwd_kernel
    for d in (32, 64):
        assert _edge_kinds([c.L for c in E.QK if c.d == d], E.LANES) >= need            # qk_prep_kernel and its backward
        assert _edge_kinds([c.grid[0] * c.grid[1] for c in E.NA if c.d == d], E.LANES) >= need - {"one"}
    assert min(c.grid[0] * c.grid[1] for c in E.NA) == 3                                # the smallest grid the windows allow here
    assert any(c.grid[0] * c.grid[1] > 256 and (c.grid[0] * c.grid[1]) % 256 for c in E.NA)
    assert _edge_kinds([c.C * c.H * c.W for c in E.PERMUTES], E.LANES) >= stride        # s2d_kernel, d2s_kernel
    assert _edge_kinds([c.C * c.h * c.w * c.P1 * c.P2 for c in E.LERP], E.LANES) >= stride   # d2s_kernel with lerp, lerp_bwd_kernel
    assert _edge_kinds([c.C * c.H * (c.W // c.P) for c in E.TOKENIZE], E.LANES) >= stride
    assert _edge_kinds([c.M * c.half for c in E.FOURIER], E.LANES) >= need
    # the sizes the issue names
    assert {c.mid * c.L for c in E.GEGLU} >= {1, 255, 257} and {c.M * c.half for c in E.FOURIER} >= {1, 255, 257}
    assert {c.L for c in E.QK if c.d == 32} == {c.L for c in E.QK if c.d == 64} == {1, 255, 256, 257}
    assert {(c.P1, c.P2) for c in E.PERMUTES} >= {(2, 2), (1, 4), (2, 1), (3, 2)}
    assert {(c.Cin, c.P) for c in E.TOKENIZE} >= {(2, 4), (1, 1), (3, 2)}
    # no model-sized shape: the largest operand is about 2M floats
    assert max(2 * c.mid * c.L * c.B for c in E.GEGLU) <= 2.2e6
    assert all(c.B * c.C * c.H * c.W <= 1.1e6 for c in E.PERMUTES) and all(c.B * max(c.C * c.H * (c.W // c.P), c.Cin * c.H * c.W) <= 1.1e6 for c in E.TOKENIZE)


def test_rmsnorm_rows_reach_every_quarter_shape_and_mode():
    g = [c for c in E.RMS if c.form == "grid"]
    assert {c.C for c in g} >= {1, 2, 3, 5, 96, 130} and {c.L for c in g} >= {1, 63, 64, 65, 129}
    assert {c.C % 4 for c in g} >= {0, 1, 2, 3} and {c.C for c in g if c.C < 4} == {1, 2, 3}
    for C in (1, 2, 3, 5, 96, 130):
        assert {c.mode for c in g if c.C == C} == set(E.MODES)
        cq = (C + 3) // 4
        lo, hi = E.rms_last_quarter(C)
        assert 0 <= lo < hi == C and hi - lo <= cq and lo % cq == 0
    assert E.rms_last_quarter(5) == (4, 5) and E.rms_last_quarter(130) == (99, 130) and E.rms_last_quarter(3) == (2, 3)
    r = [c for c in E.RMS if c.form == "rows"]
    assert {(c.B, c.C) for c in r} >= {(1, 3), (5, 3), (1, 256), (5, 256)} and {c.mode for c in r} == set(E.MODES)
    assert all(c.L == 1 for c in r)
    assert {c.xl for c in E.RMS} >= {"contig", "slice_hi", "bs1"}
    assert {c.L for c in E.RMS if c.mode == "gain" and c.B == 3} >= {1, 255, 257}
    assert {c.L for c in E.RMS if c.mode == "mod"} >= {1, 255, 257}
    z = [c for c in E.RMS if c.zero_token]
    assert z and all(bool((E.rms_ref(c).x[c.B - 1, :, c.L - 1] == 0).all()) and c.L % E.RMS_TOKENS == 1 for c in z)
    for c in E.RMS:
        if c.mode == "mod":
            assert not E.rms_ref(c).f.is_contiguous() or c.B == 1                     # a strided [B, C] view


def test_planted_values_are_in_the_built_operands():
    for c in E.GEGLU:
        x, _ = E.geglu_operands(c)
        gates = x[:, c.mid:].reshape(-1)
        if c.mid * c.L >= len(E.PLANTED_GATES):
            for v in E.PLANTED_GATES:
                hit = gates == v
                if v == 0.0:
                    hit = hit & (torch.signbit(gates) == (math.copysign(1.0, v) < 0))
                assert bool(hit.any()), (c.name, v)
        if E.passes(c.mid * c.L)[0] == 2:
            assert bool((x[-1, c.mid:].reshape(-1)[E.PASS:] == 40.0).any()), "no planted gate in the second pass"
    scales = set()
    for c in E.QK:
        t = E.qk_operands(c)
        scales |= set(t["scale"].tolist())
        norms = {"q": set(), "k": set()}
        for n, b, h, tok, norm in E.qk_plants(c.L):
            got = float(t[n][b, h * c.d:(h + 1) * c.d, tok].double().norm())
            assert (got == 0.0) if norm == 0 else abs(got / norm - 1) < 1e-6, (c.name, n, got, norm)
            # a factor 2 from the threshold: no rounding of the norm decides the branch
            assert got == 0 or got <= E.NORM_CLAMP / 1.9 or got >= E.NORM_CLAMP * 1.9
            norms[n].add(norm)
        assert norms["q"] == norms["k"] == set(E.PLANT_NORMS)
        assert {tok for _, _, _, tok, _ in E.qk_plants(c.L)} == {0, c.L - 1}
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()  # noqa: E731
    assert scales == {f32(0.7), E.LN100_F32, f32(5.2), 20.0, -30.0}
    assert {c.separate for c in E.QK} == {False, True}
    alphas = set()
    for c in E.LERP:
        alphas |= set(E.lerp_alpha(c).tolist())
        assert 0.0 in E.lerp_alpha(c).tolist(), "no channel at weight exactly 0.5"
    assert alphas == {f32(a) for a in E.ALPHAS}
    assert any(c.B == 3 for c in E.LERP)
    w = 1 / (1 + torch.exp(-torch.tensor(E.ALPHAS, dtype=torch.float32)))
    assert float(w[3]) == 0.5 and float(w[-1]) == 1.0 and 0 < float(w[0]) < 1e-8 and bool((w[:3] < 0.5).all()) and bool((w[4:] > 0.5).all())


def test_neighbourhood_rows_reach_every_multiplicity_scale_and_limit():
    grids = {c.grid for c in E.NA}
    assert grids >= {(5, 52, 5, 7), (1, 257, 1, 9), (3, 4, 3, 9), (3, 1, 3, 3), (2, 2, 1, 1)}
    mult = {g: E.na_multiplicities(g) for g in grids}
    assert mult[(3, 4, 3, 9)] == {2, 3} and mult[(3, 1, 3, 3)] == {3} and mult[(5, 52, 5, 7)] == {1} and mult[(9, 4, 9, 9)] == {2, 3}
    assert set().union(*mult.values()) == {1, 2, 3}
    for g in grids:
        assert {(c.d, c.scale) for c in E.NA if c.grid == g} == {(d, s) for d in (32, 64) for s in E.NA_SCALES}
    assert set(E.NA_SCALES) == {1.0, 0.125, 2.5}
    assert any(g[2] * g[3] == 81 and g[1] < g[3] for g in grids) and any(g[3] // 2 == g[1] for g in grids)
    assert any(g[1] == 1 for g in grids) and any(g[0] == g[2] == 1 for g in grids) and any(c.o_strided for c in E.NA)
    h, w, kh, kw = E.NA_REFUSED_GRID
    assert kh * kw == 81 and kw // 2 > w          # the issue's 9 x 3 grid: what the entries refuse (asserted below)
    # the looped table on the (2, 2, 1, 1) grid is the identity
    assert E.na_keys((2, 2, 1, 1)).reshape(-1).tolist() == [0, 1, 2, 3]


def test_neighbourhood_rows_are_conditioned_for_a_per_token_figure():
    """dq and dk of a token cancel twice; the rows keep that condition number under NA_KAPPA_MAX, so that a few 2^-24 per
    term stays inside TOL_NA_BWD whichever float32 evaluation makes them."""
    worst = 0.0
    for c in E.NA:
        if c.grid[2] * c.grid[3] > 1:
            kq, kk = E.na_kappa(c)
            assert kq <= E.NA_KAPPA_MAX and kk <= E.NA_KAPPA_MAX, (c.name, kq, kk)
            worst = max(worst, kq, kk)
    assert 4 * 2.0 ** -24 * E.NA_KAPPA_MAX <= E.TOL_NA_BWD and worst > 8     # conditioned, not trivial


# ------------------------------------------------------------------------------------------------ oracles
@pytest.mark.parametrize("c", E.RMS, ids=ids)
def test_rmsnorm_oracle_is_autograd(c):
    r = E.rms_ref(c)
    d = lambda t: None if t is None else t.double()  # noqa: E731
    y, dx, df = E.rms_autograd(d(r.x), d(r.f), c.mode, d(r.dy))
    assert _close64(r.y, y) and _close64(r.dx, dx)
    assert (df is None) == (r.df is None)
    if df is not None:
        assert _close64(r.df, df, float(r.S_df.max())) and float(r.S_df.min()) > 0
    if c.zero_token:
        assert float(r.y[c.B - 1, :, c.L - 1].abs().max()) == 0.0
        g = d(r.dy)[c.B - 1, :, c.L - 1] * (1.0 if c.mode == "plain" else (d(r.f) if c.mode == "gain" else 1 + d(r.f)[c.B - 1]))
        assert _close64(r.dx[c.B - 1, :, c.L - 1], g / math.sqrt(E.EPS))          # r = 1 / sqrt(eps), no projection


@pytest.mark.parametrize("c", E.GEGLU, ids=ids)
def test_geglu_oracle_is_autograd(c):
    r = E.geglu_ref(c)
    y, dx = E.geglu_autograd(r.x.double(), r.dy.double(), c.mid)
    assert float(((r.y - y).abs() / r.S_y.clamp_min(1e-300)).max()) < 1e-12
    assert float(((r.dx - dx).abs() / r.S_dx.clamp_min(1e-300)).max()) < 1e-12
    assert torch.isfinite(r.y).all() and torch.isfinite(r.dx).all()
    assert bool((r.S_y == 0).any())                       # the planted +-0.0 gates: the result there is exactly 0


@pytest.mark.parametrize("c", E.QK, ids=ids)
def test_qk_prep_closed_form_is_autograd(c):
    r = E.qk_ref(c)
    dq, dk, ds = E.qk_autograd(r.t)
    assert _close64(r.dq, dq) and _close64(r.dk, dk) and _close64(r.ds, ds, float(r.S_ds.max()))
    # per planted token as well: the clamped ones carry du / 1e-6 with no projection term
    for n, b, h, tok, norm in E.qk_plants(c.L):
        sl = (b, slice(h * c.d, (h + 1) * c.d), tok)
        a, g = (r.dq, dq) if n == "q" else (r.dk, dk)
        assert _close64(a[sl], g[sl]), (n, norm)
        if norm == 0:
            assert float((r.q if n == "q" else r.k)[sl].abs().max()) == 0.0
    above = r.t["scale"] > E.LN100_F32
    assert bool((r.ds[above] == 0).all()) and bool((r.S_ds[above] == 0).all()) and bool((r.S_ds[~above] > 0).all())


@pytest.mark.parametrize("c", NA_FAST, ids=ids)
def test_neighbourhood_looped_gather_is_the_index_gather(c):
    r = E.na_ref(c)
    assert _close64(r.ref["o"], E.na_gather_ref(r.t, c))
    # lse is the logsumexp of the scaled scores, written out for one query
    key = E.na_keys(c.grid)
    q, k = (E.heads_view(r.t[n].double(), E.NA_HEADS) for n in ("q", "k"))
    t0 = key.shape[0] - 1
    s = torch.stack([c.scale * (q[1, 2, :, t0] * k[1, 2, :, kk]).sum() for kk in key[t0].tolist()])
    assert abs(float(torch.logsumexp(s, 0)) - float(r.ref["lse"][1 * E.NA_HEADS + 2, t0])) < 1e-11
    if c.grid == (2, 2, 1, 1):
        assert torch.equal(r.ref["o"], r.t["v"].double()) and float(r.ref["dq"].abs().max()) == 0.0
        assert torch.equal(r.ref["dv"], r.t["do"].double())


@pytest.mark.parametrize("c", E.LERP, ids=ids)
def test_lerp_oracle_is_autograd(c):
    r = E.lerp_ref(c)
    out, dy, dskip, dalpha = E.lerp_autograd(r.t, c)
    assert float(((r.out - out).abs() / r.S_out).max()) < 1e-12
    for n, a in (("dy", dy), ("dskip", dskip), ("dalpha", dalpha)):
        # autograd's own a (1 - a) loses eight digits at alpha = 20 (1 - a = 2e-9), the restatement's sigmoid(-alpha) none
        assert float(((r.bwd[n] - a).abs() / r.bwd["S_" + n].clamp_min(1e-300)).max()) < (1e-7 if n == "dalpha" else 1e-12), n
    x = E.permute_operands(E.PERMUTES[1])
    assert torch.equal(E.d2s_ref(E.s2d_ref(x, 2, 2), 2, 2), x)


def test_permute_restatements_are_the_index_formula():
    for c in E.PERMUTES[:-1]:
        x = E.permute_operands(c)
        y = E.s2d_ref(x, c.P1, c.P2)
        for p1 in range(c.P1):
            for p2 in range(c.P2):
                for ch in range(c.C):
                    assert torch.equal(y[:, (p1 * c.P2 + p2) * c.C + ch], x[:, ch, p1::c.P1, p2::c.P2])
        assert torch.equal(E.d2s_ref(y, c.P1, c.P2), x)


@pytest.mark.parametrize("c", E.TOKENIZE, ids=ids)
def test_tokenizer_oracle_is_the_naive_loop(c):
    r = E.tokenize_ref(c)
    assert float(((r.y - E.tokenize_naive(r.t, c)).abs() / r.S).max()) < 1e-12


# ------------------------------------------------------------------------------------------------ bounds
def _all_bounds():
    for c in E.RMS:
        r = E.rms_ref(c)
        yield from ((c.name, k, r.e32[k], r.bound[k]) for k in r.e32)
    for c in E.GEGLU:
        r = E.geglu_ref(c)
        yield from ((c.name, k, r.e32[k], r.bound[k]) for k in r.e32)
    for c in E.QK:
        r = E.qk_ref(c)
        yield from ((c.name, k, r.e32[k], r.bound[k]) for k in r.e32)
    for c in E.NA:
        r = E.na_ref(c)
        yield from ((c.name, k, r.e32[k], r.bound[k]) for k in r.e32)
    for c in E.LERP:
        r = E.lerp_ref(c)
        yield from ((c.name, k, r.e32[k], r.bound[k]) for k in r.e32)
    for c in E.TOKENIZE:
        r = E.tokenize_ref(c)
        yield (c.name, "y", r.e32, r.bound)
    for c in E.FOURIER:
        r = E.fourier_ref(c)
        yield (c.name, "y", r.e32, r.bound)


def test_the_float32_oracle_is_inside_every_bound_on_its_own():
    """On every row: finite, inside the bound without the margin applied to itself, and the bound two orders below a wrong
    or missing term (O(1))."""
    n = 0
    for name, k, e32, bnd in _all_bounds():
        assert e32 == e32 and e32 < E.INF, (name, k)
        assert e32 <= bnd and bnd <= 1e-2, (name, k, e32, bnd)
        n += 1
    assert n > 300


# ------------------------------------------------------------------------------------------------ signal
def _na_signal(c, mutant):
    r = E.na_ref(c)
    figs = E.na_figures(mutant, r.ref)
    return max(v / r.bound[k] for k, v in figs.items())


@pytest.mark.parametrize("c", [c for c in NA_FAST if c.grid[2] * c.grid[3] > 1], ids=ids)
def test_neighbourhood_mutants_are_seen(c):
    r = E.na_ref(c)
    # one key dropped from one window
    assert _na_signal(c, E.na_all(r.t, c, torch.float64, mask=E.na_drop_mask(r.t, c))) >= SIG
    # a repeated key counted once
    if max(E.na_multiplicities(c.grid)) > 1:
        assert _na_signal(c, E.na_all(r.t, c, torch.float64, mask=E.na_dedup_mask(c.grid))) >= SIG
    # clamp instead of wrap, wherever the two tables differ
    if not torch.equal(E.na_keys(c.grid), E.na_keys(c.grid, clamp=True)):
        assert _na_signal(c, E.na_all(r.t, c, torch.float64, key=E.na_keys(c.grid, clamp=True))) >= SIG
    # scale applied once instead of twice in dk
    if c.scale != 1.0:
        assert _na_signal(c, dict(dk=r.ref["dk"] / c.scale)) >= SIG
    # the last token of a partial block left at zero
    if (c.grid[0] * c.grid[1]) % E.LANES:
        for n in ("o", "dq", "dk", "dv"):
            assert _na_signal(c, {n: E.zero_last_token(r.ref[n])}) >= SIG


def test_the_wrap_and_multiplicity_mutants_have_rows():
    assert sum(not torch.equal(E.na_keys(g), E.na_keys(g, clamp=True)) for g, _ in E.NA_GRIDS) >= 4
    assert sum(max(E.na_multiplicities(g)) > 1 for g, _ in E.NA_GRIDS) >= 3


@pytest.mark.parametrize("c", E.QK, ids=ids)
def test_qk_prep_mutants_are_seen(c):
    r = E.qk_ref(c)
    # the projection term kept for a clamped token
    dq, dk, _, _ = E.qk_bwd(r.t, torch.float64, keep_projection=True)
    assert E.token_err(dq, r.dq, E.QK_HEADS) >= SIG * r.bound["dq"] and E.token_err(dk, r.dk, E.QK_HEADS) >= SIG * r.bound["dk"]
    # ln 100 compared with < instead of <=
    ds = E.qk_bwd(r.t, torch.float64, strict=True)[2]
    assert float(((ds - r.ds).abs() / r.S_ds.clamp_min(1e-300)).max()) >= SIG * r.bound["ds"]
    # the last token of a partial block left at zero
    if c.L % E.LANES:
        for n in ("q", "k", "dq", "dk"):
            assert E.token_err(E.zero_last_token(getattr(r, n)), getattr(r, n), E.QK_HEADS) >= SIG * r.bound[n]


@pytest.mark.parametrize("c", E.RMS, ids=ids)
def test_rmsnorm_mutants_are_seen(c):
    r = E.rms_ref(c)
    d = lambda t: None if t is None else t.double()  # noqa: E731
    # the last channel quarter skipped in the sum of squares
    y = E.rms_fwd(d(r.x), d(r.f), c.mode, skip_last_quarter=True)
    dx = E.rms_bwd(d(r.x), d(r.f), c.mode, d(r.dy), skip_last_quarter=True)[0]
    assert E.token_err(y, r.y) >= SIG * r.bound["y"], (E.token_err(y, r.y), r.bound["y"])
    assert E.token_err(dx, r.dx) >= SIG * r.bound["dx"], (E.token_err(dx, r.dx), r.bound["dx"])
    # the last token of a partial block left at zero
    if c.L % E.RMS_TOKENS and not c.zero_token:
        assert E.token_err(E.zero_last_token(r.y), r.y) >= SIG * r.bound["y"]
        assert E.token_err(E.zero_last_token(r.dx), r.dx) >= SIG * r.bound["dx"]
    # d(mod) / d(gain): the last token's term missing from the sum
    if r.df is not None:
        t = (d(r.dy) * d(r.x) * torch.rsqrt(d(r.x).pow(2).mean(1, keepdim=True) + E.EPS))[..., -1]
        broken = r.df - (t if c.mode == "mod" else t.sum(0))
        if not c.zero_token:
            assert E.elem_err(broken, r.df, r.S_df) >= SIG * r.bound["df"]


def test_second_pass_mutant_is_seen():
    """Element e + 4096 * 256 left unwritten, on every row that has a second pass."""
    n = 0
    for c in E.GEGLU:
        if E.passes(c.mid * c.L)[0] == 2:
            r = E.geglu_ref(c)
            assert E.elem_err(E.zero_second_pass(r.y), r.y, r.S_y) >= SIG * r.bound["y"]
            lo, hi = r.dx[:, :c.mid], r.dx[:, c.mid:]
            broken = torch.cat([E.zero_second_pass(lo), E.zero_second_pass(hi)], 1)
            assert E.elem_err(broken, r.dx, r.S_dx) >= SIG * r.bound["dx"]
            n += 1
    for c in E.LERP:
        if E.passes(c.C * c.h * c.w * c.P1 * c.P2)[0] == 2:
            r = E.lerp_ref(c)
            assert E.elem_err(E.zero_second_pass(r.out), r.out, r.S_out) >= SIG * r.bound["out"]
            assert E.elem_err(E.zero_second_pass(r.bwd["dskip"]), r.bwd["dskip"], r.bwd["S_dskip"]) >= SIG * r.bound["dskip"]
            # dy is written at the depth-to-space source of element e
            dy = E.s2d_ref(E.zero_second_pass(E.d2s_ref(r.bwd["dy"], c.P1, c.P2)), c.P1, c.P2)
            assert E.elem_err(dy, r.bwd["dy"], r.bwd["S_dy"]) >= SIG * r.bound["dy"]
            n += 1
    for c in E.TOKENIZE:
        if E.passes(c.C * c.H * (c.W // c.P))[0] == 2:
            r = E.tokenize_ref(c)
            assert E.elem_err(E.zero_second_pass(r.y), r.y, r.S) >= SIG * r.bound
            n += 1
    for c in E.PERMUTES:
        if E.passes(c.C * c.H * c.W)[0] == 2:
            x = E.permute_operands(c)
            y = E.s2d_ref(x, c.P1, c.P2)
            assert not torch.equal(E.zero_second_pass(y), y) and not torch.equal(E.zero_second_pass(x), x)
            n += 1
    assert n == 4


@pytest.mark.parametrize("c", E.LERP, ids=ids)
def test_lerp_branch_swap_shows_in_the_float32_bits(c):
    """The two formulas of torch.lerp are one value in exact arithmetic: swapped at weight exactly 0.5 they differ by a
    rounding of z - s, far below any bound.  The GPU test therefore holds the alpha = 0 channels to the float32
    restatement bit for bit (a bound of zero differing elements); here: the mutant differs from it in bits wherever the
    row has enough elements for a rounding to show, and nowhere outside those channels."""
    r = E.lerp_ref(c)
    half = E.lerp_alpha(c) == 0.0
    mutant = E.lerp_fwd(r.t, c, torch.float32, swap_at_half=True)[0]
    assert torch.equal(mutant[:, ~half], r.out32[:, ~half])
    differing = int((mutant[:, half] != r.out32[:, half]).sum())
    if c.B * c.h * c.w * c.P1 * c.P2 >= 60:
        assert differing > 0
    assert E.elem_err(mutant, r.out, r.S_out) <= r.bound["out"]                   # what a tolerance would have said


# ------------------------------------------------------------------------------------------------ refusals
def test_forward_entry_points_refuse_bad_arguments_before_any_launch():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    p = 4096                                   # never dereferenced: every call below must be refused first
    op = _lib.CmOperand(p, 0, 0, 8)
    nul = _lib.CmOperand(None, 0, 0, 8)
    r = ctypes.byref
    EI, EU = E.LC_EINVAL, E.LC_EUNSUP
    # rmsnorm: (x, x_bs, x_cs, f, f_bs, mode, y, y_bs, y_cs, B, C, L, eps)
    a = [p, 0, 8, p, 0, 1, p, 0, 8, 1, 8, 8, 1e-6, None]
    bad = lambda i, v: h.lc_hdit_rmsnorm_fwd(*(a[:i] + [v] + a[i + 1:]))  # noqa: E731
    assert bad(0, None) == EI and bad(6, None) == EI and bad(3, None) == EI     # no x, no y, mode 1 without f
    assert bad(5, 3) == EI and bad(10, 0) == EI and bad(12, 0.0) == EI and bad(2, 0) == EI
    assert bad(9, 70000) == EU
    # geglu
    assert h.lc_hdit_geglu_fwd(None, 0, p, 0, 1, 8, 8, None) == EI and h.lc_hdit_geglu_fwd(p, 0, None, 0, 1, 8, 8, None) == EI
    assert h.lc_hdit_geglu_fwd(p, 0, p, 0, 1, 0, 8, None) == EI and h.lc_hdit_geglu_fwd(p, 0, p, 0, 70000, 8, 8, None) == EU
    # q / k preparation: (q, q_bs, q_cs, k, k_bs, k_cs, scale, cos, sin, B, heads, d, L)
    q = [p, 0, 8, p, 0, 8, p, p, p]
    assert h.lc_hdit_qk_prep_fwd(*q, 1, 2, 48, 8, None) == EU                    # d = 48
    assert h.lc_hdit_qk_prep_fwd(*q, 40000, 2, 32, 8, None) == EU                # B * heads > 65535
    for i in (0, 3, 6, 7, 8):                                                    # null operands
        assert h.lc_hdit_qk_prep_fwd(*(q[:i] + [None] + q[i + 1:]), 1, 2, 32, 8, None) == EI
    assert h.lc_hdit_qk_prep_fwd(*(q[:2] + [0] + q[3:]), 1, 2, 32, 8, None) == EI
    # neighbourhood attention, both forwards: (q, k, v, o, o_bs, o_hs, o_cs[, lse], B, heads, d, h, w, kh, kw, scale)
    fw = lambda *g, B=1, heads=2, d=32, ops=(op, op, op), o=p: h.lc_hdit_na_fwd(  # noqa: E731
        *(r(x) for x in ops), o, 0, 0, 8, B, heads, d, *g, 1.0, None)
    tr = lambda *g, B=1, heads=2, d=32, ops=(op, op, op), o=p, lse=p: h.lc_hdit_na_train_fwd(  # noqa: E731
        *(r(x) for x in ops), o, 0, 0, 8, lse, B, heads, d, *g, 1.0, None)
    for f in (fw, tr):
        assert f(8, 16, 3, 9, d=48) == EU
        assert f(8, 16, 3, 9, B=40000) == EU                                     # B * heads > 65535
        assert f(8, 16, 3, 8) == EU and f(8, 16, 4, 9) == EU                     # even kw, even kh
        assert f(2, 16, 3, 9) == EU                                              # kh > h
        assert f(16, 16, 9, 11) == EU                                            # kh * kw > 81
        assert f(8, 2, 3, 9) == EU                                               # kw / 2 > w
        assert f(*E.NA_REFUSED_GRID) == EU                                       # 9 x 3 with a 9 x 9 window: kw / 2 = 4 > w = 3
        assert f(8, 16, 3, 9, ops=(nul, op, op)) == EI and f(8, 16, 3, 9, ops=(op, op, nul)) == EI
        assert f(8, 16, 3, 9, o=None) == EI and f(8, 0, 3, 9) == EI
    assert tr(8, 16, 3, 9, lse=None) == EI
    # permutes: (in, in_bs, out, out_bs, B, C, H, W, P1, P2) / (in, in_bs, out, out_bs, skip, skip_bs, alpha, B, C, h, w, P1, P2)
    assert h.lc_hdit_space_to_depth_fwd(p, 0, p, 0, 1, 4, 7, 8, 2, 2, None) == EU      # H % P1
    assert h.lc_hdit_space_to_depth_fwd(p, 0, p, 0, 1, 4, 8, 7, 2, 2, None) == EU      # W % P2
    assert h.lc_hdit_space_to_depth_fwd(None, 0, p, 0, 1, 4, 8, 8, 2, 2, None) == EI
    assert h.lc_hdit_space_to_depth_fwd(p, 0, None, 0, 1, 4, 8, 8, 2, 2, None) == EI
    assert h.lc_hdit_space_to_depth_fwd(p, 0, p, 0, 1, 4, 8, 8, 0, 2, None) == EI
    assert h.lc_hdit_depth_to_space_fwd(None, 0, p, 0, None, 0, None, 1, 4, 4, 4, 2, 2, None) == EI
    assert h.lc_hdit_depth_to_space_fwd(p, 0, None, 0, None, 0, None, 1, 4, 4, 4, 2, 2, None) == EI
    assert h.lc_hdit_depth_to_space_fwd(p, 0, p, 0, p, 0, None, 1, 4, 4, 4, 2, 2, None) == EI      # skip without alpha
    assert h.lc_hdit_depth_to_space_fwd(p, 0, p, 0, None, 0, None, 70000, 4, 4, 4, 2, 2, None) == EU
    # tokenizer: (x, x_bs, wt, pe, y, y_bs, B, Cin, C, H, W, P)
    t = [p, 0, p, p, p, 0]
    assert h.lc_hdit_tokenize_fwd(*t, 1, 2, 8, 4, 30, 4, None) == EU                   # W % P
    for i in (0, 2, 3, 4):
        assert h.lc_hdit_tokenize_fwd(*(t[:i] + [None] + t[i + 1:]), 1, 2, 8, 4, 32, 4, None) == EI
    assert h.lc_hdit_tokenize_fwd(*t, 1, 0, 8, 4, 32, 4, None) == EI
    # Fourier features
    assert h.lc_hdit_fourier_fwd(None, p, p, 4, 8, None) == EI and h.lc_hdit_fourier_fwd(p, None, p, 4, 8, None) == EI
    assert h.lc_hdit_fourier_fwd(p, p, None, 4, 8, None) == EI and h.lc_hdit_fourier_fwd(p, p, p, 0, 8, None) == EI
