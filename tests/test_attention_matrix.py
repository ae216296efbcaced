"""Every attention kernel route at its tile edges and at the ends of the inference range window.  `pytest -m gpu`.

The case table and the proof that it reaches all 26 instantiations are in tests/test_attention_matrix_host.py; the
float64 / float32 restatement is tests/_attention_oracle.py.  Every result is held to the existing tolerances
(`ATTN_TOL` of test_hip_parity.py, `TOL_ATTN_BWD` of test_training.py) by query, head and channel through
`check_profiles`, and every figure is printed before it is asserted (recorded in profiles/attention_matrix.txt).

Structured inputs make a confined fault a wrong number instead of noise: a marker value whose output IS one softmax
weight, a key that dominates late / in the second segment / early, q = 0, a single key, and operands that are views
into NaN-filled buffers (channel stride above L, heads apart, base off 16-byte alignment) with a guarded `out`.
(A single key is checked in the forward and in the log2-sum-exp only: its dq is exactly zero, which no relative figure
can judge.)

The marker and dominant-key inputs run through the inference entries only; the training (PRE) instantiations of the
same template get the table, q = 0 and the single key.

Range window: the inference split routes pre-scale by the constant 16.  The contract (include/lidarcrafter_hip.h) has
two parts, with m = max|x| for x = q * scale * log2(e), k, v.  Representable: 16 * m in [4, 32768) for all three.
Accurate (ATTN_TOL against float64): in addition m_q * m_k <= 32 / sqrt(d_qk + d_pos), scores that deviate by about one
nat (`joint_limit`).  `test_range_window*` asserts ATTN_TOL at every end of the accurate part -- q or k at 0.3 with the
partner on the joint limit, v at 0.3 and at 1500 -- and, with q or k at 1500 and the partner at 0.3 (product 450: near
one-hot weights, where the float32 oracle itself is at 1.6e-6 ... 2.5e-6), only what the contract claims there: a
finite result no worse than 4 x the float32 oracle's error.
"""
import ctypes

import pytest
import torch

from lidarcrafter_amd.testing import error_profiles, rel_l2, seeded_fill, seeded_randn
from tests import _attention_oracle as AO
from tests import _profile_cases as PC
from tests import test_attention_matrix_host as H
from tests.test_attention_matrix_host import Spec

pytestmark = pytest.mark.gpu
ATTN_TOL = PC.existing_lists()["attn_tol"]
PRECISIONS = ("f32", "f16x2")
LSE_TOL = 1e-5          # test_meanflow_training.py::test_attention_jvp_against_float64: 1e-5 * max(1, max |lse|)
SHARP_MARGIN = 4.0      # test_compute_frid_vs_float64_features' margin over the float32 oracle's own error


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def assert_profiles(got, ref32, ref64, keeps, tol, name):
    lines, fails = PC.check_profiles(got, ref32, ref64, keeps, tol, name=name)
    print("\n".join(lines))
    assert not any("NOT CHECKED" in ln for ln in lines), lines
    assert not fails, "\n".join(fails)


def run_cm(t, s, prec, out=None):
    """ops.attention_cm on a dict of device operands -> [B, heads, d_v, Lq]."""
    from lidarcrafter_amd import ops as K

    g = t.get
    o = K.attention_cm(t["q"], t["k"], t["v"], s.heads, H.scale_of(s), k2=g("k2"), v2=g("v2"), q_pos=g("q_pos"),
                       k_pos=g("k_pos"), k2_pos=g("k2_pos"), precision=prec, out=out)
    return o.reshape(s.B, s.heads, s.dv, s.Lq)


def units_of(t, s, dev):
    """The keys and values of `t` in unit form (lc_attention_pack_units), or None where the form does not take `s`."""
    from lidarcrafter_amd import ops as K

    if not K.AttnUnits.eligible(s.heads, s.Lk0, s.Lk1, s.dqk, s.dpos, s.dv):
        return None
    u = K.AttnUnits(s.B, s.heads, s.Lk0, s.Lk1, s.dqk, s.dpos, s.dv, dev)
    K.attention_pack_units(u, t["k"], "k"), K.attention_pack_units(u, t["v"], "v")
    if s.dpos:
        K.attention_pack_units(u, t["k_pos"], "k_pos")
    if s.Lk1:
        K.attention_pack_units(u, t["k2"], "k", segment=1), K.attention_pack_units(u, t["v2"], "v", segment=1)
        if s.dpos:
            K.attention_pack_units(u, t["k2_pos"], "k_pos", segment=1)
    return u


def run_units(t, s, u):
    from lidarcrafter_amd import ops as K

    return K.attention_units(t["q"], u, s.heads, H.scale_of(s), q_pos=t.get("q_pos")).reshape(s.B, s.heads, s.dv, s.Lq)


# ------------------------------------------------------------------------------------------------ forward, the table
@pytest.mark.parametrize("s", H.INFERENCE, ids=str)
def test_forward(dev, s):
    """Both precisions against float64 by query, head and channel; the split route against the fp32 route; the unit
    form bit-equal to attention_cm where it takes the shape."""
    assert H.fwd_route(s, 1, waves_env=-1) == H.fwd_route(s, 1), "LC_ATTN_WAVES is set: the table's 8-wave rows are not run as such"
    c = H.case(s)
    t = c.dev(dev)
    res = {}
    for prec in PRECISIONS:
        res[prec] = run_cm(t, s, prec)
        assert_profiles(res[prec], c.ref32[0], c.ref64[0], H.O_KEEPS, ATTN_TOL[prec], f"forward {tuple(s)} {prec} {H.fwd_route(s, prec == 'f16x2')}")
    d = rel_l2(res["f16x2"], res["f32"])
    print(f"forward {tuple(s)}: split against fp32 route {d:.3e}")
    assert d < 1e-5
    assert torch.equal(run_cm(t, s, "f16x2"), res["f16x2"])
    u = units_of(t, s, dev)
    if u is not None:
        assert torch.equal(run_units(t, s, u), res["f16x2"]), "attention_units differs from attention_cm"
        print(f"forward {tuple(s)}: attention_units bit-equal")


def test_units_are_reached():
    """(no GPU work) the unit form takes at least one 4-wave and one 8-wave row of the table."""
    from lidarcrafter_amd import ops as K

    el = [s for s in H.INFERENCE if K.AttnUnits.eligible(s.heads, s.Lk0, s.Lk1, s.dqk, s.dpos, s.dv)]
    assert {H.fwd_route(s, 1)[3] for s in el} == {4, 8}


def test_qkv_projection_units(dev, monkeypatch):
    """Units written by the qkv projection's epilogue, at the smallest shape it takes (128 channels, 32 keys) with a
    31-key second segment: bit-equal to attention_cm on the plain projection, and that within ATTN_TOL of float64."""
    from lidarcrafter_amd import ops as K

    monkeypatch.setattr(K, "PS1X1_MIN_CO", 128)
    got, want, ref32, ref64, _ = _qkv_units_run(dev, 1.0, 1.0, 1.0)
    assert torch.equal(got, want)
    assert_profiles(got, ref32, ref64, H.O_KEEPS, ATTN_TOL["f16x2"], "qkv projection units")


def _qkv_units_run(dev, fq, fk, fv):
    """The layout model's block in small: GroupNorm -> 1x1 qkv projection (rows scaled by fq / fk / fv) -> attention over
    the projected keys ++ 31 further keys, positional parts on q and k.  -> (units route, attention_cm route, oracle 32 / 64)."""
    from lidarcrafter_amd import ops as K
    from lidargen.models.unets.nn import GroupNorm32, PointwiseConv1d

    B, C, L, L2, d = 4, 128, 32, 31, 32
    heads = C // d
    norm = seeded_fill(GroupNorm32(32, C), salt=41).to(dev)
    proj = seeded_fill(PointwiseConv1d(C, 3 * C), salt=42).to(dev)
    with torch.no_grad():
        for i, f in enumerate((fq, fk, fv)):
            proj.weight[i * C:(i + 1) * C] *= f
            if proj.bias is not None:
                proj.bias[i * C:(i + 1) * C] *= f
        x = seeded_randn(B, C, L, seed=43).to(dev)
        pos_q = (seeded_randn(B, heads * d, L, seed=44) * fq).to(dev)
        pos_k = (seeded_randn(B, heads * d, L, seed=48) * fk).to(dev)
        k2, k2p = (seeded_randn(B, C, L2, seed=45) * fk).to(dev), (seeded_randn(B, C, L2, seed=47) * fk).to(dev)
        v2 = (seeded_randn(B, C, L2, seed=46) * fv).to(dev)
        scale = (2 * d) ** -0.5
        assert K.presplit_1x1(C, 3 * C, 32) and K.qkv_units_ok(C, heads, L)
        qkv = proj(norm(x, split_for=proj._packed))
        want = K.attention_cm(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], heads, scale, k2=k2, v2=v2, q_pos=pos_q, k_pos=pos_k,
                              k2_pos=k2p, precision="f16x2")
        u = K.AttnUnits(B, heads, L, L2, d, d, d, dev)
        K.attention_pack_units(u, pos_k, "k_pos")
        K.attention_pack_units(u, k2, "k", 1), K.attention_pack_units(u, v2, "v", 1), K.attention_pack_units(u, k2p, "k_pos", 1)
        q = K.qkv_project_units(norm(x, split_for=proj._packed), proj._packed, proj.weight, proj.bias, u)
        got = K.attention_units(q, u, heads, scale, q_pos=pos_q)
    t = dict(q=qkv[:, :C], k=qkv[:, C:2 * C], v=qkv[:, 2 * C:], q_pos=pos_q, k_pos=pos_k, k2=k2, k2_pos=k2p, v2=v2)
    c = AO.attention_case({n: a.detach().cpu().contiguous() for n, a in t.items()}, heads, scale)
    c.amax = _group_amax(c.t, scale)
    shape = (B, heads, d, L)
    return got.reshape(shape), want.reshape(shape), c.ref32[0], c.ref64[0], c


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("mag", H.DO_MAGNITUDES)
@pytest.mark.parametrize("fwd,bwd", [("f16x2", "f16x2"), ("f32", "f32"), ("f16x2", "f32")])
@pytest.mark.parametrize("s", H.TRAINING, ids=str)
def test_training(dev, s, fwd, bwd, mag, monkeypatch):
    """autograd.FlashAttention: o, the log2-sum-exp the forward writes, dq by query, dk and dv by key against float64;
    a second run gives the same bits."""
    from lidarcrafter_amd import autograd as AG

    if fwd == bwd:
        precision = fwd
    else:
        precision = None
        monkeypatch.setattr(AG, "TRAIN_ATTN_FWD_PRECISION", fwd)
        monkeypatch.setattr(AG, "TRAIN_ATTN_BWD_PRECISION", bwd)
    c = H.case(s, mag)
    hd = lambda n: AO.heads_of(c.t[n], s.heads).contiguous().to(dev)

    def run():
        q, k, v = (hd(n).requires_grad_() for n in ("q", "k", "v"))
        o = AG.FlashAttention.apply(q, k, v, c.scale, precision)
        lse = o.grad_fn.saved_tensors[4].clone().reshape(s.B, s.heads, s.Lq)
        o.backward(hd("do"))
        return o.detach(), lse, q.grad, k.grad, v.grad

    got = run()
    name = f"training {tuple(s)} fwd {fwd} bwd {bwd} dO {mag:g}"
    assert_profiles(got[0], c.ref32[0], c.ref64[0], H.O_KEEPS, ATTN_TOL[fwd], name + " o")
    lse64 = c.ref64[1]
    e, bound = float((got[1].double().cpu() - lse64).abs().max()), LSE_TOL * max(1.0, float(lse64.abs().max()))
    print(f"{name} lse: max error {e:.3e} (float32 oracle {float((c.ref32[1].double() - lse64).abs().max()):.3e}, bound {bound:.2e})")
    assert e <= bound
    for i, n in ((2, "dq"), (3, "dk"), (4, "dv")):
        assert_profiles(got[i], c.ref32[i], c.ref64[i], H.GRAD_KEEPS, PC.TOL_ATTN_BWD, f"{name} {n}")
    again = run()
    for a, b, n in zip(got, again, ("o", "lse", "dq", "dk", "dv")):
        assert torch.equal(a, b), f"{name}: {n} differs between two runs"


# ------------------------------------------------------------------------------------------------ structured inputs
def _plain(s, seed):
    mk = lambda c, L, sd: seeded_randn(s.B, s.heads * c, L, seed=seed + sd)
    t = dict(q=mk(s.dqk, s.Lq, 1), k=mk(s.dqk, s.Lk0, 2), v=mk(s.dv, s.Lk0, 3))
    if s.dpos:
        t.update(q_pos=mk(s.dpos, s.Lq, 4), k_pos=mk(s.dpos, s.Lk0, 5))
    if s.Lk1:
        t.update(k2=mk(s.dqk, s.Lk1, 6), v2=mk(s.dv, s.Lk1, 7))
        if s.dpos:
            t["k2_pos"] = mk(s.dpos, s.Lk1, 8)
    return t


def _to(t, dev):
    return {n: a.to(dev) for n, a in t.items()}


def _key(t, s, name, pos):
    """The column of key `pos` of operand `name` ("k" / "v") across the two segments (a view)."""
    return t[name][:, :, pos] if pos < s.Lk0 else t[name + "2"][:, :, pos - s.Lk0]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("B,heads", [(2, 2), (16, 8)], ids=["4 waves", "8 waves"])
def test_marker_value(dev, B, heads, prec):
    """V = 0 except channel 0 of one key s*: o[channel 0, t] is the softmax weight of s*, every other channel exactly 0.
    s* on both sides of the first tile edge, of the segment edge, and the last key."""
    s = Spec(B, heads, 33, 129, 45, 32, 8, 8)
    assert H.fwd_route(s, 1, waves_env=-1)[3] == (8 if B * heads >= 128 else 4)
    base = _plain(s, 820)
    for star in (31, 32, s.Lk0 - 1, s.Lk0, s.Lk0 + s.Lk1 - 1):
        t = dict(base, v=torch.zeros_like(base["v"]), v2=torch.zeros_like(base["v2"]))
        _key(t, s, "v", star).reshape(s.B, s.heads, s.dv)[:, :, 0] = 1.0
        c = AO.attention_case(t, s.heads, H.scale_of(s))
        o = run_cm(_to(t, dev), s, prec).cpu()
        w64 = c.ref64[0][:, :, 0]
        e, e32 = rel_l2(o[:, :, 0], w64), rel_l2(c.ref32[0][:, :, 0], w64)
        worst = float(((o[:, :, 0].double() - w64).abs() / w64).max())
        print(f"marker s* = {star} {prec} B*heads {B * heads}: weights rel-L2 {e:.3e} (float32 oracle {e32:.3e}), worst single weight {worst:.3e}")
        assert e < ATTN_TOL[prec]
        assert bool((o[:, :, 1:] == 0).all()), "a channel of V = 0 is not exactly 0"


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("where", ["last ragged tile", "segment 1", "first tile"])
def test_dominant_key(dev, where, prec):
    """One key beats every other by 12 nats for every query: in the last ragged tile (the running maximum moves at the
    very end), in the second segment, or in the first tile (it never moves again and only weak keys follow)."""
    s = Spec(2, 2, 129, 129, 0 if where == "last ragged tile" else 13, 24, 8, 40)
    star = {"last ragged tile": s.Lk0 - 1, "segment 1": s.Lk0 + 5, "first tile": 3}[where]
    t = _plain(s, 840)
    scale = H.scale_of(s)
    AO.heads_of(t["q"], s.heads)[:, :, 0] = 3.0                       # channel 0 of every head: q = 3, k = 0 but for s*
    AO.heads_of(t["k"], s.heads)[:, :, 0] = 0.0
    if s.Lk1:
        AO.heads_of(t["k2"], s.heads)[:, :, 0] = 0.0
    _key(t, s, "k", star).reshape(s.B, s.heads, s.dqk)[:, :, 0] = (12.0 + 4.0) / (3.0 * scale)   # 12 nats over a +4 sigma rival
    c = AO.attention_case(t, s.heads, scale)
    o = run_cm(_to(t, dev), s, prec)
    e, e32 = rel_l2(o, c.ref64[0]), rel_l2(c.ref32[0], c.ref64[0])
    bound = max(ATTN_TOL[prec], SHARP_MARGIN * e32)
    print(f"dominant key in {where} (s* = {star}) {prec}: {e:.3e} (float32 oracle {e32:.3e}, bound {bound:.2e})")
    assert e <= bound
    k = error_profiles(o, c.ref64[0], ((3,),))["profiles"][(3,)]
    r = error_profiles(c.ref32[0], c.ref64[0], ((3,),))["profiles"][(3,)]
    print(f"  by query: worst {k['worst']:.3e} at {k['index']} (float32 oracle {r['worst']:.3e})")
    assert k["worst"] <= max(ATTN_TOL[prec], SHARP_MARGIN * r["worst"])


@pytest.mark.parametrize("s", [Spec(2, 2, 129, 33, 13, 32, 8, 40), Spec(16, 8, 33, 127, 0, 24, 0, 8), Spec(2, 2, 5, 1, 0, 8, 0, 64)], ids=str)
def test_zero_queries_and_single_key(dev, s):
    """q = 0: every weight is 1 / Lk, o is the mean of v and the log2-sum-exp is log2(Lk) -- with Lk = 1 in the last case,
    where o is v itself whatever q holds."""
    from lidarcrafter_amd import autograd as AG

    t = _plain(s, 860)
    Lk = s.Lk0 + s.Lk1
    if Lk > 1:
        t["q"].zero_()
        if s.dpos:
            t["q_pos"].zero_()
    c = AO.attention_case(t, s.heads, H.scale_of(s))
    vh = AO.heads_of(t["v"], s.heads).double()
    if s.Lk1:
        vh = torch.cat([vh, AO.heads_of(t["v2"], s.heads).double()], -1)
    mean = vh.mean(-1, keepdim=True).expand(-1, -1, -1, s.Lq)
    assert rel_l2(c.ref64[0], mean) < 1e-14
    for prec in PRECISIONS:
        e = rel_l2(run_cm(_to(t, dev), s, prec), mean)
        print(f"q = 0 / single key {tuple(s)} {prec}: o against mean(v) {e:.3e}")
        assert e < ATTN_TOL[prec]
    if s.dpos == 0 and s.Lk1 == 0:
        hd = lambda n: AO.heads_of(t[n], s.heads).contiguous().to(dev).requires_grad_()
        for prec in PRECISIONS:
            o = AG.FlashAttention.apply(hd("q"), hd("k"), hd("v"), c.scale, prec)
            lse = o.grad_fn.saved_tensors[4].double().cpu().reshape(s.B, s.heads, s.Lq)
            e = float((lse - c.ref64[1]).abs().max())
            bound = LSE_TOL * max(1.0, float(c.ref64[1].abs().max()))
            print(f"q = 0 / single key {tuple(s)} training {prec}: lse max error {e:.3e} (bound {bound:.2e}), o {rel_l2(o, mean):.3e}")
            assert e <= bound and rel_l2(o, mean) < ATTN_TOL[prec]
            if Lk > 1:
                assert float((c.ref64[1] - AO.log2_keys(Lk)).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ poisoned surroundings
GAP = 8          # NaN channel rows behind every head: more than the 7 rows an unguarded 8-row unit can overrun
MARK = -7.5


def _poisoned(x, heads, dev):
    """x [B, heads * d, L] -> (lc_cm_operand, keep-alive): the values inside a NaN-filled buffer with channel stride
    L + 3, GAP NaN rows behind every head's d rows (head stride (d + GAP) rows) and the base 1 element into the
    allocation, so it is not 16-byte aligned.  Every row an operand descriptor can name lies inside the allocation."""
    from lidarcrafter_amd import _lib

    B, C, L = x.shape
    d, S = C // heads, L + 3
    n = B * heads * (d + GAP) * S
    flat = torch.full((n + 1 + GAP,), float("nan"), device=dev)
    view = flat[1:1 + n].view(B, heads, d + GAP, S)
    view[:, :, :d, :L] = AO.heads_of(x, heads).to(dev)
    assert view.data_ptr() % 16 != 0
    return _lib.CmOperand(view.data_ptr(), heads * (d + GAP) * S, (d + GAP) * S, S), flat


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("s", [s for s in H.INFERENCE if s.dpos % 8] + [
    Spec(4, 2, 129, 5, 13, 24, 8, 8), Spec(4, 4, 5, 257, 13, 40, 8, 32), Spec(2, 2, 32, 128, 32, 32, 32, 64),
    Spec(16, 8, 33, 33, 45, 24, 8, 8), Spec(2, 2, 257, 33, 1, 64, 0, 33)], ids=str)
def test_poisoned_surroundings(dev, s, prec):
    """Every operand is a view into a larger NaN-filled buffer, `out` a strided view into a marked one: a read past a
    head's channel rows, past L, or of a neighbouring head shows as NaN, a write outside `out` as a changed marker.
    The d_pos = 4 and 12 rows are the fault fixed with this test: the split kernel's 8-row K units overran the
    positional block by 4 rows; such calls now run the fp32 kernels."""
    from lidarcrafter_amd import _lib
    from lidarcrafter_amd import ops as K

    c = H.case(s)
    keep, ops = [], {}
    for n in AO.OPERANDS:
        if c.t.get(n) is None:
            ops[n] = None
        else:
            op, flat = _poisoned(c.t[n], s.heads, dev)
            keep.append(flat)
            ops[n] = ctypes.byref(op)
            keep.append(op)
    So = s.Lq + 5
    n_out = s.B * s.heads * (s.dv + 2) * So
    obuf = torch.full((n_out + 2 * 256,), MARK, device=dev)
    oview = obuf[256:256 + n_out].view(s.B, s.heads, s.dv + 2, So)
    fn = _lib.lib().lc_attention_f16x2_fwd if prec == "f16x2" else _lib.lib().lc_attention_fwd
    _lib.check(fn(ops["q"], ops["q_pos"], ops["k"], ops["k_pos"], ops["v"], ops["k2"], ops["k2_pos"], ops["v2"],
                  oview.data_ptr(), s.heads * (s.dv + 2) * So, (s.dv + 2) * So, So, s.B, s.heads, s.Lq, s.Lk0, s.Lk1,
                  s.dqk, s.dpos, s.dv, float(c.scale), K._stream()), "lc_attention_fwd")
    torch.cuda.synchronize()
    o = oview[:, :, :s.dv, :s.Lq]
    assert bool(torch.isfinite(o).all()), "a NaN from outside the operands reached the output"
    e = rel_l2(o, c.ref64[0])
    print(f"poisoned {tuple(s)} {prec} {H.fwd_route(s, prec == 'f16x2')}: {e:.3e}")
    assert e < ATTN_TOL[prec]
    assert not bool((o == MARK).any())
    outside = torch.ones_like(obuf, dtype=torch.bool)
    outside[256:256 + n_out].view(s.B, s.heads, s.dv + 2, So)[:, :, :s.dv, :s.Lq] = False
    assert bool((obuf[outside] == MARK).all()), "a store landed outside `out`"
    # the same operands as plain contiguous tensors give the same bits: strides and alignment change no arithmetic
    assert torch.equal(o, run_cm(c.dev(dev), s, prec))


# ------------------------------------------------------------------------------------------------ the range window
WINDOW = (4.0, 32768.0)         # of 16 * max|x|: the representable window (csrc/attention_pre.h keeps the constant 16 inside it)
LOW, HIGH = 0.3, 1500.0         # max|x|: 16 * 0.3 = 4.8 and 16 * 1500 = 24000, each within a factor 2 of its end
GROUPS = {"q": ("q", "q_pos"), "k": ("k", "k_pos", "k2", "k2_pos"), "v": ("v", "v2")}


def joint_limit(d):
    """The accurate part of the window: m_q * m_k <= 32 / sqrt(d), d = d_qk + d_pos.  The scaled score (log2 units) is a
    sum of d products of deviation sigma_q * sigma_k; with max|x| about 4.5 sigma at these sizes, the limit is a score
    deviation of 32 / 4.5^2 = 1.6 log2 units, about one nat: the regime of every attention test of the suite (sq * sk = 1
    with scale = d^-1/2 in test_flash_attention_operand_ranges)."""
    return 32.0 / d ** 0.5


# setting -> (claim, targets(J) = max|x| of q, k, v; None: v as drawn).  "accurate": ATTN_TOL, the issue's bound, at every
# end of the accurate window -- q or k at the bottom with the partner ON the joint limit (that is also the highest q / k
# the accurate window reaches, J / 0.3), v at either end with q and k on the limit.  "representable": q or k at the top,
# the partner at the bottom, so everything is inside [4, 32768) but the product is 450, far past J: finite and no
# worse than SHARP_MARGIN x the float32 oracle's own error, which is all the contract claims there.
RANGE_SETTINGS = {
    "q low, k on the joint limit": ("accurate", lambda J: (LOW, J / LOW, None)),
    "k low, q on the joint limit": ("accurate", lambda J: (J / LOW, LOW, None)),
    "v low": ("accurate", lambda J: (J ** 0.5, J ** 0.5, LOW)),
    "v high": ("accurate", lambda J: (J ** 0.5, J ** 0.5, HIGH)),
    "q high, k low": ("representable", lambda J: (HIGH, LOW, None)),
    "k high, q low": ("representable", lambda J: (LOW, HIGH, None)),
}


def _group_amax(t, scale):
    am = {g: max(float(t[n].abs().max()) for n in names if t.get(n) is not None) for g, names in GROUPS.items()}
    am["q"] *= scale * AO.LOG2E
    return am


def _scaled(t, scale, mq, mk, mv):
    """Scale the three operand groups to the target maxima (mv None: v as drawn) -> (operands, factors)."""
    am = _group_amax(t, scale)
    f = {"q": mq / am["q"], "k": mk / am["k"], "v": 1.0 if mv is None else mv / am["v"]}
    out = {n: (None if t.get(n) is None else t[n] * f[g]) for g, names in GROUPS.items() for n in names}
    return out, f


def _assert_window(name, setting, d, got, c, amax):
    claim = RANGE_SETTINGS[setting][0]
    J = joint_limit(d)
    for g in ("q", "k", "v"):
        assert WINDOW[0] <= 16.0 * amax[g] < WINDOW[1], f"{setting}: {g} left the window, 16 * max = {16 * amax[g]:.3g}"
    inside = amax["q"] * amax["k"] <= J * (1 + 1e-4)      # (on the limit up to the rounding of the scaled operands)
    assert inside == (claim == "accurate"), f"{setting}: m_q * m_k = {amax['q'] * amax['k']:.4g} against the joint limit {J:.4g}"
    e, e32 = rel_l2(got, c.ref64[0]), rel_l2(c.ref32[0], c.ref64[0])
    bound = ATTN_TOL["f16x2"] if claim == "accurate" else SHARP_MARGIN * e32
    print(f"window {name} {setting} [{claim}]: 16 * max|x| q {16 * amax['q']:.4g} k {16 * amax['k']:.4g} v {16 * amax['v']:.4g}, "
          f"m_q * m_k {amax['q'] * amax['k']:.4g} (joint limit {J:.4g}): {e:.3e} (float32 oracle {e32:.3e}, bound {bound:.2e})")
    assert bool(torch.isfinite(got).all())
    assert e <= bound


@pytest.mark.parametrize("setting", RANGE_SETTINGS)
@pytest.mark.parametrize("s", [Spec(2, 2, 129, 128, 13, 32, 8, 32), Spec(16, 8, 33, 32, 13, 32, 8, 16)], ids=["4 waves", "8 waves"])
def test_range_window(dev, s, setting):
    """attention_cm (split, 4 and 8 waves) and attention_units at every end of the accurate window (ATTN_TOL) and at the
    top of the representable one."""
    assert H.fwd_route(s, 1, waves_env=-1)[3] == (8 if s.B * s.heads >= 128 else 4)
    d = s.dqk + s.dpos
    t, _ = _scaled(_plain(s, 880), H.scale_of(s), *RANGE_SETTINGS[setting][1](joint_limit(d)))
    c = AO.attention_case(t, s.heads, H.scale_of(s))
    amax = _group_amax(t, H.scale_of(s))
    td = _to({n: a for n, a in t.items() if a is not None}, dev)
    got = run_cm(td, s, "f16x2")
    _assert_window(f"attention_cm {tuple(s)}", setting, d, got, c, amax)
    u = units_of(td, s, dev)
    assert u is not None
    assert torch.equal(run_units(td, s, u), got), "attention_units differs from attention_cm"


@pytest.mark.parametrize("setting", RANGE_SETTINGS)
def test_range_window_qkv_projection(dev, setting, monkeypatch):
    """The same settings on units the qkv projection writes: its q / k / v rows are scaled through the weights."""
    from lidarcrafter_amd import ops as K

    monkeypatch.setattr(K, "PS1X1_MIN_CO", 128)
    d = 64
    base = _qkv_units_run(dev, 1.0, 1.0, 1.0)[4]
    _, f = _scaled(base.t, base.scale, *RANGE_SETTINGS[setting][1](joint_limit(d)))
    got, want, _, _, c = _qkv_units_run(dev, f["q"], f["k"], f["v"])
    assert torch.equal(got, want)
    _assert_window("qkv projection units", setting, d, got, c, c.amax)
