"""The case table of tests/test_attention_matrix.py, and the proof that it is complete (CPU only).

`lc_attention_route` / `lc_attention_bwd_route` are the host functions the attention launchers themselves switch on
(csrc/attention_route.h), so "which kernel does this case launch" is asked of the library, not restated here:
all 10 inference instantiations, the 4 training-forward ones and the 8 backward launches are hit, each by ragged
queries, by ragged keys and by a channel count below the instantiated width.  Every case's shape keeps every profile of
`check_profiles` (the 64-element rule is met by the shapes, never lowered), the float32 oracle's own error profile is
not degenerate on these inputs, and the oracle agrees with torch's scaled_dot_product_attention.

Lengths come from {1, 5, 31, 32, 33, 127, 128, 129, 257} (second segment {0, 1, 13, 31, 32, 33, 45}), channel counts
from d_qk {8, 20, 24, 32, 40, 64}, d_pos {0, 4, 8, 12, 32}, d_v {1, 8, 31, 32, 33, 40, 64}; d_qk = 33 is added because no
sum of the listed (all even) counts gives the edge d_qk + d_pos = 33."""
import collections
import ctypes
import functools

import pytest
import torch

from lidarcrafter_amd.testing import rel_l2, seeded_randn
from tests import _attention_oracle as AO
from tests import _profile_cases as PC

Spec = collections.namedtuple("Spec", "B heads Lq Lk0 Lk1 dqk dpos dv")

# inference: ops.attention_cm in both precisions
INFERENCE = [
    Spec(2, 2, 33, 31, 0, 8, 0, 31),        # Lk0 < 32: one ragged tile
    Spec(4, 2, 129, 5, 13, 24, 8, 8),       # d_qk + d_pos = 32; both segments inside one ragged tile
    Spec(1, 2, 257, 127, 1, 8, 12, 33),     # d_qk % 8 == 0, d_pos = 12: the split request runs the fp32 kernel (the fixed fault); Lk1 = 1
    Spec(2, 2, 127, 32, 33, 32, 0, 40),     # <32, 2>; a second segment longer than a tile
    Spec(2, 2, 31, 129, 45, 33, 0, 64),     # d_qk = 33: fp32 <64, 2> from both entries
    Spec(4, 4, 5, 257, 13, 40, 8, 32),      # <64, 1>, 48 of 64 channels
    Spec(2, 2, 257, 33, 1, 64, 0, 33),      # <64, 2>, three query blocks
    Spec(2, 2, 32, 128, 32, 32, 32, 64),    # d_qk + d_pos = 64, whole tiles everywhere
    Spec(16, 8, 33, 33, 45, 24, 8, 8),      # 8 waves <32, 1>: 128 heads x 33 queries
    Spec(8, 16, 257, 128, 31, 32, 8, 32),   # 8 waves <64, 1>, two ragged 256-query blocks per head; unit form eligible
    Spec(8, 8, 127, 33, 0, 8, 0, 1),        # d_v = 1
    Spec(8, 8, 1, 129, 13, 64, 0, 64),      # Lq = 1
    Spec(2, 4, 33, 31, 13, 24, 4, 8),       # d_qk % 8 == 0, d_pos = 4 (the fixed fault)
    Spec(2, 4, 31, 33, 32, 20, 12, 8),      # d_qk + d_pos = 32 with neither part in whole units
    Spec(2, 4, 128, 1, 13, 8, 8, 8),        # Lk0 = 1
    Spec(2, 2, 129, 32, 1, 40, 0, 31),      # unit form eligible, 4 waves, Lk1 = 1
]
# training: autograd.FlashAttention (one key segment, no positional part): Lk0 is the key count
TRAINING = [
    Spec(2, 4, 33, 127, 0, 8, 0, 31),       # <32, 1>
    Spec(2, 2, 31, 33, 0, 40, 0, 33),       # <64, 2>, 40 and 33 of 64 channels
    Spec(4, 4, 33, 129, 0, 40, 0, 8),       # <64, 1>
    Spec(2, 2, 129, 5, 0, 24, 0, 64),       # <32, 2>, Lk < 32
    Spec(2, 2, 257, 31, 0, 20, 0, 40),      # d_qk % 8 != 0: fp32 forward through the split entry, split backward with a partial unit
    Spec(2, 2, 128, 257, 0, 64, 0, 64),     # <64, 2> at full width, a whole query block
    Spec(8, 8, 127, 32, 0, 32, 0, 1),       # d_v = 1, one whole key tile
    Spec(8, 8, 1, 128, 0, 64, 0, 64),       # Lq = 1
]
DO_MAGNITUDES = (3e-5, 40.0)               # of test_training.py::test_flash_attention_gradients
O_KEEPS = PC.ATTN_KEEPS                    # query, (sample, head), value channel of o [B, heads, d_v, Lq]
GRAD_KEEPS = ((3,),)                       # dq by query, dk / dv by key


def scale_of(s):
    return (s.dqk + s.dpos) ** -0.5


@functools.lru_cache(maxsize=None)
def case(s, do_mag=None):
    """Seeded operands of a table row (do_mag: with an output gradient of that magnitude) as an oracle Case."""
    mk = lambda c, L, seed: seeded_randn(s.B, s.heads * c, L, seed=seed)
    t = dict(q=mk(s.dqk, s.Lq, 701) * 1.3, k=mk(s.dqk, s.Lk0, 702), v=mk(s.dv, s.Lk0, 703))
    if s.dpos:
        t.update(q_pos=mk(s.dpos, s.Lq, 704), k_pos=mk(s.dpos, s.Lk0, 705))
    if s.Lk1:
        t.update(k2=mk(s.dqk, s.Lk1, 706) * 1.2, v2=mk(s.dv, s.Lk1, 707))
        if s.dpos:
            t["k2_pos"] = mk(s.dpos, s.Lk1, 708)
    if do_mag is not None:
        t["do"] = mk(s.dv, s.Lq, 709) * do_mag
    return AO.attention_case(t, s.heads, scale_of(s))


def decode(code):
    """-> (family, DQK, NDV, waves, PRE) of a packed route code (include/lidarcrafter_hip.h)."""
    assert code > 0, code
    return code >> 16, code >> 8 & 0xFF, code >> 4 & 0xF, 8 if code & 2 else 4, code & 1


F32, SPLIT, BWD_F32, BWD_SPLIT = 1, 2, 3, 4


def fwd_route(s, split, has_amax=0, waves_env=0):
    from lidarcrafter_amd import _lib

    return decode(_lib.lib().lc_attention_route(split, has_amax, s.dqk, s.dpos, s.dv, s.B * s.heads, s.Lq, waves_env))


def bwd_route(s, split):
    from lidarcrafter_amd import _lib

    return decode(_lib.lib().lc_attention_bwd_route(split, s.dqk, s.dv, s.B * s.heads))


def properties(s, route):
    """Which edges a row exercises in the kernel `route`."""
    _, DQK, NDV, _, _ = route
    out = set()
    if s.Lq % 32:
        out.add("ragged queries")
    if (s.Lk0 + s.Lk1) % 32:
        out.add("ragged keys")
    if s.dqk + s.dpos < DQK or s.dv < 32 * NDV:
        out.add("channels below the width")
    return out


ALL = {"ragged queries", "ragged keys", "channels below the width"}
WIDTHS = [(32, 1), (64, 1), (32, 2), (64, 2)]


def _assert_covered(hits, wanted, what):
    for r in wanted:
        assert r in hits, f"{what}: no case launches {r}"
        assert hits[r] == ALL, f"{what}: {r} is never run with {ALL - hits[r]}"


def test_every_inference_route_is_hit_at_its_edges():
    hits = collections.defaultdict(set)
    for s in INFERENCE:
        for split in (0, 1):
            r = fwd_route(s, split)
            hits[r] |= properties(s, r)
    wanted = [(F32, d, n, 4, 0) for d, n in WIDTHS] + [(SPLIT, d, n, 4, 0) for d, n in WIDTHS] + \
             [(SPLIT, 32, 1, 8, 0), (SPLIT, 64, 1, 8, 0)]
    assert len(wanted) == 10
    _assert_covered(hits, wanted, "inference")
    # the 8-wave block is chosen by the grid: ragged Lq at B * heads >= 128, so ceil(Lq / 256) * B * heads >= 128 at tiny L
    for s in INFERENCE:
        r = fwd_route(s, 1)
        if r[3] == 8:
            assert s.B * s.heads >= 128 and s.Lq % 32 and -(-s.Lq // 256) * s.B * s.heads >= 128
            assert fwd_route(s, 1, waves_env=4)[3] == 4 and fwd_route(s, 1, waves_env=8)[3] == 8


def test_every_training_route_is_hit_at_its_edges():
    fwd, bwd = collections.defaultdict(set), collections.defaultdict(set)
    for s in TRAINING:
        assert s.Lk1 == 0 and s.dpos == 0
        r = fwd_route(s, 1, has_amax=1)
        fwd[r] |= properties(s, r)
        r = fwd_route(s, 0)
        fwd[r] |= properties(s, r)
        for split in (0, 1):
            r = bwd_route(s, split)
            bwd[r] |= properties(s, r)
    _assert_covered(fwd, [(SPLIT, d, n, 4, 1) for d, n in WIDTHS], "training forward")
    _assert_covered(bwd, [(f, d, n, 4, 0) for f in (BWD_F32, BWD_SPLIT) for d, n in WIDTHS], "backward")
    # the pairing of d_qk % 8 != 0: fp32 forward through the split entry, split backward
    odd = [s for s in TRAINING if s.dqk % 8]
    assert odd and all(fwd_route(s, 1, has_amax=1)[0] == F32 and bwd_route(s, 1)[0] == BWD_SPLIT for s in odd)


def test_partial_units_leave_the_split_kernel():
    """The split kernel stages K in units of 8 channel rows of ONE operand with no per-channel guard: a positional (or
    content) part that does not fill its last unit must run the fp32 kernels, whichever entry was called."""
    with_dpos = [s for s in INFERENCE if s.dpos % 8]
    assert {s.dpos for s in with_dpos if s.dqk % 8 == 0} == {4, 12}, "the rows that only the d_pos check keeps off the split kernel"
    for s in with_dpos:
        assert fwd_route(s, 1)[0] == F32, f"{s}: d_qk % 8 == 0 does not make a partial positional unit safe"
    for dqk, dpos, want in ((8, 8, SPLIT), (8, 4, F32), (8, 12, F32), (20, 8, F32), (24, 32, SPLIT), (32, 0, SPLIT)):
        assert fwd_route(Spec(2, 2, 64, 64, 0, dqk, dpos, 8), 1)[0] == want, (dqk, dpos)
        assert fwd_route(Spec(2, 2, 64, 64, 0, dqk, dpos, 8), 1, has_amax=1)[0] == want, (dqk, dpos)


def test_named_edges_are_in_the_table():
    inf = INFERENCE
    assert any(s.Lk0 < 32 and s.Lk1 == 0 for s in inf) and any(s.Lk1 and s.Lk0 + s.Lk1 < 32 for s in inf)
    assert {s.Lk1 for s in inf} >= {0, 1, 13, 31, 32, 33, 45}
    assert {s.dqk + s.dpos for s in inf} >= {32, 33, 64}
    assert any(s.Lq == 1 for s in inf) and any(s.dv == 1 for s in inf) and any(s.Lk0 == 1 for s in inf)
    assert any(s.Lq == 1 for s in TRAINING) and any(s.dv == 1 for s in TRAINING)
    # scalar V staging of the split kernels: a whole tile inside segment 0 with an odd channel stride
    assert any(fwd_route(s, 1)[0] == SPLIT and s.Lk0 >= 32 and s.Lk0 % 4 for s in inf)
    assert all(s.Lq <= 300 and s.Lk0 + s.Lk1 <= 300 for s in inf + TRAINING)


def _shapes(s):
    o = (s.B, s.heads, s.dv, s.Lq)
    return {"o": o, "dq": (s.B, s.heads, s.dqk, s.Lq), "dk": (s.B, s.heads, s.dqk, s.Lk0), "dv": (s.B, s.heads, s.dv, s.Lk0)}


@pytest.mark.parametrize("s", INFERENCE + TRAINING, ids=str)
def test_no_profile_is_left_unchecked(s):
    sh = _shapes(s)
    assert PC.usable(sh["o"], O_KEEPS) == O_KEEPS
    if s in TRAINING:
        for n in ("dq", "dk", "dv"):
            assert PC.usable(sh[n], GRAD_KEEPS) == GRAD_KEEPS, n


@pytest.mark.parametrize("s", INFERENCE + TRAINING, ids=str)
def test_oracle_profiles_are_not_vacuous_and_match_sdpa(s):
    tol = PC.existing_lists()["attn_tol"]["f32"]
    train = s in TRAINING
    c = case(s, DO_MAGNITUDES[1] if train else None)
    names = ("o", "lse", "dq", "dk", "dv") if train else ("o", "lse")
    for i, n in enumerate(names):
        if n == "lse":
            continue
        keeps = O_KEEPS if n == "o" else GRAD_KEEPS
        lines, fails = PC.check_profiles(c.ref32[i], c.ref32[i], c.ref64[i], keeps, tol, name=f"{s} {n}")
        assert not any("NOT CHECKED" in ln for ln in lines), lines
        assert not any("change the input" in f for f in fails), fails
    t64 = {k: v.double() for k, v in c.t.items() if k in AO.OPERANDS}
    assert rel_l2(AO.sdpa(t64, s.heads, c.scale), c.ref64[0]) < 1e-13
    # lse is the base-2 log-sum-exp of scale * log2(e) * s
    q, k = AO.heads_of(t64["q"], s.heads), AO.heads_of(t64["k"], s.heads)
    if not s.dpos and not s.Lk1:
        s2 = torch.einsum("bhct,bhcs->bhts", q, k) * (c.scale * AO.LOG2E)
        assert torch.allclose(torch.log2(torch.exp2(s2 - s2.amax(-1, keepdim=True)).sum(-1)) + s2.amax(-1), c.ref64[1], rtol=0, atol=1e-12)


def test_refusals_come_before_any_hip_call():
    """B * heads is the y extent of every attention grid: more than 65535 is LC_EUNSUP in all five entries and in the
    unit-form ones, before anything is launched or dereferenced (dummy non-null pointers, no GPU)."""
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    LC_EINVAL, LC_EUNSUP = -1, -2
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    op = ctypes.byref(_lib.CmOperand(p.value, 0, 0, 64))
    big = (257, 256)                                    # B, heads: 65792
    for fn in (h.lc_attention_fwd, h.lc_attention_f16x2_fwd):
        call = lambda B, heads, dqk=32, dv=32: fn(op, None, op, None, op, None, None, None, p, 0, 0, 64, B, heads, 64, 64, 0,
                                                  dqk, 0, dv, 1.0, None)
        assert call(*big) == LC_EUNSUP
        assert call(1, 1, dqk=72) == LC_EUNSUP and call(1, 1, dv=65) == LC_EUNSUP and call(0, 1) == LC_EINVAL
    for f16x2 in (0, 1):
        train = lambda BH, dqk=32: h.lc_attention_train_fwd(p, p, p, p, p, BH, 64, 64, dqk, 32, 1.0, f16x2, p, None)
        assert train(65536) == LC_EUNSUP and train(1, dqk=72) == LC_EUNSUP and train(0) == LC_EINVAL
    bwd = (p,) * 10
    assert h.lc_attention_bwd(*bwd, 65536, 64, 64, 32, 32, 1.0, None) == LC_EUNSUP
    assert h.lc_attention_bwd_f16x2(*bwd, 65536, 64, 64, 32, 32, 1.0, p, None) == LC_EUNSUP
    assert h.lc_attention_bwd_f16x2(*bwd, 1, 64, 64, 32, 96, 1.0, p, None) == LC_EUNSUP
    assert h.lc_attention_units_fwd(op, None, p, p, 0, 0, 64, *big, 64, 64, 0, 32, 0, 32, 1.0, None) == LC_EUNSUP
    assert h.lc_attention_pack_units(op, p, *big, 64, 64, 0, 32, 0, 0, 0, None) == LC_EUNSUP
    # the route functions refuse the same shapes with the same codes
    assert h.lc_attention_route(1, 0, 32, 0, 32, 0, 64, 0) == LC_EINVAL and h.lc_attention_route(1, 0, 32, 0, 32, 4, 0, 0) == LC_EINVAL
    assert h.lc_attention_route(1, 0, 32, -1, 32, 4, 64, 0) == LC_EINVAL and h.lc_attention_bwd_route(0, 32, 32, 0) == LC_EINVAL
    assert h.lc_attention_route(1, 0, 32, 0, 32, 65536, 64, 0) == LC_EUNSUP
    assert h.lc_attention_route(1, 0, 40, 32, 32, 4, 64, 0) == LC_EUNSUP
    assert h.lc_attention_bwd_route(0, 32, 32, 65536) == LC_EUNSUP and h.lc_attention_bwd_route(1, 65, 32, 4) == LC_EUNSUP
    assert decode(h.lc_attention_route(1, 0, 32, 0, 32, 65535, 64, 0)) == (SPLIT, 32, 1, 8, 0)
