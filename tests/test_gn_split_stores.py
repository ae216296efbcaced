"""The writers of the pre-split activation planes (gn_apply_split_kernel, split_plain_kernel) map lane = pixel: a thread owns
four pixels 256 apart and one wave store instruction covers 1 KiB contiguous of a plane.  Such a mapping can go wrong where
a 256-pixel group or the block's 1024-pixel pass is ragged, where a slab ends, and where a group lies wholly past the slab's
end (the block skips it) -- the shapes below are the smallest that have each; none of them needs an aligned plane any more.

The expected values are a torch restatement in fp64 (GroupNorm, AdaGN scale / shift, SiLU), compared with hi + lo un-scaled
at 4e-7 relative L2 -- the bound of the pre-split GroupNorm parity test (tests/test_presplit.py; the one in
tests/test_hip_parity.py goes through a convolution at 2e-6, which is wider).  The plain split is exact: bit equality.
Every case also checks a sentinel margin around the planes and the published amax.  `pytest -m gpu`."""
import ctypes as C_

import pytest
import torch

from lidarcrafter_amd.testing import rel_l2, seeded_randn

pytestmark = pytest.mark.gpu

XS = 16.0            # the consumer's x_scale (a power of two, as every range record's)
MARGIN = 64          # sentinel units in front of and behind the planes
SENT = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _planes(B, C, HW, dev):
    """(whole buffer, view of the planes' units): lc_split_act_units 16-byte units with MARGIN sentinel units around."""
    from lidarcrafter_amd._lib import lib

    units = int(lib().lc_split_act_units(B, C, 1, HW))
    assert units == B * 2 * (C // 8) * HW
    buf = torch.full((units + 2 * MARGIN, 8), SENT, device=dev, dtype=torch.float16)
    return buf, buf[MARGIN:MARGIN + units]


def _check_margin(buf):
    assert bool((buf[:MARGIN] == SENT).all()) and bool((buf[-MARGIN:] == SENT).all()), "stores outside the planes"


def _decode(body, B, C, HW):
    """planes [B][2][C/8][HW][8] -> (hi, lo) as fp64 [B, C, HW]"""
    u = body.view(B, 2, C // 8, HW, 8).double()
    return tuple(u[:, i].permute(0, 1, 3, 2).reshape(B, C, HW) for i in (0, 1))


def _range(dev):
    return torch.tensor([XS, 1.0 / XS, 0.0, 0.0], device=dev)


def _entries(x, unit, slots):
    """Producer-statistics entries (pivot, n, sum(v - pivot), sum((v - pivot)^2)) of x [B, C, HW]: per (sample, `unit`
    channels), `slots` entries over ragged pixel ranges -> [B, C / unit, slots, 4] fp32."""
    B, C, HW = x.shape
    xu = x.double().view(B, C // unit, unit, HW)
    cuts = [HW * i // slots for i in range(slots + 1)]
    e = torch.zeros(B, C // unit, slots, 4, dtype=torch.float64, device=x.device)
    for i in range(slots):
        v = xu[..., cuts[i]:cuts[i + 1]]
        piv = v[:, :, 0, 0].float().double()
        d = v - piv[:, :, None, None]
        e[:, :, i, 0] = piv
        e[:, :, i, 1] = unit * (cuts[i + 1] - cuts[i])
        e[:, :, i, 2] = d.sum((2, 3))
        e[:, :, i, 3] = (d * d).sum((2, 3))
    return e.float().contiguous()


def _restate(x, G, gamma, beta, scale, shift, act):
    """fp64: GroupNorm (biased variance, eps 1e-6) (+ affine) (+ (1 + scale) h + shift) (+ SiLU) of x [B, C, HW]"""
    B, C, HW = x.shape
    g = x.double().view(B, G, -1)
    h = ((g - g.mean(2, keepdim=True)) / torch.sqrt(g.var(2, unbiased=False, keepdim=True) + 1e-6)).view(B, C, HW)
    if gamma is not None:
        h = h * gamma.double()[None, :, None] + beta.double()[None, :, None]
    if scale is not None:
        h = h * (1.0 + scale.double()[:, :, None]) + shift.double()[:, :, None]
    return h * torch.sigmoid(h) if act else h


def _input(B, C, HW, wide, dev, seed):
    """x [B, C, HW] contiguous, or channels 8 ... 8 + C of a buffer of C + 24 channels (batch stride > C HW)"""
    if not wide:
        return (seeded_randn(B, C, HW, seed=seed) * 3 + 0.5).to(dev)
    big = (seeded_randn(B, C + 24, HW, seed=seed) * 3 + 0.5).to(dev)
    return big[:, 8:8 + C]


# (C, G, H, W, route, act, adagn, affine, wide); route: "os0" = statistics pass, ("os", [(channels, unit, slots), ...]) =
# producer entries in one or two segments
GN_CASES = [
    # one ragged pass (272 pixels: a full group, 16 pixels of the next, two groups skipped), every statistics route
    (16, 2, 4, 68, ("os", [(16, 8, 3)]), True, True, False, False),          # octet groups
    (32, 8, 4, 68, ("os", [(32, 4, 2)]), False, False, True, False),         # 4 channels per group: one group per wave
    (32, 16, 4, 68, ("os", [(32, 2, 5)]), True, False, False, False),        # 2 channels per group
    (16, 2, 4, 68, "os0", True, False, True, False),                         # no producer statistics
    # 2060 pixels in two slabs of 1030 (no multiple of 4: slabs start off 16-byte alignment); 21 pixels: HW % 4 != 0
    (16, 2, 2, 1030, ("os", [(16, 8, 7)]), True, True, True, False),
    (32, 16, 2, 1030, "os0", False, True, False, False),
    (16, 2, 3, 7, "os0", True, False, False, False),
    # 1024 pixels in two slabs of 512 (few blocks: the launcher halves the slab twice)
    (16, 2, 4, 256, ("os", [(16, 8, 4)]), True, False, True, False),
    (32, 8, 4, 256, "os0", False, True, False, False),
    # two producers, boundary on an octet; entries of different units
    (32, 2, 4, 256, ("os", [(16, 8, 2), (16, 2, 3)]), True, True, False, False),
    # a channel slice of a wider buffer
    (16, 2, 4, 68, ("os", [(16, 8, 3)]), False, True, True, True),
    (16, 2, 4, 256, "os0", True, False, False, True),
    # 4128 pixels in three slabs of 1376 = one full pass of the block + a ragged one
    (16, 2, 8, 516, ("os", [(16, 8, 9)]), True, True, False, False),
    (32, 8, 8, 516, ("os", [(32, 4, 3)]), False, False, True, True),
    (16, 2, 8, 516, "os0", True, False, False, False),
]


@pytest.mark.parametrize("C,G,H,W,route,act,adagn,affine,wide", GN_CASES)
def test_gn_apply_split_planes(dev, C, G, H, W, route, act, adagn, affine, wide):
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd._lib import OctStats, check, lib

    B, HW = 2, H * W
    x = _input(B, C, HW, wide, dev, seed=C + HW)
    x_bs = x.stride(0)
    assert (x_bs > C * HW) == wide
    gamma = (1 + 0.3 * seeded_randn(C, seed=2)).to(dev) if affine else None
    beta = (0.3 * seeded_randn(C, seed=3)).to(dev) if affine else None
    ss = (0.3 * seeded_randn(B, 2 * C, seed=4)).to(dev) if adagn else None       # the two halves of one projection
    scale, shift = (ss[:, :C], ss[:, C:]) if adagn else (None, None)
    ss_bs = 2 * C if adagn else 0
    buf, body = _planes(B, C, HW, dev)
    rng = _range(dev)
    st = K._stream()
    if route == "os0":
        part = torch.empty(int(lib().lc_groupnorm_partials_elems(B, C, H, W, G)), device=dev, dtype=torch.float64)
        check(lib().lc_groupnorm_stats(x.data_ptr(), x_bs, part.data_ptr(), B, C, H, W, G, st), "lc_groupnorm_stats")
        check(lib().lc_groupnorm_apply_split(x.data_ptr(), x_bs, part.data_ptr(), K._p(gamma), K._p(beta), K._p(scale),
                                             K._p(shift), ss_bs, body.data_ptr(), B, C, H, W, G, 1e-6, int(act),
                                             rng.data_ptr(), st), "lc_groupnorm_apply_split")
    else:
        segs, c = [], 0
        for ch, unit, slots in route[1]:
            e = _entries(x[:, c:c + ch], unit, slots)
            segs.append((e, OctStats(e.data_ptr(), ch, slots, unit)))
            c += ch
        assert c == C
        check(lib().lc_groupnorm_apply_os_split(x.data_ptr(), x_bs, C_.byref(segs[0][1]),
                                                C_.byref(segs[1][1]) if len(segs) > 1 else None, K._p(gamma), K._p(beta),
                                                K._p(scale), K._p(shift), ss_bs, body.data_ptr(), B, C, H, W, G, 1e-6,
                                                int(act), rng.data_ptr(), st), "lc_groupnorm_apply_os_split")
    torch.cuda.synchronize()
    ref = _restate(x, G, gamma, beta, scale, shift, act)
    hi, lo = _decode(body, B, C, HW)
    r = rel_l2((hi + lo) / XS, ref)
    print(f"rel-L2 {r:.3e}")
    assert r < 4e-7, r
    # every unit is the split of ONE fp32 value: |lo| is below the last of hi's 11 significant bits
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -10 + 2.0 ** -24).all())
    _check_margin(buf)
    # the published maximum: max |s| of what was stored (to the split's 2^-22), and of the restatement (fp32 against fp64
    # on one element that is several standard deviations out: a few units in the last place of 2^-24)
    rec = rng.cpu()
    assert float(rec[0]) == XS and float(rec[3]) == 0.0
    amax, stored, want = float(rec[2]), float((hi + lo).abs().max()), float(ref.abs().max()) * XS
    print(f"amax {amax!r} stored {stored!r} restated {want!r}")
    assert abs(amax - stored) <= 2.0 ** -22 * stored
    assert abs(amax - want) <= 2e-6 * want


def _split_oracle(s):
    """The split rule of csrc/f16x2.h on s [B, C, HW] (fp32, scale applied) -> the planes' units [B 2 (C/8) HW, 8] fp16."""
    B, C, HW = s.shape
    hi = (s.view(torch.int32) & ~0x1FFF).view(torch.float32)
    lo = (s - hi).half()                 # of the masked fp32 value, not of the packed one
    h16 = hi.clamp(-65504.0, 65504.0).half()   # hi is packed toward zero: saturating (never inf) above fp16's largest, ...
    up = h16.float().abs() > hi.abs()    # ... exact for normal fp16, one step down where it rounded up
    h16 = torch.where(up, (h16.view(torch.int16) - 1).view(torch.float16), h16)
    return torch.stack((h16, lo), 1).view(B, 2, C // 8, 8, HW).permute(0, 1, 2, 4, 3).reshape(-1, 8)


# (C, H, W, wide): lc_split_act_fwd takes planes of a multiple of 4 pixels
PLAIN_CASES = [(16, 4, 68, False), (32, 2, 1030, False), (16, 4, 256, True), (16, 1, 4, False), (32, 8, 516, False),
               (16, 8, 516, True), (16, 40, 256, False)]


@pytest.mark.parametrize("C,H,W,wide", PLAIN_CASES)
def test_split_plain_planes_are_exact(dev, C, H, W, wide):
    """s = x * x_scale; hi = s with the low 13 mantissa bits cleared, as fp16; lo = fp16(s - hi): bit equality.
    (8 x 516: a ragged last 1024-pixel tile behind four full ones; 40 x 256: ten full tiles.)"""
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd._lib import check, lib

    B, HW = 2, H * W
    x = _input(B, C, HW, wide, dev, seed=7 + C + HW)
    buf, body = _planes(B, C, HW, dev)
    rng = _range(dev)
    check(lib().lc_split_act_fwd(x.data_ptr(), x.stride(0), body.data_ptr(), B, C, H, W, rng.data_ptr(), K._stream()),
          "lc_split_act_fwd")
    torch.cuda.synchronize()
    s = x.contiguous() * XS
    want = _split_oracle(s)
    assert torch.equal(body, want)
    _check_margin(buf)
    assert float(rng[2]) == float(s.abs().max())


def _edge_values():
    """64 scaled values s, none NaN or inf, every class of the rule with its negative counterpart."""
    full = 2.0 - 2.0 ** -23              # all 24 significand bits set
    pos = [0.0,
           2.0 ** -30 * (1 + 2.0 ** -20), 1.5 * 2.0 ** -27, full * 2.0 ** -27,            # below 2^-25: hi and lo are zero
           2.0 ** -24, 2.0 ** -20 * (1 + 2.0 ** -10), 1.2345 * 2.0 ** -15, 2.0 ** -17 + 2.0 ** -30,   # hi subnormal in fp16
           2.0 ** -14 - 2.0 ** -30, 2.0 ** -14 * (1 + 2.0 ** -12), 2.0 ** -3 * (1 + 2.0 ** -22),     # lo subnormal / zero
           full * 2.0 ** -10, full * 2.0 ** -3, full, full * 2.0 ** 5, full * 2.0 ** 10, full * 2.0 ** 14, full * 2.0 ** 15,
           65504.0,
           65504.0 + 2.0 ** -8, 65536.0, 65536.0 + 2.0 ** -7, 70000.0, full * 2.0 ** 16,  # above: hi saturates
           1.0, 1.5, 3.0, 2047.0, 1027.0 * 2.0 ** -5,                                     # exact in 11 bits: lo is zero
           0.3, 7.77, 1234.567]
    assert len(pos) == 32
    return torch.tensor(pos + [-v for v in pos], dtype=torch.float64).float()


def test_split_plain_edge_values(dev):
    """The rule at its edges (csrc/f16x2.h): signed zeros, s below 2^-25 (hi and lo zero), hi / lo in fp16's subnormal
    range, full significands, s = +-65504, s above it (hi saturates at +-65504, lo of the masked value), values exact in
    11 bits (lo +-0) -- through both lanes of a pair (channel c starts the list at value c).  Bit equality of both planes
    (signed zeros included), untouched margins, the range record = max |s|."""
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd._lib import check, lib

    B, C, H, W = 1, 16, 1, 64
    sv = _edge_values()
    idx = (torch.arange(W)[None, :] + torch.arange(C)[:, None]) % W
    x = (sv[idx] / XS).view(B, C, W).to(dev)              # a power-of-two scale: x * XS is sv again
    assert bool(torch.isfinite(x).all())
    buf, body = _planes(B, C, W, dev)
    rng = _range(dev)
    check(lib().lc_split_act_fwd(x.data_ptr(), x.stride(0), body.data_ptr(), B, C, H, W, rng.data_ptr(), K._stream()),
          "lc_split_act_fwd")
    torch.cuda.synchronize()
    s = x * XS
    assert torch.equal(s.cpu().view(torch.int32), sv[idx].view(B, C, W).view(torch.int32))
    want = _split_oracle(s)
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) == 65504.0
    got, exp = body.view(torch.int16).cpu(), want.view(torch.int16).cpu()
    bad = (got != exp).nonzero()
    for u, k in bad[:16].tolist():
        print(f"unit {u} elem {k}: got {int(got[u, k]) & 0xFFFF:#06x} want {int(exp[u, k]) & 0xFFFF:#06x}")
    assert torch.equal(got, exp), f"{len(bad)} of {got.numel()} halves differ"
    _check_margin(buf)
    assert float(rng[2]) == float(s.abs().max()) == float(sv.abs().max())
