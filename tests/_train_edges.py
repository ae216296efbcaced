"""Case tables, float64 references and bounds of the training-edge tests (tests/test_train_edges.py on the GPU,
tests/test_train_edges_host.py on the CPU): one place, so the two files cannot drift apart.  No GPU code here.

The kernels: csrc/conv_bwd.hip (weight and bias gradient of the ring convolution, exact fp32 and f16x2 split) and the
GroupNorm backward of csrc/norm.hip.  Which branch a row takes is asked of the library (lc_conv2d_ring_wgrad_route,
lc_groupnorm_bwd_route: the functions the launchers and kernels switch on), never restated here.

Weight gradient.  x and dy carry random signs and magnitudes uniform in [0.5, 1.5] (times the row's operand magnitudes), so
no term of any sum is small.  Per element of dW and db:  e = |got - ref64| / S  with S the same contraction of |dy| and |x|
in float64; where S == 0 (taps that see only padding, dy == 0) the result must be exactly 0.
  fp32 kernel   e <= max(4 x the worst e of the float32 reference on the same row, 2^-22)
  split kernel  e <= 8 x 2^-22: three roundings of relative size 2^-22 per product against the TENSOR maxima; maximum
                times maximum over the mean product is 2.25 at magnitudes in [0.5, 1.5]: 6.75, rounded up to 8
A single missing or doubled term moves an element by at least 0.25 / S: the host file asserts that this is at least 16
bounds on every row.

GroupNorm backward.  The rule of tests/_gn_structured.py: per (sample, group) the rel-L2 of dx is at most
max(TOL_GN_BWD, 4 x the float32 oracle's); dgamma, dbeta, dscale, dshift per element |got - ref64| / S_abs with S_abs the
float64 sum of the absolute terms, under the same two-term maximum."""
import collections
import functools

import torch

from lidarcrafter_amd.testing import seeded_randn
from tests import _gn_structured as GS
from tests._profile_cases import TOL_CONV_BWD, TOL_GN_BWD, TOL_RESAMPLE   # noqa: F401  (no new tolerance)

MARGIN = GS.MARGIN
PRODUCT_ERR = 2.0 ** -22            # per-product error the split kernel's contract names (include/lidarcrafter_hip.h)
SPLIT_BOUND = 8.0 * PRODUCT_ERR
SIGNAL_OVER_BOUND = 16.0
EPS = 1e-6
F32, SPLIT = 1, 2                   # out[0] of lc_conv2d_ring_wgrad_route
CAUSE_W, CAUSE_HW, CAUSE_XBS, CAUSE_DYBS, CAUSE_XADDR, CAUSE_DYADDR = 1, 2, 4, 8, 16, 32
LC_EINVAL, LC_EUNSUP = -1, -2
PAD_CH = 3                          # channels of the wider tensor a "slice" row is cut from


# ------------------------------------------------------------------------------------------------ operand layouts
def layout(kind, C, HW):
    """-> (offset, extra batch stride) in floats of a [B, C, H, W] operand inside its buffer (16-byte aligned base):
    contig    a contiguous tensor
    slice_lo  channels [0, C) of a C + 3 channel tensor: a batch stride larger than C H W and nothing else
    slice_hi  channels [3, C + 3) of it: also starts 12 H W bytes into the buffer (a multiple of 16 iff H W % 4 == 0)
    off1      a view starting one float into a buffer
    bs1       a batch stride of C H W + 1: every second sample off 16 bytes"""
    return {"contig": (0, 0), "slice_lo": (0, PAD_CH * HW), "slice_hi": (PAD_CH * HW, PAD_CH * HW), "off1": (1, 0),
            "bs1": (0, 1)}[kind]


def batch_stride(kind, C, HW):
    return C * HW + layout(kind, C, HW)[1]


def addr_mod16(kind, C, HW):
    return 4 * layout(kind, C, HW)[0] % 16


GUARD = 64                          # floats of sentinel on either side (256 bytes: the view's alignment is the layout's)


def place(values, kind, device, fill=float("nan")):
    """`values` [B, C, H, W] (CPU float32) as a view of the given layout inside a `fill`ed buffer on `device`.
    -> (view, buffer).  Everything of the buffer the view does not cover keeps `fill`."""
    B, C, H, W = values.shape
    off, extra = layout(kind, C, H * W)
    bs = C * H * W + extra
    buf = torch.full((2 * GUARD + off + (B - 1) * bs + C * H * W,), fill, dtype=torch.float32, device=device)
    view = buf.as_strided((B, C, H, W), (bs, H * W, W, 1), GUARD + off)
    view.copy_(values)
    return view, buf


def outside(buf, view):
    """The elements of `buf` (from `place`) that `view` does not cover."""
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    mask.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
    return buf[mask]


def guarded(n, device, fill):
    """-> (n-element view, buffer): GUARD words of `fill` on either side, and `fill` inside."""
    buf = torch.full((2 * GUARD + n,), fill, dtype=torch.float32, device=device)
    return buf[GUARD:GUARD + n], buf


# ------------------------------------------------------------------------------------------------ weight gradient
WCase = collections.namedtuple("WCase", "name edge B Ci Co H W xl dyl xmag dymag zero_dy bound_mult")


def W_(name, edge, B, Ci, Co, H, W, xl="contig", dyl="contig", xmag=1.0, dymag=1.0, zero_dy=False, bound_mult=1.0):
    return WCase(name, edge, B, Ci, Co, H, W, xl, dyl, xmag, dymag, zero_dy, bound_mult)


# the exact-fp32 kernel; every row runs at ks = 1 and ks = 3
WGRAD_F32 = [
    W_("w1-h1", "W = 1 < 3: gw %= W wraps more than once; H = 1: the ky = 0, 2 taps see only padding; one tile in all", 1, 1, 1, 1, 1),
    W_("w2", "W = 2 < 3", 3, 5, 1, 2, 2),
    W_("w3", "W = 3: the narrowest ring without a repeated column", 1, 5, 5, 3, 3),
    W_("w16", "W = 16; 63 output channels: a tail on the M side", 3, 5, 63, 2, 16),
    W_("w63-slices", "W = 63, H W % 4 != 0: both operands channel slices whose byte offset is no multiple of 16", 1, 63, 5, 3, 63,
       xl="slice_hi", dyl="slice_hi"),
    W_("w64-h1", "W = 64 on the vector branch: the ring wrap inside one tile; H = 1", 1, 64, 64, 1, 64),
    W_("w64-vec", "the vector branch with three samples: the shape the scalar-cause rows differ from by ONE condition", 3, 64, 64, 2, 64),
    W_("w64-slice-lo", "vector branch, a batch stride larger than C H W on both operands", 3, 5, 65, 2, 64, xl="slice_lo", dyl="slice_lo"),
    W_("w64-slice-hi", "vector branch, channel slices at a byte offset that is a multiple of 16", 3, 65, 5, 2, 64, xl="slice_hi", dyl="slice_hi"),
    W_("cause-w", "scalar branch because of W % 64 alone (W = 96)", 1, 5, 63, 2, 96),
    W_("cause-xbs", "scalar branch because of x_bs % 4 alone", 3, 64, 64, 2, 64, xl="bs1"),
    W_("cause-dybs", "scalar branch because of dy_bs % 4 alone; the bias branch differs by sample", 3, 64, 64, 2, 64, dyl="bs1"),
    W_("cause-xaddr", "scalar branch because of the address of x alone (a view one float into a buffer)", 3, 64, 64, 2, 64, xl="off1"),
    W_("cause-dyaddr", "scalar branch because of the address of dy alone; scalar bias loads", 3, 64, 64, 2, 64, dyl="off1"),
    W_("w65", "W = 65: the second tile of a row holds one column; 65 input channels: a second channel tile of one channel", 3, 65, 64, 2, 65),
    W_("w128", "W = 128: two whole tiles per row on the vector branch; 65 output channels", 1, 64, 65, 3, 128),
    W_("w130", "W = 130: three tiles per row, the last of two columns; H = 1", 3, 5, 5, 1, 130),
    W_("c130", "130 x 130 channels: nine channel tiles, two of them 2 x 2; nsplit = tiles", 1, 130, 130, 2, 64),
    W_("tiles-not-multiple", "60 tiles dealt to 57 splits: three blocks walk two tiles, the rest one", 2, 130, 130, 10, 130),
    W_("dy-small-x-large", "dy at 1e-4, x at 900", 3, 5, 65, 2, 64, xmag=900.0, dymag=1e-4),
    W_("dy-large-x-small", "dy at 900, x at 1e-4", 3, 5, 65, 2, 64, xmag=1e-4, dymag=900.0),
    W_("dy-zero", "dy exactly zero (a zero-initialised output conv on the first step)", 3, 5, 65, 2, 64, zero_dy=True),
    W_("dy-1e-30", "dy at 1e-30", 3, 5, 65, 2, 64, dymag=1e-30),
]

# the f16x2-split kernel (rows the split entry accepts); every row runs at ks = 1 and ks = 3, and against the fp32 kernel
WGRAD_SPLIT = [
    W_("s-w32-one", "W = 32, H = 2, B = 1: one tile in all, nsplit = 2 counts 64-column tiles: one split without work", 1, 5, 63, 2, 32),
    W_("s-w32", "W = 32: half as many tiles as splits, whole splits write zero partials", 3, 64, 65, 4, 32),
    W_("s-w64", "W = 64: as many tiles as splits", 3, 65, 64, 2, 64),
    W_("s-w96", "W = 96, H = 6: three tiles per row pair, 27 tiles for 36 splits", 3, 5, 5, 6, 96),
    W_("s-c130", "130 x 130 channels, 60 tiles dealt to 57 splits: the prefetch of tile + nsplit past the last tile", 3, 130, 130, 10, 128),
    W_("s-slice-lo", "a batch stride larger than C H W on both operands", 3, 63, 5, 4, 64, xl="slice_lo", dyl="slice_lo"),
    W_("s-slice-hi", "channel slices at a byte offset that is a multiple of 16", 3, 5, 63, 2, 96, xl="slice_hi", dyl="slice_hi"),
    W_("s-dy-small-x-large", "dy at 1e-4, x at 900", 3, 5, 65, 2, 64, xmag=900.0, dymag=1e-4),
    W_("s-dy-large-x-small", "dy at 900, x at 1e-4", 3, 5, 65, 2, 64, xmag=1e-4, dymag=900.0),
    W_("s-bound-mult", "range records that are loose upper bounds (range_from_amax with bound_mult = 4/3, dropout's)", 3, 5, 65, 2, 64,
       bound_mult=4.0 / 3.0),
    W_("s-dy-zero", "dy exactly zero", 3, 5, 65, 2, 64, zero_dy=True),
    W_("s-dy-1e-30", "dy at 1e-30", 3, 5, 65, 2, 64, dymag=1e-30),
]

# what the split entry refuses (LC_EUNSUP): ConvRing.backward then takes the fp32 kernel
WGRAD_REFUSED = [
    W_("r-h-odd", "H odd", 3, 5, 5, 3, 64),
    W_("r-w48", "W % 32 != 0", 3, 5, 5, 2, 48),
    W_("r-xbs", "x_bs % 4", 3, 5, 5, 2, 64, xl="bs1"),
    W_("r-dybs", "dy_bs % 4", 3, 5, 5, 2, 64, dyl="bs1"),
    W_("r-xaddr", "x off 16 bytes", 3, 5, 5, 2, 64, xl="off1"),
    W_("r-dyaddr", "dy off 16 bytes", 3, 5, 5, 2, 64, dyl="off1"),
]
KS = (1, 3)


def wgrad_route(c, ks, split):
    """-> (rc, out[8]) of lc_conv2d_ring_wgrad_route for a row (addresses from the row's layouts on an aligned buffer)."""
    import ctypes

    from lidarcrafter_amd import _lib

    out = (ctypes.c_int32 * 8)()
    HW = c.H * c.W
    rc = _lib.lib().lc_conv2d_ring_wgrad_route(int(split), c.B, c.Ci, c.Co, c.H, c.W, ks, batch_stride(c.xl, c.Ci, HW),
                                               batch_stride(c.dyl, c.Co, HW), addr_mod16(c.xl, c.Ci, HW),
                                               addr_mod16(c.dyl, c.Co, HW), out)
    return rc, list(out)


def _signed(shape, seed, mag):
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = torch.rand(*shape, generator=g, dtype=torch.float64) + 0.5
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (m * s * mag).float()


def wgrad_operands(c):
    seed = sum(map(ord, c.name))
    x = _signed((c.B, c.Ci, c.H, c.W), 9100 + seed, c.xmag)
    dy = torch.zeros(c.B, c.Co, c.H, c.W) if c.zero_dy else _signed((c.B, c.Co, c.H, c.W), 9200 + seed, c.dymag)
    return x, dy


def wgrad_direct(x, dy, ks):
    """dW[co, ci, ky, kx] = sum dy * shift(x), db[co] = sum dy, written out without autograd, in the dtype of x."""
    from oracle import denoiser as D

    Co, Ci, h = dy.shape[1], x.shape[1], ks // 2
    dw = torch.empty(Co, Ci, ks, ks, dtype=x.dtype)
    for ky in range(ks):
        for kx in range(ks):
            xs = D._shift_w(D._shift_h(x, ky - h), kx - h)
            dw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy, xs)
    return dw, dy.sum((0, 2, 3))


def wgrad_autograd(x, dy, ks):
    from oracle import denoiser as D

    w = torch.zeros(dy.shape[1], x.shape[1], ks, ks, dtype=x.dtype, requires_grad=True)
    b = torch.zeros(dy.shape[1], dtype=x.dtype, requires_grad=True)
    D.conv_ring(x, w, b).backward(dy)
    return w.grad, b.grad


WRef = collections.namedtuple("WRef", "x dy dw db S_dw S_db e32_dw e32_db bound_f32 signal")


@functools.lru_cache(maxsize=None)
def wgrad_ref(c, ks):
    x, dy = wgrad_operands(c)
    dw, db = wgrad_direct(x.double(), dy.double(), ks)
    S_dw, S_db = wgrad_direct(x.double().abs(), dy.double().abs(), ks)
    dw32, db32 = wgrad_direct(x, dy, ks)
    e_dw, e_db = rel_to_S(dw32, dw, S_dw)[0], rel_to_S(db32, db, S_db)[0]
    bound = max(MARGIN * max(e_dw, e_db), PRODUCT_ERR)
    smax = float(S_dw.max())
    signal = 0.25 * c.xmag * c.dymag / smax if smax > 0 else float("inf")
    return WRef(x, dy, dw, db, S_dw, S_db, e_dw, e_db, bound, signal)


def rel_to_S(got, ref64, S):
    """-> (worst |got - ref64| / S over the elements with S > 0, number of elements with S == 0 that are not exactly 0,
    all finite)."""
    got = got.detach().cpu().double()
    live = S > 0
    e = float(((got - ref64).abs()[live] / S[live]).max()) if bool(live.any()) else 0.0
    return e, int((got[~live] != 0).sum()), bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ GroupNorm backward
GCase = collections.namedtuple("GCase", "name edge B C G H W affine adagn act xl dyl dxl data")


def G_(name, edge, B, C, G, H, W, affine=True, adagn=True, act=True, xl="contig", dyl="contig", dxl="contig", data=None):
    return GCase(name, edge, B, C, G, H, W, affine, adagn, act, xl, dyl, dxl, data)


GN_SHAPES = [
    # (tag, B, C, G, H, W): H W in {1, 3, 250, 4096, 4100, 4104, 8192, 8200}; channels per group in {1, 2, 6, 8, 16}; G = 1
    ("hw1-cpg8-g1", 3, 8, 1, 1, 1),
    ("hw3-cpg2", 1, 4, 2, 1, 3),
    ("hw250-cpg6", 3, 12, 2, 5, 50),
    ("hw4096-cpg1", 1, 4, 4, 32, 128),
    ("hw4100-cpg16", 1, 32, 2, 50, 82),
    ("hw4104-cpg2", 3, 4, 2, 54, 76),
    ("hw8192-cpg8", 1, 8, 1, 64, 128),
    ("hw8200-cpg1", 3, 4, 4, 100, 82),
]
GN_EDGE = {
    "hw1-cpg8-g1": "H W = 1: one pixel per plane; G = 1",
    "hw3-cpg2": "H W = 3",
    "hw250-cpg6": "H W = 250: scalar branch by H W % 4; six channels per group",
    "hw4096-cpg1": "H W = 4096: exactly one slab and one outer step; one channel per group",
    "hw4100-cpg16": "H W = 4100: two slabs of 2050, scalar branch by per % 4; sixteen channels per group",
    "hw4104-cpg2": "H W = 4104: two slabs of 2052 on the vector branch",
    "hw8192-cpg8": "H W = 8192: two whole slabs, two whole outer steps",
    "hw8200-cpg1": "H W = 8200: three slabs of 2734 (the last shorter), three outer steps",
}
GN_CASES = [G_(t, GN_EDGE[t], B, C, G, H, W) for t, B, C, G, H, W in GN_SHAPES] + [
    # the other three combinations of affine / AdaGN, and act off
    G_("affine-only", "gamma / beta without scale / shift", 3, 12, 2, 5, 50, adagn=False),
    G_("adagn-only", "scale / shift without gamma / beta", 3, 12, 2, 5, 50, affine=False),
    G_("plain", "neither", 3, 12, 2, 5, 50, affine=False, adagn=False),
    G_("both-noact", "both, without SiLU", 3, 12, 2, 5, 50, act=False),
    G_("affine-only-noact-vec", "gamma / beta alone, no SiLU, vector branch over two slabs", 3, 4, 2, 54, 76, adagn=False, act=False),
    G_("adagn-only-vec", "scale / shift alone on the vector branch", 1, 8, 1, 64, 128, affine=False),
    # strided and misaligned operands; dx written into a channel slice
    G_("slices", "x, dy channel slices (batch stride > C H W), dx written into a channel slice: vector branch", 3, 4, 2, 54, 76,
       xl="slice_lo", dyl="slice_hi", dxl="slice_hi"),
    G_("slices-odd", "H W = 250: the slices' byte offsets are no multiple of 16", 3, 12, 2, 5, 50, xl="slice_hi", dyl="slice_hi",
       dxl="slice_hi"),
    G_("x-off1", "scalar branch because of the address of x alone", 3, 4, 2, 54, 76, xl="off1"),
    G_("dy-off1", "scalar branch because of the address of dy alone", 3, 4, 2, 54, 76, dyl="off1"),
    G_("dx-off1", "scalar branch because of the address of dx alone", 3, 4, 2, 54, 76, dxl="off1"),
    G_("x-bs1", "x_bs % 4: the branch differs by sample", 3, 4, 2, 54, 76, xl="bs1"),
    G_("dy-bs1", "dy_bs % 4: the branch differs by sample", 3, 4, 2, 54, 76, dyl="bs1"),
    G_("dx-bs1", "dx_bs % 4: the branch differs by sample", 3, 4, 2, 54, 76, dxl="bs1"),
] + [G_(f"{d}-cpg{cpg}", f"channel-structured activations ({d}), {cpg} channels per group", 2, 16, 16 // cpg, 4, 64, data=d)
     for cpg in (2, 8) for d in GS.DATA_NAMES]


def gn_route(c):
    import ctypes

    from lidarcrafter_amd import _lib

    out = (ctypes.c_int32 * 4)()
    HW = c.H * c.W
    rc = _lib.lib().lc_groupnorm_bwd_route(c.B, c.C, c.H, c.W, c.G, batch_stride(c.xl, c.C, HW), batch_stride(c.dyl, c.C, HW),
                                           batch_stride(c.dxl, c.C, HW), addr_mod16(c.xl, c.C, HW), addr_mod16(c.dyl, c.C, HW),
                                           addr_mod16(c.dxl, c.C, HW), out)
    return rc, list(out)


def gn_operands(c):
    """-> (dict of float32 CPU leaves: x, dy, and gamma, beta [C] / scale, shift [B, C] where present; constant group or None)"""
    seed = sum(map(ord, c.name))
    const = None
    if c.data is None:
        x = seeded_randn(c.B, c.C, c.H, c.W, seed=9300 + seed) * 2 + 0.3
    else:
        x, const = GS.tensor_data(c.B, c.C, c.H, c.W, c.G, c.data, seed=seed % 97)
        x = x.float()
    t = dict(x=x, dy=seeded_randn(c.B, c.C, c.H, c.W, seed=9301 + seed))
    if c.affine:
        t.update(gamma=1 + 0.2 * seeded_randn(c.C, seed=9302 + seed), beta=0.3 * seeded_randn(c.C, seed=9303 + seed))
    if c.adagn:
        t.update(scale=0.3 * seeded_randn(c.B, c.C, seed=9304 + seed), shift=0.3 * seeded_randn(c.B, c.C, seed=9305 + seed))
    return t, const


PARAMS = ("gamma", "beta", "scale", "shift")


def gn_autograd(t, G, act, dtype):
    """Autograd of silu?((1 + scale) GroupNorm(x; gamma, beta) + shift) in `dtype` -> {"y", "x": dx, "gamma": dgamma, ...}."""
    from oracle import denoiser as D

    lv = {k: v.to(dtype).clone().requires_grad_() for k, v in t.items() if k != "dy"}
    y = D.group_norm(lv["x"], G, lv.get("gamma"), lv.get("beta"), EPS)
    if "scale" in lv:
        y = y * (1 + lv["scale"][:, :, None, None]) + lv["shift"][:, :, None, None]
    y = D.silu(y) if act else y
    y.backward(t["dy"].to(dtype))
    out = {k: v.grad for k, v in lv.items()}
    out["y"] = y.detach()
    return out


def gn_terms(t, G, act):
    """The float64 terms behind the parameter gradients -> ({name: signed sum}, {name: sum of the absolute terms}):
    dshift = sum_hw dt2, dscale = sum_hw dt2 t1, dbeta = sum_b,hw (1 + sc) dt2, dgamma = sum_b,hw (1 + sc) dt2 xh."""
    x, dy = t["x"].double(), t["dy"].double()
    B, C = x.shape[:2]
    v = x.reshape(B, G, -1)
    xh = ((v - v.mean(-1, keepdim=True)) * (v.var(-1, unbiased=False, keepdim=True) + EPS).rsqrt()).reshape(x.shape)
    one = lambda n, shape: t[n].double().reshape(shape) if n in t else None
    ga, be = one("gamma", (1, C, 1, 1)), one("beta", (1, C, 1, 1))
    sc, sf = one("scale", (B, C, 1, 1)), one("shift", (B, C, 1, 1))
    t1 = xh * (ga if ga is not None else 1.0) + (be if be is not None else 0.0)
    t2 = t1 * (1 + sc if sc is not None else 1.0) + (sf if sf is not None else 0.0)
    if act:
        s = torch.sigmoid(t2)
        dt2 = dy * s * (1 + t2 * (1 - s))
    else:
        dt2 = dy
    w = (1 + sc) if sc is not None else torch.ones(1, 1, 1, 1, dtype=torch.float64)
    terms = {"shift": (dt2, (2, 3)), "scale": (dt2 * t1, (2, 3)), "beta": (w * dt2, (0, 2, 3)), "gamma": (w * dt2 * xh, (0, 2, 3))}
    return ({k: a.sum(d) for k, (a, d) in terms.items() if k in t}, {k: a.abs().sum(d) for k, (a, d) in terms.items() if k in t})


GRef = collections.namedtuple("GRef", "t const ref64 ref32 S bound_dx e32_dx bound_p e32_p")


def gn_group_err(got, ref64, G, const=None):
    """rel-L2 of dx per (sample, group) -> [B, G]; the exactly constant group (if any) is set to 0 (checked as finite)."""
    e = GS.group_err(got, ref64, G)
    if const is not None:
        e = e.clone()
        e[:, const] = 0.0
    return e


def gn_param_err(got, ref64, S, name, c, const=None):
    """|got - ref64| / S_abs per element -> worst over the elements outside the constant group."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    e = (got - ref64).abs() / S.clamp_min(1e-300)
    if const is not None:
        cpg = c.C // c.G
        e = e.clone()
        e[..., const * cpg:(const + 1) * cpg] = 0.0
    return float(e.max())


@functools.lru_cache(maxsize=None)
def gn_ref(c):
    t, const = gn_operands(c)
    ref64 = gn_autograd(t, c.G, c.act, torch.float64)
    ref32 = gn_autograd(t, c.G, c.act, torch.float32)
    _, S = gn_terms(t, c.G, c.act)
    e32_dx = float(gn_group_err(ref32["x"], ref64["x"], c.G, const).max())
    e32_p = {k: gn_param_err(ref32[k], ref64[k], S[k], k, c, const) for k in PARAMS if k in t}
    assert all(v == v and v < float("inf") for v in [e32_dx, *e32_p.values()]), "the float32 oracle is not finite"
    return GRef(t, const, ref64, ref32, S, max(TOL_GN_BWD, MARGIN * e32_dx), e32_dx,
                {k: max(TOL_GN_BWD, MARGIN * v) for k, v in e32_p.items()}, e32_p)


# ------------------------------------------------------------------------------------------------ resampling adjoint
RESAMPLE_SHAPES = [(1, 1, 2, 2), (2, 3, 2, 64), (1, 5, 6, 34), (1, 2, 4, 256)]   # of x; the last: the backward of `up` runs the
                                                                                # vector down kernel (W = 512)
