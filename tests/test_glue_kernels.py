"""The once-per-sample kernels, each called directly: range post-processing and condition pre-processing in all three
depth formats (csrc/lidar.hip), the PCNet epilogue, add_scale / copy_into / pstep over mixed batch strides and past the
first trip of their grid-stride loop, the sinusoid embedding (csrc/misc.hip) and the range-image -> point-list kernel
(csrc/temporal.hip).  Every reference is a plain restatement written here: float64 torch on the CPU, or float32 torch /
numpy where every operation is one correctly rounded float32 operation and the kernel must agree bit for bit.

The input builders and the restatements (everything above the first test) touch no GPU; tests/test_glue_kernels_host.py
imports them and checks on the CPU that the float32 restatement of each reference stays inside the bounds used here and
that the edge-exclusion caps hold for the seeds chosen here."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lidarcrafter_amd.testing import seeded_randn

pytestmark = pytest.mark.gpu

MIN_D, MAX_D = 1.45, 80.0
FORMATS = ("log_depth", "inverse_depth", "depth")
IMAGES = ((3, 50), (8, 256))            # H*W = 150: no multiple of the 256-thread block; 2048: eight blocks
EDGE_MIN, EDGE_MAX, EDGE_CAP = 1e-4, 1e-3, 0.005
FILL = -7.5                             # prefilled value of every buffer a kernel writes a slice of


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def worst(got, ref, rtol, atol, keep=None):
    """max |got - ref| / (atol + rtol |ref|): torch.allclose holds iff this is <= 1."""
    r = (got.double() - ref.double()).abs() / (atol + rtol * ref.double().abs())
    if keep is not None:
        r = r[keep.expand_as(r)]
    return float(r.max()) if r.numel() else 0.0


# ---- 1. range post-processing / condition pre-processing ------------------------------------------------------------
def ray_angles(H, W):
    from lidargen.utils.lidar import get_linear_ray_angles

    return get_linear_ray_angles(H, W, 10.0, -30.0).float()


def post_input(fmt, H, W):
    """[2, 2, H, W] normalised (depth, reflectance); a few values lie slightly outside [-1, 1]."""
    seed = 300 + 10 * FORMATS.index(fmt) + IMAGES.index((H, W))
    return (seeded_randn(2, 2, H, W, seed=seed) * 0.6).clamp(-1.001, 1.001)


def post_ref(x, ang, fmt, min_d, max_d, dtype):
    """lidargen/utils/lidar.py of the reference: denormalize :61-64 -> revert_depth :109-128 (get_mask :130-132) ->
    to_xyz :71-82 -> cat[depth, xyz, reflectance].  Returns (out [B,5,H,W], the metric depth before its mask)."""
    x, ang = x.to(dtype), ang.to(dtype)
    dn = (x + 1) / 2
    n = dn[:, [0]]
    if fmt == "log_depth":
        raw = torch.exp2(n * np.log2(max_d + 1)) - 1
    elif fmt == "inverse_depth":
        raw = min_d / n.add(1e-8)
    else:
        raw = n.mul(max_d)
    metric = raw * ((raw > min_d) & (raw < max_d)).to(dtype)
    mask = ((metric > min_d) & (metric < max_d)).to(dtype)
    phi, theta = ang[:, [0]], ang[:, [1]]
    xyz = torch.cat((metric * phi.cos() * theta.cos(), metric * phi.cos() * theta.sin(), metric * phi.sin()), dim=1)
    return torch.cat([metric, xyz * mask, dn[:, [1]]], dim=1), raw


def edge_pixels(metric64, min_d, max_d):
    """Pixels whose float64 metric depth is so close to a strict threshold that float32 may decide the other way."""
    return ((metric64 - min_d).abs() < EDGE_MIN) | ((metric64 - max_d).abs() < EDGE_MAX)


def check_post(got, x, ang, fmt, min_d=MIN_D, max_d=MAX_D, planted=()):
    """`got` [B,5,H,W] against the float64 restatement: depth and reflectance at rtol = atol = 2e-6, xyz at 2e-5, away
    from the mask edges; at most 0.5 % of the pixels may be such edges.  `planted` pixels (b, h, w) are held to exact
    values by the caller: they count neither as compared nor as excluded."""
    ref, raw = post_ref(x, ang, fmt, min_d, max_d, torch.float64)
    exact = torch.zeros_like(raw, dtype=torch.bool)
    for b, h, w in planted:
        exact[b, 0, h, w] = True
    edge = edge_pixels(raw, min_d, max_d) & ~exact
    share = float(edge.double().mean())
    w_dr = worst(got[:, [0, 4]], ref[:, [0, 4]], 2e-6, 2e-6, ~edge & ~exact)
    w_xyz = worst(got[:, 1:4], ref[:, 1:4], 2e-5, 2e-5, ~edge & ~exact)
    print(f"postprocess {fmt} {tuple(x.shape)}: edge share {share:.4f}, depth/refl {w_dr:.3f} of the bound, "
          f"xyz {w_xyz:.3f} of the bound")
    assert share < EDGE_CAP
    assert w_dr <= 1.0 and w_xyz <= 1.0
    return share, w_dr, w_xyz


BOUNDARY = dict(fmt="depth", min_d=2.5, max_d=80.0)
BOUNDARY_PIXELS = {(0, 0, 0): 1.0,                       # d = 1, m = 80.0 exactly: not below the maximum
                   (0, 1, 7): -0.9375,                   # d = 2^-5, m = 2.5 exactly: not above the minimum
                   (1, 2, 49): -0.9375 + 2.0 ** -20}     # m = 2.5 + 5 * 2^-17: kept


def boundary_input(H, W):
    x = post_input("depth", H, W).clone()
    for (b, h, w), v in BOUNDARY_PIXELS.items():
        x[b, 0, h, w] = v
    return x


COND_PLANTED = ((0, 0, 0), (0, 0, 1), (1, 1, 2), (1, 2, 3))   # depth = min_depth, max_depth, 0, 1e-9


def cond_input(fmt, H, W, ncls):
    """[2, 2, H, W] (class id, metric depth): a quarter of the class ids are k + 0.9 (class k, as .long() truncates); the
    depth plane has pixels exactly on both thresholds, at 0 and at 1e-9."""
    g = torch.Generator().manual_seed(400 + 20 * FORMATS.index(fmt) + 2 * IMAGES.index((H, W)) + (ncls > 1))
    cls = torch.randint(0, ncls, (2, H, W), generator=g).float()
    cls = cls + 0.9 * (torch.rand(2, H, W, generator=g) < 0.25).float()
    d = torch.rand(2, H, W, generator=g) * 90
    for p, v in zip(COND_PLANTED, (MIN_D, MAX_D, 0.0, 1e-9)):
        d[p] = v
    return torch.stack([cls, d], dim=1)


def planted_mask(B, H, W):
    m = torch.zeros(B, 1, H, W, dtype=torch.bool)
    for b, h, w in COND_PLANTED:
        m[b, 0, h, w] = True
    return m


def cond_depth_ref(cm, fmt, min_d, max_d, dtype):
    """LiDARUtility.convert_depth, lidargen/utils/lidar.py:84-107 of the reference (mask = get_mask :130-132)."""
    metric = cm[:, [1]].to(dtype)
    mask = ((metric > min_d) & (metric < max_d)).to(dtype)
    if fmt == "log_depth":
        n = torch.log2(metric + 1) / np.log2(max_d + 1)
    elif fmt == "inverse_depth":
        n = min_d / metric.add(1e-8)
    else:
        n = metric.div(max_d)
    return n.clamp(0, 1) * mask


def check_cond_depth(got, cm, fmt):
    """The depth channel against float64 convert_depth at rtol = atol = 2e-6 away from the mask edges.  The four planted
    pixels are held to exact values by the caller, so they count neither as compared nor as excluded: the 0.5 % cap is
    on the remaining edge pixels (two planted threshold pixels alone are 0.67 % of the 2 * 3 * 50 image)."""
    B, _, H, W = cm.shape
    ref = cond_depth_ref(cm, fmt, MIN_D, MAX_D, torch.float64)
    planted = planted_mask(B, H, W)
    edge = edge_pixels(cm[:, [1]].double(), MIN_D, MAX_D) & ~planted
    share = float(edge.double().mean())
    w = worst(got, ref, 2e-6, 2e-6, ~edge & ~planted)
    print(f"condition {fmt} {tuple(cm.shape)}: edge share {share:.4f}, depth {w:.3f} of the bound")
    assert share < EDGE_CAP
    assert w <= 1.0
    assert float(got[planted].abs().max()) == 0.0, "a pixel on a threshold, at 0 or at 1e-9 is outside the strict mask"
    return share, w


# ---- 3. add_scale / copy_into / pstep ----------------------------------------------------------------------------------
# grid_for() caps the grid at 4096 blocks of 256 threads: n = 1048576 + 257 is the smallest n at which thread 0 .. 256 of
# the grid make a second trip of `for (i = ...; i < n; i += gridDim.x * 256)`.
SHAPES = ((2, 1, 1, 1048576 + 257), (3, 2, 3, 5))
PSTEP_COEF = ((0.8, 0.6, 0.9, 0.7, 0.3, 0.4, 0.0, 0.25),     # {a_t, s_t, a_s, s_s, k0, k1, clip, c7}: another row per
              (0.6, 0.8, 0.7, 0.9, 0.5, 0.2, 0.0, 0.5),      # sample; every divisor (a_t, s_t, s_s) is >= 0.6
              (0.95, 0.7, 0.85, 0.6, 0.15, 0.35, 0.0, 0.1))


@functools.lru_cache(maxsize=None)
def operands(shape):
    """(a, b, c): three contiguous float32 CPU tensors of `shape`, shared by the tests of section 3; never written."""
    i = SHAPES.index(shape)
    return tuple(seeded_randn(*shape, seed=500 + 10 * i + k) for k in range(3))


def pstep_coef(B, clip):
    c = torch.tensor(PSTEP_COEF[:B], dtype=torch.float32)
    c[:, 6] = clip
    return c


def pstep_ref(x_t, pred, noise, coef, objective, mode, dtype):
    """The formulas of lc_pstep_fwd in include/lidarcrafter_hip.h, in the order csrc/misc.hip evaluates them."""
    xt = x_t.to(dtype)
    a_t, s_t, a_s, s_s, k0, k1, clip, c7 = (coef.to(dtype)[:, k].reshape(-1, 1, 1, 1) for k in range(8))
    nz = noise.to(dtype) if noise is not None else torch.zeros_like(xt)
    x0 = pstep_x0(x_t, pred, coef, objective, mode, dtype)
    x0 = torch.where(clip > 0, torch.minimum(torch.maximum(x0, -clip), clip), x0)
    if mode == 0:       # continuous ddpm
        return a_s * (xt * (1 - k0) / a_t + k0 * x0) + k1 * nz
    if mode == 1:       # continuous ddim
        return a_s * x0 + k0 * nz + k1 * ((xt - a_t * x0) / s_t)
    if mode == 2:       # discrete ddpm
        return (a_s * x0 + s_s * xt) + k0 * nz
    out = k0 * x0 + k1 * ((xt - a_s * x0) / s_s)                 # discrete ddim
    return out + c7 * nz if noise is not None else out


def pstep_x0(x_t, pred, coef, objective, mode, dtype):
    """The x0 estimate before its clamp: pred (x_0 objective); A x_t - Bc pred (v objective, and eps in the discrete
    modes 2 / 3); (x_t - sigma_t pred) / alpha_t (eps objective of the continuous modes 0 / 1)."""
    xt, pr = x_t.to(dtype), pred.to(dtype)
    a_t, s_t = (coef.to(dtype)[:, k].reshape(-1, 1, 1, 1) for k in range(2))
    if objective == 2:
        return pr
    if objective == 1 or mode >= 2:
        return a_t * xt - s_t * pr
    return (xt - s_t * pr) / a_t


def clipped_share(x_t, pred, coef, objective, mode):
    """Share of elements whose x0 estimate exceeds the clip range of 1 (so that the clamp really acts)."""
    return float((pstep_x0(x_t, pred, coef, objective, mode, torch.float64).abs() > 1).double().mean())


# ---- 4. sinusoid -------------------------------------------------------------------------------------------------------
SINUSOID_T = (-15.0, -3.25, 0.0, 7.5, 15.0, 0.37, 11.1)


def sinusoid_ref(t, channels, max_period):
    """SinusoidalPositionalEmbedding.forward, lidargen/models/unets/ops.py:20-26 of the reference, on the float32 argument:
    h and t * h in float32 as the kernel forms them, sin and cos in float64."""
    half = channels // 2
    c = -torch.log(torch.tensor(max_period, dtype=torch.float32)) / torch.tensor(half - 1, dtype=torch.float32)
    h = torch.exp(c * torch.arange(half, dtype=torch.float32))
    a = (t.float()[:, None] * h[None, :]).double()
    return torch.cat([a.sin(), a.cos()], dim=-1)


# ---- 5. image_to_points ------------------------------------------------------------------------------------------------
def points_frame(H, W):
    """frame [2, 5, H, W] (the xyz planes are frame[b, 1:4]), refl [H, W] in [0, 1), cond [H, W] with zeros, positives,
    negatives and -0.0.  Planted in sample 1: all-zero pixels, pixels of norm exactly 5 and just above, pixels on and
    just inside the ego square of radius 2."""
    g = torch.Generator().manual_seed(700 + IMAGES.index((H, W)))
    frame = torch.randn(2, 5, H, W, generator=g) * 10
    refl = torch.rand(H, W, generator=g)
    cond = torch.randint(-1, 2, (H, W), generator=g).float() * torch.rand(H, W, generator=g).clamp_min(0.125)
    cond[0, 5] = -0.0
    xyz = frame[1, 1:4]
    planted = {(0, 0): (0.0, 0.0, 0.0), (2, W - 1): (0.0, 0.0, 0.0),
               (0, 1): (3.0, 4.0, 0.0), (1, 3): (0.0, -3.0, 4.0),        # |p| = 5 exactly in float32
               (0, 2): (3.0, 4.0, 0.25),                                  # |p|^2 = 25.0625
               (1, 0): (2.0, 0.5, 7.0), (1, 1): (0.5, -2.0, 7.0), (1, 2): (-2.0, -2.0, 7.0),      # on the square: kept
               (2, 0): (1.9999999, -1.5, 7.0), (2, 1): (-1.0, 1.9999999, 7.0)}                    # inside: dropped
    for (h, w), p in planted.items():
        xyz[:, h, w] = torch.tensor(p)
        cond[h, w] = 0.0
    return frame, refl, cond


def image_to_points_ref(xyz, refl, cond, refl_scale, min_norm, ego_radius):
    """lc_image_to_points of include/lidarcrafter_hip.h in numpy float32: rows (x, y, z, refl * refl_scale) times the
    background mask !(cond > 0); keep = 0 for |xyz| <= min_norm (min_norm >= 0) and for |x| < ego_radius and
    |y| < ego_radius (ego_radius > 0)."""
    f = np.float32
    x, y, z = (xyz[k].numpy().astype(f).reshape(-1) for k in range(3))
    m = np.ones_like(x) if cond is None else np.where(cond.numpy().reshape(-1) > 0, f(0), f(1)).astype(f)
    r = np.zeros_like(x) if refl is None else (refl.numpy().astype(f).reshape(-1) * f(refl_scale)) * m
    rows = np.stack([x * m, y * m, z * m, r], axis=1).astype(f)
    keep = np.ones(x.shape, dtype=bool)
    if min_norm >= 0:
        keep &= np.sqrt((rows[:, 0] * rows[:, 0] + rows[:, 1] * rows[:, 1]) + rows[:, 2] * rows[:, 2]) > f(min_norm)
    if ego_radius > 0:
        keep &= ~((np.abs(rows[:, 0]) < f(ego_radius)) & (np.abs(rows[:, 1]) < f(ego_radius)))
    return rows, keep.astype(np.int32)


# =====================================================================================================================
# 1. postprocess_kernel / condition_kernel
# =====================================================================================================================
@pytest.mark.parametrize("H,W", IMAGES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_range_postprocess_formats(dev, fmt, H, W):
    """Every depth format of revert(), contiguous and as the channel slice wide[:, 3:5] (sample_bs = 7 H W), through
    LiDARUtility.postprocess and ops.range_postprocess, against the float64 restatement."""
    from lidarcrafter_amd import ops as K
    from lidargen.utils.lidar import LiDARUtility

    ang = ray_angles(H, W)
    lu = LiDARUtility((H, W), fmt, MIN_D, MAX_D, ray_angles=ang).to(dev)
    x = post_input(fmt, H, W)
    y = lu.postprocess(x.to(dev))
    wide = torch.full((2, 7, H, W), FILL, device=dev)
    wide[:, 3:5] = x.to(dev)
    y_slice = lu.postprocess(wide[:, 3:5])
    assert y.shape == (2, 5, H, W)
    assert torch.equal(y, y_slice)
    assert torch.equal(y, K.range_postprocess(wide[:, 3:5], ang.to(dev), fmt, MIN_D, MAX_D))
    check_post(y.cpu(), x, ang, fmt)


@pytest.mark.parametrize("H,W", IMAGES)
def test_range_postprocess_exact_boundaries(dev, H, W):
    """depth format, min_depth 2.5, max_depth 80: a metric depth exactly on either threshold is dropped (strict
    inequalities, lidar.py:130-132), one float32 step above the minimum is kept; (x + 1) / 2 * 80 and the mask are single
    correctly rounded float32 operations, so depth and reflectance equal the float32 CPU restatement bit for bit."""
    from lidarcrafter_amd import ops as K

    ang = ray_angles(H, W)
    x = boundary_input(H, W)
    y = K.range_postprocess(x.to(dev), ang.to(dev), BOUNDARY["fmt"], BOUNDARY["min_d"], BOUNDARY["max_d"]).cpu()
    assert float(y[0, :4, 0, 0].abs().max()) == 0.0, "m == max_depth is not below the maximum"
    assert float(y[0, :4, 1, 7].abs().max()) == 0.0, "m == min_depth is not above the minimum"
    assert float(y[1, 0, 2, 49]) == 2.5 + 5 * 2.0 ** -17
    assert float(y[1, 1:4, 2, 49].abs().max()) > 0.0
    ref32, _ = post_ref(x, ang, BOUNDARY["fmt"], BOUNDARY["min_d"], BOUNDARY["max_d"], torch.float32)
    assert torch.equal(y[:, [0, 4]], ref32[:, [0, 4]])
    check_post(y, x, ang, BOUNDARY["fmt"], BOUNDARY["min_d"], BOUNDARY["max_d"], planted=BOUNDARY_PIXELS)


@pytest.mark.parametrize("ncls", [1, 9])
@pytest.mark.parametrize("H,W", IMAGES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_condition_preprocess_formats(dev, fmt, H, W, ncls):
    """one_hot(class.long()) ++ convert_depth in every depth format; the input also as the slice wide[:, 2:4] and the
    output as a slice of a wider buffer whose other channels must keep their value."""
    from lidarcrafter_amd import ops as K
    from lidargen.utils.lidar import LiDARUtility

    lu = LiDARUtility((H, W), fmt, MIN_D, MAX_D, ray_angles=ray_angles(H, W)).to(dev)
    cm = cond_input(fmt, H, W, ncls)
    z = lu.preprocess_condition_mask(cm.to(dev), ncls)
    assert z.shape == (2, ncls + 1, H, W)
    wide = torch.full((2, 6, H, W), FILL, device=dev)
    wide[:, 2:4] = cm.to(dev)
    assert torch.equal(z, lu.preprocess_condition_mask(wide[:, 2:4], ncls))
    buf = torch.full((2, ncls + 3, H, W), FILL, device=dev)
    K.condition_preprocess(wide[:, 2:4], ncls, fmt, MIN_D, MAX_D, out=buf[:, 1:ncls + 2])
    assert torch.equal(buf[:, 1:ncls + 2], z)
    assert bool((buf[:, :1] == FILL).all()) and bool((buf[:, ncls + 2:] == FILL).all())
    z = z.cpu()
    assert (cm[:, 0] != cm[:, 0].floor()).any(), "the class plane holds fractional ids"
    assert torch.equal(z[:, :ncls], F.one_hot(cm[:, 0].long(), ncls).permute(0, 3, 1, 2).float())
    check_cond_depth(z[:, ncls:], cm, fmt)
    if fmt == "depth":      # d / max_depth, clamp and mask: single correctly rounded float32 operations
        assert torch.equal(z[:, ncls:], cond_depth_ref(cm, fmt, MIN_D, MAX_D, torch.float32))


def test_condition_class_outside_range_is_all_zero(dev):
    """A class id outside [0, num_classes) is an input F.one_hot rejects; the kernel writes an all-zero one-hot for it
    (stated at lc_condition_preprocess in the header)."""
    from lidarcrafter_amd import ops as K

    H, W, ncls = 3, 50, 9
    cm = cond_input("log_depth", H, W, ncls).clone()
    cm[0, 0, 1, 1], cm[1, 0, 2, 2], cm[1, 0, 0, 7] = float(ncls), -1.0, 1e6
    z = K.condition_preprocess(cm.to(dev), ncls, "log_depth", MIN_D, MAX_D).cpu()
    for b, h, w in ((0, 1, 1), (1, 2, 2), (1, 0, 7)):
        assert float(z[b, :ncls, h, w].abs().max()) == 0.0
    ok = (cm[:, 0] >= 0) & (cm[:, 0] < ncls)
    ref = F.one_hot(cm[:, 0].long().clamp(0, ncls - 1), ncls).permute(0, 3, 1, 2).float() * ok[:, None]
    assert torch.equal(z[:, :ncls], ref)


# =====================================================================================================================
# 2. gate_bias_kernel
# =====================================================================================================================
def _gate_bias_case(N):
    B, C = 2, 5
    x = seeded_randn(B, C, N, seed=600 + N)
    res = seeded_randn(B, C, N, seed=650 + N)
    proj = seeded_randn(B, 2 * C + 7, seed=601) * 2
    proj[0, 3 + 1], proj[1, 3 + 2] = 100.0, -100.0               # saturating gate logits: gate 1 and gate 0
    return x, res, proj


@pytest.mark.parametrize("with_res", [False, True], ids=["no_res", "res"])
@pytest.mark.parametrize("leaky", [False, True], ids=["linear", "leaky"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_gate_bias_act(dev, N, leaky, with_res):
    """PCNet.forward, point_unet.py:21-25 of the reference (+ the leaky_relu / residual of its callers), with gate and
    bias as offset slices of one [B, 2C + 7] projection (row stride 17, not C), against float64 at 2e-6 of the largest
    reference magnitude."""
    from lidarcrafter_amd import ops as K

    B, C = 2, 5
    x, res, proj = _gate_bias_case(N)
    gate, bias = proj[:, 3:3 + C], proj[:, 3 + C:3 + 2 * C]
    v = x.double() * torch.sigmoid(gate.double())[:, :, None] + bias.double()[:, :, None]
    if leaky:
        v = F.leaky_relu(v, 0.01)
    ref = v + res.double() if with_res else v
    pd = proj.to(dev)
    gd, bd = pd[:, 3:3 + C], pd[:, 3 + C:3 + 2 * C]
    assert gd.stride(0) == 2 * C + 7 and gd.storage_offset() == 3
    xd, rd = x.to(dev), (res.to(dev) if with_res else None)
    y = K.gate_bias_act(xd, gd, bd, leaky, res=rd)
    err = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"gate_bias_act N={N} leaky={leaky} res={with_res}: {err:.2e} of the largest magnitude")
    assert err <= 2e-6
    # gate 1: the row is act(x + bias); gate 0: the row is act(bias), whatever x holds
    act = (lambda t: F.leaky_relu(t, 0.01)) if leaky else (lambda t: t)
    one = act(x[0, 1].double() + float(bias[0, 1]))
    zero = act(bias[1, 2].double()).expand(N)
    if with_res:
        one, zero = one + res[0, 1].double(), zero + res[1, 2].double()
    scale = float(ref.abs().max())
    assert float((y[0, 1].cpu().double() - one).abs().max()) <= 2e-6 * scale
    assert float((y[1, 2].cpu().double() - zero).abs().max()) <= 2e-6 * scale
    if not with_res:
        assert bool((y[1, 2] == y[1, 2, 0]).all()), "gate 0 leaves nothing of x in the row"
    # in place
    x_in = xd.clone()
    assert K.gate_bias_act(x_in, gd, bd, leaky, res=rd, out=x_in) is x_in
    assert torch.equal(x_in, y)


def test_gate_bias_act_refusals(dev):
    from lidarcrafter_amd import ops as K

    B, C, N = 2, 5, 16
    x, res, proj = _gate_bias_case(N)
    xd, pd = x.to(dev), proj.to(dev)
    gd, bd = pd[:, 3:3 + C], pd[:, 3 + C:3 + 2 * C]
    K.gate_bias_act(xd, gd, bd, False, res=res.to(dev))
    with pytest.raises(ValueError):
        K.gate_bias_act(torch.zeros(B, C, 2 * N, device=dev)[:, :, ::2], gd, bd, False)
    with pytest.raises(ValueError):
        K.gate_bias_act(xd, gd, bd.contiguous(), False)                      # row strides 17 and 5
    with pytest.raises(ValueError):
        K.gate_bias_act(xd, gd, bd, False, res=torch.zeros(B, C, N + 1, device=dev))


# =====================================================================================================================
# 3. add_scale_kernel / copy_kernel / pstep_kernel
# =====================================================================================================================
class _StrideMix:
    """Device operands of one shape with three different batch strides: `a` contiguous (C H W), `b` the channel slice
    [:, 1:] of a [B, C + 1, H, W] tensor, `out` the slice [:, 1:1 + C] of a [B, C + 2, H, W] buffer prefilled with FILL."""

    def __init__(self, shape, dev):
        B, C, H, W = shape
        a, b, c = operands(shape)
        self.C = C
        self.a, self.c = a.to(dev), c.to(dev)
        self.b_wide = torch.full((B, C + 1, H, W), FILL, device=dev)
        self.b_wide[:, 1:] = b.to(dev)
        self.b = self.b_wide[:, 1:]
        self.out_wide = torch.empty((B, C + 2, H, W), device=dev)
        assert len({self.a.stride(0), self.b.stride(0), self.out_wide.stride(0)}) == 3

    def out(self):
        self.out_wide.fill_(FILL)
        return self.out_wide[:, 1:1 + self.C]

    def neighbours_untouched(self):
        return bool((self.out_wide[:, :1] == FILL).all()) and bool((self.out_wide[:, 1 + self.C:] == FILL).all())


@pytest.fixture(scope="module")
def mix(dev):
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = _StrideMix(shape, dev)
        return cache[shape]

    yield get
    cache.clear()


@pytest.mark.parametrize("scale", [0.5, 1.0, -3.25])
@pytest.mark.parametrize("shape", SHAPES, ids=["second_trip", "small"])
def test_add_scale_strides(dev, mix, shape, scale):
    """(a + b) * scale, efficient_unet.py:55-57 of the reference: two single float32 operations (contraction is off in
    misc.hip), so bit-equal to float32 CPU torch.  In place (out = a) every element must be read and written exactly
    once, also by the threads that make a second trip of the grid-stride loop."""
    from lidarcrafter_amd import ops as K

    m = mix(shape)
    a, b, _ = operands(shape)
    ref = (a + b) * scale
    out = m.out()
    assert K.add_scale(m.a, m.b, scale, out=out) is out
    assert torch.equal(out.cpu(), ref)
    assert m.neighbours_untouched()
    assert torch.equal(K.add_scale(m.a, m.b, scale).cpu(), ref)
    a_in = m.a.clone()
    K.add_scale(a_in, m.b, scale, out=a_in)
    assert torch.equal(a_in.cpu(), ref)


@pytest.mark.parametrize("shape", SHAPES, ids=["second_trip", "small"])
def test_copy_into_strides(dev, mix, shape):
    """lc_copy_strided: slice to slice with different batch strides, and a batch-stride-0 source (the `enc.expand(B, ...)`
    the UNets copy into their concat buffer)."""
    from lidarcrafter_amd import ops as K

    m = mix(shape)
    _, b, _ = operands(shape)
    out = m.out()
    assert K.copy_into(out, m.b) is out
    assert torch.equal(out.cpu(), b)
    assert m.neighbours_untouched()
    out = m.out()
    K.copy_into(out, m.b[:1].expand(shape[0], -1, -1, -1))
    assert torch.equal(out.cpu(), b[:1].expand_as(b))
    assert m.neighbours_untouched()
    with pytest.raises(ValueError):
        K.copy_into(out, m.b[:, :, :, 1:])


def check_pstep(got, x_t, pred, noise, coef, objective, mode):
    ref = pstep_ref(x_t, pred, noise, coef, objective, mode, torch.float64)
    w = worst(got, ref, 2e-6, 2e-6)
    assert w <= 1.0, (objective, mode, noise is not None, float(coef[0, 6]), w)
    return w


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("objective", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["second_trip", "small"])
def test_pstep_single_steps(dev, mix, shape, objective, mode):
    """One lc_pstep_fwd launch per (objective, mode, noise given / NULL, clip 0 / 1) with per-sample coefficient rows,
    x_t and out as channel slices of different batch strides, against the float64 restatement at rtol = atol = 2e-6
    (the bound of test_pstep_golden); in place (out = x_t, as the sampler runs it) the result must be the same."""
    from lidarcrafter_amd import ops as K

    m = mix(shape)
    pred_c, x_c, noise_c = operands(shape)                      # pred = a (contiguous), x_t = b (slice), noise = c
    worst_w = 0.0
    for clip in (0.0, 1.0):
        coef = pstep_coef(shape[0], clip)
        if clip:
            assert clipped_share(x_c, pred_c, coef, objective, mode) > 0.05, "the inputs exceed the clip range"
        for noise, noise_d in ((noise_c, m.c), (None, None)):
            out = m.out()
            assert K.pstep(m.b, m.a, noise_d, coef.to(dev), objective, mode, out=out) is out
            worst_w = max(worst_w, check_pstep(out.cpu(), x_c, pred_c, noise, coef, objective, mode))
            assert m.neighbours_untouched()
            x_in = m.b_wide.clone()[:, 1:]
            K.pstep(x_in, m.a, noise_d, coef.to(dev), objective, mode, out=x_in)
            assert torch.equal(x_in, out)
    print(f"pstep {shape} objective {objective} mode {mode}: {worst_w:.3f} of the bound")


def test_pstep_refusals(dev):
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd._lib import HipError

    x = torch.zeros(3, 2, 3, 5, device=dev)
    coef = pstep_coef(3, 0.0).to(dev)
    with pytest.raises(ValueError):
        K.pstep(x, x, None, coef[:2], 0, 0)
    with pytest.raises(HipError):
        K.pstep(x, x, None, coef, 3, 0)
    with pytest.raises(HipError):
        K.pstep(x, x, None, coef, 0, 4)


# =====================================================================================================================
# 4. sinusoid_kernel
# =====================================================================================================================
@pytest.mark.parametrize("max_period", [10000.0, 100.0])
@pytest.mark.parametrize("M,channels", [(1, 4), (5, 64), (3, 258), (7, 512)])
def test_sinusoid(dev, M, channels, max_period):
    """channels = 4 is the smallest legal value (half - 1 = 1); M * half = 387 is no multiple of the 256-thread block;
    atol = 2e-6 as test_linear_sinusoid."""
    from lidarcrafter_amd import ops as K

    t = torch.tensor(SINUSOID_T[:M])
    y = K.sinusoid(t.to(dev), channels, max_period)
    assert y.shape == (M, channels)
    ref = sinusoid_ref(t, channels, max_period)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"sinusoid M={M} channels={channels} max_period={max_period}: max abs error {err:.2e}")
    assert err <= 2e-6


@pytest.mark.parametrize("channels", [2, 7])
def test_sinusoid_refuses_channels(dev, channels):
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd._lib import HipError

    with pytest.raises(HipError):
        K.sinusoid(torch.zeros(3, device=dev), channels)


# =====================================================================================================================
# 5. image_points_kernel
# =====================================================================================================================
I2P_CASES = {
    "all_off": dict(use_cond=False, refl_scale=1.0, min_norm=-1.0, ego_radius=0.0),
    "cond": dict(use_cond=True, refl_scale=1.0, min_norm=-1.0, ego_radius=0.0),
    "min_norm_0": dict(use_cond=False, refl_scale=1.0, min_norm=0.0, ego_radius=0.0),
    "min_norm_5": dict(use_cond=False, refl_scale=1.0, min_norm=5.0, ego_radius=0.0),
    "ego_2": dict(use_cond=False, refl_scale=1.0, min_norm=-1.0, ego_radius=2.0),
    "refl_255": dict(use_cond=False, refl_scale=255.0, min_norm=-1.0, ego_radius=0.0),
    "all_on": dict(use_cond=True, refl_scale=255.0, min_norm=0.0, ego_radius=2.0),
}


@pytest.mark.parametrize("refl_dims", [2, 3])
@pytest.mark.parametrize("case", list(I2P_CASES))
@pytest.mark.parametrize("H,W", IMAGES)
def test_image_to_points(dev, H, W, case, refl_dims):
    """ops.image_to_points on xyz = frame[1, 1:4] (an offset slice, plane stride H W) against the numpy float32
    restatement, rows and keep flags bit for bit, then compact_points against numpy boolean indexing.  Every row entry is
    one float32 product.  The norm of the min_norm rule is a float32 sum of squares and a square root, contraction off;
    should it still differ from numpy's by an ulp, the pixels that decide `min_norm_5` are planted at exactly
    representable norms ((3, 4, 0) and (0, -3, 4): 5, dropped; (3, 4, 0.25): kept) and no random pixel (|p| ~ 17, 150 to
    2048 of them) lies within an ulp of 5."""
    from lidarcrafter_amd import ops as K

    c = I2P_CASES[case]
    frame, refl, cond = points_frame(H, W)
    cond = cond if c["use_cond"] else None
    fd = frame.to(dev)
    xyz = fd[1, 1:4]
    assert xyz.storage_offset() == 6 * H * W and xyz.stride(0) == H * W
    rd = refl.to(dev) if refl_dims == 2 else refl.to(dev)[None]
    pts, keep = K.image_to_points(xyz, rd, None if cond is None else cond.to(dev), refl_scale=c["refl_scale"],
                                  min_norm=c["min_norm"], ego_radius=c["ego_radius"])
    rows, flags = image_to_points_ref(frame[1, 1:4], refl, cond, c["refl_scale"], c["min_norm"], c["ego_radius"])
    assert pts.shape == (H * W, 4) and keep.shape == (H * W,) and keep.dtype == torch.int32
    assert np.array_equal(pts.cpu().numpy(), rows)
    assert np.array_equal(keep.cpu().numpy(), flags)
    at = lambda h, w: int(flags[h * W + w])                      # noqa: E731
    if case == "all_off":
        assert flags.all()
    if c["use_cond"]:
        neg = (cond.reshape(-1) < 0).numpy()
        assert neg.any() and np.array_equal(rows[neg], image_to_points_ref(
            frame[1, 1:4], refl, None, c["refl_scale"], -1.0, 0.0)[0][neg]), "cond < 0 removes nothing"
        assert not rows[(cond.reshape(-1) > 0).numpy()].any()
    if c["min_norm"] >= 0:
        assert at(0, 0) == 0 and at(2, W - 1) == 0
    if c["min_norm"] == 5.0:
        assert (at(0, 1), at(1, 3), at(0, 2)) == (0, 0, 1)
    if c["ego_radius"] > 0:
        assert (at(1, 0), at(1, 1), at(1, 2), at(2, 0), at(2, 1)) == (1, 1, 1, 0, 0)
    assert 0 < flags.sum() <= H * W
    assert np.array_equal(K.compact_points(pts, keep).cpu().numpy(), rows[flags != 0])


def test_image_to_points_refusals(dev):
    from lidarcrafter_amd import ops as K

    H, W = 3, 50
    frame, refl, _ = points_frame(H, W)
    fd = frame.to(dev)
    pts, keep = K.image_to_points(fd[1, 1:4])                    # no reflectance: the fourth column is 0
    assert float(pts[:, 3].abs().max()) == 0.0 and bool(keep.all())
    with pytest.raises(ValueError):
        K.image_to_points(fd[1, 1:4, :, ::2])
    with pytest.raises(ValueError):
        K.image_to_points(fd[1, 0:4])
    with pytest.raises(ValueError):
        K.image_to_points(fd[1, 1:4], refl.to(dev).t().contiguous().t())
