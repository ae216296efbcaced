"""The product's RoI-aware pooling, chamfer and first-hit points-in-boxes kernels against the
REFERENCE's own CUDA kernels, hipified and compiled for gfx950 by oracle/build_ref_gpu.py, on the
same inputs.  Two reference builds: `off` (-ffp-contract=off, the arithmetic our kernels promise)
and `fc` (hipcc's default contraction, the closest match to nvcc's default --fmad=true).

Decision thresholds (box faces, the z slab, voxel-index fractions) are evaluated in float64 on the
float32 inputs.  A (point, box) pair is adversarial when one of them lies within
tau = 8 * 2^-24 * (|sx| + |sy| + d) of the point (d the box extent of that axis, |sz| + dz for z);
there the float `cos` overload of the reference, and contraction, may decide differently.  Every
other pair must agree bit for bit.  The reference launchers run on the null stream: every call is
synchronised on both sides.  Each case prints its count of tau-bounded disagreements."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 2.0 ** -24
MARGIN = float(F32(1e-5))
BUILDS = ["off", "fc"]
HEADINGS = [0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 7.5, -20.0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref():
    """{"off"|"fc": {"roi": module, "chamfer": module}}; skips only while nothing was built."""
    from oracle import build_ref_gpu as R

    if R.stamp() is None:
        pytest.skip("reference GPU kernels not built: oracle/_ref/gpu_ref_stamp.json is absent "
                    "(build() makes it where the reference sources exist)")
    out = {}
    for b, sfx in (("off", ""), ("fc", "_fc")):
        out[b] = {"roi": R.load_gpu_ref("roiaware_pool3d_gpu_ref" + sfx),
                  "chamfer": R.load_gpu_ref("chamfer_3d_ref" + sfx)}
    return out


def _bits_equal(a, b):
    """Bit-equal float arrays (any NaN equals any NaN: no payload is part of the contract)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    same = a.view(np.int32) == b.view(np.int32)
    return bool(np.all(same | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------- geometry in float64
def _box_terms(pts, box):
    """float64 local frame of every point for one box: (sx, sy, sz, lx, ly)."""
    p = pts.astype(np.float64)
    cx, cy, cz, dx, dy, dz, rz = (float(v) for v in box)
    sx, sy, sz = p[:, 0] - cx, p[:, 1] - cy, p[:, 2] - cz
    c, s = math.cos(-rz), math.sin(-rz)
    return sx, sy, sz, sx * c - sy * s, sx * s + sy * c


def adversarial(pts, boxes, out_size=None):
    """bool [K, P]: the pair is (nearly) inside and lies within tau of a face, the z slab or (with
    out_size) a voxel boundary along any axis."""
    adv = np.zeros((boxes.shape[0], pts.shape[0]), bool)
    for k, box in enumerate(boxes):
        dx, dy, dz = (float(v) for v in box[3:6])
        sx, sy, sz, lx, ly = _box_terms(pts, box)
        tx = 8 * EPS * (np.abs(sx) + np.abs(sy) + dx)
        ty = 8 * EPS * (np.abs(sx) + np.abs(sy) + dy)
        tz = 8 * EPS * (np.abs(sz) + dz)
        ex, ey, ez = np.abs(lx) - (dx / 2 + MARGIN), np.abs(ly) - (dy / 2 + MARGIN), np.abs(sz) - dz / 2
        near = (ex < tx) & (ey < ty) & (ez < tz)          # inside, or within tau of inside
        a = (np.abs(ex) < tx) | (np.abs(ey) < ty) | (np.abs(ez) < tz)
        if out_size is not None:
            for l, d, n, t in ((lx, dx, out_size[0], tx), (ly, dy, out_size[1], ty),
                               (sz, dz, out_size[2], tz)):
                res = d / n
                f = (l + d / 2) / res
                a |= np.abs(f - np.round(f)) * res < t
        adv[k] = near & a
    return adv


# ------------------------------------------------------------------------- scene construction
def _to_world(box, lx, ly, lz):
    cx, cy, cz, _, _, _, rz = (float(v) for v in box)
    c, s = math.cos(rz), math.sin(rz)
    return np.stack([cx + lx * c - ly * s, cy + lx * s + ly * c, cz + lz], -1).astype(F32)


def make_boxes(g, n, centre=(0.0, 0.0), headings=None, dims=((0.5, 5.0), (0.5, 3.0), (0.5, 2.0))):
    b = np.zeros((n, 7), F32)
    b[:, 0] = centre[0] + g.uniform(-20, 20, n)
    b[:, 1] = centre[1] + g.uniform(-20, 20, n)
    b[:, 2] = g.uniform(-2, 1, n)
    for i, (lo, hi) in enumerate(dims):
        b[:, 3 + i] = g.uniform(lo, hi, n)
    hs = HEADINGS if headings is None else headings
    b[:, 6] = [hs[i % len(hs)] if i < 2 * len(hs) else g.uniform(-4, 4) for i in range(n)]
    return b


def make_points(g, boxes, n, out_size=(1, 1, 1), interior=0.5):
    """n points around the boxes: `interior` of them strictly inside, the rest placed by
    construction on the x/y faces (a few ulps from d/2 + MARGIN), on the z slab, just outside -d/2
    but inside the margin, at exact voxel boundaries, or clear of the box."""
    kinds = ["face", "zslab", "wrap", "vbound", "outside"]
    pts = np.zeros((n, 3), F32)
    for i in range(n):
        box = boxes[g.integers(boxes.shape[0])]
        dx, dy, dz = (float(v) for v in box[3:6])
        lx, ly, lz = g.uniform(-0.45, 0.45, 3) * (dx, dy, dz)
        kind = "inside" if g.random() < interior else kinds[g.integers(len(kinds))]
        axis = g.integers(2)
        sign = 1.0 if g.random() < 0.5 else -1.0
        if kind == "face":
            half = (dx, dy)[axis] / 2 + MARGIN
            v = F32(half)
            for _ in range(int(g.integers(-3, 4))):
                v = np.nextafter(v, F32(np.inf) if g.random() < 0.5 else F32(-np.inf))
            if axis == 0:
                lx = sign * float(v)
            else:
                ly = sign * float(v)
        elif kind == "zslab":
            lz = sign * dz / 2
        elif kind == "wrap":
            if axis == 0:
                lx = -dx / 2 - g.uniform(0.05, 0.95) * MARGIN
            else:
                ly = -dy / 2 - g.uniform(0.05, 0.95) * MARGIN
        elif kind == "vbound":
            n_ax = out_size[axis]
            d = (dx, dy)[axis]
            v = -d / 2 + int(g.integers(0, n_ax + 1)) * d / n_ax
            if axis == 0:
                lx = v
            else:
                ly = v
        elif kind == "outside":
            lx = sign * (dx / 2 + g.uniform(5e-3, 2.0))
        pts[i] = _to_world(box, lx, ly, lz)
        if kind == "zslab":                      # |z - cz| == dz/2 exactly where representable
            z = F32(float(box[2]) + sign * dz / 2)
            pts[i, 2] = z
    return pts


# ------------------------------------------------------------------------- RoI-aware pooling
def ours_roipool(dev, rois, pts, feat, out_size, cap, method, grad_out=None):
    from lidargen.ops.roiaware_pool3d.roiaware_pool3d_utils import RoIAwarePool3dFunction
    from lidarcrafter_amd import ops as K

    r, p, f = (torch.from_numpy(a).to(dev) for a in (rois, pts, feat))
    m = {"max": 0, "avg": 1}[method]
    pooled, vox, am = K.roiaware_pool3d_forward(r, p, f, tuple(out_size), cap, m)
    fr = f.clone().requires_grad_(True)
    y = RoIAwarePool3dFunction.apply(r, p, fr, tuple(out_size), cap, method)
    assert _bits_equal(y.detach().cpu().numpy(), pooled.cpu().numpy())  # the autograd API, same kernels
    y.backward(torch.from_numpy(grad_out).to(dev))
    torch.cuda.synchronize()
    return pooled.cpu().numpy(), vox.cpu().numpy(), am.cpu().numpy(), fr.grad.cpu().numpy()


def ref_roipool(mod, dev, rois, pts, feat, out_size, cap, method, grad_out):
    """As the reference's RoIAwarePool3dFunction allocates: zeros for pooled, argmax, voxels."""
    N, C = rois.shape[0], feat.shape[1]
    r, p, f = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rois, pts, feat))
    pooled = torch.zeros((N, *out_size, C), device=dev, dtype=torch.float32)
    am = torch.zeros((N, *out_size, C), device=dev, dtype=torch.int32)
    vox = torch.zeros((N, *out_size, cap), device=dev, dtype=torch.int32)
    m = {"max": 0, "avg": 1}[method]
    torch.cuda.synchronize()
    mod.forward(r, p, f, am, vox, pooled, m)
    torch.cuda.synchronize()
    gin = torch.zeros((pts.shape[0], C), device=dev, dtype=torch.float32)
    go = torch.from_numpy(np.ascontiguousarray(grad_out)).to(dev)
    mod.backward(vox, am, go, gin, m)
    torch.cuda.synchronize()
    return pooled.cpu().numpy(), vox.cpu().numpy(), am.cpu().numpy(), gin.cpu().numpy()


def _members(vox):
    """{(box, point): flat voxel} and the per-voxel counts [K, V]."""
    K_, cap = vox.shape[0], vox.shape[-1]
    v = vox.reshape(K_, -1, cap)
    where = {}
    for b in range(K_):
        for j in np.nonzero(v[b, :, 0])[0]:
            for p in v[b, j, 1:1 + v[b, j, 0]]:
                where[(b, int(p))] = int(j)
    return where, v[..., 0]


def _bwd_bounds(vox, am, grad_out, n_pts, method):
    """float64 contribution count and |sum| per (point, channel) of the reference backward."""
    K_, cap = vox.shape[0], vox.shape[-1]
    C = grad_out.shape[-1]
    go = grad_out.reshape(K_, -1, C).astype(np.float64)
    cnt = np.zeros((n_pts, C))
    mag = np.zeros((n_pts, C))
    if method == "max":
        a = am.reshape(K_, -1, C)
        m = a >= 0
        ch = np.broadcast_to(np.arange(C), a.shape)
        np.add.at(cnt, (a[m], ch[m]), 1)
        np.add.at(mag, (a[m], ch[m]), np.abs(go[m]))
    else:
        v = vox.reshape(K_, -1, cap)
        for b in range(K_):
            for j in np.nonzero(v[b, :, 0])[0]:
                c = v[b, j, 0]
                for p in v[b, j, 1:1 + c]:
                    cnt[p] += 1
                    mag[p] += np.abs(go[b, j]) / c
    return cnt, mag


def _check_backward(g_ours, g_ref, vox, am, grad_out, method, tag):
    cnt, mag = _bwd_bounds(vox, am, grad_out, g_ours.shape[0], method)
    one = cnt <= 1
    assert _bits_equal(g_ours[one], g_ref[one]), f"{tag}: single-contribution gradient differs"
    tol = 2 * cnt[~one] * EPS * mag[~one]
    err = np.abs(g_ours[~one].astype(np.float64) - g_ref[~one])
    assert np.all(err <= tol), f"{tag}: backward beyond fp32 atomic reorder, max {err.max()}"


ROI_CASES = {
    # name: (boxes, points, channels, out_size, cap, features)
    "1box_1pt_c1_111": (1, 1, 1, (1, 1, 1), 2, "normal"),
    "1box_1000pts_c4_322_overflow": (1, 1000, 4, (3, 2, 2), 16, "normal"),
    "300box_1000pts_c130_753": (300, 1000, 130, (7, 5, 3), 128, "normal"),
    "300box_777pts_c4_255x2x1_cap2": (300, 777, 4, (255, 2, 1), 2, "normal"),
    "far_centre_779pts_c4_753": (40, 779, 4, (7, 5, 3), 16, "normal"),
    "ties_specials_833pts_c4_322": (12, 833, 4, (3, 2, 2), 128, "specials"),
    "tiny_box_negative_wrap_255": (3, 500, 1, (255, 2, 1), 128, "ties"),
}


def _roi_scene(name):
    nb, npts, C, out_size, cap, fmode = ROI_CASES[name]
    g = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("far_centre"):
        boxes = make_boxes(g, nb, centre=(1e3, -1e3), headings=[7.5, -20.0, 0.0, math.pi])
    elif name.startswith("tiny_box"):
        # voxels of dx/255 < MARGIN: a point just outside -dx/2 truncates to a NEGATIVE index,
        # which the reference stores into an unsigned and clamps to out_x - 1
        boxes = make_boxes(g, nb, dims=((1.5e-4, 3e-4), (1.5e-4, 3e-4), (0.5, 1.0)),
                           headings=[0.0, math.pi / 2, -20.0])
        boxes[:, :2] = g.uniform(-0.5, 0.5, (nb, 2))
    else:
        boxes = make_boxes(g, nb)
    pts = make_points(g, boxes, npts, out_size)
    if name.startswith("tiny_box"):
        # clear wraps: k + 1/2 voxels below -dx/2, all inside the margin
        for i in range(0, npts, 3):
            box = boxes[g.integers(nb)]
            dx, dy, dz = (float(v) for v in box[3:6])
            k = g.integers(1, int(0.9 * MARGIN * out_size[0] / dx)) + 0.5
            pts[i] = _to_world(box, -dx / 2 - k * dx / out_size[0], g.uniform(-0.4, 0.4) * dy,
                               g.uniform(-0.4, 0.4) * dz)
    if name.endswith("overflow"):
        box = boxes[0]
        dx, dy, dz = (float(v) for v in box[3:6])
        # 40 points in one voxel (0, 0, 0) with cap 16: 25 of them overflow
        lx = -dx / 2 + g.uniform(0.1, 0.9, 40) * dx / 3
        ly = -dy / 2 + g.uniform(0.1, 0.9, 40) * dy / 2
        lz = -dz / 2 + g.uniform(0.1, 0.9, 40) * dz / 2
        pts[:40] = _to_world(box, lx, ly, lz)
    if fmode == "normal":
        feat = g.normal(size=(npts, C)).astype(F32)
    else:
        # few distinct values: duplicates inside every voxel (the lowest slot must win)
        feat = g.integers(0, 3, (npts, C)).astype(F32)
        if fmode == "specials":
            sp = np.array([-np.inf, np.nan, -np.finfo(F32).max], F32)
            m = g.random((npts, C)) < 0.3
            feat[m] = sp[g.integers(0, 3, m.sum())]
            feat[g.random(npts) < 0.1] = -np.inf               # whole rows of -inf ...
            feat[g.random(npts) < 0.05] = np.nan               # ... and of NaN
    return boxes, pts, feat, out_size, cap


@pytest.mark.parametrize("method", ["max", "avg"])
@pytest.mark.parametrize("case", list(ROI_CASES))
def test_roiaware_pool3d_vs_reference_kernel(dev, ref, case, method):
    boxes, pts, feat, out_size, cap = _roi_scene(case)
    K_, C = boxes.shape[0], feat.shape[1]
    assert K_ * pts.shape[0] < 10 ** 7                    # the reference's internal box x point mask
    g = np.random.default_rng(7)
    adv = adversarial(pts, boxes, out_size)
    bulk = ~adv.any(0)
    assert bulk.sum() > 0
    grad_out = g.normal(size=(K_, *out_size, C)).astype(F32)

    # bulk: every output bit-equal in both builds
    ob = ours_roipool(dev, boxes, pts[bulk], feat[bulk], out_size, cap, method, grad_out)
    for build in BUILDS:
        rb = ref_roipool(ref[build]["roi"], dev, boxes, pts[bulk], feat[bulk], out_size, cap,
                         method, grad_out)
        tag = f"{case}/{method}/{build}/bulk"
        assert np.array_equal(ob[1], rb[1]), f"{tag}: pts_idx_of_voxels"
        if method == "max":
            assert np.array_equal(ob[2], rb[2]), f"{tag}: argmax"
        assert _bits_equal(ob[0], rb[0]), f"{tag}: pooled"
        _check_backward(ob[3], rb[3], rb[1], rb[2], grad_out, method, tag)
    if case.startswith("tiny_box"):                      # the wrap itself is exercised
        w, _ = _members(ob[1])
        assert sum(1 for (b, _), v in w.items() if v // (out_size[1] * out_size[2]) == 254) > 0
    if case.endswith("overflow"):
        assert ob[1][..., 0].max() == cap - 1

    # everything: a pair may move only within tau of a threshold
    of = ours_roipool(dev, boxes, pts, feat, out_size, cap, method, grad_out)
    wo, co = _members(of[1])
    V = int(np.prod(out_size))
    for build in BUILDS:
        rf = ref_roipool(ref[build]["roi"], dev, boxes, pts, feat, out_size, cap, method,
                         grad_out)
        wr, cr = _members(rf[1])
        moved = []
        for key in set(wo) | set(wr):
            a, b = wo.get(key), wr.get(key)
            if a == b:
                continue
            bi, p = key
            if adv[bi, p]:
                moved.append(key)
                continue
            # a clear point may only be crowded out of a voxel that a moved point filled
            full = (a is not None and cr[bi, a] == cap - 1) or (b is not None and co[bi, b] == cap - 1)
            assert full, f"{case}/{method}/{build}: point {p} in box {bi} moved from voxel " \
                         f"{b} (reference) to {a} (ours) although it is >= tau from every threshold"
        print(f"\n[tau-bounded] roiaware_pool3d {case}/{method}/{build}: {len(moved)} "
              f"(box, point) pairs {sorted(moved)[:8]}")
        same = np.all(of[1].reshape(K_, V, cap) == rf[1].reshape(K_, V, cap), axis=-1)
        po, pr = of[0].reshape(K_, V, C), rf[0].reshape(K_, V, C)
        assert _bits_equal(po[same], pr[same]), f"{case}/{method}/{build}: pooled on agreeing voxels"
        if method == "max":
            assert np.array_equal(of[2].reshape(K_, V, C)[same], rf[2].reshape(K_, V, C)[same])


# ------------------------------------------------------------------------- chamfer
def _f32_dist(q, t):
    """(dx*dx + dy*dy) + dz*dz, every operation rounded to float32 (no contraction)."""
    d = (t - q).astype(F32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F32)


def _chamfer_scene(B, N, M, kind, seed):
    g = np.random.default_rng(seed)
    if kind == "large":
        base = g.uniform(-1e4, 1e4, (B, 1, 3))
        a = (base + g.uniform(-1, 1, (B, N, 3)) * 1e-2).astype(F32)
        b = (base + g.uniform(-1, 1, (B, M, 3)) * 1e-2).astype(F32)
        return a, b
    a = g.normal(0, 5, (B, N, 3)).astype(F32)
    if kind == "same":
        return a, a.copy()
    b = g.normal(0, 5, (B, M, 3)).astype(F32)
    if kind == "dups":
        # duplicated targets within a group of four and across the 512-target chunk boundary;
        # queries sit next to them, so that the duplicate pair is the nearest (the first must win)
        pairs = [(k, k + d) for k in (0, 4, 9, 100, 508) for d in (1, 2, 3)] + \
                [(1, 513), (511, 512), (100, 612), (3, 1027), (600, 1536)]
        used = []
        for i, j in pairs:
            if j < M:
                b[:, j] = b[:, i]
                used.append(i)
        for r in range(min(N, 4 * len(used))):
            a[:, r] = b[:, used[r % len(used)]] + g.normal(0, 1e-3, (B, 3)).astype(F32)
    return a, b


CHAMFER_CASES = [
    (1, 1, 1, "rand"), (1, 3, 5, "rand"), (3, 4, 511, "rand"), (3, 5, 512, "rand"),
    (1, 511, 513, "rand"), (3, 512, 1025, "dups"), (40, 513, 4, "rand"), (40, 3, 2049, "dups"),
    (1, 9000, 513, "rand"), (3, 1025, 2049, "dups"), (3, 2049, 2049, "same"),
    (1, 513, 513, "same"), (3, 1025, 513, "large"), (40, 4, 5, "rand"),
]


def ref_chamfer(mod, dev, a, b):
    """As the reference's chamfer_3DFunction allocates: zeros of [B,N] / [B,M]."""
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    x, y = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    d1 = torch.zeros((B, N), device=dev)
    d2 = torch.zeros((B, M), device=dev)
    i1 = torch.zeros((B, N), device=dev, dtype=torch.int32)
    i2 = torch.zeros((B, M), device=dev, dtype=torch.int32)
    torch.cuda.synchronize()
    mod.forward(x, y, d1, d2, i1, i2)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (d1, d2, i1, i2)]


def _ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("B,N,M,kind", CHAMFER_CASES)
def test_chamfer3d_vs_reference_kernel(dev, ref, B, N, M, kind):
    import lidargen  # noqa: F401
    from lidargen.metrics import chamfer

    a, b = _chamfer_scene(B, N, M, kind, B * 100003 + N * 31 + M)
    x, y = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    ours = [t.cpu().numpy() for t in chamfer.chamfer_3DDist()(x, y)]
    torch.cuda.synchronize()
    off = ref_chamfer(ref["off"]["chamfer"], dev, a, b)
    fc = ref_chamfer(ref["fc"]["chamfer"], dev, a, b)
    moved = 0
    for way, (q, t) in enumerate(((a, b), (b, a))):
        d, i = ours[way], ours[way + 2]
        assert _bits_equal(d, off[way]), f"dist{way + 1} vs the contract-off reference"
        assert np.array_equal(i, off[way + 2]), f"idx{way + 1} vs the contract-off reference"
        assert np.all(_ulps(d, fc[way]) <= 4), f"dist{way + 1} vs the default-contraction reference"
        j = fc[way + 2]
        diff = i != j
        if diff.any():
            bi, qi = np.nonzero(diff)
            da = _f32_dist(q[bi, qi], t[bi, i[diff]])
            db = _f32_dist(q[bi, qi], t[bi, j[diff]])
            assert np.all(_ulps(da, db) <= 4), f"idx{way + 1}: a choice between distinct distances"
            moved += int(diff.sum())
        # independently of the reference: the chosen neighbour is a float64 nearest one
        q64, t64 = q.astype(np.float64), t.astype(np.float64)
        for bb in range(B):
            best = np.concatenate([((q64[bb, r:r + 256, None, :] - t64[bb, None]) ** 2).sum(-1).min(1)
                                   for r in range(0, q.shape[1], 256)])
            chosen = ((q64[bb] - t64[bb, i[bb]]) ** 2).sum(-1)
            tol = 4 * np.spacing(best.astype(F32)).astype(np.float64)
            assert np.all(chosen - best <= tol), f"way {way}: not a float64 nearest neighbour"
        if kind == "same":
            assert np.all(d == 0) and np.all(i == np.arange(q.shape[1]))
    print(f"\n[tau-bounded] chamfer B={B} N={N} M={M} {kind}: off 0, fc {moved} index choices")
    if B == 1:
        cd = chamfer.compute_pairwise_cd(a[0], b[0])
        want = (float(off[0][0].astype(np.float64).mean()) + float(off[1][0].astype(np.float64).mean())) / 2
        d1, d2 = torch.from_numpy(ours[0]).to(dev), torch.from_numpy(ours[1]).to(dev)
        assert cd == ((d1.mean() + d2.mean()) / 2).item()
        assert abs(cd - want) <= 1e-5 * abs(want)


# ------------------------------------------------------------------------- first-hit points-in-boxes
PIB_CASES = {
    "B1_12boxes": (1, 12, 3000),
    "B3_12boxes_overlap": (3, 12, 2999),
    "B1_2600boxes": (1, 2600, 4001),
    "B3_2600boxes_overlap": (3, 2600, 1537),
}


def _pib_scene(name):
    B, nb, npts = PIB_CASES[name]
    g = np.random.default_rng(sum(map(ord, name)))
    boxes = np.stack([make_boxes(g, nb) for _ in range(B)])
    if "overlap" in name:                                 # pairs of overlapping boxes: the first hit decides
        boxes[:, 1::2, :3] = boxes[:, 0::2, :3][:, :boxes[:, 1::2].shape[1]] + \
            g.uniform(-0.3, 0.3, (B, boxes[:, 1::2].shape[1], 3)).astype(F32)
    boxes[:, nb // 2, :3] = (3e3, -3e3, 0.0)               # a far box that holds no point
    near = [k for k in range(nb) if k != nb // 2]
    pts = np.stack([make_points(g, boxes[b, near], npts) for b in range(B)])
    # the band between margins 1e-5 and 1e-2 outside the x faces: outside at 1e-5
    for b in range(B):
        for i in range(0, npts, 17):
            box = boxes[b, near[g.integers(nb - 1)]]
            dx, dy, dz = (float(v) for v in box[3:6])
            lx = (1 if i % 2 else -1) * (dx / 2 + g.uniform(1e-3, 9e-3))
            pts[b, i] = _to_world(box, lx, g.uniform(-0.4, 0.4) * dy, g.uniform(-0.4, 0.4) * dz)
    return boxes, pts


@pytest.mark.parametrize("case", list(PIB_CASES))
def test_points_in_boxes_first_hit_vs_reference_kernel(dev, ref, case):
    from lidargen.ops.roiaware_pool3d.roiaware_pool3d_utils import points_in_boxes_gpu

    boxes, pts = _pib_scene(case)
    B, nb = boxes.shape[:2]
    x, bx = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
    ours = points_in_boxes_gpu(x, bx).cpu().numpy()
    torch.cuda.synchronize()
    assert (ours == nb // 2).sum() == 0 and (ours >= 0).any()
    for build in BUILDS:
        out = torch.full((B, pts.shape[1]), -1, device=dev, dtype=torch.int32)
        torch.cuda.synchronize()
        ref[build]["roi"].points_in_boxes_gpu(bx, x, out)
        torch.cuda.synchronize()
        r = out.cpu().numpy()
        moved = 0
        for b in range(B):
            adv = adversarial(pts[b], boxes[b])
            diff = np.nonzero(ours[b] != r[b])[0]
            for p in diff:
                last = max(ours[b, p], r[b, p])
                # only an inside flag within tau of its face, at or before the later hit, may flip
                assert adv[:last + 1, p].any(), \
                    f"{case}/{build}: point {p} of batch {b}: ours {ours[b, p]}, reference {r[b, p]}"
            moved += len(diff)
            clear = ~adv.any(0)
            assert np.array_equal(ours[b, clear], r[b, clear]), f"{case}/{build}: bulk"
        print(f"\n[tau-bounded] points_in_boxes {case}/{build}: {moved} points")
