"""numpy restatement of the rotated-box geometry of csrc/iou3d_box.h, the same statements in the same
order, vectorised over pairs and parameterised by dtype: float32 mirrors the header operation by operation (numpy does
not contract, its cos / sin / arctan2 may differ from libm's by an ulp), float64 is the yardstick's other end.  Boxes are
rows [x, y, z, dx, dy, dz, heading]."""
import numpy as np

MAX_PTS = 16


def _turn(p, c, cs, sn):
    """lc_iou3d_turn: p - c turned by the angle of cosine cs and sine sn; points are [P,2]."""
    ox, oy = p[:, 0] - c[:, 0], p[:, 1] - c[:, 1]
    return np.stack([ox * cs + oy * (-sn), ox * sn + oy * cs], axis=1)


def _orient(o, u, v):
    """lc_iou3d_orient: the z component of (u - o) x (v - o)."""
    return (u[:, 0] - o[:, 0]) * (v[:, 1] - o[:, 1]) - (v[:, 0] - o[:, 0]) * (u[:, 1] - o[:, 1])


def _spans_meet(a, b, c, d):
    return (np.minimum(a, b) <= np.maximum(c, d)) & (np.minimum(c, d) <= np.maximum(a, b))


def _segments_cross(e0, e1, f0, f1, eps):
    """lc_iou3d_segments_cross: (crosses [P], hit [P,2])."""
    near = _spans_meet(e0[:, 0], e1[:, 0], f0[:, 0], f1[:, 0]) & _spans_meet(e0[:, 1], e1[:, 1], f0[:, 1], f1[:, 1])
    f0_side, f1_side = _orient(e0, f0, e1), _orient(e0, e1, f1)
    e0_side, e1_side = _orient(f0, e0, f1), _orient(f0, f1, e1)
    crosses = near & (f0_side * f1_side > 0) & (e0_side * e1_side > 0)
    f1_neg = _orient(e0, f1, e1)
    span = f1_neg - f0_side
    by_ratio = (f1_neg[:, None] * f0 - f0_side[:, None] * f1) / span[:, None]
    eu, ev, ew = e0[:, 1] - e1[:, 1], e1[:, 0] - e0[:, 0], e0[:, 0] * e1[:, 1] - e1[:, 0] * e0[:, 1]
    fu, fv, fw = f0[:, 1] - f1[:, 1], f1[:, 0] - f0[:, 0], f0[:, 0] * f1[:, 1] - f1[:, 0] * f0[:, 1]
    det = eu * fv - fu * ev
    by_lines = np.stack([(ev * fw - fv * ew) / det, (fu * ew - eu * fw) / det], axis=1)
    return crosses, np.where((np.abs(span) > eps)[:, None], by_ratio, by_lines)


def _holds(box, p, margin):
    """lc_iou3d_obb_holds: p within the box grown by margin, tested in the box's frame."""
    local = _turn(p, box[:, :2], np.cos(-box[:, 6]), np.sin(-box[:, 6]))
    return (np.abs(local[:, 0]) < box[:, 3] / 2 + margin) & (np.abs(local[:, 1]) < box[:, 4] / 2 + margin)


def _corners(box):
    """The four turned corners of lc_iou3d_obb_make, the first repeated at the end."""
    c, hx, hy = box[:, :2], box[:, 3] / 2, box[:, 4] / 2
    lo_x, lo_y, hi_x, hi_y = c[:, 0] - hx, c[:, 1] - hy, c[:, 0] + hx, c[:, 1] + hy
    cs, sn = np.cos(box[:, 6]), np.sin(box[:, 6])
    out = [_turn(np.stack(flat, axis=1), c, cs, sn) + c for flat in ((lo_x, lo_y), (hi_x, lo_y), (hi_x, hi_y), (lo_x, hi_y))]
    return out + [out[0]]


def box_overlap(a, b, dtype=np.float32):
    """(area [P], cnt int [P]) of the paired rows a[i], b[i]."""
    a = np.ascontiguousarray(a, dtype).reshape(-1, 7)
    b = np.ascontiguousarray(b, dtype).reshape(-1, 7)
    P = a.shape[0]
    eps, margin = dtype(1e-8), dtype(1e-2)
    rows = np.arange(P)
    with np.errstate(all="ignore"):
        ca, cb = _corners(a), _corners(b)
        pts = np.zeros((P, MAX_PTS, 2), dtype)
        center = np.zeros((P, 2), dtype)
        cnt = np.zeros(P, np.int64)

        def append(flag, x):
            nonlocal center
            ok = flag & (cnt < MAX_PTS)
            center = np.where(ok[:, None], center + x, center)
            pts[rows[ok], cnt[ok]] = x[ok]
            cnt[ok] += 1

        for i in range(4):
            for j in range(4):
                append(*_segments_cross(ca[i], ca[i + 1], cb[j], cb[j + 1], eps))
        for k in range(4):
            append(_holds(a, cb[k], margin), cb[k])
            append(_holds(b, ca[k], margin), ca[k])
        center = center / cnt[:, None].astype(dtype)
        cmax = int(cnt.max()) if P else 0
        for j in range(cmax - 1):
            for i in range(cmax - j - 1):
                u, v = pts[:, i].copy(), pts[:, i + 1].copy()
                swap = (i < cnt - j - 1) & (np.arctan2(u[:, 1] - center[:, 1], u[:, 0] - center[:, 0]) >
                                            np.arctan2(v[:, 1] - center[:, 1], v[:, 0] - center[:, 0]))
                pts[:, i] = np.where(swap[:, None], v, u)
                pts[:, i + 1] = np.where(swap[:, None], u, v)
        area = np.zeros(P, dtype)
        for k in range(cmax - 1):
            du, dv = pts[:, k] - pts[:, 0], pts[:, k + 1] - pts[:, 0]
            area = np.where(k < cnt - 1, area + (du[:, 0] * dv[:, 1] - du[:, 1] * dv[:, 0]), area)
        return np.abs(area) / 2, cnt


def iou_bev(a, b, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1, 7)
    b = np.ascontiguousarray(b, dtype).reshape(-1, 7)
    s, _ = box_overlap(a, b, dtype)
    return s / np.maximum(a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4] - s, dtype(1e-8))


def iou_normal(a, b, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1, 7)
    b = np.ascontiguousarray(b, dtype).reshape(-1, 7)

    def span_overlap(ca, da, cb, db):
        return np.maximum(np.minimum(ca + da / 2, cb + db / 2) - np.maximum(ca - da / 2, cb - db / 2), dtype(0))

    inter = span_overlap(a[:, 0], a[:, 3], b[:, 0], b[:, 3]) * span_overlap(a[:, 1], a[:, 4], b[:, 1], b[:, 4])
    return inter / np.maximum(a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4] - inter, dtype(1e-8))


def all_pairs(a, b):
    """The rows of a and b expanded to the N * M pairs of the row-major [N, M] grid."""
    a, b = np.asarray(a).reshape(-1, 7), np.asarray(b).reshape(-1, 7)
    return np.repeat(a, b.shape[0], axis=0), np.tile(b, (a.shape[0], 1))


def greedy_keep(iou, thresh):
    """The reference's walk: box i is kept unless an earlier kept box j has iou[j, i] > thresh."""
    n = iou.shape[0]
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if not removed[i]:
            keep.append(i)
            removed[i + 1:] |= iou[i, i + 1:] > thresh
    return keep


def greedy_keep_mask(mask_bits):
    """The same walk over a boolean [N, N] suppression matrix (only the entries right of the diagonal are read)."""
    return greedy_keep(np.triu(np.asarray(mask_bits, bool), 1).astype(np.float64), 0.5)


def rect_overlap_f32(a, b):
    """Analytic overlap area and IoU of heading-0 rows in float32 (exact on quarter-grid coordinates)."""
    a, b = np.asarray(a, np.float32).reshape(-1, 7), np.asarray(b, np.float32).reshape(-1, 7)
    w = np.minimum(a[:, 0] + a[:, 3] / 2, b[:, 0] + b[:, 3] / 2) - np.maximum(a[:, 0] - a[:, 3] / 2, b[:, 0] - b[:, 3] / 2)
    h = np.minimum(a[:, 1] + a[:, 4] / 2, b[:, 1] + b[:, 4] / 2) - np.maximum(a[:, 1] - a[:, 4] / 2, b[:, 1] - b[:, 4] / 2)
    s = np.maximum(w, np.float32(0)) * np.maximum(h, np.float32(0))
    return s, s / np.maximum(a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4] - s, np.float32(1e-8))


def general_boxes(rng, n, spread=4.0, centres=None):
    """[n,7] float32 of the general class: centres uniform in [-spread, spread]^2 (or around `centres`), dx in [0.5, 5],
    dy in [0.5, 3], heading in [-pi, pi]; z in [-1, 1], dz in [1, 2]."""
    xy = rng.uniform(-spread, spread, (n, 2)) if centres is None else centres
    return np.stack([xy[:, 0], xy[:, 1], rng.uniform(-1, 1, n), rng.uniform(0.5, 5, n), rng.uniform(0.5, 3, n),
                     rng.uniform(1, 2, n), rng.uniform(-np.pi, np.pi, n)], axis=1).astype(np.float32)


def exact_boxes(rng, n):
    """[n,7] float32 of the exact class: heading 0, coordinates multiples of 1/4, sizes multiples of 1/2."""
    return np.stack([rng.integers(-16, 17, n) / 4, rng.integers(-16, 17, n) / 4, rng.integers(-8, 9, n) / 4,
                     rng.integers(1, 11, n) / 2, rng.integers(1, 7, n) / 2, rng.integers(1, 5, n) / 2, np.zeros(n)],
                    axis=1).astype(np.float32)


NAMED_EXACT = {   # (a, b, overlap, iou)
    "identical": ([1.0, -0.5, 0, 2.0, 1.0, 1, 0], [1.0, -0.5, 0, 2.0, 1.0, 1, 0], 2.0, 1.0),
    "touching": ([0.0, 0.0, 0, 2.0, 1.0, 1, 0], [2.0, 0.0, 0, 2.0, 1.0, 1, 0], 0.0, 0.0),
    "nested": ([0.0, 0.0, 0, 4.0, 2.0, 1, 0], [0.5, 0.25, 0, 1.0, 0.5, 1, 0], 0.5, 0.0625),
    "disjoint": ([0.0, 0.0, 0, 2.0, 1.0, 1, 0], [5.0, 3.0, 0, 2.0, 1.0, 1, 0], 0.0, 0.0),
}
