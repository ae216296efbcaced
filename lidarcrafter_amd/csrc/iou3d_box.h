// Rotated-box geometry of lidargen.ops.iou3d_nms, once, for the host and the device: what the
// reference's iou3d_nms kernels compute per pair of rows [x, y, z, dx, dy, dz, heading], in float32 and in the reference's
// order of operations, written around this project's own three pieces:
//   lc_iou3d_obb    a row prepared once: centre, half extents, the sine / cosine of the heading and of its negative, and the
//                   four turned corners (the axis-aligned corner first, then (p - c) turned by the heading, plus c);
//   lc_iou3d_poly   the overlap polygon under construction: where the caller keeps its 16 points, how many there are and
//                   their running coordinate sum.  lc_iou3d_poly_push is the ONLY writer and refuses a 17th point;
//   lc_iou3d_box_overlap / lc_iou3d_iou_bev / lc_iou3d_iou_normal over them.
//
// The polygon is collected in this order: edge i of a against edge j of b, row-major over the 16 pairs -- behind a test of the
// edges' bounding intervals and the STRICT test that each edge's end points lie on opposite sides of the other edge (both
// products of orientations > 0), the crossing point from the orientation ratio while |difference| > EPS, else from the two
// line equations --; then for k = 0..3 b's corner k if a contains it and a's corner k if b contains it (within MARGIN, in
// the containing box's frame).  The points are bubble-sorted by atan2 about their mean (sum / count) with the comparison
// `>`, the area is half the absolute fan sum from point 0.  Nothing is special-cased: no point means 0 / 0 for a mean nobody
// reads; two identical boxes give their 8 corners (4 twice) and the exact area.
//
// Valid geometry gives at most 8 crossings + 8 corners, so the bound of 16 changes nothing there; on NaN / inf / garbage rows
// it is what keeps the walk inside its array.
//
// The 16 points live where the caller says (`room`, with a stride in points between consecutive entries): the host passes a
// local array (stride 1); the kernels of csrc/iou3d_nms.hip pass a lane's column of an LDS array (stride = lanes per block),
// because an array indexed by a runtime count cannot live in registers on CDNA and would go to scratch memory.
//
// Compiles under hipcc (LC_IOU3D_HD = __host__ __device__) and under a plain C++ compiler (LC_IOU3D_HD empty).
#ifndef LC_IOU3D_BOX_H
#define LC_IOU3D_BOX_H
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define LC_IOU3D_HD __host__ __device__
#define LC_IOU3D_UNROLL _Pragma("unroll")
#else
#define LC_IOU3D_HD
#define LC_IOU3D_UNROLL
#endif

#define LC_IOU3D_EPS 1e-8f
#define LC_IOU3D_MARGIN 1e-2f
#define LC_IOU3D_MAX_PTS 16

struct lc_iou3d_pt {
    float x, y;
};

struct lc_iou3d_obb {
    lc_iou3d_pt c;            // centre
    float hx, hy;             // half extents along the box's own axes
    float cs, sn;             // cos / sin of the heading
    float ncs, nsn;           // cos / sin of minus the heading
    lc_iou3d_pt corner[4];    // counter-clockwise from (-hx, -hy), turned by the heading
};

struct lc_iou3d_poly {
    lc_iou3d_pt* room;
    int stride, n;
    lc_iou3d_pt sum;
};

// p - c turned by the angle whose cosine / sine are given: (d.x cs + d.y (-sn), d.x sn + d.y cs)
LC_IOU3D_HD static inline lc_iou3d_pt lc_iou3d_turn(lc_iou3d_pt p, lc_iou3d_pt c, float cs, float sn) {
    const float ox = p.x - c.x, oy = p.y - c.y;
    lc_iou3d_pt r;
    r.x = ox * cs + oy * (-sn);
    r.y = ox * sn + oy * cs;
    return r;
}

LC_IOU3D_HD static inline lc_iou3d_obb lc_iou3d_obb_make(const float* row) {
    lc_iou3d_obb b;
    b.c.x = row[0];
    b.c.y = row[1];
    b.hx = row[3] / 2;
    b.hy = row[4] / 2;
    b.cs = cosf(row[6]);
    b.sn = sinf(row[6]);
    b.ncs = cosf(-row[6]);
    b.nsn = sinf(-row[6]);
    const float lo_x = b.c.x - b.hx, lo_y = b.c.y - b.hy, hi_x = b.c.x + b.hx, hi_y = b.c.y + b.hy;
    const lc_iou3d_pt flat[4] = {{lo_x, lo_y}, {hi_x, lo_y}, {hi_x, hi_y}, {lo_x, hi_y}};
    LC_IOU3D_UNROLL
    for (int k = 0; k < 4; k++) {
        const lc_iou3d_pt t = lc_iou3d_turn(flat[k], b.c, b.cs, b.sn);
        b.corner[k].x = t.x + b.c.x;
        b.corner[k].y = t.y + b.c.y;
    }
    return b;
}

// p lies in b, grown by MARGIN on every side: p is brought into b's frame (turned by minus the heading)
LC_IOU3D_HD static inline bool lc_iou3d_obb_holds(const lc_iou3d_obb& b, lc_iou3d_pt p) {
    const lc_iou3d_pt local = lc_iou3d_turn(p, b.c, b.ncs, b.nsn);
    return fabsf(local.x) < b.hx + LC_IOU3D_MARGIN && fabsf(local.y) < b.hy + LC_IOU3D_MARGIN;
}

// orientation of (u, v) seen from o: the z component of (u - o) x (v - o)
LC_IOU3D_HD static inline float lc_iou3d_orient(lc_iou3d_pt o, lc_iou3d_pt u, lc_iou3d_pt v) {
    return (u.x - o.x) * (v.y - o.y) - (v.x - o.x) * (u.y - o.y);
}

// the closed intervals [min(a, b), max(a, b)] and [min(c, d), max(c, d)] meet
LC_IOU3D_HD static inline bool lc_iou3d_spans_meet(float a, float b, float c, float d) {
    return fminf(a, b) <= fmaxf(c, d) && fminf(c, d) <= fmaxf(a, b);
}

// Do the segments e0-e1 and f0-f1 cross properly?  If so, *hit is the crossing point.
LC_IOU3D_HD static inline bool lc_iou3d_segments_cross(lc_iou3d_pt e0, lc_iou3d_pt e1, lc_iou3d_pt f0, lc_iou3d_pt f1,
                                                       lc_iou3d_pt* hit) {
    if (!(lc_iou3d_spans_meet(e0.x, e1.x, f0.x, f1.x) && lc_iou3d_spans_meet(e0.y, e1.y, f0.y, f1.y))) return false;
    const float f0_side = lc_iou3d_orient(e0, f0, e1);      // f0 and f1 on opposite sides of e: these two have one sign
    const float f1_side = lc_iou3d_orient(e0, e1, f1);
    const float e0_side = lc_iou3d_orient(f0, e0, f1);      // likewise e0 and e1 about f
    const float e1_side = lc_iou3d_orient(f0, f1, e1);
    if (!(f0_side * f1_side > 0 && e0_side * e1_side > 0)) return false;
    const float f1_neg = lc_iou3d_orient(e0, f1, e1);       // f1's orientation with f0's sign convention
    const float span = f1_neg - f0_side;
    if (fabsf(span) > LC_IOU3D_EPS) {
        // f0 and f1 weighted by each other's distance from e
        hit->x = (f1_neg * f0.x - f0_side * f1.x) / span;
        hit->y = (f1_neg * f0.y - f0_side * f1.y) / span;
    } else {
        // the lines u x + v y + w = 0 through e and through f, solved by Cramer's rule
        const float eu = e0.y - e1.y, ev = e1.x - e0.x, ew = e0.x * e1.y - e1.x * e0.y;
        const float fu = f0.y - f1.y, fv = f1.x - f0.x, fw = f0.x * f1.y - f1.x * f0.y;
        const float det = eu * fv - fu * ev;
        hit->x = (ev * fw - fv * ew) / det;
        hit->y = (fu * ew - eu * fw) / det;
    }
    return true;
}

LC_IOU3D_HD static inline void lc_iou3d_poly_push(lc_iou3d_poly& poly, lc_iou3d_pt p) {
    if (poly.n >= LC_IOU3D_MAX_PTS) return;       // never a 17th point
    poly.sum.x = poly.sum.x + p.x;
    poly.sum.y = poly.sum.y + p.y;
    poly.room[poly.n * poly.stride] = p;
    poly.n++;
}

LC_IOU3D_HD static inline float lc_iou3d_bearing(lc_iou3d_pt p, lc_iou3d_pt about) {
    return atan2f(p.y - about.y, p.x - about.x);
}

// The overlap area of the BEV rectangles of two rows.  room[k * stride], k < 16, is the caller's room for the polygon;
// *count (may be null) receives the number of points found.
LC_IOU3D_HD static inline float lc_iou3d_box_overlap(const float* row_a, const float* row_b, lc_iou3d_pt* room, int stride,
                                                     int* count) {
    const lc_iou3d_obb a = lc_iou3d_obb_make(row_a), b = lc_iou3d_obb_make(row_b);
    lc_iou3d_poly poly = {room, stride, 0, {0.f, 0.f}};

    LC_IOU3D_UNROLL
    for (int i = 0; i < 4; i++) {
        LC_IOU3D_UNROLL
        for (int j = 0; j < 4; j++) {
            lc_iou3d_pt hit;
            if (lc_iou3d_segments_cross(a.corner[i], a.corner[(i + 1) & 3], b.corner[j], b.corner[(j + 1) & 3], &hit))
                lc_iou3d_poly_push(poly, hit);
        }
    }
    LC_IOU3D_UNROLL
    for (int k = 0; k < 4; k++) {
        if (lc_iou3d_obb_holds(a, b.corner[k])) lc_iou3d_poly_push(poly, b.corner[k]);
        if (lc_iou3d_obb_holds(b, a.corner[k])) lc_iou3d_poly_push(poly, a.corner[k]);
    }
    const int n = poly.n;
    if (count) *count = n;

    lc_iou3d_pt mean = poly.sum;
    mean.x /= n;
    mean.y /= n;

    // bubble sort, ascending bearing about the mean; a pair is exchanged only on a strict `>`
    for (int pass = 0; pass + 1 < n; pass++) {
        for (int k = 0; k + 1 < n - pass; k++) {
            const lc_iou3d_pt lo = room[k * stride], hi = room[(k + 1) * stride];
            if (lc_iou3d_bearing(lo, mean) > lc_iou3d_bearing(hi, mean)) {
                room[k * stride] = hi;
                room[(k + 1) * stride] = lo;
            }
        }
    }

    // twice the signed area: the fan of triangles (point 0, point k, point k + 1)
    float twice = 0;
    for (int k = 0; k + 1 < n; k++) {
        const lc_iou3d_pt apex = room[0], u = room[k * stride], v = room[(k + 1) * stride];
        const float ux = u.x - apex.x, uy = u.y - apex.y, vx = v.x - apex.x, vy = v.y - apex.y;
        twice += ux * vy - uy * vx;
    }
    return fabsf(twice) / 2;
}

LC_IOU3D_HD static inline float lc_iou3d_iou_bev(const float* row_a, const float* row_b, lc_iou3d_pt* room, int stride) {
    const float area_a = row_a[3] * row_a[4], area_b = row_b[3] * row_b[4];
    const float inter = lc_iou3d_box_overlap(row_a, row_b, room, stride, 0);
    return inter / fmaxf(area_a + area_b - inter, LC_IOU3D_EPS);
}

// length of the overlap of the intervals of size da about ca and of size db about cb, 0 when they are apart
LC_IOU3D_HD static inline float lc_iou3d_span_overlap(float ca, float da, float cb, float db) {
    const float from = fmaxf(ca - da / 2, cb - db / 2), to = fminf(ca + da / 2, cb + db / 2);
    return fmaxf(to - from, 0.f);
}

// The IoU of the axis-aligned extents: the heading is not read.
LC_IOU3D_HD static inline float lc_iou3d_iou_normal(const float* row_a, const float* row_b) {
    const float inter = lc_iou3d_span_overlap(row_a[0], row_a[3], row_b[0], row_b[3]) *
                        lc_iou3d_span_overlap(row_a[1], row_a[4], row_b[1], row_b[4]);
    const float area_a = row_a[3] * row_a[4], area_b = row_b[3] * row_b[4];
    return inter / fmaxf(area_a + area_b - inter, LC_IOU3D_EPS);
}

#endif  // LC_IOU3D_BOX_H
