// Stand-alone check of csrc/iou3d_box.h on the CPU, meant for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I lidarcrafter_amd/csrc
//       devtools/iou3d_host_check.cpp -o iou3d_host_check && ./iou3d_host_check
// It runs the overlap, the BEV IoU and the unrotated IoU over random rotated pairs, axis-aligned pairs, zero-sized, huge,
// NaN and inf rows -- every pair of a pool of special rows included -- with the 16 points in a heap block of exactly 16
// entries (a 17th write is an AddressSanitizer error) and once more with a stride of 3 in a block of 46.  It checks what
// holds for every input: 0 <= cnt <= 16; and for finite, positive-sized boxes: 0 <= area, IoU of a box with itself 1
// within 1e-4.  Exit status 0 when all of it held.  tests/test_iou3d_host.py builds and runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "iou3d_box.h"

namespace {

uint64_t state = 0x9e3779b97f4a7c15ULL;

double uniform() {   // xorshift64*: no library generator whose stream could differ between builds
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (double)((state * 0x2545f4914f6cdd1dULL) >> 11) / 9007199254740992.0;
}

float range(double lo, double hi) { return (float)(lo + (hi - lo) * uniform()); }

struct Box {
    float v[7];
};

Box random_box() {
    return {{range(-4, 4), range(-4, 4), range(-1, 1), range(0.5, 5), range(0.5, 3), range(1, 2), range(-3.14159265, 3.14159265)}};
}

Box grid_box() {
    return {{std::floor(range(-16, 17)) / 4, std::floor(range(-16, 17)) / 4, 0.f, std::floor(range(1, 11)) / 2,
             std::floor(range(1, 7)) / 2, 1.f, 0.f}};
}

long failures = 0;

void expect(bool ok, const char* what, const Box& a, const Box& b) {
    if (ok) return;
    if (failures++ < 10)
        std::fprintf(stderr, "FAILED %s: a = %g %g %g %g %g %g %g, b = %g %g %g %g %g %g %g\n", what, a.v[0], a.v[1], a.v[2],
                     a.v[3], a.v[4], a.v[5], a.v[6], b.v[0], b.v[1], b.v[2], b.v[3], b.v[4], b.v[5], b.v[6]);
}

void one_pair(const Box& a, const Box& b, bool regular) {
    // exactly 16 points on the heap: one past the end is a sanitizer report
    lc_iou3d_pt* pts = (lc_iou3d_pt*)std::malloc(sizeof(lc_iou3d_pt) * LC_IOU3D_MAX_PTS);
    int cnt = -1;
    const float area = lc_iou3d_box_overlap(a.v, b.v, pts, 1, &cnt);
    const float iou = lc_iou3d_iou_bev(a.v, b.v, pts, 1);
    std::free(pts);
    const int stride = 3;
    lc_iou3d_pt* wide = (lc_iou3d_pt*)std::malloc(sizeof(lc_iou3d_pt) * ((LC_IOU3D_MAX_PTS - 1) * stride + 1));
    int cnt2 = -1;
    const float area2 = lc_iou3d_box_overlap(a.v, b.v, wide, stride, &cnt2);
    std::free(wide);
    const float plain = lc_iou3d_iou_normal(a.v, b.v);
    expect(cnt >= 0 && cnt <= LC_IOU3D_MAX_PTS, "0 <= cnt <= 16", a, b);
    expect(cnt2 == cnt, "the count does not depend on the stride", a, b);
    if (regular) {
        expect(area >= 0.f && std::isfinite(area), "finite area >= 0", a, b);
        expect(area == area2, "the area does not depend on the stride", a, b);
        expect(iou >= 0.f && std::isfinite(iou), "finite IoU >= 0", a, b);
        expect(plain >= 0.f && plain <= 1.0001f, "0 <= unrotated IoU <= 1", a, b);
    }
}

}  // namespace

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    long pairs = 0;
    for (int i = 0; i < 200000; i++, pairs++) one_pair(random_box(), random_box(), true);
    for (int i = 0; i < 50000; i++, pairs++) one_pair(grid_box(), grid_box(), true);
    for (int i = 0; i < 20000; i++, pairs++) {   // a box with itself and with a slightly moved copy
        const Box a = random_box();
        Box b = a;
        lc_iou3d_pt pts[LC_IOU3D_MAX_PTS];
        const float self = lc_iou3d_iou_bev(a.v, a.v, pts, 1);
        expect(std::fabs(self - 1.f) < 1e-4f, "IoU of a box with itself is 1", a, a);
        b.v[0] += range(-1e-3, 1e-3);
        b.v[6] += range(-1e-3, 1e-3);
        one_pair(a, b, true);
    }
    // special rows, every ordered pair of them, and each against random boxes
    std::vector<Box> pool = {
        {{0, 0, 0, 0, 0, 0, 0}},         {{0.5f, 0, 0, 0, 1, 1, 1}},        {{0, 0, 0, 2, 0, 1, -2}},
        {{nan, nan, nan, nan, nan, nan, nan}}, {{inf, inf, inf, inf, inf, inf, inf}}, {{0, 0, 0, inf, 1, 1, 0}},
        {{0, 0, 0, 1, 1, 1, nan}},       {{0, 0, 0, 1, 1, 1, inf}},         {{-inf, 0, 0, 1, 1, 1, 0.5f}},
        {{1e30f, -1e30f, 0, 1e30f, 1e30f, 1, 2}}, {{0, 0, 0, -1, -2, 1, 0.3f}},     {{0, 0, 0, 1e-30f, 1e-30f, 1, 0.1f}},
        {{nan, 0, 0, 2, 1, 1, 0}},       {{0, 0, 0, nan, 1, 1, 0}},         {{0, 0, 0, 3e38f, 3e38f, 1, 0.7f}},
        {{1, -0.5f, 0, 2, 1, 1, 0}},
    };
    for (const Box& a : pool)
        for (const Box& b : pool) {
            one_pair(a, b, false);
            pairs++;
        }
    for (int i = 0; i < 2000; i++)
        for (const Box& s : pool) {
            const Box r = random_box();
            one_pair(s, r, false);
            one_pair(r, s, false);
            pairs += 2;
        }
    std::printf("%ld pairs, %ld failures\n", pairs, failures);
    return failures == 0 ? 0 : 1;
}
