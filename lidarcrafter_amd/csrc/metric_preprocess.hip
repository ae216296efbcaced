// The step in front of the three learned scores' networks (FRID, FSVD, FPVD), a ragged batch of clouds at a time
// (DESIGN.md section 5u).  A batch is one contiguous [N, 3] buffer of float32 or float64 points and int32 offsets [B + 1];
// the cloud of point i is found by a binary search of the offsets.
//   range images   lidargen/metrics/metric_utils.py pcd2range + range2xyz (preprocess_range) -> float32 [B, 4, H, W].
//     Per point the host's expressions in the host's order in float64 (a float32 point is widened first: the contract of
//     the device route), the depth rounded to float32, an integer atomicMin on its bit pattern (positive floats order as
//     their bits): the nearest point wins whatever the order, no float atomics, the same bits every run.  Per pixel then
//     the depth (or -1) and the back-projection float32(dir64 * double(depth32)) under range2xyz's own mask, which numpy
//     evaluates in float32 on a float32 image.
//   voxels         preprocess_pcd + pcd2voxel + sparse_collate -> (feats [n, 4], coords [n, 4], offsets [B + 1]).
//     Depth filter and rint(p / voxel) in the cloud's own dtype (IEEE division, round half to even), per-cloud integer
//     minima by integer atomics, ONE stable radix sort of the batch on (cloud, x, y, z) bit fields -- the lexicographic
//     order of (x, y, z) is the order of ravel_hash for any extents, so the key needs neither the minima nor the extents --
//     with the point index as the value: a run's head is the voxel's smallest original index, np.unique's first
//     occurrence.  Filtered points carry cloud index B and sort behind everything.
#include <climits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"

namespace {

#pragma clang fp contract(off)

#define MP_EMPTY 0xFFFFFFFFu

// the last b with offsets[b] <= i (empty clouds share an offset with their successor and are skipped); 0 <= result < B
__device__ __forceinline__ int mp_cloud_of(const int* __restrict__ offsets, int B, int i) {
    int lo = 0, hi = B;                      // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- range images ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mp_fill_u32_kernel(unsigned* __restrict__ p, long long n, unsigned v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void mp_range_scatter_kernel(const T* __restrict__ pts, const int* __restrict__ offsets,
                                                              int B, int N, int H, int W, double lo, double hi,
                                                              double fov_down_abs, double fov_range,
                                                              unsigned* __restrict__ zbuf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double x = (double)pts[3ll * i], y = (double)pts[3ll * i + 1], z = (double)pts[3ll * i + 2];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double s = xx + yy;
    const double depth = sqrt(s + zz);                                  // np.linalg.norm: (x^2 + y^2) + z^2
    if (!(depth > lo && depth < hi)) return;
    const double yaw = -atan2(y, x);
    const double pitch = asin(z / depth);
    double px = 0.5 * (yaw / 3.141592653589793 + 1.0);
    const double t = pitch + fov_down_abs;
    double py = 1.0 - t / fov_range;
    px = px * (double)W;
    py = py * (double)H;
    // np.maximum(0, np.minimum(size - 1, np.floor(.))); a NaN never gets here (the mask is false for it)
    const int ix = (int)fmax(0.0, fmin((double)(W - 1), floor(px)));
    const int iy = (int)fmax(0.0, fmin((double)(H - 1), floor(py)));
    const int b = mp_cloud_of(offsets, B, i);
    const float d32 = (float)depth;                                     // proj_range is float32: round to nearest
    atomicMin(zbuf + ((long long)b * H + iy) * W + ix, __float_as_uint(d32));
}

__global__ __launch_bounds__(256) void mp_range_image_kernel(const unsigned* __restrict__ zbuf,
                                                            const double* __restrict__ dir, int B, int HW, float lo32,
                                                            float hi32, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * HW) return;
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    const unsigned bits = zbuf[i];
    const float d = bits == MP_EMPTY ? -1.0f : __uint_as_float(bits);
    float* o = out + (long long)b * 4 * HW + p;
    o[0] = d;
    const bool in = d > lo32 && d < hi32;                               // range2xyz's mask on the float32 image
    const double dd = (double)d;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(long long)(c + 1) * HW] = in ? (float)(dir[(long long)c * HW + p] * dd) : -1.0f;
}

// ---- voxels ------------------------------------------------------------------------------------------------------------
struct VxScratch {
    int* mn; unsigned long long* key_a; unsigned long long* key_b; int* idx_a; int* idx_b; int* head; int* uid;
    void* tmp; size_t tmp_bytes;
};

size_t mp_align256(size_t v) { return (v + 255) / 256 * 256; }

size_t vx_tmp_bytes(int N) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr,
                                    (int*)nullptr, (size_t)N);
    (void)rocprim::exclusive_scan(nullptr, b, (int*)nullptr, (int*)nullptr, 0, (size_t)N, rocprim::plus<int>());
    return a > b ? a : b;
}

size_t vx_carve(void* base, int N, int B, VxScratch* s) {
    char* p = static_cast<char*>(base);
    auto take = [&](size_t bytes) { char* r = p; p += mp_align256(bytes); return (void*)r; };
    void* mn = take((size_t)B * 3 * 4);
    void* ka = take((size_t)N * 8);
    void* kb = take((size_t)N * 8);
    void* ia = take((size_t)N * 4);
    void* ib = take((size_t)N * 4);
    void* hd = take((size_t)N * 4);
    void* ud = take((size_t)N * 4);
    const size_t tb = vx_tmp_bytes(N);
    void* tmp = take(tb);
    if (s) *s = VxScratch{(int*)mn, (unsigned long long*)ka, (unsigned long long*)kb, (int*)ia, (int*)ib, (int*)hd, (int*)ud,
                          tmp, tb};
    return (size_t)(p - static_cast<char*>(base));
}

// bits of the fields of the sort key: [0] the cloud index (0 ... B, B = filtered), [1] one axis (q + R, |q| <= R)
bool vx_key_bits(int B, double hi, double voxel, int* cloud_bits, int* axis_bits, int* R) {
    if (B < 1 || !(hi > 0.0) || !(voxel > 0.0)) return false;
    const double r = ceil(hi / voxel) + 2.0;
    if (!(r < 1073741824.0)) return false;
    int cb = 0, ab = 0;
    while (((long long)B >> cb) != 0) ++cb;
    while (((2ll * (long long)r + 1) >> ab) != 0) ++ab;
    *cloud_bits = cb; *axis_bits = ab; *R = (int)r;
    return true;
}

template <typename T>
__device__ __forceinline__ bool vx_quantize(const T* __restrict__ p, T lo, T hi, T voxel, int q[3]) {
    const T x = p[0], y = p[1], z = p[2];
    const T xx = x * x, yy = y * y, zz = z * z;
    const T s = xx + yy;
    const T depth = sqrt(s + zz);
    if (!(depth > lo && depth < hi)) return false;
    q[0] = (int)rint(x / voxel); q[1] = (int)rint(y / voxel); q[2] = (int)rint(z / voxel);
    return true;
}

__global__ __launch_bounds__(256) void vx_init_kernel(int* __restrict__ mn, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) mn[i] = INT_MAX;
}

template <typename T>
__global__ __launch_bounds__(256) void vx_key_kernel(const T* __restrict__ pts, const int* __restrict__ offsets, int B, int N,
                                                    T lo, T hi, T voxel, int R, int axis_bits, int* __restrict__ mn,
                                                    unsigned long long* __restrict__ key, int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ic = min(i, N - 1);                                       // lanes past the end look on, they keep nothing
    const int b = mp_cloud_of(offsets, B, ic);
    int q[3] = {0, 0, 0};
    const bool keep = i < N && vx_quantize(pts + 3ll * ic, lo, hi, voxel, q);
    if (i < N) {
        unsigned long long k = (unsigned long long)(keep ? b : B);
        // |q| <= R by the depth filter; the mask keeps the cloud field what it is whatever the input
        const unsigned long long m = (1ull << axis_bits) - 1ull;
#pragma unroll
        for (int d = 0; d < 3; ++d) k = (k << axis_bits) | ((unsigned long long)(keep ? q[d] + R : 0) & m);
        key[i] = k;
        idx[i] = i;
    }
    // per-cloud minima: one atomic per wave and axis where the wave lies in one cloud, else one per kept lane
    const bool uniform = __all(b == __shfl(b, 0, 64));
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        int v = keep ? q[d] : INT_MAX;
        if (uniform) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
            if ((threadIdx.x & 63) == 0 && v != INT_MAX) atomicMin(mn + b * 3 + d, v);
        } else if (keep) {
            atomicMin(mn + b * 3 + d, v);
        }
    }
}

__global__ __launch_bounds__(256) void vx_heads_kernel(const unsigned long long* __restrict__ key, int N, int B,
                                                      int cloud_shift, int* __restrict__ head) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long k = key[i];
    head[i] = ((int)(k >> cloud_shift) < B && (i == 0 || k != key[i - 1])) ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(256) void vx_emit_kernel(const T* __restrict__ pts, const unsigned long long* __restrict__ key,
                                                     const int* __restrict__ sidx, const int* __restrict__ head,
                                                     const int* __restrict__ uid, const int* __restrict__ mn, int N, int B,
                                                     int R, int axis_bits, float* __restrict__ feats,
                                                     int* __restrict__ coords, int* __restrict__ out_offsets) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long k = key[i];
    const int cloud_shift = 3 * axis_bits;
    const int b = (int)(k >> cloud_shift);                              // 0 ... B
    const int u = uid[i];                                               // unique voxels in front of this element
    const int prev = i == 0 ? -1 : (int)(key[i - 1] >> cloud_shift);
    for (int c = prev + 1; c <= b; ++c) out_offsets[c] = u;             // clouds that begin here (empty ones included)
    if (i == N - 1)
        for (int c = b + 1; c <= B; ++c) out_offsets[c] = u + head[i];
    if (!head[i]) return;
    const unsigned long long m = (1ull << axis_bits) - 1ull;
    const int src = sidx[i];
    const T* p = pts + 3ll * src;
    float* f = feats + 4ll * u;
    int* c4 = coords + 4ll * u;
    f[0] = (float)p[0]; f[1] = (float)p[1]; f[2] = (float)p[2]; f[3] = -1.0f;
    c4[0] = (int)((k >> (2 * axis_bits)) & m) - R - mn[b * 3];
    c4[1] = (int)((k >> axis_bits) & m) - R - mn[b * 3 + 1];
    c4[2] = (int)(k & m) - R - mn[b * 3 + 2];
    c4[3] = b;
}

template <typename T>
int vx_run(const T* pts, const int* offsets, int B, int N, double lo, double hi, double voxel, int R, int cloud_bits,
           int axis_bits, const VxScratch& w, float* feats, int* coords, int* out_offsets, hipStream_t st) {
    const dim3 g((N + 255) / 256), blk(256);
    hipLaunchKernelGGL(vx_init_kernel, dim3((B * 3 + 255) / 256), blk, 0, st, w.mn, B * 3);
    hipLaunchKernelGGL((vx_key_kernel<T>), g, blk, 0, st, pts, offsets, B, N, (T)lo, (T)hi, (T)voxel, R, axis_bits, w.mn,
                       w.key_a, w.idx_a);
    size_t tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.key_a, w.key_b, w.idx_a, w.idx_b, (size_t)N, 0, cloud_bits + 3 * axis_bits,
                                  st) != hipSuccess)
        return lc_launch_status() ? lc_launch_status() : LC_EUNSUP;
    hipLaunchKernelGGL(vx_heads_kernel, g, blk, 0, st, w.key_b, N, B, 3 * axis_bits, w.head);
    tb = w.tmp_bytes;
    if (rocprim::exclusive_scan(w.tmp, tb, w.head, w.uid, 0, (size_t)N, rocprim::plus<int>(), st) != hipSuccess)
        return lc_launch_status() ? lc_launch_status() : LC_EUNSUP;
    hipLaunchKernelGGL((vx_emit_kernel<T>), g, blk, 0, st, pts, w.key_b, w.idx_b, w.head, w.uid, w.mn, N, B, R, axis_bits,
                       feats, coords, out_offsets);
    return lc_launch_status();
}

}  // namespace

extern "C" int lc_range_batch_fwd(const void* pts, int is_f64, const int32_t* offsets, int B, int N, int H, int W, double lo,
                                  double hi, float lo32, float hi32, double fov_down_abs, double fov_range,
                                  const double* dir, uint32_t* zbuf, float* out, lc_stream_t s) {
    if ((!pts && N > 0) || !offsets || !dir || !zbuf || !out || B < 1 || N < 0 || H < 1 || W < 1 || !(lo >= 0.0) ||
        !(hi > lo) || !(fov_range > 0.0) || (is_f64 != 0 && is_f64 != 1))
        return LC_EINVAL;
    const long long px = (long long)B * H * W;
    if (px > 0x7FFFFFFFll * 64 || (long long)H * W > 0x7FFFFFFF) return LC_EUNSUP;
    hipStream_t st = lc_s(s);
    const dim3 blk(256), gp((unsigned)((px + 255) / 256));
    hipLaunchKernelGGL(mp_fill_u32_kernel, gp, blk, 0, st, zbuf, px, MP_EMPTY);
    if (N > 0) {
        const dim3 g((N + 255) / 256);
        if (is_f64)
            hipLaunchKernelGGL((mp_range_scatter_kernel<double>), g, blk, 0, st, (const double*)pts, offsets, B, N, H, W, lo,
                               hi, fov_down_abs, fov_range, zbuf);
        else
            hipLaunchKernelGGL((mp_range_scatter_kernel<float>), g, blk, 0, st, (const float*)pts, offsets, B, N, H, W, lo, hi,
                               fov_down_abs, fov_range, zbuf);
    }
    hipLaunchKernelGGL(mp_range_image_kernel, gp, blk, 0, st, zbuf, dir, B, H * W, lo32, hi32, out);
    return lc_launch_status();
}

extern "C" int lc_voxel_batch_key_bits(int B, double hi, double voxel, int32_t* bits) {
    int cb, ab, R;
    if (!bits || !vx_key_bits(B, hi, voxel, &cb, &ab, &R)) return LC_EINVAL;
    bits[0] = cb; bits[1] = 3 * ab;
    return cb + 3 * ab > 64 ? LC_EUNSUP : LC_OK;
}

extern "C" int64_t lc_voxel_batch_scratch_bytes(int N, int B) {
    if (N < 1 || B < 1) return 0;
    return (int64_t)vx_carve(nullptr, N, B, nullptr);
}

extern "C" int lc_voxel_batch_fwd(const void* pts, int is_f64, const int32_t* offsets, int B, int N, double lo, double hi,
                                  double voxel, void* scratch, float* feats, int32_t* coords, int32_t* out_offsets,
                                  lc_stream_t s) {
    int cb, ab, R;
    if (!pts || !offsets || !scratch || !feats || !coords || !out_offsets || N < 1 || !(lo >= 0.0) || !(hi > lo) ||
        (is_f64 != 0 && is_f64 != 1) || !vx_key_bits(B, hi, voxel, &cb, &ab, &R))
        return LC_EINVAL;
    if (cb + 3 * ab > 64) return LC_EUNSUP;
    VxScratch w;
    vx_carve(scratch, N, B, &w);
    if (is_f64)
        return vx_run<double>((const double*)pts, offsets, B, N, lo, hi, voxel, R, cb, ab, w, feats, coords, out_offsets, lc_s(s));
    return vx_run<float>((const float*)pts, offsets, B, N, lo, hi, voxel, R, cb, ab, w, feats, coords, out_offsets, lc_s(s));
}
