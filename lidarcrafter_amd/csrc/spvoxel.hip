// Point <-> voxel exchanges of the Frechet Point-Voxel Distance: what the reference's SPVCNN
// (lidargen/metrics/models/spvcnn/model.py, models/ts/utils.py) takes from torchsparse 1.4.0 as sphashquery,
// calc_ti_weights, spdevoxelize and spvoxelize.  Three gather / scatter passes bound by memory, no MFMA, no atomics.
//   spv_query_kernel    one thread per point p = (x, y, z, batch) float: base = floor(p / s) * s (s a power of two: exact),
//                       the eight probes base + {0, s}^3 with z fastest (k = 4 ix + 2 iy + iz, the order of kind 1 of
//                       sp_map_kernel) in the level's coordinate hash, every component tested against
//                       [0, LC_SPCONV_MAX_COORD] before a key is formed (spconv_hash.h), and the trilinear weights in the
//                       same pass: a = (base + s) - p on an axis whose offset is 0, p - base where it is s,
//                       w_k = (a_x a_y) a_z, / s^3, 0 where the probe is absent, / (sum_k w_k + 1e-8) with the sum taken
//                       in ascending k, one addition after the other.  Every product, sum and quotient is a single
//                       rounded operation (__fmul_rn ...): nothing is contracted or reordered.  A point reads 16 bytes and
//                       writes 2 x 32: its 8 probes are independent loads in flight together.
//   spv_devox_kernel    out[i, :] = (sum_k w[i, k] F[idx[i, k], :]) + addend[i, :].  C / 4 lanes per point, each one quad
//                       of the row: 128-bit loads and stores.  The block's idx / w entries are read once, coalesced, into
//                       LDS (an entry outside [0, n_rows) becomes -1 there); a lane issues its eight row loads, then
//                       accumulates acc = fma(w_k, F_k, acc) in ascending k over the present entries (an absent one reads
//                       nothing and adds nothing), then adds the addend.  The addend may be `out` itself: a lane reads the
//                       quad it writes.
//   spv_vox_kernel      out[v, :] = sum_j F[perm[j], :] / count, j = offsets[v] .. offsets[v + 1] - 1 ascending (perm: the
//                       points in voxel order, within a voxel in ascending point order), count = the number of them, every
//                       term divided and then added, acc = acc + F / count from 0.  One lane per (voxel, channel), so a
//                       wave holds 64 / C voxels (C = 16: 4), one voxel at C = 64, half of one at C = 128, and a block is
//                       one wave: a voxel of hundreds of points holds up at most 64 / C - 1 others, never a block's
//                       worth.  Four rows are in flight per lane; a row is read as C consecutive floats by C lanes.
#include "common.h"
#include "spconv_hash.h"

namespace {

__global__ __launch_bounds__(256) void spv_query_kernel(const float* __restrict__ pts, int N, float s, float inv_s,
                                                       float inv_s3, int si,
                                                       const unsigned long long* __restrict__ keys,
                                                       const int32_t* __restrict__ vals, unsigned cap, int n_table,
                                                       int32_t* __restrict__ idx, float* __restrict__ w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const f32x4 p = *reinterpret_cast<const f32x4*>(pts + (size_t)4 * i);
    float pf[3], a0[3], a1[3];
    bool ok = p[3] >= 0.f && p[3] <= (float)LC_SPCONV_MAX_BATCH;          // (a NaN fails every comparison)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        pf[d] = __fmul_rn(floorf(__fmul_rn(p[d], inv_s)), s);
        a0[d] = __fsub_rn(__fadd_rn(pf[d], s), p[d]);
        a1[d] = __fsub_rn(p[d], pf[d]);
        ok = ok && pf[d] >= 0.f && pf[d] <= (float)LC_SPCONV_MAX_COORD;
    }
    const int b = ok ? (int)p[3] : -1, bx = ok ? (int)pf[0] : -1, by = ok ? (int)pf[1] : -1, bz = ok ? (int)pf[2] : -1;
    int r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int v = -1;
        if (ok) v = sp_find(keys, vals, cap, b, bx + (k >> 2) * si, by + ((k >> 1) & 1) * si, bz + (k & 1) * si);
        r[k] = (v >= 0 && v < n_table) ? v : -1;
    }
    int4* io = reinterpret_cast<int4*>(idx + (size_t)8 * i);
    io[0] = make_int4(r[0], r[1], r[2], r[3]);
    io[1] = make_int4(r[4], r[5], r[6], r[7]);
    if (!w) return;
    float wk[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float ax = (k >> 2) ? a1[0] : a0[0], ay = ((k >> 1) & 1) ? a1[1] : a0[1], az = (k & 1) ? a1[2] : a0[2];
        wk[k] = r[k] >= 0 ? __fmul_rn(__fmul_rn(__fmul_rn(ax, ay), az), inv_s3) : 0.f;
    }
    float sum = wk[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) sum = __fadd_rn(sum, wk[k]);
    const float den = __fadd_rn(sum, 1e-8f);
    f32x4* wo = reinterpret_cast<f32x4*>(w + (size_t)8 * i);
    wo[0] = f32x4{__fdiv_rn(wk[0], den), __fdiv_rn(wk[1], den), __fdiv_rn(wk[2], den), __fdiv_rn(wk[3], den)};
    wo[1] = f32x4{__fdiv_rn(wk[4], den), __fdiv_rn(wk[5], den), __fdiv_rn(wk[6], den), __fdiv_rn(wk[7], den)};
}

// (min. 8 waves per SIMD: the kernel needs 42 VGPRs; left to itself the compiler spends 200 and halves a memory-bound
// pass's waves in flight to 2 per SIMD)
template <int LPP>   // lanes per point = C / 4
__global__ __launch_bounds__(256, 8) void spv_devox_kernel(const float* __restrict__ f, long long ldf, int n_rows,
                                                       const int32_t* __restrict__ idx, const float* __restrict__ w,
                                                       const float* addend, long long lda, float* out, long long ldo,
                                                       int N) {
    constexpr int PPB = 256 / LPP;            // points per block
    __shared__ int sidx[PPB * 8];
    __shared__ float sw[PPB * 8];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * PPB;
    for (int e = tid; e < PPB * 8; e += 256) {
        const long long g = p0 * 8 + e;
        int v = -1;
        float ww = 0.f;
        if (g < (long long)N * 8) {
            v = idx[g];
            ww = w[g];
            if (v < 0 || v >= n_rows) v = -1;
        }
        sidx[e] = v;
        sw[e] = ww;
    }
    __syncthreads();
    const int pl = tid / LPP, q = tid - pl * LPP;
    const long long i = p0 + pl;
    if (pl >= PPB || i >= N) return;
    f32x4 row[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int v = sidx[pl * 8 + k];
        row[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (v >= 0) row[k] = *reinterpret_cast<const f32x4*>(f + (size_t)v * ldf + 4 * q);
    }
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (sidx[pl * 8 + k] >= 0) {
            const float wk = sw[pl * 8 + k];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(wk, row[k][c], acc[c]);
        }
    }
    if (addend) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(addend + (size_t)i * lda + 4 * q);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], a[c]);
    }
    *reinterpret_cast<f32x4*>(out + (size_t)i * ldo + 4 * q) = acc;
}

template <int C>
__global__ __launch_bounds__(64) void spv_vox_kernel(const float* __restrict__ f, long long ldf, int n_rows,
                                                    const int32_t* __restrict__ perm, int n_perm,
                                                    const int32_t* __restrict__ offsets, int V, float* __restrict__ out,
                                                    long long ldo) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long v = t / C;
    const int c = (int)(t - v * C);
    if (v >= V) return;
    int lo = offsets[v], hi = offsets[v + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_perm ? n_perm : hi;
    const float cnt = (float)(hi - lo);
    float acc = 0.f;
    for (int j = lo; j < hi; j += 4) {
        float x[4];
        bool has[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            has[u] = false;
            x[u] = 0.f;
            if (j + u < hi) {
                const int r = perm[j + u];
                has[u] = r >= 0 && r < n_rows;
                if (has[u]) x[u] = f[(size_t)r * ldf + c];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (has[u]) acc = __fadd_rn(acc, __fdiv_rn(x[u], cnt));
    }
    out[(size_t)v * ldo + c] = acc;
}

}  // namespace

extern "C" int lc_spvox_query(const float* pts, int N, int stride, const void* table, int n_table, int32_t* idx, float* w,
                              lc_stream_t s) {
    if (!pts || !table || !idx || N < 1 || n_table < 1 || stride < 1) return LC_EINVAL;
    if (N > LC_SPCONV_MAX_ROWS || n_table > LC_SPCONV_MAX_ROWS || stride > LC_SPCONV_MAX_STRIDE) return LC_EUNSUP;
    if (stride & (stride - 1)) return LC_EUNSUP;                       // floor(p / s) * s is exact for a power of two only
    if (!lc_aligned16(pts) || !lc_aligned16(idx) || (w && !lc_aligned16(w))) return LC_EUNSUP;
    const unsigned cap = sp_capacity(n_table);
    const unsigned long long* keys = static_cast<const unsigned long long*>(table);
    const int32_t* vals = reinterpret_cast<const int32_t*>(keys + cap);
    const float fs = (float)stride, inv = 1.0f / fs;
    hipLaunchKernelGGL(spv_query_kernel, dim3((N + 255) / 256), dim3(256), 0, lc_s(s), pts, N, fs, inv, inv * inv * inv,
                       stride, keys, vals, cap, n_table, idx, w);
    return lc_launch_status();
}

extern "C" int lc_spvox_devoxelize(const float* f, int64_t ldf, int n_rows, const int32_t* idx, const float* w,
                                   const float* addend, int64_t lda, float* out, int64_t ldo, int N, int C,
                                   lc_stream_t s) {
    if (!f || !idx || !w || !out || N < 1 || n_rows < 1 || C < 1) return LC_EINVAL;
    if (C != 16 && C != 48 && C != 64 && C != 128) return LC_EUNSUP;
    if (N > LC_SPCONV_MAX_ROWS || n_rows > LC_SPCONV_MAX_ROWS) return LC_EUNSUP;
    if (ldf < C || ldo < C || (addend && lda < C)) return LC_EINVAL;
    if ((ldf & 3) || (ldo & 3) || (addend && (lda & 3))) return LC_EUNSUP;                  // rows are read and written as quads
    if (!lc_aligned16(f) || !lc_aligned16(out) || (addend && !lc_aligned16(addend))) return LC_EUNSUP;
#define SPV_DEVOX(LPP)                                                                                               \
    hipLaunchKernelGGL(spv_devox_kernel<LPP>, dim3((unsigned)((N + (256 / LPP) - 1) / (256 / LPP))), dim3(256), 0,  \
                       lc_s(s), f, (long long)ldf, n_rows, idx, w, addend, (long long)lda, out, (long long)ldo, N)
    switch (C) {
        case 16: SPV_DEVOX(4); break;
        case 48: SPV_DEVOX(12); break;
        case 64: SPV_DEVOX(16); break;
        default: SPV_DEVOX(32); break;
    }
#undef SPV_DEVOX
    return lc_launch_status();
}

extern "C" int lc_spvox_voxelize(const float* f, int64_t ldf, int n_rows, const int32_t* perm, int n_perm,
                                 const int32_t* offsets, int V, float* out, int64_t ldo, int C, lc_stream_t s) {
    if (!f || !perm || !offsets || !out || V < 1 || n_rows < 1 || n_perm < 1 || C < 1) return LC_EINVAL;
    if (C != 4 && C != 16 && C != 64 && C != 128) return LC_EUNSUP;
    if (V > LC_SPCONV_MAX_ROWS || n_rows > LC_SPCONV_MAX_ROWS || n_perm > LC_SPCONV_MAX_ROWS) return LC_EUNSUP;
    if (ldf < C || ldo < C) return LC_EINVAL;
    const unsigned blocks = (unsigned)(((long long)V * C + 63) / 64);
#define SPV_VOX(CC)                                                                                                  \
    hipLaunchKernelGGL(spv_vox_kernel<CC>, dim3(blocks), dim3(64), 0, lc_s(s), f, (long long)ldf, n_rows, perm, n_perm, \
                       offsets, V, out, (long long)ldo)
    switch (C) {
        case 4: SPV_VOX(4); break;
        case 16: SPV_VOX(16); break;
        case 64: SPV_VOX(64); break;
        default: SPV_VOX(128); break;
    }
#undef SPV_VOX
    return lc_launch_status();
}
