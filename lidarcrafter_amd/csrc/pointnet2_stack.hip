// lidargen.ops.pointnet2.pointnet2_stack: the ragged-batch set-abstraction operators.  Tensors are
// contiguous float32 / int32, clouds are rows start_b .. start_b + n_b - 1 of a stacked [N, .] tensor, the counts live in
// DEVICE memory.  No float atomics, every sum in a fixed order, a cloud's bits do not depend on the batch it is in.
//
//   pn2_scan_kernel      once per call: the exclusive scans of the two count vectors (clamped into their totals, so that no
//       offset leaves its tensor whatever the counts say) and the cloud of every row of the second ("query") side, -1 for a
//       row the counts do not cover.  No other kernel adds counts up.
//   pn2_ball_query_kernel   one wave per centre: 64 lanes test 64 consecutive points of the centre's cloud, a ballot and a
//       prefix popcount keep the hits in ascending index order, the wave stops at nsample hits; the rest of the row is the
//       first hit, an empty ball is [-1, 0, 0, ...].  d < r2 strictly, d = lc_dist2 (common.h: the project's expression).
//   pn2_group_kernel   out[m, c, s] = features[start + idx[m, s], c], zero for an index outside its cloud (forward only).
//   pn2_three_nn_kernel, pn2_interp_kernel, pn2_interp_bwd_kernel   three nearest known points in ascending (distance,
//       index) with strict <; out = (w0 f0 + w1 f1) + w2 f2, each operation rounded; the backward pass reads an inverse
//       table (the stable sort of the indices, built by the caller) and adds every row's terms in ascending (n, j) order.
//   pn2_voxel_query_kernel   the (dz, dy, dx)-ascending walk over point_indices [B, Z, Y, X], d <= r2.
//   Pn2GatherSrc   y [Co, M nsample] = relu(W G + bias), G the grouped operand of QueryAndGroup: the dense engine's kernel
//       (dense_f32.h df_conv_kernel) with the pointwise geometry and epilogue (dense_pointwise.h), as lc_pointmlp_conv_fwd
//       runs it, and this operand source in place of the image's: a block resolves its columns to (point row, centre)
//       pairs in LDS and fills each chunk's tile from the point-major rows.  One kernel body, so the bits are those of
//       lc_pointmlp_conv_fwd on the materialised tensor.
#include "dense_pointwise.h"

namespace {

// scratch: [0 .. B] offsets of side a, [B + 1 .. 2 B + 1] offsets of side b, then the cloud of every one of the Mb rows
__global__ __launch_bounds__(256) void pn2_scan_kernel(const int* __restrict__ cnt_a, const int* __restrict__ cnt_b, int B,
                                                       int Na, int Mb, int* __restrict__ scratch) {
    int* oa = scratch;
    int* ob = scratch + (B + 1);
    int* bid = scratch + 2 * (B + 1);
    if (threadIdx.x == 0) {
        long long sa = 0, sb = 0;
        oa[0] = 0;
        ob[0] = 0;
        for (int b = 0; b < B; ++b) {
            const int ca = cnt_a[b], cb = cnt_b[b];
            sa += ca > 0 ? ca : 0;
            sb += cb > 0 ? cb : 0;
            sa = sa < Na ? sa : Na;
            sb = sb < Mb ? sb : Mb;
            oa[b + 1] = (int)sa;
            ob[b + 1] = (int)sb;
        }
    }
    __syncthreads();
    for (int b = 0; b < B; ++b)
        for (int m = ob[b] + threadIdx.x; m < ob[b + 1]; m += 256) bid[m] = b;
    for (int m = ob[B] + threadIdx.x; m < Mb; m += 256) bid[m] = -1;
}

int pn2_scan(const int* cnt_a, const int* cnt_b, int B, int Na, int Mb, int* scratch, lc_stream_t s) {
    hipLaunchKernelGGL(pn2_scan_kernel, dim3(1), dim3(256), 0, lc_s(s), cnt_a, cnt_b, B, Na, Mb, scratch);
    return lc_launch_status();
}

// ---- ball query ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pn2_ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                             const int* __restrict__ scratch, int* __restrict__ idx, int B,
                                                             int M, float r2, int nsample) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;                       // no barrier below
    int* row = idx + (size_t)m * nsample;
    const int b = scratch[2 * (B + 1) + m];
    int cnt = 0, first = -1;
    if (b >= 0) {
        const int start = scratch[b], n = scratch[b + 1] - start;
        const float* p = xyz + (size_t)start * 3;
        const float cx = new_xyz[3 * (size_t)m], cy = new_xyz[3 * (size_t)m + 1], cz = new_xyz[3 * (size_t)m + 2];
        for (int k0 = 0; k0 < n && cnt < nsample; k0 += 64) {
            const int k = k0 + lane;
            bool hit = false;
            if (k < n) hit = lc_dist2(cx, cy, cz, p[3 * k], p[3 * k + 1], p[3 * k + 2]) < r2;
            const unsigned long long mask = __ballot(hit);
            if (mask == 0ull) continue;
            if (first < 0) first = k0 + (int)__builtin_ctzll(mask);
            const int slot = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            if (hit && slot < nsample) row[slot] = k;
            cnt += (int)__popcll(mask);
        }
        cnt = cnt < nsample ? cnt : nsample;
    }
    if (cnt == 0) {
        for (int l = lane; l < nsample; l += 64) row[l] = l == 0 ? -1 : 0;
    } else {
        for (int l = cnt + lane; l < nsample; l += 64) row[l] = first;
    }
}

// ---- grouping --------------------------------------------------------------------------------------------------------
// one thread per (m, c, s), s fastest
__global__ __launch_bounds__(256) void pn2_group_kernel(const float* __restrict__ features, const int* __restrict__ idx,
                                                        const int* __restrict__ scratch, float* __restrict__ out, int B, int C,
                                                        int nsample, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int s = (int)(t % nsample);
    const long long mc = t / nsample;
    const int m = (int)(mc / C), c = (int)(mc - (long long)m * C);
    const int b = scratch[2 * (B + 1) + m];
    float v = 0.f;
    if (b >= 0) {
        const int start = scratch[b], n = scratch[b + 1] - start;
        const int i = idx[(size_t)m * nsample + s];
        if (i >= 0 && i < n) v = features[(size_t)(start + i) * C + c];
    }
    out[t] = v;
}

// ---- three nearest neighbours and interpolation ----------------------------------------------------------------------
// side a: known, side b: unknown.  One thread per unknown point.
__global__ __launch_bounds__(256) void pn2_three_nn_kernel(const float* __restrict__ unknown, const float* __restrict__ known,
                                                           const int* __restrict__ scratch, float* __restrict__ dist2,
                                                           int* __restrict__ idx, int B, int N) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const int b = scratch[2 * (B + 1) + t];
    const float inf = __builtin_inff();
    float b1 = inf, b2 = inf, b3 = inf;
    int i1 = 0, i2 = 0, i3 = 0, start = 0;
    if (b >= 0) {
        start = scratch[b];
        const int n = scratch[b + 1] - start;
        const float* p = known + (size_t)start * 3;
        const float ux = unknown[3 * (size_t)t], uy = unknown[3 * (size_t)t + 1], uz = unknown[3 * (size_t)t + 2];
        for (int k = 0; k < n; ++k) {
            const float d = lc_dist2(ux, uy, uz, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
            if (d < b1) {
                b3 = b2, i3 = i2;
                b2 = b1, i2 = i1;
                b1 = d, i1 = k;
            } else if (d < b2) {
                b3 = b2, i3 = i2;
                b2 = d, i2 = k;
            } else if (d < b3) {
                b3 = d, i3 = k;
            }
        }
    }
    dist2[3 * (size_t)t] = b1, dist2[3 * (size_t)t + 1] = b2, dist2[3 * (size_t)t + 2] = b3;
    idx[3 * (size_t)t] = i1 + start, idx[3 * (size_t)t + 1] = i2 + start, idx[3 * (size_t)t + 2] = i3 + start;
}

// one thread per (n, c)
__global__ __launch_bounds__(256) void pn2_interp_kernel(const float* __restrict__ features, const int* __restrict__ idx,
                                                         const float* __restrict__ weight, float* __restrict__ out, int C, int M,
                                                         long long total) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long n = t / C;
    const int c = (int)(t - n * C);
    float term[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = idx[3 * n + j];
        term[j] = (i >= 0 && i < M) ? weight[3 * n + j] * features[(size_t)i * C + c] : 0.f;
    }
    const float s = term[0] + term[1];
    out[t] = s + term[2];
}

// one thread per (m, c): entries order[seg[m] .. seg[m + 1]) (entry e = 3 n + j) in ascending (n, j) order
__global__ __launch_bounds__(256) void pn2_interp_bwd_kernel(const float* __restrict__ grad_out, const int* __restrict__ order,
                                                             const int* __restrict__ seg, const float* __restrict__ weight,
                                                             float* __restrict__ grad_features, int C, long long entries,
                                                             long long total) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int m = (int)(t / C), c = (int)(t - (long long)m * C);
    long long j0 = seg[m], j1 = seg[m + 1];
    j0 = j0 < 0 ? 0 : j0;
    j1 = j1 > entries ? entries : j1;
    float acc = 0.f;
    for (long long j = j0; j < j1; ++j) {
        const long long e = order[j];
        if (e < 0 || e >= entries) continue;
        const float p = grad_out[(size_t)(e / 3) * C + c] * weight[e];
        acc = acc + p;
    }
    grad_features[t] = acc;
}

// ---- voxel query -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pn2_voxel_query_kernel(const float* __restrict__ new_xyz, const float* __restrict__ xyz,
                                                              const int* __restrict__ new_coords,
                                                              const int* __restrict__ point_indices, int* __restrict__ idx,
                                                              int M, int N, int B, int Z, int Y, int X, int nsample, float r2,
                                                              int zr, int yr, int xr) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    int* row = idx + (size_t)m * nsample;
    const float cx = new_xyz[3 * (size_t)m], cy = new_xyz[3 * (size_t)m + 1], cz = new_xyz[3 * (size_t)m + 2];
    const int* co = new_coords + 4 * (size_t)m;
    const int b = co[0], z0 = co[1], y0 = co[2], x0 = co[3];
    int cnt = 0;
    if (b >= 0 && b < B) {
        for (int dz = -zr; dz <= zr && cnt < nsample; ++dz) {
            const long long z = (long long)z0 + dz;
            if (z < 0 || z >= Z) continue;
            for (int dy = -yr; dy <= yr && cnt < nsample; ++dy) {
                const long long y = (long long)y0 + dy;
                if (y < 0 || y >= Y) continue;
                for (int dx = -xr; dx <= xr && cnt < nsample; ++dx) {
                    const long long x = (long long)x0 + dx;
                    if (x < 0 || x >= X) continue;
                    const int k = point_indices[(((size_t)b * Z + z) * Y + y) * X + x];
                    if (k < 0 || k >= N) continue;
                    const float d = lc_dist2(xyz[3 * (size_t)k], xyz[3 * (size_t)k + 1], xyz[3 * (size_t)k + 2], cx, cy, cz);
                    if (d > r2) continue;
                    if (cnt == 0)
                        for (int l = 0; l < nsample; ++l) row[l] = k;
                    row[cnt++] = k;
                }
            }
        }
    }
    if (cnt == 0) {
        row[0] = -1;
        for (int l = 1; l < nsample; ++l) row[l] = 0;
    }
}

// ---- the gathered first layer ----------------------------------------------------------------------------------------
// The engine's operand source (dense_f32.h) of the grouped operand [C + xo, L], which is never in memory: column
// l = m nsample + s is point idx[m, s] of centre m's cloud, rows 0 .. xo - 1 its coordinates minus the centre's, then its
// features.
struct Pn2GatherSrc {
    const float* xyz;        // [N, 3]
    const float* new_xyz;    // [M, 3]
    const float* features;   // [N, C] or null (C == 0)
    const int* idx;          // [M, nsample], the ball query's rows: idx[m, 0] < 0 marks an empty ball
    const int* scratch;
    int B, C, nsample, xo, vec4;              // xo: 3 coordinate rows in front of the features, or 0
    long long L;

    template <class G>
    struct Stage {
        static constexpr int KC = G::KC, CS = DfTile<G>::CS, TWB = DfTile<G>::TWB;
        static constexpr bool LDS_SETUP = true;
        const Pn2GatherSrc* a;

        // per column of the block: [0] its global point row, -1: it reads none; [1] its centre, -1: the whole column is zero
        __device__ __forceinline__ static int* tables() {
            __shared__ int t[2][TWB];
            return t[0];
        }
        __device__ __forceinline__ void setup(const Pn2GatherSrc& src, const DfArgs&, int, int p0, int) {
            a = &src;
            int* const s_row = tables(), * const s_ctr = s_row + TWB;
            for (int c = threadIdx.x; c < TWB; c += 256) {
                const long long col = (long long)p0 + c;
                int row = -1, ctr = -1;
                if (col < a->L) {
                    const int m = (int)(col / a->nsample);
                    const int b = a->scratch[2 * (a->B + 1) + m];
                    if (b >= 0 && a->idx[(size_t)m * a->nsample] >= 0) {
                        const int start = a->scratch[b], n = a->scratch[b + 1] - start;
                        const int i = a->idx[col];
                        ctr = m;
                        if (i >= 0 && i < n) row = start + i;
                    }
                }
                s_row[c] = row;
                s_ctr[c] = ctr;
            }
        }
        __device__ __forceinline__ void fill(float* tile, int chunk) const {
            const int tid = threadIdx.x, xo = a->xo;
            const int* const s_row = tables(), * const s_ctr = s_row + TWB;
            if (chunk == 0 && xo) {
                for (int t = tid; t < 3 * TWB; t += 256) {
                    const int r = t / TWB, c = t - r * TWB;
                    const int row = s_row[c], ctr = s_ctr[c];
                    float v = 0.f;
                    if (ctr >= 0) v = (row >= 0 ? a->xyz[(size_t)row * 3 + r] : 0.f) - a->new_xyz[(size_t)ctr * 3 + r];
                    tile[r * CS + c] = v;
                }
            }
            // feature quads 4 fq .. 4 fq + 3 that overlap the chunk's channels f_lo .. f_lo + 31 (f = tile channel - xo)
            const int f_lo = chunk * KC - xo;
            const int fq0 = f_lo >= 0 ? f_lo / 4 : -1;
            for (int t = tid; t < 9 * TWB; t += 256) {
                const int qi = t / TWB, c = t - qi * TWB;
                const int f0 = 4 * (fq0 + qi);
                if (f0 + 3 < f_lo || f0 >= f_lo + KC || f0 + 3 < 0) continue;
                const int row = s_ctr[c] >= 0 ? s_row[c] : -1;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (row >= 0) {
                    const float* fp = a->features + (size_t)row * a->C;
                    if (a->vec4 && f0 >= 0 && f0 + 3 < a->C) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(fp + f0);
                        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (f0 + e >= 0 && f0 + e < a->C) v[e] = fp[f0 + e];
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int f = f0 + e, ch = f - f_lo;
                    if (f >= 0 && ch >= 0 && ch < KC) tile[ch * CS + c] = v[e];
                }
            }
        }
        __device__ __forceinline__ void published(int) {}
    };
};

inline unsigned pn2_blocks(long long total) { return (unsigned)((total + 255) / 256); }
inline bool pn2_grid_ok(long long total) { return (total + 255) / 256 <= 2147483647ll; }

}  // namespace

extern "C" int lc_pn2_limit(int which) {
    switch (which) {
        case 0: return LC_PN2_MAX_NSAMPLE;
        case 1: return LC_PN2_MAX_BATCH;
        case 2: return DfTile<PwGeom<1>>::TWB;
        default: return 0;
    }
}

extern "C" int64_t lc_pn2_scratch_elems(int B, int M) {
    if (B < 1 || M < 0) return 0;
    return 2 * ((int64_t)B + 1) + M;
}

#define PN2_CHECK_BATCH(B)                       \
    do {                                         \
        if ((B) < 1) return LC_EINVAL;           \
        if ((B) > LC_PN2_MAX_BATCH) return LC_EUNSUP; \
    } while (0)

extern "C" int lc_pn2_ball_query_fwd(const float* xyz, const int* xyz_cnt, const float* new_xyz, const int* new_cnt, int* idx,
                                     int* scratch, int B, int N, int M, float radius, int nsample, lc_stream_t s) {
    PN2_CHECK_BATCH(B);
    if (N < 0 || M < 0 || nsample < 1 || !(radius >= 0.f)) return LC_EINVAL;
    if (nsample > LC_PN2_MAX_NSAMPLE) return LC_EUNSUP;
    if (M == 0) return LC_OK;
    if (!xyz_cnt || !new_xyz || !new_cnt || !idx || !scratch || (N > 0 && !xyz)) return LC_EINVAL;
    if (N > 715827882 || M > 715827882) return LC_EUNSUP;          // 3 k stays an int
    int e = pn2_scan(xyz_cnt, new_cnt, B, N, M, scratch, s);
    if (e != LC_OK) return e;
    const float r2 = radius * radius;
    hipLaunchKernelGGL(pn2_ball_query_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, lc_s(s), xyz, new_xyz, scratch, idx, B,
                       M, r2, nsample);
    return lc_launch_status();
}

extern "C" int lc_pn2_group_fwd(const float* features, const int* features_cnt, const int* idx, const int* idx_cnt, float* out,
                                int* scratch, int B, int N, int C, int M, int nsample, lc_stream_t s) {
    PN2_CHECK_BATCH(B);
    if (N < 0 || M < 0 || C < 1 || nsample < 1) return LC_EINVAL;
    if (M == 0) return LC_OK;
    if (!features_cnt || !idx || !idx_cnt || !out || !scratch || (N > 0 && !features)) return LC_EINVAL;
    const long long total = (long long)M * C * nsample;
    if (!pn2_grid_ok(total)) return LC_EUNSUP;
    int e = pn2_scan(features_cnt, idx_cnt, B, N, M, scratch, s);
    if (e != LC_OK) return e;
    hipLaunchKernelGGL(pn2_group_kernel, dim3(pn2_blocks(total)), dim3(256), 0, lc_s(s), features, idx, scratch, out, B, C,
                       nsample, total);
    return lc_launch_status();
}

extern "C" int lc_pn2_three_nn_fwd(const float* unknown, const int* unknown_cnt, const float* known, const int* known_cnt,
                                   float* dist2, int* idx, int* scratch, int B, int N, int M, lc_stream_t s) {
    PN2_CHECK_BATCH(B);
    if (N < 0 || M < 0) return LC_EINVAL;
    if (N == 0) return LC_OK;
    if (!unknown || !unknown_cnt || !known_cnt || !dist2 || !idx || !scratch || (M > 0 && !known)) return LC_EINVAL;
    if (N > 715827882 || M > 715827882) return LC_EUNSUP;
    int e = pn2_scan(known_cnt, unknown_cnt, B, M, N, scratch, s);
    if (e != LC_OK) return e;
    hipLaunchKernelGGL(pn2_three_nn_kernel, dim3(pn2_blocks(N)), dim3(256), 0, lc_s(s), unknown, known, scratch, dist2, idx, B, N);
    return lc_launch_status();
}

extern "C" int lc_pn2_three_interpolate_fwd(const float* features, const int* idx, const float* weight, float* out, int N, int C,
                                            int M, lc_stream_t s) {
    if (N < 0 || M < 0 || C < 1) return LC_EINVAL;
    if (N == 0) return LC_OK;
    if (!idx || !weight || !out || (M > 0 && !features)) return LC_EINVAL;
    const long long total = (long long)N * C;
    if (!pn2_grid_ok(total)) return LC_EUNSUP;
    hipLaunchKernelGGL(pn2_interp_kernel, dim3(pn2_blocks(total)), dim3(256), 0, lc_s(s), features, idx, weight, out, C, M, total);
    return lc_launch_status();
}

extern "C" int lc_pn2_three_interpolate_bwd(const float* grad_out, const int* order, const int* seg, const float* weight,
                                            float* grad_features, int N, int C, int M, lc_stream_t s) {
    if (N < 0 || M < 0 || C < 1) return LC_EINVAL;
    if (M == 0) return LC_OK;
    if (!seg || !grad_features || (N > 0 && (!grad_out || !order || !weight))) return LC_EINVAL;
    const long long entries = 3ll * N, total = (long long)M * C;
    if (entries > 2147483647ll || !pn2_grid_ok(total)) return LC_EUNSUP;
    hipLaunchKernelGGL(pn2_interp_bwd_kernel, dim3(pn2_blocks(total)), dim3(256), 0, lc_s(s), grad_out, order, seg, weight,
                       grad_features, C, entries, total);
    return lc_launch_status();
}

extern "C" int lc_pn2_voxel_query_fwd(const float* new_xyz, const float* xyz, const int* new_coords, const int* point_indices,
                                      int* idx, int M, int N, int B, int Z, int Y, int X, int nsample, float radius, int z_range,
                                      int y_range, int x_range, lc_stream_t s) {
    if (M < 0 || N < 0 || B < 1 || Z < 1 || Y < 1 || X < 1 || nsample < 1 || !(radius >= 0.f) || z_range < 0 || y_range < 0 ||
        x_range < 0)
        return LC_EINVAL;
    if (nsample > LC_PN2_MAX_NSAMPLE || z_range > 1024 || y_range > 1024 || x_range > 1024) return LC_EUNSUP;
    if (M == 0) return LC_OK;
    if (!new_xyz || !new_coords || !point_indices || !idx || (N > 0 && !xyz)) return LC_EINVAL;
    const float r2 = radius * radius;
    hipLaunchKernelGGL(pn2_voxel_query_kernel, dim3(pn2_blocks(M)), dim3(256), 0, lc_s(s), new_xyz, xyz, new_coords,
                       point_indices, idx, M, N, B, Z, Y, X, nsample, r2, z_range, y_range, x_range);
    return lc_launch_status();
}

extern "C" int lc_pn2_sa_first_fwd(const float* xyz, const int* xyz_cnt, const float* new_xyz, const int* new_cnt,
                                   const float* features, const int* idx, const float* wpk, const float* bias, float* y,
                                   int* scratch, int B, int N, int M, int C, int Co, int nsample, int use_xyz, lc_stream_t s) {
    PN2_CHECK_BATCH(B);
    if (N < 0 || M < 0 || C < 0 || Co < 1 || nsample < 1 || (C == 0 && !use_xyz)) return LC_EINVAL;
    if (nsample > LC_PN2_MAX_NSAMPLE) return LC_EUNSUP;
    if (M == 0) return LC_OK;
    if (!xyz_cnt || !new_xyz || !new_cnt || !idx || !wpk || !bias || !y || !scratch) return LC_EINVAL;
    if (N > 0 && (!xyz || (C > 0 && !features))) return LC_EINVAL;
    if (!lc_aligned16(wpk)) return LC_EUNSUP;
    const long long L = (long long)M * nsample;
    if (L > 2147483647ll || N > 715827882) return LC_EUNSUP;
    int e = pn2_scan(xyz_cnt, new_cnt, B, N, M, scratch, s);
    if (e != LC_OK) return e;
    const int xo = use_xyz ? 3 : 0, vec4 = (C % 4 == 0 && lc_aligned16(features)) ? 1 : 0;
    const Pn2GatherSrc src{xyz, new_xyz, features, idx, scratch, B, C, nsample, xo, vec4, L};
    // the pointwise layer on [1, C + xo, L]: relu, no residual
    const DfArgs a{nullptr, wpk, C + xo, Co, 1, (int)L, (int)L, 1};
    return df_dispatch<PwGeom>(a, PwEpi{bias, nullptr, y, 1}, 1, L, s, src);
}
