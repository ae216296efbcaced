// PointMLP object extractor: the network behind the evaluator's object scores and CGF
// (lidargen/metrics/extractor/pointmlp.py).  Five kernel families, no atomics anywhere, every reduction in a fixed order,
// a cloud's bits do not depend on the batch it is in:
//
//   pm_fps_kernel<P, LDSXYZ>   farthest point sampling, one block (at most 256 threads) per cloud, P points per thread in
//       registers (coordinates + running distance).  Per pick: d = (dx dx + dy dy) + dz dz with separately rounded
//       operations (common.h lc_dist2: contraction off), running distance = min(d, running), then ONE maximum of a packed 64-bit word
//       (distance bits << 32 | ~tie) through the wave (6 exchanges) and, in blocks of more than one wave, one barrier: the
//       wave maxima go through a double-buffered LDS slot, so the slot of pick j is not written again before every wave has
//       passed the barrier of pick j + 1.  The winner's coordinates are read from an LDS copy of the cloud (N <= 4096) or
//       from global memory.
//       tie = rev(k mod bs) << 4 | k / bs, bs = the largest power of two <= min(N, 1024), rev = the bit reversal over
//       log2 bs bits: among equal maxima the smallest (rev(k mod bs), k) wins -- the order a strided scan with `>` over bs
//       threads (thread t keeps its first maximum) followed by a tree over strides bs/2 .. 1 that keeps the left operand
//       on ties produces: the last level prefers even threads, the one before it threads = 0 mod 4, and so on.
//       Distances are sums of squares (never -0, never NaN for finite input): their bit patterns order like the floats.
//   pm_knn_kernel<NPL> / pm_knn_stream_kernel   one wave per query: packed words (distance bits << 32 | index), K rounds
//       of "the smallest word above the last one taken" -- ascending (distance, index).  N <= 1024: the words live in
//       registers (NPL per lane); above, every round computes them again from global memory.
//   pm_group_stats_kernel / pm_group_apply_kernel   the operand of a stage's `transfer` convolution:
//       rows 0..d-1 alpha (x[idx] - x[anchor]) / (sigma_b + 1e-5) + beta, rows d..2d-1 x[anchor], columns s K + k.
//       sigma_b (unbiased, over all S K d differences of cloud b) is a two-level sum in float64: one (sum, sum of squares)
//       pair per block of 256 columns, then every apply block adds the pairs in the same order.
//   lc_pointmlp_conv_fwd   y = act(W x + b (+ res)) on [B, C, L]: the dense tile engine of dense_f32.h (exact fp32 on
//       v_mfma_f32_32x32x2_f32; the kernel, the packed weights and the k order are RangeNet's 1x1 mode: chunks of 32 input
//       channels summed from zero, then added in ascending order) with the pointwise geometry and epilogue of
//       dense_pointwise.h (PwGeom<CW> / PwEpi), a wave = 32 output channels x 64 columns.  The residual is added BEFORE
//       the activation.  No kernel of this family is defined here.
//   pm_groupmax_kernel   out[b, c, g] = max_k x[b, c, g K + k], out with caller-given strides.
#include "dense_pointwise.h"

namespace {

typedef unsigned long long pm_u64;

__device__ __forceinline__ pm_u64 pm_wave_max(pm_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const pm_u64 w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ pm_u64 pm_wave_min(pm_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const pm_u64 w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// ---- farthest point sampling -----------------------------------------------------------------------------------------
// bit reversal over `bits` bits (an involution); bits == 0: the only value is 0
__device__ __forceinline__ unsigned pm_rev(unsigned v, int bits) { return bits ? __brev(v) >> (32 - bits) : 0u; }

constexpr int FPS_T = 256;                    // threads per block at most
constexpr int FPS_LDS_N = 4096;               // clouds up to here keep a copy of their coordinates in LDS

template <int P, bool LDSXYZ>
__global__ __launch_bounds__(FPS_T) void pm_fps_kernel(const float* __restrict__ xyz, int* __restrict__ idx, int N, int M,
                                                       int bs_log2, int off) {
    __shared__ float sx[LDSXYZ ? 3 * FPS_LDS_N : 3];
    __shared__ pm_u64 slot[2][FPS_T / 64];
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = T >> 6;
    const float* p = xyz + (size_t)blockIdx.x * N * 3;
    int* out = idx + (size_t)blockIdx.x * M;
    const unsigned bsm = (1u << bs_log2) - 1u;

    // a slot past the cloud: distance 0 and key 0, below every point (a point's key is ~tie > 0)
    float px[P], py[P], pz[P], run[P];
    unsigned key[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int k = tid + i * T;
        const bool in = k < N;
        px[i] = in ? p[3 * k] : 0.f;
        py[i] = in ? p[3 * k + 1] : 0.f;
        pz[i] = in ? p[3 * k + 2] : 0.f;
        run[i] = in ? 1e10f : 0.f;
        key[i] = in ? ~((pm_rev((unsigned)k & bsm, bs_log2) << 4) | ((unsigned)k >> bs_log2)) : 0u;
        if (LDSXYZ && in) {
            sx[3 * k] = px[i];
            sx[3 * k + 1] = py[i];
            sx[3 * k + 2] = pz[i];
        }
    }
    if (tid == 0) out[0] = off;
    if (LDSXYZ) __syncthreads();

    int old = 0;
    for (int j = 1; j < M; ++j) {
        const float x1 = LDSXYZ ? sx[3 * old] : p[3 * old];
        const float y1 = LDSXYZ ? sx[3 * old + 1] : p[3 * old + 1];
        const float z1 = LDSXYZ ? sx[3 * old + 2] : p[3 * old + 2];
        pm_u64 best = 0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const float d2 = fminf(lc_dist2(px[i], py[i], pz[i], x1, y1, z1), run[i]);
            run[i] = d2;
            const pm_u64 pk = ((pm_u64)__float_as_uint(d2) << 32) | key[i];
            best = pk > best ? pk : best;
        }
        best = pm_wave_max(best);
        if (nw > 1) {
            if (lane == 0) slot[j & 1][wave] = best;
            __syncthreads();
            best = slot[j & 1][0];
            for (int w = 1; w < nw; ++w) {
                const pm_u64 o = slot[j & 1][w];
                best = o > best ? o : best;
            }
        }
        const unsigned tie = ~(unsigned)best;
        old = (int)(pm_rev(tie >> 4, bs_log2) + ((tie & 15u) << bs_log2));
        if (tid == 0) out[j] = old + off;
    }
}

template <int P, bool LDSXYZ>
int pm_fps_launch(const float* xyz, int* idx, int B, int N, int M, int T, int bs_log2, int off, lc_stream_t s) {
    hipLaunchKernelGGL((pm_fps_kernel<P, LDSXYZ>), dim3((unsigned)B), dim3((unsigned)T), 0, lc_s(s), xyz, idx, N, M, bs_log2,
                       off);
    return lc_launch_status();
}

// bs_log2: the block of the tie rule; off: added to every index written
int pm_fps_dispatch(const float* xyz, int* idx, int B, int N, int M, int bs_log2, int off, lc_stream_t s) {
    const int T = N >= FPS_T ? FPS_T : (N + 63) / 64 * 64;
    const int per = (N + T - 1) / T;
    if (N > FPS_LDS_N) return pm_fps_launch<32, false>(xyz, idx, B, N, M, T, bs_log2, off, s);
    if (per <= 1) return pm_fps_launch<1, true>(xyz, idx, B, N, M, T, bs_log2, off, s);
    if (per <= 2) return pm_fps_launch<2, true>(xyz, idx, B, N, M, T, bs_log2, off, s);
    if (per <= 4) return pm_fps_launch<4, true>(xyz, idx, B, N, M, T, bs_log2, off, s);
    if (per <= 8) return pm_fps_launch<8, true>(xyz, idx, B, N, M, T, bs_log2, off, s);
    return pm_fps_launch<16, true>(xyz, idx, B, N, M, T, bs_log2, off, s);
}

// ---- k nearest neighbours --------------------------------------------------------------------------------------------
constexpr int KNN_REG_N = 1024;               // clouds up to here keep their packed words in registers

__device__ __forceinline__ pm_u64 pm_knn_word(const float* p, int k, float qx, float qy, float qz) {
    return ((pm_u64)__float_as_uint(lc_dist2(p[3 * k], p[3 * k + 1], p[3 * k + 2], qx, qy, qz)) << 32) | (unsigned)k;
}

// NPL > 0: N <= 64 NPL, the words of lane l are those of points l, l + 64, ...; NPL == 0: streamed
template <int NPL>
__global__ __launch_bounds__(256) void pm_knn_kernel(const float* __restrict__ xyz, const int* __restrict__ qidx,
                                                     int* __restrict__ out, int N, int S, int K) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;                       // no barrier below
    const int b = blockIdx.y;
    const float* p = xyz + (size_t)b * N * 3;
    int* o = out + ((size_t)b * S + s) * K;
    const int q = qidx[(size_t)b * S + s];
    if (q < 0 || q >= N) {                    // a query index outside the cloud: the row says so, nothing is read
        if (lane < K) o[lane] = -1;
        return;
    }
    const float qx = p[3 * q], qy = p[3 * q + 1], qz = p[3 * q + 2];
    constexpr int R = NPL > 0 ? NPL : 1;
    pm_u64 pk[R];
    if (NPL > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int k = lane + 64 * i;
            pk[i] = k < N ? pm_knn_word(p, k, qx, qy, qz) : ~0ull;
        }
    }
    pm_u64 lo = 0;
    int mine = -1;
    for (int r = 0; r < K; ++r) {
        pm_u64 m = ~0ull;
        if (NPL > 0) {
#pragma unroll
            for (int i = 0; i < R; ++i) m = (pk[i] >= lo && pk[i] < m) ? pk[i] : m;
        } else {
            for (int k = lane; k < N; k += 64) {
                const pm_u64 w = pm_knn_word(p, k, qx, qy, qz);
                m = (w >= lo && w < m) ? w : m;
            }
        }
        m = pm_wave_min(m);
        if (lane == r) mine = (int)(unsigned)m;
        lo = m + 1;
    }
    if (lane < K) o[lane] = mine;
}

template <int NPL>
int pm_knn_launch(const float* xyz, const int* qidx, int* out, int B, int N, int S, int K, lc_stream_t s) {
    hipLaunchKernelGGL((pm_knn_kernel<NPL>), dim3((unsigned)((S + 3) / 4), (unsigned)B), dim3(256), 0, lc_s(s), xyz, qidx, out,
                       N, S, K);
    return lc_launch_status();
}

// ---- grouping --------------------------------------------------------------------------------------------------------
constexpr int GR_T = 256;                     // columns per block
constexpr int GR_CH = 16;                     // channels per apply block

__device__ __forceinline__ int pm_clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// part[(b * nblk + blk) * 2 + {0, 1}] = sum, sum of squares of the block's 256 columns x d channels of differences
__global__ __launch_bounds__(GR_T) void pm_group_stats_kernel(const float* __restrict__ x, const int* __restrict__ fps,
                                                              const int* __restrict__ knn, double* __restrict__ part, int d,
                                                              int N, int S, int K) {
    __shared__ double ws[2][GR_T / 64];
    const int b = blockIdx.y, tid = threadIdx.x, L = S * K;
    const int col = blockIdx.x * GR_T + tid;
    const float* xb = x + (size_t)b * d * N;
    double sum = 0.0, sq = 0.0;
    if (col < L) {
        const int i = pm_clampi(knn[(size_t)b * L + col], N), a = pm_clampi(fps[(size_t)b * S + col / K], N);
        for (int c = 0; c < d; ++c) {
            const float v = xb[(size_t)c * N + i] - xb[(size_t)c * N + a];
            sum += (double)v;
            sq += (double)v * (double)v;
        }
    }
    sum = lc_wave_sum(sum);
    sq = lc_wave_sum(sq);
    if ((tid & 63) == 0) {
        ws[0][tid >> 6] = sum;
        ws[1][tid >> 6] = sq;
    }
    __syncthreads();
    if (tid == 0) {
        double a0 = ws[0][0], a1 = ws[1][0];
        for (int w = 1; w < GR_T / 64; ++w) {
            a0 += ws[0][w];
            a1 += ws[1][w];
        }
        double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
        o[0] = a0;
        o[1] = a1;
    }
}

__global__ __launch_bounds__(GR_T) void pm_group_apply_kernel(const float* __restrict__ x, const int* __restrict__ fps,
                                                              const int* __restrict__ knn, const float* __restrict__ alpha,
                                                              const float* __restrict__ beta, const double* __restrict__ part,
                                                              float* __restrict__ out, float* __restrict__ sigma, int d, int N,
                                                              int S, int K) {
    __shared__ float s_den;
    const int b = blockIdx.z, tid = threadIdx.x, L = S * K, nblk = gridDim.x;
    if (tid < 64) {                           // every block adds the same pairs in the same order
        const double* pb = part + (size_t)b * nblk * 2;
        double sum = 0.0, sq = 0.0;
        for (int i = tid; i < nblk; i += 64) {
            sum += pb[2 * i];
            sq += pb[2 * i + 1];
        }
        sum = lc_wave_sum(sum);
        sq = lc_wave_sum(sq);
        if (tid == 0) {
            const double n = (double)L * (double)d;
            double var = (sq - sum * sum / n) / (n - 1.0);
            var = var > 0.0 ? var : 0.0;
            const float sg = (float)sqrt(var);
            s_den = sg + 1e-5f;
            if (sigma && blockIdx.x == 0 && blockIdx.y == 0) sigma[b] = sg;
        }
    }
    __syncthreads();
    const int col = blockIdx.x * GR_T + tid;
    if (col >= L) return;
    const float den = s_den;
    const int i = pm_clampi(knn[(size_t)b * L + col], N), a = pm_clampi(fps[(size_t)b * S + col / K], N);
    const float* xb = x + (size_t)b * d * N;
    float* ob = out + (size_t)b * 2 * d * L;
    const int c1 = min(d, (int)(blockIdx.y + 1) * GR_CH);
    for (int c = blockIdx.y * GR_CH; c < c1; ++c) {
        const float av = xb[(size_t)c * N + a];
        const float v = xb[(size_t)c * N + i] - av;
        ob[(size_t)c * L + col] = alpha[c] * (v / den) + beta[c];
        ob[(size_t)(d + c) * L + col] = av;
    }
}

// ---- maximum over groups ---------------------------------------------------------------------------------------------
// one thread per (b, c, g)
__global__ __launch_bounds__(256) void pm_groupmax_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int G,
                                                          int K, long long n, long long obs, long long ocs, long long ogs) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int g = (int)(t % G);
    const long long bc = t / G;
    const int c = (int)(bc % C);
    const long long b = bc / C;
    const float* p = x + (size_t)t * K;
    float m = p[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, p[k]);
    out[b * obs + c * ocs + g * ogs] = m;
}

}  // namespace

extern "C" int lc_pointmlp_limit(int which) {
    switch (which) {
        case 0: return LC_FPS_MAX_N;
        case 1: return LC_KNN_MAX_N;
        case 2: return LC_KNN_MAX_K;
        case 3: return PwGeom<1>::KC;
        case 4: return DF_CO;
        case 5: return PwGeom<1>::PXW;
        case 6: return GR_T;
        default: return 0;
    }
}

extern "C" int lc_fps_fwd(const float* xyz, int* idx, int B, int N, int M, lc_stream_t s) {
    if (!xyz || !idx || B < 1 || N < 1 || M < 1) return LC_EINVAL;
    if (N > LC_FPS_MAX_N) return LC_EUNSUP;
    int bs_log2 = 0;                          // the reference's block: the largest power of two <= min(N, 1024)
    while (bs_log2 < 10 && (2 << bs_log2) <= N) ++bs_log2;
    return pm_fps_dispatch(xyz, idx, B, N, M, bs_log2, 0, s);
}

// one cloud of a stacked batch (lidargen.ops.pointnet2.pointnet2_stack): the tie rule of a 1024-thread block whatever N
// is, indices + off
extern "C" int lc_fps_stack_fwd(const float* xyz, int* idx, int N, int M, int off, lc_stream_t s) {
    if (!xyz || !idx || N < 1 || M < 1 || off < 0) return LC_EINVAL;
    if (N > LC_FPS_MAX_N) return LC_EUNSUP;
    return pm_fps_dispatch(xyz, idx, 1, N, M, 10, off, s);
}

extern "C" int lc_knn_fwd(const float* xyz, const int* query_idx, int* out, int B, int N, int S, int K, lc_stream_t s) {
    if (!xyz || !query_idx || !out || B < 1 || N < 1 || S < 1 || K < 1 || K > N) return LC_EINVAL;
    if (K > LC_KNN_MAX_K || N > LC_KNN_MAX_N || B > 65535) return LC_EUNSUP;
    if (N > KNN_REG_N) return pm_knn_launch<0>(xyz, query_idx, out, B, N, S, K, s);
    const int per = (N + 63) / 64;
    if (per <= 1) return pm_knn_launch<1>(xyz, query_idx, out, B, N, S, K, s);
    if (per <= 2) return pm_knn_launch<2>(xyz, query_idx, out, B, N, S, K, s);
    if (per <= 4) return pm_knn_launch<4>(xyz, query_idx, out, B, N, S, K, s);
    if (per <= 8) return pm_knn_launch<8>(xyz, query_idx, out, B, N, S, K, s);
    return pm_knn_launch<16>(xyz, query_idx, out, B, N, S, K, s);
}

extern "C" int64_t lc_pointmlp_group_scratch_elems(int B, int S, int K) {
    if (B < 1 || S < 1 || K < 1) return 0;
    return (int64_t)B * (((int64_t)S * K + GR_T - 1) / GR_T) * 2;
}

extern "C" int lc_pointmlp_group_fwd(const float* x, const int* fps_idx, const int* knn_idx, const float* alpha,
                                     const float* beta, float* out, double* scratch, float* sigma, int B, int d, int N, int S,
                                     int K, lc_stream_t s) {
    if (!x || !fps_idx || !knn_idx || !alpha || !beta || !out || !scratch || B < 1 || d < 1 || N < 1 || S < 1 || K < 1)
        return LC_EINVAL;
    const long long L = (long long)S * K;
    if (L * d < 2) return LC_EINVAL;          // the unbiased deviation of one value does not exist
    if (out == x) return LC_EINVAL;
    const long long nblk = (L + GR_T - 1) / GR_T, ny = (d + GR_CH - 1) / GR_CH;
    if (L > 2147483647ll || nblk > 2147483647ll || ny > 65535 || B > 65535) return LC_EUNSUP;
    if (reinterpret_cast<uintptr_t>(scratch) & 7u) return LC_EUNSUP;
    hipLaunchKernelGGL(pm_group_stats_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(GR_T), 0, lc_s(s), x, fps_idx, knn_idx,
                       scratch, d, N, S, K);
    int e = lc_launch_status();
    if (e != LC_OK) return e;
    hipLaunchKernelGGL(pm_group_apply_kernel, dim3((unsigned)nblk, (unsigned)ny, (unsigned)B), dim3(GR_T), 0, lc_s(s), x, fps_idx,
                       knn_idx, alpha, beta, scratch, out, sigma, d, N, S, K);
    return lc_launch_status();
}

extern "C" int64_t lc_pointmlp_packed_weight_elems(int Ci, int Co) {
    if (Ci < 1 || Co < 1) return 0;
    return df_packed_elems(PwGeom<1>::KC, 1, Ci, Co);
}

// HOST pointers.  w [Co][Ci].  out: the engine's layout at one tap (dense_f32.h: df_pack_weight).
extern "C" int lc_pointmlp_pack_weight(const float* w, int Ci, int Co, float* out) {
    if (!w || !out || Ci < 1 || Co < 1) return LC_EINVAL;
    df_pack_weight(PwGeom<1>::KC, 1, Ci, Co, out, [=](int co, int ci, int) { return w[(size_t)co * Ci + ci]; });
    return LC_OK;
}

extern "C" int lc_pointmlp_conv_fwd(const float* x, const float* wpk, const float* bias, const float* res, float* y, int B,
                                    int Ci, int Co, int L, int act, lc_stream_t s) {
    if (!x || !wpk || !bias || !y || B < 1 || Ci < 1 || Co < 1 || L < 1) return LC_EINVAL;
    if (y == x || y == res) return LC_EINVAL;                     // a block reads columns other blocks write
    if (!lc_aligned16(wpk)) return LC_EUNSUP;                     // read as 128-bit quads
    return df_dispatch<PwGeom>(DfArgs{x, wpk, Ci, Co, 1, L, L, 1}, PwEpi{bias, res, y, act ? 1 : 0}, B, L, s);
}

extern "C" int lc_pointmlp_groupmax_fwd(const float* x, float* out, int B, int C, int G, int K, int64_t out_bs, int64_t out_cs,
                                        int64_t out_gs, lc_stream_t s) {
    if (!x || !out || B < 1 || C < 1 || G < 1 || K < 1 || out == x) return LC_EINVAL;
    const long long n = (long long)B * C * G, nb = (n + 255) / 256;
    if (nb > 2147483647ll) return LC_EUNSUP;
    hipLaunchKernelGGL(pm_groupmax_kernel, dim3((unsigned)nb), dim3(256), 0, lc_s(s), x, out, C, G, K, n, (long long)out_bs,
                       (long long)out_cs, (long long)out_gs);
    return lc_launch_status();
}
