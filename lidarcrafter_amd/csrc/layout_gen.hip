// Scene-graph layout generator (UNet1DModel on a 1-D signal of length 1): every conv / linear of one denoiser step is a
// skinny dense layer on row-major [M, K] activations, M = objects or triples (1 ... a few thousand).  DESIGN.md section 5h.
//
//   lc_skinny_gemm_fwd     partial products  P[c][m][n] = sum_{k in chunk c} X[m,k] W[n,k]   (exact fp32 FMA)
//   lc_skinny_combine_fwd  Y = act(sum_c P[c] + bias) + vec[row_of[m]] + residual            (fixed chunk order)
//   lc_rowprep_fwd         per-row GroupNorm / LayerNorm (+SiLU) or a plain gathered concatenation of row segments
//   lc_graph_pool_fwd      scatter-mean of triple rows onto object rows through a CSR, no atomics
//   lc_time_embed_fwd      [cos(t f) | sin(t f)]
//
// Summation order.  K is cut into chunks of SK_KC = 128; inside a chunk ONE thread owns an output element and adds its
// products in ascending k with fmaf.  With a K split every chunk is a block of its own (the weight stream of a layer
// with a handful of column tiles is spread over the chip) and the combine pass adds the chunk sums in ascending chunk
// order; without a split the block walks the chunks itself and adds each chunk sum to its total in the same order.  Both
// give the same bits, and neither depends on M, on the tile a row falls into or on scheduling.
#include "common.h"

#define SK_BM 32
#define SK_BN 64
#define SK_KC 128
#define SK_KS 32

struct SkSegs {
    const float* p0; const float* p1; const float* p2;
    const int* i0; const int* i1; const int* i2;
    long long ld0, ld1, ld2;
    int w0, w1, w2;
};

// element (row, k) of the virtual matrix [seg0 | seg1 | seg2]; k < w0 + w1 + w2
__device__ __forceinline__ float sk_load(const SkSegs& s, int row, int k) {
    const float* p = s.p0;
    const int* ix = s.i0;
    long long ld = s.ld0;
    if (k >= s.w0) {
        k -= s.w0; p = s.p1; ix = s.i1; ld = s.ld1;
        if (k >= s.w1) { k -= s.w1; p = s.p2; ix = s.i2; ld = s.ld2; }
    }
    const int r = ix ? ix[row] : row;
    return p[(long long)r * ld + k];
}

static int sk_segs(const lc_row_segment* segs, int nseg, int K, SkSegs* out) {
    if (!segs || nseg < 1 || nseg > 3) return LC_EINVAL;
    SkSegs s = {};
    int tot = 0;
    for (int j = 0; j < nseg; ++j) {
        if (!segs[j].p || segs[j].width < 1 || segs[j].ld < segs[j].width) return LC_EINVAL;
        tot += segs[j].width;
    }
    if (tot != K) return LC_EINVAL;
    s.p0 = segs[0].p; s.i0 = segs[0].idx; s.ld0 = segs[0].ld; s.w0 = segs[0].width;
    if (nseg > 1) { s.p1 = segs[1].p; s.i1 = segs[1].idx; s.ld1 = segs[1].ld; s.w1 = segs[1].width; }
    if (nseg > 2) { s.p2 = segs[2].p; s.i2 = segs[2].idx; s.ld2 = segs[2].ld; s.w2 = segs[2].width; }
    *out = s;
    return LC_OK;
}

__global__ __launch_bounds__(256) void sk_gemm_kernel(SkSegs s, const float* __restrict__ W, float* __restrict__ parts,
                                                      int M, int N, int K, int split) {
    __shared__ float Xs[SK_KS][SK_BM + 1];
    __shared__ float Ws[SK_KS][SK_BN + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * SK_BN, m0 = blockIdx.y * SK_BM;
    const int nchunks = (K + SK_KC - 1) / SK_KC;
    const int c0 = split ? (int)blockIdx.z : 0, c1 = split ? c0 + 1 : nchunks;
    float tot[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[i][j] = 0.0f;
    for (int c = c0; c < c1; ++c) {
        float acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
        for (int ks = 0; ks < SK_KC / SK_KS; ++ks) {
            const int k0 = c * SK_KC + ks * SK_KS;
            if (k0 >= K) break;                                   // block-uniform
#pragma unroll
            for (int i = 0; i < (SK_BN * SK_KS) / 256; ++i) {
                const int e = tid + 256 * i, kk = e & (SK_KS - 1), nn = e / SK_KS;
                const int n = n0 + nn, k = k0 + kk;
                Ws[kk][nn] = (n < N && k < K) ? W[(long long)n * K + k] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < (SK_BM * SK_KS) / 256; ++i) {
                const int e = tid + 256 * i, kk = e & (SK_KS - 1), rr = e / SK_KS;
                const int m = m0 + rr, k = k0 + kk;
                Xs[kk][rr] = (m < M && k < K) ? sk_load(s, m, k) : 0.0f;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < SK_KS; ++kk) {
                const float x0 = Xs[kk][ty * 2], x1 = Xs[kk][ty * 2 + 1];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float w = Ws[kk][tx + 16 * j];
                    acc[0][j] = fmaf(x0, w, acc[0][j]);
                    acc[1][j] = fmaf(x1, w, acc[1][j]);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[i][j] += acc[i][j];
    }
    float* dst = parts + (split ? (long long)blockIdx.z * M * N : 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + ty * 2 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx + 16 * j;
            if (n < N) dst[(long long)m * N + n] = tot[i][j];
        }
    }
}

__device__ __forceinline__ float sk_sum_parts(const float* __restrict__ parts, int nparts, long long slab, long long at) {
    float v = 0.0f;
    for (int c = 0; c < nparts; ++c) v += parts[c * slab + at];
    return v;
}

__global__ __launch_bounds__(256) void sk_combine_kernel(const float* __restrict__ parts, int nparts,
                                                         const float* __restrict__ bias, int act,
                                                         const float* __restrict__ vec, long long vec_ld,
                                                         const int* __restrict__ vec_row,
                                                         const float* __restrict__ res, long long res_ld,
                                                         float* __restrict__ y, long long y_ld, int M, int N) {
    const int No = act == 2 ? N / 2 : N;
    const long long total = (long long)M * No, slab = (long long)M * N;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int m = (int)(e / No), n = (int)(e - (long long)m * No);
        float v = sk_sum_parts(parts, nparts, slab, (long long)m * N + n);
        if (bias) v += bias[n];
        if (act == 1) {
            v = fmaxf(v, 0.0f);
        } else if (act == 2) {
            float g = sk_sum_parts(parts, nparts, slab, (long long)m * N + No + n);
            if (bias) g += bias[No + n];
            v = v * (0.5f * g * (1.0f + erff(g * 0.70710678118654752440f)));
        }
        if (vec) v += vec[(long long)(vec_row ? vec_row[m] : 0) * vec_ld + n];
        if (res) v += res[(long long)m * res_ld + n];
        y[(long long)m * y_ld + n] = v;
    }
}

// one block per row; the row (<= 4096 values) sits in LDS, every wave takes whole groups
__global__ __launch_bounds__(256) void sk_rowprep_kernel(SkSegs s, float* __restrict__ y, long long y_ld, int C, int G,
                                                         float eps, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int silu) {
    __shared__ float row[4096];
    const int m = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) row[c] = sk_load(s, m, c);
    __syncthreads();
    if (G > 0) {
        const int cs = C / G, wave = tid >> 6, lane = tid & 63;
        for (int g = wave; g < G; g += 4) {
            float sum = 0.0f;
            for (int c = lane; c < cs; c += 64) sum += row[g * cs + c];
            const float mean = lc_wave_sum(sum) / (float)cs;
            float sq = 0.0f;
            for (int c = lane; c < cs; c += 64) { const float d = row[g * cs + c] - mean; sq = fmaf(d, d, sq); }
            const float rstd = 1.0f / sqrtf(lc_wave_sum(sq) / (float)cs + eps);
            for (int c = lane; c < cs; c += 64) {
                const int ch = g * cs + c;
                float v = (row[ch] - mean) * rstd;
                if (gamma) v = v * gamma[ch] + (beta ? beta[ch] : 0.0f);
                row[ch] = v;
            }
        }
        __syncthreads();
    }
    for (int c = tid; c < C; c += 256) {
        float v = row[c];
        if (silu) v = v / (1.0f + expf(-v));
        y[(long long)m * y_ld + c] = v;
    }
}

// object o: sum of t[triple, s_col + h] over the triples it is the subject of (ascending), then of t[triple, o_col + h]
// over the triples it is the object of (ascending) -- the order two sequential scatter_add calls visit them in -- divided
// by max(count, 1).  slots[] holds 2 * triple + (0 subject | 1 object) in that order, row_ptr[] is its CSR index.
__global__ __launch_bounds__(256) void sk_pool_kernel(const float* __restrict__ t, long long t_ld, int s_col, int o_col,
                                                      const int* __restrict__ row_ptr, const int* __restrict__ slots,
                                                      float* __restrict__ y, long long y_ld, int H) {
    const int o = blockIdx.x;
    const int b = row_ptr[o], e = row_ptr[o + 1];
    const float cnt = (float)(e - b > 1 ? e - b : 1);
    for (int h = threadIdx.x; h < H; h += 256) {
        float v = 0.0f;
        for (int i = b; i < e; ++i) {
            const int sl = slots[i];
            v += t[(long long)(sl >> 1) * t_ld + ((sl & 1) ? o_col : s_col) + h];
        }
        y[(long long)o * y_ld + h] = v / cnt;
    }
}

__global__ __launch_bounds__(256) void sk_time_embed_kernel(const float* __restrict__ t, const float* __restrict__ freqs,
                                                            float* __restrict__ y, int U, int half) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= U * half) return;
    const int u = e / half, i = e - u * half;
    const float a = t[u] * freqs[i];
    y[(long long)u * 2 * half + i] = cosf(a);
    y[(long long)u * 2 * half + half + i] = sinf(a);
}

extern "C" {

int64_t lc_skinny_parts(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    const int64_t tiles = (int64_t)((M + SK_BM - 1) / SK_BM) * ((N + SK_BN - 1) / SK_BN);
    const int nchunks = (K + SK_KC - 1) / SK_KC;
    // split while the column/row tiles alone leave most of the 256 CUs without a block
    return (tiles < 256 && nchunks > 1) ? nchunks : 1;
}

int lc_skinny_gemm_fwd(const lc_row_segment* segs, int nseg, const float* w, float* parts, int M, int N, int K,
                       int nparts, lc_stream_t s) {
    if (!w || !parts || M < 1 || N < 1 || K < 1) return LC_EINVAL;
    const int nchunks = (K + SK_KC - 1) / SK_KC;
    if (nparts != 1 && nparts != nchunks) return LC_EINVAL;
    if (nchunks > 65535 || (int64_t)M * N * nparts >= (1ll << 40)) return LC_EUNSUP;
    SkSegs sg;
    const int rc = sk_segs(segs, nseg, K, &sg);
    if (rc != LC_OK) return rc;
    const int mt = (M + SK_BM - 1) / SK_BM;
    if (mt > 65535) return LC_EUNSUP;
    const int split = nparts > 1 ? 1 : 0;
    dim3 grid((N + SK_BN - 1) / SK_BN, mt, split ? nchunks : 1);
    hipLaunchKernelGGL(sk_gemm_kernel, grid, dim3(256), 0, lc_s(s), sg, w, parts, M, N, K, split);
    return lc_launch_status();
}

int lc_skinny_combine_fwd(const float* parts, int nparts, const float* bias, int act, const float* vec, int64_t vec_ld,
                          const int32_t* vec_row, const float* res, int64_t res_ld, float* y, int64_t y_ld, int M, int N,
                          lc_stream_t s) {
    if (!parts || !y || nparts < 1 || M < 1 || N < 1 || act < 0 || act > 2) return LC_EINVAL;
    if (act == 2 && (N & 1)) return LC_EINVAL;
    const int No = act == 2 ? N / 2 : N;
    if (y_ld < No || (res && res_ld < No) || (vec && vec_ld < No)) return LC_EINVAL;
    const int64_t total = (int64_t)M * No;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sk_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, lc_s(s), parts, nparts, bias, act, vec,
                       (long long)vec_ld, vec_row, res, (long long)res_ld, y, (long long)y_ld, M, N);
    return lc_launch_status();
}

int lc_rowprep_fwd(const lc_row_segment* segs, int nseg, float* y, int64_t y_ld, int M, int C, int G, float eps,
                   const float* gamma, const float* beta, int silu, lc_stream_t s) {
    if (!y || M < 1 || C < 1 || y_ld < C || G < 0) return LC_EINVAL;
    if (C > 4096 || (G > 0 && C % G != 0)) return LC_EUNSUP;
    SkSegs sg;
    const int rc = sk_segs(segs, nseg, C, &sg);
    if (rc != LC_OK) return rc;
    hipLaunchKernelGGL(sk_rowprep_kernel, dim3(M), dim3(256), 0, lc_s(s), sg, y, (long long)y_ld, C, G, eps, gamma, beta,
                       silu);
    return lc_launch_status();
}

int lc_graph_pool_fwd(const float* t, int64_t t_ld, int s_col, int o_col, const int32_t* row_ptr, const int32_t* slots,
                      float* y, int64_t y_ld, int O, int H, lc_stream_t s) {
    if (!t || !row_ptr || !slots || !y || O < 1 || H < 1 || s_col < 0 || o_col < 0) return LC_EINVAL;
    if (t_ld < s_col + H || t_ld < o_col + H || y_ld < H) return LC_EINVAL;
    hipLaunchKernelGGL(sk_pool_kernel, dim3(O), dim3(256), 0, lc_s(s), t, (long long)t_ld, s_col, o_col, row_ptr, slots, y,
                       (long long)y_ld, H);
    return lc_launch_status();
}

int lc_time_embed_fwd(const float* t, const float* freqs, float* y, int U, int half, lc_stream_t s) {
    if (!t || !freqs || !y || U < 1 || half < 1) return LC_EINVAL;
    const int total = U * half;
    hipLaunchKernelGGL(sk_time_embed_kernel, dim3((total + 255) / 256), dim3(256), 0, lc_s(s), t, freqs, y, U, half);
    return lc_launch_status();
}

}  // extern "C"
