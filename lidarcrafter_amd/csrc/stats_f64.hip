// Float64 statistics behind the Frechet distance and the squared MMD of lidargen/metrics/distribution.py (DESIGN.md
// section 5t; include/lidarcrafter_hip.h: lc_stats_*).
//   * one 64 x 64 x 16 tile engine on v_mfma_f64_16x16x4_f64: C[i][j] = sum_k P(i, k) Q(j, k), both operands described by a
//     row and a k stride (so P Q^T, P^T Q and P Q are the same kernel), optionally gathered through a row index;
//   * two epilogues: the plain store, and the cubic kernel (g / width + 1)^3 reduced to one partial sum per tile;
//   * centring, fixed-order reductions, and a one-sided (Hestenes) Jacobi eigen-solver on the rows of a symmetric matrix.
// No float atomics anywhere; every sum has one order, a function of the shapes alone, so two runs give the same bits.
//
// Fragment layout of the f64 MFMA (checked bit for bit by tests/test_stats_f64.py::test_engine_exact): lane l holds
// A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one double each; result register r of lane l is
// D[row (l >> 4) + 4 r][col l & 15].
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TM = 64, TN = 64, TK = 16;     // block tile; 4 waves, each a 32 x 32 quarter = 2 x 2 MFMA tiles
constexpr int LDT = TM + 4;                  // LDS row pitch in doubles ([k][row] layout)
constexpr int NT = 256;
constexpr int EPT = TM * TK / NT;            // elements of one operand tile per thread (4)

// One operand of the engine: element (row, k) = base[src(row) * rs + k * ks], src(row) = idx ? idx[row] : row; a row
// outside [0, rows), a gathered row outside [0, src_rows) and k outside [0, K) read as 0 and touch no memory.
struct Operand {
    const double* base;
    const int* idx;
    int64_t rs, ks;
    int rows, src_rows;
};

// where thread t finds element e of its tile share: consecutive threads along k when k is the contiguous direction,
// along the rows otherwise
__device__ __forceinline__ void tile_pos(bool kfast, int t, int e, int& r, int& k) {
    const int f = t + NT * e;
    if (kfast) { k = f & (TK - 1); r = f >> 4; }
    else { r = f & (TM - 1); k = f >> 6; }
}

struct TileLoader {
    int64_t off[EPT];      // element offset of (row, k = 0), -1: reads as zero
    int kk[EPT], rr[EPT];
    const double* base;
    int64_t ks;
    __device__ __forceinline__ void init(const Operand& o, int row0, int t) {
        base = o.base;
        ks = o.ks;
        const bool kfast = o.ks == 1;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            tile_pos(kfast, t, e, rr[e], kk[e]);
            const int row = row0 + rr[e];
            int64_t src = -1;
            if (row < o.rows) {
                src = row;
                if (o.idx) {
                    const int g = o.idx[row];
                    src = (g >= 0 && g < o.src_rows) ? g : -1;
                }
            }
            off[e] = src < 0 ? -1 : src * o.rs;
        }
    }
    __device__ __forceinline__ void load(double (&v)[EPT], int k0, int K) const {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int k = k0 + kk[e];
            v[e] = (off[e] >= 0 && k < K) ? base[off[e] + (int64_t)k * ks] : 0.0;
        }
    }
    __device__ __forceinline__ void store(double (*lds)[LDT], const double (&v)[EPT]) const {
#pragma unroll
        for (int e = 0; e < EPT; ++e) lds[kk[e]][rr[e]] = v[e];
    }
};

// acc[mi][ni] of this wave's quarter of the tile (i0, j0) .. : the K loop, global -> registers -> LDS -> MFMA, the next
// tile's loads in flight while the current one is multiplied.
__device__ __forceinline__ void tile_product(const Operand& P, const Operand& Q, int K, int i0, int j0, f64x4 (&acc)[2][2]) {
    __shared__ double sP[TK][LDT];
    __shared__ double sQ[TK][LDT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    TileLoader lp, lq;
    lp.init(P, i0, t);
    lq.init(Q, j0, t);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
    double vp[EPT], vq[EPT];
    lp.load(vp, 0, K);
    lq.load(vq, 0, K);
    for (int k0 = 0; k0 < K; k0 += TK) {
        lp.store(sP, vp);
        lq.store(sQ, vq);
        __syncthreads();
        if (k0 + TK < K) {
            lp.load(vp, k0 + TK, K);
            lq.load(vq, k0 + TK, K);
        }
#pragma unroll
        for (int ks = 0; ks < TK; ks += 4) {
            const int kr = ks + (lane >> 4), c = lane & 15;
            const double a0 = sP[kr][wm + c], a1 = sP[kr][wm + 16 + c];
            const double b0 = sQ[kr][wn + c], b1 = sQ[kr][wn + 16 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}

// (row, col) inside the block tile of result register r of acc[mi][ni]
__device__ __forceinline__ void frag_pos(int mi, int ni, int r, int& row, int& col) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    row = (wave >> 1) * 32 + mi * 16 + (lane >> 4) + 4 * r;
    col = (wave & 1) * 32 + ni * 16 + (lane & 15);
}

// the sum of v over the block in one fixed order: lanes by the xor tree, then waves 0, 1, 2, ...; the same value in every
// thread (every thread of the block must call it)
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double part[NT / 64];
    v = lc_wave_sum(v);
    __syncthreads();              // `part` may still be read by the previous call
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(NT) void gemm_kernel(Operand P, Operand Q, double* __restrict__ C, int64_t ldc, int K) {
    const int i0 = blockIdx.y * TM, j0 = blockIdx.x * TN;
    f64x4 acc[2][2];
    tile_product(P, Q, K, i0, j0, acc);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row, col;
                frag_pos(mi, ni, r, row, col);
                if (i0 + row < P.rows && j0 + col < Q.rows) C[(int64_t)(i0 + row) * ldc + j0 + col] = acc[mi][ni][r];
            }
}

// blockIdx.z = 3 subset + which: 0 x x^T, 1 y y^T (diagonal dropped), 2 x y^T; x = fx rows table[subset][0][:], y = fy rows
// table[subset][1][:].  partial[(3 subset + which) tiles + tile] = the tile's sum of (g / width + 1)^3.
__global__ __launch_bounds__(NT) void mmd_kernel(const double* __restrict__ fx, int nx, const double* __restrict__ fy, int ny,
                                                 const int* __restrict__ table, int m, int width,
                                                 double* __restrict__ partial) {
    const int subset = blockIdx.z / 3, which = blockIdx.z % 3;
    const int* tx = table + (int64_t)subset * 2 * m;
    const int* ty = tx + m;
    const Operand X{fx, tx, width, 1, m, nx}, Y{fy, ty, width, 1, m, ny};
    const Operand& P = which == 1 ? Y : X;
    const Operand& Q = which == 0 ? X : Y;
    const int i0 = blockIdx.y * TM, j0 = blockIdx.x * TN;
    f64x4 acc[2][2];
    tile_product(P, Q, width, i0, j0, acc);
    const double w = (double)width;
    double sum = 0.0;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row, col;
                frag_pos(mi, ni, r, row, col);
                row += i0;
                col += j0;
                const double u = acc[mi][ni][r] / w + 1.0;
                const double v = (u * u) * u;
                const bool keep = row < m && col < m && (which == 2 || row != col);
                sum += keep ? v : 0.0;
            }
    sum = block_sum(sum);
    if (threadIdx.x == 0)
        partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
}

// out[subset][0] = the sum of the 2 * tiles within-set partials, out[subset][1] = the sum of the cross partials
__global__ __launch_bounds__(NT) void mmd_sum_kernel(const double* __restrict__ partial, int tiles, double* __restrict__ out) {
    const int subset = blockIdx.x, cross = blockIdx.y;
    const double* p = partial + ((int64_t)subset * 3 + (cross ? 2 : 0)) * tiles;
    const int n = cross ? tiles : 2 * tiles;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) s += p[i];
    s = block_sum(s);
    if (threadIdx.x == 0) out[subset * 2 + cross] = s;
}

// mean[j] of the n rows: 64 columns x 4 row classes per block, each class summed in row order, then ((0 + 1) + (2 + 3)) / n
__global__ __launch_bounds__(NT) void colmean_kernel(const double* __restrict__ X, int n, int d, double* __restrict__ mean) {
    __shared__ double part[4][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6, j = blockIdx.x * 64 + c;
    double s = 0.0;
    if (j < d)
        for (int i = g; i < n; i += 4) s += X[(int64_t)i * d + j];
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && j < d) mean[j] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) / (double)n;
}

__global__ __launch_bounds__(NT) void center_kernel(const double* __restrict__ X, const double* __restrict__ mean, int64_t total,
                                                    int d, double scale, double* __restrict__ A) {
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT)
        A[e] = (X[e] - mean[e % d]) / scale;
}

// mode 0: a, 1: a^2, 2: (a - b)^2, 3: sqrt(max(a, 0))
__device__ __forceinline__ double reduce_term(int mode, const double* a, int64_t sa, const double* b, int64_t sb, int64_t i) {
    const double x = a[i * sa];
    if (mode == 0) return x;
    if (mode == 1) return x * x;
    if (mode == 2) { const double y = x - b[i * sb]; return y * y; }
    return sqrt(fmax(x, 0.0));
}

// block g sums the elements of chunk g in one order; the last launch (one block) adds the chunk sums in chunk order
__global__ __launch_bounds__(NT) void reduce_kernel(const double* __restrict__ a, int64_t sa, const double* __restrict__ b,
                                                    int64_t sb, int64_t n, int64_t chunk, int mode, double* __restrict__ out) {
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += NT) s += reduce_term(mode, a, sa, b, sb, i);
    s = block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// out row i = sqrt(lam_i) V row i, 0 where lam_i <= cut max_j lam_j (the numerical rank: such an eigenvalue is rounding noise
// of the largest)
__global__ __launch_bounds__(NT) void scale_rows_kernel(const double* __restrict__ V, const double* __restrict__ lam, int k,
                                                        double cut, double* __restrict__ out) {
    const int i = blockIdx.x;
    double top = 0.0;
    for (int j = threadIdx.x; j < k; j += NT) top = fmax(top, lam[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = fmax(top, __shfl_xor(top, o, 64));
    __shared__ double wtop[NT / 64];
    if ((threadIdx.x & 63) == 0) wtop[threadIdx.x >> 6] = top;
    __syncthreads();
    top = fmax(fmax(wtop[0], wtop[1]), fmax(wtop[2], wtop[3]));
    const double f = lam[i] > cut * top ? sqrt(lam[i]) : 0.0;
    for (int j = threadIdx.x; j < k; j += NT) out[(int64_t)i * k + j] = f * V[(int64_t)i * k + j];
}

__global__ __launch_bounds__(NT) void row_norm_kernel(const double* __restrict__ W, int k, double* __restrict__ lam) {
    const int i = blockIdx.x;
    double s = 0.0;
    for (int j = threadIdx.x; j < k; j += NT) { const double x = W[(int64_t)i * k + j]; s += x * x; }
    s = block_sum(s);
    if (threadIdx.x == 0) lam[i] = sqrt(s);
}

__global__ __launch_bounds__(NT) void identity_kernel(double* __restrict__ V, int k) {
    const int i = blockIdx.x;
    for (int j = threadIdx.x; j < k; j += NT) V[(int64_t)i * k + j] = i == j ? 1.0 : 0.0;
}

}  // namespace

// The round-robin ("circle") schedule of the Jacobi sweeps over n = k rounded up to even players: player n - 1 stays, the
// others rotate.  Step s in [0, n - 1), slot i in [0, n / 2): the pair (p, q); a pair that names the player k of an odd k is
// the idle slot.
__host__ __device__ inline void lc_jacobi_pair_of(int k, int step, int slot, int& p, int& q) {
    const int n = k + (k & 1), r = n - 1;
    if (slot == 0) { p = r; q = step % r; }
    else { p = (step + slot) % r; q = (step - slot + r) % r; }
    if (p > q) { const int t = p; p = q; q = t; }
}

namespace {

// One step: block = one pair of rows (p, q) of W (and of V).  alpha = |w_p|^2, beta = |w_q|^2, gamma = w_p . w_q in one
// fixed order.  The pair is rotated when both hold, and then *flag = 1 (a plain store of one value from every rotating
// block):
//   |gamma| > tol sqrt(alpha) sqrt(beta)                      the rows are not orthogonal to rounding, and
//   |gamma| > atol sqrt(*fro2 / k) sqrt(max(alpha, beta))     the entry (p, q) of V S V^T, gamma over the larger norm, is above
//                                                             atol times the matrix' root-mean-square eigenvalue.
// The second is two-sided Jacobi's absolute criterion: the eigenvalues are wanted to k eps lambda_max, not to relative
// accuracy, and without it the rows of a rank-deficient matrix that are rounding noise keep rotating against each other.
// A pair whose norms multiply to zero is left alone.
template <int E>
__global__ __launch_bounds__(NT) void jacobi_step_kernel(double* __restrict__ W, double* __restrict__ V, int k, int step,
                                                         double tol, double atol, const double* __restrict__ fro2,
                                                         int* __restrict__ flag) {
    int p, q;
    lc_jacobi_pair_of(k, step, blockIdx.x, p, q);
    if (q >= k) return;                                  // the idle slot of an odd k (p < q)
    double* wp = W + (int64_t)p * k;
    double* wq = W + (int64_t)q * k;
    double a[E], b[E];
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = threadIdx.x + NT * e;
        a[e] = j < k ? wp[j] : 0.0;
        b[e] = j < k ? wq[j] : 0.0;
        alpha += a[e] * a[e];
        beta += b[e] * b[e];
        gamma += a[e] * b[e];
    }
    alpha = block_sum(alpha);
    beta = block_sum(beta);
    gamma = block_sum(gamma);
    const double scale = sqrt(alpha) * sqrt(beta);
    if (!(scale > 0.0) || !(fabs(gamma) > tol * scale)) return;      // block-uniform
    if (fro2 && !(fabs(gamma) > atol * sqrt(*fro2 / (double)k) * sqrt(fmax(alpha, beta)))) return;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
    if (threadIdx.x == 0) *flag = 1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = threadIdx.x + NT * e;
        if (j < k) {
            wp[j] = c * a[e] - s * b[e];
            wq[j] = s * a[e] + c * b[e];
        }
    }
    if (V) {
        double* vp = V + (int64_t)p * k;
        double* vq = V + (int64_t)q * k;
        for (int j = threadIdx.x; j < k; j += NT) {
            const double x = vp[j], y = vq[j];
            vp[j] = c * x - s * y;
            vq[j] = s * x + c * y;
        }
    }
}

inline bool fits_i32(int64_t v) { return v >= 0 && v <= (int64_t)0x7fffffff; }

}  // namespace

extern "C" int lc_stats_limit(int which) { return which == 0 ? LC_STATS_MAX_EIG : which == 1 ? LC_STATS_REDUCE_SCRATCH : -1; }

extern "C" int lc_stats_jacobi_pair(int k, int step, int slot, int* pq) {
    if (!pq || k < 2) return LC_EINVAL;
    const int n = k + (k & 1);
    if (step < 0 || step >= n - 1 || slot < 0 || slot >= n / 2) return LC_EINVAL;
    int p, q;
    lc_jacobi_pair_of(k, step, slot, p, q);
    pq[0] = p;
    pq[1] = q < k ? q : -1;
    return LC_OK;
}

extern "C" int lc_stats_gemm_f64(const double* P, int64_t p_rs, int64_t p_ks, const double* Q, int64_t q_rs, int64_t q_ks,
                                 double* C, int64_t ldc, int M, int N, int K, lc_stream_t s) {
    if (!P || !Q || !C || M < 1 || N < 1 || K < 1 || ldc < N) return LC_EINVAL;
    if (p_rs < 0 || p_ks < 0 || q_rs < 0 || q_ks < 0) return LC_EINVAL;
    const int gy = (M + TM - 1) / TM, gx = (N + TN - 1) / TN;
    if (gy > 65535) return LC_EUNSUP;
    const Operand p{P, nullptr, p_rs, p_ks, M, M}, q{Q, nullptr, q_rs, q_ks, N, N};
    gemm_kernel<<<dim3(gx, gy), NT, 0, lc_s(s)>>>(p, q, C, ldc, K);
    return lc_launch_status();
}

extern "C" int64_t lc_stats_mmd_partials(int num_subsets, int m) {
    if (num_subsets < 1 || m < 1) return 0;
    const int64_t t = (m + TM - 1) / TM;
    return (int64_t)num_subsets * 3 * t * t;
}

extern "C" int lc_stats_mmd_f64(const double* fx, int nx, const double* fy, int ny, int width, const int32_t* table,
                                int num_subsets, int m, double* partial, double* out, lc_stream_t s) {
    if (!fx || !fy || !table || !partial || !out || nx < 1 || ny < 1 || width < 1 || num_subsets < 1 || m < 1) return LC_EINVAL;
    const int t = (m + TM - 1) / TM;
    if (t > 65535 || (int64_t)num_subsets * 3 > 65535 || !fits_i32((int64_t)t * t * 2)) return LC_EUNSUP;
    mmd_kernel<<<dim3(t, t, num_subsets * 3), NT, 0, lc_s(s)>>>(fx, nx, fy, ny, table, m, width, partial);
    mmd_sum_kernel<<<dim3(num_subsets, 2), NT, 0, lc_s(s)>>>(partial, t * t, out);
    return lc_launch_status();
}

extern "C" int lc_stats_center_f64(const double* X, int n, int d, double* mean, double* A, lc_stream_t s) {
    if (!X || !mean || !A || n < 2 || d < 1) return LC_EINVAL;
    const int64_t total = (int64_t)n * d;
    colmean_kernel<<<(d + 63) / 64, NT, 0, lc_s(s)>>>(X, n, d, mean);
    const int64_t blocks = (total + NT - 1) / NT;
    center_kernel<<<(int)(blocks < 4096 ? blocks : 4096), NT, 0, lc_s(s)>>>(X, mean, total, d, sqrt((double)(n - 1)), A);
    return lc_launch_status();
}

extern "C" int lc_stats_reduce_f64(const double* a, int64_t sa, const double* b, int64_t sb, int64_t n, int mode,
                                   double* scratch, double* out, lc_stream_t s) {
    if (!a || !scratch || !out || n < 1 || sa < 1 || mode < 0 || mode > 3 || (mode == 2 && (!b || sb < 1))) return LC_EINVAL;
    int64_t chunk = (n + LC_STATS_REDUCE_SCRATCH - 1) / LC_STATS_REDUCE_SCRATCH;
    if (chunk < 4 * NT) chunk = 4 * NT;
    const int blocks = (int)((n + chunk - 1) / chunk);
    reduce_kernel<<<blocks, NT, 0, lc_s(s)>>>(a, sa, b, sb, n, chunk, mode, scratch);
    reduce_kernel<<<1, NT, 0, lc_s(s)>>>(scratch, 1, nullptr, 0, blocks, blocks, 0, out);
    return lc_launch_status();
}

extern "C" int lc_stats_scale_rows_f64(const double* V, const double* lam, int k, double cut, double* out, lc_stream_t s) {
    if (!V || !lam || !out || k < 1 || !(cut >= 0.0)) return LC_EINVAL;
    scale_rows_kernel<<<k, NT, 0, lc_s(s)>>>(V, lam, k, cut, out);
    return lc_launch_status();
}

extern "C" int lc_stats_jacobi_init(double* V, int k, lc_stream_t s) {
    if (!V || k < 1) return LC_EINVAL;
    if (k > LC_STATS_MAX_EIG) return LC_EUNSUP;
    identity_kernel<<<k, NT, 0, lc_s(s)>>>(V, k);
    return lc_launch_status();
}

extern "C" int lc_stats_jacobi_sweep(double* W, double* V, int k, double tol, double atol, const double* fro2, int32_t* flag,
                                     lc_stream_t s) {
    if (!W || !flag || k < 1 || !(tol >= 0.0) || !(atol >= 0.0)) return LC_EINVAL;
    if (k > LC_STATS_MAX_EIG) return LC_EUNSUP;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), lc_s(s));
    if (e != hipSuccess) return (int)e;
    const int n = k + (k & 1);
    for (int step = 0; step < n - 1; ++step) {
        if (k <= NT) jacobi_step_kernel<1><<<n / 2, NT, 0, lc_s(s)>>>(W, V, k, step, tol, atol, fro2, flag);
        else if (k <= 4 * NT) jacobi_step_kernel<4><<<n / 2, NT, 0, lc_s(s)>>>(W, V, k, step, tol, atol, fro2, flag);
        else jacobi_step_kernel<16><<<n / 2, NT, 0, lc_s(s)>>>(W, V, k, step, tol, atol, fro2, flag);
    }
    return lc_launch_status();
}

extern "C" int lc_stats_jacobi_values(const double* W, int k, double* lam, lc_stream_t s) {
    if (!W || !lam || k < 1) return LC_EINVAL;
    row_norm_kernel<<<k, NT, 0, lc_s(s)>>>(W, k, lam);
    return lc_launch_status();
}
