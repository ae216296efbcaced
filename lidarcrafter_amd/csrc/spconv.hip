// Sparse 3-D convolution of the Frechet Sparse Volume Distance: the coordinate hash, the three
// kinds of neighbour table, one output-stationary convolution kernel and the depth-sector means of the features --
// what the reference's MinkUNet (lidargen/metrics/models/minkowskinet/model.py) takes from torchsparse 1.4.0.
//   sp_hash_insert_kernel  key = batch << 54 | x << 36 | y << 18 | z (18 bits each, 9 for the batch: non-negative as an
//                          int64) into an open-addressing table of 64-bit keys through atomicMin, linear probing, the
//                          smaller key keeps a contested slot: one arrangement whatever the order of the threads.
//   sp_hash_value_kernel   value = the row (the largest of equal ones), once the keys stand.  (The key, the probe and
//                          the range rule: spconv_hash.h.)
//   sp_map_kernel          nbr[j][k] = row of C[j] + offset_k in the table or -1.  A query with a component below 0 or
//                          above LC_SPCONV_MAX_COORD is absent before any key is formed: nothing wraps into a
//                          neighbouring field of the key, so no cloud sees another cloud's voxel.
//       kind 0  ks 3, stride 1:  offsets {-s, 0, s}^3, x fastest, K = 27, queried in the table of the same level
//       kind 1  ks 2, stride 2:  offsets {0, s}^3, z fastest, K = 8: the children of a coarse voxel, fine table
//       kind 2  the transpose of kind 1: for a fine voxel the one (j, k) with C_fine = C_coarse[j] + offset_k, coarse table
//   sp_conv_kernel         y[j, c0 : c0 + Co] = act(sum_k x[nbr[j,k], :] w[k] + b + res[j]).  One block = SP_T output rows,
//                          4 waves of 16 rows each, all Co columns.  Per offset k and chunk of <= 64 input channels the
//                          gathered rows (128-bit global loads, zeros for -1) and the chunk of w[k] are staged in LDS;
//                          v_mfma_f32_16x16x4_f32 with w as the A operand (rows = output channels) and the gathered rows
//                          as B (columns = output rows): a lane ends with 4 consecutive channels of one row, one 128-bit
//                          store.  An offset no row of the block has is not staged, one no row of a wave has is not
//                          multiplied: both only leave out exact zeros.  The f32-input MFMA is a k-ordered fma chain;
//                          an offset's product (<= 192 terms) is summed on its own and then added to the row's total
//                          (the error of one long chain over 27 x 192 terms grows with its length), in the fixed order
//                          (offset, channel): a row's bits depend on its own neighbours only, whatever batch or tile it
//                          is in.  No atomics.
//   sp_sector_kernel       one block per cloud: mean of the coordinates from exact integer sums, d = |c - mean| * voxel,
//                          16 depth sectors; thread (group g, channel c) sums rows g, g + G, ... into its own LDS slots,
//                          the G partial sums are added in the order of g: no float atomics, the same bits every run.
#include "common.h"
#include "spconv_hash.h"

namespace {

constexpr int SP_T = LC_SPCONV_TILE;          // output rows per block
constexpr int SP_CK = 64;                     // input channels staged at a time
constexpr int SP_XS = SP_CK + 4;              // row stride of the gathered tile in LDS (16-byte aligned rows)
constexpr int SP_MAXCO = 128;

__global__ __launch_bounds__(256) void sp_hash_clear_kernel(unsigned long long* keys, int32_t* vals, unsigned cap) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < cap) {
        keys[i] = SP_EMPTY;
        vals[i] = -1;
    }
}

// Ordered insertion (Amble & Knuth 1974): of two keys that meet in a slot the smaller one stays and the thread carries the
// larger one on (the empty marker is the largest value, so one atomicMin does both).  Every stored key then has only
// smaller keys between its home slot and its own, and a set of keys has exactly one such arrangement: the table's bytes
// do not depend on the order in which the threads arrive.  (With a plain compare-and-swap two keys of one home slot took
// the slots in the order of arrival: the same maps, other bytes from run to run.)  sp_find needs no change: a key is
// still reachable from its home slot over occupied slots.
__global__ __launch_bounds__(256) void sp_hash_insert_kernel(const int32_t* __restrict__ coords, int N,
                                                            unsigned long long* keys, unsigned cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int x = coords[4 * i], y = coords[4 * i + 1], z = coords[4 * i + 2], b = coords[4 * i + 3];
    if (!sp_in_range(b, x, y, z)) return;     // (the host entry refuses such inputs; a row outside is never found)
    unsigned long long key = sp_key(b, x, y, z);
    const unsigned mask = cap - 1;
    unsigned h = sp_slot(key, mask);
    for (unsigned probe = 0; probe < cap; ++probe, h = (h + 1) & mask) {
        const unsigned long long prev = atomicMin(&keys[h], key);
        if (prev == SP_EMPTY || prev == key) return;
        if (prev > key) key = prev;           // the slot keeps the smaller key, the displaced one moves on
    }
}

// the rows of the finished keys, in a launch of its own (a key may move while keys are still being inserted)
__global__ __launch_bounds__(256) void sp_hash_value_kernel(const int32_t* __restrict__ coords, int N,
                                                           const unsigned long long* __restrict__ keys, int32_t* vals,
                                                           unsigned cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int x = coords[4 * i], y = coords[4 * i + 1], z = coords[4 * i + 2], b = coords[4 * i + 3];
    if (!sp_in_range(b, x, y, z)) return;
    const unsigned long long key = sp_key(b, x, y, z);
    const unsigned mask = cap - 1;
    unsigned h = sp_slot(key, mask);
    for (unsigned probe = 0; probe < cap; ++probe, h = (h + 1) & mask) {
        const unsigned long long k = keys[h];
        if (k == key) {
            atomicMax(&vals[h], i);           // (rows are unique by contract; of equal ones the last wins, every run)
            return;
        }
        if (k == SP_EMPTY) return;
    }
}

// one thread per (row j, offset k)
__global__ __launch_bounds__(256) void sp_map_kernel(const int32_t* __restrict__ coords, int M, int kind, int s,
                                                    const unsigned long long* __restrict__ keys,
                                                    const int32_t* __restrict__ vals, unsigned cap, int n_table,
                                                    int32_t* __restrict__ nbr) {
    const int K = kind == 0 ? 27 : 8;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)M * K) return;
    const int j = (int)(t / K), k = (int)(t % K);
    const int x = coords[4 * j], y = coords[4 * j + 1], z = coords[4 * j + 2], b = coords[4 * j + 3];
    int r = -1;
    if (kind == 0) {
        r = sp_find(keys, vals, cap, b, x + (k % 3 - 1) * s, y + (k / 3 % 3 - 1) * s, z + (k / 9 - 1) * s);
    } else {
        const int ox = (k >> 2) * s, oy = ((k >> 1) & 1) * s, oz = (k & 1) * s;
        if (kind == 1) {
            r = sp_find(keys, vals, cap, b, x + ox, y + oy, z + oz);
        } else if (x >= 0 && y >= 0 && z >= 0) {
            const int s2 = 2 * s, qx = x - ox, qy = y - oy, qz = z - oz;
            if (qx >= 0 && qy >= 0 && qz >= 0 && qx % s2 == 0 && qy % s2 == 0 && qz % s2 == 0)
                r = sp_find(keys, vals, cap, b, qx, qy, qz);
        }
    }
    nbr[t] = (r >= 0 && r < n_table) ? r : -1;
}

// C/D of the 16x16 MFMA: register v of lane l is row 4 (l >> 4) + v, column l & 15.  A: lane holds A[l & 15][l >> 4],
// B: B[l >> 4][l & 15].  Here rows = output channels, columns = output rows of the tile, and the instruction's four k are
// channels 16 q + 4 g + t (g = l >> 4) of step (q, t): lane (., g) reads channels 16 q + 4 g .. + 3 of its row as one quad.
template <int NCT>   // Co / 16
__global__ __launch_bounds__(256) void sp_conv_kernel(const float* __restrict__ x, long long ldx,
                                                     const int32_t* __restrict__ nbr, int n_in,
                                                     const float* __restrict__ w, const float* __restrict__ bias,
                                                     const float* __restrict__ res, long long ldr, float* __restrict__ y,
                                                     long long ldy, int M, int Ci, int K, int relu) {
    constexpr int Co = NCT * 16, WS = Co + 4;
    __shared__ __attribute__((aligned(16))) float xs[SP_T * SP_XS];
    __shared__ __attribute__((aligned(16))) float ws[SP_CK * WS];
    __shared__ int nb[SP_T * 27];
    __shared__ int wave_has[4][27];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * SP_T;
    const int col = lane & 15, g = lane >> 4;

    for (int i = tid; i < SP_T * K; i += 256) {
        const int r = i / K, k = i - r * K, j = row0 + r;
        int v = -1;
        if (j < M) {
            v = nbr ? nbr[(size_t)j * K + k] : j;
            if (v < 0 || v >= n_in) v = -1;
        }
        nb[r * 27 + k] = v;
    }
    __syncthreads();
    if (tid < 4 * 32) {
        const int wv = tid >> 5, k = tid & 31;
        if (k < K) {
            int any = 0;
            for (int r = 0; r < 16; ++r) any |= nb[(wv * 16 + r) * 27 + k] >= 0;
            wave_has[wv][k] = any;
        }
    }
    __syncthreads();

    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int Cie = Ci < 16 ? 16 : Ci;        // Ci = 4 (the stem): zero-padded to one step of 16 in LDS
    for (int k = 0; k < K; ++k) {
        if (!(wave_has[0][k] | wave_has[1][k] | wave_has[2][k] | wave_has[3][k])) continue;   // block-uniform
        const bool mine = wave_has[wave][k] != 0;
        f32x4 part[NCT];                      // one offset's product: summed on its own, then added to the row's total
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) part[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < Cie; c0 += SP_CK) {
            const int ck = Cie - c0 < SP_CK ? Cie - c0 : SP_CK, q4 = ck >> 2;
            __syncthreads();                  // the previous chunk has been read
            for (int i = tid; i < SP_T * q4; i += 256) {
                const int r = i / q4, c4 = (i - r * q4) * 4;
                const int src = nb[r * 27 + k];
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (src >= 0 && c0 + c4 < Ci) v = *reinterpret_cast<const f32x4*>(x + (size_t)src * ldx + c0 + c4);
                *reinterpret_cast<f32x4*>(&xs[r * SP_XS + c4]) = v;
            }
            const float* wk = w + ((size_t)k * Ci + c0) * Co;
            for (int i = tid; i < ck * (Co / 4); i += 256) {
                const int r = i / (Co / 4), c4 = (i - r * (Co / 4)) * 4;
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (c0 + r < Ci) v = *reinterpret_cast<const f32x4*>(wk + (size_t)r * Co + c4);
                *reinterpret_cast<f32x4*>(&ws[r * WS + c4]) = v;
            }
            __syncthreads();
            if (mine) {
                for (int q = 0; q < (ck >> 4); ++q) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(&xs[(wave * 16 + col) * SP_XS + 16 * q + 4 * g]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float* wr = &ws[(16 * q + 4 * g + t) * WS + col];
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct)
                            part[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[16 * ct], bv[t], part[ct], 0, 0, 0);
                    }
                }
            }
        }
        if (mine) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] += part[ct];
        }
    }

    const int j = row0 + wave * 16 + col;
    if (j < M) {
        float* yr = y + (size_t)j * ldy;
        const float* rr = res ? res + (size_t)j * ldr : nullptr;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int c = 16 * ct + 4 * g;
            f32x4 o = acc[ct];
            if (bias) o += *reinterpret_cast<const f32x4*>(bias + c);
            if (rr) o += *reinterpret_cast<const f32x4*>(rr + c);
            if (relu) {
#pragma unroll
                for (int v = 0; v < 4; ++v) o[v] = fmaxf(o[v], 0.f);
            }
            *reinterpret_cast<f32x4*>(yr + c) = o;
        }
    }
}

constexpr int SP_SECT = 16;

__global__ __launch_bounds__(256) void sp_sector_kernel(const float* __restrict__ f, long long ldf,
                                                       const int32_t* __restrict__ coords,
                                                       const int32_t* __restrict__ offsets, int C,
                                                       const float* __restrict__ edges, float voxel,
                                                       float* __restrict__ out) {
    extern __shared__ float sm[];             // [G][16][C] sums, then [G][16] counts
    __shared__ long long isum[4][3];
    __shared__ float mean[3];
    __shared__ float ed[SP_SECT + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
    const int G = 256 / C;
    float* cnt = sm + G * SP_SECT * C;
    for (int i = tid; i < G * SP_SECT * C + G * SP_SECT; i += 256) sm[i] = 0.f;
    if (tid <= SP_SECT) ed[tid] = edges[tid];
    long long s0 = 0, s1 = 0, s2 = 0;
    for (int i = lo + tid; i < hi; i += 256) {
        s0 += coords[4 * i];
        s1 += coords[4 * i + 1];
        s2 += coords[4 * i + 2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if ((tid & 63) == 0) {
        isum[tid >> 6][0] = s0;
        isum[tid >> 6][1] = s1;
        isum[tid >> 6][2] = s2;
    }
    __syncthreads();
    if (tid < 3 && n > 0)
        mean[tid] = (float)((double)(isum[0][tid] + isum[1][tid] + isum[2][tid] + isum[3][tid]) / (double)n);
    __syncthreads();
    const int grp = tid / C, c = tid - grp * C;
    if (grp < G) {
        for (int i = lo + grp; i < hi; i += G) {
            const float cx = __fsub_rn((float)coords[4 * i], mean[0]), cy = __fsub_rn((float)coords[4 * i + 1], mean[1]),
                        cz = __fsub_rn((float)coords[4 * i + 2], mean[2]);
            const float d = __fmul_rn(__fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)),
                                                           __fmul_rn(cz, cz))), voxel);
            int sct = -1;
#pragma unroll
            for (int e = 0; e < SP_SECT; ++e)
                if (d >= ed[e] && d < ed[e + 1]) sct = e;
            if (sct >= 0) {
                sm[(grp * SP_SECT + sct) * C + c] += f[(size_t)i * ldf + c];
                if (c == 0) cnt[grp * SP_SECT + sct] += 1.f;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < SP_SECT * C; i += 256) {
        const int sct = i / C;
        float s = 0.f, m = 0.f;
        for (int gg = 0; gg < G; ++gg) {
            s += sm[gg * SP_SECT * C + i];
            m += cnt[gg * SP_SECT + sct];
        }
        out[(size_t)b * SP_SECT * C + i] = m > 0.f ? s / m : 0.f;
    }
}

bool sp_width_in(int c) { return c == 4 || c == 16 || c == 32 || c == 48 || c == 64 || c == 96 || c == 128 || c == 192; }
bool sp_width_out(int c) { return c == 16 || c == 32 || c == 48 || c == 64 || c == 128; }

}  // namespace

extern "C" int64_t lc_spconv_hash_bytes(int N) {
    if (N < 1 || N > LC_SPCONV_MAX_ROWS) return 0;
    return (int64_t)sp_capacity(N) * 12;
}

extern "C" int lc_spconv_hash_build(const int32_t* coords, int N, int max_coord, int n_batch, void* table,
                                    int64_t table_bytes, lc_stream_t s) {
    if (!coords || !table || N < 1 || max_coord < 0 || n_batch < 1) return LC_EINVAL;
    if (N > LC_SPCONV_MAX_ROWS || max_coord > LC_SPCONV_MAX_COORD || n_batch - 1 > LC_SPCONV_MAX_BATCH) return LC_EUNSUP;
    const unsigned cap = sp_capacity(N);
    if (table_bytes < (int64_t)cap * 12) return LC_EINVAL;
    unsigned long long* keys = static_cast<unsigned long long*>(table);
    int32_t* vals = reinterpret_cast<int32_t*>(keys + cap);
    hipLaunchKernelGGL(sp_hash_clear_kernel, dim3((cap + 255) / 256), dim3(256), 0, lc_s(s), keys, vals, cap);
    hipLaunchKernelGGL(sp_hash_insert_kernel, dim3((N + 255) / 256), dim3(256), 0, lc_s(s), coords, N, keys, cap);
    hipLaunchKernelGGL(sp_hash_value_kernel, dim3((N + 255) / 256), dim3(256), 0, lc_s(s), coords, N, keys, vals, cap);
    return lc_launch_status();
}

extern "C" int lc_spconv_map(const int32_t* coords, int M, int kind, int stride, const void* table, int n_table,
                             int32_t* nbr, lc_stream_t s) {
    if (!coords || !table || !nbr || M < 1 || n_table < 1 || stride < 1 || kind < 0 || kind > 2) return LC_EINVAL;
    if (M > LC_SPCONV_MAX_ROWS || n_table > LC_SPCONV_MAX_ROWS || stride > LC_SPCONV_MAX_STRIDE) return LC_EUNSUP;
    const unsigned cap = sp_capacity(n_table);
    const unsigned long long* keys = static_cast<const unsigned long long*>(table);
    const int32_t* vals = reinterpret_cast<const int32_t*>(keys + cap);
    const long long total = (long long)M * (kind == 0 ? 27 : 8);
    hipLaunchKernelGGL(sp_map_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, lc_s(s), coords, M, kind,
                       stride, keys, vals, cap, n_table, nbr);
    return lc_launch_status();
}

extern "C" int lc_spconv_fwd(const float* x, int64_t ldx, const int32_t* nbr, int n_in, const float* w, const float* b,
                             const float* res, int64_t ldr, float* y, int64_t ldy, int y_col, int M, int Ci, int Co,
                             int K, int relu, lc_stream_t s) {
    if (!x || !w || !y || M < 1 || n_in < 1 || Ci < 1 || Co < 1 || y_col < 0) return LC_EINVAL;
    if (K != 1 && K != 8 && K != 27) return LC_EUNSUP;
    if (K != 1 && !nbr) return LC_EINVAL;
    if (!nbr && n_in < M) return LC_EINVAL;
    if (!sp_width_in(Ci) || !sp_width_out(Co) || Co > SP_MAXCO) return LC_EUNSUP;
    if (M > LC_SPCONV_MAX_ROWS || n_in > LC_SPCONV_MAX_ROWS) return LC_EUNSUP;
    if (ldx < Ci || ldy < (int64_t)y_col + Co || (res && ldr < Co)) return LC_EINVAL;
    if ((ldx & 3) || (ldy & 3) || (y_col & 3) || (res && (ldr & 3))) return LC_EUNSUP;   // rows are read and written as quads
    if (!lc_aligned16(x) || !lc_aligned16(w) || !lc_aligned16(y) || (b && !lc_aligned16(b)) || (res && !lc_aligned16(res)))
        return LC_EUNSUP;
    float* yo = y + y_col;
    const dim3 grid((M + SP_T - 1) / SP_T), block(256);
#define SP_LAUNCH(NCT)                                                                                              \
    hipLaunchKernelGGL(sp_conv_kernel<NCT>, grid, block, 0, lc_s(s), x, (long long)ldx, nbr, n_in, w, b, res,        \
                       (long long)ldr, yo, (long long)ldy, M, Ci, K, relu ? 1 : 0)
    switch (Co / 16) {
        case 1: SP_LAUNCH(1); break;
        case 2: SP_LAUNCH(2); break;
        case 3: SP_LAUNCH(3); break;
        case 4: SP_LAUNCH(4); break;
        case 8: SP_LAUNCH(8); break;
        default: return LC_EUNSUP;
    }
#undef SP_LAUNCH
    return lc_launch_status();
}

extern "C" int lc_spconv_sector_means(const float* f, int64_t ldf, const int32_t* coords, const int32_t* offsets,
                                      int n_clouds, int C, const float* edges, float voxel, float* out, lc_stream_t s) {
    if (!f || !coords || !offsets || !edges || !out || n_clouds < 1 || C < 1 || ldf < C) return LC_EINVAL;
    if (C > 256 || n_clouds > 65535) return LC_EUNSUP;
    const int G = 256 / C;
    const size_t lds = ((size_t)G * SP_SECT * C + (size_t)G * SP_SECT) * sizeof(float);
    hipLaunchKernelGGL(sp_sector_kernel, dim3(n_clouds), dim3(256), lds, lc_s(s), f, (long long)ldf, coords, offsets, C,
                       edges, voxel, out);
    return lc_launch_status();
}
