// Chamfer distance, backward: lidargen/metrics/modules/chamfer3D/chamfer3D.cu:155-195 (NmDistanceGradKernel, launched
// once per direction) and its 2-D twin chamfer2D.cu:145-171.  The reference scatters with float atomicAdd into
// zero-filled buffers; here every output row is a gather over an inverse table, summed in a fixed order, so the bits
// are the same alone, in any batch and from run to run.
//
// Terms, every operation rounded to float32 on its own (no contraction), as the reference writes them:
//   g = grad * 2,  t = g * (own - other),  the point itself receives t, its nearest neighbour -(t).
// Row j of grad_xyz1 (per batch entry, per coordinate) therefore has
//   its direct term       d   = (grad_dist1[j] * 2) * (xyz1[j] - xyz2[idx1[j]])
//   its scattered terms   s_i = -((grad_dist2[k_i] * 2) * (xyz2[k_i] - xyz1[j]))   for k_0 < k_1 < ... < k_{L-1},
//                               the rows k of xyz2 with idx2[k] == j in ASCENDING k.
// grad_xyz2 is the same with the roles of the two clouds exchanged.
//
// Summation order of one row (it depends on idx1, idx2, N and M only):
//   a = +0 + d                                      (the reference's zero-filled accumulator: a term -0 reads +0)
//   L <= 32:  row = (((a + s_0) + s_1) + ...) + s_{L-1}
//   L  > 32:  row = a + T, where lane t of 256 holds q_t = ((+0 + s_t) + s_{t+256}) + s_{t+512} + ...  (q_t = +0 for
//             t >= L) and T is the tree  for h = 128, 64, ..., 1:  q_t = q_t + q_{t+h}  (t < h),  T = q_0.
// An index outside its cloud (the forward writes none) adds no term.
//
// The inverse table, built on the device with integer work only (no host read, nothing that depends on timing):
//   entries e = 0 .. B N - 1 are the rows of xyz1, key b M + idx1 (the flat row of xyz2 they point at); entries
//   e = B N .. B (N + M) - 1 the rows of xyz2, key B M + b N + idx2; an index outside its cloud gets the key B (N + M),
//   behind every row.  One stable radix sort of (key, e) over the used bits (rocPRIM; equal keys keep ascending e, i.e.
//   ascending source index), then seg[r] = the first sorted position whose key is >= r, by binary search, r = 0 ..
//   B (N + M).  Flat row r of xyz2 reads the sorted entries seg[r] .. seg[r + 1], flat row r of xyz1 those of B M + r.
// One thread per output row; a row with a long segment (a collapsed cloud puts every source on one target) is summed
// by its whole block, 256 lanes striding the segment with coalesced reads of the table, so no thread walks more than
// ceil(L / 256) terms.  Gather bound.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace {

#pragma clang fp contract(off)

constexpr int CB_BLOCK = 256;   // rows per block = lanes of the long-segment tree
constexpr int CB_SERIAL = 32;   // the longest segment one thread adds serially

// (key, entry) of both directions; rows1 = B N, rows2 = B M
__global__ __launch_bounds__(256) void chamfer_bwd_key_kernel(const int* __restrict__ idx1, const int* __restrict__ idx2,
                                                             int rows1, int rows2, int n, int m,
                                                             unsigned* __restrict__ key, unsigned* __restrict__ val) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)rows1 + rows2;
    if (e >= total) return;
    unsigned k = (unsigned)total;
    if (e < rows1) {
        const int j = idx1[e];
        if ((unsigned)j < (unsigned)m) k = (unsigned)((e / n) * m + j);
    } else {
        const long long e2 = e - rows1;
        const int j = idx2[e2];
        if ((unsigned)j < (unsigned)n) k = (unsigned)(rows2 + (e2 / m) * n + j);
    }
    key[e] = k;
    val[e] = (unsigned)e;
}

// seg[r] = the first position of the sorted keys that holds a key >= r, r = 0 .. total
__global__ __launch_bounds__(256) void chamfer_bwd_seg_kernel(const unsigned* __restrict__ skey, int total,
                                                             int* __restrict__ seg) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > total) return;
    int lo = 0, hi = total;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (skey[mid] < (unsigned)r) lo = mid + 1; else hi = mid;
    }
    seg[r] = lo;
}

// own [rows, D] <- its direct terms and the terms of the entries order[seg[r] .. seg[r + 1]) - src_base, rows of `other`
template <int D>
__global__ __launch_bounds__(CB_BLOCK) void chamfer_bwd_kernel(
    const float* __restrict__ own, const float* __restrict__ other, const float* __restrict__ g_own,
    const int* __restrict__ idx_own, const float* __restrict__ g_other, const unsigned* __restrict__ order,
    const int* __restrict__ seg, float* __restrict__ out, int rows, int n, int m, int others, unsigned src_base,
    int entries) {
    __shared__ float red[D][CB_BLOCK];
    __shared__ unsigned long long long_mask[CB_BLOCK / 64];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * CB_BLOCK;
    const long long r = r0 + tid;
    const bool valid = r < rows;
    float x[D], acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { x[d] = 0.f; acc[d] = 0.f; }
    int lo = 0, hi = 0;
    if (valid) {
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = own[r * D + d];
        const int j2 = idx_own[r];
        if ((unsigned)j2 < (unsigned)m) {
            const long long o = (r / n) * m + j2;
            const float g = g_own[r] * 2.f;
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += g * (x[d] - other[o * D + d]);
        }
        lo = seg[r];
        hi = seg[r + 1];
        lo = lo < 0 ? 0 : (lo > entries ? entries : lo);
        hi = hi < lo ? lo : (hi > entries ? entries : hi);
    }
    const bool is_long = hi - lo > CB_SERIAL;
    if (valid && !is_long) {
        for (int p = lo; p < hi; ++p) {
            const unsigned src = order[p] - src_base;
            if (src >= (unsigned)others) continue;
            const float g = g_other[src] * 2.f;
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += -(g * (other[(long long)src * D + d] - x[d]));
        }
#pragma unroll
        for (int d = 0; d < D; ++d) out[r * D + d] = acc[d];
    }
    if (!__syncthreads_or(is_long)) return;

    const unsigned long long mine = __ballot(is_long);
    if ((tid & 63) == 0) long_mask[tid >> 6] = mine;
    __syncthreads();
    for (int w = 0; w < CB_BLOCK / 64; ++w) {
        unsigned long long mask = long_mask[w];
        while (mask) {
            const int owner = w * 64 + __builtin_ctzll(mask);
            mask &= mask - 1;
            const long long R = r0 + owner;              // < rows: only valid rows are long
            int slo = seg[R], shi = seg[R + 1];
            slo = slo < 0 ? 0 : (slo > entries ? entries : slo);
            shi = shi < slo ? slo : (shi > entries ? entries : shi);
            float xr[D], q[D];
#pragma unroll
            for (int d = 0; d < D; ++d) { xr[d] = own[R * D + d]; q[d] = 0.f; }
            // no branch around the gathers, so that the loads of four rounds are in flight together; a foreign entry
            // adds +0, which changes no bit (q_t is never -0: it starts at +0)
#pragma unroll 4
            for (int p = slo + tid; p < shi; p += CB_BLOCK) {
                const unsigned v = order[p] - src_base;
                const bool ok = v < (unsigned)others;
                const unsigned src = ok ? v : 0u;
                const float g = g_other[src] * 2.f;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float t = -(g * (other[(long long)src * D + d] - xr[d]));
                    q[d] += ok ? t : 0.f;
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d) red[d][tid] = q[d];
            __syncthreads();
            for (int h = CB_BLOCK / 2; h > 0; h >>= 1) {
                if (tid < h) {
#pragma unroll
                    for (int d = 0; d < D; ++d) red[d][tid] = red[d][tid] + red[d][tid + h];
                }
                __syncthreads();
            }
            if (tid == owner) {
#pragma unroll
                for (int d = 0; d < D; ++d) out[R * D + d] = acc[d] + red[d][0];
            }
            __syncthreads();
        }
    }
}

struct CbScratch {
    unsigned* key_a; unsigned* key_b; unsigned* val_a; unsigned* val_b; int* seg; void* tmp; size_t tmp_bytes;
};

size_t cb_align256(size_t v) { return (v + 255) / 256 * 256; }

size_t cb_carve(void* base, long long total, CbScratch* s) {
    char* p = static_cast<char*>(base);
    auto take = [&](size_t bytes) { char* r = p; p += cb_align256(bytes); return (void*)r; };
    void* ka = take((size_t)total * 4);
    void* kb = take((size_t)total * 4);
    void* va = take((size_t)total * 4);
    void* vb = take((size_t)total * 4);
    void* sg = take(((size_t)total + 1) * 4);
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tb, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                    (unsigned*)nullptr, (size_t)total);
    void* tmp = take(tb);
    if (s) *s = CbScratch{(unsigned*)ka, (unsigned*)kb, (unsigned*)va, (unsigned*)vb, (int*)sg, tmp, tb};
    return (size_t)(p - static_cast<char*>(base));
}

// B N + B M entries and seg[r + 1] stay int32
bool cb_sizes_ok(int B, int N, int M) { return (long long)B * N + (long long)B * M <= 2147483646ll; }

template <int D>
int chamfer_bwd(const float* xyz1, const float* xyz2, const float* grad_dist1, const float* grad_dist2,
                const int32_t* idx1, const int32_t* idx2, int B, int N, int M, float* grad_xyz1, float* grad_xyz2,
                void* scratch, lc_stream_t s) {
    if (!xyz1 || !xyz2 || !grad_dist1 || !grad_dist2 || !idx1 || !idx2 || !grad_xyz1 || !grad_xyz2 || !scratch ||
        B <= 0 || N <= 0 || M <= 0)
        return LC_EINVAL;
    if (!cb_sizes_ok(B, N, M)) return LC_EUNSUP;
    const int rows1 = B * N, rows2 = B * M, total = rows1 + rows2;
    CbScratch w;
    cb_carve(scratch, total, &w);
    hipStream_t st = lc_s(s);
    const unsigned eblocks = (unsigned)(((long long)total + 256) / 256);          // total + 1 threads: the seg kernel's
    hipLaunchKernelGGL(chamfer_bwd_key_kernel, dim3(eblocks), dim3(256), 0, st, idx1, idx2, rows1, rows2, N, M, w.key_a,
                       w.val_a);
    int bits = 1;
    while (((long long)total >> bits) != 0) ++bits;                                // keys 0 .. total
    size_t tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.key_a, w.key_b, w.val_a, w.val_b, (size_t)total, 0, bits, st) != hipSuccess)
        return lc_launch_status() ? lc_launch_status() : LC_EUNSUP;
    hipLaunchKernelGGL(chamfer_bwd_seg_kernel, dim3(eblocks), dim3(256), 0, st, w.key_b, total, w.seg);
    hipLaunchKernelGGL(chamfer_bwd_kernel<D>, dim3((unsigned)((rows1 + CB_BLOCK - 1) / CB_BLOCK)), dim3(CB_BLOCK), 0, st, xyz1,
                       xyz2, grad_dist1, idx1, grad_dist2, w.val_b, w.seg + rows2, grad_xyz1, rows1, N, M, rows2,
                       (unsigned)rows1, total);
    hipLaunchKernelGGL(chamfer_bwd_kernel<D>, dim3((unsigned)((rows2 + CB_BLOCK - 1) / CB_BLOCK)), dim3(CB_BLOCK), 0, st, xyz2,
                       xyz1, grad_dist2, idx2, grad_dist1, w.val_b, w.seg, grad_xyz2, rows2, M, N, rows1, 0u, total);
    return lc_launch_status();
}

}  // namespace

extern "C" int64_t lc_chamfer_bwd_scratch_bytes(int B, int N, int M) {
    if (B < 1 || N < 1 || M < 1 || !cb_sizes_ok(B, N, M)) return 0;
    return (int64_t)cb_carve(nullptr, (long long)B * N + (long long)B * M, nullptr);
}

extern "C" int lc_chamfer3d_bwd(const float* xyz1, const float* xyz2, const float* grad_dist1, const float* grad_dist2,
                                const int32_t* idx1, const int32_t* idx2, int B, int N, int M, float* grad_xyz1,
                                float* grad_xyz2, void* scratch, lc_stream_t s) {
    return chamfer_bwd<3>(xyz1, xyz2, grad_dist1, grad_dist2, idx1, idx2, B, N, M, grad_xyz1, grad_xyz2, scratch, s);
}

extern "C" int lc_chamfer2d_bwd(const float* xyz1, const float* xyz2, const float* grad_dist1, const float* grad_dist2,
                                const int32_t* idx1, const int32_t* idx2, int B, int N, int M, float* grad_xyz1,
                                float* grad_xyz2, void* scratch, lc_stream_t s) {
    return chamfer_bwd<2>(xyz1, xyz2, grad_dist1, grad_dist2, idx1, idx2, B, N, M, grad_xyz1, grad_xyz2, scratch, s);
}
