// Chamfer distance of BEV cell sets on their grid: what eval_utils.compute_mmd needs.
//   pcd2bev_bin (lidargen/metrics/metric_utils.py:261-284) turns every cloud into the unique cells of an nx x ny grid,
//   stored as cell / (nx, ny); chamfer_2DDist on two such sets is a brute-force nearest neighbour.  On the grid the squared
//   nearest-neighbour distance from EVERY cell to a set is one exact integer distance transform of the set's occupancy
//   bitmap, and the chamfer distance of a pair is two gathers of |r| + |s| values.
//     occ_bits_kernel / occ_count_kernel  clouds (ragged, any point stride) -> one bitmap per cloud (row-padded to whole
//                                         words; the bitmap IS the deduplication) + its number of cells
//     cell_list_kernel                    bitmap -> ascending cell list (= np.unique order of ravel_hash: x major)
//     dt_kernel                           D[c] = min over occupied c' of (di^2 ny^2 + dj^2 nx^2), u32, separable: nearest set
//                                         bit along j per row (bitmap in LDS), then a min over rows per 64-column strip
//     transpose_kernel                    D [bitmap][cell] -> [cell][bitmap]: the layout the pair sums read coalesced
//     pair_sum_kernel                     A[i][j] = sum over cells(i) of D_j[cell], u64; lane = j, the cell list is a scalar
//     combine_kernel                      cd = (A_rs/|r| + A_sr/|s|) / (2 nx^2 ny^2) in fp64, row minimum + arg-minimum merged
//                                         into the running one (first index wins)
// Integer throughout until the last division: no float atomics, results do not depend on scheduling.
#include <climits>

#include "common.h"

namespace {

#pragma clang fp contract(off)

constexpr int STRIP = 64;
constexpr unsigned DT_INF = 0xFFFFFFFFu;
constexpr int DT_LDS_MAX = 64 * 1024;

__global__ __launch_bounds__(256) void occ_bits_kernel(const float* __restrict__ pts, int stride,
                                                      const long long* __restrict__ offs, int bpc, float x0, float x1,
                                                      float y0, float y1, float voxel, int minbx, int minby, int nx,
                                                      int ny, int wpr, unsigned* __restrict__ bits) {
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x - cloud * bpc;
    const long long b = offs[cloud], e = offs[cloud + 1];
    unsigned* mine = bits + (size_t)cloud * nx * wpr;
    for (long long p = b + blk * 256 + threadIdx.x; p < e; p += (long long)bpc * 256) {
        const float x = pts[p * stride], y = pts[p * stride + 1];
        if (!(x > x0 && x < x1 && y > y0 && y < y1)) continue;          // bev_occupancy_kernel's mask and floor
        const int ix = (int)floorf(x / voxel) - minbx, iy = (int)floorf(y / voxel) - minby;
        if (ix < 0 || ix >= nx || iy < 0 || iy >= ny) continue;
        unsigned* wd = mine + (size_t)ix * wpr + (iy >> 5);
        const unsigned m = 1u << (iy & 31);
        if (!(__hip_atomic_load(wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(wd, m);
    }
}

__global__ __launch_bounds__(256) void occ_count_kernel(const unsigned* __restrict__ bits, int W,
                                                       int* __restrict__ counts) {
    __shared__ int ws[4];
    const unsigned* mine = bits + (size_t)blockIdx.x * W;
    int c = 0;
    for (int w = threadIdx.x; w < W; w += 256) c += __popc(mine[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ __launch_bounds__(256) void cell_list_kernel(const unsigned* __restrict__ bits, int W, int wpr, int ny,
                                                       const long long* __restrict__ offs, int* __restrict__ cells) {
    __shared__ int ws[4];
    const unsigned* mine = bits + (size_t)blockIdx.x * W;
    const long long base = offs[blockIdx.x], end = offs[blockIdx.x + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int run = 0;
    for (int w0 = 0; w0 < W; w0 += 256) {
        const int w = w0 + threadIdx.x;
        unsigned v = w < W ? mine[w] : 0u;
        const int c = __popc(v);
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int pre = 0;
        for (int k = 0; k < wave; ++k) pre += ws[k];
        const int total = (ws[0] + ws[1]) + (ws[2] + ws[3]);
        long long pos = base + run + pre + inc - c;
        const int row = w / wpr, col0 = (w - row * wpr) * 32;
        while (v) {
            const int bit = __ffs(v) - 1;
            v &= v - 1;
            if (pos < end) cells[pos] = row * ny + col0 + bit;
            ++pos;
        }
        run += total;
        __syncthreads();
    }
}

// one block per (64-column strip, bitmap); LDS: the bitmap (W words), then h[nx][64] = (distance along j)^2 nx^2
__global__ __launch_bounds__(256) void dt_kernel(const unsigned* __restrict__ bits, int nx, int ny, int wpr,
                                                unsigned* __restrict__ D) {
    extern __shared__ unsigned dt_lds[];
    const int W = nx * wpr;
    unsigned* sb = dt_lds;
    unsigned* h = dt_lds + W;
    const int j0 = blockIdx.x * STRIP;
    const unsigned* mine = bits + (size_t)blockIdx.y * W;
    for (int w = threadIdx.x; w < W; w += 256) sb[w] = mine[w];
    __syncthreads();
    const unsigned nx2 = (unsigned)nx * nx, ny2 = (unsigned)ny * ny;
    for (int e = threadIdx.x; e < nx * STRIP; e += 256) {
        const int ip = e >> 6, j = j0 + (e & 63);
        unsigned hv = DT_INF;
        if (j < ny) {
            const unsigned* row = sb + ip * wpr;
            const int w = j >> 5, b = j & 31;
            int g = INT_MAX;
            unsigned m = row[w] & (0xFFFFFFFFu >> (31 - b));           // bits 0 .. b: the nearest at or below j
            int ww = w;
            while (m == 0u && --ww >= 0) m = row[ww];
            if (m) g = j - (ww * 32 + 31 - __clz(m));
            m = b == 31 ? 0u : row[w] & (0xFFFFFFFFu << (b + 1));      // above j
            ww = w;
            while (m == 0u && ++ww < wpr) m = row[ww];
            if (m) g = min(g, ww * 32 + (__ffs(m) - 1) - j);
            if (g != INT_MAX) hv = (unsigned)g * (unsigned)g * nx2;
        }
        h[e] = hv;
    }
    __syncthreads();
    unsigned* out = D + (size_t)blockIdx.y * nx * ny;
    for (int e = threadIdx.x; e < nx * STRIP; e += 256) {
        const int i = e >> 6, jj = e & 63, j = j0 + jj;
        if (j >= ny) continue;
        // a = (i - k)^2 ny^2 stepped over k with second differences (mod 2^32; every true value is < 2^31)
        unsigned a = (unsigned)i * (unsigned)i * ny2, d = (2u * (unsigned)i - 1u) * ny2;
        unsigned best = DT_INF;
#pragma unroll 4
        for (int k = 0; k < nx; ++k) {
            const unsigned hv = h[k * STRIP + jj];
            const unsigned v = hv == DT_INF ? DT_INF : a + hv;         // a + hv < 2 nx^2 ny^2 < 2^32
            best = min(best, v);
            a -= d;
            d -= 2u * ny2;
        }
        out[(size_t)i * ny + j] = best;
    }
}

__global__ __launch_bounds__(256) void transpose_kernel(const unsigned* __restrict__ in, int nb, int cells,
                                                       unsigned* __restrict__ out, int ld) {
    __shared__ unsigned t[64][65];
    const int c0 = blockIdx.x * 64, b0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int b = b0 + r, c = c0 + tx;
        t[r][tx] = (b < nb && c < cells) ? in[(size_t)b * cells + c] : 0u;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, b = b0 + tx;
        if (c < cells && b < ld) out[(size_t)c * ld + b] = t[tx][r];
    }
}

__global__ __launch_bounds__(256) void pair_sum_kernel(const int* __restrict__ cells, const long long* __restrict__ offs,
                                                      const unsigned* __restrict__ Dt, int ld, int nJ,
                                                      unsigned long long* __restrict__ A) {
    __shared__ unsigned long long red[4][64];
    const int i = blockIdx.y, lane = threadIdx.x & 63, j = blockIdx.x * 64 + lane;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long b = offs[i], e = offs[i + 1];
    unsigned long long acc = 0ull;
    if (j < nJ) {
#pragma unroll 4
        for (long long k = b + wave; k < e; k += 4) acc += Dt[(size_t)cells[k] * ld + j];
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && j < nJ)
        A[(size_t)i * nJ + j] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(64) void combine_kernel(const unsigned long long* __restrict__ Ars,
                                                    const unsigned long long* __restrict__ Asr,
                                                    const int* __restrict__ cnt_r, const int* __restrict__ cnt_s, int nI,
                                                    int nJ, long long j0, int first, double norm,
                                                    double* __restrict__ minv, long long* __restrict__ argmin,
                                                    double* __restrict__ matrix, long long ldm) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const double nr = (double)cnt_r[i];
    double best = __builtin_huge_val();
    long long bj = LLONG_MAX;
    for (int j = lane; j < nJ; j += 64) {
        const double v = ((double)Ars[(size_t)i * nJ + j] / nr + (double)Asr[(size_t)j * nI + i] / (double)cnt_s[j]) / norm;
        if (matrix) matrix[(size_t)i * ldm + j0 + j] = v;
        if (v < best) { best = v; bj = j0 + j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o, 64);
        const long long oj = __shfl_xor(bj, o, 64);
        if (ov < best || (ov == best && oj < bj)) { best = ov; bj = oj; }
    }
    if (lane == 0 && (first || best < minv[i])) { minv[i] = best; argmin[i] = bj; }
}

// 0 when the grid is one the distance transform takes, else the error code
int grid_status(int nx, int ny) {
    if (nx <= 0 || ny <= 0) return LC_EINVAL;
    const unsigned long long cells = (unsigned long long)nx * (unsigned long long)ny;
    if (cells >= 46341ull) return LC_EUNSUP;                            // 2 nx^2 ny^2 >= 2^32
    const long long lds = (long long)nx * ((ny + 31) / 32) * 4 + (long long)nx * STRIP * 4;
    return lds > DT_LDS_MAX ? LC_EUNSUP : LC_OK;
}

}  // namespace

extern "C" int lc_bev_grid_supported(int nx, int ny) { return grid_status(nx, ny); }

extern "C" int lc_bev_occupancy_bits(const float* pts, int pt_stride, const int64_t* offsets, int n_clouds, int64_t max_points,
                                     float x0, float x1, float y0, float y1, float voxel, int min_bound_x, int min_bound_y,
                                     int nx, int ny, uint32_t* bits, int32_t* counts, lc_stream_t s) {
    if (!offsets || !bits || !counts || n_clouds <= 0 || max_points < 0 || (max_points > 0 && !pts) || pt_stride < 2 ||
        nx <= 0 || ny <= 0 || !(voxel > 0.f))
        return LC_EINVAL;
    const long long W = (long long)nx * ((ny + 31) / 32);
    if (W > INT_MAX || W * n_clouds > (1ll << 40)) return LC_EUNSUP;
    long long bpc = (max_points + 255) / 256;
    bpc = bpc < 1 ? 1 : (bpc > 64 ? 64 : bpc);
    if (bpc * n_clouds > INT_MAX) return LC_EUNSUP;
    if (hipMemsetAsync(bits, 0, (size_t)W * n_clouds * 4, lc_s(s)) != hipSuccess) return lc_launch_status();
    if (max_points > 0)
        hipLaunchKernelGGL(occ_bits_kernel, dim3((unsigned)(bpc * n_clouds)), dim3(256), 0, lc_s(s), pts, pt_stride,
                           (const long long*)offsets, (int)bpc, x0, x1, y0, y1, voxel, min_bound_x, min_bound_y, nx, ny,
                           (ny + 31) / 32, bits);
    hipLaunchKernelGGL(occ_count_kernel, dim3(n_clouds), dim3(256), 0, lc_s(s), bits, (int)W, counts);
    return lc_launch_status();
}

extern "C" int lc_bev_cell_lists(const uint32_t* bits, int n_clouds, int nx, int ny, const int64_t* cell_offsets,
                                 int32_t* cells, lc_stream_t s) {
    if (!bits || !cell_offsets || !cells || n_clouds <= 0 || nx <= 0 || ny <= 0) return LC_EINVAL;
    const long long W = (long long)nx * ((ny + 31) / 32);
    if (W > INT_MAX || (long long)nx * ny > INT_MAX) return LC_EUNSUP;
    hipLaunchKernelGGL(cell_list_kernel, dim3(n_clouds), dim3(256), 0, lc_s(s), bits, (int)W, (ny + 31) / 32, ny,
                       (const long long*)cell_offsets, cells);
    return lc_launch_status();
}

extern "C" int lc_bev_distance_transform(const uint32_t* bits, int n_maps, int nx, int ny, uint32_t* tmp, uint32_t* Dt,
                                         int ld, lc_stream_t s) {
    if (!bits || !tmp || !Dt || n_maps <= 0 || nx <= 0 || ny <= 0 || ld < n_maps) return LC_EINVAL;
    const int st = grid_status(nx, ny);
    if (st != LC_OK) return st;
    if (n_maps > 65535) return LC_EUNSUP;
    const int wpr = (ny + 31) / 32, cells = nx * ny;
    const size_t lds = (size_t)nx * wpr * 4 + (size_t)nx * STRIP * 4;
    hipLaunchKernelGGL(dt_kernel, dim3((ny + STRIP - 1) / STRIP, n_maps), dim3(256), lds, lc_s(s), bits, nx, ny, wpr, tmp);
    hipLaunchKernelGGL(transpose_kernel, dim3((cells + 63) / 64, (ld + 63) / 64), dim3(256), 0, lc_s(s), tmp, n_maps,
                       cells, Dt, ld);
    return lc_launch_status();
}

extern "C" int lc_bev_pair_sums(const int32_t* cells, const int64_t* cell_offsets, int nI, const uint32_t* Dt, int ld,
                                int nJ, uint64_t* A, lc_stream_t s) {
    if (!cells || !cell_offsets || !Dt || !A || nI <= 0 || nJ <= 0 || ld < nJ) return LC_EINVAL;
    if (nI > 65535) return LC_EUNSUP;
    hipLaunchKernelGGL(pair_sum_kernel, dim3((nJ + 63) / 64, nI), dim3(256), 0, lc_s(s), cells,
                       (const long long*)cell_offsets, Dt, ld, nJ, (unsigned long long*)A);
    return lc_launch_status();
}

extern "C" int lc_bev_chamfer_combine(const uint64_t* A_rs, const uint64_t* A_sr, const int32_t* count_r,
                                      const int32_t* count_s, int nI, int nJ, int64_t j0, int first, int nx, int ny,
                                      double* min_out, int64_t* argmin_out, double* matrix, int64_t matrix_ld,
                                      lc_stream_t s) {
    if (!A_rs || !A_sr || !count_r || !count_s || !min_out || !argmin_out || nI <= 0 || nJ <= 0 || j0 < 0 ||
        (matrix && matrix_ld < j0 + nJ))
        return LC_EINVAL;
    const int st = grid_status(nx, ny);
    if (st != LC_OK) return st;
    const double norm = 2.0 * ((double)nx * nx) * ((double)ny * ny);
    hipLaunchKernelGGL(combine_kernel, dim3(nI), dim3(64), 0, lc_s(s), (const unsigned long long*)A_rs,
                       (const unsigned long long*)A_sr, count_r, count_s, nI, nJ, (long long)j0, first, norm, min_out,
                       (long long*)argmin_out, matrix, (long long)matrix_ld);
    return lc_launch_status();
}
