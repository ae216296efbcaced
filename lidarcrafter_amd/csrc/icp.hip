// Point-to-point ICP on a ragged batch of float64 clouds: the registration behind the temporal metric TTCE
// (lidargen/metrics/temporal.py estimate_transform_icp, i.e. Open3D registration_icp with
// TransformationEstimationPointToPoint and default criteria, restated -- DESIGN.md section 5p).
//
//   grid build   per cloud: bounding box -> cell edge h (doubled until the grid fits ICP_CELL_BUDGET cells) -> integer
//                histogram -> exclusive scan -> scatter of (x, y, z, original index) into cell order.  The order of the
//                points INSIDE a cell is a race of the scatter's atomics; nothing below depends on it.
//   pass         one thread per source point: p' = T p, then the cells around p' in shells of growing Chebyshev distance,
//                a row of cells (consecutive in x) at a time; a row is skipped when its box is farther than the best
//                distance so far or the radius, the walk ends when the next shell is.  The minimum of (dx dx + dy dy) + dz dz
//                (no contraction) with d2 <= radius^2 wins, among equal minima the smallest original index.  The block then
//                adds its count, sum p', sum q, sum p' q^T and sum d2 in a fixed tree: one slot per (pair, block).
//   update       one block per pair: the slots in block order, the centred covariance, the rotation by Horn's quaternion
//                form (largest eigenvector of a symmetric 4x4, cyclic Jacobi), T <- update T, fitness, rmse, stopping rule.
// lc_icp_run enqueues init + pass + max_iteration x (update, pass) + update with no read-back; the kernels of a finished
// pair return at once.  No float atomics; a pair's bits depend neither on the run nor on the batch it is in.
#include "common.h"

namespace {

#pragma clang fp contract(off)

constexpr int ICP_BLK = 256;               // source points per pass block
constexpr int ICP_NW = ICP_BLK / LC_WAVE;
constexpr int ICP_TERMS = 17;              // count, sum p (3), sum q (3), sum p q^T (9), sum d2
constexpr int ICP_CELL_BUDGET = 1 << 20;   // cells per cloud
constexpr int ICP_BUILD_BLK = 1024;         // threads of a cloud's scan block
constexpr int ICP_HDR_BLK = 256;            // threads of a cloud's bounding-box block
constexpr int ICP_MAX_Y = 65535;           // gridDim.y

struct GridHdr {
    double org[3], top[3];   // bounding box
    double h, slack;         // cell edge; what a cell's box may be off by (rounding of (x - org) / h)
    int dim[3], ncells;      // ncells == 0: an empty or refused cloud
    int n, first;            // points of the cloud, its first row in `points`
    int pad[2];
};
static_assert(sizeof(GridHdr) == 96, "GridHdr layout");

struct GridView {
    GridHdr* hdr;     // [C]
    int* count;       // [C][ICP_CELL_BUDGET]      histogram, then the scatter's countdown
    int* start;       // [C][ICP_CELL_BUDGET + 1]  first sorted row of a cell, cloud-relative
    double* sxyz;     // [total][3]  points in cell order
    int* sidx;        // [total]     their index inside the cloud
};

inline long long grid_bytes(int C, long long total) {
    long long b = (long long)C * sizeof(GridHdr);
    b += (long long)C * ICP_CELL_BUDGET * 4;
    b += (long long)C * (ICP_CELL_BUDGET + 1) * 4;
    b = (b + 15) / 16 * 16;
    b += total * 24;
    b += total * 4;
    return (b + 15) / 16 * 16;
}

__host__ __device__ inline GridView grid_view(void* base, int C, long long total) {
    GridView g;
    char* p = static_cast<char*>(base);
    g.hdr = reinterpret_cast<GridHdr*>(p);
    p += (long long)C * sizeof(GridHdr);
    g.count = reinterpret_cast<int*>(p);
    p += (long long)C * ICP_CELL_BUDGET * 4;
    g.start = reinterpret_cast<int*>(p);
    p += (long long)C * (ICP_CELL_BUDGET + 1) * 4;
    long long off = p - static_cast<char*>(base);
    p += (off + 15) / 16 * 16 - off;
    g.sxyz = reinterpret_cast<double*>(p);
    p += total * 24;
    g.sidx = reinterpret_cast<int*>(p);
    return g;
}

// rows [first, first + n) of `points` that cloud c owns; n = 0 when the offsets do not describe rows of the operand
__device__ __forceinline__ void cloud_rows(const int* __restrict__ offsets, int c, int C, long long total, int& first, int& n) {
    first = 0;
    n = 0;
    if (c < 0 || c >= C) return;
    const int a = offsets[c], b = offsets[c + 1];
    if (a < 0 || b < a || b > total) return;
    first = a;
    n = b - a;
}

__device__ __forceinline__ int cell_of(double x, double org, double h, int dim) {
    double f = floor((x - org) / h);
    f = f >= 0.0 ? f : 0.0;   // (NaN too)
    f = f > (double)(dim - 1) ? (double)(dim - 1) : f;
    return (int)f;
}

// Block-wide minimum / maximum in a fixed tree (min and max do not depend on the order anyway).
__device__ __forceinline__ double block_min(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = sh[0];
    for (int i = 1; i < ICP_HDR_BLK / LC_WAVE; ++i) m = fmin(m, sh[i]);
    return m;
}

// One block per cloud: bounding box, cell edge, dimensions; clears the cloud's histogram.
__global__ __launch_bounds__(ICP_HDR_BLK) void icp_grid_header_kernel(const double* __restrict__ points,
                                                                         const int* __restrict__ offsets, int C,
                                                                         long long total, double h0, GridView g) {
    __shared__ double sh[ICP_HDR_BLK / LC_WAVE];
    __shared__ int s_ncells;
    const int c = blockIdx.x;
    int first, n;
    cloud_rows(offsets, c, C, total, first, n);
    double lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = __builtin_huge_val();
        hi[a] = -__builtin_huge_val();
    }
#pragma unroll 2
    for (int i = threadIdx.x; i < n; i += ICP_HDR_BLK) {
        const double* p = points + (long long)(first + i) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], p[a]);
            hi[a] = fmax(hi[a], p[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = block_min(lo[a], sh);
        hi[a] = -block_min(-hi[a], sh);
    }
    if (threadIdx.x == 0) {
        GridHdr& H = g.hdr[c];   // written field by field: a local copy of the struct lands on the stack
        H.n = n;
        H.first = first;
        H.pad[0] = H.pad[1] = 0;
        double h = h0, scale = h0;
        bool finite = n > 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            H.org[a] = lo[a];
            H.top[a] = hi[a];
            finite = finite && (hi[a] - lo[a]) < 1e300 && lo[a] == lo[a] && hi[a] == hi[a];
            scale = fmax(scale, fmax(fabs(lo[a]), fabs(hi[a])));
        }
        int d[3] = {0, 0, 0};
        long long cells = 0;
        if (finite) {
            // doubling h never costs exactness: any extent fits after at most ~1000 doublings of a finite h0
#pragma unroll 1
            for (int it = 0; it < 2200; ++it) {
                double prod = 1.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) prod *= floor((hi[a] - lo[a]) / h) + 1.0;
                if (prod <= (double)ICP_CELL_BUDGET) break;
                h *= 2.0;
            }
            cells = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                d[a] = (int)(floor((hi[a] - lo[a]) / h) + 1.0);
                cells *= d[a];
            }
            if (cells > ICP_CELL_BUDGET || cells < 1) cells = 0;   // (h overflowed: cannot happen for finite input)
        }
        H.h = h;
        H.slack = 1e-12 * (scale + h);
        H.dim[0] = d[0];
        H.dim[1] = d[1];
        H.dim[2] = d[2];
        H.ncells = (int)cells;
        s_ncells = (int)cells;
    }
    __syncthreads();
    const int ncells = s_ncells;
    int* cnt = g.count + (long long)c * ICP_CELL_BUDGET;
    for (int i = threadIdx.x; i < ncells; i += ICP_HDR_BLK) cnt[i] = 0;
}

__device__ __forceinline__ int point_cell(const GridHdr& H, const double* p) {
    const int cx = cell_of(p[0], H.org[0], H.h, H.dim[0]);
    const int cy = cell_of(p[1], H.org[1], H.h, H.dim[1]);
    const int cz = cell_of(p[2], H.org[2], H.h, H.dim[2]);
    return (cz * H.dim[1] + cy) * H.dim[0] + cx;
}

__global__ __launch_bounds__(ICP_BLK) void icp_grid_count_kernel(const double* __restrict__ points, GridView g) {
    const int c = blockIdx.y;
    const GridHdr H = g.hdr[c];
    const int i = blockIdx.x * ICP_BLK + threadIdx.x;
    if (H.ncells == 0 || i >= H.n) return;
    const int cell = point_cell(H, points + (long long)(H.first + i) * 3);
    atomicAdd(g.count + (long long)c * ICP_CELL_BUDGET + cell, 1);
}

// One block per cloud: start[] = exclusive scan of count[], start[ncells] = n.  Thread t owns a contiguous chunk.
__global__ __launch_bounds__(ICP_BUILD_BLK) void icp_grid_scan_kernel(GridView g) {
    __shared__ int sums[ICP_BUILD_BLK];
    const int c = blockIdx.x;
    const int ncells = g.hdr[c].ncells;
    const int* cnt = g.count + (long long)c * ICP_CELL_BUDGET;
    int* st = g.start + (long long)c * (ICP_CELL_BUDGET + 1);
    const int chunk = (ncells + ICP_BUILD_BLK - 1) / ICP_BUILD_BLK;
    const int a = min(ncells, (int)threadIdx.x * chunk), b = min(ncells, a + chunk);
    int s = 0;
    for (int i = a; i < b; ++i) s += cnt[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < ICP_BUILD_BLK; o <<= 1) {   // inclusive Hillis-Steele scan of the chunk sums
        const int v = threadIdx.x >= o ? sums[threadIdx.x - o] : 0;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    int run = sums[threadIdx.x] - s;
    for (int i = a; i < b; ++i) {
        st[i] = run;
        run += cnt[i];
    }
    if (threadIdx.x == ICP_BUILD_BLK - 1) st[ncells] = sums[ICP_BUILD_BLK - 1];
}

__global__ __launch_bounds__(ICP_BLK) void icp_grid_scatter_kernel(const double* __restrict__ points, GridView g) {
    const int c = blockIdx.y;
    const GridHdr H = g.hdr[c];
    const int i = blockIdx.x * ICP_BLK + threadIdx.x;
    if (H.ncells == 0 || i >= H.n) return;
    const double* p = points + (long long)(H.first + i) * 3;
    const int cell = point_cell(H, p);
    const int left = atomicSub(g.count + (long long)c * ICP_CELL_BUDGET + cell, 1);   // n_cell ... 1
    const int row = g.start[(long long)c * (ICP_CELL_BUDGET + 1) + cell] + left - 1;
    if (row < 0 || row >= H.n) return;   // (cannot happen: histogram and scatter see the same cells)
    double* o = g.sxyz + (long long)(H.first + row) * 3;
    o[0] = p[0];
    o[1] = p[1];
    o[2] = p[2];
    g.sidx[H.first + row] = i;
}

// distance from x to [lo, hi], made smaller by the slack of the cell boxes, never negative
__device__ __forceinline__ double axis_gap(double x, double lo, double hi, double slack) {
    const double gap = fmax(lo - x, x - hi) - slack;
    return gap > 0.0 ? gap : 0.0;
}

struct Best {
    double d2;
    int idx;
    double q[3];
};

// cells [xa, xb] of row (y, z): consecutive in the sorted order
__device__ __forceinline__ void scan_row(const GridHdr& H, const int* __restrict__ st, const double* __restrict__ sxyz,
                                         const int* __restrict__ sidx, const double* p, double r2, double gyz2, int xa,
                                         int xb, int y, int z, Best& best) {
    const double gx = axis_gap(p[0], H.org[0] + xa * H.h, H.org[0] + (xb + 1) * H.h, H.slack);
    const double lb2 = gx * gx + gyz2;
    if (lb2 > fmin(best.d2, r2)) return;
    const int row = (z * H.dim[1] + y) * H.dim[0];
    const int s = st[row + xa], e = st[row + xb + 1];
    for (int k = s; k < e; ++k) {
        const double* q = sxyz + (long long)(H.first + k) * 3;
        const double qx = q[0], qy = q[1], qz = q[2];
        const double dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= r2 && d2 <= best.d2) {
            const int oi = sidx[H.first + k];
            if (d2 < best.d2 || oi < best.idx) {   // equal distances: the smallest original index, whatever the cell order
                best.d2 = d2;
                best.idx = oi;
                best.q[0] = qx;
                best.q[1] = qy;
                best.q[2] = qz;
            }
        }
    }
}

// nearest target point within the radius of p (best.idx = -1: none)
__device__ __forceinline__ void nn_search(const GridHdr& H, const int* __restrict__ st, const double* __restrict__ sxyz,
                                          const int* __restrict__ sidx, const double* p, double radius, double r2,
                                          Best& best) {
    best.d2 = __builtin_huge_val();
    best.idx = -1;
    best.q[0] = best.q[1] = best.q[2] = 0.0;
    if (H.ncells == 0) return;
    int c0[3], lo[3], hi[3];
    const double reach = radius + H.slack;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(p[a] + reach >= H.org[a] && p[a] - reach <= H.top[a])) return;   // the ball misses the box (or p is NaN)
        c0[a] = cell_of(p[a], H.org[a], H.h, H.dim[a]);
        lo[a] = cell_of(p[a] - reach, H.org[a], H.h, H.dim[a]);
        hi[a] = cell_of(p[a] + reach, H.org[a], H.h, H.dim[a]);
    }
    int kmax = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) kmax = max(kmax, max(c0[a] - lo[a], hi[a] - c0[a]));
    for (int k = 0; k <= kmax; ++k) {
        for (int dz = -k; dz <= k; ++dz) {
            const int z = c0[2] + dz;
            if (z < lo[2] || z > hi[2]) continue;
            const double gz = axis_gap(p[2], H.org[2] + z * H.h, H.org[2] + (z + 1) * H.h, H.slack);
            for (int dy = -k; dy <= k; ++dy) {
                const int y = c0[1] + dy;
                if (y < lo[1] || y > hi[1]) continue;
                const double gy = axis_gap(p[1], H.org[1] + y * H.h, H.org[1] + (y + 1) * H.h, H.slack);
                const double gyz2 = gy * gy + gz * gz;
                if (gyz2 > fmin(best.d2, r2)) continue;
                const bool face = dz == -k || dz == k || dy == -k || dy == k;
                if (face) {
                    const int xa = max(lo[0], c0[0] - k), xb = min(hi[0], c0[0] + k);
                    if (xa <= xb) scan_row(H, st, sxyz, sidx, p, r2, gyz2, xa, xb, y, z, best);
                } else {   // k > 0 here: the two end cells of the row
                    const int x0 = c0[0] - k, x1 = c0[0] + k;
                    if (x0 >= lo[0]) scan_row(H, st, sxyz, sidx, p, r2, gyz2, x0, x0, y, z, best);
                    if (x1 <= hi[0]) scan_row(H, st, sxyz, sidx, p, r2, gyz2, x1, x1, y, z, best);
                }
            }
        }
        // every cell of a later shell is at least k h away (p lies in, or beyond, its own cell)
        const double next = k * H.h - H.slack;
        if (next > 0.0 && best.d2 < next * next) break;
    }
}

struct PairState {
    double prev_fitness, prev_rmse;
    int done, iters;
};

// grid (blocks over the largest source, P).  idx / d2: [P][ld] or NULL; part: [P][nblk_ld][ICP_TERMS] or NULL;
// state: NULL = every pair is live.
__global__ __launch_bounds__(ICP_BLK) void icp_pass_kernel(const double* __restrict__ points, const int* __restrict__ offsets,
                                                           int C, long long total, GridView g, const int* __restrict__ pairs,
                                                           const double* __restrict__ Tm, double radius, int ld,
                                                           int* __restrict__ idx, double* __restrict__ d2out,
                                                           double* __restrict__ part, int nblk_ld,
                                                           const PairState* __restrict__ state) {
    __shared__ double wsum[ICP_NW][ICP_TERMS];
    const int pr = blockIdx.y;
    if (state != nullptr && state[pr].done) return;
    const int src = pairs[2 * pr], tgt = pairs[2 * pr + 1];
    int first, n;
    cloud_rows(offsets, src, C, total, first, n);
    n = min(n, ld);
    if ((long long)blockIdx.x * ICP_BLK >= n) return;
    const int i = blockIdx.x * ICP_BLK + threadIdx.x;
    double v[ICP_TERMS];
#pragma unroll
    for (int t = 0; t < ICP_TERMS; ++t) v[t] = 0.0;
    if (i < n) {
        const double* T = Tm + (long long)pr * 16;
        const double* s = points + (long long)(first + i) * 3;
        const double x = s[0], y = s[1], z = s[2];
        double p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
        Best best;
        best.d2 = __builtin_huge_val();
        best.idx = -1;
        best.q[0] = best.q[1] = best.q[2] = 0.0;
        if (tgt >= 0 && tgt < C) {
            const GridHdr H = g.hdr[tgt];
            nn_search(H, g.start + (long long)tgt * (ICP_CELL_BUDGET + 1), g.sxyz, g.sidx, p, radius, radius * radius, best);
        }
        if (idx != nullptr) idx[(long long)pr * ld + i] = best.idx;
        if (d2out != nullptr) d2out[(long long)pr * ld + i] = best.d2;
        if (best.idx >= 0) {
            v[0] = 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[1 + a] = p[a];
                v[4 + a] = best.q[a];
#pragma unroll
                for (int b = 0; b < 3; ++b) v[7 + 3 * a + b] = p[a] * best.q[b];
            }
            v[16] = best.d2;
        }
    }
    if (part == nullptr) return;
#pragma unroll
    for (int t = 0; t < ICP_TERMS; ++t) v[t] = lc_wave_sum(v[t]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int t = 0; t < ICP_TERMS; ++t) wsum[threadIdx.x >> 6][t] = v[t];
    }
    __syncthreads();
    if (threadIdx.x < ICP_TERMS) {
        double s = wsum[0][threadIdx.x];
        for (int w = 1; w < ICP_NW; ++w) s += wsum[w][threadIdx.x];
        part[((long long)pr * nblk_ld + blockIdx.x) * ICP_TERMS + threadIdx.x] = s;
    }
}

__global__ void icp_init_kernel(const int* __restrict__ offsets, int C, long long total, const int* __restrict__ pairs, int P,
                                int ld, PairState* __restrict__ state, double* __restrict__ fitness,
                                double* __restrict__ rmse, int* __restrict__ iters) {
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    if (pr >= P) return;
    int f, n, m;
    cloud_rows(offsets, pairs[2 * pr], C, total, f, n);
    cloud_rows(offsets, pairs[2 * pr + 1], C, total, f, m);
    PairState s;
    s.prev_fitness = 0.0;
    s.prev_rmse = 0.0;
    s.done = (n < 1 || m < 1 || n > ld) ? 1 : 0;   // nothing to register: T stays, fitness 0
    s.iters = 0;
    state[pr] = s;
    fitness[pr] = 0.0;
    rmse[pr] = 0.0;
    iters[pr] = 0;
}

// Largest eigenvector of the symmetric 4x4 A (cyclic Jacobi; A is destroyed, V receives the eigenvectors in its columns).
// Among equal eigenvalues the first column wins: A == 0 gives (1, 0, 0, 0), the identity rotation.
__device__ __forceinline__ void jacobi4_largest(double (*A)[4], double (*V)[4], double* q) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 4; ++i) {
            diag += A[i][i] * A[i][i];
            for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
        }
        if (off == 0.0 || off <= 1e-40 * diag) break;
        for (int p = 0; p < 3; ++p)
            for (int r = p + 1; r < 4; ++r) {
                const double apr = A[p][r];
                if (apr == 0.0) continue;
                const double theta = (A[r][r] - A[p][p]) / (2.0 * apr);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {   // A <- A J
                    const double akp = A[k][p], akr = A[k][r];
                    A[k][p] = c * akp - s * akr;
                    A[k][r] = s * akp + c * akr;
                }
                for (int k = 0; k < 4; ++k) {   // A <- J^T A
                    const double apk = A[p][k], ark = A[r][k];
                    A[p][k] = c * apk - s * ark;
                    A[r][k] = s * apk + c * ark;
                }
                A[p][r] = 0.0;
                A[r][p] = 0.0;
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkr = V[k][r];
                    V[k][p] = c * vkp - s * vkr;
                    V[k][r] = s * vkp + c * vkr;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > A[best][best]) best = i;
    double nrm = 0.0;
    for (int k = 0; k < 4; ++k) nrm += V[k][best] * V[k][best];
    nrm = sqrt(nrm);
    for (int k = 0; k < 4; ++k) q[k] = V[k][best] / nrm;
}

// One block per pair.  `it`: updates applied so far, i.e. the pass whose slots lie in `part` is pass number `it`.
__global__ __launch_bounds__(LC_WAVE) void icp_update_kernel(const int* __restrict__ offsets, int C, long long total,
                                                             const int* __restrict__ pairs, const double* __restrict__ part,
                                                             int nblk_ld, int it, int max_it, double rel_fitness,
                                                             double rel_rmse, double* __restrict__ Tm,
                                                             PairState* __restrict__ state, double* __restrict__ fitness,
                                                             double* __restrict__ rmse, int* __restrict__ iters) {
    __shared__ double S[ICP_TERMS];
    __shared__ double A[4][4], V[4][4], q[4];
    const int pr = blockIdx.x;
    if (state[pr].done) return;
    int first, n;
    cloud_rows(offsets, pairs[2 * pr], C, total, first, n);
    const int nblk = min(nblk_ld, (n + ICP_BLK - 1) / ICP_BLK);
    if (threadIdx.x < ICP_TERMS) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += part[((long long)pr * nblk_ld + b) * ICP_TERMS + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double cnt = S[0];
    const double fit = cnt / (double)n;
    const double rms = cnt > 0.0 ? sqrt(S[16] / cnt) : 0.0;
    fitness[pr] = fit;
    rmse[pr] = rms;
    iters[pr] = it;
    PairState st = state[pr];
    const bool converged = it > 0 && fabs(fit - st.prev_fitness) < rel_fitness && fabs(rms - st.prev_rmse) < rel_rmse;
    if (converged || it >= max_it) {
        st.done = 1;
        st.iters = it;
        state[pr] = st;
        return;
    }
    st.prev_fitness = fit;
    st.prev_rmse = rms;
    st.iters = it;
    state[pr] = st;
    if (!(cnt > 0.0)) return;   // no correspondences: the update is the identity
    double mp[3], mq[3], M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mp[a] = S[1 + a] / cnt;
        mq[a] = S[4 + a] / cnt;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) M[a][b] = S[7 + 3 * a + b] / cnt - mp[a] * mq[b];   // sum (p - mp)(q - mq)^T / n
    // Horn 1987: the rotation maximising sum q . R p is the largest eigenvector of N(M)
    A[0][0] = M[0][0] + M[1][1] + M[2][2];
    A[1][1] = M[0][0] - M[1][1] - M[2][2];
    A[2][2] = -M[0][0] + M[1][1] - M[2][2];
    A[3][3] = -M[0][0] - M[1][1] + M[2][2];
    A[0][1] = A[1][0] = M[1][2] - M[2][1];
    A[0][2] = A[2][0] = M[2][0] - M[0][2];
    A[0][3] = A[3][0] = M[0][1] - M[1][0];
    A[1][2] = A[2][1] = M[0][1] + M[1][0];
    A[1][3] = A[3][1] = M[2][0] + M[0][2];
    A[2][3] = A[3][2] = M[1][2] + M[2][1];
    jacobi4_largest(A, V, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z);
    R[0][1] = 2.0 * (x * y - w * z);
    R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z);
    R[1][1] = 1.0 - 2.0 * (x * x + z * z);
    R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y);
    R[2][1] = 2.0 * (y * z + w * x);
    R[2][2] = 1.0 - 2.0 * (x * x + y * y);
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = mq[a] - ((R[a][0] * mp[0] + R[a][1] * mp[1]) + R[a][2] * mp[2]);
    double* T = Tm + (long long)pr * 16;
    double N4[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double s = (R[a][0] * T[b] + R[a][1] * T[4 + b]) + R[a][2] * T[8 + b];
            if (b == 3) s += t[a];
            N4[a][b] = s;
        }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) T[4 * a + b] = N4[a][b];
}

inline int nblk_of(int max_src) { return (max_src + ICP_BLK - 1) / ICP_BLK; }

struct IcpScratch {
    PairState* state;
    double* part;
};
inline long long scratch_bytes(int P, int max_src) {
    long long b = ((long long)P * sizeof(PairState) + 15) / 16 * 16;
    return b + (long long)P * nblk_of(max_src) * ICP_TERMS * 8;
}
inline IcpScratch scratch_view(void* base, int P) {
    IcpScratch s;
    s.state = static_cast<PairState*>(base);
    s.part = reinterpret_cast<double*>(static_cast<char*>(base) + ((long long)P * sizeof(PairState) + 15) / 16 * 16);
    return s;
}

inline bool sizes_ok(int C, long long total, int P, int max_src) {
    return C >= 1 && total >= 1 && P >= 1 && max_src >= 1 && max_src <= total;
}

}  // namespace

extern "C" {

int64_t lc_nn_grid_bytes(int C, int64_t total) {
    if (C < 1 || total < 1 || C > ICP_MAX_Y || total > 0x7fffffffLL / 3) return 0;
    return grid_bytes(C, total);
}

int lc_nn_grid_build(const double* points, const int32_t* offsets, int C, int64_t total, int max_cloud, double h0, void* grid,
                     lc_stream_t s) {
    if (!points || !offsets || !grid || C < 1 || total < 1 || max_cloud < 1 || max_cloud > total || !(h0 > 0.0) ||
        !(h0 < 1e300))
        return LC_EINVAL;
    if (C > ICP_MAX_Y || total > 0x7fffffffLL / 3 || (reinterpret_cast<uintptr_t>(grid) & 15)) return LC_EUNSUP;
    const GridView g = grid_view(grid, C, total);
    const dim3 per_point((max_cloud + ICP_BLK - 1) / ICP_BLK, C);
    hipLaunchKernelGGL(icp_grid_header_kernel, dim3(C), dim3(ICP_HDR_BLK), 0, lc_s(s), points, offsets, C, (long long)total,
                       h0, g);
    hipLaunchKernelGGL(icp_grid_count_kernel, per_point, dim3(ICP_BLK), 0, lc_s(s), points, g);
    hipLaunchKernelGGL(icp_grid_scan_kernel, dim3(C), dim3(ICP_BUILD_BLK), 0, lc_s(s), g);
    hipLaunchKernelGGL(icp_grid_scatter_kernel, per_point, dim3(ICP_BLK), 0, lc_s(s), points, g);
    return lc_launch_status();
}

int lc_nn_radius(const double* points, const int32_t* offsets, int C, int64_t total, const void* grid, const int32_t* pairs,
                 const double* T, int P, int max_src, double radius, int32_t* idx, double* d2, lc_stream_t s) {
    if (!points || !offsets || !grid || !pairs || !T || !idx || !d2 || !sizes_ok(C, total, P, max_src) || !(radius > 0.0) ||
        !(radius < 1e150))
        return LC_EINVAL;
    if (C > ICP_MAX_Y || P > ICP_MAX_Y || total > 0x7fffffffLL / 3) return LC_EUNSUP;
    const GridView g = grid_view(const_cast<void*>(grid), C, total);
    hipLaunchKernelGGL(icp_pass_kernel, dim3(nblk_of(max_src), P), dim3(ICP_BLK), 0, lc_s(s), points, offsets, C,
                       (long long)total, g, pairs, T, radius, max_src, idx, d2, (double*)nullptr, 0,
                       (const PairState*)nullptr);
    return lc_launch_status();
}

int64_t lc_icp_scratch_bytes(int P, int max_src) {
    if (P < 1 || max_src < 1 || P > ICP_MAX_Y) return 0;
    return scratch_bytes(P, max_src);
}

int lc_icp_run(const double* points, const int32_t* offsets, int C, int64_t total, const void* grid, const int32_t* pairs,
               int P, int max_src, double radius, int max_iteration, double relative_fitness, double relative_rmse, double* T,
               double* fitness, double* inlier_rmse, int32_t* iterations, void* scratch, lc_stream_t s) {
    if (!points || !offsets || !grid || !pairs || !T || !fitness || !inlier_rmse || !iterations || !scratch ||
        !sizes_ok(C, total, P, max_src) || !(radius > 0.0) || !(radius < 1e150) || max_iteration < 0 ||
        !(relative_fitness == relative_fitness) || !(relative_rmse == relative_rmse))
        return LC_EINVAL;
    if (C > ICP_MAX_Y || P > ICP_MAX_Y || total > 0x7fffffffLL / 3 || max_iteration > 100000 ||
        (reinterpret_cast<uintptr_t>(scratch) & 15))
        return LC_EUNSUP;
    const GridView g = grid_view(const_cast<void*>(grid), C, total);
    const IcpScratch sc = scratch_view(scratch, P);
    const int nblk = nblk_of(max_src);
    const long long tot = total;
    hipLaunchKernelGGL(icp_init_kernel, dim3((P + 63) / 64), dim3(64), 0, lc_s(s), offsets, C, tot, pairs, P, max_src,
                       sc.state, fitness, inlier_rmse, iterations);
    for (int it = 0; it <= max_iteration; ++it) {
        hipLaunchKernelGGL(icp_pass_kernel, dim3(nblk, P), dim3(ICP_BLK), 0, lc_s(s), points, offsets, C, tot, g, pairs,
                           (const double*)T, radius, max_src, (int*)nullptr, (double*)nullptr, sc.part, nblk,
                           (const PairState*)sc.state);
        hipLaunchKernelGGL(icp_update_kernel, dim3(P), dim3(LC_WAVE), 0, lc_s(s), offsets, C, tot, pairs,
                           (const double*)sc.part, nblk, it, max_iteration, relative_fitness, relative_rmse, T, sc.state,
                           fitness, inlier_rmse, iterations);
    }
    return lc_launch_status();
}

}  // extern "C"
