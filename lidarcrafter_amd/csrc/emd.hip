// Earth Mover's Distance by the auction algorithm, forward: lidargen/metrics/modules/emd/emd_cuda.cu (emd_cuda_forward
// with the state emd_module.py:59-70 allocates).  DESIGN.md section 5i.
//
// Per iteration every unassigned point j of cloud 1 bids for the object k of cloud 2 of the largest value
//   d(j, k) = (float)(3.0 - (double)sqrtf(|xyz2[k] - xyz1[j]|^2) - (double)price[k])
// with the increment inc = (best - second best) + eps; an object goes to its highest bidder, who evicts the previous owner
// and raises the price by inc.  The last iteration gives every still-unassigned point its own bid without eviction.
//
// Three launches per iteration, none of them sized by a value read back from the device:
//   emd_bid_kernel    (point group) x (span of object chunks) per block, object coordinates + prices of a chunk in LDS,
//                     T = 1 / 4 / 16 / 64 lanes per point chosen ON THE DEVICE from the number of unassigned points so that
//                     the pass fills the chip with 32 k bidders and with 20; one (best, second, index) triple per point and span
//   emd_merge_kernel  merges a point's triples, writes its bid and increment and publishes (increment bits, j + 1) with one
//                     64-bit atomicMax per bid: the object's exact highest bidder, highest j among equal increments
//   emd_assign_kernel the winners take their objects; losers and evicted owners are appended to the next iteration's list
//                     through a per-pair counter (one atomic per wave) -- no clear / count / scan / compact passes
// The order of that list varies from run to run; nothing read from it depends on the order (ties in a point's best value go
// to the lowest object index, ties in an object's increment to the highest point index), so a call's bits are reproducible.
#include "common.h"

namespace {

#pragma clang fp contract(off)

constexpr int EMD_BLK = 256;
constexpr int EMD_CH = 512;          // objects of one LDS chunk (x, y, z, price: 8 KiB)
constexpr float EMD_FLOOR = -1e9f;   // the reference's initial best / second best and its max_increments reset
constexpr int EMD_MAX_N = 1 << 24;
constexpr int EMD_MAX_B = 65535;     // gridDim.y

typedef unsigned long long u64;

inline int emd_auto_target(int B) {
    const int t = 2048 / B;           // blocks per pair the bid pass aims for: ~8 blocks per CU over the whole batch
    return t < 64 ? 64 : t;
}
inline long long emd_cap(int B, int n) { return (long long)EMD_BLK * emd_auto_target(B) + n; }

struct EmdPlan {
    int T, groups, nspans, cps, nch;
};

// The split of one pair's bid pass for `cnt` bidders: T lanes per point (so 256 / T points per block), `groups` point groups,
// `nspans` spans of `cps` object chunks.  cnt * nspans <= max(256 * tgt, cnt) <= emd_cap: the triples fit (one span when
// groups >= tgt; else nspans <= tgt / groups and cnt <= 256 * groups / T).  256 * groups itself may exceed emd_cap at T = 64.
__device__ __forceinline__ EmdPlan emd_plan(int cnt, int n, int tgt) {
    EmdPlan p;
    p.nch = (n + EMD_CH - 1) / EMD_CH;
    p.T = 1;
    while (p.T < 64 && (((long long)cnt * p.T + EMD_BLK - 1) / EMD_BLK) * p.nch < tgt) p.T *= 4;
    p.groups = (int)(((long long)cnt * p.T + EMD_BLK - 1) / EMD_BLK);
    int ns = tgt / p.groups;
    ns = ns < 1 ? 1 : (ns > p.nch ? p.nch : ns);
    p.cps = (p.nch + ns - 1) / ns;
    p.nspans = (p.nch + p.cps - 1) / p.cps;
    return p;
}

// (best, better, bi) <- the two largest values (as a multiset) and the lowest index of the largest of both operands
__device__ __forceinline__ void emd_merge(float& best, float& better, int& bi, float ob, float obetter, int oi) {
    if (ob > best || (ob == best && (unsigned)oi < (unsigned)bi)) {
        better = fmaxf(best, obetter);
        best = ob;
        bi = oi;
    } else {
        better = fmaxf(better, ob);
    }
}

__global__ __launch_bounds__(EMD_BLK) void emd_init_kernel(int n, int* __restrict__ assignment, int* __restrict__ inv,
                                                          float* __restrict__ price, u64* __restrict__ pack,
                                                          int* __restrict__ list, int* __restrict__ cnt2) {
    const int b = blockIdx.y, B = gridDim.y;
    const int j = blockIdx.x * EMD_BLK + threadIdx.x;
    if (j == 0) {
        cnt2[b] = n;
        cnt2[B + b] = 0;
    }
    if (j >= n) return;
    const long long e = (long long)b * n + j;
    assignment[e] = -1;
    inv[e] = -1;
    price[e] = 0.f;
    pack[e] = 0ull;
    list[e] = j;
}

__global__ __launch_bounds__(EMD_BLK) void emd_bid_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                         int n, int tgt, int it, const float* __restrict__ price,
                                                         const int* __restrict__ list, int* __restrict__ cnt2,
                                                         float* __restrict__ pbest, float* __restrict__ pbetter,
                                                         int* __restrict__ pidx, long long cap) {
    __shared__ float4 sobj[EMD_CH];
    const int b = blockIdx.y, B = gridDim.y;
    const int cnt = cnt2[(it & 1) * B + b];
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt2[((it + 1) & 1) * B + b] = 0;   // the list this iteration's assign pass fills
    if (cnt <= 0) return;
    const EmdPlan p = emd_plan(cnt, n, tgt);
    const int T = p.T, PB = EMD_BLK / T;
    const int ps = threadIdx.x / T, sl = threadIdx.x % T;
    const long long base = (long long)b * n;
    const float* __restrict__ q = xyz1 + base * 3;
    const float* __restrict__ o = xyz2 + base * 3;
    const float* __restrict__ pr = price + base;
    const int* __restrict__ lst = list + ((long long)(it & 1) * B + b) * n;
    const int items = p.groups * p.nspans;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int g = item / p.nspans, s = item % p.nspans;
        const int pos = g * PB + ps;
        const bool live = pos < cnt;
        float x1 = 0.f, y1 = 0.f, z1 = 0.f;
        if (live) {
            const int j = lst[pos];
            x1 = q[3 * j];
            y1 = q[3 * j + 1];
            z1 = q[3 * j + 2];
        }
        float best = EMD_FLOOR, better = EMD_FLOOR;
        int bi = -1;
        const int c0 = s * p.cps, c1 = (c0 + p.cps < p.nch ? c0 + p.cps : p.nch);
        for (int c = c0; c < c1; ++c) {
            const int k0 = c * EMD_CH;
            const int kc = (n - k0 < EMD_CH ? n - k0 : EMD_CH);
            __syncthreads();
            for (int e = threadIdx.x; e < kc; e += EMD_BLK)
                sobj[e] = make_float4(o[3 * (k0 + e)], o[3 * (k0 + e) + 1], o[3 * (k0 + e) + 2], pr[k0 + e]);
            __syncthreads();
            if (live) {
                for (int k = sl; k < kc; k += T) {
                    const float4 v = sobj[k];
                    const float dx = v.x - x1, dy = v.y - y1, dz = v.z - z1;
                    const float d = (float)((3.0 - (double)sqrtf((dx * dx + dy * dy) + dz * dz)) - (double)v.w);
                    if (d > best) {
                        better = best;
                        best = d;
                        bi = k0 + k;
                    } else if (d > better) {
                        better = d;
                    }
                }
            }
        }
        for (int off = T >> 1; off > 0; off >>= 1) {   // the T lanes of a point are an aligned run of one wave
            const float ob = __shfl_xor(best, off, 64), obetter = __shfl_xor(better, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            emd_merge(best, better, bi, ob, obetter, oi);
        }
        if (live && sl == 0) {
            const long long e = (long long)b * cap + (long long)s * cnt + pos;
            pbest[e] = best;
            pbetter[e] = better;
            pidx[e] = bi;
        }
    }
}

__global__ __launch_bounds__(EMD_BLK) void emd_merge_kernel(int n, int tgt, int it, float eps, const int* __restrict__ list,
                                                           const int* __restrict__ cnt2, const float* __restrict__ pbest,
                                                           const float* __restrict__ pbetter, const int* __restrict__ pidx,
                                                           long long cap, int* __restrict__ bid, float* __restrict__ bid_inc,
                                                           u64* __restrict__ pack) {
    const int b = blockIdx.y, B = gridDim.y;
    const int cnt = cnt2[(it & 1) * B + b];
    const int pos = blockIdx.x * EMD_BLK + threadIdx.x;
    if (pos >= cnt) return;
    const EmdPlan p = emd_plan(cnt, n, tgt);
    float best = EMD_FLOOR, better = EMD_FLOOR;
    int bi = -1;
    for (int s = 0; s < p.nspans; ++s) {
        const long long e = (long long)b * cap + (long long)s * cnt + pos;
        emd_merge(best, better, bi, pbest[e], pbetter[e], pidx[e]);
    }
    if ((unsigned)bi >= (unsigned)n) bi = 0;   // only when no value compared greater than the floor (NaN coordinates)
    const long long base = (long long)b * n;
    const int j = list[((long long)(it & 1) * B + b) * n + pos];
    const float inc = (best - better) + eps;   // >= eps >= 0: its bit pattern orders like the value
    bid[base + j] = bi;
    bid_inc[base + j] = inc;
    atomicMax(pack + base + bi, ((u64)__float_as_uint(inc) << 32) | (u64)(unsigned)(j + 1));
}

__global__ __launch_bounds__(EMD_BLK) void emd_assign_kernel(int n, int it, int last, int* __restrict__ list,
                                                            int* __restrict__ cnt2, const int* __restrict__ bid,
                                                            const float* __restrict__ bid_inc, u64* __restrict__ pack,
                                                            int* __restrict__ assignment, int* __restrict__ inv,
                                                            float* __restrict__ price) {
    const int b = blockIdx.y, B = gridDim.y;
    const int cnt = cnt2[(it & 1) * B + b];
    if ((int)(blockIdx.x * EMD_BLK) >= cnt) return;
    const int pos = blockIdx.x * EMD_BLK + threadIdx.x;
    const long long base = (long long)b * n;
    int app = -1;   // the point this thread leaves unassigned, if any
    if (pos < cnt) {
        const int j = list[((long long)(it & 1) * B + b) * n + pos];
        const int k = bid[base + j];
        if (last) {
            assignment[base + j] = k;
        } else if ((unsigned)(pack[base + k] & 0xffffffffull) == (unsigned)(j + 1)) {
            const int prev = inv[base + k];
            if (prev >= 0) {
                assignment[base + prev] = -1;
                app = prev;
            }
            inv[base + k] = j;
            assignment[base + j] = k;
            price[base + k] += bid_inc[base + j];
            pack[base + k] = 0ull;
        } else {
            app = j;
        }
    }
    const u64 mask = __ballot(app >= 0);
    if (mask == 0ull) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    int at = 0;
    if (lane == leader) at = atomicAdd(cnt2 + ((it + 1) & 1) * B + b, __popcll(mask));
    at = __shfl(at, leader, 64);
    if (app >= 0) list[((long long)((it + 1) & 1) * B + b) * n + at + __popcll(mask & ((1ull << lane) - 1ull))] = app;
}

__global__ __launch_bounds__(EMD_BLK) void emd_dist_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                          int n, const int* __restrict__ assignment,
                                                          float* __restrict__ dist) {
    const int j = blockIdx.x * EMD_BLK + threadIdx.x;
    if (j >= n) return;
    const long long base = (long long)blockIdx.y * n;
    int k = assignment[base + j];
    if ((unsigned)k >= (unsigned)n) k = 0;   // (every point holds an object after the last iteration)
    const float* a = xyz1 + (base + j) * 3;
    const float* c = xyz2 + (base + k) * 3;
    const float dx = a[0] - c[0], dy = a[1] - c[1], dz = a[2] - c[2];
    dist[base + j] = (dx * dx + dy * dy) + dz * dz;
}

struct EmdScratch {
    u64* pack;
    int *inv, *bid, *list, *cnt2, *pidx;
    float *price, *bid_inc, *pbest, *pbetter;
    int64_t bytes;
};

inline EmdScratch emd_carve(void* scratch, int B, int n) {
    const int64_t bn = (int64_t)B * n, pc = (int64_t)B * emd_cap(B, n);
    char* p = static_cast<char*>(scratch);
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char* r = p + off;
        off += (bytes + 15) / 16 * 16;
        return r;
    };
    EmdScratch s;
    s.pack = reinterpret_cast<u64*>(take(bn * 8));
    s.inv = reinterpret_cast<int*>(take(bn * 4));
    s.bid = reinterpret_cast<int*>(take(bn * 4));
    s.list = reinterpret_cast<int*>(take(2 * bn * 4));
    s.cnt2 = reinterpret_cast<int*>(take(2 * (int64_t)B * 4));
    s.pidx = reinterpret_cast<int*>(take(pc * 4));
    s.price = reinterpret_cast<float*>(take(bn * 4));
    s.bid_inc = reinterpret_cast<float*>(take(bn * 4));
    s.pbest = reinterpret_cast<float*>(take(pc * 4));
    s.pbetter = reinterpret_cast<float*>(take(pc * 4));
    s.bytes = off;
    return s;
}

}  // namespace

extern "C" int64_t lc_emd_scratch_bytes(int B, int n) {
    if (B < 1 || n < 1 || B > EMD_MAX_B || n > EMD_MAX_N) return 0;
    return emd_carve(nullptr, B, n).bytes;
}

extern "C" int lc_emd_fwd(const float* xyz1, const float* xyz2, int B, int n, float eps, int iters, int target_blocks,
                          float* dist, int32_t* assignment, void* scratch, lc_stream_t s) {
    if (!xyz1 || !xyz2 || !dist || !assignment || !scratch || B < 1 || n < 1 || iters < 1 || !(eps >= 0.f))
        return LC_EINVAL;
    if (B > EMD_MAX_B || n > EMD_MAX_N) return LC_EUNSUP;
    const int tgt_auto = emd_auto_target(B);
    if (target_blocks < 0 || target_blocks > tgt_auto) return LC_EINVAL;   // the scratch holds tgt_auto's triples
    const int tgt = target_blocks ? target_blocks : tgt_auto;
    const EmdScratch w = emd_carve(scratch, B, n);
    const long long cap = emd_cap(B, n);
    const int nch = (n + EMD_CH - 1) / EMD_CH;
    // the most items any split makes: 64 lanes per point (4 points per block) x every chunk, or one span of every group
    long long most = (long long)((n + 3) / 4) * nch;
    if (most < (n + EMD_BLK - 1) / EMD_BLK) most = (n + EMD_BLK - 1) / EMD_BLK;
    const int gx_bid = (int)(most < tgt ? most : tgt);
    const dim3 per_point((n + EMD_BLK - 1) / EMD_BLK, B), blk(EMD_BLK);
    hipStream_t st = lc_s(s);
    hipLaunchKernelGGL(emd_init_kernel, per_point, blk, 0, st, n, assignment, w.inv, w.price, w.pack, w.list, w.cnt2);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(emd_bid_kernel, dim3(gx_bid, B), blk, 0, st, xyz1, xyz2, n, tgt, it, w.price, w.list, w.cnt2,
                           w.pbest, w.pbetter, w.pidx, cap);
        hipLaunchKernelGGL(emd_merge_kernel, per_point, blk, 0, st, n, tgt, it, eps, w.list, w.cnt2, w.pbest, w.pbetter,
                           w.pidx, cap, w.bid, w.bid_inc, w.pack);
        hipLaunchKernelGGL(emd_assign_kernel, per_point, blk, 0, st, n, it, it == iters - 1 ? 1 : 0, w.list, w.cnt2, w.bid,
                           w.bid_inc, w.pack, assignment, w.inv, w.price);
    }
    hipLaunchKernelGGL(emd_dist_kernel, per_point, blk, 0, st, xyz1, xyz2, n, assignment, dist);
    return lc_launch_status();
}
