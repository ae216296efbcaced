// Fused PointNet trunk: the per-point MLP 3 -> 64 -> 128 -> 1024 of the reference's STN3d and
// PointNetfeat (lidargen/metrics/extractor/pointnet.py) followed by the max over the points, BatchNorm folded into the
// weights by the caller.  Nothing wider than the 3 input channels is read from memory and only per-tile channel maxima
// are written.
//   pn_trunk_kernel   (its three stages are in csrc/pointnet_trunk.h)  one block = PN_T points of one cloud, 4 waves, 64 KiB of LDS: two blocks per CU, so one block's
//                     layer 1, weight loads and reductions run under the other block's MFMAs.
//       layer 1 (K = 3, the optional 3x3 transform in front of it) on the vector ALUs -> h1 [64][PN_T] in LDS
//       layer 2 on v_mfma_f32_32x32x2_f32: wave w owns output channels 32 w .. 32 w + 31, its 32 x 64 slice of W2 sits
//               in 32 registers (the MFMA's A operand), the points are the MFMA's columns -> relu -> h2 [128][PN_T],
//               which takes h1's place in LDS (the results wait in registers across a barrier)
//       layer 3 on the same instruction in 32 chunks of 32 output channels, 8 per wave: the chunk's 32 x 128 slice of W3
//               in 64 registers, four 32 x 32 accumulators (column j of accumulator s is point 4 j + s: one 128-bit LDS
//               read feeds four MFMAs), reduced to a per-channel maximum in registers, then across the 32 lanes of a
//               half wave -> part[b][tile][1024].  Lanes past N are masked with -inf (the tail is not padded with points).
//   pn_reduce_kernel  y[b][c] = [relu](max over the tiles of part[b][.][c] + b3[c]).  Bias and ReLU commute with the max
//                     exactly (both are monotone), a BatchNorm scale does not: it is in W3.
// The f32-input MFMA is a k-ordered fp32 fma chain: exact fp32, no operand splitting, no range bookkeeping.  The k order
// is fixed (lane half h sums k = h K/2 .. (h + 1) K/2 - 1 interleaved with the other half by the instruction), a cloud's
// blocks depend on nothing but the cloud, and the maxima are merged in a fixed order without atomics: the same bits for
// a cloud in every batch and every run.  A point (0,0,0) is a point like any other.
#include "common.h"
#include "pointnet_trunk.h"   // the three stages of a tile: one definition shared with csrc/glenet.hip

namespace {

constexpr int PN_T = PNT_T;                   // points per block
constexpr int PN_C1 = PNT_C1, PN_C2 = PNT_C2, PN_C3 = 1024;

__global__ __launch_bounds__(256, 2) void pn_trunk_kernel(const float* __restrict__ x, long long x_bs,
                                                      const float* __restrict__ trans, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, const float* __restrict__ w3, int N,
                                                      int tiles, float* __restrict__ part) {
    // h1 [64][PN_T], then h2 [128][PN_T] in its place (layer 2 holds its results in registers across a barrier): 64 KiB,
    // two blocks per CU, so one block's layer 1, loads and reductions run under the other's MFMAs
    __shared__ __attribute__((aligned(16))) float h2[PN_C2 * PN_T];
    float* const h1 = h2;
    const int b = blockIdx.y, tile = blockIdx.x, t0 = tile * PN_T;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;

    {   // layer 1: thread = (point, half of the 64 channels)
        const int p = tid & (PN_T - 1), c0 = __builtin_amdgcn_readfirstlane(tid >> 7) * 32;
        const int n = t0 + p;
        const float* xb = x + (size_t)b * x_bs;
        float q0 = 0.f, q1 = 0.f, q2 = 0.f;
        if (n < N) {
            q0 = xb[n];
            q1 = xb[(size_t)N + n];
            q2 = xb[2 * (size_t)N + n];
        }
        if (trans) {                          // p' = p^T . trans[b]
            const float* t = trans + (size_t)b * 9;
            const float r0 = fmaf(q2, t[6], fmaf(q1, t[3], q0 * t[0]));
            const float r1 = fmaf(q2, t[7], fmaf(q1, t[4], q0 * t[1]));
            const float r2 = fmaf(q2, t[8], fmaf(q1, t[5], q0 * t[2]));
            q0 = r0, q1 = r1, q2 = r2;
        }
        pnt_layer1(h1, p, c0, q0, q1, q2, w1, b1);
    }
    __syncthreads();
    pnt_layer2(h2, w2, b2, wave, j, h);
    __syncthreads();

    // layer 3 in 32 chunks of 32 output channels, 8 per wave
    float* out = part + ((size_t)b * tiles + tile) * PN_C3;
    const int nvalid = N - t0;                // >= 1; < PN_T only in the cloud's last tile
    for (int it = 0; it < PN_C3 / 32 / 4; ++it) {
        const int chunk = wave + 4 * it;
        float m[16];
        pnt_layer3_chunk(h2, w3, chunk, j, h, nvalid, m);
        if (j == 0) {
#pragma unroll
            for (int v = 0; v < 16; ++v) out[chunk * 32 + mfma_row(v, h)] = m[v];
        }
    }
}

// one block = 64 channels of one cloud; wave g merges tiles g, g + 4, ...
__global__ __launch_bounds__(256) void pn_reduce_kernel(const float* __restrict__ part, int tiles,
                                                       const float* __restrict__ b3, int relu3, float* __restrict__ y,
                                                       long long y_bs) {
    __shared__ float red[4][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const float* mine = part + (size_t)b * tiles * PN_C3 + c;
    float m = -__builtin_huge_valf();
    for (int t = g; t < tiles; t += 4) m = fmaxf(m, mine[(size_t)t * PN_C3]);
    red[g][lane] = m;
    __syncthreads();
    if (g == 0) {
        float v = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane])) + b3[c];
        if (relu3) v = fmaxf(v, 0.f);
        y[(size_t)b * y_bs + c] = v;
    }
}

}  // namespace

extern "C" int64_t lc_pointnet_trunk_scratch_elems(int B, int N) {
    if (B < 1 || N < 1) return 0;
    return (int64_t)B * ((N + PN_T - 1) / PN_T) * PN_C3;
}

extern "C" int lc_pointnet_trunk_fwd(const float* x, int64_t x_bs, const float* trans, const float* w1, const float* b1,
                                     const float* w2, const float* b2, const float* w3, const float* b3, int relu3,
                                     float* y, int64_t y_bs, int B, int N, float* scratch, lc_stream_t s) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !y || !scratch || B < 1 || N < 1) return LC_EINVAL;
    if (B > 65535 || N >= (1 << 24)) return LC_EUNSUP;
    if (x_bs < 3ll * N || y_bs < PN_C3) return LC_EUNSUP;
    if (!lc_aligned16(w2) || !lc_aligned16(w3)) return LC_EUNSUP;      // their rows are read as 128-bit quads
    const int tiles = (N + PN_T - 1) / PN_T;
    hipLaunchKernelGGL(pn_trunk_kernel, dim3(tiles, B), dim3(256), 0, lc_s(s), x, (long long)x_bs, trans, w1, b1, w2, b2,
                       w3, N, tiles, scratch);
    hipLaunchKernelGGL(pn_reduce_kernel, dim3(PN_C3 / 64, B), dim3(256), 0, lc_s(s), scratch, tiles, b3, relu3 ? 1 : 0, y,
                       (long long)y_bs);
    return lc_launch_status();
}
