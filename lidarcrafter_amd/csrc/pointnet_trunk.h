// The three stages of a fused per-point trunk 3 -> 64 -> 128 -> C3 on one tile of PNT_T points, shared by pn_trunk_kernel
// (csrc/pointnet.hip, C3 = 1024, dense loads) and gl_trunk_kernel (csrc/glenet.hip, C3 = 512, gathered loads): ONE definition
// of the k order.  A block is 256 threads = 4 waves; `hbuf` is PNT_C2 * PNT_T floats of LDS, first h1 [64][PNT_T], then
// h2 [128][PNT_T] in its place (layer 2 holds its results in registers across a barrier).  What differs between the kernels
// stays with them: how a thread gets its point, how many chunks of 32 output channels layer 3 has and where their maxima go.
//   layer 1 (K = 3) on the vector ALUs: an fma chain from the bias
//   layer 2 on v_mfma_f32_32x32x2_f32: wave w owns output channels 32 w .. 32 w + 31, its 32 x 64 slice of W2 sits in 32
//           registers (the MFMA's A operand), the points are the MFMA's columns -> relu -> h2
//   layer 3 on the same instruction, one chunk of 32 output channels at a time: the chunk's 32 x 128 slice of W3 in 64
//           registers, four 32 x 32 accumulators (column j of accumulator s is point 4 j + s: one 128-bit LDS read feeds four
//           MFMAs), reduced to a per-channel maximum in registers, then across the 32 lanes of a half wave.
// The f32-input MFMA is a k-ordered fp32 fma chain: lane half h sums k = h K/2 .. (h + 1) K/2 - 1, interleaved with the other
// half by the instruction.
#pragma once
#include "common.h"
#include "f16x2.h"      // mfma_row

constexpr int PNT_T = 128;                    // points per tile
constexpr int PNT_C1 = 64, PNT_C2 = 128;

// layer 1: thread = (point p of the tile, half of the 64 channels, c0 = 0 or 32); (q0, q1, q2) its point
__device__ __forceinline__ void pnt_layer1(float* __restrict__ h1, int p, int c0, float q0, float q1, float q2,
                                           const float* __restrict__ w1, const float* __restrict__ b1) {
#pragma unroll 8
    for (int c = c0; c < c0 + 32; ++c) {
        const float v = fmaf(w1[c * 3 + 2], q2, fmaf(w1[c * 3 + 1], q1, fmaf(w1[c * 3], q0, b1[c])));
        h1[c * PNT_T + p] = fmaxf(v, 0.f);
    }
}

// layer 2: lane (j, h) holds W2[32 wave + j][32 h .. 32 h + 31]; column j of accumulator s is point 4 j + s.  Every thread
// of the block calls it after a barrier behind layer 1; h2 is complete after the caller's next barrier.
__device__ __forceinline__ void pnt_layer2(float* __restrict__ hbuf, const float* __restrict__ w2,
                                           const float* __restrict__ b2, int wave, int j, int h) {
    const f32x4* wp = reinterpret_cast<const f32x4*>(w2 + (size_t)(wave * 32 + j) * PNT_C1 + h * 32);
    f32x4 a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = wp[i];
    f32x16 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[s][v] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        if ((kk & 7) == 0) __builtin_amdgcn_sched_barrier(0);   // LDS reads run at most 8 steps ahead
        const f32x4 bv = *reinterpret_cast<const f32x4*>(&hbuf[(h * 32 + kk) * PNT_T + 4 * j]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk >> 2][kk & 3], bv[s], acc[s], 0, 0, 0);
    }
    __syncthreads();                          // every wave has read h1
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int c = wave * 32 + mfma_row(v, h);
        const float bias = b2[c];
        f32x4 o;
#pragma unroll
        for (int s = 0; s < 4; ++s) o[s] = fmaxf(acc[s][v] + bias, 0.f);
        *reinterpret_cast<f32x4*>(&hbuf[c * PNT_T + 4 * j]) = o;
    }
}

// layer 3, one chunk: lane (j, h) holds W3[32 chunk + j][64 h .. 64 h + 63]; m[v] = the maximum over the tile's first
// `nvalid` points of channel 32 chunk + mfma_row(v, h), without the bias (the same value in all 32 lanes of the half wave)
__device__ __forceinline__ void pnt_layer3_chunk(const float* __restrict__ h2, const float* __restrict__ w3, int chunk, int j,
                                                 int h, int nvalid, float (&m)[16]) {
    f32x4 a[16];
    {
        const f32x4* wp = reinterpret_cast<const f32x4*>(w3 + (size_t)(chunk * 32 + j) * PNT_C2 + h * 64);
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = wp[i];
    }
    f32x16 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[s][v] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 64; ++kk) {
        if ((kk & 7) == 0) __builtin_amdgcn_sched_barrier(0);   // LDS reads run at most 8 steps ahead
        const f32x4 bv = *reinterpret_cast<const f32x4*>(&h2[(h * 64 + kk) * PNT_T + 4 * j]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk >> 2][kk & 3], bv[s], acc[s], 0, 0, 0);
    }
    if (nvalid < PNT_T) {
        const float ninf = -__builtin_huge_valf();
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (4 * j + s >= nvalid) {
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[s][v] = ninf;
            }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        float t = fmaxf(fmaxf(acc[0][v], acc[1][v]), fmaxf(acc[2][v], acc[3][v]));
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) t = fmaxf(t, __shfl_xor(t, o, 64));   // stays inside the half wave
        m[v] = t;
    }
}
