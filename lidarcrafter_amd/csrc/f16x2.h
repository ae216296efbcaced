// THE f16x2 operand split: its rule, every form of it, and what the MFMA kernels share around it.
//
// An fp32 value v is multiplied by a power-of-two scale, s = v * scale, and cut in two fp16 halves
//     hi = s with the low 13 significand bits cleared (11 significant bits: exact in fp32), packed toward zero;
//     lo = fp16(s - hi), RTNE, of the MASKED fp32 value, not of the packed one;
// and a product a * b is accumulated in fp32 as the three fp16 products al * bh + ah * bl + ah * bh on
// v_mfma_f32_32x32x16_f16 (the dropped al * bl term is 2^-22 relative).  hi is exact below 65504 and saturates at
// +-65504 (never inf) above; under 2^-14 it is subnormal in fp16 and loses its low bits toward zero; lo is subnormal below
// 2^-14 and (signed) zero below 2^-25.  Zeros keep their sign in hi; lo of an exact hi is +0.  `amax` accumulates max |s|,
// which the range records publish.  (tests/test_gn_split_stores.py pins all of this bit for bit.)
//
// pair_split / f16x2_split_scalar are the only code that holds the mask and the pack.
#pragma once
#include "common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));     // (`half2` is HIP's __half2)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));                  // (four: lc_u32x4 of common.h)

// ---- the rule ------------------------------------------------------------------------------------------------------------

#ifndef LC_SPLIT_ABL
#define LC_SPLIT_ABL 0   // developer ablation: 1 no amax accumulation, 2 round-to-nearest split
#endif

// THE pair rule: two values that already carry their scale -> their packed hi and lo halves
__device__ __forceinline__ void pair_split(float s0, float s1, half2v& ph, half2v& pl) {
    if (LC_SPLIT_ABL & 2) {
        const _Float16 a0 = (_Float16)s0, a1 = (_Float16)s1;
        ph.x = a0; ph.y = a1;
        pl.x = (_Float16)(s0 - (float)a0); pl.y = (_Float16)(s1 - (float)a1);
        return;
    }
    const float h0 = __uint_as_float(__float_as_uint(s0) & 0xFFFFE000u);
    const float h1 = __uint_as_float(__float_as_uint(s1) & 0xFFFFE000u);
    ph = __builtin_bit_cast(half2v, __builtin_amdgcn_cvt_pkrtz(h0, h1));
    f32x2 r; r.x = s0 - h0; r.y = s1 - h1;
    pl = __builtin_convertvector(r, half2v);
}
// max |s| so far (v_max3_f32)
__device__ __forceinline__ float pair_amax(float am, float s0, float s1) {
    if (LC_SPLIT_ABL & 1) return am;
    return __builtin_fmaxf(am, __builtin_fmaxf(__builtin_fabsf(s0), __builtin_fabsf(s1)));
}
// the pair rule with max |s| accumulated
__device__ __forceinline__ void pair_split_amax(float s0, float s1, half2v& ph, half2v& pl, float& am) {
    am = pair_amax(am, s0, s1);
    pair_split(s0, s1, ph, pl);
}
// ... with the scale multiply
template <bool NOPACK = false>
__device__ __forceinline__ void pair_split_scale(float v0, float v1, float scale, half2v& ph, half2v& pl, float& am) {
    float s0 = v0 * scale, s1 = v1 * scale;
    // NOPACK: keep hipcc's SLP vectoriser from fusing the two multiplies into v_pk_mul_f32 -- the
    // packed form needs an aligned register pair, and in the 2-blocks/CU kernel the v_mov_b64 that
    // builds it (with its s_waitcnt) lands between the global loads of the next chunk and
    // serialises them (1x1 convs 26 -> 35 us, 33 -> 61 us, measured r02g)
    if (NOPACK) asm volatile("" : "+v"(s0), "+v"(s1));
    pair_split_amax(s0, s1, ph, pl, am);
}

// eight values -> one hi and one lo MFMA operand register; `scale` is multiplied in, with and without amax
template <bool NOPACK = false>
__device__ __forceinline__ void split8(const float (&v)[8], float scale, half8& hi, half8& lo, float& am) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        half2v ph, pl;
        pair_split_scale<NOPACK>(v[k], v[k + 1], scale, ph, pl, am);
        hi[k] = ph.x; hi[k + 1] = ph.y; lo[k] = pl.x; lo[k + 1] = pl.y;
    }
}
__device__ __forceinline__ void split8(const float (&v)[8], float scale, half8& hi, half8& lo) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        half2v ph, pl;
        pair_split(v[k] * scale, v[k + 1] * scale, ph, pl);
        hi[k] = ph.x; hi[k + 1] = ph.y; lo[k] = pl.x; lo[k + 1] = pl.y;
    }
}
// ... the inference attention kernels' form: a scale of exactly 1 is not multiplied in.  v * 1 == v, so the halves are the
// same; the form is kept because it is those kernels' instruction text (a compare and a select per value).
__device__ __forceinline__ void split8_skip1(const float (&v)[8], float scale, half8& hi, half8& lo) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        half2v ph, pl;
        pair_split(scale == 1.0f ? v[k] : v[k] * scale, scale == 1.0f ? v[k + 1] : v[k + 1] * scale, ph, pl);
        hi[k] = ph.x; hi[k + 1] = ph.y; lo[k] = pl.x; lo[k + 1] = pl.y;
    }
}
// four values (conv_bwd.hip: one 16-byte load of a channel row)
__device__ __forceinline__ void split4(const f32x4 v, float scale, half4& hi, half4& lo) {
    half2v a, b, c, d;
    pair_split(v.x * scale, v.y * scale, a, c);
    pair_split(v.z * scale, v.w * scale, b, d);
    hi = half4{a.x, a.y, b.x, b.y};
    lo = half4{c.x, c.y, d.x, d.y};
}

// The scalar form, for one element per thread (weight packing, halo columns): no second value to pack with, so no pack
// builtin -- hi is exact in 11 bits, and a plain conversion of it is exact wherever fp16 holds it.
__device__ __forceinline__ void f16x2_split_scalar(float s, _Float16& hi, _Float16& lo) {
    const float hf = __uint_as_float(__float_as_uint(s) & 0xFFFFE000u);
    hi = (_Float16)hf;
    lo = (_Float16)(s - hf);
}

// ---- the range record -------------------------------------------------------------------------------------------------

// publish the wave's max |x * x_scale| (am >= 0: unsigned order == float order); a cached read
// keeps all but the first few blocks of a launch off the atomic
#ifndef LC_RANGE_ABL
#define LC_RANGE_ABL 0   // developer ablation: 1 no amax publish, 2 constant scales (no device loads)
#endif
__device__ __forceinline__ void publish_amax(lc_conv_range* rg, float am, float seen) {
    if (LC_RANGE_ABL & 1) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = __builtin_fmaxf(am, __shfl_xor(am, o, 64));
    if ((threadIdx.x & 63) == 0 && am > seen)
        atomicMax(reinterpret_cast<unsigned*>(&rg->amax_scaled), __float_as_uint(am));
}

// ---- the 32 x 32 MFMA ----------------------------------------------------------------------------------------------------

// C/D row of accumulator register r (0 .. 15) in lane half `half` (lane >> 5); the column is lane & 31.  The same map
// orders the k index of a B operand taken from a previous product's accumulator registers.  `base`: the row is counted
// from there -- where r is still a loop variable when the sum is formed, base + mfma_row(r) and this are different code.
__device__ __forceinline__ constexpr int mfma_row(int r, int half = 0, int base = 0) {
    return base + (r & 3) + 8 * (r >> 2) + 4 * half;
}

#ifndef LC_F16X2_TERMS
// which of the three products are accumulated: bit 0 ah*bh, bit 1 al*bh, bit 2 ah*bl.  7 in the
// product library; 3 / 5 exist only to MEASURE what fewer passes cost in accuracy
// (devtools/passes_error.py, profiles/r02_passes_error.json); 1 = the single-product build
// liblidarcrafter_hip_p1.so that serves callers running under fp16 autocast (ops.conv_products).
#define LC_F16X2_TERMS 7
#endif

// THE triple product: acc + al * bh + ah * bl + ah * bh, issued back to back in this order (the order of accumulation
// is part of every kernel's result).  Kernels of the single-product build pass TERMS = LC_F16X2_TERMS.
template <int TERMS = 7>
__device__ __forceinline__ f32x16 f16x2_mma(f32x16 acc, const half8 ah, const half8 al, const half8 bh, const half8 bl) {
    if (TERMS & 2) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
    if (TERMS & 4) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}
