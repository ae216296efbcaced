// What the inference attention kernels share (attn_h_kernel of attention.hip, the unit-form kernels of attention_units.hip,
// the split backward of attention_bwd_h.hip): the pre-scales of their f16x2 operands (the split itself: f16x2.h) and the
// head pointer of a channel-major operand.
#pragma once
#include "f16x2.h"

constexpr float QK_PRE = 16.0f;      // q (after the softmax scale) and k are pre-scaled by 16
constexpr float P_PRE = 2048.0f;     // p in [0,1]
constexpr float P_LOG2 = 11.0f;      // log2(P_PRE)
constexpr float V_PRE = 16.0f;

__device__ __forceinline__ const float* head_ptr(const lc_cm_operand& x, int b, int h) {
    return x.p ? x.p + b * x.bs + h * x.hs : nullptr;
}
