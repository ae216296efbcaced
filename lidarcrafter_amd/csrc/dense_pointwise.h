// The dense tile engine's pointwise geometry and epilogue (dense_f32.h): y = act(W x + b (+ res)) on
// [B, C, L].  One definition for the layers of csrc/pointmlp.hip and the gathered first layer of csrc/pointnet2_stack.hip.
#pragma once
#include "dense_f32.h"

// 1x1, one row per block, a wave = 32 output channels x 64 columns = two MFMA column groups per weight register
// (accumulator r reads LDS offset 32 r)
template <int CW_>
struct PwGeom {
    static constexpr int KC = 32, T = 1, CW = CW_;
    static constexpr int TH = 1, PXW = 2 * DF_TW;
    static constexpr bool FLAT = true;
    static constexpr int S = 1, PADH = 0, PADW = 0;
    static constexpr int R = 2, NACC = 2;
    static constexpr int PF_MAX_NLD = 32;
    static constexpr int lds_off(int r, int, int) { return DF_TW * r; }
    static constexpr int acc_of(int r, int) { return r; }
    static constexpr int out_row(int) { return 0; }
    __host__ __device__ static constexpr long long out_col(int i, long long px) { return px + DF_TW * i; }
};

// the residual is added BEFORE the activation (ReLU)
struct PwEpi {
    const float* bias;
    const float* res;
    float* y;
    int act;
    __device__ __forceinline__ void operator()(int co, size_t o, float acc) const {
        float val = acc + bias[co];
        if (res) val += res[o];
        if (act) val = val > 0.f ? val : 0.f;
        y[o] = val;
    }
};
