// Dense convolutions of RangeNet-53/-21: the extractor of the Frechet Range Image Distance
// (lidargen/metrics/models/rangenet/model.py) and of FRD (lidargen/metrics/extractor/rangenet.py).  Zero padding, stride
// (1,1) or (1,2), a transposed 1x4 up conv, folded BatchNorm + LeakyReLU(0.1) + up to two addends AFTER the activation.
// Exact fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered fma chain), no operand split, no range bookkeeping: the inputs are raw
// metres with -1 holes and a checkpoint of unknown scale.
//
// The kernel, the packed-weight layout, the staging and the k order are the dense tile engine's (dense_f32.h); this file
// holds what is RangeNet's: the four geometries, the epilogue and the reduction.
//   RnMode<MODE>::Geom<CW>   one block = RN_TH (2) output rows x 32 * (4 / CW) pixels x 32 * CW output channels, one
//       accumulator per output row (mode 3: per output row and column parity); chunks of 16 input channels (32 for the
//       1x1): no fma chain is longer than 9 * 16 = 144 terms (the deepest layer has K = 4608), the totals are a chain of at
//       most 64 adds.
//   taps in k order: ky * 3 + kx; mode 3: k = 1, 3 for even output columns, 2, 0 for odd ones.
//   mode 3 (ConvTranspose2d kernel (1,4), stride (1,2), padding (0,1)) is two 1x2 convolutions: output column 2 j takes
//       taps k = 1 (input j) and k = 3 (input j - 1), column 2 j + 1 taps k = 2 (input j) and k = 0 (input j + 1).  Its
//       blocks tile the INPUT columns.
//   epilogue: v = acc + bias[co]; act: v = v > 0 ? v : 0.1f v; v += res1; v += res2.
//   rn_reduce_kernel  one wave per output: the mean of a [rows x columns] window of one channel, lane-strided partial sums
//       in ascending order, then a butterfly -- fixed order, no atomics.
#include "dense_f32.h"

namespace {

constexpr int RN_TH = 2;                      // output rows per block

constexpr int rn_kc(int mode) { return mode == 0 ? 32 : 16; }
constexpr int rn_taps(int mode) { return mode == 0 ? 1 : (mode == 3 ? 4 : 9); }

template <int MODE>
struct RnMode {
    template <int CW_>
    struct Geom {
        static constexpr int KC = rn_kc(MODE), T = rn_taps(MODE), CW = CW_;
        static constexpr int TH = RN_TH, PXW = DF_TW;
        static constexpr bool FLAT = false;
        static constexpr int S = MODE == 2 ? 2 : 1;
        static constexpr int PADH = (MODE == 1 || MODE == 2) ? 1 : 0, PADW = MODE == 0 ? 0 : 1;
        static constexpr int R = RN_TH, NACC = MODE == 3 ? 2 * RN_TH : RN_TH;
        static constexpr int PF_MAX_NLD = 17;
        // LDS offset of the tap and, in mode 3, the column parity it feeds
        static constexpr int dy(int t) { return (MODE == 1 || MODE == 2) ? t / 3 : 0; }
        static constexpr int dx(int t) { return MODE == 0 ? 0 : (MODE == 3 ? (t == 1 ? 0 : (t == 3 ? 2 : 1)) : t % 3); }
        static constexpr int par(int t) { return MODE == 3 ? (t >= 2 ? 1 : 0) : 0; }
        static constexpr int lds_off(int r, int t, int ldw) { return (r + dy(t)) * ldw + dx(t); }
        static constexpr int acc_of(int r, int t) { return MODE == 3 ? 2 * r + par(t) : r; }
        static constexpr int out_row(int i) { return MODE == 3 ? i >> 1 : i; }
        __host__ __device__ static constexpr long long out_col(int i, long long px) { return MODE == 3 ? 2 * px + (i & 1) : px; }
    };
};

struct RnEpi {
    const float* bias;
    const float* res1;
    const float* res2;
    float* y;
    int act;
    __device__ __forceinline__ void operator()(int co, size_t o, float acc) const {
        float val = acc + bias[co];
        if (act) val = val > 0.f ? val : 0.1f * val;
        if (res1) val += res1[o];
        if (res2) val += res2[o];
        y[o] = val;
    }
};

// kind 0: the whole map; 1: 16 column bands; 2: 16 row bands.  One wave per (b, c, band).
__global__ __launch_bounds__(64) void rn_reduce_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H,
                                                      int W, int kind) {
    const int nb = kind == 0 ? 1 : 16;
    const int n = blockIdx.x % nb, bc = blockIdx.x / nb, lane = threadIdx.x;
    const int nr = kind == 2 ? H / 16 : H, nc = kind == 1 ? W / 16 : W;
    const int r0 = kind == 2 ? n * nr : 0, c0 = kind == 1 ? n * nc : 0;
    const float* p = x + (size_t)bc * H * W;
    float s = 0.f;
    for (int i = lane; i < nr * nc; i += 64) {
        const int r = i / nc, c = i - r * nc;
        s += p[(size_t)(r0 + r) * W + c0 + c];
    }
    s = lc_wave_sum(s);
    if (lane == 0) out[blockIdx.x] = s / (float)(nr * nc);
}

// mode 2 stages two input columns per pixel: at most 64 pixels per block row
template <int MODE>
int rn_dispatch(const DfArgs& a, const RnEpi& epi, int B, lc_stream_t s) {
    return df_dispatch<RnMode<MODE>::template Geom, MODE == 2 ? 2 : 1>(a, epi, B, MODE == 3 ? a.W : a.Wo, s);
}

}  // namespace

extern "C" int lc_rangenet_tile_extent(int which) {
    switch (which) {
        case 0: return DF_TW;
        case 1: return RN_TH;
        case 2: return DF_CO;
        case 3: return 4 * DF_TW;             // the widest block row (Co <= 32)
        default: return 0;
    }
}

extern "C" int64_t lc_rangenet_packed_weight_elems(int mode, int Ci, int Co) {
    if (mode < 0 || mode > 3 || Ci < 1 || Co < 1) return 0;
    return df_packed_elems(rn_kc(mode), rn_taps(mode), Ci, Co);
}

// HOST pointers.  w: modes 0-2 [Co][Ci][kh][kw] (Conv2d), mode 3 [Ci][Co][1][4] (ConvTranspose2d).  out: the engine's
// layout (dense_f32.h: df_pack_weight).
extern "C" int lc_rangenet_pack_weight(const float* w, int mode, int Ci, int Co, float* out) {
    if (!w || !out || mode < 0 || mode > 3 || Ci < 1 || Co < 1) return LC_EINVAL;
    const int T = rn_taps(mode);
    df_pack_weight(rn_kc(mode), T, Ci, Co, out, [=](int co, int ci, int t) {
        // mode 3: accumulation order k = 1, 3 (even columns), 2, 0 (odd columns)
        if (mode == 3) return w[((size_t)ci * Co + co) * 4 + (t == 0 ? 1 : (t == 1 ? 3 : (t == 2 ? 2 : 0)))];
        return w[((size_t)co * Ci + ci) * T + t];
    });
    return LC_OK;
}

extern "C" int lc_rangenet_conv_fwd(const float* x, const float* wpk, const float* bias, const float* res1,
                                    const float* res2, float* y, int B, int Ci, int Co, int H, int W, int mode, int act,
                                    lc_stream_t s) {
    if (!x || !wpk || !bias || !y || B < 1 || Ci < 1 || Co < 1 || H < 1 || W < 1 || mode < 0 || mode > 3) return LC_EINVAL;
    if (!lc_aligned16(wpk)) return LC_EUNSUP;                     // read as 128-bit quads
    if (W > (1 << 29) || H > (1 << 29)) return LC_EUNSUP;
    const int Wo = mode == 2 ? (W - 1) / 2 + 1 : (mode == 3 ? 2 * W : W);
    if (y == x || y == res1 || y == res2) return LC_EINVAL;       // a block reads pixels other blocks write
    const DfArgs a{x, wpk, Ci, Co, H, W, Wo, 1};
    const RnEpi epi{bias, res1, res2, y, act ? 1 : 0};
    switch (mode) {
        case 0: return rn_dispatch<0>(a, epi, B, s);
        case 1: return rn_dispatch<1>(a, epi, B, s);
        case 2: return rn_dispatch<2>(a, epi, B, s);
        default: return rn_dispatch<3>(a, epi, B, s);
    }
}

extern "C" int lc_rangenet_reduce_fwd(const float* x, float* out, int B, int C, int H, int W, int kind, lc_stream_t s) {
    if (!x || !out || B < 1 || C < 1 || H < 1 || W < 1 || kind < 0 || kind > 2) return LC_EINVAL;
    if ((kind == 1 && W % 16) || (kind == 2 && H % 16)) return LC_EUNSUP;
    const long long n = (long long)B * C * (kind == 0 ? 1 : 16);
    if (n > 2147483647ll || (long long)H * W > 2147483647ll) return LC_EUNSUP;
    hipLaunchKernelGGL(rn_reduce_kernel, dim3((unsigned)n), dim3(64), 0, lc_s(s), x, out, C, H, W, kind);
    return lc_launch_status();
}
