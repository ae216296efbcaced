// Dense convolutions of RangeNet-53/-21: the extractor of the Frechet Range Image Distance
// (lidargen/metrics/models/rangenet/model.py) and of FRD (lidargen/metrics/extractor/rangenet.py).  Zero padding, stride
// (1,1) or (1,2), a transposed 1x4 up conv, folded BatchNorm + LeakyReLU(0.1) + up to two addends AFTER the activation.
// Exact fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered fma chain), no operand split, no range bookkeeping: the inputs are raw
// metres with -1 holes and a checkpoint of unknown scale.
//
//   rn_conv_kernel<MODE, CW>   one block = 4 waves = RN_TH (2) output rows x 32 * (4 / CW) pixels x 32 * CW output channels
//       wave w: output channels 32 (w % CW) .. + 31 (the MFMA's rows: the A operand is one packed weight per lane),
//               pixel group w / CW = 32 pixels (the MFMA's columns: lane l holds pixel l & 31 of channel 2 s + (l >> 5)),
//               one accumulator per output row (mode 3: per output row and column parity).
//       per chunk of KC input channels (16; 32 for the 1x1): the block stages [KC][rows + halo][columns + halo] of the
//       NCHW input in LDS, zeros where the image or the channels end -- one staged tile serves all taps (the next chunk's
//       tile is fetched into registers before this chunk's products start and stored after them); then for every
//       tap t and channel pair s one weight register feeds the MFMAs of both rows.  The chunk's products are summed in
//       accumulators that start at zero and are then added to the running total: no fma chain is longer than 9 * 16 = 144
//       terms (the guide's measured error is 0.75 - 1.5e-7 sum|ab| up to K = 1024, 3.5e-7 at 4096; the deepest layer has
//       K = 4608), the totals are a chain of at most 64 adds.
//   k order (fixed): chunk ascending; inside a chunk tap ascending (ky * 3 + kx; mode 3: k = 1, 3 for even output columns,
//       2, 0 for odd ones), inside a tap channel ascending.  A pixel's bits depend on its own receptive field only: not on
//       the batch, not on the run.  No atomics.
//   mode 3 (ConvTranspose2d kernel (1,4), stride (1,2), padding (0,1)) is two 1x2 convolutions: output column 2 j takes
//       taps k = 1 (input j) and k = 3 (input j - 1), column 2 j + 1 taps k = 2 (input j) and k = 0 (input j + 1).
//   epilogue: v = acc + bias[co]; act: v = v > 0 ? v : 0.1f v; v += res1; v += res2.
//   rn_reduce_kernel  one wave per output: the mean of a [rows x columns] window of one channel, lane-strided partial sums
//       in ascending order, then a butterfly -- fixed order, no atomics.
#include "common.h"
#include "f16x2.h"      // mfma_row

namespace {

constexpr int RN_TW = 32;                     // pixels per wave = MFMA columns
constexpr int RN_TH = 2;                      // output rows per block
constexpr int RN_CO = 32;                     // output channels per wave = MFMA rows

__host__ __device__ constexpr int rn_kc(int mode) { return mode == 0 ? 32 : 16; }
__host__ __device__ constexpr int rn_taps(int mode) { return mode == 0 ? 1 : (mode == 3 ? 4 : 9); }

struct RnArgs {
    const float* x;
    const float* wpk;
    const float* bias;
    const float* res1;
    const float* res2;
    float* y;
    int Ci, Co, H, W, Wo, act, co_groups;
};

template <int MODE, int CW>
struct RnGeom {
    static constexpr int KC = rn_kc(MODE), T = rn_taps(MODE);
    static constexpr int PG = 4 / CW, TWB = RN_TW * PG;           // pixel groups, pixels per block row
    static constexpr int S = MODE == 2 ? 2 : 1;
    static constexpr int NCOL = MODE == 0 ? TWB : (MODE == 2 ? 2 * TWB + 1 : TWB + 2);
    static constexpr int NROW = (MODE == 1 || MODE == 2) ? RN_TH + 2 : RN_TH;
    static constexpr int LDW = NCOL;
    // channel stride: odd modulo the 64 banks, so the two lane halves (channels 2 s, 2 s + 1) do not meet in every bank
    static constexpr int CS = NROW * LDW + ((33 - (NROW * LDW) % 64) + 64) % 64;
    static constexpr int NACC = MODE == 3 ? 2 * RN_TH : RN_TH;
};

template <int MODE, int CW>
__global__ __launch_bounds__(256, 2) void rn_conv_kernel(RnArgs a) {
    using G = RnGeom<MODE, CW>;
    constexpr int KC = G::KC, T = G::T, CS = G::CS, LDW = G::LDW, NACC = G::NACC;
    __shared__ float tile[KC * CS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int b = blockIdx.z / a.co_groups, cg = blockIdx.z - b * a.co_groups;
    const int p0 = blockIdx.x * G::TWB;       // first pixel column of the block (mode 3: input column, else output column)
    const int h0 = blockIdx.y * RN_TH;
    const int cb = cg * CW + wave % CW;       // block of 32 output channels
    const int pg = wave / CW;
    const bool live = cb * RN_CO < a.Co;
    const int nchunk = (a.Ci + KC - 1) / KC;
    const int col0 = MODE == 0 ? p0 : p0 * G::S - 1, row0 = G::NROW == RN_TH ? h0 : h0 - 1;
    const float* xb = a.x + (size_t)b * a.Ci * a.H * a.W;

    f32x16 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;

    // the next chunk's tile travels in registers while this chunk's products run
    // (not where the tile is wide or the accumulators many: the registers would spill; those blocks stage in place)
    constexpr int NE = KC * G::NROW * G::NCOL, NLD = (NE + 255) / 256;
    constexpr bool PF = NLD <= 17 && NLD + 32 * NACC <= 140;
    float stg[PF ? NLD : 1];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < (PF ? NLD : 0); ++i) {
            const int e = tid + 256 * i;
            const int ch = e / (G::NROW * G::NCOL), rem = e - ch * (G::NROW * G::NCOL);
            const int r = rem / G::NCOL, c = rem - r * G::NCOL;
            const int gc = chunk * KC + ch, gh = row0 + r, gw = col0 + c;
            float v = 0.f;
            if (e < NE && gc < a.Ci && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W) v = xb[((size_t)gc * a.H + gh) * a.W + gw];
            stg[i] = v;
        }
    };
    if (PF) fetch(0);
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        if (chunk) __syncthreads();           // every wave has read the previous chunk
        if constexpr (PF) {
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int e = tid + 256 * i;
                const int ch = e / (G::NROW * G::NCOL), rem = e - ch * (G::NROW * G::NCOL);
                const int r = rem / G::NCOL, c = rem - r * G::NCOL;
                if (e < NE) tile[ch * CS + r * LDW + c] = stg[i];
            }
        } else {
            for (int e = tid; e < NE; e += 256) {
                const int ch = e / (G::NROW * G::NCOL), rem = e - ch * (G::NROW * G::NCOL);
                const int r = rem / G::NCOL, c = rem - r * G::NCOL;
                const int gc = chunk * KC + ch, gh = row0 + r, gw = col0 + c;
                float v = 0.f;
                if (gc < a.Ci && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W) v = xb[((size_t)gc * a.H + gh) * a.W + gw];
                tile[ch * CS + r * LDW + c] = v;
            }
        }
        __syncthreads();
        if (PF && chunk + 1 < nchunk) fetch(chunk + 1);
        if (live) {
            f32x16 part[NACC];
#pragma unroll
            for (int i = 0; i < NACC; ++i)
#pragma unroll
                for (int v = 0; v < 16; ++v) part[i][v] = 0.f;
            const f32x4* wp = reinterpret_cast<const f32x4*>(a.wpk) + ((size_t)cb * nchunk + chunk) * (T * (KC / 8) * 64) + lane;
            const float* bp = &tile[h * CS + (pg * RN_TW + j) * G::S];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                // LDS offset of the tap and, in mode 3, the column parity it feeds
                const int dy = (MODE == 1 || MODE == 2) ? t / 3 : 0;
                const int dx = MODE == 0 ? 0 : (MODE == 3 ? (t == 1 ? 0 : (t == 3 ? 2 : 1)) : t % 3);
                const int par = MODE == 3 ? (t >= 2 ? 1 : 0) : 0;
#pragma unroll
                for (int q = 0; q < KC / 8; ++q) {
                    const f32x4 w4 = wp[(t * (KC / 8) + q) * 64];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int s = 4 * q + e;
#pragma unroll
                        for (int r = 0; r < RN_TH; ++r) {
                            const float bv = bp[2 * s * CS + (r + dy) * LDW + dx];
                            const int ai = MODE == 3 ? 2 * r + par : r;
                            part[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[e], bv, part[ai], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] += part[i];
        }
    }
    if (!live) return;

    const int px = p0 + pg * RN_TW + j;       // this lane's pixel column
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int r = MODE == 3 ? i >> 1 : i;
        const int oh = h0 + r, ow = MODE == 3 ? 2 * px + (i & 1) : px;
        if (oh >= a.H || ow >= a.Wo) continue;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int co = mfma_row(v, h, cb * RN_CO);
            if (co >= a.Co) continue;
            const size_t o = (((size_t)b * a.Co + co) * a.H + oh) * a.Wo + ow;
            float val = acc[i][v] + a.bias[co];
            if (a.act) val = val > 0.f ? val : 0.1f * val;
            if (a.res1) val += a.res1[o];
            if (a.res2) val += a.res2[o];
            a.y[o] = val;
        }
    }
}

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

template <int MODE, int CW>
int rn_launch(const RnArgs& a, int B, lc_stream_t s) {
    using G = RnGeom<MODE, CW>;
    const int Wp = MODE == 3 ? a.W : a.Wo;    // pixel columns the blocks tile
    const long long gx = (Wp + G::TWB - 1) / G::TWB, gy = (a.H + RN_TH - 1) / RN_TH, gz = (long long)B * a.co_groups;
    if (gx > 2147483647ll || gy > 65535 || gz > 65535) return LC_EUNSUP;
    hipLaunchKernelGGL((rn_conv_kernel<MODE, CW>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), 0, lc_s(s), a);
    return lc_launch_status();
}

template <int MODE>
int rn_dispatch(RnArgs& a, int B, lc_stream_t s) {
    // narrow layers give their waves to more pixels instead of idle channel blocks (mode 2 stages two input columns per
    // pixel: at most 64 pixels per block row)
    const int cw = a.Co <= 32 && MODE != 2 ? 1 : (a.Co <= 64 ? 2 : 4);
    a.co_groups = ((a.Co + RN_CO - 1) / RN_CO + cw - 1) / cw;
    if (cw == 1) {
        if constexpr (MODE != 2) return rn_launch<MODE, 1>(a, B, s);
    }
    if (cw == 2) return rn_launch<MODE, 2>(a, B, s);
    return rn_launch<MODE, 4>(a, B, s);
}

bool rn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int lc_rangenet_tile_extent(int which) {
    switch (which) {
        case 0: return RN_TW;
        case 1: return RN_TH;
        case 2: return RN_CO;
        case 3: return 4 * RN_TW;             // the widest block row (Co <= 32)
        default: return 0;
    }
}

extern "C" int64_t lc_rangenet_packed_weight_elems(int mode, int Ci, int Co) {
    if (mode < 0 || mode > 3 || Ci < 1 || Co < 1) return 0;
    const int KC = rn_kc(mode);
    return (int64_t)((Co + RN_CO - 1) / RN_CO) * ((Ci + KC - 1) / KC) * rn_taps(mode) * KC * RN_CO;
}

// HOST pointers.  w: modes 0-2 [Co][Ci][kh][kw] (Conv2d), mode 3 [Ci][Co][1][4] (ConvTranspose2d).  out: [co block]
// [chunk][tap][KC / 8][lane][4]: entry e of lane l is the weight of output channel 32 block + (l & 31), input channel
// KC chunk + 2 (4 q + e) + (l >> 5); zeros past Ci and Co.
extern "C" int lc_rangenet_pack_weight(const float* w, int mode, int Ci, int Co, float* out) {
    if (!w || !out || mode < 0 || mode > 3 || Ci < 1 || Co < 1) return LC_EINVAL;
    const int KC = rn_kc(mode), T = rn_taps(mode);
    const int nchunk = (Ci + KC - 1) / KC, ncb = (Co + RN_CO - 1) / RN_CO;
    size_t o = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int t = 0; t < T; ++t) {
                // mode 3: accumulation order k = 1, 3 (even columns), 2, 0 (odd columns)
                const int k = mode == 3 ? (t == 0 ? 1 : (t == 1 ? 3 : (t == 2 ? 2 : 0))) : t;
                for (int q = 0; q < KC / 8; ++q)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 4; ++e, ++o) {
                            const int co = cb * RN_CO + (l & 31), ci = ch * KC + 2 * (4 * q + e) + (l >> 5);
                            float v = 0.f;
                            if (co < Co && ci < Ci)
                                v = mode == 3 ? w[((size_t)ci * Co + co) * 4 + k] : w[((size_t)co * Ci + ci) * T + k];
                            out[o] = v;
                        }
            }
    return LC_OK;
}

extern "C" int lc_rangenet_conv_fwd(const float* x, const float* wpk, const float* bias, const float* res1,
                                    const float* res2, float* y, int B, int Ci, int Co, int H, int W, int mode, int act,
                                    lc_stream_t s) {
    if (!x || !wpk || !bias || !y || B < 1 || Ci < 1 || Co < 1 || H < 1 || W < 1 || mode < 0 || mode > 3) return LC_EINVAL;
    if (!rn_aligned16(wpk)) return LC_EUNSUP;                     // read as 128-bit quads
    if (W > (1 << 29) || H > (1 << 29)) return LC_EUNSUP;
    const int Wo = mode == 2 ? (W - 1) / 2 + 1 : (mode == 3 ? 2 * W : W);
    if (y == x || y == res1 || y == res2) return LC_EINVAL;       // a block reads pixels other blocks write
    RnArgs a{x, wpk, bias, res1, res2, y, Ci, Co, H, W, Wo, act ? 1 : 0, 1};
    switch (mode) {
        case 0: return rn_dispatch<0>(a, B, s);
        case 1: return rn_dispatch<1>(a, B, s);
        case 2: return rn_dispatch<2>(a, B, s);
        default: return rn_dispatch<3>(a, B, s);
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
