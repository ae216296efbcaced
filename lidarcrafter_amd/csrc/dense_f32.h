// The exact-fp32 dense tile engine on v_mfma_f32_32x32x2_f32 (a k-ordered fma chain, no operand split): ONE definition of
// the packed-weight layout, the LDS tile, the chunk loop and its barriers, the chunk product loop (and with it the k order),
// the epilogue walk and the dispatch, shared by the RangeNet convolutions (csrc/rangenet.hip, DESIGN.md section 5n: four
// geometries), the pointwise layers of PointMLP, GLENet's head and the classifiers (csrc/pointmlp.hip, section 5o: a fifth,
// dense_pointwise.h) and the gathered first layer of the stacked set abstraction (csrc/pointnet2_stack.hip, section 5s: the
// fifth again).  What differs stays with the files: the geometry (a policy struct, below), the epilogue (a functor called
// once per output value) and the operand source (how a chunk's tile gets into LDS; the contract stands at DfImageSrc, the
// default, which reads an NCHW image).
//
//   df_conv_kernel<G, E, Src>   one block = 4 waves = G::TH output rows x G::PXW * (4 / CW) pixels x 32 * CW output channels
//       wave w: output channels 32 (w % CW) .. + 31 (the MFMA's rows: the A operand is one packed weight per lane),
//               pixel group w / CW (the MFMA's columns: lane l holds pixel l & 31 of channel 2 s + (l >> 5)),
//               G::NACC accumulators, G::R of them fed by one weight register per tap.
//       per chunk of G::KC input channels the source stages [KC][rows + halo][columns + halo] of the operand in LDS, zeros
//       where the image or the channels end -- one staged tile serves all taps (the image source, where registers allow,
//       fetches the next chunk's tile into registers before this chunk's products start and stores it after them); then
//       for every tap t and channel pair s one weight register feeds G::R MFMAs.  The chunk's products are summed in
//       accumulators that start at zero and are then added to the running total: no fma chain is longer than T * KC terms
//       (the guide's measured error is 0.75 - 1.5e-7 sum|ab| up to K = 1024, 3.5e-7 at 4096), the totals are a chain of adds.
//   k order (fixed): chunk ascending; inside a chunk tap ascending, inside a tap channel ascending.  A pixel's bits depend on
//       its own receptive field only: not on the batch, not on the run, not on the geometry's tile.  No atomics.
//
// A geometry G supplies (all static constexpr):
//   KC, T, CW     input channels per chunk (a multiple of 8), taps, channel blocks (waves) per block: 1, 2 or 4
//   TH, PXW       output rows per block, tile pixels per wave
//   FLAT          the tensors are [B, C, L]: one row, known to the compiler (TH = 1, PADH = 0)
//   S             input columns per tile pixel (the stride)
//   PADH, PADW    halo rows / columns in front of the tile (as many behind it)
//   R, NACC       accumulators per weight register and tap, accumulators per wave
//   PF_MAX_NLD    the most staged registers per thread with which the geometry's kernels hold the next chunk's tile
//   lds_off(r, t, ldw)   LDS offset, from the lane's own pixel, of what accumulator slot r reads for tap t (ldw: row stride)
//   acc_of(r, t)         the accumulator that slot r of tap t feeds
//   out_row(i), out_col(i, px)   the output row (from the block's first) and column of accumulator i; px: the lane's tile pixel
//                        (px and the column are long long: a flat tensor may have up to 2^31 - 1 columns)
#pragma once
#include "common.h"
#include "f16x2.h"      // mfma_row

constexpr int DF_CO = 32;                     // output channels per wave = MFMA rows
constexpr int DF_TW = 32;                     // columns of one MFMA column group

struct DfArgs {
    const float* x;
    const float* wpk;
    int Ci, Co, H, W, Wo, co_groups;          // W: input columns, Wo: output columns
};

// channel stride of an LDS tile of n floats per channel: odd modulo the 64 banks, so the two lane halves (channels 2 s,
// 2 s + 1) do not meet in every bank
constexpr int df_bank_stride(int n) { return n + ((33 - n % 64) + 64) % 64; }

template <class G>
struct DfTile {
    static constexpr int PG = 4 / G::CW, TWB = G::PXW * PG;       // pixel groups, tile pixels per block row
    static constexpr int NROW = G::TH + 2 * G::PADH, NCOL = (TWB - 1) * G::S + 1 + 2 * G::PADW, LDW = NCOL;
    static constexpr int CS = df_bank_stride(NROW * LDW);
    static constexpr int NE = G::KC * NROW * NCOL, NLD = (NE + 255) / 256;
    // the next chunk's tile travels in registers while this chunk's products run
    // (not where the tile is wide or the accumulators many: the registers would spill; those blocks stage in place)
    static constexpr bool PF = NLD <= G::PF_MAX_NLD && NLD + 32 * G::NACC <= 140;
};

// ---- packed weights (host) -------------------------------------------------------------------------------------------
inline int64_t df_packed_elems(int KC, int T, int Ci, int Co) {
    return (int64_t)((Co + DF_CO - 1) / DF_CO) * ((Ci + KC - 1) / KC) * T * KC * DF_CO;
}

// out: [co block][chunk][tap][KC / 8][lane][4]: entry e of lane l is the weight of output channel 32 block + (l & 31), input
// channel KC chunk + 2 (4 q + e) + (l >> 5); zeros past Ci and Co.  w(co, ci, tap): the layer's weight, taps in k order.
template <class W>
void df_pack_weight(int KC, int T, int Ci, int Co, float* out, W w) {
    const int nchunk = (Ci + KC - 1) / KC, ncb = (Co + DF_CO - 1) / DF_CO;
    size_t o = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int t = 0; t < T; ++t)
                for (int q = 0; q < KC / 8; ++q)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 4; ++e, ++o) {
                            const int co = cb * DF_CO + (l & 31), ci = ch * KC + 2 * (4 * q + e) + (l >> 5);
                            out[o] = (co < Co && ci < Ci) ? w(co, ci, t) : 0.f;
                        }
}

// ---- operand sources -------------------------------------------------------------------------------------------------
// A source Src travels to the kernel by value; Src::Stage<G> is its state in a thread and owns how a chunk's
// [KC][NROW][NCOL] tile gets into LDS:
//   LDS_SETUP                     setup() writes LDS of its own that a barrier must publish before the first fill()
//   setup(src, a, b, p0, h0)      once, before the chunk loop; b: the sample, p0 / h0: the block's first tile pixel / row
//   fill(tile, chunk)             the block writes the chunk's tile
//   published(chunk)              after the barrier that publishes the tile
// The image source: DfArgs::x is [B, Ci, H, W].  Where DfTile<G>::PF, the next chunk's tile is fetched into registers
// behind the barrier and stored by the next fill().
struct DfImageSrc {
    template <class G>
    struct Stage {
        using D = DfTile<G>;
        static constexpr int KC = G::KC, CS = D::CS, LDW = D::LDW, NROW = D::NROW, NCOL = D::NCOL, NE = D::NE, NLD = D::NLD;
        static constexpr bool PF = D::PF, LDS_SETUP = false;
        const float* xb;
        int Ci, H, W, row0, col0;
        float stg[PF ? NLD : 1];

        // element e of the staged tile [KC][NROW][NCOL]: its channel, row and column, its place in LDS and its value (zero
        // outside the image and past Ci).  A tile of whole 256-element passes needs no test of e.
        __device__ __forceinline__ static void split(int e, int& ch, int& r, int& c) {
            ch = e / (NROW * NCOL);
            const int rem = e - ch * (NROW * NCOL);
            r = rem / NCOL, c = rem - r * NCOL;
        }
        __device__ __forceinline__ static int lds_of(int e) {
            int ch, r, c;
            split(e, ch, r, c);
            return ch * CS + r * LDW + c;
        }
        __device__ __forceinline__ float value_of(int chunk, int e) const {
            int ch, r, c;
            split(e, ch, r, c);
            const int gc = chunk * KC + ch, gh = row0 + r;
            // unsigned: in the last block of a flat tensor of nearly 2^31 columns the sum passes INT_MAX; a column in front
            // of the image wraps to above every W
            const unsigned gw = (unsigned)col0 + (unsigned)c;
            float v = 0.f;
            if ((NE % 256 == 0 || e < NE) && gc < Ci && gh >= 0 && gh < H && gw < (unsigned)W)
                v = xb[((size_t)gc * H + gh) * W + gw];
            return v;
        }
        __device__ __forceinline__ void fetch(int chunk) {
#pragma unroll
            for (int i = 0; i < (PF ? NLD : 0); ++i) stg[i] = value_of(chunk, threadIdx.x + 256 * i);
        }
        __device__ __forceinline__ void setup(const DfImageSrc&, const DfArgs& a, int b, int p0, int h0) {
            Ci = a.Ci, H = G::FLAT ? 1 : a.H, W = a.W;
            col0 = p0 * G::S - G::PADW, row0 = h0 - G::PADH;
            xb = a.x + (size_t)b * Ci * H * W;
            if (PF) fetch(0);
        }
        __device__ __forceinline__ void fill(float* tile, int chunk) const {
            const int tid = threadIdx.x;
            if constexpr (PF) {
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const int e = tid + 256 * i;
                    if (NE % 256 == 0 || e < NE) tile[lds_of(e)] = stg[i];
                }
            } else {
                for (int e = tid; e < NE; e += 256) tile[lds_of(e)] = value_of(chunk, e);
            }
        }
        __device__ __forceinline__ void published(int chunk) {
            if (PF && (chunk + 1) * KC < Ci) fetch(chunk + 1);
        }
    };
};

// ---- kernel ----------------------------------------------------------------------------------------------------------
// epi(co, o, v): the epilogue of output channel co at element offset o of the contiguous [B, Co, H, Wo] output, v its sum
template <class G, class E, class Src = DfImageSrc>
__global__ __launch_bounds__(256, 2) void df_conv_kernel(DfArgs a, E epi, Src from) {
    using D = DfTile<G>;
    using Stage = typename Src::template Stage<G>;
    constexpr int KC = G::KC, T = G::T, CW = G::CW, CS = D::CS, LDW = D::LDW, NACC = G::NACC;
    static_assert(KC % 8 == 0 && (CW == 1 || CW == 2 || CW == 4), "a chunk is whole weight quads, a block is 4 waves");
    static_assert(!G::FLAT || (G::TH == 1 && G::PADH == 0), "a flat geometry has one row");
    __shared__ float tile[KC * CS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int b = blockIdx.z / a.co_groups, cg = blockIdx.z - b * a.co_groups;
    const int p0 = blockIdx.x * D::TWB;       // first tile pixel of the block
    const int H = G::FLAT ? 1 : a.H, h0 = G::FLAT ? 0 : blockIdx.y * G::TH;
    const int cb = cg * CW + wave % CW;       // block of 32 output channels
    const int pg = wave / CW;
    const bool live = cb * DF_CO < a.Co;
    const int nchunk = (a.Ci + KC - 1) / KC;

    f32x16 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;

    Stage src;
    src.setup(from, a, b, p0, h0);
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        if (chunk || Stage::LDS_SETUP) __syncthreads();           // every wave has read the previous chunk
        src.fill(tile, chunk);
        __syncthreads();
        src.published(chunk);
        if (live) {
            f32x16 part[NACC];
#pragma unroll
            for (int i = 0; i < NACC; ++i)
#pragma unroll
                for (int v = 0; v < 16; ++v) part[i][v] = 0.f;
            const f32x4* wp = reinterpret_cast<const f32x4*>(a.wpk) + ((size_t)cb * nchunk + chunk) * (T * (KC / 8) * 64) + lane;
            const float* bp = &tile[h * CS + (pg * G::PXW + j) * G::S];
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int q = 0; q < KC / 8; ++q) {
                    const f32x4 w4 = wp[(t * (KC / 8) + q) * 64];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int s = 4 * q + e;
#pragma unroll
                        for (int r = 0; r < G::R; ++r) {
                            const float bv = bp[2 * s * CS + G::lds_off(r, t, LDW)];
                            const int ai = G::acc_of(r, t);
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

    // this lane's tile pixel; 64 bits: in the last block of a flat tensor of nearly 2^31 columns it passes INT_MAX
    const long long px = (long long)p0 + pg * G::PXW + j;
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int oh = h0 + G::out_row(i);
        const long long ow = G::out_col(i, px);
        if (oh >= H || ow >= a.Wo) continue;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int co = mfma_row(v, h, cb * DF_CO);
            if (co >= a.Co) continue;
            epi(co, (((size_t)b * a.Co + co) * H + oh) * a.Wo + ow, acc[i][v]);
        }
    }
}

// ---- launch ----------------------------------------------------------------------------------------------------------
// cols: the pixel columns the blocks tile; src: the operand source (by default the image DfArgs::x)
template <class G, class E, class Src = DfImageSrc>
int df_launch(const DfArgs& a, const E& epi, int B, long long cols, lc_stream_t s, const Src& src = Src()) {
    constexpr int TWB = DfTile<G>::TWB;
    const long long gx = (cols + TWB - 1) / TWB, gy = (a.H + G::TH - 1) / G::TH, gz = (long long)B * a.co_groups;
    if (gx > 2147483647ll || gy > 65535 || gz > 65535) return LC_EUNSUP;
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz);
    hipLaunchKernelGGL((df_conv_kernel<G, E, Src>), grid, dim3(256), 0, lc_s(s), a, epi, src);
    return lc_launch_status();
}

// GF<CW>: the geometry family.  Narrow layers give their waves to more pixels instead of idle channel blocks; MINCW: the
// fewest channel blocks per block the family has.
template <template <int> class GF, int MINCW = 1, class E, class Src = DfImageSrc>
int df_dispatch(DfArgs a, const E& epi, int B, long long cols, lc_stream_t s, const Src& src = Src()) {
    const int cw = a.Co <= 32 && MINCW == 1 ? 1 : (a.Co <= 64 ? 2 : 4);
    a.co_groups = ((a.Co + DF_CO - 1) / DF_CO + cw - 1) / cw;
    if constexpr (MINCW == 1) {
        if (cw == 1) return df_launch<GF<1>>(a, epi, B, cols, s, src);
    }
    if (cw == 2) return df_launch<GF<2>>(a, epi, B, cols, s, src);
    return df_launch<GF<4>>(a, epi, B, cols, s, src);
}
