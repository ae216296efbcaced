// Which way a weight-gradient call runs: the pure functions the launchers and kernels of conv_bwd.hip switch on, in ONE
// place, and exported to the tests as lc_conv2d_ring_wgrad_route, so that the case table of tests/test_train_edges_host.py
// is proven against the library's own choice (the pattern of attention_route.h).  No arithmetic lives here.
//
//   out[0] family        1 conv_wgrad_kernel (exact fp32 MFMA), 2 conv_wgrad_h_kernel (f16x2 split)
//   out[1] staging       1 float4 staging, 0 scalar staging (the split kernel only has the float4 form)
//   out[2] nsplit        blocks per channel tile = partial sums per weight (wgrad_splits; BOTH kernels use this count)
//   out[3] tiles         pixel tiles of the chosen kernel: B H ceil(W / 64) (fp32), B (H / 2) (W / 32) (split)
//   out[4] bias branch   1 every (sample, channel) plane takes the float4 loop, 0 none does, 2 it differs by sample
//   out[5] bias offset   floats in front of the fp64 bias partials in the scratch (an even count)
//   out[6] causes        fp32 kernel: which conditions of the float4 staging fail (LC_WGRAD_SCALAR_*), 0 = none
//   out[7] 0
#pragma once

#include "../../include/lidarcrafter_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC_ROUTE_HD __host__ __device__
#else
#define LC_ROUTE_HD
#endif

constexpr int LC_WGRAD_F32 = 1, LC_WGRAD_SPLIT = 2;
constexpr int LC_WGRAD_TW = 64;                       // columns of a pixel tile of the fp32 kernel (one image row)
constexpr int LC_WGRAD_H_TR = 2, LC_WGRAD_H_TW = 32;  // rows x columns of a pixel tile of the split kernel

// why conv_wgrad_kernel stages with scalar loads
constexpr int LC_WGRAD_SCALAR_W = 1,        // W % 64: the last tile of a row is partial
              LC_WGRAD_SCALAR_HW = 2,       // H W % 4: a channel plane does not start on 16 bytes
              LC_WGRAD_SCALAR_XBS = 4,      // x_bs % 4
              LC_WGRAD_SCALAR_DYBS = 8,     // dy_bs % 4
              LC_WGRAD_SCALAR_XADDR = 16,   // x off 16 bytes
              LC_WGRAD_SCALAR_DYADDR = 32;  // dy off 16 bytes

// float4 staging when rows are 16-byte aligned and tiles are whole: 0, else the failing conditions
LC_ROUTE_HD inline int lc_wgrad_scalar_causes(int W, long long HW, long long x_bs, long long dy_bs, int x_addr_mod16,
                                              int dy_addr_mod16) {
    return ((W % LC_WGRAD_TW) != 0 ? LC_WGRAD_SCALAR_W : 0) | ((HW & 3) != 0 ? LC_WGRAD_SCALAR_HW : 0) |
           ((x_bs & 3) != 0 ? LC_WGRAD_SCALAR_XBS : 0) | ((dy_bs & 3) != 0 ? LC_WGRAD_SCALAR_DYBS : 0) |
           ((x_addr_mod16 & 15) != 0 ? LC_WGRAD_SCALAR_XADDR : 0) | ((dy_addr_mod16 & 15) != 0 ? LC_WGRAD_SCALAR_DYADDR : 0);
}

LC_ROUTE_HD inline int lc_wgrad_tiles_w(int W) { return (W + LC_WGRAD_TW - 1) / LC_WGRAD_TW; }
LC_ROUTE_HD inline int lc_wgrad_tiles(int B, int H, int W) { return B * H * lc_wgrad_tiles_w(W); }
LC_ROUTE_HD inline int lc_wgrad_h_tiles(int B, int H, int W) { return B * (H / LC_WGRAD_H_TR) * (W / LC_WGRAD_H_TW); }

// the split kernel wants whole 2 x 32 tiles and 16-byte aligned rows (anything else: lc_conv2d_ring_wgrad)
inline bool lc_wgrad_h_unsupported(int H, int W, long long x_bs, long long dy_bs, int x_addr_mod16, int dy_addr_mod16) {
    return (H & 1) || (W & 31) || (x_bs & 3) || (dy_bs & 3) || (x_addr_mod16 & 15) || (dy_addr_mod16 & 15);
}

inline int lc_wgrad_splits(int B, int Ci, int Co, int H, int W) {
    const int tiles = lc_wgrad_tiles(B, H, W);
    const int ctiles = ((Co + 63) / 64) * ((Ci + 63) / 64);
    int n = (512 + ctiles - 1) / ctiles;              // one full wave of blocks (2 resident per CU): equal
                                                      // work per block, and half the partials to reduce
    if (n > tiles) n = tiles;
    if (n < 1) n = 1;
    return n;
}

// scratch: nsplit x Co x Ci x ks x ks weight partials (rounded up to an even count of floats), then Co * B fp64 bias partials
inline long long lc_wgrad_bias_offset(int nsplit, int Ci, int Co, int ks) {
    return ((long long)nsplit * Co * Ci * ks * ks + 1) & ~1LL;
}
inline long long lc_wgrad_scratch_elems(int nsplit, int B, int Ci, int Co, int ks) {
    return lc_wgrad_bias_offset(nsplit, Ci, Co, ks) + 2 * (long long)Co * B;
}

// bias_grad_plane_kernel: float4 loads of a (sample, channel) plane that is whole float4s and starts on 16 bytes
LC_ROUTE_HD inline bool lc_bias_grad_vec(long long HW, int plane_addr_mod16) {
    return (HW & 3) == 0 && (plane_addr_mod16 & 15) == 0;
}

// 1 / 0 / 2 (see out[4]): plane (b, c) of a tensor at `addr_mod16` with batch stride `bs` starts at addr + 4 (b bs + c HW)
inline int lc_planes_vec(int B, long long HW, long long bs, int addr_mod16) {
    if (HW & 3) return 0;
    int n = 0;
    const int nb = B < 4 ? B : 4;                     // 4 b bs mod 16 has period 4 in b
    for (int b = 0; b < nb; ++b) n += ((addr_mod16 + 4 * (int)((b * bs) & 3)) & 15) == 0;
    return n == nb ? 1 : (n == 0 ? 0 : 2);
}

inline int lc_wgrad_route(int split, int B, int Ci, int Co, int H, int W, int ks, long long x_bs, long long dy_bs,
                          int x_addr_mod16, int dy_addr_mod16, int32_t out[8]) {
    if (!out || B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return LC_EINVAL;
    if (ks != 1 && ks != 3) return LC_EUNSUP;
    if (split && lc_wgrad_h_unsupported(H, W, x_bs, dy_bs, x_addr_mod16, dy_addr_mod16)) return LC_EUNSUP;
    const int nsplit = lc_wgrad_splits(B, Ci, Co, H, W);
    const int causes = split ? 0 : lc_wgrad_scalar_causes(W, (long long)H * W, x_bs, dy_bs, x_addr_mod16, dy_addr_mod16);
    out[0] = split ? LC_WGRAD_SPLIT : LC_WGRAD_F32;
    out[1] = causes == 0;
    out[2] = nsplit;
    out[3] = split ? lc_wgrad_h_tiles(B, H, W) : lc_wgrad_tiles(B, H, W);
    out[4] = lc_planes_vec(B, (long long)H * W, dy_bs, dy_addr_mod16);
    out[5] = (int32_t)lc_wgrad_bias_offset(nsplit, Ci, Co, ks);
    out[6] = causes;
    out[7] = 0;
    return LC_OK;
}
