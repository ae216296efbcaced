// How lc_groupnorm_bwd_train walks a plane: the pure functions its launcher and kernels (norm.hip) switch on, exported to
// the tests as lc_groupnorm_bwd_route (the pattern of attention_route.h / conv_bwd_route.h).
//
//   out[0] slabs        blocks per (sample, channel) plane of gn_bwd_apply_kernel = ceil(H W / 4096)
//   out[1] per          pixels per slab = ceil(H W / slabs)
//   out[2] apply branch 1 every plane takes the float4 loop, 0 none does, 2 it differs by sample
//   out[3] outer        outer iterations (4096 pixels each: fp32 over 16 values, then fp64) of gn_bwd_rows_kernel
#pragma once

#include "conv_bwd_route.h"

constexpr long long LC_GN_BWD_SLAB = 4096;            // pixels per apply block, and per outer step of the rows kernel

inline int lc_gn_bwd_slabs(long long HW) {
    const int slabs = (int)((HW + LC_GN_BWD_SLAB - 1) / LC_GN_BWD_SLAB);
    return slabs < 1 ? 1 : slabs;
}

LC_ROUTE_HD inline long long lc_gn_bwd_per(long long HW, int slabs) { return (HW + slabs - 1) / slabs; }

// float4 loads and stores of a slab: whole float4s, slabs that start on one, and the three planes on 16 bytes
LC_ROUTE_HD inline bool lc_gn_bwd_vec(long long HW, long long per, int x_addr_mod16, int dy_addr_mod16, int dx_addr_mod16) {
    return (HW & 3) == 0 && (per & 3) == 0 && ((x_addr_mod16 | dy_addr_mod16 | dx_addr_mod16) & 15) == 0;
}

inline int lc_gn_bwd_route(int B, int C, int H, int W, int G, long long x_bs, long long dy_bs, long long dx_bs,
                           int x_addr_mod16, int dy_addr_mod16, int dx_addr_mod16, int32_t out[4]) {
    if (!out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || G <= 0 || C % G) return LC_EINVAL;
    const long long HW = (long long)H * W;
    const int slabs = lc_gn_bwd_slabs(HW);
    const long long per = lc_gn_bwd_per(HW, slabs);
    int n = 0;
    const int nb = B < 4 ? B : 4;                     // 4 b bs mod 16 has period 4 in b
    for (int b = 0; b < nb; ++b)
        n += lc_gn_bwd_vec(HW, per, x_addr_mod16 + 4 * (int)((b * x_bs) & 3), dy_addr_mod16 + 4 * (int)((b * dy_bs) & 3),
                           dx_addr_mod16 + 4 * (int)((b * dx_bs) & 3));
    out[0] = slabs;
    out[1] = (int32_t)per;
    out[2] = n == nb ? 1 : (n == 0 ? 0 : 2);
    out[3] = (int32_t)((HW + LC_GN_BWD_SLAB - 1) / LC_GN_BWD_SLAB);
    return LC_OK;
}
