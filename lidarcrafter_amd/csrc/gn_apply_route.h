// Launch shape of the GroupNorm apply passes: gn_apply_kernel (norm.hip) and gn_jvp_apply_kernel (flow_jvp.hip) run on the
// SAME grid, because both leave one partial maximum per block in buffers sized by lc_groupnorm_amax_partials.  One rule, in
// one place (the pattern of gn_bwd_route.h): a second copy that drifted would leave slots unwritten or write past the end.
#pragma once

#include "conv_bwd_route.h"

constexpr long long LC_GN_APPLY_SLAB = 4096;          // elements of a plane per apply block (at least)

// slabs of >= 4096 elements; small planes: several channels of a group per block, so the per-block fold of the partials
// (fp64 divide + sqrt) is paid once per >= 4096 elements while >= 512 blocks remain
inline void lc_gn_apply_grid(int B, int C, int G, long long HW, int* slabs, int* cpb) {
    int sl = (int)((HW + LC_GN_APPLY_SLAB - 1) / LC_GN_APPLY_SLAB);
    if (sl < 1) sl = 1;
    int c = 1;
    const int cpg = C / G;
    while (c * 2 <= cpg && cpg % (c * 2) == 0 && HW * c * 2 <= LC_GN_APPLY_SLAB && (long long)B * (C / (c * 2)) * sl >= 512)
        c *= 2;
    *slabs = sl; *cpb = c;
}

// blocks of the apply pass = partial maxima it writes
inline long long lc_gn_apply_blocks(int B, int C, int G, long long HW) {
    int slabs, cpb;
    lc_gn_apply_grid(B, C, G, HW, &slabs, &cpb);
    return (long long)slabs * (C / cpb) * B;
}
