// Which attention kernel a call runs: ONE pure host function per pass, used by the launchers (attention.hip,
// attention_bwd.hip, attention_bwd_h.hip) and exported to the tests as lc_attention_route / lc_attention_bwd_route, so
// that the case table of tests/test_attention_matrix_host.py is proven against the launchers' own choice.
//
// Packed code: family << 16 | DQK << 8 | NDV << 4 | (waves == 8) << 1 | PRE
//   family 1  attn_kernel<DQK, NDV>                   fp32 MFMA forward
//          2  attn_h_kernel<DQK, NDV, waves, PRE>     f16x2-split forward (PRE: measured pre-scales, the training entry)
//          3  attn_bwd_{dq,dkv}_kernel<DQK, NDV>      fp32 MFMA backward
//          4  attn_bwd_{dq,dkv}_h_kernel<DQK, NDV>    f16x2-split backward
//   DQK = 32 or 64 (channels of q / k the kernel is instantiated for), NDV = 1 or 2 (32-channel blocks of v).
#pragma once

#include "../../include/lidarcrafter_hip.h"

constexpr int LC_ATTN_F32 = 1, LC_ATTN_SPLIT = 2, LC_ATTN_BWD_F32 = 3, LC_ATTN_BWD_SPLIT = 4;

constexpr int lc_attn_code(int family, int dqk_inst, int ndv, int waves, int pre) {
    return family << 16 | dqk_inst << 8 | ndv << 4 | (waves == 8 ? 2 : 0) | (pre ? 1 : 0);
}

// B * heads is the y extent of every attention grid
constexpr long long LC_ATTN_MAX_BH = 65535;

// split: the caller asked for the f16x2 arithmetic; has_amax: the training entry's measured maxima are present;
// waves_env: the LC_ATTN_WAVES value (0 = unset: 8 waves where d_v <= 32 and 256-query blocks still cover the chip).
// -> the packed code; LC_EINVAL / LC_EUNSUP exactly where the entries return them: a size that is not positive
// (dpos: negative) is invalid, a shape no kernel is instantiated for is unsupported.
inline int lc_attn_route_fwd(int split, int has_amax, int dqk, int dpos, int dv, long long bh, int Lq, int waves_env) {
    if (bh <= 0 || Lq <= 0 || dpos < 0) return LC_EINVAL;
    if (dqk <= 0 || dqk + dpos > 64 || dv <= 0 || dv > 64 || bh > LC_ATTN_MAX_BH) return LC_EUNSUP;
    const int dq = (dqk + dpos) <= 32 ? 32 : 64, nd = dv <= 32 ? 1 : 2;
    // a K unit of the split kernel = 8 channel rows of ONE operand, loaded without a per-channel guard: a content or a
    // positional part that does not fill its last unit goes to the fp32 kernel, which guards every channel
    if (!split || dqk % 8 || dpos % 8) return lc_attn_code(LC_ATTN_F32, dq, nd, 4, 0);
    if (has_amax) return lc_attn_code(LC_ATTN_SPLIT, dq, nd, 4, 1);
    // 256 queries per block (8 waves) where d_v <= 32 and the grid still covers the chip (measured: every such layer
    // of the layout model and the 512-key self-attention gain 6-14 %; a 300-token batch-2 case loses 12 %)
    const long long blocks8 = (long long)((Lq + 255) / 256) * bh;
    const bool w8 = nd == 1 && (waves_env == 8 || (waves_env == 0 && blocks8 >= 128));
    return lc_attn_code(LC_ATTN_SPLIT, dq, nd, w8 ? 8 : 4, 0);
}

inline int lc_attn_route_bwd(int split, int dqk, int dv, long long bh) {
    if (bh <= 0) return LC_EINVAL;
    if (dqk <= 0 || dqk > 64 || dv <= 0 || dv > 64 || bh > LC_ATTN_MAX_BH) return LC_EUNSUP;
    return lc_attn_code(split ? LC_ATTN_BWD_SPLIT : LC_ATTN_BWD_F32, dqk <= 32 ? 32 : 64, dv <= 32 ? 1 : 2, 4, 0);
}
