// Which way a call of the MeanFlow tangent kernels (flow_jvp.hip) runs: the pure functions its launchers and kernels switch
// on, in ONE place, and exported to the tests as lc_groupnorm_jvp_route / lc_qk_norm_cm_route / lc_attention_jvp_route, so
// that the case tables of tests/_flow_jvp_edges.py are proven against the library's own choice (the pattern of
// conv_bwd_route.h / gn_bwd_route.h).  No arithmetic lives here.
//
// lc_groupnorm_jvp_route
//   out[0] chunk        elements per statistics block (gn_chunk_elems: 4096 or 16384)
//   out[1] chunks       statistics blocks per (sample, group)
//   out[2] stats branch 1 every (sample, group) takes the float4 loop, 0 none does, 2 it differs by sample
//   out[3] causes       LC_GNJ_CAUSE_* seen on any (sample, group): why a row leaves the float4 loop (N4, XADDR), or
//                       stays in it with scalar loads of dx (DXADDR -> dvec == false)
//   out[4] dvec         of the rows in the float4 loop: 1 all load dx as float4, 0 none does, 2 it differs by sample
//   out[5] slabs        blocks per plane of the apply pass
//   out[6] cpb          channels per apply block
//   out[7] amax slots   blocks of the apply pass = lc_groupnorm_amax_partials(B, C, H, W, G, 0)
// lc_qk_norm_cm_route
//   out[0] DMAX         channels held in registers per token: 16, 32 or 64
//   out[1] blocks       256-token blocks per (sample, head)
//   out[2] partials     fp64 partials of dL/dg = lc_qk_norm_cm_bwd_partials(B, heads, L)
//   out[3] trips        trips of the reduce kernel's 256-lane strided loop over them
// lc_attention_jvp_route
//   out[0] D            padded head width: 32 or 64
//   out[1] rows         query rows per block: 64 (D = 32), 32 (D = 64)
//   out[2] qblocks      query blocks per (sample, head)
//   out[3] tiles        16-key tiles
//   out[4] last         keys in the last tile (1 .. 16)
//   out[5] last rows    query rows in the last block (1 .. rows)
//   out[6] q pad        channels of q / k padded inside the last lane that holds any (0 .. 7)
//   out[7] v pad        the same of v
#pragma once

#include "gn_apply_route.h"

// ---- GroupNorm JVP statistics ---------------------------------------------------------------------------------------------
constexpr int LC_GNJ_CAUSE_N4 = 1,          // n % 4: a group is no whole number of float4s
              LC_GNJ_CAUSE_XADDR = 2,       // a group of x does not start on 16 bytes
              LC_GNJ_CAUSE_DXADDR = 4;      // a group of dx does not start on 16 bytes (x does): scalar loads of dx only

// 0: the float4 loop; else the failing conditions
LC_ROUTE_HD inline int lc_gnj_scalar_causes(long long n, int x_addr_mod16) {
    return ((n & 3) != 0 ? LC_GNJ_CAUSE_N4 : 0) | ((x_addr_mod16 & 15) != 0 ? LC_GNJ_CAUSE_XADDR : 0);
}
LC_ROUTE_HD inline bool lc_gnj_dvec(int dx_addr_mod16) { return (dx_addr_mod16 & 15) == 0; }

// ---- q / k RMSNorm ----------------------------------------------------------------------------------------------------------
constexpr int LC_QKJ_TOKENS = 256;          // tokens per block (one per lane)

LC_ROUTE_HD inline int lc_qkj_dmax(int d) { return d <= 16 ? 16 : (d <= 32 ? 32 : 64); }
LC_ROUTE_HD inline int lc_qkj_blocks(int L) { return (L + LC_QKJ_TOKENS - 1) / LC_QKJ_TOKENS; }
inline long long lc_qkj_partials(int B, int heads, int L) { return (long long)lc_qkj_blocks(L) * B * heads; }

// ---- attention JVP ----------------------------------------------------------------------------------------------------------
constexpr int LC_ATTNJ_JK = 16;             // keys per LDS tile
constexpr int LC_ATTNJ_PC = 8;              // channels per lane

LC_ROUTE_HD constexpr int lc_attnj_width(int dqk, int dv_ch) { return (dqk <= 32 && dv_ch <= 32) ? 32 : 64; }
LC_ROUTE_HD constexpr int lc_attnj_rows(int D) { return 256 / (D / LC_ATTNJ_PC); }
LC_ROUTE_HD inline int lc_attnj_qblocks(int Lq, int D) { return (Lq + lc_attnj_rows(D) - 1) / lc_attnj_rows(D); }
LC_ROUTE_HD inline int lc_attnj_tiles(int Lk) { return (Lk + LC_ATTNJ_JK - 1) / LC_ATTNJ_JK; }
// keys of the tile that starts at key k0
LC_ROUTE_HD inline int lc_attnj_tile_keys(int Lk, int k0) { return Lk - k0 < LC_ATTNJ_JK ? Lk - k0 : LC_ATTNJ_JK; }

// ---- the queries --------------------------------------------------------------------------------------------------------------
// (chunk, chunks: gn_chunk_elems / gn_chunks of common.h are passed in by flow_jvp.hip, which includes both)
inline int lc_gnj_route(int B, int C, int H, int W, int G, long long x_bs, long long dx_bs, int x_addr_mod16,
                        int dx_addr_mod16, int chunk, int chunks, int32_t out[8]) {
    if (!out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || G <= 0 || C % G) return LC_EINVAL;
    if (B > 65535 || G > 65535) return LC_EUNSUP;
    const long long HW = (long long)H * W, n = (long long)(C / G) * HW;
    int rows = 0, vec = 0, dvec = 0, causes = 0;
    const int nb = B < 4 ? B : 4, ng = G < 4 ? G : 4;         // 4 (b bs + g n) mod 16 has period 4 in b and in g
    for (int b = 0; b < nb; ++b)
        for (int g = 0; g < ng; ++g) {
            const int xa = (x_addr_mod16 + 4 * (int)((b * x_bs + g * n) & 3)) & 15;
            const int da = (dx_addr_mod16 + 4 * (int)((b * dx_bs + g * n) & 3)) & 15;
            const int cz = lc_gnj_scalar_causes(n, xa);
            ++rows;
            causes |= cz;
            if (cz == 0) {
                ++vec;
                if (lc_gnj_dvec(da)) ++dvec;
                else causes |= LC_GNJ_CAUSE_DXADDR;
            }
        }
    int slabs, cpb;
    lc_gn_apply_grid(B, C, G, HW, &slabs, &cpb);
    out[0] = chunk;
    out[1] = chunks;
    out[2] = vec == rows ? 1 : (vec == 0 ? 0 : 2);
    out[3] = causes;
    out[4] = vec == 0 ? 0 : (dvec == vec ? 1 : (dvec == 0 ? 0 : 2));
    out[5] = slabs;
    out[6] = cpb;
    out[7] = (int32_t)lc_gn_apply_blocks(B, C, G, HW);
    return LC_OK;
}

inline int lc_qkj_route(int B, int heads, int d, int L, int32_t out[4]) {
    if (!out || B <= 0 || heads <= 0 || d <= 0 || L <= 0) return LC_EINVAL;
    if (d > 64 || (long long)B * heads > 65535) return LC_EUNSUP;
    const long long parts = lc_qkj_partials(B, heads, L);
    out[0] = lc_qkj_dmax(d);
    out[1] = lc_qkj_blocks(L);
    out[2] = (int32_t)parts;
    out[3] = (int32_t)((parts + 255) / 256);
    return LC_OK;
}

inline int lc_attnj_route(int BH, int Lq, int Lk, int dqk, int dv_ch, int32_t out[8]) {
    if (!out || BH <= 0 || Lq <= 0 || Lk <= 0 || dqk <= 0 || dv_ch <= 0) return LC_EINVAL;
    if (dqk > 64 || dv_ch > 64 || BH > 65535) return LC_EUNSUP;
    const int D = lc_attnj_width(dqk, dv_ch), rows = lc_attnj_rows(D);
    const int qblocks = lc_attnj_qblocks(Lq, D), tiles = lc_attnj_tiles(Lk);
    out[0] = D;
    out[1] = rows;
    out[2] = qblocks;
    out[3] = tiles;
    out[4] = lc_attnj_tile_keys(Lk, (tiles - 1) * LC_ATTNJ_JK);
    out[5] = Lq - (qblocks - 1) * rows;
    out[6] = (LC_ATTNJ_PC - dqk % LC_ATTNJ_PC) % LC_ATTNJ_PC;
    out[7] = (LC_ATTNJ_PC - dv_ch % LC_ATTNJ_PC) % LC_ATTNJ_PC;
    return LC_OK;
}
