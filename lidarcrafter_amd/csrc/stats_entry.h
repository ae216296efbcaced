// THE GroupNorm statistics entry: its format, and every operation on it.
//
// A producing kernel (a conv epilogue, the split-K reduce, a resampler) leaves one entry
//     (pivot, n, S = sum(v - pivot), Q = sum((v - pivot)^2))                         -- four floats, one f32x4
// per sample, channel UNIT (8, 4, 2 or 1 consecutive channels: octets, quads, pairs, channels) and wave tile of what it
// stores, so that the GroupNorm behind it needs no statistics pass:
//     ostats[(b * (C / unit) + unit_index) * slots + slot],    slot = the producer's wave-tile index
//                                                              (conv: (tile_row * tiles_w + tile_col) * WPX + wave_px)
// `ush` = log2(unit) = 3, 2, 1 or 0 is the unit shift.  An unwritten slot of a zeroed buffer (n = 0) adds nothing.
//
// The pivot rule.  Every entry's pivot is the first value of the entry's OWN channels, bit for bit: lane 0's value for an
// entry of the whole wave; for the two entries a wave writes per half-wave (pairs in the deferred epilogues, quads in the
// pre-split and stride-2 kernels) lane 0's for lanes 0-31 and lane 32's for lanes 32-63, pairs taking a second pivot at
// the first value of channels q = 2, 3; the first active lane's for the one-channel producers.  With a pivot shared
// between units a unit whose level sits D away from it summed d ~ D in float32 and lost (D / std)^2 ulps of its variance
// (GroupNorm32 on channels at different levels: tests/test_gn_structured.py).  stat_pivot / StatAcc::start are the only
// pivot code.
//
// A consumer re-centres every entry of a group (contiguous: whole entries of ONE segment) on one common pivot P0 (the
// group's first entry's pivot, a typical value of the tensor):
//     S' = S + n d,  Q' = Q + d (2 S + n d),  d = pivot - P0
// and fp64 sums of N, S', Q' give mean = P0 + S'/N, var = Q'/N - (S'/N)^2: no division per entry, no cancellation beyond
// |mean - P0| / std (a few), fixed summation order (deterministic).
#pragma once
#include "common.h"

// ---- producer side -----------------------------------------------------------------------------------------------------

// 64-lane sum with DPP adds (VALU rate, no LDS): row_shr 1,2,4,8, then row_bcast:15 into rows 1,3
// and row_bcast:31 into rows 2,3 -- lane 63 ends up with the total.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                                                     CTRL, ROW_MASK, 0xF, true));
}
// the sum without its last step: lanes 31 / 63 hold the sums of lanes 0-31 / 32-63
__device__ __forceinline__ float half_sum_to_lane31_63(float v) {
    v = dpp_add<0x111, 0xF>(v);
    v = dpp_add<0x112, 0xF>(v);
    v = dpp_add<0x114, 0xF>(v);
    v = dpp_add<0x118, 0xF>(v);
    v = dpp_add<0x142, 0xA>(v);
    return v;
}
__device__ __forceinline__ float wave_sum_to_lane63(float v) { return dpp_add<0x143, 0xC>(half_sum_to_lane31_63(v)); }

// Which lanes share a pivot: the wave (lane 0's value); each half-wave (lane 0's / lane 32's; bit arithmetic, no select:
// fit for a deferred epilogue); each half-wave only where the kernel learns it at run time (both lanes' values are kept,
// wave-uniform, and start's upper_half = "the entries are per half-wave and this lane is one of 32-63" picks one at each
// use); or the wave around its first active lane's value (the one-channel producers).
enum StatPivot { PIVOT_WAVE, PIVOT_HALF, PIVOT_HALF_RT, PIVOT_FIRST };

// THE pivot code: the pivot of an entry whose first value is `first` in the lane(s) named above
template <StatPivot PV>
__device__ __forceinline__ float stat_pivot(float first) {
    static_assert(PV != PIVOT_HALF_RT, "kept as two wave-uniform values: StatAcc");
    if constexpr (PV == PIVOT_FIRST) return lc_readfirstlane_f32(first);
    const float lo = lc_readlane_f32(first, 0);
    if constexpr (PV == PIVOT_WAVE) return lo;
    else return lc_half_select(lo, lc_readlane_f32(first, 32));
}

// The running sums of one entry: pivot, sum (v - p), sum (v - p)^2.  p is wave-uniform or, for PIVOT_HALF, per lane.
template <StatPivot PV>
struct StatAcc {
    float p, s, q;
    float ph; bool upper;      // PIVOT_HALF_RT only: lane 32's value, and whether this lane takes it
    __device__ __forceinline__ void start(float first, bool upper_half = false) {
        if constexpr (PV == PIVOT_HALF_RT) {
            p = lc_readlane_f32(first, 0); ph = lc_readlane_f32(first, 32); upper = upper_half;
        } else {
            p = stat_pivot<PV>(first);
        }
        s = 0.f; q = 0.f;
    }
    __device__ __forceinline__ float pivot() const {
        if constexpr (PV == PIVOT_HALF_RT) return upper ? ph : p;
        else return p;
    }
    __device__ __forceinline__ void add(float v, bool ok = true) {
        const float d = ok ? v - pivot() : 0.0f;
        s += d;
        q = fmaf(d, d, q);
    }
    // two values whose deviations are added to each other first (the resamplers' order of operations)
    __device__ __forceinline__ void add2(float v0, float v1) {
        const float d0 = v0 - pivot(), d1 = v1 - pivot();
        s += d0 + d1;
        q = fmaf(d0, d0, q);
        q = fmaf(d1, d1, q);
    }
};

// One entry (pivot, n, s, q) as ONE 32-bit buffer store: the sums sit in the reducing lane R (63, or 31 and 63 for two
// half-wave entries), pivot and count are uniform over the lanes that store; lanes R-3 .. R carry the fields 0 .. 3 (their
// voffset = entry byte offset + 4 * (lane & 3); every other lane: an out-of-range offset).  One store instruction per
// entry, no wide store data, no waits.
// Rounds 1-3 wrote the entry as one 128-bit buffer store with an SGPR soffset; ~3 entries in 10^7 then arrived with a
// foreign upper dword (a VALU write of the data registers one or two instructions behind the store: LLVM exempts MUBUF
// stores with an SGPR soffset from the ISA's ">64-bit store data" wait state, and under ~27 stores in flight per wave that
// exemption does not hold on gfx950).  Measured in round 4 (devtools/entry_stress.py, profiles/r04_entry_store.txt):
// 128-bit + SGPR soffset 17 bad entries in 5e7, 32-bit stores 0 in 1e8.  32-bit stores fetch their data at issue -- the
// form every output value of the deferred epilogue has always used.  (First form of round 4: four 32-bit stores from lane
// R with four different cache-policy bits to keep the load/store optimizer from re-merging them -- the sc0 sc1 one cost
// the level-0 launch ~100 us.  Round 5, pre-split kernel: four volatile 32-bit stores from that lane compiled to sc0 sc1
// stores with a vmcnt(0) behind each, i.e. every entry waited for all of the tile's output stores: +6 ... +11 us per
// launch, profiles/r05_level0.txt section 7.)
__device__ __forceinline__ void store_entry_4lanes(__amdgpu_buffer_rsrc_t rs, float p_, float n_, float s_, float q_,
                                                   unsigned voffset, unsigned soffset = 0) {
    // row_shl:1 -- lane R-1 reads lane R's sum
    const float s1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s_), 0x101, 0xF, 0xF, true));
    // field select by lane & 3 with masks, not selects: hipcc turned the nested ?: (one arm is a DPP result) into
    // exec-mask BRANCHES -- four basic-block splits per tile inside the MFMA stream (ISA of rounds 3-4)
    const int f = (int)(threadIdx.x & 3);
    const unsigned k0 = (unsigned)((f - 1) >> 31), k1 = (unsigned)(((f ^ 1) - 1) >> 31);
    const unsigned k2 = (unsigned)(((f ^ 2) - 1) >> 31), k3 = (unsigned)(((f ^ 3) - 1) >> 31);
    const unsigned vu = (__float_as_uint(p_) & k0) | (__float_as_uint(n_) & k1) | (__float_as_uint(s1) & k2) |
                        (__float_as_uint(q_) & k3);
    __builtin_amdgcn_raw_buffer_store_b32(vu, rs, voffset, soffset, 0);
}

// The entry (or, `quads`, the two entries) of channel octet co_oct of one wave tile, from an accumulator every lane ran over
// its pixels of the octet.  Octet entry: lane 63 holds the sums.  Quad entries (a consumer GroupNorm with 4 / 12 channels
// per group): lanes 0-31 hold channels 8m .. 8m+3, lanes 32-63 8m+4 .. 8m+7 -- the two half-wave sums in lanes 31 / 63,
// each around a pivot of its own quad (the accumulator was started with upper_half = quads && lane >= 32).  `rs` covers
// the sample's entries, nvalid = valid pixels per half-wave, ok = the octet (and the tile) exists.
__device__ __forceinline__ void emit_octet_or_quads(__amdgpu_buffer_rsrc_t rs, const StatAcc<PIVOT_HALF_RT>& a, bool quads,
                                                    int nvalid, int co_oct, bool ok, int oslots, int slot) {
    const int lane = threadIdx.x & 63;
    const bool mine = quads ? (lane & 31) >= 28 : lane >= 60;
    const float nv = (float)((quads ? 4 : 8) * nvalid);
    const float sh = half_sum_to_lane31_63(a.s), qh = half_sum_to_lane31_63(a.q);
    const float sf = dpp_add<0x143, 0xC>(sh), qf = dpp_add<0x143, 0xC>(qh);   // lane 63: the wave's sum
    const int ent = quads ? (co_oct >> 2) + (lane >> 5) : (co_oct >> 3);
    const unsigned vo = (mine && ok) ? ((unsigned)ent * (unsigned)oslots + (unsigned)slot) * 16u + 4u * (lane & 3)
                                     : 0x80000000u;
    store_entry_4lanes(rs, a.pivot(), nv, quads ? sh : sf, quads ? qh : qf, vo);
}

// ---- consumer side -----------------------------------------------------------------------------------------------------

// The entries a GroupNorm reads: segment 0 covers channels [0, seg[0].channels), segment 1 the rest (a concatenated
// input has two producers); ush: log2(channels per entry) of the segment.
struct StatSegs {
    struct Seg { const f32x4* p; int channels, slots, ush; } seg[2];
};
constexpr StatSegs STAT_SEGS_NONE = {{{nullptr, 0, 0, 3}, {nullptr, 0, 0, 3}}};

// lc_oct_stats s0 (, s1) -> StatSegs for a GroupNorm of C channels, cpg per group (C % cpg == 0): every group must be
// whole entries of ONE segment.  A unit this library does not write returns rc_unknown_unit (the launchers differ there).
static inline int stat_segs_from(const lc_oct_stats* s0, const lc_oct_stats* s1, int C, int cpg, int rc_unknown_unit,
                                 StatSegs& out) {
    out = STAT_SEGS_NONE;
    const lc_oct_stats* in[2] = {s0, s1};
    if (!s0) return LC_EINVAL;
    for (int i = 0; i < 2; ++i)
        if (in[i] && (!in[i]->p || in[i]->channels <= 0 || in[i]->slots <= 0)) return LC_EINVAL;
    int total = 0;
    for (int i = 0; i < 2 && in[i]; ++i) {
        const int u = in[i]->unit;
        const int ush = u == 8 ? 3 : (u == 4 ? 2 : (u == 2 ? 1 : (u == 1 ? 0 : -1)));
        if (ush < 0) return rc_unknown_unit;
        out.seg[i] = StatSegs::Seg{reinterpret_cast<const f32x4*>(in[i]->p), in[i]->channels, in[i]->slots, ush};
        total += in[i]->channels;
    }
    if (total != C || s0->channels % cpg || cpg % s0->unit || (s1 && cpg % s1->unit)) return LC_EUNSUP;
    return LC_OK;
}

// the entries of the group whose first channel is cg0, sample b
struct StatGroup { const f32x4* e; int n_ent; };
__device__ __forceinline__ StatGroup stat_group(const StatSegs& ss, int b, int cg0, int cpg) {
    const bool s1 = cg0 >= ss.seg[0].channels;
    const int slots = s1 ? ss.seg[1].slots : ss.seg[0].slots;
    const int ush = s1 ? ss.seg[1].ush : ss.seg[0].ush;
    const f32x4* e =
        s1 ? ss.seg[1].p + ((long long)b * (ss.seg[1].channels >> ush) + ((cg0 - ss.seg[0].channels) >> ush)) * slots
           : ss.seg[0].p + ((long long)b * (ss.seg[0].channels >> ush) + (cg0 >> ush)) * slots;
    return StatGroup{e, (cpg >> ush) * slots};
}

// K entries base, base + STRIDE, ... of a group in flight (load half), and their fold around P0 (fold half): a kernel may
// put independent loads between the two.  An absent entry (past the group, or n = 0) adds nothing.
template <int STRIDE, int K>
__device__ __forceinline__ void load_entries(f32x4 (&v)[K], const f32x4* e, int n_ent, int base) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = base + STRIDE * k < n_ent ? e[base + STRIDE * k] : f32x4{0.f, 0.f, 0.f, 0.f};
}
template <int K>
__device__ __forceinline__ void fold_loaded(const f32x4 (&v)[K], double P0, double& N, double& S, double& Q) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double n = v[k].y, d = (double)v[k].x - P0, s_ = v[k].z;
        N += n;
        S += s_ + n * d;
        Q += (double)v[k].w + d * (2.0 * s_ + n * d);
    }
}
// this thread's share of the group: entries first, first + STRIDE, ..., K loads in flight
template <int STRIDE, int K>
__device__ __forceinline__ void fold_entries(const f32x4* e, int n_ent, int first, double P0, double& N, double& S,
                                             double& Q) {
    for (int base = first; base < n_ent; base += STRIDE * K) {
        f32x4 v[K];
        load_entries<STRIDE, K>(v, e, n_ent, base);
        fold_loaded(v, P0, N, S, Q);
    }
}

// every lane gets the wave's sums (xor butterfly)
__device__ __forceinline__ void stat_wave_sum(double& N, double& S, double& Q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        N += __shfl_xor(N, o, 64); S += __shfl_xor(S, o, 64); Q += __shfl_xor(Q, o, 64);
    }
}
// every thread of a 256-thread block gets the block's sums; sh: 12 doubles of LDS, used once per kernel
__device__ __forceinline__ void stat_block_sum(double* sh, double& N, double& S, double& Q) {
    stat_wave_sum(N, S, Q);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[3 * wv] = N; sh[3 * wv + 1] = S; sh[3 * wv + 2] = Q; }
    __syncthreads();
    N = (sh[0] + sh[3]) + (sh[6] + sh[9]);
    S = (sh[1] + sh[4]) + (sh[7] + sh[10]);
    Q = (sh[2] + sh[5]) + (sh[8] + sh[11]);
}
// (mean, rstd) of the group from its folded sums; an empty group (N = 0) has mean P0 and variance 0
__device__ __forceinline__ float2 stat_finish(double N, double S, double Q, double P0, float eps) {
    const double m = N > 0.0 ? S / N : 0.0;
    double var = N > 0.0 ? Q / N - m * m : 0.0;
    if (var < 0.0) var = 0.0;
    return float2{(float)(P0 + m), (float)(1.0 / sqrt(var + (double)eps))};
}
