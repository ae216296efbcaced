/*
 * lidarcrafter_hip.h -- C ABI of the MI355X (gfx950) hot path of LiDARCrafter's range-image
 * diffusion denoiser.  Built as lidarcrafter_amd/liblidarcrafter_hip.so by hipcc.
 *
 * Conventions (all entry points):
 *   - extern "C", return int: 0 = ok, >0 = hipError_t of the launch, <0 = LC_E* argument error.
 *   - raw DEVICE pointers + sizes + a hipStream_t passed as void* (NULL = default stream).
 *   - no allocation, no synchronisation, no host<->device copies inside: every call is legal
 *     under hipStreamBeginCapture (HIP graphs).
 *   - tensors are fp32, [B, C, H, W] with the inner [C, H, W] block contiguous; `*_bs` is the
 *     batch stride in ELEMENTS (>= C*H*W).  A channel slice of a wider buffer is therefore a
 *     valid tensor, which is how torch.cat([h, skip], 1) of the reference
 *     (efficient_unet.py:293-295, layout_unet_v1.py:893) is made free: producers write into
 *     slices of one pre-concatenated buffer.
 *
 * Each function cites the reference code it replaces (paths relative to /root/reference/).
 * The reference reaches these through ATen ops of its nn.Modules, not through an FFI of its
 * own; INTEGRATION.md shows the binding a maintainer of the reference would add.
 */
#ifndef LIDARCRAFTER_HIP_H
#define LIDARCRAFTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_OK 0
#define LC_EINVAL (-1)  /* bad size / null pointer */
#define LC_EUNSUP (-2)  /* shape outside what the kernels are instantiated for */

typedef void* lc_stream_t;

/* Library / device probe.  Returns the ABI version (this header = 6: lc_sparse_quantize takes its voxel sizes as doubles;
 * 5: the up-path fold's entry points, lc_up2_combine9_fwd / lc_split_act_fwd; 4: the
 * unit-form attention; 3: round 6 -- lc_conv2d_ring_f16x2_ps_fwd carries
 * gn_ostats_unit, the stride-2 / calibration entry points exist; 2: round 3 -- field-of-view arguments are doubles,
 * lc_layout_condition takes float32 or float64 boxes, float64 point sets).  Bumped whenever an exported signature
 * changes; lidarcrafter_amd/_lib.py refuses a library of another version. */
int lc_abi_version(void);
/* Writes gcnArchName of the current device into buf (NUL terminated). */
int lc_device_arch(char* buf, int buflen);
/* Loads the code objects of every translation unit of the library for the CURRENT device now (HIP defers that to a
 * unit's first kernel launch, i.e. into the first sampling step of a process).  Idempotent, no device work.
 * Returns LC_OK or -- like every launcher of this header when the HIP runtime refuses a launch -- the POSITIVE hipError_t
 * of the failing runtime call (LC_E* codes are negative); callers treat it as a warm-up that did not happen. */
int lc_load_code_objects(void);

/* ---------------------------------------------------------------------------------------------
 * Convolution: lidargen/models/unets/ops.py:149-173 (ops.Conv2d) with ops.py:32-49 (Pad,
 * ring=True: W circular, H zeros) for 3x3, and plain 1x1 (ring=False, padding 0).
 * Used by every conv of EfficientUNet (efficient_unet.py:79,89,94,141,179,260,271) and
 * LayoutUnetV1 (nn.py:34-44 conv_nd_range; Conv1d 1x1 projections layout_unet_v1.py:386-399).
 *
 * Weights are consumed in a PACKED layout wp[tap][Cip][Cop] (tap = ky*ks+kx, Cip = Ci rounded
 * up to 8, Cop = Co rounded up to 64, zero filled) produced once per weight version by
 * lc_pack_conv_weight from the checkpoint layout OIHW [Co][Ci][ks][ks].
 * Arithmetic: fp32 inputs, fp32 MFMA (v_mfma_f32_32x32x2_f32) accumulate == an fmaf chain.
 *   y = (conv(x) + bias [+ res]) * out_scale          (ResidualBlock efficient_unet.py:111-115)
 * ------------------------------------------------------------------------------------------- */
int64_t lc_packed_conv_weight_elems(int Co, int Ci, int ks);
int lc_pack_conv_weight(const float* w_oihw, float* wp, int Co, int Ci, int ks, lc_stream_t s);
int lc_conv2d_ring_fwd(const float* x, int64_t x_bs, const float* wp, const float* bias,
                       const float* res, int64_t res_bs, float* y, int64_t y_bs,
                       int B, int Ci, int Co, int H, int W, int ks, float out_scale,
                       int tile_cfg /* 0 = auto */, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Same convolution on the f16 matrix cores with fp32-class accuracy ("f16x2 split"): operands are
 * split into hi+lo fp16 halves (activations on the fly, weights at pack time) and
 * xh*wh + xh*wl + xl*wh is accumulated in fp32 by three v_mfma_f32_32x32x16_f16 per block --
 * ~5e-7 relative error per product, 5.3x the fp32 matrix peak.  Packed weights: two planes
 * (hi, lo) of lc_packed_conv_weight_f16x2_elems() fp16 values each, layout [tap][Ci^16/8][Co^64][8].
 * Arguments otherwise identical to lc_conv2d_ring_fwd.
 * ------------------------------------------------------------------------------------------- */
int64_t lc_packed_conv_weight_f16x2_elems(int Co, int Ci, int ks);
/* wmeta: 4 device floats written here, read by lc_conv2d_ring_f16x2_fwd:
 *   {w_scale, 1 / w_scale, max |w|, 0}.  w_scale is the power of two the weights are multiplied by
 * before the hi/lo split: 256 while max|w| * 256 lies in [2^5, 2^15] (every trained layer seen so
 * far), otherwise the power of two that puts max|w| * w_scale into [2^12, 2^13) -- so weights of
 * any magnitude (1e-30 ... 1e30) keep 22 significant bits and none saturates fp16.  The scale is
 * derived on the device (no host synchronisation): an all-zero / non-finite tensor keeps 256. */
int lc_pack_conv_weight_f16x2(const float* w_oihw, void* wp_hi, void* wp_lo, int Co, int Ci, int ks,
                              float* wmeta, lc_stream_t s);
/* The packed weight of a layer's INPUT-GRADIENT conv (dX = the same ring conv of dY with the transposed, 180-degree
 * rotated kernel) straight from the layer's forward weight w_fwd [Cf_o][Cf_i][ks][ks] -- the rotation and transposition
 * happen in the pack kernel's addressing, no rotated copy exists.  Co / Ci are those of the dX conv (Co = Cf_i,
 * Ci = Cf_o).  wmeta_fwd (may be NULL) = the wmeta lc_pack_conv_weight_f16x2 wrote for the SAME version of w_fwd: its
 * max|w| is reused (one launch instead of memset + reduction + pack).  Training packs every weight twice per step
 * (lidarcrafter_amd/autograd.py ConvRing.backward). */
int lc_pack_conv_weight_f16x2_dx(const float* w_fwd, void* wp_hi, void* wp_lo, int Co, int Ci, int ks,
                                 float* wmeta, const float* wmeta_fwd, lc_stream_t s);
/* All conv weights of a model at once (training: every weight changes at every optimizer step -- two packs per layer
 * and step): `jobs` is a DEVICE array of n records; each names a forward weight w [Co][Ci][ks][ks] (contiguous), the
 * buffers of its own pack (as lc_pack_conv_weight_f16x2: planes of lc_packed_conv_weight_f16x2_elems(Co, Ci, ks)
 * halves, fwd_meta 4 floats) and, when with_dx != 0, of its input-gradient pack (as lc_pack_conv_weight_f16x2_dx:
 * planes of lc_packed_conv_weight_f16x2_elems(Ci, Co, ks) halves, dx_meta 4 floats).  Three launches in total, same
 * bytes as the per-layer functions. */
typedef struct lc_weight_pack_job {
    const float* w;
    void *fwd_hi, *fwd_lo;
    float* fwd_meta;
    void *dx_hi, *dx_lo;
    float* dx_meta;
    int Co, Ci, ks, reserved;
} lc_weight_pack_job;
int lc_pack_conv_weights_f16x2_multi(const lc_weight_pack_job* jobs, int n, int with_dx, lc_stream_t s);
/* Range state of ONE conv layer's input (device memory, 16 bytes, owned by the caller, initialise
 * with {16, 1/16, 0, 0}).  The kernel multiplies x by x_scale before the fp16 hi/lo split and
 * publishes the largest |x * x_scale| it staged (after the fused input GroupNorm, if any) into
 * amax_scaled with atomicMax -- fp16 saturates at 65504, so the caller must treat a launch whose
 * amax_scaled reached 2^15 as INVALID: pick x_scale = a power of two with max|x| * x_scale ~ 2^12,
 * reset amax_scaled and run the layer (and everything downstream) again.  lidarcrafter_amd.ops
 * does exactly that after every forward / sampling run (`range_poll`); nothing saturated is ever
 * returned silently.  amax_scaled accumulates over launches until the caller zeroes it. */
typedef struct lc_conv_range {
    float x_scale, x_unscale, amax_scaled, reserved;
} lc_conv_range;
/* The record of a tensor measured on the device: max |x| over B samples of n floats (sample stride
 * x_bs) -> x_scale = the power of two with max|x| * x_scale in [2^12, 2^13), amax_scaled = 0.  Two
 * tiny launches, no host synchronisation; `reserved` is the reduction's scratch word (0 between
 * calls).  Training uses it right before every f16x2 conv (activations in the forward, gradients in
 * the backward: lidarcrafter_amd/autograd.py), where a poll-and-repeat protocol is not available. */
int lc_range_from_tensor(const float* x, int64_t x_bs, int B, int64_t n, lc_conv_range* range,
                         lc_stream_t s);
/* The same record from the partial maxima the PRODUCER of x left while writing it (amax: n device floats whose maximum is
 * max|x| -- lc_groupnorm_apply_train / lc_groupnorm_bwd_train store one per block, no atomics) -- one single-block launch,
 * x is not read again.  bound_mult >= 1 (LC_EINVAL otherwise): the tensor the conv will read is an elementwise rescale of
 * the measured one by at most this factor (dropout: 1 / (1 - p)); max|x| * bound_mult is then an upper bound, which is
 * all the record needs. */
int lc_range_from_amax(const float* amax, int64_t n, float bound_mult, lc_conv_range* range, lc_stream_t s);
/* Producer-side GroupNorm statistics of one channel segment: the entries a conv wrote through
 * gn_ostats_out (below), consumed by lc_groupnorm_apply_os or by the next conv's fused input norm. */
typedef struct lc_oct_stats {
    const float* p;     /* [B, channels/unit, slots, 4] */
    int channels, slots;
    int unit;           /* channels per entry: 8 (octets: the conv epilogues), 2 (pairs: lc_conv2d_ring_f16x2_fwd with
                           gn_ostats_unit = 2, for a GroupNorm with 2 / 4 / 6 channels per group), 1 (single
                           channels: lc_resample2x_stats_fwd), 4.  Every consumer -- the conv's fused input norm,
                           lc_groupnorm_apply_os, lc_groupnorm_apply_os_split -- folds any of them as long as a
                           group is a whole number of entries (round 5; before: octets only in the apply passes) */
} lc_oct_stats;
/* Input normalisation straight from the statistics (no lc_groupnorm_coeffs launch): the partials
 * of lc_groupnorm_stats over the conv's input plus the GroupNorm / AdaGN parameters; every block
 * derives the rows of its sample in its prologue with the arithmetic of lc_groupnorm_coeffs.
 * Alternatively (partials == NULL, os0 != NULL) from the octet statistics the input's producer(s)
 * emitted -- then no statistics pass over the input exists at all; os0 covers channels
 * [0, os0->channels), os1 (may be NULL) the rest, as in lc_groupnorm_apply_os; needs
 * (Ci/G) % 8 == 0, every group inside one segment and G <= 128 (LC_EUNSUP otherwise). */
typedef struct lc_gn_stats_input {
    const double* partials;   /* lc_groupnorm_stats(x, ...) of THIS conv's input, or NULL */
    int G, nch;               /* groups; chunks per group = partials_elems / (2 * B * G) */
    float eps;
    const float *gamma, *beta, *scale, *shift;   /* each may be NULL, as in lc_groupnorm_apply */
    int64_t ss_bs;
    const lc_oct_stats *os0, *os1;               /* used when partials == NULL */
} lc_gn_stats_input;

/* Layout constraints of the pipelined tile configurations (12-28, 33; the configurations the heuristic picks for every
 * 3x3 conv with Ci >= 24): they fetch both weight planes by LDS-DMA through ONE buffer descriptor, so wp_lo must lie
 * ABOVE wp_hi at a distance below 2 GiB -- in practice one allocation holding both planes, which is what
 * lc_pack_conv_weight_f16x2's callers in lidarcrafter_amd.ops make (LC_EINVAL otherwise); and a sample of the input,
 * of the output and of the residual is addressed with 32-bit byte offsets: Ci*H*W*4, Co*H*W*4 < 2^31 (LC_EUNSUP).
 * tile_cfg 33 = the ping-pong kernel (csrc/conv_f16x2_pp.h): 3x3, Ci % 16 == 0, 64 <= Ci <= 512, Co % 64 == 0,
 * H % 4 == 0, W % 64 == 0 (LC_EUNSUP otherwise); the heuristic (tile_cfg 0) picks it only with LC_PP_MIN_STRIPS set.
 * tile_cfg 27 (round 5) = the tall kernel (csrc/conv_f16x2_tall.hip: halo rows kept in LDS across the block's walk down H,
 * 64-bit input loads): 3x3, Ci 32 or 64, H % 4 == 0, W % 64 == 0; any other shape given this id runs on the pipelined
 * 64 co x (4 x 64 px) tile (23), whose statistics partition it shares.  The heuristic picks 27 wherever it would pick 23 and
 * the shape qualifies (LC_TALL=0: never). */
int lc_conv2d_ring_f16x2_fwd(const float* x, int64_t x_bs, const void* wp_hi, const void* wp_lo,
                             const float* bias, const float* res, int64_t res_bs, float* y,
                             int64_t y_bs, int B, int Ci, int Co, int H, int W, int ks,
                             float out_scale, int tile_cfg /* 0 = auto */,
                             const float* gn_coeffs /* NULL or [B, gn_cpad, 4] */, int gn_cpad,
                             int gn_silu, const lc_gn_stats_input* gn_stats /* NULL, or instead of
                             gn_coeffs */,
                             float* gn_ostats_out /* NULL or [B, Co/unit, slots, 4], see below */,
                             int gn_ostats_unit /* 8 (octet entries) or 2 (pair entries, lc_oct_stats) */,
                             const float* wmeta /* from lc_pack_conv_weight_f16x2 */,
                             lc_conv_range* range /* this layer's input range state */,
                             lc_stream_t s);
/* Output statistics for the NEXT GroupNorm (every GroupNorm input of the denoiser is a conv
 * output, efficient_unet.py:101-108): with gn_ostats_out != NULL every wave of the pipelined kernel
 * also writes, per octet of 8 consecutive output channels and wave tile, the entry
 * (pivot, n, sum(y - pivot), sum((y - pivot)^2)) of the values it stored; lc_groupnorm_apply_os
 * folds them, so no statistics pass re-reads the tensor.  slots = entries per (sample, octet) for
 * this problem and tile configuration, 0 when the chosen kernel emits none (Co % 8 != 0, or the
 * 2-blocks/CU kernel): ask before allocating. */
int64_t lc_conv2d_ring_f16x2_stats_slots(int B, int Ci, int Co, int H, int W, int ks, int tile_cfg);
/* PRE-SPLIT activations.  The f16x2 kernels need every conv input as fp16 hi + lo halves; instead of
 * splitting the fp32 tile inside the conv's K loop (once per 64-output-channel block), the PRODUCER
 * of the tensor -- the GroupNorm apply pass in front of almost every conv of the denoisers
 * (efficient_unet.py:101-108, layout_unet_v1.py:171-175) -- can write the split form directly:
 *   y_split: 16-byte units (8 fp16 channels of one pixel), [B][plane = hi, lo][C/8][H][W]
 *            = lc_split_act_units(B, C, H, W) units, the same bytes as fp32 NCHW (needs C % 16 == 0;
 *            lc_groupnorm_apply_os_split also needs groups of whole octets -- LC_EUNSUP otherwise,
 *            use lc_groupnorm_apply_split or the fp32 forms then),
 * already multiplied by the CONSUMER layer's x_scale (`range`, whose amax_scaled it maintains: the
 * range-safety contract of lc_conv_range moves to the producer).  lc_conv2d_ring_f16x2_ps_fwd then
 * stages its tiles with LDS-DMA (`buffer_load_dwordx4 ... lds`): no VGPRs, no VALU, no ds_write in
 * the K loop.  3x3 ring convolution, pipelined tile shapes (tile_cfg 0 = auto, 12/13/15/22/23/25/28);
 * wp_lo must be wp_hi + one plane (ONE allocation holding both planes of
 * lc_pack_conv_weight_f16x2).  Everything else as lc_conv2d_ring_f16x2_fwd. */
int64_t lc_split_act_units(int B, int C, int H, int W);
int lc_groupnorm_apply_split(const float* x, int64_t x_bs, const double* partials, const float* gamma,
                             const float* beta, const float* scale, const float* shift, int64_t ss_bs,
                             void* y_split, int B, int C, int H, int W, int G, float eps, int act_silu,
                             lc_conv_range* range, lc_stream_t s);
int lc_groupnorm_apply_os_split(const float* x, int64_t x_bs, const lc_oct_stats* s0,
                                const lc_oct_stats* s1, const float* gamma, const float* beta,
                                const float* scale, const float* shift, int64_t ss_bs, void* y_split,
                                int B, int C, int H, int W, int G, float eps, int act_silu,
                                lc_conv_range* range, lc_stream_t s);
int lc_conv2d_ring_f16x2_ps_fwd(const void* x_split, const void* wp_hi, const void* wp_lo,
                                const float* bias, const float* res, int64_t res_bs, float* y,
                                int64_t y_bs, int B, int Ci, int Co, int H, int W, float out_scale,
                                int tile_cfg, float* gn_ostats_out /* NULL, or [B, Co / unit, slots, 4] */,
                                int gn_ostats_unit /* 8 = octet entries, 4 = quad entries (else LC_EUNSUP) */,
                                float* splitk_part /* NULL, or [ksplit, B, Co, H, W] */, int ksplit,
                                const float* wmeta, lc_conv_range* range, lc_stream_t s);
/* 1x1 convolution of a pre-split activation (the same planes; H * W is one pixel axis): LDS-DMA staging, 128 output
 * channels x 256 pixels per block -- for projections with many output channels, where the fp32-input kernel splits the
 * same input tile once per 64-channel block (qkv projections of the layout model).  Needs Ci % 32 == 0 (LC_EUNSUP
 * otherwise); weights: the ks = 1 pack, lo plane directly behind the hi plane; no statistics output, no split-K. */
int lc_conv1x1_f16x2_ps_fwd(const void* x_split, const void* wp_hi, const void* wp_lo, const float* bias,
                            const float* res, int64_t res_bs, float* y, int64_t y_bs, int B, int Ci, int Co,
                            int H, int W, float out_scale, const float* wmeta, lc_conv_range* range,
                            lc_stream_t s);
/* SPLIT-K for small grids (batch 1-2 at the deep levels: 16-64 blocks on 256 CUs): with splitk_part
 * != NULL the conv launches ksplit (2 ... Ci/16) blocks per tile, each over a contiguous range of
 * the K chunks, and stores raw partial sums only (bias / res / out_scale / statistics are ignored);
 * lc_splitk_reduce sums the planes in index order (deterministic) and applies the epilogue, with
 * optional GroupNorm statistics of the result in the conv epilogue's entry format
 * (lc_splitk_stats_slots(H, W) entries per (sample, octet)). */
int64_t lc_splitk_stats_slots(int H, int W);
int lc_splitk_reduce(const float* part, int ksplit, const float* bias, const float* res,
                     int64_t res_bs, float* y, int64_t y_bs, int B, int Co, int H, int W,
                     float out_scale, float* gn_ostats_out, lc_stream_t s);

/* Fused input normalisation: with gn_coeffs != NULL the kernel applies
 *   x <- silu?( (x - mu) * A + Bc )       rows (mu, A, Bc, 0) from lc_groupnorm_coeffs
 * while staging the input tile (the GN -> SiLU -> Conv chain of efficient_unet.py:101-108 and
 * layout_unet_v1.py:171-175 becomes stats + conv; the normalised tensor never reaches HBM).
 * gn_cpad = channels per sample in the table, >= Ci rounded up to 16. */
int lc_groupnorm_coeffs(const float* x, int64_t x_bs, const double* partials, const float* gamma,
                        const float* beta, const float* scale, const float* shift, int64_t ss_bs,
                        float* coeffs, int B, int C, int Cpad, int H, int W, int G, float eps,
                        lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * GroupNorm (+ affine | + AdaGN scale/shift) (+ SiLU):
 *   nn.GroupNorm(8, C, 1e-6) efficient_unet.py:37,77; ops.AdaGN ops.py:176-200;
 *   GroupNorm32 nn.py:17-19 + scale-shift norm layout_unet_v1.py:243-245; nn.SiLU.
 * Two launches: lc_groupnorm_stats writes per-(b,g,chunk) fp64 partial (sum, sumsq) into
 * `partials` (>= lc_groupnorm_partials_elems doubles); lc_groupnorm_apply folds them in a fixed
 * order (deterministic), then
 *   y = ((x-mean)*rstd * gamma[c] + beta[c]) * (1 + scale[b,c]) + shift[b,c] ; y = silu(y) if act
 * gamma/beta may be NULL (affine=False); scale/shift may be NULL; ss_bs = batch stride of
 * scale/shift rows in elements.
 * ------------------------------------------------------------------------------------------- */
int64_t lc_groupnorm_partials_elems(int B, int C, int H, int W, int G);
int lc_groupnorm_stats(const float* x, int64_t x_bs, double* partials, int B, int C, int H, int W,
                       int G, lc_stream_t s);
int lc_groupnorm_apply(const float* x, int64_t x_bs, const double* partials, const float* gamma,
                       const float* beta, const float* scale, const float* shift, int64_t ss_bs,
                       float* y, int64_t y_bs, int B, int C, int H, int W, int G, float eps,
                       int act_silu, lc_stream_t s);
/* The apply pass as the training graph runs it: additionally writes the (mean, rstd) it normalised with into
 * mean_rstd_out [B, G, 2] (may be NULL; what lc_groupnorm_bwd* reads -- no lc_groupnorm_meanrstd launch) and stores max|y|
 * of every block of the pass into amax_out[0 .. lc_groupnorm_amax_partials(B, C, H, W, G, 0)) (may be NULL; every
 * element is written, nothing to initialise) for lc_range_from_amax of the conv that consumes y. */
int64_t lc_groupnorm_amax_partials(int B, int C, int H, int W, int G, int backward);
int lc_groupnorm_apply_train(const float* x, int64_t x_bs, const double* partials, const float* gamma,
                             const float* beta, const float* scale, const float* shift, int64_t ss_bs,
                             float* y, int64_t y_bs, int B, int C, int H, int W, int G, float eps,
                             int act_silu, float* mean_rstd_out, float* amax_out, lc_stream_t s);

/* The same normalisation from the PRODUCER's octet statistics (lc_conv2d_ring_f16x2_fwd
 * gn_ostats_out): one launch, the tensor is read once.  A tensor may be the channel concatenation of
 * two producers' outputs (torch.cat([h, skip]) efficient_unet.py:293-295): s0 covers channels
 * [0, s0->channels), s1 (may be NULL) the rest.  Needs (C/G) % 8 == 0 and every group inside one
 * segment (LC_EUNSUP otherwise: use stats + apply).  The fold is fp64 around one common pivot per
 * group in a fixed order (deterministic). */
int lc_groupnorm_apply_os(const float* x, int64_t x_bs, const lc_oct_stats* s0, const lc_oct_stats* s1,
                          const float* gamma, const float* beta, const float* scale,
                          const float* shift, int64_t ss_bs, float* y, int64_t y_bs, int B, int C,
                          int H, int W, int G, float eps, int act_silu, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * FIR resampling x2, window [1,3,3,1], ring=True: ops.Resample ops.py:52-146
 * (closed forms SURVEY.md §8a-10).  dir = +1 upsample (H,W -> 2H,2W), -1 downsample.
 * ------------------------------------------------------------------------------------------- */
int lc_resample2x_fwd(const float* x, int64_t x_bs, float* y, int64_t y_bs, int B, int C, int H,
                      int W, int dir, lc_stream_t s);
/* Round 6: a resampling ResBlock of the layout model (layout_unet_v1.py:81-150: h = op(SiLU(GroupNorm(x))), x = op(x)) in ONE
 * pass over x.  lc_groupnorm_coeffs_os: the rows (mu, A, Bc, 0) [B][Cpad] of lc_groupnorm_coeffs, derived from the producer's
 * statistics entries (no statistics pass); lc_resample2x_pair_fwd: y = resample(x) (bit-identical to lc_resample2x_fwd) and
 * y_act = resample(SiLU((x - mu) * A + Bc)). */
int lc_groupnorm_coeffs_os(const lc_oct_stats* s0, const lc_oct_stats* s1, const float* gamma, const float* beta,
                           const float* scale, const float* shift, int64_t ss_bs, float* coeffs, int B, int C, int Cpad,
                           int G, float eps, lc_stream_t s);
int lc_resample2x_pair_fwd(const float* x, int64_t x_bs, const float* coeffs, int Cpad, float* y, int64_t y_bs,
                           float* y_act, int64_t ya_bs, int B, int C, int H, int W, int dir, lc_stream_t s);
/* Down-sampling that also leaves GroupNorm statistics of its OUTPUT (round 5): one entry per (sample, channel, slot) in
 * the producer-statistics format with unit = 1 -- ostats[B, C, slots, 4], slots = lc_resample2x_stats_slots(H, W, -1)
 * (0: the shape takes the scalar kernel, which leaves none; lc_resample2x_stats_fwd then returns LC_EUNSUP).  The
 * GroupNorm behind a Resample(down=2) (efficient_unet.py:141-143 -> :79) folds them instead of taking a statistics pass. */
int64_t lc_resample2x_stats_slots(int H, int W, int dir);
int lc_resample2x_stats_fwd(const float* x, int64_t x_bs, float* y, int64_t y_bs, int B, int C, int H,
                            int W, int dir, float* ostats, lc_stream_t s);

/* Round 6 (third part): Conv2d(3x3, ring) BEHIND Resample(up=2) folded -- layout_unet_v1.py:219-235 (ResBlock up=True:
 * in_rest -> op(h) -> in_conv) and efficient_unet.py:143-145 (Block.upsample), ops.py:52-173.  Both operators are linear:
 *   conv3x3(U(a))[r][s] = bias + sum_{ky,kx} U(P_{ky,kx})[r + ky - 1][s + kx - 1 (ring)],   P_{ky,kx} = W[:, :, ky, kx] . a
 * (rows of U(.) outside [0, 2H) are the conv's zero padding).  The nine planes are ONE 1x1 projection Ci -> 9 Co of the
 * LOW-resolution operand (lc_conv1x1_f16x2_ps_fwd with the weight rows ordered t Co + co, t = 3 ky + kx: a quarter of the
 * 3x3 conv's multiply-adds), lc_up2_combine9_fwd reads them once and writes y [B][Co][2H][2W] once, with the bias and --
 * ostats != NULL -- one GroupNorm statistics entry per (sample, channel, slot) of what it stores (lc_oct_stats, unit = 1,
 * ostats[B][Co][slots][4], slots = lc_up2_combine9_stats_slots(H, W); 0: shape unsupported).  Needs W % 128 == 0, p9
 * 8-byte and y 16-byte aligned (LC_EUNSUP otherwise).
 * lc_split_act_fwd: the plain fp32 -> pre-split pass (x * range->x_scale as fp16 hi / lo planes in the layout of
 * lc_groupnorm_apply_split, lc_split_act_units(B, C, H, W) units; publishes max |x * x_scale|) for an operand that no
 * GroupNorm apply pass writes; C % 16 == 0, H * W % 4 == 0, x 16-byte aligned. */
int lc_split_act_fwd(const float* x, int64_t x_bs, void* y_split, int B, int C, int H, int W, lc_conv_range* range,
                     lc_stream_t s);
int64_t lc_up2_combine9_stats_slots(int H, int W);
int lc_up2_combine9_fwd(const float* p9, int64_t p_bs, const float* bias, float* y, int64_t y_bs, int B, int Co, int H,
                        int W, float* ostats, lc_stream_t s);
/* ... the same, and y2 [B][Co][2H][2W] = Resample(up=2)(x) of a second low-resolution tensor x [B][Co][H][W] in the same launch
 * (the skip path of LayoutUnetV1's up-sampling ResBlock, layout_unet_v1.py:232; bit-identical to lc_resample2x_fwd). */
int lc_up2_combine9_xup_fwd(const float* p9, int64_t p_bs, const float* bias, float* y, int64_t y_bs, const float* x,
                            int64_t x_bs, float* y2, int64_t y2_bs, int B, int Co, int H, int W, float* ostats, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Small dense layer  y[m, n] = sum_k act(x[m,k]) * w[n,k] + b[n]   (w in nn.Linear layout).
 * Time-embedding MLP efficient_unet.py:237-242 / layout_unet_v1.py:683-688, AdaGN projection
 * ops.py:190-194, ResBlock.emb_layers layout_unet_v1.py:196-202.  act_in: 0 none, 1 SiLU.
 * lc_sinusoid: ops.SinusoidalPositionalEmbedding ops.py:14-29 (input = log-SNR).
 * ------------------------------------------------------------------------------------------- */
int lc_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int K, int N,
                  int act_in, int act_out, lc_stream_t s);
int lc_sinusoid_fwd(const float* t, float* y, int M, int channels, float max_period,
                    lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Attention over range-image tokens, channel-major operands (a [d, L] matrix per head with L
 * contiguous), flash-style (no score matrix in HBM), fp32 MFMA for QK^T and PV:
 *   o[c, t] = sum_s softmax_s(scale * sum_c' q[c',t] k[c',s]) v[c, s]
 * nn.MultiheadAttention in SelfAttentionBlock efficient_unet.py:28-58;
 * QKVAttentionLegacy layout_unet_v1.py:555-596; ObjectAwareCrossAttention.forward
 * layout_unet_v1.py:489-506 (image keys ++ 13 layout keys, d_qk = 2*d_v).
 * An operand is described by lc_cm_operand: head (b,h) starts at p + b*bs + h*hs, channel
 * stride cs, unit token stride.  The q/k channels of a head are the concatenation of a content
 * part (dqk channels, operands q / k / k2) and an optional positional part (dpos channels,
 * operands q_pos / k_pos / k2_pos; NULL when dpos == 0) -- the torch.cat([content, positional])
 * of layout_unet_v1.py:453-454,476 is never materialised.  Keys/values come in two token
 * segments: (k, k_pos, v) with Lk0 tokens and optionally (k2, k2_pos, v2) with Lk1 tokens
 * (the 13 layout tokens, layout_unet_v1.py:479-480).  dqk+dpos <= 64, dv <= 64.
 * ------------------------------------------------------------------------------------------- */
typedef struct lc_cm_operand {
    const float* p;
    int64_t bs, hs, cs;
} lc_cm_operand;

int lc_attention_fwd(const lc_cm_operand* q, const lc_cm_operand* q_pos,
                     const lc_cm_operand* k, const lc_cm_operand* k_pos, const lc_cm_operand* v,
                     const lc_cm_operand* k2, const lc_cm_operand* k2_pos, const lc_cm_operand* v2,
                     float* o, int64_t o_bs, int64_t o_hs, int64_t o_cs,
                     int B, int heads, int Lq, int Lk0, int Lk1, int dqk, int dpos, int dv,
                     float scale, lc_stream_t s);
/* Same contract, f16x2-split arithmetic (the default of the Python layer): q, k, p and v are split
 * into fp16 hi/lo parts of the pre-scaled fp32 values, every product is accumulated in fp32 as
 * ah*bh + ah*bl + al*bh with v_mfma_f32_32x32x16_f16 (per-product error ~5e-7, same tolerance as
 * lc_attention_fwd in tests/test_hip_parity.py). */
int lc_attention_f16x2_fwd(const lc_cm_operand* q, const lc_cm_operand* q_pos,
                           const lc_cm_operand* k, const lc_cm_operand* k_pos,
                           const lc_cm_operand* v, const lc_cm_operand* k2,
                           const lc_cm_operand* k2_pos, const lc_cm_operand* v2, float* o,
                           int64_t o_bs, int64_t o_hs, int64_t o_cs, int B, int heads, int Lq,
                           int Lk0, int Lk1, int dqk, int dpos, int dv, float scale,
                           lc_stream_t s);
/* Which kernel a call runs (pure host code, no GPU needed; the launchers switch on the same function, csrc/attention_route.h).
 * lc_attention_route: the forward entries.  split: 1 for lc_attention_f16x2_fwd and lc_attention_train_fwd(f16x2 = 1);
 *   has_amax: lc_attention_train_fwd with qkv_amax; bh = B * heads; waves_env: an LC_ATTN_WAVES value (0 = unset), or < 0
 *   for the value this process cached.  lc_attention_bwd_route: lc_attention_bwd (split 0) / lc_attention_bwd_f16x2 (1).
 * Both return  family << 16 | DQK << 8 | NDV << 4 | (waves == 8) << 1 | PRE  with family 1 fp32 forward (attn_kernel),
 *   2 f16x2-split forward (attn_h_kernel), 3 fp32 backward, 4 split backward; DQK = 32 / 64 and NDV = 1 / 2 the
 *   instantiated q / k channel count and 32-channel blocks of v; PRE = 1: pre-scales from the measured maxima.
 *   The codes of the entries where they refuse: LC_EINVAL for bh <= 0, Lq <= 0, dpos < 0; LC_EUNSUP for dqk <= 0,
 *   dqk + dpos > 64, dv <= 0, dv > 64, B * heads > 65535 (the grid's y extent).
 * A split request goes to the fp32 kernels when dqk % 8 or dpos % 8: the split kernel stages K in units of 8 channel
 * rows of ONE operand without a per-channel guard.
 * Range contract of the inference split routes (lc_attention_f16x2_fwd, lc_attention_units_fwd and the units the qkv
 * projection writes): the operands are split with the CONSTANT pre-scale 16.  With m_q = max|q * scale * log2(e)|,
 * m_k = max|k|, m_v = max|v| (every positional part and second segment included):
 *   representable  16 * m in [4, 32768), i.e. 0.25 <= m < 2048, for each of m_q, m_k, m_v: nothing saturates, the
 *                  result is finite and no worse than 4 x the error of the same attention evaluated in float32;
 *   accurate       the tolerance of lc_attention_fwd (2e-6 rel-L2 against float64) holds where, in addition,
 *                  m_q * m_k <= 32 / sqrt(dqk + dpos): scores that deviate by about one nat over the keys.  With both
 *                  operands representable this ends at m = 128 / sqrt(dqk + dpos) for q and k; m_v may be anywhere
 *                  in its window.  With sharper scores float32 itself comes to that tolerance or past it.
 * Outside the representable window the result loses accuracy (below) or saturates (above) silently;
 * lc_attention_fwd and the training entry (measured pre-scales) have no such window. */
int lc_attention_route(int split, int has_amax, int dqk, int dpos, int dv, int64_t bh, int Lq, int waves_env);
int lc_attention_bwd_route(int split, int dqk, int dv, int64_t bh);
/* MeanFlow generator (MFEfficientUNet, lidargen/models/unets/efficient_mf_unet.py; csrc/flow.hip).
 * lc_qk_norm_cm_fwd: in place, per (sample b, head h, token t) of the channel-major q and k operands -- the q / k
 *   channel slices of the qkv projection's [B, 3C, L] output -- the d channels h*d .. h*d+d-1 (channel stride q_cs / k_cs,
 *   unit token stride, sample stride q_bs / k_bs) become v / max(||v||_2, 1e-12) * sqrt(d) * g, g = g_q[0] / g_k[0]
 *   (device pointers: timm Attention's q_norm / k_norm RMSNorm gains, read on the device).  d <= 64 and
 *   B * heads <= 65535 (LC_EUNSUP), every size positive (LC_EINVAL); checked before any launch.
 * lc_flow_step_fwd: out[b] = z[b] - dt[b] * u[b] over n elements per sample (batch strides z_bs, u_bs, out_bs; dt a
 *   device float [B]); out == z is allowed.  The product and the difference are rounded separately, as torch does. */
int lc_qk_norm_cm_fwd(float* q, int64_t q_bs, int64_t q_cs, float* k, int64_t k_bs, int64_t k_cs, const float* g_q,
                      const float* g_k, int B, int heads, int d, int L, lc_stream_t s);
int lc_flow_step_fwd(const float* z, int64_t z_bs, const float* u, int64_t u_bs, const float* dt, float* out,
                     int64_t out_bs, int B, int64_t n, lc_stream_t s);
/* Hourglass Diffusion Transformer (HDiT, lidargen/models/dits/hdit.py; csrc/hdit.hip).  Token grids are channel-major
 * [B, C, h, w] with unit token stride; every size positive and every pointer non-NULL (LC_EINVAL), B (or B * heads)
 * <= 65535 (LC_EUNSUP); all checked before any launch.
 * lc_hdit_rmsnorm_fwd: per (sample b, token t): y[c] = x[c] * rsqrt(mean_c x^2 + eps) * f, f = 1 (mode 0),
 *   1 + m[b * f_bs + c] (mode 1, AdaRMSNorm) or g[c] (mode 2, gain); channel strides x_cs / y_cs, L tokens.
 *   Rows [B, C] are L = 1 with x_cs = y_cs = 1.
 * lc_hdit_geglu_fwd: y[b, c, l] = x[b, c, l] * gelu_erf(x[b, mid + c, l]) for c < mid (x: [B, 2 mid, L] per sample).
 * lc_hdit_qk_prep_fwd: in place on q and k ([B, heads * d, L], channel strides q_cs / k_cs, d in {32, 64}): per head,
 *   v / max(||v||_2, 1e-6) * sqrt(exp(min(scale[head], ln 100))), then channel i < d/2 and i + d/2 rotated by
 *   theta[head, i, t] given as cos_t / sin_t [heads, d/2, L] (the axial RoPE tables).
 * lc_hdit_na_fwd: neighbourhood attention on an h x w grid: query (i, j) attends to rows r0 .. r0+kh-1,
 *   r0 = clamp(i - kh/2, 0, h - kh), and columns (j - kw/2 + s) mod w, s < kw; softmax(scale * q.k) v in fp32.
 *   kh, kw odd, kh * kw <= 81, kh <= h, kw/2 <= w, d in {32, 64} (LC_EUNSUP).  o: [B, heads * d, h * w] strides.
 * lc_hdit_space_to_depth_fwd: out[b, (p1*P2+p2)*C + c, y, x] = in[b, c, P1*y+p1, P2*x+p2]; H % P1 == W % P2 == 0.
 * lc_hdit_depth_to_space_fwd: out[b, c, P1*y+p1, P2*x+p2] = in[b, (p1*P2+p2)*C + c, y, x], then, when skip is given,
 *   torch.lerp(skip, ., sigmoid(alpha[c])).  in is [B, C*P1*P2, h, w], out / skip [B, C, h*P1, w*P2] per sample.
 * lc_hdit_tokenize_fwd: y[b, c, h, x] = sum_{ci, p} wt[c, ci, p] x[b, ci, h, P*x+p] + pe[c, h, x] (Conv2d kernel and
 *   stride (1, P), no bias, plus the channel-major positional embedding [C, H, W/P]).
 * lc_hdit_fourier_fwd: y[m] = [cos | sin](t[m] * 2 pi * freqs[i]), i < half; y is [M, 2 half]. */
int lc_hdit_rmsnorm_fwd(const float* x, int64_t x_bs, int64_t x_cs, const float* f, int64_t f_bs, int mode, float* y,
                        int64_t y_bs, int64_t y_cs, int B, int C, int L, float eps, lc_stream_t s);
int lc_hdit_geglu_fwd(const float* x, int64_t x_bs, float* y, int64_t y_bs, int B, int mid, int L, lc_stream_t s);
int lc_hdit_qk_prep_fwd(float* q, int64_t q_bs, int64_t q_cs, float* k, int64_t k_bs, int64_t k_cs, const float* scale,
                        const float* cos_t, const float* sin_t, int B, int heads, int d, int L, lc_stream_t s);
int lc_hdit_na_fwd(const lc_cm_operand* q, const lc_cm_operand* k, const lc_cm_operand* v, float* o, int64_t o_bs,
                   int64_t o_hs, int64_t o_cs, int B, int heads, int d, int h, int w, int kh, int kw, float scale,
                   lc_stream_t s);
int lc_hdit_space_to_depth_fwd(const float* in, int64_t in_bs, float* out, int64_t out_bs, int B, int C, int H, int W,
                               int P1, int P2, lc_stream_t s);
int lc_hdit_depth_to_space_fwd(const float* in, int64_t in_bs, float* out, int64_t out_bs, const float* skip,
                               int64_t skip_bs, const float* alpha, int B, int C, int h, int w, int P1, int P2,
                               lc_stream_t s);
int lc_hdit_tokenize_fwd(const float* x, int64_t x_bs, const float* wt, const float* pe, float* y, int64_t y_bs, int B,
                         int Cin, int C, int H, int W, int P, lc_stream_t s);
int lc_hdit_fourier_fwd(const float* t, const float* freqs, float* y, int M, int half, lc_stream_t s);
/* HDiT training (csrc/hdit.hip, csrc/hdit_bwd.hip; lidarcrafter_amd/autograd_hdit.py).  Same conventions as the HDiT
 * forward entries above: sizes positive and pointers non-NULL (LC_EINVAL), B (or B * heads) <= 65535, d in {32, 64}
 * (LC_EUNSUP), all checked before any launch.  Every reduction runs in a fixed order without atomics (bit-reproducible).
 * lc_hdit_na_train_fwd: lc_hdit_na_fwd (o bit-identical) that also stores lse[(b * heads + h) * h*w + t] = m + log l,
 *   the log-sum-exp of the query's scaled logits.
 * lc_hdit_rmsnorm_bwd: the backward of lc_hdit_rmsnorm_fwd (same x, f, mode, eps): dx (strides dx_bs / dx_cs, unit
 *   token stride), and when df is given (mode 1 or 2, rs then required) d(mod)[b * df_bs + c] (mode 1) or d(gain)[c]
 *   (mode 2) = sum of dy x rsqrt(mean x^2 + eps) over the tokens (and samples).  rs: scratch of B * L floats (the
 *   per-token rsqrt, may be NULL without df).
 * lc_hdit_geglu_bwd: dx[:, :mid] = dy gelu_erf(x[:, mid:]), dx[:, mid:] = dy x[:, :mid] gelu_erf'(x[:, mid:]).
 * lc_hdit_qk_prep_bwd: the backward of lc_hdit_qk_prep_fwd taken out of place: q / k the RAW slices (before the
 *   preparation), gq / gk the gradients of the prepared q / k, dq / dk the raw gradients (all [B, heads * d, L], their
 *   own batch / channel strides, unit token stride).  part: scratch of heads * B * 2 * L doubles; dscale [heads] (NULL
 *   skips it) = d(loss)/d(scale): (s / 2) sum(dq' . q' + dk' . k') / s with s = sqrt(exp(min(scale, ln 100))), 0 for
 *   a head with scale > ln 100 (float compare, torch's clamp rule: the gradient passes at the clamp value itself).
 * lc_hdit_na_bwd: the backward of lc_hdit_na_train_fwd: q, k, v, o, dout as operands, lse from the forward, dsum a
 *   scratch of B * heads * h*w floats (rowsum(dout * o)); dq, dk, dv contiguous [B, heads * d, h*w].  dk / dv gather
 *   over each key's inverse neighbourhood; the window limits are lc_hdit_na_fwd's.
 * lc_hdit_lerp_bwd: the backward of lc_hdit_depth_to_space_fwd with skip: dout [B, C, h*P1, w*P2]; y the forward's
 *   input in depth form [B, C*P1*P2, h, w]; dskip = (1 - a) dout, dy = space_to_depth(a dout) (batch strides
 *   dskip_bs / dy_bs, samples contiguous), dalpha[c] = a (1 - a) sum dout (d2s(y) - skip), a = sigmoid(alpha[c])
 *   (NULL skips it). */
int lc_hdit_na_train_fwd(const lc_cm_operand* q, const lc_cm_operand* k, const lc_cm_operand* v, float* o,
                         int64_t o_bs, int64_t o_hs, int64_t o_cs, float* lse, int B, int heads, int d, int h, int w,
                         int kh, int kw, float scale, lc_stream_t s);
int lc_hdit_rmsnorm_bwd(const float* x, int64_t x_bs, int64_t x_cs, const float* f, int64_t f_bs, int mode,
                        const float* dy, int64_t dy_bs, int64_t dy_cs, float* dx, int64_t dx_bs, int64_t dx_cs,
                        float* rs, float* df, int64_t df_bs, int B, int C, int L, float eps, lc_stream_t s);
int lc_hdit_geglu_bwd(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs, float* dx, int64_t dx_bs, int B,
                      int mid, int L, lc_stream_t s);
int lc_hdit_qk_prep_bwd(const float* q, int64_t q_bs, int64_t q_cs, const float* k, int64_t k_bs, int64_t k_cs,
                        const float* gq, int64_t gq_bs, int64_t gq_cs, const float* gk, int64_t gk_bs, int64_t gk_cs,
                        float* dq, int64_t dq_bs, int64_t dq_cs, float* dk, int64_t dk_bs, int64_t dk_cs,
                        const float* scale, const float* cos_t, const float* sin_t, double* part, float* dscale, int B,
                        int heads, int d, int L, lc_stream_t s);
int lc_hdit_na_bwd(const lc_cm_operand* q, const lc_cm_operand* k, const lc_cm_operand* v, const lc_cm_operand* o,
                   const lc_cm_operand* dout, const float* lse, float* dsum, float* dq, float* dk, float* dv, int B,
                   int heads, int d, int h, int w, int kh, int kw, float scale, lc_stream_t s);
int lc_hdit_lerp_bwd(const float* dout, int64_t dout_bs, const float* y, int64_t y_bs, const float* skip,
                     int64_t skip_bs, const float* alpha, float* dskip, int64_t dskip_bs, float* dy, int64_t dy_bs,
                     float* dalpha, int B, int C, int h, int w, int P1, int P2, lc_stream_t s);
/* MeanFlow training (csrc/flow_jvp.hip): the tangent evaluation u, du/dt = jvp(model, (z, t, r), (v, 1, 0)) of
 * MeanFlow.loss next to the differentiable primal, and the backward of the q / k RMSNorm.
 * lc_groupnorm_jvp_stats: per (sample, group, chunk) fp64 partials of sum(x - p), sum((x - p)^2), sum(dx), sum((x - p) dx)
 *   (p = the group's first element) into `partials` (lc_groupnorm_jvp_partials_elems doubles); the first two exactly as
 *   lc_groupnorm_stats forms them.
 * lc_groupnorm_jvp_apply_train: lc_groupnorm_apply_train's y, (mean, rstd) and partial maxima of |y| (same count), plus the
 *   tangent dy of y along (dx, dscale, dshift) (dscale / dshift may be NULL: zero; they need scale / shift) and the partial
 *   maxima of |dy| into damax_out (may be NULL).  gamma and beta are both given or both NULL.
 * lc_qk_norm_cm_jvp: out of place, per (sample, head, token) of channel-major operands (as lc_qk_norm_cm_fwd):
 *   y = sqrt(d) g x / max(||x||, 1e-12) (may be NULL) and dy = J dx, J = the Jacobian of that map (dx, dy both given or
 *   both NULL).  y is bit-identical to lc_qk_norm_cm_fwd's in-place result.
 * lc_qk_norm_cm_bwd: gx = J gy (J symmetric) and, when dg_partials (lc_qk_norm_cm_bwd_partials doubles) and dg (one
 *   float) are given, dg[0] = sum gy . y / g, reduced in a fixed order (no atomics).  d <= 64, B * heads <= 65535.
 * lc_attention_jvp_fwd: plain operands as lc_attention_train_fwd (q, dq [BH, dqk, Lq], k, dk [BH, dqk, Lk], v, dv
 *   [BH, dv, Lk]); writes o [BH, dv, Lq], lse [BH, Lq] (the base-2 log-sum-exp lc_attention_bwd* read) and the tangent
 *   dout [BH, dv, Lq] of o along (dq, dk, dv), in one pass over the keys (exact fp32).  dqk, dv <= 64, BH <= 65535.
 * Every entry checks its arguments before any launch (LC_EINVAL / LC_EUNSUP). */
int64_t lc_groupnorm_jvp_partials_elems(int B, int C, int H, int W, int G);
int lc_groupnorm_jvp_stats(const float* x, int64_t x_bs, const float* dx, int64_t dx_bs, double* partials, int B, int C,
                           int H, int W, int G, lc_stream_t s);
int lc_groupnorm_jvp_apply_train(const float* x, int64_t x_bs, const float* dx, int64_t dx_bs, const double* partials,
                                 const float* gamma, const float* beta, const float* scale, const float* shift,
                                 const float* dscale, const float* dshift, int64_t ss_bs, float* y, int64_t y_bs,
                                 float* dy, int64_t dy_bs, int B, int C, int H, int W, int G, float eps, int act_silu,
                                 float* mean_rstd_out, float* amax_out, float* damax_out, lc_stream_t s);
int lc_qk_norm_cm_jvp(const float* x, int64_t x_bs, int64_t x_cs, const float* dx, int64_t dx_bs, int64_t dx_cs,
                      const float* g, float* y, int64_t y_bs, int64_t y_cs, float* dy, int64_t dy_bs, int64_t dy_cs,
                      int B, int heads, int d, int L, lc_stream_t s);
int64_t lc_qk_norm_cm_bwd_partials(int B, int heads, int L);
int lc_qk_norm_cm_bwd(const float* x, int64_t x_bs, int64_t x_cs, const float* gy, int64_t gy_bs, int64_t gy_cs,
                      const float* g, float* gx, int64_t gx_bs, int64_t gx_cs, double* dg_partials, float* dg, int B,
                      int heads, int d, int L, lc_stream_t s);
int lc_attention_jvp_fwd(const float* q, const float* k, const float* v, const float* dq, const float* dk,
                         const float* dv, float* o, float* lse, float* dout, int BH, int Lq, int Lk, int dqk, int dv_ch,
                         float scale, lc_stream_t s);
/* Which way a call of the tangent kernels runs (pure host code, no GPU needed; the launchers and kernels switch on the
 * same functions, csrc/flow_jvp_route.h and csrc/gn_apply_route.h).  Addresses are passed modulo 16.  Each returns LC_OK,
 * or the code of its entry where that refuses a size (LC_EINVAL not positive or C % G, LC_EUNSUP beyond a limit).
 * lc_groupnorm_jvp_route: lc_groupnorm_jvp_stats / lc_groupnorm_jvp_apply_train.  Fills
 *   out[0] chunk          elements per statistics block (4096 or 16384)
 *   out[1] chunks         statistics blocks per (sample, group): lc_groupnorm_jvp_partials_elems = 4 B G out[1]
 *   out[2] stats branch   1 every (sample, group) is read as float4, 0 none is, 2 it differs by sample
 *   out[3] causes         seen on any (sample, group): bit 0 n % 4 (n = C / G H W), bit 1 a group of x off 16 bytes (either
 *                         sends the group to the scalar loop), bit 2 a group of dx off 16 bytes where x is not (the float4
 *                         loop with scalar loads of dx)
 *   out[4] dx loads       of the groups in the float4 loop: 1 all load dx as float4, 0 none does, 2 it differs by sample
 *   out[5] slabs          blocks per plane of the apply pass (ceil(H W / 4096))
 *   out[6] cpb            channels per apply block (1, 2, 4, ...: lc_groupnorm_apply_train's rule)
 *   out[7] amax slots     blocks of the apply pass = lc_groupnorm_amax_partials(B, C, H, W, G, 0)
 * lc_qk_norm_cm_route: lc_qk_norm_cm_jvp / lc_qk_norm_cm_bwd.  Fills out[0] channels held per token (16, 32 or 64),
 *   out[1] 256-token blocks per (sample, head), out[2] fp64 partials of dg (= lc_qk_norm_cm_bwd_partials), out[3] trips of
 *   the reduce's 256-lane loop over them.
 * lc_attention_jvp_route: lc_attention_jvp_fwd.  Fills out[0] padded head width (32 or 64), out[1] query rows per block
 *   (64 or 32), out[2] query blocks, out[3] 16-key tiles, out[4] keys in the last tile, out[5] query rows in the last
 *   block, out[6] / out[7] padded channels inside the last lane that holds a channel of q, k / of v (8 channels per lane). */
int lc_groupnorm_jvp_route(int B, int C, int H, int W, int G, int64_t x_bs, int64_t dx_bs, int x_addr_mod16,
                           int dx_addr_mod16, int32_t* out /* [8] */);
int lc_qk_norm_cm_route(int B, int heads, int d, int L, int32_t* out /* [4] */);
int lc_attention_jvp_route(int BH, int Lq, int Lk, int dqk, int dv_ch, int32_t* out /* [8] */);
/* Keys and values in UNIT FORM (round 6; csrc/attention_units.hip): the fp16 hi / lo split of lc_attention_f16x2_fwd
 * made once per step (or once per condition, for the step-invariant positional channels and the layout keys of
 * ObjectAwareCrossAttention, layout_unet_v1.py:431-476) instead of once per query block inside the attention kernel.
 * kv: [B][heads][tiles = Lk0 / 32 + (Lk1 > 0)][768] units of 8 halves -- per 32-key tile K hi, K lo ([8 channels-octets][32
 * keys]) and V hi, V lo ([2][2][32 channels], keys in MFMA accumulator order); zero where a head has no channel / key.
 * lc_attention_units_elems: halves to allocate (zero-filled by the caller), -1 for unsupported sizes (Lk0 % 32, Lk1 > 32).
 * lc_attention_pack_units: which = 0 writes keys (src: [B][heads * d][L] fp32 channel-major; the d channels land in
 * octets cb0 ... of a head's 64 q/k channels), which = 1 values (d <= 32); key0 (multiple of 32) = first destination key.
 * lc_attention_units_fwd: same result, bit for bit, as lc_attention_f16x2_fwd on the operands the units were packed
 * from (dqk + dpos <= 64, both multiples of 8, dv <= 32). */
/* lc_conv1x1_f16x2_ps_qkv_fwd: the qkv projection of ObjectAwareCrossAttention (conv_nd(1, C, 3 C, 1),
 * layout_unet_v1.py:381,416-430) on a pre-split input (lc_groupnorm_apply*_split) whose key and value rows are written
 * in unit form by the kernel's own epilogue -- q [B][C][H * W] fp32 (batch stride q_bs); 32 channels per head,
 * C % 128 == 0, (H * W) % 32 == 0; kv sized by lc_attention_units_elems(B, C / 32, H * W, Lk1). */
int lc_conv1x1_f16x2_ps_qkv_fwd(const void* x_split, const void* wp_hi, const void* wp_lo, const float* bias, float* q,
                                int64_t q_bs, void* kv, int B, int Ci, int C, int H, int W, int Lk1, const float* wmeta,
                                lc_conv_range* range, lc_stream_t s);
int64_t lc_attention_units_elems(int B, int heads, int Lk0, int Lk1);
int lc_attention_pack_units(const lc_cm_operand* src, void* kv, int B, int heads, int L, int Lk0, int Lk1, int d,
                            int cb0, int key0, int which, lc_stream_t s);
int lc_attention_units_fwd(const lc_cm_operand* q, const lc_cm_operand* q_pos, const void* kv, float* o,
                           int64_t o_bs, int64_t o_hs, int64_t o_cs, int B, int heads, int Lq, int Lk0, int Lk1,
                           int dqk, int dpos, int dv, float scale, lc_stream_t s);
/* ---------------------------------------------------------------------------------------------
 * Training: the same attention with a backward pass, so that loss.backward() never materialises
 * the [B*heads, Lq, Lk] scores or their gradient (autograd of nn.MultiheadAttention efficient_unet.py:28-58 and
 * of ObjectAwareCrossAttention.forward layout_unet_v1.py:489-506 as tools/train/train_lidm_cond.py:259-322 runs
 * them; softmax in fp32, layout_unet_v1.py:502).  Plain operands: heads back to back, per head a [d, L] matrix
 * with L contiguous -- q [BH, dqk, Lq], k [BH, dqk, Lk], v [BH, dv, Lk], o / do [BH, dv, Lq]; the caller
 * concatenates content / positional channels and image / layout keys (lidarcrafter_amd/autograd.py).
 * lc_attention_train_fwd = lc_attention_fwd (f16x2 = 0) or lc_attention_f16x2_fwd (1) + lse [BH, Lq]: the
 * log2-sum-exp of the scaled scores per query.  lc_attention_bwd recomputes P = exp2(S - lse) tile by tile in
 * exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) and writes dq, dk, dv (same shapes as q, k, v); deterministic (one
 * kernel with the queries as the outer dimension for dq, one with the keys for dk / dv; no atomics).
 * dsum_scratch: float [BH, Lq].  dqk, dv <= 64.
 * qkv_amax (round 6; f16x2 = 1 only, may be NULL): 3 floats of scratch the caller keeps alive until the backward pass has
 * run.  The forward measures max |q|, max |k|, max |v| into them on the device and both passes derive the powers of two
 * their fp16 hi / lo operand splits use from those words (16 while max |x| * 16 lies in [2^2, 2^15): the results of
 * rounds 1-5; otherwise the power of two that fits -- csrc/attention_pre.h).  NULL: the constant 16, which saturates
 * |x| >= 4094 silently.
 * ------------------------------------------------------------------------------------------- */
int lc_attention_train_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int BH, int Lq,
                           int Lk, int dqk, int dv, float scale, int f16x2, float* qkv_amax, lc_stream_t s);
int lc_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* dout,
                     const float* lse, float* dsum_scratch, float* dq, float* dk, float* dv, int BH, int Lq, int Lk,
                     int dqk, int dv_ch, float scale, lc_stream_t s);
/* The same backward pass with the f16x2-split arithmetic of lc_attention_f16x2_fwd (three v_mfma_f32_32x32x16_f16 per
 * product, fp32 accumulation; the default of lidarcrafter_amd.autograd).  The gradient dO may have any magnitude: its
 * maximum is measured next to D and the power of two that normalises it is carried exactly through dP, dS and the
 * outputs.  dsum_scratch: float [BH * Lq + 1] (the extra word holds max |dO|).  qkv_amax: the words
 * lc_attention_train_fwd measured for the same q, k, v (or NULL: constant pre-scale 16). */
int lc_attention_bwd_f16x2(const float* q, const float* k, const float* v, const float* o, const float* dout,
                           const float* lse, float* dsum_scratch, float* dq, float* dk, float* dv, int BH, int Lq,
                           int Lk, int dqk, int dv_ch, float scale, const float* qkv_amax, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Reverse-diffusion update, one fused elementwise pass:
 *   ContinuousTimeGaussianDiffusion.p_step continuous_time.py:209-231 (also
 *   continuous_time_cond.py:229-252).  coef[b*8 + ...] = {alpha_t, sigma_t, alpha_s, sigma_s,
 *   k0, k1, clip_range (<=0: no clip), unused}: ddpm k0 = c = -expm1(l_t-l_s), k1 = sigma_s*sqrt(c);
 *   ddim k0 = c1, k1 = c2.  objective: 0 eps, 1 v, 2 x_0.  mode: 0 ddpm, 1 ddim.
 *   noise may be NULL when its coefficient is 0 (ddim eta=0).  n = C*H*W per sample.
 *   DiscreteTimeGaussianDiffusion.p_step discrete_time.py:126-180 (round 3): mode 2 ddpm, 3 ddim with
 *   coef = {A, Bc, c2, c3, c4, c5, clip, c7}: x0 = A x_t - Bc pred (eps: A = rsqrt(ab), Bc =
 *   sqrt(1/ab - 1); v: sqrt(ab), sqrt(1 - ab); x_0: x0 = pred); ddpm (c2 x0 + c3 x_t) + c4 noise with
 *   c2 = sqrt(ab_prev) beta / (1 - ab), c3 = (1 - ab_prev) sqrt(alpha) / (1 - ab), c4 = sigma (0 at
 *   step 0); ddim c4 x0 + c5 (x_t - c2 x0) / c3 [+ c7 noise] with c2 = sqrt(ab), c3 = sqrt(1 - ab),
 *   c4 = sqrt(ab_prev), c5 = sqrt(1 - ab_prev - sd^2), c7 = sd.
 * ------------------------------------------------------------------------------------------- */
int lc_pstep_fwd(const float* x_t, int64_t xt_bs, const float* pred, int64_t pred_bs,
                 const float* noise, int64_t noise_bs, const float* coef, float* x_s,
                 int64_t xs_bs, int B, int64_t n, int objective, int mode, lc_stream_t s);

/* Point Condition Network epilogue of the foreground-object denoiser
 * (lidargen/models/unets/point_unet.py:14-26, PCNet): channel-major rows [B, C, N],
 *   y = act( x * sigmoid(gate_logit[b,c]) + bias[b,c] ) [+ res],  act: 0 none, 1 leaky_relu(0.01)
 * x = fea_layer(fea) from lc_conv2d_ring_*_fwd (1x1); gate_logit / bias rows [B, >=C] with row
 * stride gb_bs (slices of ONE batched cond_gate | cond_bias projection); res may be NULL. */
int lc_gate_bias_act(const float* x, int64_t x_bs, const float* gate_logit, const float* bias,
                     int64_t gb_bs, const float* res, int64_t res_bs, float* y, int64_t y_bs,
                     int B, int C, int N, int act, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Block.downsample of EfficientUNet folded: `ops.Conv2d(3x3, ring)` followed by `ops.Resample(down=2)`
 * (lidargen/models/unets/efficient_unet.py:132-135; ops.py:52-146 FIR [1 3 3 1] / 8, ring along W, zero padding of the
 * conv's OUTPUT along H; ops.py:149-173) evaluated as ONE stride-2 3x3 convolution of the FIR-pre-filtered input -- a quarter
 * of the reference conv's multiply-adds and output bytes, no resampling pass (csrc/conv_f16x2_s2.hip has the algebra).
 *
 * lc_fir_down2_prefilter_split: x [B, C, H, W] fp32 (batch stride x_bs floats, channel stride H*W; C % 16 == 0, H even >= 4,
 *   W % 128 == 0) -> y_split: the pre-filtered tensor F in the pre-split form of lc_groupnorm_apply_split (fp16 hi / lo
 *   planes, 16-byte units of 8 channels, already multiplied by range->x_scale; max |F * x_scale| is published into *range),
 *   per sample [2 planes][C / 8][H + 3 rows][W units]: rows 0 .. H = F[-1 .. H-1], row H + 1 / H + 2 = the top / bottom
 *   boundary variants; inside a row the odd input columns first (unit i = column 2 i - 1, ring), then the even ones.
 *   lc_fir_down2_split_units gives the number of 16-byte units of y_split.
 * lc_conv2d_ring_s2_f16x2_ps_fwd: y [B, Co, Ho, Wo] = (stride-2 conv of F with the layer's packed 3x3 weights + bias) *
 *   out_scale; Ho = H / 2, Wo = W / 2 (Wo % 64 == 0).  wp_hi / wp_lo / wmeta / range: as lc_conv2d_ring_f16x2_ps_fwd.
 *   gn_ostats_out (optional): octet (unit 8) or quad (unit 4) GroupNorm statistics entries of what it stores,
 *   [B][Co / unit][lc_conv2d_ring_s2_stats_slots(Ho, Wo)][4] floats. */
int64_t lc_fir_down2_split_units(int B, int C, int H, int W);
int lc_fir_down2_prefilter_split(const float* x, int64_t x_bs, void* y_split, int B, int C, int H, int W,
                                 lc_conv_range* range, lc_stream_t s);
int64_t lc_conv2d_ring_s2_stats_slots(int Ho, int Wo);
int lc_conv2d_ring_s2_f16x2_ps_fwd(const void* x_split, const void* wp_hi, const void* wp_lo, const float* bias, float* y,
                                   int64_t y_bs, int B, int Ci, int Co, int Ho, int Wo, float out_scale,
                                   float* gn_ostats_out, int gn_ostats_unit, const float* wmeta, lc_conv_range* range,
                                   lc_stream_t s);

/* Box calibration for bench.py (`box_calibration`): what THIS box's matrix pipes and memory sustain, so that numbers of
 * different boxes of the pool can be compared.  No counterpart in the reference.
 * lc_calibrate_mfma_f16: `blocks` blocks of 8 waves run `iters` x 16 v_mfma_f32_32x32x16_f16 per wave on the caller's
 * operands (blocks * 512 * 4 half8 vectors = blocks * 32 KiB of fp16; random data: the sustained rate depends on the
 * operand bits), one float per thread into sink[blocks * 512].  Returns the FLOPs of the launch (> 0) or a negative code.
 * lc_calibrate_stream_copy: dst[i] = src[i], n floats (multiple of 4, 16-byte aligned), float4 grid-stride. */
int64_t lc_calibrate_mfma_f16(const void* operands, int blocks, int iters, float* sink, lc_stream_t s);
int lc_calibrate_stream_copy(const float* src, float* dst, int64_t n, lc_stream_t s);

/* Strided copy of [B, C*H*W] blocks (fills a channel slice of a concat buffer). */
int lc_copy_strided(const float* x, int64_t x_bs, float* y, int64_t y_bs, int B, int64_t n,
                    lc_stream_t s);
/* y = (a + b) * scale  (SelfAttentionBlock residual efficient_unet.py:55-57). */
int lc_add_scale(const float* a, int64_t a_bs, const float* b, int64_t b_bs, float* y,
                 int64_t y_bs, int B, int64_t n, float scale, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * BACKWARD kernels (training: tools/train/train_lidm[_cond].py:259-322 run autograd through the
 * denoiser).  Plain fp32 NCHW tensors with batch strides as in the forward.
 *
 * Ring convolution.  The gradient with respect to the input is the SAME ring convolution applied to
 * dY with the transposed, 180-degree rotated kernel (run lc_conv2d_ring_*_fwd on it); the gradient
 * with respect to the weights and bias is lc_conv2d_ring_wgrad:
 *   dW[co][ci][ky][kx] (+)= sum_{b,h,w} dY[b,co,h,w] * Xpad[b,ci,h+ky-1,w+kx-1],  db[co] (+)= sum dY
 * fp32 matrix cores (exact fp32 products, fp32 accumulation), deterministic two-stage reduction;
 * scratch: lc_conv2d_ring_wgrad_scratch_elems floats (8-byte aligned); dbias may be NULL; accumulate != 0 adds to
 * dw / dbias (gradient accumulation), 0 overwrites.
 *
 * GroupNorm (+affine) (+AdaGN scale/shift) (+SiLU), forward y = silu?(((x-mu) rstd g + be)(1+sc) + sf):
 *   lc_groupnorm_meanrstd: (mean, rstd) per (sample, group) [B, G, 2] from the lc_groupnorm_stats partials;
 *   lc_groupnorm_bwd: rows[b][c] = (sum_hw dt2, sum_hw dt2 * xhat) as doubles [B, C, 2] with
 *   dt2 = dy * silu'(.), and dx = rstd (g (1+sc) dt2 - mean_g(.) - xhat mean_g(. xhat)).  The small
 *   parameter gradients follow from `rows`: dshift = r1, dscale = g r3 + be r1,
 *   dbeta = sum_b (1+sc) r1, dgamma = sum_b (1+sc) r3.
 * ------------------------------------------------------------------------------------------- */
int64_t lc_conv2d_ring_wgrad_scratch_elems(int B, int Ci, int Co, int H, int W, int ks);
int lc_conv2d_ring_wgrad(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs, float* scratch,
                         float* dw /* [Co,Ci,ks,ks] */, float* dbias /* [Co] or NULL */, int B, int Ci,
                         int Co, int H, int W, int ks, int accumulate, lc_stream_t s);
/* The same gradient on the f16 matrix cores with the operand split of the f16x2 forward (3 MFMAs per
 * product, per-product error ~2^-22, fp32 accumulation; contraction over pixels, which NCHW stores
 * contiguously -- no transposition): x and dy are pre-scaled by the power-of-two x_scale of
 * `x_range` / `dy_range` (records of exactly these tensors: lc_range_from_tensor right before the
 * forward conv of x and the input-gradient conv of dy, lidarcrafter_amd/autograd.py) and the result
 * is unscaled by both.  Needs H even, W % 32 == 0 and 16-byte aligned rows (LC_EUNSUP otherwise: use
 * lc_conv2d_ring_wgrad); scratch and everything else as lc_conv2d_ring_wgrad. */
int lc_conv2d_ring_wgrad_f16x2(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs,
                               const lc_conv_range* x_range, const lc_conv_range* dy_range,
                               float* scratch, float* dw, float* dbias, int B, int Ci, int Co, int H,
                               int W, int ks, int accumulate, lc_stream_t s);
int lc_groupnorm_meanrstd(const float* x, int64_t x_bs, const double* partials, float* mean_rstd,
                          int B, int C, int H, int W, int G, float eps, lc_stream_t s);
int lc_groupnorm_bwd(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs,
                     const float* mean_rstd, const float* gamma, const float* beta, const float* scale,
                     const float* shift, int64_t ss_bs, double* rows, float* dx, int64_t dx_bs, int B,
                     int C, int H, int W, int G, int act_silu, lc_stream_t s);
/* lc_groupnorm_bwd plus, in the same two launches: the parameter gradients from `rows` (fp64 arithmetic, fp32 results;
 * any of them may be NULL): dgamma, dbeta [C]; dscale, dshift [B, C] contiguous -- and the partial maxima of |dx| into
 * amax_out[0 .. lc_groupnorm_amax_partials(..., 1)) (may be NULL; as lc_groupnorm_apply_train): dx is the dY of the conv
 * that produced x. */
int lc_groupnorm_bwd_train(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs,
                           const float* mean_rstd, const float* gamma, const float* beta, const float* scale,
                           const float* shift, int64_t ss_bs, double* rows, float* dx, int64_t dx_bs,
                           float* dgamma, float* dbeta, float* dscale, float* dshift, int B, int C, int H, int W,
                           int G, int act_silu, float* amax_out, lc_stream_t s);
/* Which way a backward call runs (pure host code, no GPU needed; the launchers and kernels switch on the same functions,
 * csrc/conv_bwd_route.h and csrc/gn_bwd_route.h).  Addresses are passed modulo 16.
 * lc_conv2d_ring_wgrad_route: split 0 = lc_conv2d_ring_wgrad, 1 = lc_conv2d_ring_wgrad_f16x2.  Fills
 *   out[0] kernel family   1 exact-fp32 MFMA kernel, 2 f16x2-split kernel
 *   out[1] staging         1 float4 loads, 0 scalar loads (fp32 kernel: W % 64, H W % 4, x_bs % 4, dy_bs % 4 or an address
 *                          off 16 bytes; the split kernel has the float4 form only)
 *   out[2] nsplit          blocks per 64 x 64 channel tile = partial sums per weight, from B H ceil(W / 64) pixel tiles
 *   out[3] tiles           pixel tiles of the chosen kernel: B H ceil(W / 64) (fp32), B (H / 2) (W / 32) (split); blocks
 *                          beyond the tile count write zero partials
 *   out[4] bias branch     1 every (sample, channel) plane of dy is read as float4, 0 none is, 2 it differs by sample
 *   out[5] bias offset     floats of the scratch in front of the Co * B fp64 bias partials (an even count);
 *                          lc_conv2d_ring_wgrad_scratch_elems = out[5] + 2 Co B
 *   out[6] scalar causes   fp32 kernel: bit 0 W % 64, 1 H W % 4, 2 x_bs % 4, 3 dy_bs % 4, 4 x address, 5 dy address
 *   out[7] 0
 *   and returns LC_OK, or the code of the entry where it refuses: LC_EINVAL for a size that is not positive, LC_EUNSUP for
 *   ks other than 1 / 3 and, split = 1, for H odd, W % 32, a batch stride % 4 or an address off 16 bytes.
 * lc_groupnorm_bwd_route: lc_groupnorm_bwd_train / lc_groupnorm_bwd.  Fills out[0] blocks per plane of the apply pass
 *   (ceil(H W / 4096)), out[1] pixels per block, out[2] the apply pass's branch (1 float4, 0 scalar, 2 differs by sample:
 *   float4 needs H W % 4 == 0, out[1] % 4 == 0 and the planes of x, dy and dx on 16 bytes), out[3] outer iterations of
 *   the rows pass (4096 pixels each); LC_EINVAL for a size that is not positive or C % G. */
int lc_conv2d_ring_wgrad_route(int split, int B, int Ci, int Co, int H, int W, int ks, int64_t x_bs, int64_t dy_bs,
                               int x_addr_mod16, int dy_addr_mod16, int32_t* out /* [8] */);
int lc_groupnorm_bwd_route(int B, int C, int H, int W, int G, int64_t x_bs, int64_t dy_bs, int64_t dx_bs,
                           int x_addr_mod16, int dy_addr_mod16, int dx_addr_mod16, int32_t* out /* [4] */);

/* ---------------------------------------------------------------------------------------------
 * Voxel scatter of the weight-free metrics (lidargen/metrics/metric_utils.py).
 * lc_bev_occupancy_accumulate: ONE sweep of pcd2bev_sum (:233-258): points with x in (x0, x1) and
 *   y in (y0, y1) are binned to ix = floor(x / voxel) - min_bound_x (float32 division, as numpy),
 *   every voxel the sweep touches gets +1 in `grid` [nx, ny] float32 -- exactly once per sweep:
 *   `stamps` [nx*ny] int32 (zero-initialised by the caller, one per grid) holds the id of the last
 *   sweep that touched the voxel; pass a `stamp` != 0 that differs from sweep to sweep, and run
 *   the sweeps of one grid in stream order.  pt_stride = floats per point row (>= 2).
 * lc_sparse_quantize (:28-66): floor(coords / voxel) -> int32 [N, D] (D = 2 or 3; the float64 quotient of
 *   the float32 coordinate by the DOUBLE voxel size, as numpy divides by a float64 array), unique rows in
 *   ravel-hash (= lexicographic) order -> out_coords (first *out_count rows valid), out_index =
 *   index of each unique row's FIRST occurrence (may be NULL), out_inverse [N] (may be NULL) --
 *   np.unique(ravel_hash(q), return_index, return_inverse).  out_count: device uint64.
 *   scratch: lc_sparse_quantize_scratch_bytes(N, D) bytes of device memory.
 * ------------------------------------------------------------------------------------------- */
int lc_bev_occupancy_accumulate(const float* pts, int pt_stride, int N, float x0, float x1, float y0,
                                float y1, float voxel, int min_bound_x, int min_bound_y, int nx,
                                int ny, int stamp, int32_t* stamps, float* grid, lc_stream_t s);
int64_t lc_sparse_quantize_scratch_bytes(int N, int D);
int lc_sparse_quantize(const float* coords, int N, int D, double vx, double vy, double vz, void* scratch,
                       int32_t* out_coords, int64_t* out_index, int64_t* out_inverse,
                       uint64_t* out_count, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Point cloud -> range image, lidargen/dataset/transforms_3d/common.py:26-91 with
 * scan_unfolding=False: spherical cell per point, nearest point per cell wins (z-buffer via
 * 64-bit atomicMin on (depth_bits<<32 | point_idx); equal depths: lowest index wins), mask
 * channel = depth in [min_depth, max_depth] applied by the caller like the reference.
 * points [N,4] (x,y,z,intensity); zbuf u64[H*W] scratch; image [H,W,6]; winner int32[H*W] (-1
 * empty) may be NULL; cells int32[N,2] (grid_h, grid_w) may be NULL.  All float32 operations
 * correctly rounded (asin/atan2 evaluated in fp64, rounded once).  elev_f64 = 1: the elevation ->
 * row arithmetic runs in float64 on the float32 asin, as the reference computes under numpy >= 2
 * (oracle/lidar.py "native_cr" -- the mode the committed reference fixtures are reproduced in);
 * 0: all-float32, the reference under its pinned numpy 1.23.5 (oracle "f32").
 * ------------------------------------------------------------------------------------------- */
int lc_project_points(const float* points, int N, int H, int W, double fov_up_deg,
                      double fov_down_deg, float min_depth, float max_depth, uint64_t* zbuf,
                      float* image, int32_t* winner, int32_t* cells, int elev_f64, lc_stream_t s);
/* Workspace variant (round 4): `zbuf` is a caller-owned u64[H*W] that holds ~0 in every cell on entry --
 * lc_project_workspace_init leaves it so -- and is handed back in that state (the gather pass re-empties each cell
 * it reads), so a projection is two launches instead of three and the caller allocates nothing per call: 18 -> 8 us
 * at the 34 720 points of a nuScenes sweep, where the three-launch form is latency-bound.  One projection at a time
 * per workspace.  Same results as lc_project_points. */
int lc_project_workspace_init(uint64_t* zbuf, int n_cells, lc_stream_t s);
int lc_project_points_ws(const float* points, int N, int H, int W, double fov_up_deg,
                         double fov_down_deg, float min_depth, float max_depth, uint64_t* zbuf,
                         float* image, int32_t* winner, int32_t* cells, int elev_f64, lc_stream_t s);
/* The same projection of FLOAT64 points [N,4] -- what the temporal glue hands over
 * (tools/vis_tools/utils/pipe_related.py:245-258: the float64 product `Ts @ homo` and the float64
 * concatenation [background | re-posed objects]): every line of common.py:41-84 runs in float64
 * and the image is rounded to float32 once (:87-91).  winner int32[H*W] is REQUIRED (pass 2 of the
 * z-buffer: lowest index among the points at the cell's minimum depth).  Pinned on the reference's
 * own CustomDataset item / refine_next_frame_points (tests/golden/pipe_next.npz). */
int lc_project_points_f64(const double* points, int N, int H, int W, double fov_up_deg,
                          double fov_down_deg, double min_depth, double max_depth, uint64_t* zbuf,
                          int32_t* winner, float* image, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Points in rotated boxes: lidargen/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:128-168
 * (points_in_boxes_cpu: int32 [N_box, M] 0/1, MARGIN 1e-2) and
 * src/roiaware_pool3d_kernel.cu:23-36,313-336 (points_in_boxes_gpu: int32 [B, M] index of the
 * first containing box or -1, MARGIN 1e-5).  boxes [.., 7] = x,y,z,dx,dy,dz,heading.
 * The boxes of a block sit in LDS with their per-box constants (rotation, half extents): at most
 * 1250 boxes per call / per sample (LC_EUNSUP beyond; the reference's scenes hold tens).
 * ------------------------------------------------------------------------------------------- */
int lc_points_in_boxes_mask(const float* boxes, int n_boxes, const float* pts, int n_pts,
                            float margin, int32_t* out_mask, lc_stream_t s);
int lc_points_in_boxes_index(const float* boxes, const float* pts, int B, int n_boxes, int n_pts,
                             float margin, int32_t* out_idx, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Range-image pre/post-processing fused into single passes.
 * lc_range_postprocess: sample [B,2,H,W] in [-1,1] (depth, reflectance) -> out [B,5,H,W] =
 *   (metric depth, x, y, z, reflectance): LiDARUtility.denormalize / revert_depth / to_xyz
 *   (lidargen/utils/lidar.py:61-82,109-128) as chained in tools/evaluation/
 *   sample_and_save_cond.py:119-124.  ray_angles [1,2,H,W] (elevation, azimuth) radians.
 * lc_condition_preprocess: condition_mask [B,2,H,W] (class id, metric depth) -> out
 *   [B,num_classes+1,H,W] = one_hot(class) ++ LiDARUtility.convert_depth(depth)
 *   (sample_and_save_cond.py:106-117, utils/lidar.py:84-107).  The class id is truncated like .long(); an id outside
 *   [0, num_classes), which F.one_hot rejects, gives an all-zero one-hot.
 * depth_format: 0 log_depth, 1 inverse_depth, 2 depth.
 * ------------------------------------------------------------------------------------------- */
int lc_range_postprocess(const float* sample, int64_t sample_bs, const float* ray_angles,
                         float* out, int B, int H, int W, int depth_format, float min_depth,
                         float max_depth, lc_stream_t s);
int lc_condition_preprocess(const float* condition_mask, int64_t cm_bs, float* out, int64_t out_bs,
                            int B, int H, int W, int num_classes, int depth_format,
                            float min_depth, float max_depth, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Layout condition rasteriser (the step immediately before the path):
 * lidargen/dataset/transforms_3d/common.py:99-215 (convert_boxes_to_2d + convert_points_to_2d).
 * boxes [B,T,box_stride>=8] = (x,y,z,l,w,h,yaw,class,...), n_valid int32 [B] (first n rows used),
 * -> corners_2d [B,T,4] (x1,y1,x2,y2 normalised; zeros for padding rows; may be NULL),
 *    condition_mask [B,2,H,W] (class id, centre depth; later boxes overwrite earlier ones),
 *    loss_weight_map [B,H,W] (may be NULL).  scratch: lc_layout_scratch_bytes(B,T) bytes.
 * ------------------------------------------------------------------------------------------- */
int64_t lc_layout_scratch_bytes(int B, int T);
/* boxes_f64 = 0: float32 boxes (yaw cos/sin and centre depth in float32, like numpy on float32
 * input); 1: float64 boxes -- what NuscDataset.pre_process hands over (nuscenes_dataset.py:384-397)
 * -- everything in float64, the centre depth rounded to float32 when painted. */
int lc_layout_condition(const void* boxes, int boxes_f64, int box_stride, const int32_t* n_valid,
                        int B, int T, int H, int W, double fov_up_deg, double fov_down_deg,
                        void* scratch, float* corners_2d, float* condition_mask,
                        float* loss_weight_map, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * RoI-aware voxel pooling of point features: lidargen/ops/roiaware_pool3d/
 *   roiaware_pool3d_utils.py:55-107 (RoIAwarePool3dFunction) -> src/roiaware_pool3d.cpp:30-117
 *   (pybind forward / backward :173-174) -> src/roiaware_pool3d_kernel.cu:39-310.
 * rois [N,7], pts [P,3], pts_feature [P,C] -> pooled [N,X,Y,Z,C] (must be zero-filled by the
 * caller like the reference's new_zeros), pts_idx_of_voxels int32 [N,X,Y,Z,max_pts] (slot 0 =
 * count), argmax int32 [N,X,Y,Z,C] (max pooling).  pts_mask_scratch: int32 [N,P].
 * pool_method: 0 max, 1 avg.  Backward accumulates into grad_in [P,C] (zero-filled by the caller)
 * with atomicAdd, like the reference.
 * ------------------------------------------------------------------------------------------- */
int lc_roiaware_pool3d_fwd(const float* rois, const float* pts, const float* pts_feature,
                           int n_boxes, int n_pts, int channels, int out_x, int out_y, int out_z,
                           int max_pts_each_voxel, int pool_method, int32_t* pts_mask_scratch,
                           int32_t* pts_idx_of_voxels, int32_t* argmax, float* pooled,
                           lc_stream_t s);
int lc_roiaware_pool3d_bwd(const int32_t* pts_idx_of_voxels, const int32_t* argmax,
                           const float* grad_out, float* grad_in, int n_boxes, int channels,
                           int out_x, int out_y, int out_z, int max_pts_each_voxel,
                           int pool_method, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Point-set glue of the autoregressive (temporal) loop, SURVEY.md section 8(f)-2 -- keeps
 * tools/evaluation/sample_and_save_temporal.py:262-331 on the device between frames.
 * Points are [N,4] float32 rows (x, y, z, intensity), 16-byte aligned.
 *  lc_transform_points: out.xyz = T[0:3,0:3] p + T[0:3,3] (T row-major 4x4 of doubles on the HOST,
 *    product in fp64, rounded once), intensity copied: `(Ts @ homo_pts.T).T`
 *    tools/vis_tools/utils/pipe_related.py:245-249; warp_lidar_future common.py:59-112; the
 *    object <-> box-frame moves pipe_related.py:56-66,263-268 are the same op with another T.
 *  lc_image_to_points: xyz [3,H,W] (+reflectance [H,W]) -> rows, times the background mask
 *    !(cond[h,w] > 0) when cond != NULL; keep[i] = 0 for |xyz| <= min_norm (min_norm < 0: off)
 *    and for |x|,|y| < ego_radius (<= 0: off): pipe_related.py:68-75,274-283 and :11-13.
 *  lc_points_in_boxes_mask4: points_in_boxes_cpu on [N,4] rows; out_mask [n_boxes, N] and / or
 *    out_count [N] = number of boxes containing the point (delete_fg_points :266-272).
 *  lc_compact_points: out = rows[keep != 0] (or keep == 0 when keep_if_zero) in input order --
 *    numpy boolean indexing; count[0] = rows kept; src_index (may be NULL) = source row of each
 *    kept row; scratch = lc_compact_scratch_elems(N) int32.  Three launches, no host sync.
 * ------------------------------------------------------------------------------------------- */
int lc_transform_points(const float* pts, int N, const double* T16_host, float* out, lc_stream_t s);
/* float64 rows out [N,4] (32-byte aligned), NOT rounded: the reference keeps `(Ts @ homo_pts.T).T`
 * in float64 and projects it in float64 (pipe_related.py:245-257).  rot_f32 = 1: out.xyz =
 * (double)(float)(R p) + t, i.e. `rotate_points_along_z(p, yaw)` (float32 matmul,
 * lidargen/dataset/utils.py:37-59) `+ np.array([x, y, z])` (float64), pipe_related.py:263-266. */
int lc_transform_points_f64(const float* pts, int N, const double* T16_host, int rot_f32,
                            double* out, lc_stream_t s);
int lc_image_to_points(const float* xyz, int64_t plane_stride, const float* refl, const float* cond,
                       int H, int W, float refl_scale, float min_norm, float ego_radius, float* pts,
                       int32_t* keep, lc_stream_t s);
int lc_points_in_boxes_mask4(const float* boxes, int n_boxes, const float* pts4, int n_pts,
                             float margin, int32_t* out_mask, int32_t* out_count, lc_stream_t s);
int64_t lc_compact_scratch_elems(int N);
int lc_compact_points(const float* rows, const int32_t* keep, int N, int keep_if_zero, float* out,
                      int32_t* src_index, int32_t* count, int32_t* scratch, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * BEV metrics front-end, lidargen/metrics/bev.py (SURVEY.md section 8f-3 ii):
 *  lc_bev_histogram: point_cloud_to_histogram :5-24 -- rows with min_depth < |xyz| < max_depth are
 *    binned by (x, y) into hist[bx*bins + by] with torch.histogramdd's rule (edges [bins+1] as
 *    torch computes them, e[b] <= v < e[b+1], last bin right-inclusive); scratch = bins*bins int32.
 *  lc_rbf_kernel_sum: partials[] (lc_rbf_partials_elems doubles) whose sum is
 *    sum_ij exp(-gamma |p_i - q_j|^2), p [M,D], q [Mq,D] -- cdist_rbf(...).mean() * M * Mq of
 *    compute_mmd_2d :47-55.
 * ------------------------------------------------------------------------------------------- */
int lc_bev_histogram(const float* pts, int pt_stride, int N, const float* edges, int bins,
                     float min_depth, float max_depth, float* hist, int32_t* scratch, lc_stream_t s);
int64_t lc_rbf_partials_elems(int M, int Mq);
int lc_rbf_kernel_sum(const float* p, const float* q, int M, int Mq, int D, float gamma,
                      double* partials, lc_stream_t s);
/* Chamfer distance forward (lidargen/metrics/modules/chamfer3D/chamfer3D.cu:12-155 via
 * dist_chamfer_3D.py:27-49): xyz1 [B,N,3], xyz2 [B,M,3] -> squared distance to and index of the
 * nearest point of the other set, both directions; first minimum wins. */
int lc_chamfer3d_fwd(const float* xyz1, const float* xyz2, int B, int N, int M, float* dist1,
                     int32_t* idx1, float* dist2, int32_t* idx2, lc_stream_t s);
/* The 2-D variant (lidargen/metrics/modules/chamfer2D/chamfer2D.cu NmDistanceKernel): xyz1 [B,N,2], xyz2 [B,M,2];
 * d = dx*dx + dy*dy with separate float32 roundings, first minimum wins.  B <= 65535 (LC_EUNSUP otherwise). */
int lc_chamfer2d_fwd(const float* xyz1, const float* xyz2, int B, int N, int M, float* dist1,
                     int32_t* idx1, float* dist2, int32_t* idx2, lc_stream_t s);
/* Chamfer distance backward (chamfer3D.cu:155-195 NmDistanceGradKernel, chamfer2D.cu:145-171; csrc/chamfer_bwd.hip,
 * DESIGN.md section 5v): xyz1 [B,N,D], xyz2 [B,M,D], grad_dist1 [B,N], grad_dist2 [B,M], idx1 [B,N], idx2 [B,M] as the
 * forward writes them -> grad_xyz1 [B,N,D], grad_xyz2 [B,M,D], D = 3 / 2.  Terms g = grad * 2, t = g * (own - other), each
 * operation rounded to float32; no float atomics: row j of grad_xyz1 = (+0 + its direct term) + the terms
 * -(2 grad_dist2[k] (xyz2[k] - xyz1[j])) of the k with idx2[k] == j in ascending k (more than 32 of them: 256 strided lane
 * sums and a halving tree, csrc/chamfer_bwd.hip); grad_xyz2 likewise.  An index outside its cloud adds no term.  The table
 * of the k of every j is built on the device in `scratch` (lc_chamfer_bwd_scratch_bytes(B, N, M) bytes, 0 for sizes the
 * entries refuse): one stable radix sort of the B (N + M) indices and a binary search per row, no host read.
 * Any B (also for D = 2); B (N + M) < 2^31 - 1 (LC_EUNSUP otherwise). */
int64_t lc_chamfer_bwd_scratch_bytes(int B, int N, int M);
int lc_chamfer3d_bwd(const float* xyz1, const float* xyz2, const float* grad_dist1, const float* grad_dist2,
                     const int32_t* idx1, const int32_t* idx2, int B, int N, int M, float* grad_xyz1, float* grad_xyz2,
                     void* scratch, lc_stream_t s);
int lc_chamfer2d_bwd(const float* xyz1, const float* xyz2, const float* grad_dist1, const float* grad_dist2,
                     const int32_t* idx1, const int32_t* idx2, int B, int N, int M, float* grad_xyz1, float* grad_xyz2,
                     void* scratch, lc_stream_t s);
/* Chamfer distance of BEV cell sets on their nx x ny grid (csrc/bev_chamfer.hip).
 * lc_bev_grid_supported: LC_OK when the distance transform takes the grid; LC_EINVAL for a non-positive size; LC_EUNSUP
 *   when 2 nx^2 ny^2 >= 2^32 (the u32 distances would overflow) or a 64-column strip of it does not fit 64 KiB of LDS.
 * lc_bev_occupancy_bits: clouds (float32 points `pt_stride` floats apart, x / y first; cloud c is points offsets[c] ..
 *   offsets[c+1], max_points the longest) -> bits [n_clouds][nx][ceil(ny/32)] (bit iy & 31 of word iy >> 5 of row ix; mask
 *   and floor of lc_bev_occupancy_accumulate) and counts[c], the number of cells of cloud c.  Any grid.
 * lc_bev_cell_lists: cells[cell_offsets[c] .. cell_offsets[c+1]) = ix * ny + iy of the set bits of cloud c, ascending;
 *   cell_offsets is the exclusive prefix sum of counts.
 * lc_bev_distance_transform: Dt[cell * ld + m] = min over the cells c' of bitmap m of (di^2 ny^2 + dj^2 nx^2), 0xFFFFFFFF
 *   for an empty bitmap; columns n_maps .. ld are zeroed.  tmp: n_maps * nx * ny words.  n_maps <= 65535.
 * lc_bev_pair_sums: A[i * nJ + j] = sum over the cells of list i (cell_offsets[i] .. cell_offsets[i+1]) of Dt[cell * ld + j].
 *   nI <= 65535.
 * lc_bev_chamfer_combine: cd[i][j] = (A_rs[i*nJ+j] / count_r[i] + A_sr[j*nI+i] / count_s[j]) / (2 nx^2 ny^2) in float64;
 *   matrix (may be NULL) [i * matrix_ld + j0 + j] = cd; the row minimum and j0 + its first arg-minimum replace
 *   min_out[i] / argmin_out[i] when `first` or when the minimum is smaller (chunks in ascending j0: first index wins). */
int lc_bev_grid_supported(int nx, int ny);
int lc_bev_occupancy_bits(const float* pts, int pt_stride, const int64_t* offsets, int n_clouds, int64_t max_points,
                          float x0, float x1, float y0, float y1, float voxel, int min_bound_x, int min_bound_y,
                          int nx, int ny, uint32_t* bits, int32_t* counts, lc_stream_t s);
int lc_bev_cell_lists(const uint32_t* bits, int n_clouds, int nx, int ny, const int64_t* cell_offsets,
                      int32_t* cells, lc_stream_t s);
int lc_bev_distance_transform(const uint32_t* bits, int n_maps, int nx, int ny, uint32_t* tmp, uint32_t* Dt,
                              int ld, lc_stream_t s);
int lc_bev_pair_sums(const int32_t* cells, const int64_t* cell_offsets, int nI, const uint32_t* Dt, int ld,
                     int nJ, uint64_t* A, lc_stream_t s);
int lc_bev_chamfer_combine(const uint64_t* A_rs, const uint64_t* A_sr, const int32_t* count_r,
                           const int32_t* count_s, int nI, int nJ, int64_t j0, int first, int nx, int ny,
                           double* min_out, int64_t* argmin_out, double* matrix, int64_t matrix_ld, lc_stream_t s);
/* Earth Mover's Distance by the auction algorithm, forward (lidargen/metrics/modules/emd/emd_cuda.cu emd_cuda_forward
 * with the state of emd_module.py:59-70; csrc/emd.hip): xyz1, xyz2 [B,n,3] -> assignment [B,n]
 * (the object of xyz2 each point of xyz1 holds after `iters` iterations; the last one gives every unassigned point its
 * own bid, so objects may repeat) and dist [B,n] = |xyz1[j] - xyz2[assignment[j]]|^2.  Any n >= 1 (<= 2^24), B >= 1
 * (<= 65535), iters >= 1, eps >= 0.  All state lives in `scratch` (lc_emd_scratch_bytes(B, n) bytes, 16-byte aligned)
 * and is initialised by every call; no host synchronisation.  target_blocks: blocks per pair the bid pass spreads over,
 * 0 = auto (max(64, 2048 / B)), otherwise 1 ... auto (tests: it moves the thresholds between the pass's splits). */
int64_t lc_emd_scratch_bytes(int B, int n);
int lc_emd_fwd(const float* xyz1, const float* xyz2, int B, int n, float eps, int iters, int target_blocks,
               float* dist, int32_t* assignment, void* scratch, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Scene-graph layout generator (lidargen/models/unets/unet_1d.py UNet1DModel on a signal of length 1, graph.py
 * GraphTripleConv): skinny dense layers on row-major activations, csrc/layout_gen.hip, DESIGN.md section 5h.
 *
 * lc_row_segment: `width` columns of a gathered activation matrix; row m of the matrix reads row idx[m] (m when idx is
 *   NULL) of p, rows `ld` floats apart.  Up to three segments side by side make the K axis ([s | p | o] rows of a
 *   triple, [h | skip]).  The entry points do NOT check index VALUES (idx[], vec_row[], slots[], row_ptr[]): the caller
 *   guarantees that every one names a row of its tensor (unet_1d._Plan checks them on the host, once per call).
 * lc_skinny_gemm_fwd: parts[c][m][n] = sum over chunk c of X[m,k] w[n,k] (w in nn.Linear layout [N, K], fp32 FMA).
 *   K is summed in chunks of 128 in ascending order; nparts = lc_skinny_parts(M, N, K) is either the chunk count (every
 *   chunk a block of its own: the weight stream spreads over the chip) or 1 (the block adds the chunk sums itself, in
 *   the same order).  Both forms give the same bits, for every M.
 * lc_skinny_combine_fwd: y[m,n] = act(sum_c parts[c][m][n] + bias[n]) + vec[vec_row[m]][n] + res[m][n];
 *   act 0 none, 1 ReLU, 2 GEGLU (N even, y has N/2 columns: a * gelu(gate), gate = columns N/2 ...).  bias, vec, res may
 *   be NULL; vec_row NULL reads row 0 of vec for every m.
 * lc_rowprep_fwd: y[m, :C] = [SiLU](norm(row m of the segments)); G > 0: statistics over G groups of C / G columns
 *   (GroupNorm on [M, C, 1]; G = 1: LayerNorm), biased variance, affine gamma / beta (NULL: none); G = 0: no norm
 *   (a plain gathered concatenation when silu is 0 too).  C <= 4096.
 * lc_graph_pool_fwd: y[o, :H] = (sum over slots[row_ptr[o] .. row_ptr[o+1]) of t[slot >> 1, (slot & 1 ? o_col : s_col) + h])
 *   / max(count, 1), summed in the order of slots[] -- no atomics, the result does not depend on scheduling.
 * lc_time_embed_fwd: y[u] = [cos(t[u] freqs) | sin(t[u] freqs)], freqs [half] (nn.py timestep_embedding).
 * ------------------------------------------------------------------------------------------- */
typedef struct lc_row_segment {
    const float* p;
    const int32_t* idx;
    int64_t ld;
    int32_t width;
} lc_row_segment;
int64_t lc_skinny_parts(int M, int N, int K);
int lc_skinny_gemm_fwd(const lc_row_segment* segs, int nseg, const float* w, float* parts, int M, int N, int K,
                       int nparts, lc_stream_t s);
int lc_skinny_combine_fwd(const float* parts, int nparts, const float* bias, int act, const float* vec, int64_t vec_ld,
                          const int32_t* vec_row, const float* res, int64_t res_ld, float* y, int64_t y_ld, int M, int N,
                          lc_stream_t s);
int lc_rowprep_fwd(const lc_row_segment* segs, int nseg, float* y, int64_t y_ld, int M, int C, int G, float eps,
                   const float* gamma, const float* beta, int silu, lc_stream_t s);
int lc_graph_pool_fwd(const float* t, int64_t t_ld, int s_col, int o_col, const int32_t* row_ptr, const int32_t* slots,
                      float* y, int64_t y_ld, int O, int H, lc_stream_t s);
int lc_time_embed_fwd(const float* t, const float* freqs, float* y, int U, int half, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Fused PointNet trunk (lidargen/metrics/extractor/pointnet.py: the per-point MLP 3 -> 64 -> 128 -> 1024 and the max
 * over the points of STN3d and PointNetfeat; csrc/pointnet.hip).  BatchNorm is folded into
 * (w, b) by the caller, its scale included (a negative scale does not commute with the max).
 *   x [B,3,N] channel-major, clouds x_bs floats apart; trans [B,9] row-major 3x3 or NULL: p' = p^T trans[b];
 *   h1 = relu(w1 p' + b1), h2 = relu(w2 h1 + b2), y[b,c] = max over the N points of (w3 h2 + b3)[c], ReLU on y when
 *   relu3; w1 [64,3], w2 [128,64], w3 [1024,128] row-major (w2, w3 16-byte aligned), rows of y y_bs floats apart.
 * Exact fp32 (f32-input MFMA).  Every point counts, (0,0,0) too.  Finite inputs (a NaN activation is dropped by the max,
 * not propagated).  scratch: lc_pointnet_trunk_scratch_elems(B, N) floats, every word read is written by the same call.
 * No atomics; a cloud's result does not depend on the batch it is in.  B <= 65535, N < 2^24. */
int64_t lc_pointnet_trunk_scratch_elems(int B, int N);
int lc_pointnet_trunk_fwd(const float* x, int64_t x_bs, const float* trans, const float* w1, const float* b1,
                          const float* w2, const float* b2, const float* w3, const float* b3, int relu3, float* y,
                          int64_t y_bs, int B, int N, float* scratch, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Sparse 3-D convolution (csrc/spconv.hip): what the MinkUNet of the Frechet Sparse Volume Distance
 * (lidargen/metrics/models/minkowskinet/model.py) takes from torchsparse 1.4.0.  A sparse tensor at stride s is rows
 * F [N, C] over coordinates [N, 4] int32 = (x, y, z, batch), spatial entries multiples of s and unique rows.
 * Limits (LC_EUNSUP beyond them, before any launch): 0 <= x, y, z <= LC_SPCONV_MAX_COORD, 0 <= batch <=
 * LC_SPCONV_MAX_BATCH, stride <= LC_SPCONV_MAX_STRIDE, rows <= LC_SPCONV_MAX_ROWS.  The coordinates live on the device:
 * the caller states `max_coord` (the largest spatial entry) and `n_batch`; a row outside the limits all the same is never
 * inserted and never found.  A query at C + offset outside [0, LC_SPCONV_MAX_COORD] is absent: it never aliases another
 * batch's voxel and never wraps.
 *   lc_spconv_hash_build: table (lc_spconv_hash_bytes(N) bytes, 8-byte aligned) <- the rows of coords.  The table's bytes
 *     are a function of the rows alone (of equal rows the last one is found): the same for every run.
 *   lc_spconv_map: nbr [M, K] int32 <- for every row of coords [M, 4] the table row at coords + offset_k, -1 when absent;
 *     `table` built from n_table rows.  kind 0: K = 27, offsets {-stride, 0, stride}^3, k = ix + 3 iy + 9 iz.
 *     kind 1: K = 8, offsets {0, stride}^3, k = 4 ix + 2 iy + iz (coords coarse at 2 stride, table fine at stride).
 *     kind 2: K = 8, the transpose of kind 1 (coords fine at stride, table coarse at 2 stride): entry k of a row is the
 *     coarse row j with coords = coarse[j] + offset_k, one k per row at the most.
 *   lc_spconv_fwd: y[j, y_col : y_col + Co] = act(sum_k x[nbr[j,k], :] w[k] + b + res[j, :Co]) for j < M; x rows ldx floats
 *     apart (n_in of them), w [K, Ci, Co], b [Co] or NULL, res rows ldr apart or NULL, y rows ldy apart; relu != 0: ReLU.
 *     K in {1, 8, 27}; K = 1 with nbr NULL is the dense product x w.  An entry -1 (or outside [0, n_in)) adds zeros and
 *     reads nothing.  Ci in {4, 16, 32, 48, 64, 96, 128, 192}, Co in {16, 32, 48, 64, 128} (LC_EUNSUP otherwise); ldx, ldr,
 *     ldy, y_col multiples of 4 and every pointer 16-byte aligned (LC_EUNSUP).  Exact fp32 (f32-input MFMA), no atomics,
 *     a row's bits depend on its own neighbours only.  y may not overlap x or res.
 *   lc_spconv_sector_means: out [n_clouds, 16 C] <- per cloud (rows offsets[c] .. offsets[c+1] of f / coords; offsets a
 *     device int32 [n_clouds + 1]) and depth sector i the mean of the rows with edges[i] <= d < edges[i+1], d = |xyz -
 *     mean xyz| * voxel in float32, edges a device float [17]; 0 for an empty sector.  C <= 256, n_clouds <= 65535.
 *     Fixed summation order, no atomics. */
#define LC_SPCONV_TILE 64
#define LC_SPCONV_MAX_COORD 262143
#define LC_SPCONV_MAX_BATCH 510
#define LC_SPCONV_MAX_STRIDE 65536
#define LC_SPCONV_MAX_ROWS 67108864
int64_t lc_spconv_hash_bytes(int N);
int lc_spconv_hash_build(const int32_t* coords, int N, int max_coord, int n_batch, void* table, int64_t table_bytes,
                         lc_stream_t s);
int lc_spconv_map(const int32_t* coords, int M, int kind, int stride, const void* table, int n_table, int32_t* nbr,
                  lc_stream_t s);
int lc_spconv_fwd(const float* x, int64_t ldx, const int32_t* nbr, int n_in, const float* w, const float* b,
                  const float* res, int64_t ldr, float* y, int64_t ldy, int y_col, int M, int Ci, int Co, int K, int relu,
                  lc_stream_t s);
int lc_spconv_sector_means(const float* f, int64_t ldf, const int32_t* coords, const int32_t* offsets, int n_clouds,
                           int C, const float* edges, float voxel, float* out, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Point <-> voxel exchanges (csrc/spvoxel.hip): what the SPVCNN of the Frechet Point-Voxel Distance
 * (lidargen/metrics/models/spvcnn/model.py) takes from torchsparse 1.4.0 (sphashquery, calc_ti_weights, spdevoxelize,
 * spvoxelize).  Points are rows (x, y, z, batch) of floats; a level is the lc_spconv_hash_build table of its coordinates.
 * Limits as above (LC_EUNSUP); rows <= LC_SPCONV_MAX_ROWS.  No atomics anywhere: the same bits every run, and a point's or
 * a voxel's bits depend on its own neighbours / points only.
 *   lc_spvox_query: for every point the eight voxels base + {0, stride}^3, base = floor(p / stride) * stride, in the
 *     point's own batch: idx [N, 8] int32, k = 4 ix + 2 iy + iz (kind 1 of lc_spconv_map), -1 when absent; a probe with a
 *     component outside [0, LC_SPCONV_MAX_COORD] (or a point that is not finite) is absent before a key is formed.
 *     w [N, 8] or NULL (idx only): a = (base + stride) - p on an axis with offset 0, p - base with offset stride;
 *     w_k = ((a_x a_y) a_z) / stride^3, 0 where idx is -1, then w_k / (S + 1e-8) with S = ((((((w_0 + w_1) + w_2) + w_3)
 *     + w_4) + w_5) + w_6) + w_7, every operation rounded once to float32.  A point without a neighbour gets zeros.
 *     stride a power of two (LC_EUNSUP otherwise: the base is exact); pts, idx, w 16-byte aligned.
 *   lc_spvox_devoxelize: out[i, :C] = (sum over k ascending with idx[i, k] in [0, n_rows) of w[i, k] f[idx[i, k], :C], an
 *     fma chain from 0) + addend[i, :C]; f rows ldf floats apart (n_rows of them), addend rows lda apart or NULL, out rows
 *     ldo apart.  An entry -1 or outside [0, n_rows) reads nothing and adds nothing.  addend may be out itself; out may not
 *     overlap f.  C in {16, 48, 64, 128}; ldf, lda, ldo multiples of 4 and f, addend, out 16-byte aligned (LC_EUNSUP).
 *   lc_spvox_voxelize: out[v, :C] = sum over j = offsets[v] .. offsets[v + 1] - 1 ascending of f[perm[j], :C] / (offsets[v
 *     + 1] - offsets[v]), each term divided and then added to the running sum, which starts at 0: with perm the points in
 *     voxel order (a stable sort of their voxel) the mean of a voxel's points added in ascending point order.  offsets a
 *     device int32 [V + 1] into perm [n_perm]; a voxel without points gives zeros; an entry of perm outside [0, n_rows) adds
 *     nothing.  C in {4, 16, 64, 128}. */
int lc_spvox_query(const float* pts, int N, int stride, const void* table, int n_table, int32_t* idx, float* w,
                   lc_stream_t s);
int lc_spvox_devoxelize(const float* f, int64_t ldf, int n_rows, const int32_t* idx, const float* w, const float* addend,
                        int64_t lda, float* out, int64_t ldo, int N, int C, lc_stream_t s);
int lc_spvox_voxelize(const float* f, int64_t ldf, int n_rows, const int32_t* perm, int n_perm, const int32_t* offsets,
                      int V, float* out, int64_t ldo, int C, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Dense convolutions of RangeNet-53 / -21 (csrc/rangenet.hip): the extractor of the Frechet Range
 * Image Distance (lidargen/metrics/models/rangenet/model.py) and of FRD (lidargen/metrics/extractor/rangenet.py).
 * Contiguous float32 NCHW tensors, zero padding, exact fp32 on the f32-input MFMA, no atomics; a sample's bits do not depend
 * on the batch it is in.
 *   mode 0: 1x1            mode 1: 3x3, padding (1,1)            mode 2: 3x3, stride (1,2), padding (1,1), W_out = (W-1)/2+1
 *   mode 3: transposed 1x4, stride (1,2), padding (0,1), W_out = 2 W: output column 2j = w[1] x[j] + w[3] x[j-1], column
 *           2j+1 = w[2] x[j] + w[0] x[j+1]
 *   y = acc + bias[co]; act: y = y > 0 ? y : 0.1f y; y += res1; y += res2 (res1, res2 [B,Co,H,W_out] or NULL).
 *   k order: input channels in chunks of 16 (mode 0: 32) ascending, inside a chunk tap ascending (ky*3+kx; mode 3: 1, 3, 2,
 *   0), inside a tap channel ascending; every chunk is an fma chain from zero, the chunks are added in ascending order.
 * lc_rangenet_pack_weight works on HOST memory: w [Co,Ci,kh,kw] (mode 3: [Ci,Co,1,4]) -> out,
 * lc_rangenet_packed_weight_elems(mode, Ci, Co) floats (0 for arguments it does not take), zero-filled past Ci and Co.
 * wpk must be 16-byte aligned (LC_EUNSUP); y may not alias x, res1 or res2 (LC_EINVAL); B * ceil(Co / 128) <= 65535 and
 * H <= 131070 (LC_EUNSUP).  lc_rangenet_tile_extent(i): 0 pixels per wave, 1 rows per block, 2 channels per wave, 3 the
 * widest block row in pixels (Co <= 32).
 *   lc_rangenet_reduce_fwd: kind 0 out[b, c] = mean over the map; 1 out[b, 16 c + n] = mean over all rows and columns
 *   n W/16 .. (n+1) W/16 - 1 (W % 16 == 0, LC_EUNSUP otherwise); 2 the same over rows n H/16 .. (H % 16 == 0).  One wave per
 *   output, lane-strided partial sums then a butterfly: a fixed order. */
int lc_rangenet_tile_extent(int which);
int64_t lc_rangenet_packed_weight_elems(int mode, int Ci, int Co);
int lc_rangenet_pack_weight(const float* w, int mode, int Ci, int Co, float* out);
int lc_rangenet_conv_fwd(const float* x, const float* wpk, const float* bias, const float* res1, const float* res2, float* y,
                         int B, int Ci, int Co, int H, int W, int mode, int act, lc_stream_t s);
int lc_rangenet_reduce_fwd(const float* x, float* out, int B, int C, int H, int W, int kind, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * PointMLP object extractor (csrc/pointmlp.hip): farthest point sampling, k nearest neighbours, the
 * grouped and normalised operand of a stage, dense layers on [B, C, L] and the maximum over groups of columns.  Contiguous
 * float32 / int32 tensors; no atomics, every reduction in a fixed order, a cloud's bits do not depend on the batch it is
 * in; every entry checks its arguments before any launch.
 *   lc_fps_fwd: xyz [B,N,3] (finite) -> idx [B,M], the greedy farthest-point sequence from index 0: running distances
 *     start at 1e10, d = (dx dx + dy dy) + dz dz in float32 with separately rounded operations, among equal maxima the
 *     smallest (rev(k mod bs), k) wins, bs = the largest power of two <= min(N, 1024) and rev the bit reversal over log2 bs
 *     bits (the reference kernel's strided scan and reduction tree).  M may exceed the number of distinct points (index 0
 *     repeats).  N <= LC_FPS_MAX_N (LC_EUNSUP above).
 *   lc_knn_fwd: query_idx [B,S] indexes xyz [B,N,3]; out [B,S,K] = the K points nearest to each query, the same distance
 *     expression, ascending (distance, index).  1 <= K <= min(N, LC_KNN_MAX_K) (K > N: LC_EINVAL), N <= LC_KNN_MAX_N,
 *     B <= 65535.  A query index outside [0, N) gives a row of -1.
 *   lc_pointmlp_group_fwd: x [B,d,N], fps_idx [B,S], knn_idx [B,S,K] (indices are clamped into [0, N)) ->
 *     out [B,2d,S K]: out[b,c,sK+k] = alpha[c] (x[b,c,knn] - x[b,c,fps[s]]) / (sigma_b + 1e-5) + beta[c],
 *     out[b,d+c,sK+k] = x[b,c,fps[s]]; sigma_b the UNBIASED standard deviation over all S K d differences of cloud b (float64
 *     two-level sum; sigma [B] receives it when not NULL).  scratch: lc_pointmlp_group_scratch_elems(B,S,K) doubles, written
 *     before they are read by the same call.  S K d >= 2 (LC_EINVAL).
 *   lc_pointmlp_conv_fwd: y [B,Co,L] = act(W x + bias (+ res)), x [B,Ci,L], res [B,Co,L] or NULL added BEFORE the
 *     activation, act 1 = ReLU, 0 = none.  Exact fp32 on the f32-input MFMA; k order: input channels in chunks of 32
 *     ascending, every chunk an fma chain from zero, the chunks added in ascending order.  wpk: the device copy of
 *     lc_pointmlp_pack_weight (HOST memory: w [Co,Ci] -> lc_pointmlp_packed_weight_elems(Ci,Co) floats, zero-filled past Ci and
 *     Co; any positive widths), 16-byte aligned (LC_EUNSUP).  y may not alias x or res (LC_EINVAL).
 *   lc_pointmlp_groupmax_fwd: x [B,C,G K] -> out[b out_bs + c out_cs + g out_gs] = max over k of x[b,c,gK+k].
 *   lc_pointmlp_limit(i): 0 LC_FPS_MAX_N, 1 LC_KNN_MAX_N, 2 LC_KNN_MAX_K, 3 channels per chunk, 4 output channels per wave,
 *     5 columns per wave, 6 columns per grouping block. */
#define LC_FPS_MAX_N 8192
#define LC_KNN_MAX_N 8192
#define LC_KNN_MAX_K 32
int lc_pointmlp_limit(int which);
int lc_fps_fwd(const float* xyz, int* idx, int B, int N, int M, lc_stream_t s);
/* one cloud xyz [N,3] of a stacked batch: the same kernel with the tie rule of a 1024-thread block whatever N is (the
 * reference's stack_farthest_point_sampling_kernel; lc_fps_fwd's rule for N >= 1024), idx [M] = the picks + off. */
int lc_fps_stack_fwd(const float* xyz, int* idx, int N, int M, int off, lc_stream_t s);
int lc_knn_fwd(const float* xyz, const int* query_idx, int* out, int B, int N, int S, int K, lc_stream_t s);
int64_t lc_pointmlp_group_scratch_elems(int B, int S, int K);
int lc_pointmlp_group_fwd(const float* x, const int* fps_idx, const int* knn_idx, const float* alpha, const float* beta,
                          float* out, double* scratch, float* sigma, int B, int d, int N, int S, int K, lc_stream_t s);
int64_t lc_pointmlp_packed_weight_elems(int Ci, int Co);
int lc_pointmlp_pack_weight(const float* w, int Ci, int Co, float* out);
int lc_pointmlp_conv_fwd(const float* x, const float* wpk, const float* bias, const float* res, float* y, int B, int Ci,
                         int Co, int L, int act, lc_stream_t s);
int lc_pointmlp_groupmax_fwd(const float* x, float* out, int B, int C, int G, int K, int64_t out_bs, int64_t out_cs,
                             int64_t out_gs, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Radius-limited nearest neighbour and point-to-point ICP on a ragged batch of float64 clouds (csrc/icp.hip, DESIGN.md
 * section 5p): the registration of the temporal metric TTCE (lidargen/metrics/temporal.py estimate_transform_icp, i.e.
 * Open3D registration_icp with TransformationEstimationPointToPoint and default criteria, restated).
 * Operands: points [total,3] float64 (finite), offsets [C+1] int32 (cloud c owns rows offsets[c] ... offsets[c+1]-1), pairs
 * [P,2] int32 (source cloud, target cloud), T [P,4,4] float64 row-major -- all DEVICE memory; max_cloud / max_src: an upper
 * bound of the largest cloud / the largest source cloud (it sizes the launches; a larger cloud is not registered).
 * Offsets or pair entries that do not describe rows of `points` make an empty cloud, never an access outside the operands.
 *   lc_nn_grid_build: the search structure of EVERY cloud, once: a grid of cubic cells over the cloud's bounding box, edge h0
 *     doubled until the grid has at most 2^20 cells (histogram, exclusive scan, scatter).  grid: lc_nn_grid_bytes(C, total)
 *     bytes, 16-byte aligned (0: C > 65535 or total beyond 32-bit element offsets).  Any h0 > 0 gives the same results.
 *   lc_nn_radius: one correspondence pass.  For source point i of pair p: q = T[p] points[i] (float64, no contraction),
 *     idx[p*max_src+i] = the target point of the smallest d2 = (dx dx + dy dy) + dz dz among those with d2 <= radius^2, the
 *     SMALLEST index among equal minima (whatever the order inside a cell), -1 if none; d2[p*max_src+i] that distance (+inf
 *     if none).  Entries past a pair's source size are not written.
 *   lc_icp_run: T (in: the initial transforms, out: the result) <- the ICP loop: pass; for i < max_iteration { update =
 *     the rigid least-squares fit of the current correspondences (Umeyama without scale; computed as Horn's quaternion, the
 *     same optimum; identity without correspondences); T = update T; pass; stop when |d fitness| < relative_fitness and
 *     |d rmse| < relative_rmse }.  fitness [P] = correspondences / source points, inlier_rmse [P] = sqrt(sum d2 /
 *     correspondences) (0 without), iterations [P] = updates applied.  T is always applied to the original source points.
 *     2 max_iteration + 3 launches, no host synchronisation; the kernels of a finished pair return at once.  Sums are
 *     float64 partials per 256-point block added in block order: no float atomics, the bits of a pair are the same in every
 *     run and in every batch.  scratch: lc_icp_scratch_bytes(P, max_src) bytes, 16-byte aligned, initialised by the call.
 * P <= 65535 and C <= 65535 (LC_EUNSUP above, before any launch); null pointers, sizes < 1, radius or h0 not positive and
 * finite: LC_EINVAL. */
int64_t lc_nn_grid_bytes(int C, int64_t total);
int lc_nn_grid_build(const double* points, const int32_t* offsets, int C, int64_t total, int max_cloud, double h0, void* grid,
                     lc_stream_t s);
int lc_nn_radius(const double* points, const int32_t* offsets, int C, int64_t total, const void* grid, const int32_t* pairs,
                 const double* T, int P, int max_src, double radius, int32_t* idx, double* d2, lc_stream_t s);
int64_t lc_icp_scratch_bytes(int P, int max_src);
int lc_icp_run(const double* points, const int32_t* offsets, int C, int64_t total, const void* grid, const int32_t* pairs,
               int P, int max_src, double radius, int max_iteration, double relative_fitness, double relative_rmse, double* T,
               double* fitness, double* inlier_rmse, int32_t* iterations, void* scratch, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * GLENet box sampler and rotated IoU of the RGF object metric (csrc/glenet.hip): the reference's
 * lidargen/metrics/models/glenet/{point_net,model,loss_utils}.py and eval_utils/eval_utils.py.  DEVICE memory, contiguous
 * float32 / int32 (variance, mean_overlap: float64); no atomics, an object's / a row's / a pair's bits depend on its own
 * operands only.  Null pointers and sizes < 1: LC_EINVAL before any launch.
 * A ragged batch: points [total,3], offsets [B+1] int32, object b owns rows offsets[b] ... offsets[b+1]-1; offsets that do
 * not describe rows of `points` make an empty object, never an access outside the operand.  total < 2^31 (LC_EUNSUP).
 *   lc_segment_center_fwd: mean [B,3] = float32(sum in float64 / n) per object (per-thread strided partial sums, a fixed tree;
 *     0 for an empty object); out[i] = float32((double)(p[i] - mean) / (sx, sy, sz)), the difference in float32.  Scales > 0.
 *   lc_glenet_trunk_fwd: rows r < R, object b = r mod B (a [D,B] grid of draws and objects, R = D B).  Row r reads its K
 *     points as norm[offsets[b] + choice[r K + j]] (an index is clamped into the object's range; an empty object reads
 *     zeros).  featA [512,R] = max over the K points of w3 relu(w2 relu(w1 p + b1) + b2) + b3 (PointNetfeat's trunk, w1
 *     [64,3], w2 [128,64], w3 [512,128] row-major, w2 / w3 16-byte aligned, BatchNorm folded by the caller, scale included);
 *     featS [8,R] the same for SimPointNetfeat's 3 -> 8 -> 8 -> 8 (sw1 [8,3], sw2, sw3 [8,8]), every output an fma chain over
 *     ascending input channel from the bias.  Both CHANNEL-MAJOR: the [1,C,R] operand of lc_pointmlp_conv_fwd.  Exact fp32
 *     on the f32-input MFMA in the k order of lc_pointnet_trunk_fwd; tails past K masked with -inf.  Any K >= 1 (< 2^24),
 *     any R < 2^31: the row is the block index.
 *   lc_rbox_inter_fwd: corners_g, corners_q [N,8] (x0 y0 ... x3 y3) -> pts [N,16] (the vertices in the order compute_vertex
 *     finds them: corners of g inside q -- with the extra test adad > 0 and abab > 0 --, corners of q inside g, edge i of g
 *     against edge j of q row-major; a ninth vertex is skipped; zeros past cnt), cnt [N], area [N] (sort_vertex: descending
 *     angle in [0, 2 * 3.1415926) about the float32 centroid, stable, unused slots as angle 0, the angle a float64 atan2
 *     rounded to float32; area_polygon: a fan from the first sorted vertex, abs per triangle).  One thread per pair, every
 *     float32 operation rounded on its own (no contraction).  The reference's quirks are kept: two identical boxes give 0.
 *   lc_riou3d_paired_fwd: boxes (x, y, z, dx, dy, dz, ry) in the first 7 of ldg / ldq (>= 7) columns: clamp to +-200,
 *     rbbox_to_corners, the intersection above, the height overlap, inter / (vol_g + vol_q - inter) -> iou [N].
 *   lc_glenet_score_fwd: box [D,B,9] (the sampler's output), gt [B,7], both normalised.  Decode: centres times (diag, diag,
 *     dza) -- diag a float64 factor, the product rounded once --, sizes exp(.) times (dxa, dya, dza); pred [D,B,9] the decoded
 *     box (columns 7, 8 copied), overlap [D,B] = the paired IoU of the decoded gt and draw.  Then in draw order and float64:
 *     variance [B,7] the population variance over the draws of columns 0..5 and of sin(w - floor(w / 2 pi) 2 pi), w = ry -
 *     gt ry; mean_overlap [B].  One wave per object, lane = draw (any D). */
int lc_segment_center_fwd(const float* points, const int32_t* offsets, int B, int64_t total, double sx, double sy, double sz,
                          float* out, float* mean, lc_stream_t s);
int lc_glenet_trunk_fwd(const float* norm, int64_t total, const int32_t* offsets, const int32_t* choice, int B, int K,
                        int64_t R, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                        const float* b3, const float* sw1, const float* sb1, const float* sw2, const float* sb2,
                        const float* sw3, const float* sb3, float* featA, float* featS, lc_stream_t s);
int lc_rbox_inter_fwd(const float* corners_g, const float* corners_q, int N, float* pts, int32_t* cnt, float* area,
                      lc_stream_t s);
int lc_riou3d_paired_fwd(const float* g, int ldg, const float* q, int ldq, int N, float* iou, lc_stream_t s);
int lc_glenet_score_fwd(const float* box, const float* gt, int D, int B, double diag, float dxa, float dya, float dza,
                        float* pred, float* overlap, double* variance, double* mean_overlap, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Rotated BEV overlap / IoU, 3-D IoU and NMS of lidargen.ops.iou3d_nms (csrc/iou3d_nms.hip over the geometry of
 * csrc/iou3d_box.h): the reference's lidargen/ops/iou3d_nms.  Boxes are contiguous float32 rows
 * [x, y, z, dx, dy, dz, heading] in DEVICE memory (the two *_host entries: HOST memory, no GPU touched).  Every entry checks
 * its arguments before any launch: null pointers and negative counts LC_EINVAL; a count of 0 returns LC_OK with nothing
 * launched and nothing dereferenced beyond the null checks.  No contraction into fused multiply-adds anywhere; a pair's
 * bits depend on its two rows only.  The geometry is not the GLENet metric's (lc_riou3d_paired_fwd): two identical boxes
 * overlap in their whole area here.
 *   mode: 0 the BEV overlap area, 1 the BEV IoU overlap / max(sa + sb - overlap, 1e-8), 2 the 3-D IoU: with
 *     h = clamp(min(za + dza/2, zb + dzb/2) - max(za - dza/2, zb - dzb/2), min=0), o3 = overlap * h and v = dx * dy * dz
 *     (left to right): o3 / clamp(va + vb - o3, min=1e-6), every operation rounded to float32 on its own.
 *   lc_boxes_iou_pairwise_fwd: out [na, nb] row-major.  na * nb <= 2^38, mode in 0..2 (LC_EUNSUP otherwise).
 *   lc_boxes_iou_aligned_fwd: out [n], row i of a with row i of b, mode 0 or 2 (LC_EUNSUP otherwise); the same kernel, so the
 *     same bits as entry [i, i] of the pairwise form.
 *   lc_nms_mask_fwd: mask [n, ceil(n / 64)] 64-bit words, bit c of word [r, w] set iff iou(r, 64 w + c) > thresh and
 *     64 w + c > r; iou is the BEV IoU (normal == 0) or the IoU of the unrotated extents (normal != 0).  Only the words
 *     with w >= r / 64 are written; the others are left as they were.  n <= LC_NMS_MAX_BOXES (LC_EUNSUP above: the mask
 *     would pass 512 MiB).
 *   lc_nms_select_fwd: the greedy walk over such a mask in index order -- box i is kept unless an earlier kept box has
 *     its bit set -- on the device, reading only the words lc_nms_mask_fwd writes.  keep [n] receives the kept indices in
 *     ascending order, *count their number (device memory both; entries of keep past *count are not written).
 *   lc_boxes_iou_bev_host / lc_boxes_overlap_bev_host: the BEV IoU / the overlap area (and, where cnt is not null, the
 *     number of polygon points found, [na, nb] int32) of every pair on the CPU, through the same header. */
#define LC_NMS_MAX_BOXES 65536
int lc_boxes_iou_pairwise_fwd(const float* boxes_a, int na, const float* boxes_b, int nb, int mode, float* out, lc_stream_t s);
int lc_boxes_iou_aligned_fwd(const float* boxes_a, const float* boxes_b, int n, int mode, float* out, lc_stream_t s);
int lc_nms_mask_fwd(const float* boxes, int n, float thresh, int normal, uint64_t* mask, lc_stream_t s);
int lc_nms_select_fwd(const uint64_t* mask, int n, int64_t* keep, int32_t* count, lc_stream_t s);
int lc_boxes_iou_bev_host(const float* boxes_a, int na, const float* boxes_b, int nb, float* out);
int lc_boxes_overlap_bev_host(const float* boxes_a, int na, const float* boxes_b, int nb, float* out, int32_t* cnt);

/* ---------------------------------------------------------------------------------------------
 * lidargen.ops.pointnet2.pointnet2_stack (csrc/pointnet2_stack.hip): the ragged-batch set-abstraction
 * operators.  Contiguous float32 / int32 DEVICE tensors; a stacked tensor holds cloud b in rows start_b .. start_b + n_b - 1,
 * the counts [B] are device memory.  Every entry checks its arguments before any launch (null pointers, negative sizes:
 * LC_EINVAL; B > LC_PN2_MAX_BATCH, nsample > LC_PN2_MAX_NSAMPLE, sizes past the 32-bit index range: LC_EUNSUP); a row count
 * of 0 on the output side returns LC_OK with nothing launched.  The offsets are one exclusive scan per call (clamped into
 * the tensors, so counts that do not add up to the row counts leave rows empty, never an access outside an operand); every
 * index is checked against its own cloud before it is dereferenced.  No float atomics, fixed summation orders, a cloud's bits
 * do not depend on the batch.  Distances: d = (dx dx + dy dy) + dz dz in float32, each operation rounded on its own.
 * scratch: lc_pn2_scratch_elems(B, rows of the query side) int32, written before it is read by the same call.
 *   lc_pn2_ball_query_fwd: idx [M, nsample] = the first nsample points (ascending, local indices) of the centre's cloud with
 *     d < radius * radius (float32 product, strict), the rest of the row the first hit; an empty ball is [-1, 0, ...].
 *   lc_pn2_group_fwd: out [M, C, nsample], out[m, c, s] = features[start + idx[m, s], c], 0 for an index outside [0, n_b).
 *     (No backward entry.)
 *   lc_pn2_three_nn_fwd: unknown [N, 3], known [M, 3] -> dist2 [N, 3], idx [N, 3] (global rows), ascending (distance,
 *     index) under strict <; a slot never filled holds +inf and the cloud's start row.
 *   lc_pn2_three_interpolate_fwd: out [N, C] = (w0 f0 + w1 f1) + w2 f2, features [M, C]; an index outside [0, M) adds 0.
 *   lc_pn2_three_interpolate_bwd: grad_features [M, C]: row m = the sum of grad_out[n, c] weight[n, j] over the entries
 *     e = 3 n + j in order[seg[m] .. seg[m + 1]), in that order (order: the stable sort of the flat indices, seg [M + 1]
 *     the first position of every row).
 *   lc_pn2_voxel_query_fwd: new_coords [M, 4] = (batch, z, y, x), point_indices [B, Z, Y, X] (global rows of xyz [N, 3] or
 *     -1): the (dz, dy, dx)-ascending walk over the cells within the ranges, d <= radius * radius (inclusive), the first
 *     nsample hits, the row pre-filled with the first; an empty row is [-1, 0, ...].  Ranges <= 1024.
 *   lc_pn2_sa_first_fwd: y [Co, M nsample] = relu(W G + bias), G the grouped operand of QueryAndGroup (rows 0..2
 *     xyz[start + idx] - new_xyz[m] when use_xyz, then features [N, C]; C may be 0 with use_xyz; a column of an empty ball,
 *     idx[m, 0] < 0, is zero) gathered into the dense engine's tile: wpk = lc_pointmlp_pack_weight of W [Co, C + 3 use_xyz],
 *     16-byte aligned; the bits of lc_pointmlp_conv_fwd (act = 1, no residual) on the materialised operand.
 *   lc_pn2_limit(i): 0 LC_PN2_MAX_NSAMPLE, 1 LC_PN2_MAX_BATCH, 2 the columns per block of the gathered layer at Co <= 32. */
#define LC_PN2_MAX_NSAMPLE 256
#define LC_PN2_MAX_BATCH 4096
int lc_pn2_limit(int which);
int64_t lc_pn2_scratch_elems(int B, int M);
int lc_pn2_ball_query_fwd(const float* xyz, const int* xyz_cnt, const float* new_xyz, const int* new_cnt, int* idx,
                          int* scratch, int B, int N, int M, float radius, int nsample, lc_stream_t s);
int lc_pn2_group_fwd(const float* features, const int* features_cnt, const int* idx, const int* idx_cnt, float* out,
                     int* scratch, int B, int N, int C, int M, int nsample, lc_stream_t s);
int lc_pn2_three_nn_fwd(const float* unknown, const int* unknown_cnt, const float* known, const int* known_cnt, float* dist2,
                        int* idx, int* scratch, int B, int N, int M, lc_stream_t s);
int lc_pn2_three_interpolate_fwd(const float* features, const int* idx, const float* weight, float* out, int N, int C, int M,
                                 lc_stream_t s);
int lc_pn2_three_interpolate_bwd(const float* grad_out, const int* order, const int* seg, const float* weight,
                                 float* grad_features, int N, int C, int M, lc_stream_t s);
int lc_pn2_voxel_query_fwd(const float* new_xyz, const float* xyz, const int* new_coords, const int* point_indices, int* idx,
                           int M, int N, int B, int Z, int Y, int X, int nsample, float radius, int z_range, int y_range,
                           int x_range, lc_stream_t s);
int lc_pn2_sa_first_fwd(const float* xyz, const int* xyz_cnt, const float* new_xyz, const int* new_cnt, const float* features,
                        const int* idx, const float* wpk, const float* bias, float* y, int* scratch, int B, int N, int M, int C,
                        int Co, int nsample, int use_xyz, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * Float64 statistics of lidargen/metrics/distribution.py on the device (csrc/stats_f64.hip): the
 * Frechet distance and the squared MMD.  Contiguous float64 / int32 DEVICE memory unless a stride is given.  Every entry
 * checks its arguments before any launch (null pointers, sizes < 1: LC_EINVAL; a grid or index range that is not built:
 * LC_EUNSUP).  No float atomics, every sum in one order that depends on the shapes alone: two calls give the same bits.
 *   lc_stats_gemm_f64: C [M, N] (row pitch ldc) = sum_k P(i, k) Q(j, k) on v_mfma_f64_16x16x4_f64, P(i, k) =
 *     P[i p_rs + k p_ks], Q(j, k) = Q[j q_rs + k q_ks] (strides in elements, >= 0), so P Q^T, P^T Q and P Q are one kernel.
 *     Any M, N, K >= 1; tile edges and K tails are zero-filled in the tile, never read.
 *   lc_stats_mmd_f64: fx [nx, width], fy [ny, width], table [num_subsets, 2, m] int32: subset s is x = fx[table[s][0]],
 *     y = fy[table[s][1]] (a row index outside its matrix reads as a zero row).  Per subset and 64 x 64 tile of x x^T, y y^T
 *     and x y^T the sum of (g / width + 1)^3, the diagonal of the first two dropped, goes to partial
 *     (lc_stats_mmd_partials(num_subsets, m) doubles); then out [num_subsets, 2] = (the within-set off-diagonal sum, the cross
 *     sum), the partials added in tile order.  The m x m matrices are never written.
 *   lc_stats_center_f64: X [n, d], n >= 2 -> mean [d] and A [n, d] = (X - mean) / sqrt(n - 1).
 *   lc_stats_reduce_f64: *out = the sum over i < n of t(a[i sa], b[i sb]), mode 0: a, 1: a a, 2: (a - b)(a - b),
 *     3: sqrt(max(a, 0)); scratch: LC_STATS_REDUCE_SCRATCH doubles.
 *   lc_stats_scale_rows_f64: out [k, k] row i = sqrt(lam[i]) V row i, a zero row where lam[i] <= cut max_j lam[j] (cut >= 0).
 *   One-sided (Hestenes) Jacobi on the ROWS of W [k, k] (a symmetric matrix is its own transpose), k <= LC_STATS_MAX_EIG:
 *   lc_stats_jacobi_sweep: one round-robin sweep, k - 1 steps (k for odd k) of floor(k / 2) disjoint row pairs, one launch
 *     per step.  A pair is rotated when |w_p . w_q| > tol |w_p| |w_q| (never when the norms multiply to zero) and, where
 *     fro2 is not null, |w_p . w_q| > atol sqrt(*fro2 / k) max(|w_p|, |w_q|) (*fro2: device, the squared Frobenius norm of the
 *     matrix; the left side over the larger norm is the entry (p, q) of V S V^T); V (may be null; lc_stats_jacobi_init
 *     writes the identity) receives the same rotations.  *flag (device int32): 1 if any pair was
 *     rotated in this sweep, else 0.  At convergence row i of W is lambda_i times eigenvector i and row i of V eigenvector i.
 *   lc_stats_jacobi_values: lam [k] = the row norms of W (the absolute eigenvalues).
 *   lc_stats_jacobi_pair (host only): pq[0] < pq[1] the pair of (step, slot) for this k >= 2, pq[1] = -1 for the idle slot.
 *   lc_stats_limit(i): 0 LC_STATS_MAX_EIG, 1 LC_STATS_REDUCE_SCRATCH. */
#define LC_STATS_MAX_EIG 4096
#define LC_STATS_REDUCE_SCRATCH 1024
int lc_stats_limit(int which);
int lc_stats_jacobi_pair(int k, int step, int slot, int* pq);
int lc_stats_gemm_f64(const double* P, int64_t p_rs, int64_t p_ks, const double* Q, int64_t q_rs, int64_t q_ks, double* C,
                      int64_t ldc, int M, int N, int K, lc_stream_t s);
int64_t lc_stats_mmd_partials(int num_subsets, int m);
int lc_stats_mmd_f64(const double* fx, int nx, const double* fy, int ny, int width, const int32_t* table, int num_subsets,
                     int m, double* partial, double* out, lc_stream_t s);
int lc_stats_center_f64(const double* X, int n, int d, double* mean, double* A, lc_stream_t s);
int lc_stats_reduce_f64(const double* a, int64_t sa, const double* b, int64_t sb, int64_t n, int mode, double* scratch,
                        double* out, lc_stream_t s);
int lc_stats_scale_rows_f64(const double* V, const double* lam, int k, double cut, double* out, lc_stream_t s);
int lc_stats_jacobi_init(double* V, int k, lc_stream_t s);
int lc_stats_jacobi_sweep(double* W, double* V, int k, double tol, double atol, const double* fro2, int32_t* flag,
                          lc_stream_t s);
int lc_stats_jacobi_values(const double* W, int k, double* lam, lc_stream_t s);

/* ---------------------------------------------------------------------------------------------
 * The step in front of the FRID / FSVD / FPVD networks on the device, a ragged batch of clouds at a time
 * (csrc/metric_preprocess.hip; lidargen/metrics/metric_utils.py preprocess_range, preprocess_pcd +
 * pcd2voxel + sparse_collate).  pts: contiguous [N, 3] float32 (is_f64 = 0) or float64 (1); offsets: int32 [B + 1],
 * offsets[0] = 0, non-decreasing, offsets[B] = N (the CALLER guarantees it; a kernel only ever derives a cloud index in
 * [0, B) from them).  0 <= lo < hi: the open depth interval.  Integer atomics only: two calls give the same bits.
 *   lc_range_batch_fwd: out float32 [B, 4, H, W] = (depth, x, y, z) of preprocess_range applied to each cloud WIDENED TO
 *     FLOAT64.  zbuf: uint32 [B, H, W] scratch.  dir: float64 [3, H, W], the ray directions of range2xyz at the pixel
 *     centres.  fov_down_abs, fov_range: |fov_down| and |fov_down| + |fov_up| in radians.  lo32, hi32: the bounds rounded to
 *     float32 (range2xyz's mask on the float32 depth image).  N = 0 is legal (every pixel -1).
 *   lc_voxel_batch_fwd: feats float32 [n, 4] = (the first point of each voxel, -1), coords int32 [n, 4] = (rint(p / voxel)
 *     - the cloud's minimum, cloud index), out_offsets int32 [B + 1]; n = out_offsets[B] <= N rows are written, feats and
 *     coords hold N rows.  Filter and quotient in the dtype of pts (lo, hi, voxel rounded to it).  N >= 1.
 *     scratch: lc_voxel_batch_scratch_bytes(N, B) bytes.
 *   lc_voxel_batch_key_bits (host only): bits[0] = the bits of the cloud field of the sort key (values 0 ... B), bits[1] =
 *     those of the three axis fields (each holds q + R, R = ceil(hi / voxel) + 2); LC_EUNSUP when they exceed 64 together,
 *     which lc_voxel_batch_fwd refuses alike. */
int lc_range_batch_fwd(const void* pts, int is_f64, const int32_t* offsets, int B, int N, int H, int W, double lo, double hi,
                       float lo32, float hi32, double fov_down_abs, double fov_range, const double* dir, uint32_t* zbuf,
                       float* out, lc_stream_t s);
int lc_voxel_batch_key_bits(int B, double hi, double voxel, int32_t* bits);
int64_t lc_voxel_batch_scratch_bytes(int N, int B);
int lc_voxel_batch_fwd(const void* pts, int is_f64, const int32_t* offsets, int B, int N, double lo, double hi, double voxel,
                       void* scratch, float* feats, int32_t* coords, int32_t* out_offsets, lc_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* LIDARCRAFTER_HIP_H */
