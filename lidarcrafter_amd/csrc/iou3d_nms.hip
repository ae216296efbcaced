// lidargen.ops.iou3d_nms on HIP: rotated BEV overlap / IoU, 3-D IoU and NMS over float32 rows
// [x, y, z, dx, dy, dz, heading].  The geometry is csrc/iou3d_box.h, shared with the host entry and the stand-alone host
// check; csrc/glenet.hip restates a different algorithm (GLENet's) and shares nothing with this file.
//   iou3d_pair_kernel    one lane per pair, 256 lanes per block.  Pair t is (t / M, t % M) of the N x M grid, or (t, t)
//                        for the row-aligned form: ONE kernel, so the aligned and the pairwise results of the same two rows
//                        are the same instructions and the same bits.  Mode 0 the BEV overlap area, 1 the BEV IoU, 2 the 3-D
//                        IoU: the reference's torch epilogue applied to the overlap in its order, each operation rounded on
//                        its own.
//   iou3d_mask_kernel    one wave per (block of 64 row boxes, block of 64 column boxes) ON OR ABOVE the diagonal -- the
//                        triangular block index is unfolded on the device; the blocks below it, which the reference fills
//                        and never reads, are not launched.  The 64 column boxes sit in LDS; lane r walks them and builds
//                        the 64-bit word of its row in a register (one lane's loop, not a ballot), bit c set iff
//                        iou(row, col) > thresh, in the diagonal block only for col > row.
//   iou3d_select_kernel  the reference's host-side greedy walk, on the device, one block of 1024 lanes: per block of 64
//                        boxes (1) wave 0 resolves the 64 sequential decisions from the 64 diagonal words, held one per
//                        lane and read with v_readlane, against the running removal word; (2) all lanes OR the kept rows'
//                        words into the removal words of the later blocks (LDS, ds_or_b64: the order of ORs does not
//                        matter); (3) wave 0 writes the kept indices in ascending order.  Only words at or right of the
//                        diagonal are read.  The count goes to device memory; the caller reads 4 bytes.
// The polygon's 16 points are a lane's column of an LDS array ([16][lanes] of 8-byte points, conflict-free): indexed by the
// runtime count they cannot be registers, and LDS spares the scratch-memory round trips.
// Floating-point contraction is OFF for the whole file: every float32 operation is rounded on its own, as in the host
// build of the same header, and the epilogue equals the torch expressions bit for bit.
#pragma clang fp contract(off)
#include "common.h"
#include "iou3d_box.h"

namespace {

constexpr int IO_PAIR_T = 256;        // lanes per block of the pair kernel
constexpr int IO_NMS_T = 64;          // boxes per mask word: one wave
constexpr int IO_SEL_T = 1024;        // lanes of the selection block
constexpr int IO_MAX_WORDS = LC_NMS_MAX_BOXES / IO_NMS_T;

// torch.maximum / torch.minimum / torch.clamp(min=) of the device: a NaN operand is the result, else the IEEE max / min
__device__ inline float io_tmax(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
__device__ inline float io_tmin(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ inline float io_tclamp_min(float v, float lo) { return v != v ? v : fmaxf(v, lo); }

__device__ inline float io_iou3d(const float* a, const float* b, float overlap) {
    // the shared height: lowest roof minus highest floor, not below 0
    const float roof = io_tmin(a[2] + a[5] / 2, b[2] + b[5] / 2);
    const float floor_ = io_tmax(a[2] - a[5] / 2, b[2] - b[5] / 2);
    const float shared = overlap * io_tclamp_min(roof - floor_, 0.f);
    const float volumes = a[3] * a[4] * a[5] + b[3] * b[4] * b[5];       // each product left to right
    return shared / io_tclamp_min(volumes - shared, 1e-6f);
}

__global__ __launch_bounds__(IO_PAIR_T) void iou3d_pair_kernel(const float* __restrict__ boxes_a,
                                                               const float* __restrict__ boxes_b, long long total, int M,
                                                               int aligned, int mode, float* __restrict__ out) {
    __shared__ lc_iou3d_pt pts[LC_IOU3D_MAX_PTS * IO_PAIR_T];
    const long long t = (long long)blockIdx.x * IO_PAIR_T + threadIdx.x;
    if (t >= total) return;
    const long long ia = aligned ? t : t / M, ib = aligned ? t : t % M;
    float a[7], b[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        a[k] = boxes_a[ia * 7 + k];
        b[k] = boxes_b[ib * 7 + k];
    }
    lc_iou3d_pt* mine = pts + threadIdx.x;
    float r;
    if (mode == 1) {
        r = lc_iou3d_iou_bev(a, b, mine, IO_PAIR_T);
    } else {
        r = lc_iou3d_box_overlap(a, b, mine, IO_PAIR_T, nullptr);
        if (mode == 2) r = io_iou3d(a, b, r);
    }
    out[t] = r;
}

template <bool NORMAL>
__global__ __launch_bounds__(IO_NMS_T) void iou3d_mask_kernel(const float* __restrict__ boxes, int n, int words, float thresh,
                                                              unsigned long long* __restrict__ mask) {
    __shared__ float tile[IO_NMS_T * 7];                                     // the rows of the column tile
    __shared__ lc_iou3d_pt pts[NORMAL ? 1 : LC_IOU3D_MAX_PTS * IO_NMS_T];
    // Unfold the launch index into the tile (ty, tx), tx >= ty, of the upper triangle of the words x words tile grid: tile
    // row y owns the words - y indices from first(y) = y words - y (y - 1) / 2.  A float64 root estimates y; the two loops
    // settle it in integers.
    const long long launch = blockIdx.x;
    const auto first = [words](long long y) { return y * words - y * (y - 1) / 2; };
    const double w = 2.0 * words + 1.0;
    long long ty = (long long)((w - sqrt(w * w - 8.0 * (double)launch)) * 0.5);
    ty = ty < 0 ? 0 : (ty > words - 1 ? words - 1 : ty);
    while (ty + 1 < words && first(ty + 1) <= launch) ty++;
    while (ty > 0 && first(ty) > launch) ty--;
    const long long tx = ty + (launch - first(ty));
    if (tx >= words) return;   // (cannot happen for launch < words (words + 1) / 2)

    const int lane = threadIdx.x;
    const long long row0 = ty * IO_NMS_T, col0 = tx * IO_NMS_T;                 // first box of the tile's rows / columns
    const int rows_here = (int)min((long long)IO_NMS_T, n - row0), cols_here = (int)min((long long)IO_NMS_T, n - col0);
    for (int e = lane; e < cols_here * 7; e += IO_NMS_T) tile[e] = boxes[col0 * 7 + e];   // a flat, coalesced copy
    __syncthreads();
    if (lane >= rows_here) return;

    float mine[7];
#pragma unroll
    for (int k = 0; k < 7; k++) mine[k] = boxes[(row0 + lane) * 7 + k];
    unsigned long long word = 0;
    for (int c = (tx == ty ? lane + 1 : 0); c < cols_here; c++) {             // on the diagonal: later boxes only
        const float* other = tile + c * 7;
        const float iou = NORMAL ? lc_iou3d_iou_normal(mine, other) : lc_iou3d_iou_bev(mine, other, pts + lane, IO_NMS_T);
        word |= (unsigned long long)(iou > thresh) << c;
    }
    mask[(row0 + lane) * words + tx] = word;
}

__global__ __launch_bounds__(IO_SEL_T) void iou3d_select_kernel(const unsigned long long* __restrict__ mask, int n,
                                                                int words, long long* __restrict__ keep,
                                                                int* __restrict__ count) {
    __shared__ unsigned long long gone[IO_MAX_WORDS];
    __shared__ unsigned long long s_kept;
    const int tid = threadIdx.x;
    for (int j = tid; j < words; j += IO_SEL_T) gone[j] = 0ULL;
    int num = 0;   // kept so far (wave 0 keeps it; uniform there)
    for (int b = 0; b < words; b++) {
        __syncthreads();   // gone[b] is final: every earlier block's ORs have landed
        const int size = min(n - b * IO_NMS_T, IO_NMS_T);
        if (tid < IO_NMS_T) {
            // (1) lane i holds the diagonal word of row 64 b + i; the 64 decisions run in every lane alike
            const unsigned long long d = tid < size ? mask[((long long)b * IO_NMS_T + tid) * words + b] : 0ULL;
            const int dlo = (int)(unsigned)(d & 0xffffffffULL), dhi = (int)(unsigned)(d >> 32);
            unsigned long long r = gone[b], kept = 0ULL;
#pragma unroll
            for (int i = 0; i < IO_NMS_T; i++) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane(dlo, i);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane(dhi, i);
                if (i < size && !((r >> i) & 1ULL)) {
                    kept |= 1ULL << i;
                    r |= ((unsigned long long)hi << 32) | lo;
                }
            }
            // (3) ascending: lane i writes after the kept lanes below it
            if ((kept >> tid) & 1ULL) keep[num + __popcll(kept & ((1ULL << tid) - 1ULL))] = (long long)b * IO_NMS_T + tid;
            num += __popcll(kept);
            if (tid == 0) s_kept = kept;
        }
        __syncthreads();
        // (2) the kept rows' words right of the diagonal into the running removal words
        const unsigned long long kept = s_kept;
        const int W = words - b - 1;
        for (int idx = tid; idx < IO_NMS_T * W; idx += IO_SEL_T) {
            const int i = idx / W, j = b + 1 + idx % W;
            if ((kept >> i) & 1ULL) {
                const unsigned long long word = mask[((long long)b * IO_NMS_T + i) * words + j];
                if (word) atomicOr(&gone[j], word);
            }
        }
    }
    if (tid == 0) *count = num;
}

}  // namespace

extern "C" int lc_boxes_iou_pairwise_fwd(const float* boxes_a, int na, const float* boxes_b, int nb, int mode, float* out,
                                         lc_stream_t s) {
    if (!boxes_a || !boxes_b || !out || na < 0 || nb < 0) return LC_EINVAL;
    if (mode < 0 || mode > 2) return LC_EUNSUP;
    if (na == 0 || nb == 0) return LC_OK;
    const long long total = (long long)na * nb;
    if (total > (1LL << 38)) return LC_EUNSUP;    // the pair index is the lane index of a 1-D grid of 2^31 blocks at the most
    hipLaunchKernelGGL(iou3d_pair_kernel, dim3((unsigned)((total + IO_PAIR_T - 1) / IO_PAIR_T)), dim3(IO_PAIR_T), 0, lc_s(s),
                       boxes_a, boxes_b, total, nb, 0, mode, out);
    return lc_launch_status();
}

extern "C" int lc_boxes_iou_aligned_fwd(const float* boxes_a, const float* boxes_b, int n, int mode, float* out,
                                        lc_stream_t s) {
    if (!boxes_a || !boxes_b || !out || n < 0) return LC_EINVAL;
    if (mode != 0 && mode != 2) return LC_EUNSUP;
    if (n == 0) return LC_OK;
    hipLaunchKernelGGL(iou3d_pair_kernel, dim3((unsigned)((n + IO_PAIR_T - 1) / IO_PAIR_T)), dim3(IO_PAIR_T), 0, lc_s(s),
                       boxes_a, boxes_b, (long long)n, 1, 1, mode, out);
    return lc_launch_status();
}

extern "C" int lc_nms_mask_fwd(const float* boxes, int n, float thresh, int normal, uint64_t* mask, lc_stream_t s) {
    if (!boxes || !mask || n < 0) return LC_EINVAL;
    if (n > LC_NMS_MAX_BOXES) return LC_EUNSUP;
    if (n == 0) return LC_OK;
    const int cb = (n + IO_NMS_T - 1) / IO_NMS_T;
    const unsigned blocks = (unsigned)((long long)cb * (cb + 1) / 2);
    if (normal)
        hipLaunchKernelGGL(iou3d_mask_kernel<true>, dim3(blocks), dim3(IO_NMS_T), 0, lc_s(s), boxes, n, cb, thresh,
                           (unsigned long long*)mask);
    else
        hipLaunchKernelGGL(iou3d_mask_kernel<false>, dim3(blocks), dim3(IO_NMS_T), 0, lc_s(s), boxes, n, cb, thresh,
                           (unsigned long long*)mask);
    return lc_launch_status();
}

extern "C" int lc_nms_select_fwd(const uint64_t* mask, int n, int64_t* keep, int32_t* count, lc_stream_t s) {
    if (!mask || !keep || !count || n < 0) return LC_EINVAL;
    if (n > LC_NMS_MAX_BOXES) return LC_EUNSUP;
    if (n == 0) return LC_OK;
    hipLaunchKernelGGL(iou3d_select_kernel, dim3(1), dim3(IO_SEL_T), 0, lc_s(s), (const unsigned long long*)mask, n,
                       (n + IO_NMS_T - 1) / IO_NMS_T, (long long*)keep, count);
    return lc_launch_status();
}

extern "C" int lc_boxes_iou_bev_host(const float* boxes_a, int na, const float* boxes_b, int nb, float* out) {
    if (!boxes_a || !boxes_b || !out || na < 0 || nb < 0) return LC_EINVAL;
    lc_iou3d_pt pts[LC_IOU3D_MAX_PTS];
    for (long long i = 0; i < na; i++)
        for (long long j = 0; j < nb; j++) out[i * nb + j] = lc_iou3d_iou_bev(boxes_a + i * 7, boxes_b + j * 7, pts, 1);
    return LC_OK;
}

extern "C" int lc_boxes_overlap_bev_host(const float* boxes_a, int na, const float* boxes_b, int nb, float* out,
                                         int32_t* cnt) {
    if (!boxes_a || !boxes_b || !out || na < 0 || nb < 0) return LC_EINVAL;
    lc_iou3d_pt pts[LC_IOU3D_MAX_PTS];
    for (long long i = 0; i < na; i++)
        for (long long j = 0; j < nb; j++) {
            int c = 0;
            out[i * nb + j] = lc_iou3d_box_overlap(boxes_a + i * 7, boxes_b + j * 7, pts, 1, &c);
            if (cnt) cnt[i * nb + j] = c;
        }
    return LC_OK;
}
