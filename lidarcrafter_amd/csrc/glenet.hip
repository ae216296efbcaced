// GLENet box sampler and rotated IoU of the RGF object metric: what the reference's
// lidargen/metrics/models/glenet/{point_net,model,loss_utils}.py and eval_utils/eval_utils.py compute per object and draw.
//   gl_center_kernel   one block per object of a ragged batch: the mean of its points (float64 partial sums per thread over
//                      a strided walk, a fixed tree over the 256 threads, rounded once to float32), then
//                      out = float32((p - mean) / scale) with the float32 difference divided in float64.
//   gl_trunk_kernel    one block per row r = (draw, object): the per-point MLP 3 -> 64 -> 128 -> 512 of PointNetfeat and, in
//                      the same pass over the same points, the 3 -> 8 -> 8 -> 8 of SimPointNetfeat, each followed by the max
//                      over the row's K points.  The three stages of a tile are pn_trunk_kernel's (csrc/pointnet_trunk.h: layer 1 on the vector
//                      ALUs, layers 2 and 3 on v_mfma_f32_32x32x2_f32 with the points as columns, the same k order), with
//                      three differences: layer 1 GATHERS its point as norm[offsets[b] + choice[r][n]] (no [R,3,K] tensor
//                      exists), the block walks all tiles of its row and keeps the running channel maxima in LDS (no partial
//                      maxima in memory, no second launch), and the results are written channel-major, [C][R], the operand
//                      layout of lc_pointmlp_conv_fwd.  The row index is the block index (x dimension): any R.
//   gl_inter / gl_iou  device functions, one thread per pair: a literal float32 restatement of compute_vertex, sort_vertex
//                      and area_polygon with floating-point contraction off (numpy does not fuse), and iou3d around them.
//   gl_score_kernel    one wave per object, lane = draw: decode, paired IoU, then the variance of the seven box columns and
//                      the mean overlap in float64, in draw order.
// No atomics anywhere; a row's / an object's / a pair's bits depend on its own operands only.
#include "common.h"
#include "pointnet_trunk.h"   // the three stages of a tile, shared with csrc/pointnet.hip

namespace {

constexpr int GL_T = PNT_T;                   // points per tile of the trunk
constexpr int GL_C2 = PNT_C2, GL_C3 = 512, GL_CS = 8;

// ---------------------------------------------------------------------------------------------------- segment centre
__global__ __launch_bounds__(256) void gl_center_kernel(const float* __restrict__ pts, const int* __restrict__ offsets,
                                                        long long total, double sx, double sy, double sz,
                                                        float* __restrict__ out, float* __restrict__ mean) {
    __shared__ double red[3][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    long long lo = offsets[b], hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > total ? total : lo);
    hi = hi < lo ? lo : (hi > total ? total : hi);
    const long long n = hi - lo;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long i = lo + tid; i < hi; i += 256) {
        s0 += (double)pts[3 * i];
        s1 += (double)pts[3 * i + 1];
        s2 += (double)pts[3 * i + 2];
    }
    red[0][tid] = s0, red[1][tid] = s1, red[2][tid] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
            red[2][tid] += red[2][tid + o];
        }
        __syncthreads();
    }
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    if (n > 0) {
        m0 = (float)(red[0][0] / (double)n);
        m1 = (float)(red[1][0] / (double)n);
        m2 = (float)(red[2][0] / (double)n);
    }
    if (tid == 0) {
        mean[3 * (size_t)b] = m0;
        mean[3 * (size_t)b + 1] = m1;
        mean[3 * (size_t)b + 2] = m2;
    }
    for (long long i = lo + tid; i < hi; i += 256) {
        const float d0 = pts[3 * i] - m0, d1 = pts[3 * i + 1] - m1, d2 = pts[3 * i + 2] - m2;
        out[3 * i] = (float)((double)d0 / sx);
        out[3 * i + 1] = (float)((double)d1 / sy);
        out[3 * i + 2] = (float)((double)d2 / sz);
    }
}

// ---------------------------------------------------------------------------------------------------- trunk
__global__ __launch_bounds__(256, 2) void gl_trunk_kernel(
    const float* __restrict__ norm, long long total, const int* __restrict__ offsets, const int* __restrict__ choice, int B,
    int K, long long R, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3,
    const float* __restrict__ sw1, const float* __restrict__ sb1, const float* __restrict__ sw2,
    const float* __restrict__ sb2, const float* __restrict__ sw3, const float* __restrict__ sb3, float* __restrict__ featA,
    float* __restrict__ featS) {
    // h1 [64][GL_T], then h2 [128][GL_T] in its place (layer 2 holds its results in registers across a barrier)
    __shared__ __attribute__((aligned(16))) float h2[GL_C2 * GL_T];
    __shared__ float rmax[GL_C3];             // running maxima of the main trunk: channel c is written by one lane only
    __shared__ float smax[GL_CS];             // running maxima of the side trunk
    __shared__ float sred[2][GL_CS];          // the side trunk's maxima of the current tile, per wave
    float* const h1 = h2;
    const long long r = blockIdx.x;
    const int b = (int)(r % B);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const float ninf = -__builtin_huge_valf();

    long long lo = offsets[b], hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > total ? total : lo);
    hi = hi < lo ? lo : (hi > total ? total : hi);
    const int cnt = (int)((hi - lo) > 0x7fffffffll ? 0x7fffffffll : (hi - lo));
    const int* const ch = choice + (size_t)r * K;

    for (int c = tid; c < GL_C3; c += 256) rmax[c] = ninf;
    if (tid < GL_CS) smax[tid] = ninf;
    // (the first barrier of the tile loop orders these stores before their first use)

    const int tiles = (K + GL_T - 1) / GL_T;
    for (int tile = 0; tile < tiles; ++tile) {
        const int t0 = tile * GL_T;
        {   // layer 1: thread = (point, half of the 64 channels); the threads of half 0 run the side trunk of their point too
            const int p = tid & (GL_T - 1), half = __builtin_amdgcn_readfirstlane(tid >> 7), c0 = half * 32;
            const int n = t0 + p;
            float q0 = 0.f, q1 = 0.f, q2 = 0.f;
            if (n < K && cnt > 0) {
                int i = ch[n];
                i = i < 0 ? 0 : (i >= cnt ? cnt - 1 : i);
                const float* q = norm + 3 * (size_t)(lo + i);
                q0 = q[0], q1 = q[1], q2 = q[2];
            }
            pnt_layer1(h1, p, c0, q0, q1, q2, w1, b1);
            if (half == 0) {                  // waves 0 and 1
                float s1[GL_CS], s2[GL_CS];
#pragma unroll
                for (int c = 0; c < GL_CS; ++c)
                    s1[c] = fmaxf(fmaf(sw1[c * 3 + 2], q2, fmaf(sw1[c * 3 + 1], q1, fmaf(sw1[c * 3], q0, sb1[c]))), 0.f);
#pragma unroll
                for (int c = 0; c < GL_CS; ++c) {
                    float v = sb2[c];
#pragma unroll
                    for (int k = 0; k < GL_CS; ++k) v = fmaf(sw2[c * GL_CS + k], s1[k], v);
                    s2[c] = fmaxf(v, 0.f);
                }
#pragma unroll
                for (int c = 0; c < GL_CS; ++c) {
                    float v = sb3[c];
#pragma unroll
                    for (int k = 0; k < GL_CS; ++k) v = fmaf(sw3[c * GL_CS + k], s2[k], v);
                    if (n >= K) v = ninf;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
                    if (lane == 0) sred[wave][c] = v;
                }
            }
        }
        __syncthreads();
        if (tid < GL_CS) smax[tid] = fmaxf(smax[tid], fmaxf(sred[0][tid], sred[1][tid]));

        pnt_layer2(h2, w2, b2, wave, j, h);
        __syncthreads();

        // layer 3 in 16 chunks of 32 output channels, 4 per wave
        const int nvalid = K - t0;            // >= 1; < GL_T only in the row's last tile
        for (int it = 0; it < GL_C3 / 32 / 4; ++it) {
            const int chunk = wave + 4 * it;
            float m[16];
            pnt_layer3_chunk(h2, w3, chunk, j, h, nvalid, m);
            if (j == 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int c = chunk * 32 + mfma_row(v, h);
                    rmax[c] = fmaxf(rmax[c], m[v]);
                }
            }
        }
        __syncthreads();                      // h2 is free for the next tile's h1; rmax is complete after the last tile
    }
    // bias behind the max: exact, the addition is monotone (a BatchNorm scale is not: it is in W3)
    for (int c = tid; c < GL_C3; c += 256) featA[(size_t)c * R + r] = rmax[c] + b3[c];
    if (tid < GL_CS) featS[(size_t)tid * R + r] = smax[tid];
}

// ---------------------------------------------------------------------------------------------------- rotated boxes
// compute_vertex + sort_vertex + area_polygon of glenet/loss_utils.py on one pair; every float32 operation rounded on its
// own.  pts[16] receives compute_vertex's vertices (unsorted, zero past cnt); returns area_polygon's area.  Every loop is
// unrolled and every array index is a constant, so the arrays live in registers (a slot is chosen by compares, not by an
// address): no scratch memory.
__host__ __device__ inline void gl_put(float* pts, int& cnt, float x, float y) {
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (cnt == s) {
            pts[2 * s] = x;
            pts[2 * s + 1] = y;
        }
    ++cnt;
}

// numpy's sort order of floats: NaN last
__host__ __device__ inline bool gl_before(float a, float b) { return a < b || (b != b && a == a); }

__host__ __device__ inline float gl_inter(const float* g, const float* q, float* pts, int* cnt_out) {
#pragma clang fp contract(off)
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) pts[i] = 0.f;
    {   // corners of g inside q
        const float ab0 = q[2] - q[0], ab1 = q[3] - q[1], ad0 = q[6] - q[0], ad1 = q[7] - q[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ap0 = g[2 * i] - q[0], ap1 = g[2 * i + 1] - q[1];
            const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
            const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
            if (abab >= abap && abap >= 0.f && adad >= adap && adap >= 0.f && adad > 0.f && abab > 0.f)
                gl_put(pts, cnt, g[2 * i], g[2 * i + 1]);
        }
    }
    {   // corners of q inside g
        const float ab0 = g[2] - g[0], ab1 = g[3] - g[1], ad0 = g[6] - g[0], ad1 = g[7] - g[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ap0 = q[2 * i] - g[0], ap1 = q[2 * i + 1] - g[1];
            const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
            const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
            if (abab >= abap && abap >= 0.f && adad >= adap && adap >= 0.f) gl_put(pts, cnt, q[2 * i], q[2 * i + 1]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)               // edge i of g against edge j of q
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const float A0 = g[2 * i], A1 = g[2 * i + 1], B0 = g[2 * ((i + 1) & 3)], B1 = g[2 * ((i + 1) & 3) + 1];
            const float C0 = q[2 * jj], C1 = q[2 * jj + 1], D0 = q[2 * ((jj + 1) & 3)], D1 = q[2 * ((jj + 1) & 3) + 1];
            const float BA0 = B0 - A0, BA1 = B1 - A1, CA0 = C0 - A0, CA1 = C1 - A1, DA0 = D0 - A0, DA1 = D1 - A1;
            const bool acd = DA1 * CA0 > CA1 * DA0;
            const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
            const bool abc = CA1 * BA0 > BA1 * CA0;
            const bool abd = DA1 * BA0 > BA1 * DA0;
            if (acd != bcd && abc != abd && cnt <= 7) {          // with 8 vertices held the reference prints and skips
                const float DC0 = D0 - C0, DC1 = D1 - C1;
                const float ABBA = A0 * B1 - B0 * A1, CDDC = C0 * D1 - D0 * C1;
                const float DH = BA1 * DC0 - BA0 * DC1;
                const float Dx = ABBA * DC0 - BA0 * CDDC, Dy = ABBA * DC1 - BA1 * CDDC;
                gl_put(pts, cnt, Dx / DH, Dy / DH);
            }
        }
    *cnt_out = cnt;
    if (cnt < 1) return 0.f;
    // sort_vertex: descending angle about the float32 centroid; all 8 slots are sorted, the unused ones with angle 0
    float c0 = 0.f, c1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < cnt) {
            c0 += pts[2 * i];
            c1 += pts[2 * i + 1];
        }
    c0 /= (float)cnt;
    c1 /= (float)cnt;
    float key[8];                             // -angle: ascending
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float ang = 0.f;
        if (i < cnt) {
            float v0 = pts[2 * i] - c0, v1 = pts[2 * i + 1] - c1;
            const float d = (float)sqrt((double)(v0 * v0 + v1 * v1));
            v0 = v0 / d;
            v1 = v1 / d;
            const double a = atan2((double)v1, (double)v0);
            ang = (float)(a < 0.0 ? a + 2 * 3.1415926 : a);
        }
        key[i] = -ang;
    }
    // a stable sort as ranks: slot i goes to place rank[i] = the number of slots in front of it (NaN keys last, as numpy
    // orders them; equal keys in slot order)
    float s[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j != i && (gl_before(key[j], key[i]) || (!gl_before(key[i], key[j]) && j < i))) ++rank;
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (rank == t && t < cnt) {
                s[2 * t] = pts[2 * i];
                s[2 * t + 1] = pts[2 * i + 1];
            }
    }
    float area = 0.f;                         // area_polygon: a fan from the first sorted vertex
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (i < cnt - 2) {
            const float p10 = s[0], p11 = s[1], p20 = s[2 * i + 2], p21 = s[2 * i + 3], p30 = s[2 * i + 4], p31 = s[2 * i + 5];
            const float t = ((p10 - p30) * (p21 - p31) - (p11 - p31) * (p20 - p30)) / 2.0f;
            area += fabsf(t);
        }
    return area;
}

__host__ __device__ inline float gl_clamp200(float v) { return fminf(fmaxf(v, -200.f), 200.f); }

// rbbox_to_corners of (x, y, dx, dy, ry); the cosine and sine are the correctly rounded float32 values (a float64 evaluation
// rounded once): degenerate pairs -- a box against itself turned by pi -- hang on their last bit
__host__ __device__ inline void gl_corners(float x, float y, float dx, float dy, float ry, float* c) {
#pragma clang fp contract(off)
    const float cs = (float)cos((double)ry), sn = (float)sin((double)ry);
    const float dxcos = dx * cs / 2.0f, dxsin = dx * sn / 2.0f, dycos = dy * cs / 2.0f, dysin = dy * sn / 2.0f;
    c[0] = -dxcos - dysin + x;
    c[1] = dxsin - dycos + y;
    c[2] = -dxcos + dysin + x;
    c[3] = dxsin + dycos + y;
    c[4] = dxcos + dysin + x;
    c[5] = -dxsin + dycos + y;
    c[6] = dxcos - dysin + x;
    c[7] = -dxsin - dycos + y;
}

// iou3d of eval_utils.py on one pair of boxes (x, y, z, dx, dy, dz, ry)
__host__ __device__ inline float gl_iou(const float* gb, const float* qb) {
#pragma clang fp contract(off)
    float g[7], q[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        g[i] = gl_clamp200(gb[i]);
        q[i] = gl_clamp200(qb[i]);
    }
    float cg[8], cq[8], pts[16];
    int cnt;
    gl_corners(g[0], g[1], g[3], g[4], g[6], cg);
    gl_corners(q[0], q[1], q[3], q[4], q[6], cq);
    const float area = gl_inter(cg, cq, pts, &cnt);
    float ih = fminf(g[2] + 0.5f * g[5], q[2] + 0.5f * q[5]) - fmaxf(g[2] - 0.5f * g[5], q[2] - 0.5f * q[5]);
    if (ih < 0.f) ih = 0.f;
    const float vg = g[3] * g[4] * g[5], vq = q[3] * q[4] * q[5];
    const float inc = ih * area;
    const float uni = vg + vq - inc;
    return inc / uni;
}

__global__ __launch_bounds__(64) void gl_inter_kernel(const float* __restrict__ cg, const float* __restrict__ cq, int N,
                                                      float* __restrict__ pts, int* __restrict__ cnt,
                                                      float* __restrict__ area) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= N) return;
    float g[8], q[8], p[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        g[k] = cg[8 * (size_t)i + k];
        q[k] = cq[8 * (size_t)i + k];
    }
    int c;
    const float a = gl_inter(g, q, p, &c);
#pragma unroll
    for (int k = 0; k < 16; ++k) pts[16 * (size_t)i + k] = p[k];
    cnt[i] = c;
    area[i] = a;
}

__global__ __launch_bounds__(64) void gl_iou_kernel(const float* __restrict__ gb, int ldg, const float* __restrict__ qb,
                                                    int ldq, int N, float* __restrict__ iou) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= N) return;
    float g[7], q[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        g[k] = gb[(size_t)i * ldg + k];
        q[k] = qb[(size_t)i * ldq + k];
    }
    iou[i] = gl_iou(g, q);
}

// ---------------------------------------------------------------------------------------------------- score
// eval_one_epoch's decode of a normalised box (x, y, z, log dx, log dy, log dz, ry): the centres times (diag, diag, dza) --
// diag is a float64 in the reference, the product is rounded once --, the sizes exp(.) times the anchor in float32
__host__ __device__ inline void gl_decode(const float* in, double diag, float dxa, float dya, float dza, float* o) {
#pragma clang fp contract(off)
    o[0] = (float)((double)in[0] * diag);
    o[1] = (float)((double)in[1] * diag);
    o[2] = in[2] * dza;
    o[3] = expf(in[3]) * dxa;
    o[4] = expf(in[4]) * dya;
    o[5] = expf(in[5]) * dza;
    o[6] = in[6];
}

__global__ __launch_bounds__(64) void gl_score_kernel(const float* __restrict__ box, const float* __restrict__ gt, int D,
                                                      int B, double diag, float dxa, float dya, float dza,
                                                      float* __restrict__ pred, float* __restrict__ overlap,
                                                      double* __restrict__ variance, double* __restrict__ mean_overlap) {
    __shared__ double col[64][9];             // the seven variance columns and the overlap of the current 64 draws
    const int b = blockIdx.x, lane = threadIdx.x;
    float g[7];
    gl_decode(gt + 7 * (size_t)b, diag, dxa, dya, dza, g);
    const double gt_angle = (double)gt[7 * (size_t)b + 6];
    const double two_pi = 2.0 * 3.14159265358979323846;
    double sum = 0.0, mean = 0.0, ssq = 0.0;  // lane c < 7: column c; lane 7: the overlap
    for (int pass = 0; pass < 2; ++pass) {
        for (int d0 = 0; d0 < D; d0 += 64) {
            const int d = d0 + lane;
            if (d < D) {
                const float* in = box + ((size_t)d * B + b) * 9;
                float p[7];
                gl_decode(in, diag, dxa, dya, dza, p);
                if (pass == 0) {
                    float* o = pred + ((size_t)d * B + b) * 9;
#pragma unroll
                    for (int k = 0; k < 7; ++k) o[k] = p[k];
                    o[7] = in[7];
                    o[8] = in[8];
                    const float ov = gl_iou(g, p);
                    overlap[(size_t)d * B + b] = ov;
                    col[lane][7] = (double)ov;
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) col[lane][k] = (double)p[k];
                const double w = (double)p[6] - gt_angle;
                col[lane][6] = sin(w - floor(w / two_pi) * two_pi);
            }
            __syncthreads();
            const int nd = D - d0 < 64 ? D - d0 : 64;
            if (lane < 8) {
                if (pass == 0) {
                    for (int i = 0; i < nd; ++i) sum += col[i][lane];
                } else if (lane < 7) {
                    for (int i = 0; i < nd; ++i) {
                        const double e = col[i][lane] - mean;
                        ssq += e * e;
                    }
                }
            }
            __syncthreads();
        }
        if (pass == 0) mean = sum / (double)D;
    }
    if (lane < 7) variance[7 * (size_t)b + lane] = ssq / (double)D;
    if (lane == 7) mean_overlap[b] = mean;
}

}  // namespace

extern "C" int lc_segment_center_fwd(const float* points, const int32_t* offsets, int B, int64_t total, double sx, double sy,
                                     double sz, float* out, float* mean, lc_stream_t s) {
    if (!points || !offsets || !out || !mean || B < 1 || total < 1) return LC_EINVAL;
    if (!(sx > 0.0) || !(sy > 0.0) || !(sz > 0.0)) return LC_EINVAL;
    if (total > (int64_t)0x7fffffff) return LC_EUNSUP;    // offsets are int32
    hipLaunchKernelGGL(gl_center_kernel, dim3(B), dim3(256), 0, lc_s(s), points, offsets, (long long)total, sx, sy, sz, out,
                       mean);
    return lc_launch_status();
}

extern "C" int lc_glenet_trunk_fwd(const float* norm, int64_t total, const int32_t* offsets, const int32_t* choice, int B,
                                   int K, int64_t R, const float* w1, const float* b1, const float* w2, const float* b2,
                                   const float* w3, const float* b3, const float* sw1, const float* sb1, const float* sw2,
                                   const float* sb2, const float* sw3, const float* sb3, float* featA, float* featS,
                                   lc_stream_t s) {
    if (!norm || !offsets || !choice || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !sw1 || !sb1 || !sw2 || !sb2 || !sw3 ||
        !sb3 || !featA || !featS || B < 1 || K < 1 || R < 1 || total < 1)
        return LC_EINVAL;
    if (total > (int64_t)0x7fffffff || R > (int64_t)0x7fffffff || K >= (1 << 24)) return LC_EUNSUP;
    if (!lc_aligned16(w2) || !lc_aligned16(w3)) return LC_EUNSUP;      // their rows are read as 128-bit quads
    hipLaunchKernelGGL(gl_trunk_kernel, dim3((unsigned)R), dim3(256), 0, lc_s(s), norm, (long long)total, offsets, choice, B, K,
                       (long long)R, w1, b1, w2, b2, w3, b3, sw1, sb1, sw2, sb2, sw3, sb3, featA, featS);
    return lc_launch_status();
}

extern "C" int lc_rbox_inter_fwd(const float* corners_g, const float* corners_q, int N, float* pts, int32_t* cnt, float* area,
                                 lc_stream_t s) {
    if (!corners_g || !corners_q || !pts || !cnt || !area || N < 1) return LC_EINVAL;
    hipLaunchKernelGGL(gl_inter_kernel, dim3((N + 63) / 64), dim3(64), 0, lc_s(s), corners_g, corners_q, N, pts, cnt, area);
    return lc_launch_status();
}

extern "C" int lc_riou3d_paired_fwd(const float* g, int ldg, const float* q, int ldq, int N, float* iou, lc_stream_t s) {
    if (!g || !q || !iou || N < 1 || ldg < 7 || ldq < 7) return LC_EINVAL;
    hipLaunchKernelGGL(gl_iou_kernel, dim3((N + 63) / 64), dim3(64), 0, lc_s(s), g, ldg, q, ldq, N, iou);
    return lc_launch_status();
}

extern "C" int lc_glenet_score_fwd(const float* box, const float* gt, int D, int B, double diag, float dxa, float dya,
                                   float dza, float* pred, float* overlap, double* variance, double* mean_overlap,
                                   lc_stream_t s) {
    if (!box || !gt || !pred || !overlap || !variance || !mean_overlap || D < 1 || B < 1) return LC_EINVAL;
    if (!(diag > 0.0) || !(dxa > 0.f) || !(dya > 0.f) || !(dza > 0.f)) return LC_EINVAL;
    hipLaunchKernelGGL(gl_score_kernel, dim3(B), dim3(64), 0, lc_s(s), box, gt, D, B, diag, dxa, dya, dza, pred, overlap,
                       variance, mean_overlap);
    return lc_launch_status();
}
