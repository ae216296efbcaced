// Hourglass Diffusion Transformer (HDiT, lidargen/models/dits/hdit.py): the operations the model adds to the kernels of
// the UNet path.  Every Linear of the model runs as a 1x1 conv on the channel-major token grid [B, C, h, w]
// (conv_f16x2.hip); everything else of a forward is here:
//
//  * lc_hdit_rmsnorm_fwd: RMSNorm over the channels of every token, y = x * rsqrt(mean_c x^2 + eps) * f[b, c] with
//    f = 1 + m[b, c] (AdaRMSNorm, the modulation rows of the whole run are one lc_linear_fwd) or a gain g[c], or 1.
//    Four lanes per token (a quarter of the channels each): adjacent lanes read adjacent tokens of one channel; fp64
//    sum of squares.  The row form of the
//    time path (MappingNetwork, [M, C] rows) is the same kernel with L = 1 and unit channel stride.
//  * lc_hdit_geglu_fwd: y[b, c, l] = x[b, c, l] * gelu_erf(x[b, mid + c, l]), c < mid.
//  * lc_hdit_qk_prep_fwd: in place on the q / k slices of the qkv projection, per (sample, head, token):
//    v / max(||v||_2, 1e-6) * sqrt(exp(min(scale[head], ln 100))), then the axial RoPE: channel i is rotated with
//    channel i + d/2 by theta[head, i, token] (cos / sin tables [heads, d/2, L], derived from the coords buffer).
//  * lc_hdit_na_fwd: neighbourhood attention of query (i, j) of an h x w grid over the kh x kw keys with rows
//    r0 .. r0+kh-1, r0 = clamp(i - kh/2, 0, h - kh) (clamped, not padded) and columns (j - kw/2 + s) mod w (circular):
//    what the reference's circular W padding + natten's clamped windows + crop compute.  One lane per query, the q
//    channels and the output accumulator in registers, an online fp32 softmax over the keys.  lc_hdit_na_train_fwd is
//    the same kernel storing the log-sum-exp per query as well (the backward is csrc/hdit_bwd.hip).
//  * lc_hdit_space_to_depth_fwd / lc_hdit_depth_to_space_fwd: the patch permutes of PatchMerging
//    (channel (p1*P2+p2)*C + c <- x[c, P1*y+p1, P2*x+p2]), PatchExpanding and the Detokenizer (the inverse); the
//    depth-to-space optionally ends in torch.lerp(skip, ., sigmoid(alpha[c])) (PatchExpanding).
//  * lc_hdit_tokenize_fwd: the Tokenizer, Conv2d(Cin -> C, kernel (1, P), stride (1, P), no bias) + the positional
//    embedding, exact fp32 (Cin * P products per output).
//  * lc_hdit_fourier_fwd: RandomFourierFeatures, [cos | sin](t[m] * (2 pi * freqs[i])) with the accurate sinf / cosf
//    (the arguments reach a few hundred radians).
#include "common.h"

namespace {

// 64 tokens x 4 channel quarters per block: each lane sums the squares of its quarter (fp64), the four partials meet in
// LDS and are added in a fixed order (deterministic), then each lane writes its quarter
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, long long x_bs, long long x_cs,
                                                      const float* __restrict__ f, long long f_bs, int mode,
                                                      float* y, long long y_bs, long long y_cs, int C, int L,
                                                      float eps) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, qtr = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    const int cq = (C + 3) / 4;
    const int c0 = qtr * cq, c1 = min(C, c0 + cq);
    const bool live = t < L;
    const float* xp = x + b * x_bs + (live ? t : 0);
    double ss = 0.0;
    if (live) {
#pragma unroll 4
        for (int c = c0; c < c1; ++c) {
            const double v = (double)xp[c * x_cs];
            ss = fma(v, v, ss);
        }
    }
    part[qtr][lane] = ss;
    __syncthreads();
    if (!live) return;
    ss = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    const float r = (float)(1.0 / sqrt((double)(float)(ss / C) + (double)eps));
    float* yp = y + b * y_bs + t;
    const float* fp = mode == 1 ? f + b * f_bs : f;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
        float v = xp[c * x_cs] * r;
        if (mode == 1)
            v = v * (1.0f + fp[c]);
        else if (mode == 2)
            v = v * fp[c];
        yp[c * y_cs] = v;
    }
}

__global__ __launch_bounds__(256) void geglu_kernel(const float* __restrict__ x, long long x_bs, float* y,
                                                    long long y_bs, int mid, int L) {
    const int b = blockIdx.y;
    const long long n = (long long)mid * L;
    const float* xp = x + b * x_bs;
    float* yp = y + b * y_bs;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        yp[i] = xp[i] * gelu_erf(xp[i + n]);
}

template <int D>
__global__ __launch_bounds__(256) void qk_prep_kernel(float* q, long long q_bs, long long q_cs, float* k,
                                                      long long k_bs, long long k_cs,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ cos_t,
                                                      const float* __restrict__ sin_t, int heads, int L) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const int bh = blockIdx.y;
    const int b = bh / heads, h = bh - b * heads;
    const bool is_k = blockIdx.z != 0;
    const long long cs = is_k ? k_cs : q_cs;
    float* p = (is_k ? k + b * k_bs : q + b * q_bs) + (long long)h * D * cs + t;
    float v[D];
    double ss = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        v[c] = p[c * cs];
        ss = fma((double)v[c], (double)v[c], ss);
    }
    // F.normalize(eps = 1e-6) then * scale.clamp(max = ln 100).exp().sqrt(), both rounded as torch rounds them
    const float nrm = fmaxf((float)sqrt(ss), 1e-6f);
    const float sc = sqrtf(expf(fminf(scale[h], 4.60517018598809136f)));
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = (v[c] / nrm) * sc;
    const float* ct = cos_t + (long long)h * (D / 2) * L + t;
    const float* st = sin_t + (long long)h * (D / 2) * L + t;
#pragma unroll
    for (int i = 0; i < D / 2; ++i) {
        const float c = ct[(long long)i * L], s = st[(long long)i * L];
        const float x1 = v[i], x2 = v[i + D / 2];
        p[i * cs] = x1 * c - x2 * s;
        p[(i + D / 2) * cs] = x1 * s + x2 * c;
    }
}

// LSE: also store the log-sum-exp m + log(l) of every (sample, head, query) for the backward (lc_hdit_na_train_fwd);
// o is computed by the same instructions either way
template <int D, bool LSE>
__global__ __launch_bounds__(256) void na_kernel(lc_cm_operand q, lc_cm_operand k, lc_cm_operand v, float* o,
                                                 long long o_bs, long long o_hs, long long o_cs, float* lse,
                                                 int heads, int h, int w, int kh, int kw, float scale) {
    const int L = h * w;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const int bh = blockIdx.y;
    const int b = bh / heads, hd = bh - b * heads;
    const int i = t / w, j = t - i * w;
    const float* qp = q.p + b * q.bs + hd * q.hs + t;
    const float* kp = k.p + b * k.bs + hd * k.hs;
    const float* vp = v.p + b * v.bs + hd * v.hs;
    float qr[D], acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        qr[c] = qp[c * q.cs] * scale;
        acc[c] = 0.0f;
    }
    int r0 = i - kh / 2;
    r0 = r0 < 0 ? 0 : (r0 > h - kh ? h - kh : r0);
    float m = -INFINITY, l = 0.0f;
    for (int r = r0; r < r0 + kh; ++r) {
        for (int s = 0; s < kw; ++s) {
            int col = j - kw / 2 + s;                  // kw/2 <= w: col in [-w, 2w)
            col = col < 0 ? col + w : (col >= w ? col - w : col);
            const int key = r * w + col;
            float sc = 0.0f;
#pragma unroll
            for (int c = 0; c < D; ++c) sc = fmaf(qr[c], kp[c * k.cs + key], sc);
            const float mn = fmaxf(m, sc);
            const float corr = expf(m - mn);           // 0 on the first key (m = -inf)
            const float pw = expf(sc - mn);
            l = l * corr + pw;
#pragma unroll
            for (int c = 0; c < D; ++c) acc[c] = fmaf(pw, vp[c * v.cs + key], acc[c] * corr);
            m = mn;
        }
    }
    const float inv = 1.0f / l;
    float* op = o + b * o_bs + hd * o_hs + t;
#pragma unroll
    for (int c = 0; c < D; ++c) op[c * o_cs] = acc[c] * inv;
    if (LSE) lse[(long long)bh * L + t] = m + logf(l);
}

// out[b, (p1*P2+p2)*C + c, y, x] = in[b, c, P1*y+p1, P2*x+p2]; one lane per output element
__global__ __launch_bounds__(256) void s2d_kernel(const float* __restrict__ in, long long in_bs, float* out,
                                                  long long out_bs, int C, int H, int W, int P1, int P2) {
    const int b = blockIdx.y;
    const int ho = H / P1, wo = W / P2;
    const long long n = (long long)C * H * W;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int x = (int)(e % wo);
        const long long r = e / wo;
        const int y = (int)(r % ho);
        const int co = (int)(r / ho);
        const int p = co / C, c = co - p * C;
        const int p1 = p / P2, p2 = p - p1 * P2;
        out[b * out_bs + e] = in[b * in_bs + ((long long)c * H + (long long)y * P1 + p1) * W + (long long)x * P2 + p2];
    }
}

// out[b, c, P1*y+p1, P2*x+p2] = in[b, (p1*P2+p2)*C + c, y, x]  (optionally lerp(skip, ., sigmoid(alpha[c])))
__global__ __launch_bounds__(256) void d2s_kernel(const float* __restrict__ in, long long in_bs, float* out,
                                                  long long out_bs, const float* __restrict__ skip,
                                                  long long skip_bs, const float* __restrict__ alpha, int C,
                                                  int h, int w, int P1, int P2) {
    const int b = blockIdx.y;
    const int H = h * P1, W = w * P2;
    const long long n = (long long)C * H * W;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int X = (int)(e % W);
        const long long r = e / W;
        const int Y = (int)(r % H);
        const int c = (int)(r / H);
        const int y = Y / P1, p1 = Y - y * P1, x = X / P2, p2 = X - x * P2;
        const int ci = (p1 * P2 + p2) * C + c;
        float val = in[b * in_bs + ((long long)ci * h + y) * w + x];
        if (skip) {
            const float wt = 1.0f / (1.0f + expf(-alpha[c]));
            const float s0 = skip[b * skip_bs + e];
            // torch.lerp: start + weight * (end - start) below 0.5, end - (end - start) * (1 - weight) from 0.5
            val = wt < 0.5f ? s0 + wt * (val - s0) : val - (val - s0) * (1.0f - wt);
        }
        out[b * out_bs + e] = val;
    }
}

__global__ __launch_bounds__(256) void tokenize_kernel(const float* __restrict__ x, long long x_bs,
                                                       const float* __restrict__ wt, const float* __restrict__ pe,
                                                       float* y, long long y_bs, int Cin, int C, int H, int W, int P) {
    const int b = blockIdx.y;
    const int wo = W / P;
    const long long L = (long long)H * wo;
    const long long n = (long long)C * L;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e / L);
        const long long t = e - (long long)c * L;
        const int yy = (int)(t / wo), xx = (int)(t - (long long)yy * wo);
        float acc = 0.0f;
        for (int ci = 0; ci < Cin; ++ci)
            for (int p = 0; p < P; ++p)
                acc = fmaf(wt[(c * Cin + ci) * P + p], x[b * x_bs + ((long long)ci * H + yy) * W + (long long)xx * P + p],
                           acc);
        y[b * y_bs + e] = acc + pe[e];
    }
}

__global__ __launch_bounds__(256) void fourier_kernel(const float* __restrict__ t, const float* __restrict__ freqs,
                                                      float* y, int M, int half) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= M * half) return;
    const int m = e / half, i = e - m * half;
    float f2 = 6.28318530717958648f * freqs[i];
    asm volatile("" : "+v"(f2));          // rounded as torch rounds 2 pi * freqs, then the outer product
    const float a = t[m] * f2;
    y[(long long)m * 2 * half + i] = cosf(a);
    y[(long long)m * 2 * half + half + i] = sinf(a);
}

inline int grid_for(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int lc_hdit_rmsnorm_fwd(const float* x, int64_t x_bs, int64_t x_cs, const float* f, int64_t f_bs, int mode,
                                   float* y, int64_t y_bs, int64_t y_cs, int B, int C, int L, float eps,
                                   lc_stream_t s) {
    if (!x || !y || B <= 0 || C <= 0 || L <= 0 || x_cs <= 0 || y_cs <= 0 || mode < 0 || mode > 2 || !(eps > 0.0f))
        return LC_EINVAL;
    if (mode != 0 && !f) return LC_EINVAL;
    if (B > 65535) return LC_EUNSUP;
    hipLaunchKernelGGL(rmsnorm_kernel, dim3((L + 63) / 64, B), dim3(256), 0, lc_s(s), x, (long long)x_bs,
                       (long long)x_cs, f, (long long)f_bs, mode, y, (long long)y_bs, (long long)y_cs, C, L, eps);
    return lc_launch_status();
}

extern "C" int lc_hdit_geglu_fwd(const float* x, int64_t x_bs, float* y, int64_t y_bs, int B, int mid, int L,
                                 lc_stream_t s) {
    if (!x || !y || B <= 0 || mid <= 0 || L <= 0) return LC_EINVAL;
    if (B > 65535) return LC_EUNSUP;
    hipLaunchKernelGGL(geglu_kernel, dim3(grid_for((long long)mid * L), B), dim3(256), 0, lc_s(s), x, (long long)x_bs,
                       y, (long long)y_bs, mid, L);
    return lc_launch_status();
}

extern "C" int lc_hdit_qk_prep_fwd(float* q, int64_t q_bs, int64_t q_cs, float* k, int64_t k_bs, int64_t k_cs,
                                   const float* scale, const float* cos_t, const float* sin_t, int B, int heads, int d,
                                   int L, lc_stream_t s) {
    if (!q || !k || !scale || !cos_t || !sin_t || B <= 0 || heads <= 0 || L <= 0 || q_cs <= 0 || k_cs <= 0)
        return LC_EINVAL;
    if ((d != 32 && d != 64) || (long long)B * heads > 65535) return LC_EUNSUP;
    const dim3 grid((L + 255) / 256, B * heads, 2);
    if (d == 32)
        hipLaunchKernelGGL(qk_prep_kernel<32>, grid, dim3(256), 0, lc_s(s), q, (long long)q_bs, (long long)q_cs, k,
                           (long long)k_bs, (long long)k_cs, scale, cos_t, sin_t, heads, L);
    else
        hipLaunchKernelGGL(qk_prep_kernel<64>, grid, dim3(256), 0, lc_s(s), q, (long long)q_bs, (long long)q_cs, k,
                           (long long)k_bs, (long long)k_cs, scale, cos_t, sin_t, heads, L);
    return lc_launch_status();
}

extern "C" int lc_hdit_na_fwd(const lc_cm_operand* q, const lc_cm_operand* k, const lc_cm_operand* v, float* o,
                              int64_t o_bs, int64_t o_hs, int64_t o_cs, int B, int heads, int d, int h, int w, int kh,
                              int kw, float scale, lc_stream_t s) {
    if (!q || !k || !v || !o || !q->p || !k->p || !v->p || B <= 0 || heads <= 0 || h <= 0 || w <= 0 || kh <= 0 ||
        kw <= 0)
        return LC_EINVAL;
    if (!(kh & 1) || !(kw & 1) || kh * kw > 81 || kh > h || kw / 2 > w) return LC_EUNSUP;
    if ((d != 32 && d != 64) || (long long)B * heads > 65535 || (long long)h * w >= (1ll << 30)) return LC_EUNSUP;
    const int L = h * w;
    const dim3 grid((L + 255) / 256, B * heads);
    if (d == 32)
        hipLaunchKernelGGL((na_kernel<32, false>), grid, dim3(256), 0, lc_s(s), *q, *k, *v, o, (long long)o_bs,
                           (long long)o_hs, (long long)o_cs, nullptr, heads, h, w, kh, kw, scale);
    else
        hipLaunchKernelGGL((na_kernel<64, false>), grid, dim3(256), 0, lc_s(s), *q, *k, *v, o, (long long)o_bs,
                           (long long)o_hs, (long long)o_cs, nullptr, heads, h, w, kh, kw, scale);
    return lc_launch_status();
}

extern "C" int lc_hdit_na_train_fwd(const lc_cm_operand* q, const lc_cm_operand* k, const lc_cm_operand* v, float* o,
                                    int64_t o_bs, int64_t o_hs, int64_t o_cs, float* lse, int B, int heads, int d,
                                    int h, int w, int kh, int kw, float scale, lc_stream_t s) {
    if (!q || !k || !v || !o || !lse || !q->p || !k->p || !v->p || B <= 0 || heads <= 0 || h <= 0 || w <= 0 ||
        kh <= 0 || kw <= 0)
        return LC_EINVAL;
    if (!(kh & 1) || !(kw & 1) || kh * kw > 81 || kh > h || kw / 2 > w) return LC_EUNSUP;
    if ((d != 32 && d != 64) || (long long)B * heads > 65535 || (long long)h * w >= (1ll << 30)) return LC_EUNSUP;
    const int L = h * w;
    const dim3 grid((L + 255) / 256, B * heads);
    if (d == 32)
        hipLaunchKernelGGL((na_kernel<32, true>), grid, dim3(256), 0, lc_s(s), *q, *k, *v, o, (long long)o_bs,
                           (long long)o_hs, (long long)o_cs, lse, heads, h, w, kh, kw, scale);
    else
        hipLaunchKernelGGL((na_kernel<64, true>), grid, dim3(256), 0, lc_s(s), *q, *k, *v, o, (long long)o_bs,
                           (long long)o_hs, (long long)o_cs, lse, heads, h, w, kh, kw, scale);
    return lc_launch_status();
}

extern "C" int lc_hdit_space_to_depth_fwd(const float* in, int64_t in_bs, float* out, int64_t out_bs, int B, int C,
                                          int H, int W, int P1, int P2, lc_stream_t s) {
    if (!in || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || P1 <= 0 || P2 <= 0) return LC_EINVAL;
    if (H % P1 || W % P2 || B > 65535 || (long long)C * H * W >= (1ll << 31)) return LC_EUNSUP;
    hipLaunchKernelGGL(s2d_kernel, dim3(grid_for((long long)C * H * W), B), dim3(256), 0, lc_s(s), in,
                       (long long)in_bs, out, (long long)out_bs, C, H, W, P1, P2);
    return lc_launch_status();
}

extern "C" int lc_hdit_depth_to_space_fwd(const float* in, int64_t in_bs, float* out, int64_t out_bs,
                                          const float* skip, int64_t skip_bs, const float* alpha, int B, int C, int h,
                                          int w, int P1, int P2, lc_stream_t s) {
    if (!in || !out || B <= 0 || C <= 0 || h <= 0 || w <= 0 || P1 <= 0 || P2 <= 0 || (skip && !alpha))
        return LC_EINVAL;
    if (B > 65535 || (long long)C * h * w * P1 * P2 >= (1ll << 31)) return LC_EUNSUP;
    hipLaunchKernelGGL(d2s_kernel, dim3(grid_for((long long)C * h * w * P1 * P2), B), dim3(256), 0, lc_s(s), in,
                       (long long)in_bs, out, (long long)out_bs, skip, (long long)skip_bs, alpha, C, h, w, P1, P2);
    return lc_launch_status();
}

extern "C" int lc_hdit_tokenize_fwd(const float* x, int64_t x_bs, const float* wt, const float* pe, float* y,
                                    int64_t y_bs, int B, int Cin, int C, int H, int W, int P, lc_stream_t s) {
    if (!x || !wt || !pe || !y || B <= 0 || Cin <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0) return LC_EINVAL;
    if (W % P || B > 65535 || (long long)C * H * W >= (1ll << 31) || (long long)Cin * H * W >= (1ll << 31))
        return LC_EUNSUP;
    hipLaunchKernelGGL(tokenize_kernel, dim3(grid_for((long long)C * H * (W / P)), B), dim3(256), 0, lc_s(s), x,
                       (long long)x_bs, wt, pe, y, (long long)y_bs, Cin, C, H, W, P);
    return lc_launch_status();
}

extern "C" int lc_hdit_fourier_fwd(const float* t, const float* freqs, float* y, int M, int half, lc_stream_t s) {
    if (!t || !freqs || !y || M <= 0 || half <= 0) return LC_EINVAL;
    if ((long long)M * half >= (1ll << 31)) return LC_EUNSUP;
    hipLaunchKernelGGL(fourier_kernel, dim3((M * half + 255) / 256), dim3(256), 0, lc_s(s), t, freqs, y, M, half);
    return lc_launch_status();
}
