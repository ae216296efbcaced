// MeanFlow generator (MFEfficientUNet / MeanFlow, lidargen/models/unets/efficient_mf_unet.py and
// lidargen/models/flows/mean_flow.py): the two operations the model adds to the EfficientUNet hot path.
//
//  * lc_qk_norm_cm_fwd: timm Attention(qk_norm=True, norm_layer=RMSNorm) normalises q and k of every head,
//    F.normalize(v, dim=-1) * sqrt(d) * g, on the channel-major output of the qkv projection.  One lane per token:
//    adjacent lanes read adjacent tokens of one channel (256 bytes per wave and channel), the d channels of a
//    token are held in registers, the sum of squares is accumulated in fp64 (d <= 64 products: the result is
//    the correctly rounded fp32 of the float64 formula up to one rounding), the gains are read on the device.
//  * lc_flow_step_fwd: z <- z - dt[b] * u, the update of one MeanFlow step (rounded as torch rounds it: the
//    product, then the difference -- no contraction to an fma).
#include "common.h"

namespace {

template <int DMAX>
__global__ __launch_bounds__(256) void qk_norm_cm_kernel(float* q, long long q_bs, long long q_cs, float* k,
                                                         long long k_bs, long long k_cs, const float* __restrict__ g_q,
                                                         const float* __restrict__ g_k, int heads, int d, int L) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const int bh = blockIdx.y;
    const int b = bh / heads, h = bh - b * heads;
    const bool is_k = blockIdx.z != 0;
    const long long bs = is_k ? k_bs : q_bs;
    const long long cs = is_k ? k_cs : q_cs;
    float* p = (is_k ? k : q) + b * bs + (long long)h * d * cs + t;
    const double g = (double)(is_k ? g_k[0] : g_q[0]);

    float v[DMAX];
    double ss = 0.0;
#pragma unroll
    for (int c = 0; c < DMAX; ++c) {
        v[c] = c < d ? p[c * cs] : 0.0f;
        ss = fma((double)v[c], (double)v[c], ss);
    }
    // F.normalize: v / max(||v||_2, 1e-12); RMSNorm: * sqrt(d) * g
    const double s = sqrt((double)d) * g / fmax(sqrt(ss), 1e-12);
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < d) p[c * cs] = (float)((double)v[c] * s);
}

__global__ __launch_bounds__(256) void flow_step_kernel(const float* z, long long z_bs, const float* __restrict__ u,
                                                        long long u_bs, const float* __restrict__ dt, float* out,
                                                        long long out_bs, long long n) {
    const int b = blockIdx.y;
    const float* zp = z + b * z_bs;
    const float* up = u + b * u_bs;
    float* op = out + b * out_bs;
    const float step = dt[b];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float prod = step * up[i];
        asm volatile("" : "+v"(prod));        // the rounded product: keeps the compiler from fusing it into an fma
        op[i] = zp[i] - prod;
    }
}

inline int grid_for(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int lc_qk_norm_cm_fwd(float* q, int64_t q_bs, int64_t q_cs, float* k, int64_t k_bs, int64_t k_cs,
                                 const float* g_q, const float* g_k, int B, int heads, int d, int L, lc_stream_t s) {
    if (!q || !k || !g_q || !g_k || B <= 0 || heads <= 0 || d <= 0 || L <= 0 || q_cs <= 0 || k_cs <= 0)
        return LC_EINVAL;
    if (d > 64 || (long long)B * heads > 65535) return LC_EUNSUP;
    const dim3 grid((L + 255) / 256, B * heads, 2);
    if (d <= 16)
        hipLaunchKernelGGL(qk_norm_cm_kernel<16>, grid, dim3(256), 0, lc_s(s), q, (long long)q_bs, (long long)q_cs, k,
                           (long long)k_bs, (long long)k_cs, g_q, g_k, heads, d, L);
    else if (d <= 32)
        hipLaunchKernelGGL(qk_norm_cm_kernel<32>, grid, dim3(256), 0, lc_s(s), q, (long long)q_bs, (long long)q_cs, k,
                           (long long)k_bs, (long long)k_cs, g_q, g_k, heads, d, L);
    else
        hipLaunchKernelGGL(qk_norm_cm_kernel<64>, grid, dim3(256), 0, lc_s(s), q, (long long)q_bs, (long long)q_cs, k,
                           (long long)k_bs, (long long)k_cs, g_q, g_k, heads, d, L);
    return lc_launch_status();
}

extern "C" int lc_flow_step_fwd(const float* z, int64_t z_bs, const float* u, int64_t u_bs, const float* dt, float* out,
                                int64_t out_bs, int B, int64_t n, lc_stream_t s) {
    if (!z || !u || !dt || !out || B <= 0 || n <= 0) return LC_EINVAL;
    if (B > 65535) return LC_EUNSUP;
    hipLaunchKernelGGL(flow_step_kernel, dim3(grid_for(n), B), dim3(256), 0, lc_s(s), z, (long long)z_bs, u,
                       (long long)u_bs, dt, out, (long long)out_bs, (long long)n);
    return lc_launch_status();
}
