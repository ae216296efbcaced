// MeanFlow training (lidargen/models/flows/mean_flow.py MeanFlow.loss): the tangent (forward-mode) evaluation of
// MFEfficientUNet next to its primal, u, du/dt = jvp(model, (z, t, r), (v, 1, 0)), and the backward of the one op the
// training graph of that model adds to EfficientUNet's (the q / k RMSNorm).  The linear ops of the network (ring / 1x1
// convs, FIR resampling, concatenation) take their tangents through their existing kernels; the three nonlinear ones are
// here:
//
//  * lc_groupnorm_jvp_stats / lc_groupnorm_jvp_apply_train: y = silu?((GN(x) gamma + beta)(1 + s) + sh) and its tangent
//    dy along (dx, ds, dsh).  The statistics pass reads x and dx once and leaves per-(sample, group, chunk) fp64 partials
//    of sum(x - p), sum((x - p)^2), sum(dx), sum((x - p) dx) (p = the group's first element).  The first two are formed
//    exactly as lc_groupnorm_stats forms them (same chunks, same lane order), so mean / rstd / y are GroupNormAct's.
//    With n = (x - mu) rho:  dn = rho (dx - mean(dx) - n mean(n dx)),  da = dn gamma (1 + s) + (n gamma + beta) ds + dsh,
//    dy = silu'(a) da.
//  * lc_qk_norm_cm_jvp / lc_qk_norm_cm_bwd: y = sqrt(d) g v / max(||v||, 1e-12) per (sample, head, token).  Its Jacobian
//    J = sqrt(d) g / ||v|| (I - v~ v~^T) is symmetric, so tangent and backward are the same projection; dL/dg =
//    sum gy . y / g as per-block fp64 partials, reduced by one block in a fixed order (no atomics).
//  * lc_attention_jvp_fwd: flash attention with its tangent in one pass over the keys.  Per query row, with online-softmax
//    rescaling: l = sum p, O = sum p v, T = sum p (dS v + dv), mu = sum p dS;  o = O / l, do = T / l - (mu / l) o, where
//    dS = scale (dq^T k + q^T dk).  Also the base-2 log-sum-exp lc_attention_bwd* read (as lc_attention_train_fwd).
//    Exact fp32 on the vector ALUs (fma): 8 channels per lane, the lanes of a query row adjacent (4 for heads of <= 32
//    channels, 8 for <= 64), 256 lanes per block, 16-key tiles of k, dk, v, dv in LDS.
#include "common.h"
#include "flow_jvp_route.h"

namespace {

// ---- GroupNorm ----------------------------------------------------------------------------------------------------------
// (the chunking of the statistics partials: gn_chunk_elems / gn_chunks of common.h, shared with norm.hip)
// (the launch shape of the apply pass: lc_gn_apply_grid of gn_apply_route.h, norm.hip's, so the partial maxima of |y| come
//  out in the same count and order; the branches below: flow_jvp_route.h, which lc_groupnorm_jvp_route reports)

__global__ __launch_bounds__(256) void gn_jvp_stats_kernel(const float* __restrict__ x, long long x_bs,
                                                          const float* __restrict__ dx, long long dx_bs,
                                                          double* __restrict__ part, int C, int G, long long HW, int nch,
                                                          int chunk_elems) {
    const int chunk = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int cpg = C / G;
    const long long n = (long long)cpg * HW;
    const float* p = x + b * x_bs + (long long)g * n;
    const float* dp = dx + b * dx_bs + (long long)g * n;
    const long long lo = (long long)chunk * chunk_elems;
    const long long hi = (lo + chunk_elems < n) ? lo + chunk_elems : n;
    const float piv = p[0];
    float s = 0.f, q = 0.f, sd = 0.f, sxd = 0.f;
    if (lc_gnj_scalar_causes(n, (int)(reinterpret_cast<uintptr_t>(p) & 15)) == 0) {
        const bool dvec = lc_gnj_dvec((int)(reinterpret_cast<uintptr_t>(dp) & 15));
        for (long long i = lo + threadIdx.x * 4; i < hi; i += 1024) {
            f32x4 v = *reinterpret_cast<const f32x4*>(p + i);
            f32x4 d;
            if (dvec) d = *reinterpret_cast<const f32x4*>(dp + i);
            else { d.x = dp[i]; d.y = dp[i + 1]; d.z = dp[i + 2]; d.w = dp[i + 3]; }
            v.x -= piv; v.y -= piv; v.z -= piv; v.w -= piv;
            s += (v.x + v.y) + (v.z + v.w);
            q += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            sd += (d.x + d.y) + (d.z + d.w);
            sxd += (v.x * d.x + v.y * d.y) + (v.z * d.z + v.w * d.w);
        }
    } else {
        for (long long i = lo + threadIdx.x; i < hi; i += 256) {
            const float v = p[i] - piv, d = dp[i];
            s += v; q += v * v;
            sd += d; sxd += v * d;
        }
    }
    const double r0 = lc_wave_sum((double)s), r1 = lc_wave_sum((double)q);
    const double r2 = lc_wave_sum((double)sd), r3 = lc_wave_sum((double)sxd);
    __shared__ double sh[16];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[w] = r0; sh[4 + w] = r1; sh[8 + w] = r2; sh[12 + w] = r3; }
    __syncthreads();
    if (threadIdx.x < 4) {               // one 64-bit store per lane (a 128-bit store here sat right before the LDS read
        const int j = threadIdx.x;       // that overwrites its data registers: tests/test_isa_audit.py)
        part[(((long long)b * G + g) * nch + chunk) * 4 + j] = (sh[4 * j] + sh[4 * j + 1]) + (sh[4 * j + 2] + sh[4 * j + 3]);
    }
}

// one block per (b, cpb channels of one group, slab of the H*W plane) -- norm.hip gn_apply_kernel's decomposition
__global__ __launch_bounds__(256) void gn_jvp_apply_kernel(
    const float* __restrict__ x, long long x_bs, const float* __restrict__ dx, long long dx_bs,
    const double* __restrict__ part, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ dscale,
    const float* __restrict__ dshift, long long ss_bs, float* __restrict__ y, long long y_bs, float* __restrict__ dy,
    long long dy_bs, int C, int G, long long HW, int nch, float eps, int act, int cpb, float* mr_out, float* amax_out,
    float* damax_out) {
    const int c_first = blockIdx.y * cpb, b = blockIdx.z;
    float am = 0.0f, dam = 0.0f;
    const int cpg = C / G, g = c_first / cpg;
    const double* pp = part + ((long long)b * G + g) * nch * 4;
    double s = 0.0, q = 0.0, sd = 0.0, sxd = 0.0;
    for (int i = 0; i < nch; ++i) { s += pp[4 * i]; q += pp[4 * i + 1]; sd += pp[4 * i + 2]; sxd += pp[4 * i + 3]; }
    const double n = (double)cpg * (double)HW;
    const double dm = s / n;                                   // mean of (x - pivot)
    double var = q / n - dm * dm;
    if (var < 0.0) var = 0.0;
    const double rstd_d = 1.0 / sqrt(var + (double)eps);
    const float rstd = (float)rstd_d;
    const float mu = (float)((double)x[b * x_bs + (long long)g * cpg * HW] + dm);
    // mean(dx) and mean(n dx) = rho (E[(x - p) dx] - E[x - p] E[dx])
    const double mdx_d = sd / n;
    const float mdx = (float)mdx_d;
    const float mndx = (float)(rstd_d * (sxd / n - dm * mdx_d));
    if (mr_out && blockIdx.x == 0 && c_first == g * cpg && threadIdx.x == 0) {
        mr_out[2 * (b * G + g)] = mu;
        mr_out[2 * (b * G + g) + 1] = rstd;
    }
    const long long per = (HW + gridDim.x - 1) / gridDim.x;
    const long long lo = blockIdx.x * per;
    const long long hi = lo + per < HW ? lo + per : HW;
    for (int c = c_first; c < c_first + cpb; ++c) {
        const float ga = gamma ? gamma[c] : 1.0f, be = beta ? beta[c] : 0.0f;
        const float sc = scale ? 1.0f + scale[b * ss_bs + c] : 1.0f;
        const float sh = shift ? shift[b * ss_bs + c] : 0.0f;
        const float dsc = dscale ? dscale[b * ss_bs + c] : 0.0f;
        const float dsh = dshift ? dshift[b * ss_bs + c] : 0.0f;
        const float gsc = ga * sc;
        const float* xp = x + b * x_bs + (long long)c * HW;
        const float* dxp = dx + b * dx_bs + (long long)c * HW;
        float* yp = y + b * y_bs + (long long)c * HW;
        float* dyp = dy + b * dy_bs + (long long)c * HW;
        for (long long i = lo + threadIdx.x; i < hi; i += 256) {
            const float v = xp[i];
            const float nrm = (v - mu) * rstd;
            float t = nrm * ga + be;
            const float aff = t;
            t = t * sc + sh;
            const float dn = rstd * (dxp[i] - mdx - nrm * mndx);
            float dt = dn * gsc + aff * dsc + dsh;
            float r = t;
            if (act) {
                const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-t));
                r = t * sg;
                dt *= sg * (1.0f + t * (1.0f - sg));
            }
            yp[i] = r;
            dyp[i] = dt;
            am = fmaxf(am, fabsf(r));
            dam = fmaxf(dam, fabsf(dt));
        }
    }
    const long long slot = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (amax_out) lc_block_amax_store(am, amax_out + slot);
    __syncthreads();                     // (the two calls share lc_block_amax_store's LDS words)
    if (damax_out) lc_block_amax_store(dam, damax_out + slot);
}

// ---- q / k RMSNorm ------------------------------------------------------------------------------------------------------
struct QkArgs {
    const float* x; long long x_bs, x_cs;
    const float* dx; long long dx_bs, dx_cs;      // tangent (jvp) or output gradient (bwd); may be NULL in the jvp
    const float* g;
    float* y; long long y_bs, y_cs;               // jvp: the primal (may be NULL); bwd: unused
    float* dy; long long dy_bs, dy_cs;            // jvp: the tangent; bwd: the input gradient
    double* dg_part;                              // bwd: one fp64 partial of dL/dg per block (may be NULL)
    int heads, d, L;
};

template <int DMAX, bool BWD>
__global__ __launch_bounds__(256) void qk_norm_jvp_kernel(QkArgs a) {
    const int t = blockIdx.x * LC_QKJ_TOKENS + threadIdx.x;
    const int bh = blockIdx.y;
    const int b = bh / a.heads, h = bh - b * a.heads;
    double gpart = 0.0;
    if (t < a.L) {
        const float* xp = a.x + b * a.x_bs + (long long)h * a.d * a.x_cs + t;
        const double g = (double)a.g[0];
        float v[DMAX];
        double ss = 0.0;
#pragma unroll
        for (int c = 0; c < DMAX; ++c) {
            v[c] = c < a.d ? xp[c * a.x_cs] : 0.0f;
            ss = fma((double)v[c], (double)v[c], ss);
        }
        const double nrm = sqrt(ss);
        const double den = fmax(nrm, 1e-12);
        const double s = sqrt((double)a.d) * g / den;          // lc_qk_norm_cm_fwd's factor
        if (!BWD && a.y) {
            float* yp = a.y + b * a.y_bs + (long long)h * a.d * a.y_cs + t;
#pragma unroll
            for (int c = 0; c < DMAX; ++c)
                if (c < a.d) yp[c * a.y_cs] = (float)((double)v[c] * s);
        }
        if (a.dx) {
            const float* dp = a.dx + b * a.dx_bs + (long long)h * a.d * a.dx_cs + t;
            float w[DMAX];
            double vd = 0.0;
#pragma unroll
            for (int c = 0; c < DMAX; ++c) {
                w[c] = c < a.d ? dp[c * a.dx_cs] : 0.0f;
                vd = fma((double)v[c], (double)w[c], vd);
            }
            // J w = s (w - v (v . w) / ||v||^2) while ||v|| > 1e-12; below, the clamped map is linear: s w
            const double proj = nrm > 1e-12 ? vd / ss : 0.0;
            float* op = a.dy + b * a.dy_bs + (long long)h * a.d * a.dy_cs + t;
#pragma unroll
            for (int c = 0; c < DMAX; ++c)
                if (c < a.d) op[c * a.dy_cs] = (float)(s * ((double)w[c] - (double)v[c] * proj));
            // dL/dg = sum gy . y / g = sqrt(d) (v . gy) / max(||v||, 1e-12)
            if (BWD) gpart = sqrt((double)a.d) * vd / den;
        }
    }
    if (BWD && a.dg_part) {
        gpart = lc_wave_sum(gpart);
        __shared__ double wsum[4];
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = gpart;
        __syncthreads();
        if (threadIdx.x == 0)
            a.dg_part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
}

// one block: the partials in a fixed order (lane-strided, then the wave / block tree) -> dg[0]
__global__ __launch_bounds__(256) void qk_norm_dg_reduce_kernel(const double* __restrict__ part, long long n,
                                                               float* __restrict__ dg) {
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += part[i];
    s = lc_wave_sum(s);
    __shared__ double wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) dg[0] = (float)((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}

// ---- attention ----------------------------------------------------------------------------------------------------------
constexpr int JK = LC_ATTNJ_JK;      // keys per LDS tile

struct AttnJvpArgs {
    const float *q, *k, *v, *dq, *dk, *dv;
    float *o, *lse, *dout;
    int Lq, Lk, dqk, dvc;
    float scale, qscale;    // qscale = scale * log2(e)
};

// D = padded head width (32 or 64) of q / k and v alike; lane j of a query row's LPQ lanes owns channels 8j .. 8j + 7
template <int D>
__global__ __launch_bounds__(256) void attn_jvp_kernel(AttnJvpArgs a) {
    constexpr int PC = LC_ATTNJ_PC, LPQ = D / PC, QB = lc_attnj_rows(D);
    __shared__ float ks[D][JK + 1], dks[D][JK + 1], vs[D][JK + 1], dvs[D][JK + 1];
    const int bh = blockIdx.y;
    const int lj = threadIdx.x & (LPQ - 1);
    const int t = blockIdx.x * QB + threadIdx.x / LPQ;
    const bool tok = t < a.Lq;
    const long long qb = (long long)bh * a.dqk * a.Lq, kb = (long long)bh * a.dqk * a.Lk;
    const long long vb = (long long)bh * a.dvc * a.Lk, ob = (long long)bh * a.dvc * a.Lq;
    const int c0 = lj * PC;

    float qr[PC], dqr[PC], O[PC], T[PC];
#pragma unroll
    for (int i = 0; i < PC; ++i) {
        const int c = c0 + i;
        const bool ok = tok && c < a.dqk;
        qr[i] = ok ? a.q[qb + (long long)c * a.Lq + t] : 0.0f;
        dqr[i] = ok ? a.dq[qb + (long long)c * a.Lq + t] : 0.0f;
        O[i] = 0.0f;
        T[i] = 0.0f;
    }
    float m = -INFINITY, l = 0.0f, mu = 0.0f;

    for (int k0 = 0; k0 < a.Lk; k0 += JK) {
        __syncthreads();                                 // the previous tile is consumed
        for (int e = threadIdx.x; e < D * JK; e += 256) {
            const int c = e / JK, s = e - c * JK, key = k0 + s;
            const bool kin = key < a.Lk;
            const bool cq = kin && c < a.dqk, cv = kin && c < a.dvc;
            ks[c][s] = cq ? a.k[kb + (long long)c * a.Lk + key] : 0.0f;
            dks[c][s] = cq ? a.dk[kb + (long long)c * a.Lk + key] : 0.0f;
            vs[c][s] = cv ? a.v[vb + (long long)c * a.Lk + key] : 0.0f;
            dvs[c][s] = cv ? a.dv[vb + (long long)c * a.Lk + key] : 0.0f;
        }
        __syncthreads();
        const int nk = lc_attnj_tile_keys(a.Lk, k0);
        // qk[s]: the unscaled q . k.  The exponent of p is formed below as fma(qk, qscale, -m): one rounding of the
        // DIFFERENCE.  Rounding qk * qscale first costs half an ulp of the score itself, 2^-16 at a common offset of 500 --
        // a relative error of 1e-5 in p that differs from key to key (tests/test_flow_jvp_edges.py, the offset500 rows).
        // The running maximum is still the rounded product: its rounding is common to every key of the row and cancels
        // in O / l; lse = m + log2(l) gains what l carries of it.
        float qk[JK], ds[JK];
        float mt = m;
#pragma unroll
        for (int s = 0; s < JK; ++s) {
            float sp = 0.0f, dp = 0.0f;
#pragma unroll
            for (int i = 0; i < PC; ++i) {
                const float kk = ks[c0 + i][s];
                sp = fmaf(qr[i], kk, sp);
                dp = fmaf(dqr[i], kk, dp);
                dp = fmaf(qr[i], dks[c0 + i][s], dp);
            }
#pragma unroll
            for (int o = 1; o < LPQ; o <<= 1) {
                sp += __shfl_xor(sp, o, 64);
                dp += __shfl_xor(dp, o, 64);
            }
            qk[s] = sp;
            ds[s] = dp * a.scale;
            mt = fmaxf(mt, s < nk ? sp * a.qscale : -INFINITY);
        }
        const float alpha = exp2f(m - mt);               // 0 on the first tile (m = -inf, mt finite)
        m = mt;
        l *= alpha;
        mu *= alpha;
#pragma unroll
        for (int i = 0; i < PC; ++i) { O[i] *= alpha; T[i] *= alpha; }
#pragma unroll
        for (int s = 0; s < JK; ++s) {
            const float p = s < nk ? exp2f(fmaf(qk[s], a.qscale, -m)) : 0.0f;      // 0 for keys past Lk
            l += p;
            mu = fmaf(p, ds[s], mu);
            const float pds = p * ds[s];
#pragma unroll
            for (int i = 0; i < PC; ++i) {
                const float vv = vs[c0 + i][s];
                O[i] = fmaf(p, vv, O[i]);
                T[i] = fmaf(pds, vv, fmaf(p, dvs[c0 + i][s], T[i]));
            }
        }
    }
    if (!tok) return;
    const float il = 1.0f / l;
    const float mul = mu * il;
#pragma unroll
    for (int i = 0; i < PC; ++i) {
        const int c = c0 + i;
        if (c < a.dvc) {
            const float oo = O[i] * il;
            a.o[ob + (long long)c * a.Lq + t] = oo;
            a.dout[ob + (long long)c * a.Lq + t] = fmaf(-mul, oo, T[i] * il);
        }
    }
    if (lj == 0) a.lse[(long long)bh * a.Lq + t] = m + log2f(l);
}

}  // namespace

// ---- entry points ---------------------------------------------------------------------------------------------------------
extern "C" int64_t lc_groupnorm_jvp_partials_elems(int B, int C, int H, int W, int G) {
    if (B <= 0 || G <= 0 || C <= 0 || C % G || H <= 0 || W <= 0) return 0;
    return (int64_t)B * G * gn_chunks(B, G, (long long)(C / G) * H * W) * 4;
}

extern "C" int lc_groupnorm_jvp_stats(const float* x, int64_t x_bs, const float* dx, int64_t dx_bs, double* partials,
                                      int B, int C, int H, int W, int G, lc_stream_t s) {
    if (!x || !dx || !partials || B <= 0 || C <= 0 || H <= 0 || W <= 0 || G <= 0 || C % G) return LC_EINVAL;
    if (B > 65535 || G > 65535) return LC_EUNSUP;
    const long long HW = (long long)H * W;
    const long long n = (long long)(C / G) * HW;
    const int nch = gn_chunks(B, G, n);
    hipLaunchKernelGGL(gn_jvp_stats_kernel, dim3(nch, G, B), dim3(256), 0, lc_s(s), x, (long long)x_bs, dx,
                       (long long)dx_bs, partials, C, G, HW, nch, gn_chunk_elems(B, G, n));
    return lc_launch_status();
}

extern "C" int lc_groupnorm_jvp_apply_train(const float* x, int64_t x_bs, const float* dx, int64_t dx_bs,
                                            const double* partials, const float* gamma, const float* beta,
                                            const float* scale, const float* shift, const float* dscale,
                                            const float* dshift, int64_t ss_bs, float* y, int64_t y_bs, float* dy,
                                            int64_t dy_bs, int B, int C, int H, int W, int G, float eps, int act_silu,
                                            float* mean_rstd_out, float* amax_out, float* damax_out, lc_stream_t s) {
    if (!x || !dx || !partials || !y || !dy || B <= 0 || C <= 0 || H <= 0 || W <= 0 || G <= 0 || C % G)
        return LC_EINVAL;
    if ((gamma == nullptr) != (beta == nullptr) || (dscale && !scale) || (dshift && !shift)) return LC_EINVAL;
    if (B > 65535) return LC_EUNSUP;
    const long long HW = (long long)H * W;
    const int nch = gn_chunks(B, G, (long long)(C / G) * HW);
    int slabs, cpb;
    lc_gn_apply_grid(B, C, G, HW, &slabs, &cpb);
    hipLaunchKernelGGL(gn_jvp_apply_kernel, dim3(slabs, C / cpb, B), dim3(256), 0, lc_s(s), x, (long long)x_bs, dx,
                       (long long)dx_bs, partials, gamma, beta, scale, shift, dscale, dshift, (long long)ss_bs, y,
                       (long long)y_bs, dy, (long long)dy_bs, C, G, HW, nch, eps, act_silu, cpb, mean_rstd_out, amax_out,
                       damax_out);
    return lc_launch_status();
}

static int qk_norm_launch(const QkArgs& a, int B, bool bwd, lc_stream_t s) {
    const dim3 grid(lc_qkj_blocks(a.L), B * a.heads);
#define LC_QKJ(DM)                                                                                       \
    do {                                                                                                 \
        if (bwd) hipLaunchKernelGGL((qk_norm_jvp_kernel<DM, true>), grid, dim3(256), 0, lc_s(s), a);    \
        else hipLaunchKernelGGL((qk_norm_jvp_kernel<DM, false>), grid, dim3(256), 0, lc_s(s), a);       \
    } while (0)
    switch (lc_qkj_dmax(a.d)) {
        case 16: LC_QKJ(16); break;
        case 32: LC_QKJ(32); break;
        default: LC_QKJ(64); break;
    }
#undef LC_QKJ
    return lc_launch_status();
}

extern "C" int lc_qk_norm_cm_jvp(const float* x, int64_t x_bs, int64_t x_cs, const float* dx, int64_t dx_bs,
                                 int64_t dx_cs, const float* g, float* y, int64_t y_bs, int64_t y_cs, float* dy,
                                 int64_t dy_bs, int64_t dy_cs, int B, int heads, int d, int L, lc_stream_t s) {
    if (!x || !g || B <= 0 || heads <= 0 || d <= 0 || L <= 0 || x_cs <= 0) return LC_EINVAL;
    if ((dx == nullptr) != (dy == nullptr) || (!y && !dy)) return LC_EINVAL;
    if ((y && y_cs <= 0) || (dy && (dx_cs <= 0 || dy_cs <= 0))) return LC_EINVAL;
    if (d > 64 || (long long)B * heads > 65535) return LC_EUNSUP;
    QkArgs a{x, (long long)x_bs, (long long)x_cs, dx, (long long)dx_bs, (long long)dx_cs, g, y, (long long)y_bs,
             (long long)y_cs, dy, (long long)dy_bs, (long long)dy_cs, nullptr, heads, d, L};
    return qk_norm_launch(a, B, false, s);
}

extern "C" int64_t lc_qk_norm_cm_bwd_partials(int B, int heads, int L) {
    if (B <= 0 || heads <= 0 || L <= 0) return 0;
    return (int64_t)lc_qkj_partials(B, heads, L);
}

extern "C" int lc_qk_norm_cm_bwd(const float* x, int64_t x_bs, int64_t x_cs, const float* gy, int64_t gy_bs,
                                 int64_t gy_cs, const float* g, float* gx, int64_t gx_bs, int64_t gx_cs,
                                 double* dg_partials, float* dg, int B, int heads, int d, int L, lc_stream_t s) {
    if (!x || !gy || !g || !gx || B <= 0 || heads <= 0 || d <= 0 || L <= 0 || x_cs <= 0 || gy_cs <= 0 || gx_cs <= 0)
        return LC_EINVAL;
    if ((dg_partials == nullptr) != (dg == nullptr)) return LC_EINVAL;
    if (d > 64 || (long long)B * heads > 65535) return LC_EUNSUP;
    QkArgs a{x, (long long)x_bs, (long long)x_cs, gy, (long long)gy_bs, (long long)gy_cs, g, nullptr, 0, 0, gx,
             (long long)gx_bs, (long long)gx_cs, dg_partials, heads, d, L};
    int e = qk_norm_launch(a, B, true, s);
    if (e != LC_OK || !dg) return e;
    hipLaunchKernelGGL(qk_norm_dg_reduce_kernel, dim3(1), dim3(256), 0, lc_s(s), dg_partials,
                       (long long)lc_qk_norm_cm_bwd_partials(B, heads, L), dg);
    return lc_launch_status();
}

extern "C" int lc_attention_jvp_fwd(const float* q, const float* k, const float* v, const float* dq, const float* dk,
                                    const float* dv, float* o, float* lse, float* dout, int BH, int Lq, int Lk, int dqk,
                                    int dv_ch, float scale, lc_stream_t s) {
    if (!q || !k || !v || !dq || !dk || !dv || !o || !lse || !dout || BH <= 0 || Lq <= 0 || Lk <= 0 || dqk <= 0 ||
        dv_ch <= 0)
        return LC_EINVAL;
    if (dqk > 64 || dv_ch > 64 || BH > 65535) return LC_EUNSUP;
    AttnJvpArgs a{q, k, v, dq, dk, dv, o, lse, dout, Lq, Lk, dqk, dv_ch, scale, scale * 1.4426950408889634f};
    if (lc_attnj_width(dqk, dv_ch) == 32)
        hipLaunchKernelGGL(attn_jvp_kernel<32>, dim3(lc_attnj_qblocks(Lq, 32), BH), dim3(256), 0, lc_s(s), a);
    else
        hipLaunchKernelGGL(attn_jvp_kernel<64>, dim3(lc_attnj_qblocks(Lq, 64), BH), dim3(256), 0, lc_s(s), a);
    return lc_launch_status();
}

// ---- which way a call runs (pure host code: flow_jvp_route.h) ------------------------------------------------------------
extern "C" int lc_groupnorm_jvp_route(int B, int C, int H, int W, int G, int64_t x_bs, int64_t dx_bs, int x_addr_mod16,
                                      int dx_addr_mod16, int32_t* out) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || G <= 0 || C % G) return LC_EINVAL;
    const long long n = (long long)(C / G) * H * W;
    return lc_gnj_route(B, C, H, W, G, x_bs, dx_bs, x_addr_mod16, dx_addr_mod16, gn_chunk_elems(B, G, n), gn_chunks(B, G, n),
                        out);
}

extern "C" int lc_qk_norm_cm_route(int B, int heads, int d, int L, int32_t* out) { return lc_qkj_route(B, heads, d, L, out); }

extern "C" int lc_attention_jvp_route(int BH, int Lq, int Lk, int dqk, int dv_ch, int32_t* out) {
    return lc_attnj_route(BH, Lq, Lk, dqk, dv_ch, out);
}
