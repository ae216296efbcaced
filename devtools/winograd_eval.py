"""evaluate Winograd F(2x2, 3x3) for the L1-L3 pre-split convolutions BEFORE building it.
(a) error of the f16x2-split arithmetic applied to the Winograd domain vs fp64 direct convolution on the five
layer shapes (must stay <= 2e-6 rel-L2, the per-kernel bound of the parity tests);
(b) a rate estimate per layer: matrix time at the measured MFMA rate with 16/36 of the products, memory time
with the 4x larger transformed activation (what a producer-side transform writes and the conv reads).
CPU only (numpy / torch fp32 emulation of the MFMA accumulate):  python devtools/winograd_eval.py > profiles/r03_winograd_eval.txt"""
import numpy as np
import torch

G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def split(v, scale):
    """pair_split of csrc/f16x2.h: hi = 11 significant bits, round toward zero; lo = fp16(s - hi)."""
    s = (v * np.float32(scale)).astype(np.float32)
    hi = (s.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)
    lo = (s - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def pow2_scale(a, target_log2=12):
    m = float(np.abs(a).max())
    return 2.0 ** (target_log2 + 1 - np.frexp(m)[1]) if m > 0 else 1.0


def pad_ring(x):
    x = np.concatenate([x[..., -1:], x, x[..., :1]], axis=-1)          # ring in W
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (0, 0)))                 # zeros in H


def conv_fp64(x, w):
    xp = torch.from_numpy(pad_ring(x).astype(np.float64))
    return torch.nn.functional.conv2d(xp, torch.from_numpy(w.astype(np.float64))).numpy()


def mm3(ah, al, bh, bl):
    """three-product split GEMM, fp32 accumulate (torch fp32 matmul stands in for the MFMA order)."""
    t = lambda a: torch.from_numpy(a)
    return (t(ah) @ t(bh) + t(al) @ t(bh) + t(ah) @ t(bl)).numpy()


def direct_split(x, w):
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    xs, ws = pow2_scale(x), pow2_scale(w)
    xh, xl = split(pad_ring(x), xs)
    wh, wl = split(w, ws)
    y = np.zeros((B, Co, H, W), np.float32)
    for dy in range(3):
        for dx in range(3):
            a_h, a_l = wh[:, :, dy, dx], wl[:, :, dy, dx]
            for b in range(B):
                bh = xh[b, :, dy:dy + H, dx:dx + W].reshape(Ci, -1)
                bl = xl[b, :, dy:dy + H, dx:dx + W].reshape(Ci, -1)
                y[b] += mm3(a_h, a_l, bh, bl).reshape(Co, H, W)
    return y / np.float32(xs * ws)


def winograd_split(x, w):
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    xp = pad_ring(x)                                            # [B, Ci, H+2, W+2]
    th, tw = H // 2, W // 2
    # input tiles d[b, ci, th, tw, 4, 4] -> V = BT d B  (fp32, like a producer kernel would compute it)
    idx_h = (2 * np.arange(th))[:, None] + np.arange(4)[None]
    idx_w = (2 * np.arange(tw))[:, None] + np.arange(4)[None]
    d = xp[:, :, idx_h][:, :, :, :, idx_w]                      # [B, Ci, th, 4, tw, 4]
    d = d.transpose(0, 1, 2, 4, 3, 5).astype(np.float32)        # [B, Ci, th, tw, 4, 4]
    bt = BT.astype(np.float32)
    V = np.einsum("ij,bcthjk,lk->bcthil", bt, d, bt, optimize=True).astype(np.float32)
    U = np.einsum("ij,ocjk,lk->ocil", G, w.astype(np.float64), G).astype(np.float32)   # packed once per weight version
    vs, us = pow2_scale(V), pow2_scale(U)
    Vh, Vl = split(V, vs)
    Uh, Ul = split(U, us)
    M = np.zeros((B, Co, th, tw, 4, 4), np.float32)
    for i in range(4):
        for l in range(4):
            for b in range(B):
                m = mm3(Uh[:, :, i, l], Ul[:, :, i, l], Vh[b, :, :, :, i, l].reshape(Ci, -1),
                        Vl[b, :, :, :, i, l].reshape(Ci, -1))
                M[b, :, :, :, i, l] = m.reshape(Co, th, tw)
    M = M / np.float32(vs * us)
    at = AT.astype(np.float32)
    Y = np.einsum("ij,bothjk,lk->bothil", at, M, at, optimize=True).astype(np.float32)   # [B, Co, th, tw, 2, 2]
    return Y.transpose(0, 1, 2, 4, 3, 5).reshape(B, Co, H, W), float(np.abs(V).max() / np.abs(x).max())


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


# (Ci, Co, H, W, microseconds per launch of the pre-split kernel today: devtools/conv_bench.py --ps --emit --res, batch 8,
#  gpurun_out r03e / profiles/r02_conv_microbench.txt)
SHAPES = [(128, 128, 16, 512, 65.0), (256, 256, 8, 256, 51.8), (512, 512, 4, 128, 53.1), (256, 512, 8, 256, 97.8),
          (512, 128, 8, 256, 52.3)]
MFMA_PFLOPS = 1.69       # sustained v_mfma_f32_32x32x16_f16 rate on random data (profiles/r01_e_ubench_mfma.txt)
HBM_TBS = 5.0            # what the streaming kernels of this repo reach
FIXED_US = 10.0          # dispatch + prologue + store drain of a launch (PMC r02: wave lifetime 47 of 61 us)
print("# Winograd F(2x2,3x3) with the f16x2 split -- evaluation only, nothing built (devtools/winograd_eval.py)")
print("# error: one sample, seeded N(0,1) activations after a SiLU-like positive skew, weights N(0, 1/(9 Ci)), vs fp64")
print(f"{'layer':>22s} {'direct split':>13s} {'winograd split':>15s} {'max|V|/max|x|':>14s}")
g = np.random.default_rng(0)
worst = 0.0
for Ci, Co, H, W, _ in SHAPES:
    x = g.normal(0, 1, (1, Ci, H, W)).astype(np.float32)
    x = (x * (1 / (1 + np.exp(-x)))).astype(np.float32)                      # SiLU output statistics
    w = (g.normal(0, 1, (Co, Ci, 3, 3)) / np.sqrt(9 * Ci)).astype(np.float32)
    ref = conv_fp64(x, w)
    e_d = rel(direct_split(x, w), ref)
    yw, growth = winograd_split(x, w)
    e_w = rel(yw, ref)
    worst = max(worst, e_w)
    print(f"{Ci:4d}->{Co:4d} @{H:3d}x{W:4d} {e_d:13.2e} {e_w:15.2e} {growth:14.2f}")
print(f"# worst Winograd error {worst:.2e} (bound 2e-6): {'inside' if worst <= 2e-6 else 'OUTSIDE'} the per-kernel bound")
print()
print("# rate estimate at batch 8: matrix time = 3 products x (16/36) x 2 B H W Ci Co 9 / 1.69 PFLOP/s; memory = transformed input")
print("# (16 values per 2x2 outputs = 4x the pixels, hi + lo fp16 = 4 B each) + fp32 output + fp32 residual at 5 TB/s; + 10 us fixed")
print(f"{'layer':>22s} {'now us':>8s} {'mfma us':>8s} {'mem us':>8s} {'est us':>8s} {'speed-up':>9s} {'+producer':>10s} {'net':>6s}")
tot_now = tot_est = tot_net = 0.0
COUNT = {(128, 128): 10, (256, 256): 10, (512, 512): 6, (256, 512): 1, (512, 128): 1}     # launches per step (approx.)
for Ci, Co, H, W, now in SHAPES:
    B = 8
    flop = 2.0 * B * H * W * Ci * Co * 9
    mfma = 3 * flop * (16 / 36) / (MFMA_PFLOPS * 1e15) * 1e6
    mem = (B * Ci * H * W * 4 * 4 + 2 * B * Co * H * W * 4) / (HBM_TBS * 1e12) * 1e6
    est = max(mfma, mem) + FIXED_US
    # the producer (GroupNorm apply pass) has to WRITE the transformed tiles: 3 extra copies of the activation
    prod = 3 * B * Ci * H * W * 4 / (HBM_TBS * 1e12) * 1e6
    n = COUNT[(Ci, Co)]
    tot_now += n * now
    tot_est += n * est
    tot_net += n * (est + prod)
    print(f"{Ci:4d}->{Co:4d} @{H:3d}x{W:4d} {now:8.1f} {mfma:8.1f} {mem:8.1f} {est:8.1f} {now / est:9.2f} {prod:10.1f} {now / (est + prod):6.2f}")
print(f"# over the ~28 pre-split launches of a step: {tot_now / 1e3:.2f} ms now -> {tot_est / 1e3:.2f} ms conv only = "
      f"{tot_now / tot_est:.2f}x; with the producer's extra writes {tot_net / 1e3:.2f} ms = {tot_now / tot_net:.2f}x")
print("# also not counted: the 16 frequency GEMMs need 4x the accumulator registers of the direct kernel (128 per thread at")
print("# the 64co x 256px block) and 16/9 of the weight bytes in LDS per K chunk (65 KB: its double buffer no longer fits")
print("# beside a double-buffered x tile).")
print("# DECISION (round 3): NOT built.  The arithmetic is safe (<= 5.7e-7), but at level 1 (128 channels, 16x512) the 4x")
print("# activation bytes cost what the 2.25x fewer MFMAs return; the gain sits in the 256- / 512-channel layers (~1.3-1.8x")
print("# net on ~18 launches, ~0.25 ms of a 3.9 ms step) and needs a new kernel (16 GEMMs per tile, 128 accumulators), a new")
print("# producer layout and a new weight packing -- a candidate for a later round, L2 / L3 only.")
