"""GPU parity tests: every HIP kernel / module through the C ABI vs the CPU oracle on identical
seeded inputs, plus the committed golden vectors of the reference.  `pytest -m gpu`.
Tolerances: fp32 kernels (exact-fp32 MFMA, different summation order than oneDNN) rel-L2 <= 2e-5
per op and <= 1e-4 per full forward / trajectory step (north-star gate: 1e-3); integer/index
work bit-exact."""
import numpy as np
import pytest
import torch

from lidarcrafter_amd.testing import rel_l2, seeded_fill, seeded_randn, synth_points

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from lidarcrafter_amd import _lib
    import ctypes

    buf = ctypes.create_string_buffer(64)
    assert _lib.lib().lc_device_arch(buf, 64) == 0
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------- conv
@pytest.mark.parametrize("B,Ci,Co,H,W,ks", [
    (2, 5, 7, 4, 16, 3), (2, 5, 7, 4, 16, 1), (1, 32, 64, 32, 1024, 3), (2, 64, 64, 16, 128, 3),
    (2, 128, 256, 8, 256, 3), (2, 512, 512, 4, 128, 3), (1, 64, 2, 32, 256, 3),
    (2, 42, 64, 8, 64, 3), (1, 512, 256, 4, 128, 1), (2, 48, 144, 1, 8, 3), (3, 16, 32, 2, 16, 3),
    (2, 64, 96, 1, 2048, 1), (1, 32, 64, 1, 192, 1),
    (2, 96, 64, 4, 64, 1), (1, 192, 64, 8, 64, 1),      # 1x1 with a partial last 64-channel chunk
])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 12, 13, 15, 22, 23, 25, 27, 227, 427, 223, 423, 425, 412, 212, 28, 228, 33])
@pytest.mark.parametrize("prec", ["f32", "f16x2"])
def test_conv(dev, B, Ci, Co, H, W, ks, cfg, prec):
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    if prec == "f32" and cfg > 5:
        pytest.skip("pipelined tile configurations exist for the f16x2 kernel only")
    if cfg == 33 and not (ks == 3 and Ci % 16 == 0 and Ci >= 64 and Co % 64 == 0 and H % 8 == 0 and W % 64 == 0):
        pytest.skip("outside the ping-pong kernel's shapes (the launcher refuses them: test_abi)")
    x = seeded_randn(B, Ci, H, W, seed=1)
    w = seeded_randn(Co, Ci, ks, ks, seed=2) / (Ci * ks * ks) ** 0.5
    b = seeded_randn(Co, seed=3)
    res = seeded_randn(B, Co, H, W, seed=4)
    ref = (D.conv_ring(x, w, b) + res) * 0.7071
    pk = K.PackedConv()
    y = K.conv2d_ring(x.to(dev), pk, w.to(dev), b.to(dev), res=res.to(dev), out_scale=0.7071,
                      tile_cfg=cfg, precision=prec)
    assert rel_l2(y, ref) < 2e-6, rel_l2(y, ref)


def test_conv_f16x2_accuracy_vs_fp64(dev):
    """Split-fp16 conv error vs an fp64 reference is of fp32 class (not fp16 class ~5e-4), also
    for small-magnitude weights/activations (lo parts near fp16's subnormal range)."""
    from lidarcrafter_amd import ops as K

    for xs, ws in ((1.0, 1.0), (0.05, 0.02), (30.0, 4.0)):
        x = seeded_randn(2, 256, 8, 64, seed=40) * xs
        w = seeded_randn(128, 256, 3, 3, seed=41) * ws / 48.0
        ref = torch.nn.functional.conv2d(
            torch.nn.functional.pad(torch.cat([x[..., -1:], x, x[..., :1]], -1).double(),
                                    (0, 0, 1, 1)), w.double())
        e16 = rel_l2(K.conv2d_ring(x.to(dev), K.PackedConv(), w.to(dev), precision="f16x2"), ref)
        e32 = rel_l2(K.conv2d_ring(x.to(dev), K.PackedConv(), w.to(dev), precision="f32"), ref)
        assert e16 < 2e-6 and e32 < 1e-6, (xs, ws, e16, e32)


@pytest.mark.parametrize("B,Ci,Co,H,W,ks,G", [(2, 64, 64, 8, 128, 3, 8), (1, 256, 128, 8, 256, 3, 32),
                                              (2, 48, 32, 4, 64, 3, 8), (2, 512, 96, 4, 128, 1, 32),
                                              (1, 128, 64, 32, 1024, 3, 8)])
@pytest.mark.parametrize("cfg", [0, 2, 3, 5, 12, 13, 23, 25, 27, 227, 423, 225])
def test_conv_fused_groupnorm(dev, B, Ci, Co, H, W, ks, G, cfg):
    """GN(+AdaGN scale/shift)+SiLU applied inside the conv staging == GN kernel then conv."""
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D


    x = seeded_randn(B, Ci, H, W, seed=50) * 1.3 + 0.4
    w = seeded_randn(Co, Ci, ks, ks, seed=51) / (Ci * ks * ks) ** 0.5
    bias = seeded_randn(Co, seed=52)
    ga, be = 1 + 0.1 * seeded_randn(Ci, seed=53), 0.1 * seeded_randn(Ci, seed=54)
    ss = 0.3 * seeded_randn(B, 2 * Ci, seed=55)
    a = D.silu(D.group_norm(x, G, ga, be, 1e-6) * (1 + ss[:, :Ci, None, None]) + ss[:, Ci:, None, None])
    ref = D.conv_ring(a, w, bias)
    ssd = ss.to(dev)
    co = K.groupnorm_coeffs(x.to(dev), G, 1e-6, ga.to(dev), be.to(dev), ssd[:, :Ci], ssd[:, Ci:])
    y = K.conv2d_ring(x.to(dev), K.PackedConv(), w.to(dev), bias.to(dev), tile_cfg=cfg,
                      precision="f16x2", gn_coeffs=co, gn_silu=True)
    assert rel_l2(y, ref) < 3e-6, rel_l2(y, ref)
    # no activation (attention qkv projection): GN only
    ref2 = D.conv_ring(D.group_norm(x, G, ga, be, 1e-6), w, bias)
    co2 = K.groupnorm_coeffs(x.to(dev), G, 1e-6, ga.to(dev), be.to(dev))
    y2 = K.conv2d_ring(x.to(dev), K.PackedConv(), w.to(dev), bias.to(dev), tile_cfg=cfg,
                       precision="f16x2", gn_coeffs=co2, gn_silu=False)
    assert rel_l2(y2, ref2) < 3e-6, rel_l2(y2, ref2)
    # statistics handed to the conv directly (rows derived in its prologue): identical bits
    xd = x.to(dev)
    st = K.groupnorm_stats(xd, G, 1e-6, ga.to(dev), be.to(dev), ssd[:, :Ci], ssd[:, Ci:])
    y3 = K.conv2d_ring(xd, K.PackedConv(), w.to(dev), bias.to(dev), tile_cfg=cfg, precision="f16x2",
                       gn_coeffs=st, gn_silu=True)
    assert torch.equal(y3, y)
    st2 = K.groupnorm_stats(xd, G, 1e-6, ga.to(dev), be.to(dev))
    y4 = K.conv2d_ring(xd, K.PackedConv(), w.to(dev), bias.to(dev), tile_cfg=cfg, precision="f16x2",
                       gn_coeffs=st2, gn_silu=False)
    assert torch.equal(y4, y2)
    other = K.groupnorm_stats(torch.zeros(B, Ci, H, 2 * W, device=dev), G, 1e-6)
    with pytest.raises(ValueError):      # statistics of a different tensor shape are refused
        K.conv2d_ring(xd, K.PackedConv(), w.to(dev), bias.to(dev), gn_coeffs=other)


def test_conv_strided_views(dev):
    """Producer writes into a channel slice of a concat buffer; consumer reads a slice."""
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    x = seeded_randn(2, 24, 4, 64, seed=5)
    w = seeded_randn(16, 8, 3, 3, seed=6) / 8.5
    xd = x.to(dev)
    cat = torch.zeros(2, 40, 4, 64, device=dev)
    K.conv2d_ring(xd[:, 8:16], K.PackedConv(), w.to(dev), None, out=cat[:, 24:])
    ref = D.conv_ring(x[:, 8:16], w)
    assert rel_l2(cat[:, 24:], ref) < 2e-6
    assert float(cat[:, :24].abs().max()) == 0.0


def test_conv_golden(dev, golden):
    from lidarcrafter_amd import ops as K
    from tests.test_oracle_vs_golden import _fill_sd

    g = golden("ops")
    x = seeded_randn(2, 5, 4, 16, seed=11).to(dev)
    sd = _fill_sd({"weight": (7, 5, 3, 3), "bias": (7,)}, 1)
    y = K.conv2d_ring(x, K.PackedConv(), sd["weight"].to(dev), sd["bias"].to(dev))
    assert rel_l2(y, T(g["conv3_y"])) < 2e-6
    sd = _fill_sd({"weight": (7, 5, 1, 1), "bias": (7,)}, 2)
    y = K.conv2d_ring(x, K.PackedConv(), sd["weight"].to(dev), sd["bias"].to(dev))
    assert rel_l2(y, T(g["conv1_y"])) < 2e-6


# ------------------------------------------------------------------------------------- norm
@pytest.mark.parametrize("B,C,H,W,G", [(2, 16, 4, 8, 8), (2, 64, 32, 1024, 8), (1, 512, 4, 128, 8),
                                       (2, 256, 8, 256, 32), (3, 48, 1, 8, 8), (2, 96, 3, 5, 32),
                                       (8, 512, 4, 128, 8), (8, 256, 8, 256, 8), (8, 384, 4, 128, 32)])
@pytest.mark.parametrize("mode", ["affine", "ada", "plain"])
def test_groupnorm(dev, B, C, H, W, G, mode):
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    x = seeded_randn(B, C, H, W, seed=7) * 1.7 + 0.3
    ga, be = 1 + 0.1 * seeded_randn(C, seed=8), 0.1 * seeded_randn(C, seed=9)
    ss = seeded_randn(B, 2 * C, seed=10) * 0.3
    xd = x.to(dev)
    if mode == "affine":
        ref = D.silu(D.group_norm(x, G, ga, be, 1e-6))
        y = K.groupnorm(xd, G, 1e-6, ga.to(dev), be.to(dev), act_silu=True)
    elif mode == "ada":
        ref = D.silu(D.group_norm(x, G, None, None, 1e-6) * (1 + ss[:, :C, None, None])
                     + ss[:, C:, None, None])
        ssd = ss.to(dev)
        y = K.groupnorm(xd, G, 1e-6, None, None, ssd[:, :C], ssd[:, C:], act_silu=True)
    else:
        ref = D.group_norm(x, G, None, None, 1e-5)
        y = K.groupnorm(xd, G, 1e-5)
    assert rel_l2(y, ref) < 2e-6, rel_l2(y, ref)


@pytest.mark.parametrize("B,Ci,Co,H,W,ks,G,cfg", [
    (2, 64, 128, 16, 128, 3, 8, 0), (2, 64, 128, 16, 128, 3, 8, 23), (2, 64, 64, 16, 128, 3, 8, 423),
    (1, 128, 256, 8, 256, 3, 32, 25), (2, 48, 96, 5, 50, 3, 4, 13), (1, 64, 72, 3, 100, 3, 3, 15),
    (1, 64, 64, 32, 1024, 3, 8, 0), (2, 64, 512, 4, 128, 3, 8, 0), (1, 32, 64, 9, 70, 3, 8, 22),
    (2, 64, 128, 16, 128, 3, 8, 28), (1, 64, 64, 32, 1024, 3, 8, 423),
])
def test_groupnorm_from_conv_epilogue_stats(dev, B, Ci, Co, H, W, ks, G, cfg):
    """The octet statistics emitted by the pipelined conv's epilogue drive GroupNorm to the same
    result as the statistics pass over the tensor -- every pipelined tile shape, ragged planes,
    persistent tiles, an output with a large mean (pivot-shifted sums)."""
    from lidarcrafter_amd import ops as K

    x = seeded_randn(B, Ci, H, W, seed=81).to(dev)
    w = (seeded_randn(Co, Ci, ks, ks, seed=82) / (Ci * ks * ks) ** 0.5).to(dev)
    b = (seeded_randn(Co, seed=83) + 300.0).to(dev)         # |mean| >> std
    res = seeded_randn(B, Co, H, W, seed=84).to(dev)
    gamma, beta = seeded_randn(Co, seed=85).to(dev), seeded_randn(Co, seed=86).to(dev)
    ss = seeded_randn(B, 2 * Co, seed=87).to(dev) * 0.3
    y = K.conv2d_ring(x, K.PackedConv(), w, b, res=res, out_scale=0.7, tile_cfg=cfg, emit_stats=True)
    assert K._find_stats(y, G) is not None
    got = K.groupnorm(y, G, 1e-6, gamma, beta, ss[:, :Co], ss[:, Co:], act_silu=True)
    y2 = y.clone()                                           # new object: no statistics attached
    assert K._find_stats(y2, G) is None
    ref = K.groupnorm(y2, G, 1e-6, gamma, beta, ss[:, :Co], ss[:, Co:], act_silu=True)
    assert rel_l2(got, ref) < 5e-6, rel_l2(got, ref)
    yd = y.double().reshape(B, G, -1)
    mu, var = yd.mean(-1), yd.var(-1, unbiased=False)
    exact = ((yd - mu[..., None]) / (var[..., None] + 1e-6).sqrt()).reshape(B, Co, H, W)
    exact = (exact * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]) * \
        (1 + ss[:, :Co].double())[..., None, None] + ss[:, Co:].double()[..., None, None]
    exact = exact * torch.sigmoid(exact)
    assert rel_l2(got, exact.float()) < 2e-4, rel_l2(got, exact.float())   # fp32 y at mean 300
    # group sizes that are not whole octets fall back to the statistics pass
    if (Co // 3) % 8:
        assert K._find_stats(y, 3) is None


def test_groupnorm_concat_segments_and_invalidation(dev):
    """Two producers write the halves of a concat buffer (different tile shapes -> different slot
    counts); GroupNorm over the buffer folds both segments; overwriting a half drops them."""
    from lidarcrafter_amd import ops as K

    B, C, H, W, G = 2, 64, 16, 128, 8
    cat = torch.empty(B, 2 * C, H, W, device=dev)
    x = seeded_randn(B, 32, H, W, seed=91).to(dev)
    w1 = (seeded_randn(C, 32, 3, 3, seed=92) / 17.0).to(dev)
    w2 = (seeded_randn(C, 32, 3, 3, seed=93) / 17.0).to(dev)
    K.conv2d_ring(x, K.PackedConv(), w1, None, out=cat[:, :C], tile_cfg=23, emit_stats=True)
    K.conv2d_ring(x, K.PackedConv(), w2, None, out=cat[:, C:], tile_cfg=13, emit_stats=True)
    hs = K._find_stats(cat, G)
    assert hs is not None and len(hs) == 2 and hs[0].slots != hs[1].slots
    got = K.groupnorm(cat, G, 1e-6, act_silu=False)
    ref = K.groupnorm(cat.clone(), G, 1e-6, act_silu=False)
    assert rel_l2(got, ref) < 2e-6, rel_l2(got, ref)
    assert K._find_stats(cat[:, :C], G) is not None        # a half on its own also resolves
    K.resample2x(torch.zeros(B, C, H // 2, W // 2, device=dev), up=True, out=cat[:, C:])
    assert K._find_stats(cat, G) is None and K._find_stats(cat[:, :C], G) is not None
    K.conv2d_ring(x, K.PackedConv(), w1, None, out=cat[:, :C])       # no emission: stats dropped
    assert K._find_stats(cat[:, :C], G) is None
    # the 2-blocks/CU kernel emits none: the request is a no-op and GroupNorm takes the old route
    y = K.conv2d_ring(x[:, :8].contiguous(), K.PackedConv(), w1[:, :8].contiguous(), None, emit_stats=True)
    assert K._find_stats(y, G) is None


@pytest.mark.parametrize("cfg", [0, 3, 5, 13, 23, 25, 28, 223])
@pytest.mark.parametrize("B,C,H,W,G,ks", [(2, 64, 16, 128, 8, 3), (1, 64, 32, 1024, 8, 3),
                                          (2, 64, 5, 72, 4, 3), (2, 64, 8, 64, 8, 1)])
def test_conv_fused_groupnorm_from_producer_stats(dev, B, C, H, W, G, ks, cfg):
    """The consumer conv derives its fused-GroupNorm rows from the octet statistics its input's
    producers emitted (no statistics pass): same result as the two-pass route, for a single
    producer and for a concat of two (different slot counts), with AdaGN scale/shift."""
    from lidarcrafter_amd import ops as K

    if ks == 1 and cfg not in (0, 3, 5):
        pytest.skip("1x1 convs run on the 2-blocks/CU kernel")
    if ks == 3 and cfg == 28:
        Co = 32
    else:
        Co = 64
    x = seeded_randn(B, 32, H, W, seed=191).to(dev)
    w1 = (seeded_randn(C, 32, 3, 3, seed=192) / 17.0).to(dev)
    w2 = (seeded_randn(C, 32, 3, 3, seed=193) / 11.0).to(dev)
    bias1 = (seeded_randn(C, seed=194) * 2.0).to(dev)      # a mean far from the pivot
    cat = torch.empty(B, 2 * C, H, W, device=dev)
    K.conv2d_ring(x, K.PackedConv(), w1, bias1, out=cat[:, :C], tile_cfg=23, emit_stats=True)
    K.conv2d_ring(x, K.PackedConv(), w2, None, out=cat[:, C:], tile_cfg=13, emit_stats=True)
    for src, Ci, GG in ((cat[:, :C], C, G), (cat, 2 * C, 2 * G)):
        wc = (seeded_randn(Co, Ci, ks, ks, seed=195) / (Ci * ks * ks) ** 0.5).to(dev)
        ga, be = (1 + 0.1 * seeded_randn(Ci, seed=196)).to(dev), (0.1 * seeded_randn(Ci, seed=197)).to(dev)
        ss = (0.3 * seeded_randn(B, 2 * Ci, seed=198)).to(dev)
        st = K.groupnorm_stats(src, GG, 1e-6, ga, be, ss[:, :Ci], ss[:, Ci:])
        assert st._struct.partials is None and st._struct.os0      # took the producer's statistics
        got = K.conv2d_ring(src, K.PackedConv(), wc, None, tile_cfg=cfg, gn_coeffs=st, gn_silu=True)
        ref_in = src.clone()                                      # a copy carries no statistics
        st_ref = K.groupnorm_stats(ref_in, GG, 1e-6, ga, be, ss[:, :Ci], ss[:, Ci:])
        assert st_ref._struct.partials is not None
        ref = K.conv2d_ring(ref_in, K.PackedConv(), wc, None, tile_cfg=cfg, gn_coeffs=st_ref, gn_silu=True)
        assert rel_l2(got, ref) < 2e-6, rel_l2(got, ref)


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 8, 128), (1, 64, 32, 1024), (3, 64, 6, 96)])
@pytest.mark.parametrize("cfg", [0, 23, 25, 13])
def test_conv_fused_groupnorm_from_pair_stats(dev, B, C, H, W, cfg):
    """GroupNorm32 at 64 / 128 channels has 2 / 4 channels per group: the producers leave one entry
    per channel PAIR (emit_stats=2) and the consumer conv folds those -- same result as the two-pass
    route; single producer (2 per group), concat of two producers with different tiles (4 per group);
    the apply kernel folds the same pair entries (round 5: entries of any unit that divides a group)."""
    from lidarcrafter_amd import ops as K

    x = seeded_randn(B, 32, H, W, seed=291).to(dev)
    w1 = (seeded_randn(C, 32, 3, 3, seed=292) / 17.0).to(dev)
    w2 = (seeded_randn(C, 32, 3, 3, seed=293) / 11.0).to(dev)
    bias1 = (seeded_randn(C, seed=294) * 2.0).to(dev)
    res = seeded_randn(B, C, H, W, seed=299).to(dev)
    cat = torch.empty(B, 2 * C, H, W, device=dev)
    K.conv2d_ring(x, K.PackedConv(), w1, bias1, res=res, out=cat[:, :C], tile_cfg=23 if H % 4 == 0 else 25,
                  emit_stats=2)
    K.conv2d_ring(x, K.PackedConv(), w2, None, out=cat[:, C:], tile_cfg=13, emit_stats=2)
    assert K._find_stats(cat, 32) is not None and K._find_stats(cat, 32, octet_groups=True) is not None
    assert K._find_stats(cat, 16, octet_groups=True) is not None      # (whole-octet groups from pair entries)
    assert K._find_stats(cat, 128) is None           # (one channel per group: half a pair entry)
    for src, Ci in ((cat[:, :C], C), (cat, 2 * C)):
        wc = (seeded_randn(64, Ci, 3, 3, seed=295) / (Ci * 9) ** 0.5).to(dev)
        ga, be = (1 + 0.1 * seeded_randn(Ci, seed=296)).to(dev), (0.1 * seeded_randn(Ci, seed=297)).to(dev)
        ss = (0.3 * seeded_randn(B, 2 * Ci, seed=298)).to(dev)
        st = K.groupnorm_stats(src, 32, 1e-6, ga, be, ss[:, :Ci], ss[:, Ci:])
        assert st._struct.partials is None and st._struct.os0      # took the producers' pair entries
        got = K.conv2d_ring(src, K.PackedConv(), wc, None, tile_cfg=cfg, gn_coeffs=st, gn_silu=True)
        ref_in = src.clone()
        st_ref = K.groupnorm_stats(ref_in, 32, 1e-6, ga, be, ss[:, :Ci], ss[:, Ci:])
        assert st_ref._struct.partials is not None
        ref = K.conv2d_ring(ref_in, K.PackedConv(), wc, None, tile_cfg=cfg, gn_coeffs=st_ref, gn_silu=True)
        assert rel_l2(got, ref) < 2e-6, rel_l2(got, ref)
    # the apply kernel from the same pair entries against its own statistics pass
    y = K.groupnorm(cat, 32, 1e-6, act_silu=True)
    assert rel_l2(y, K.groupnorm(cat.clone(), 32, 1e-6, act_silu=True)) < 2e-6
    # ... and the pre-split apply pass: 4 channels per group over the concat (one group per wave), 2 over its first half
    for src, Ci in ((cat[:, :C], C), (cat, 2 * C)):
        wc = (seeded_randn(64, Ci, 3, 3, seed=295) / (Ci * 9) ** 0.5).to(dev)
        pk1, pk2 = K.PackedConv(), K.PackedConv()
        s1 = K.groupnorm(src, 32, 1e-6, act_silu=True, split_for=pk1)
        s2 = K.groupnorm(src.clone(), 32, 1e-6, act_silu=True, split_for=pk2)
        assert isinstance(s1, K.SplitAct) and isinstance(s2, K.SplitAct)
        assert rel_l2(K.conv2d_ring(s1, pk1, wc, None), K.conv2d_ring(s2, pk2, wc, None)) < 2e-6


@pytest.mark.parametrize("B,Ci,Co,H,W", [(8, 512, 512, 1, 512), (2, 128, 64, 32, 256), (1, 64, 72, 6, 50), (3, 96, 256, 4, 128),
                                         (2, 256, 512, 1, 100)])
@pytest.mark.parametrize("cfg", [0, 3, 5, 1, 23])
def test_conv1x1_statistics_entries(dev, B, Ci, Co, H, W, cfg):
    """Octet entries from 1x1 launches -- also the non-pipelined kernel's (tiles 1 ... 5: it writes them since round 5;
    the token projections behind the attention blocks then need no statistics pass): every entry recomputed from the
    stored output (bias, residual, output scale, ragged planes and channel tails), output identical to the launch
    without entries, and a GroupNorm fed from them against the statistics-pass route."""
    from lidarcrafter_amd import ops as K

    x = (seeded_randn(B, Ci, H, W, seed=611) * 1.2 + 0.3).to(dev)
    w = (seeded_randn(Co, Ci, 1, 1, seed=612) / Ci ** 0.5).to(dev)
    bias = seeded_randn(Co, seed=613).to(dev)
    res = seeded_randn(B, Co, H, W, seed=614).to(dev)
    pk = K.PackedConv()
    y0 = K.conv2d_ring(x, pk, w, bias, res=res, out_scale=0.7071, tile_cfg=cfg)
    y = K.conv2d_ring(x, pk, w, bias, res=res, out_scale=0.7071, tile_cfg=cfg, emit_stats=True)
    assert torch.equal(y, y0)
    d = getattr(y, "_lc_gnstats", None)
    if cfg in (3, 5, 1) or (cfg == 0 and (B, Ci, Co, H, W) == (8, 512, 512, 1, 512)):
        assert d, "the non-pipelined kernel left no entries"
    if not d:
        return
    h = d[(0, Co)]
    assert h.unit == 8 and tuple(h.buf.shape) == (B, Co // 8, h.slots, 4)
    e = h.buf.double()
    n, tot = e[..., 1], e[..., 0] * e[..., 1] + e[..., 2]
    sq = e[..., 3] + 2 * e[..., 0] * e[..., 2] + e[..., 0] ** 2 * e[..., 1]
    yo = y.double().view(B, Co // 8, -1)
    assert bool((n.sum(-1) == 8.0 * H * W).all())
    assert float((tot.sum(-1) - yo.sum(-1)).abs().max()) < 2e-3 * (H * W) ** 0.5
    assert float(((sq.sum(-1) - (yo * yo).sum(-1)).abs() / (yo * yo).sum(-1)).max()) < 1e-5
    G = Co // 8
    assert rel_l2(K.groupnorm(y, G, 1e-6, act_silu=True), K.groupnorm(y.clone(), G, 1e-6, act_silu=True)) < 2e-6


@pytest.mark.parametrize("unit", [8, 2])
def test_epilogue_statistics_entries_under_load(dev, unit):
    """Every entry the deferred epilogue writes, at the level-0 shape of the bench (8 x 64 x 32 x 1024, fused
    input GroupNorm + residual, ~27 stores in flight per wave), against a recomputation from the stored
    output -- repeated launches (1 M entries per case)."""
    from lidarcrafter_amd import ops as K

    B, C, H, W = 8, 64, 32, 1024
    x = seeded_randn(B, C, H, W, seed=301).to(dev)
    w = (seeded_randn(C, C, 3, 3, seed=302) / 17.0).to(dev)
    res = seeded_randn(B, C, H, W, seed=303).to(dev)
    gn = K.groupnorm_stats(x, 32 if unit == 2 else 8, 1e-6)
    n_bad = 0
    for rep in range(16):
        y = K.conv2d_ring(x, K.PackedConv(), w, None, tile_cfg=23, emit_stats=True if unit == 8 else 2,
                          gn_coeffs=gn, res=res)
        h = y._lc_gnstats[(0, C)]
        assert h.unit == unit and h.slots == (H // 4) * (W // 64) * 4
        e = h.buf.double()                                             # [B, C / unit, slots, 4]
        # slot = (tile_row * tiles_w + tile_col) * 4 + px_wave; a wave owns image row px_wave of the 4 x 64 tile
        yv = y.double().view(B, C // unit, unit, H // 4, 4, W // 64, 64).permute(0, 1, 3, 5, 4, 2, 6)
        ref = yv.reshape(B, C // unit, h.slots, unit * 64)
        rs, rq = ref.sum(-1), (ref * ref).sum(-1)
        p, n, s_, q = e[..., 0], e[..., 1], e[..., 2], e[..., 3]
        assert torch.equal(n, torch.full_like(n, unit * 64.0))
        es, eq = p * n + s_, q + 2 * p * s_ + p * p * n
        bad = ((es - rs).abs() > 2e-3) | (((eq - rq).abs() / rq.clamp(min=1.0)) > 1e-4)
        n_bad += int(bad.sum())
    # rounds 1-3 wrote the entry as one 128-bit store and ~3 in 10^7 arrived with a foreign upper dword; as four 32-bit
    # stores (round 4) none does: devtools/entry_stress.py checks 10^8 per unit, profiles/r04_entry_store.txt
    assert n_bad == 0, f"{n_bad} corrupted statistics entries in {16 * e.shape[0] * e.shape[1] * e.shape[2]}"


@pytest.mark.parametrize("cfg", [27, 23])
@pytest.mark.parametrize("unit", [8, 2])
def test_conv_statistics_entries_stress(dev, cfg, unit):
    """Regression guard for the statistics-entry store (round 3: a 128-bit store with an SGPR soffset lost ~3 entries in
    10^7 under the store pressure of the deferred epilogue): 40 launches of the level-0 shape, every one of the
    40 x 65 536 (octet) / 262 144 (pair) entries recomputed from the output the same launch stored; none may be off.
    cfg 27 = the tall kernel (pair entries: its launcher's instantiation of the same DefEpi), cfg 23 = the pipelined one."""
    from lidarcrafter_amd import ops as K

    B, C, H, W = 8, 64, 32, 1024
    x = (seeded_randn(B, C, H, W, seed=901) * 1.1 + 0.3).to(dev)
    w = (seeded_randn(C, C, 3, 3, seed=902) / 24.0).to(dev)
    res = seeded_randn(B, C, H, W, seed=903).to(dev)
    ga = (1 + 0.1 * seeded_randn(C, seed=904)).to(dev)
    pk = K.PackedConv()
    bad = 0
    for it in range(40):
        gn = K.groupnorm_stats(x, 8, 1e-6, ga, None)
        y = K.conv2d_ring(x, pk, w, None, res=res, out_scale=0.7071, tile_cfg=cfg, gn_coeffs=gn, gn_silu=True,
                          emit_stats=True if unit == 8 else 2)
        h = y._lc_gnstats[(0, C)]
        assert h.unit == unit
        e = h.buf.double()
        yv = y.double().view(B, C // unit, unit, H // 4, 4, W // 64, 64).permute(0, 1, 3, 5, 4, 2, 6)
        rv = yv.reshape(B, C // unit, h.slots, unit * 64)
        rs, rq = rv.sum(-1), (rv * rv).sum(-1)
        pv, n, s_, q = e[..., 0], e[..., 1], e[..., 2], e[..., 3]
        es, eq = pv * n + s_, q + 2 * pv * s_ + pv * pv * n
        off = (n != unit * 64.0) | ((es - rs).abs() > 4e-3) | (((eq - rq).abs() / rq.clamp(min=1.0)) > 1e-4) | \
            ~torch.isfinite(e).all(-1)
        bad += int(off.sum())
        x = x + 0.01 * (it % 3 - 1)          # (new values every launch)
    assert bad == 0, f"{bad} statistics entries off"


@pytest.mark.parametrize("B,Ci,Co,H,W,ns", [(2, 64, 64, 8, 128, 1), (1, 64, 64, 32, 256, 2), (1, 128, 64, 16, 128, 2),
                                             (2, 64, 128, 16, 64, 1), (1, 192, 64, 8, 64, 1), (1, 64, 64, 32, 128, 4),
                                             (1, 64, 64, 12, 64, 3), (8, 64, 64, 32, 1024, 0), (1, 64, 64, 32, 64, 8),
                                             (2, 32, 64, 16, 128, 2), (1, 32, 96, 8, 64, 0), (1, 128, 64, 32, 64, 0)])
@pytest.mark.parametrize("mode", ["plain", "gn_silu_res_oct", "gn_res_pairs", "gn_oct_nores", "adagn_two_segments"])
@pytest.mark.parametrize("kern", [33, 27])
def test_conv_pp_matches_pipe(dev, B, Ci, Co, H, W, ns, mode, kern):
    """The ping-pong kernel (tile cfg 33, conv_f16x2_pp.h) against the oracle and -- bit for bit -- against the
    pipelined kernel (cfg 23) on the same inputs: plain input, fused GroupNorm(+SiLU) from a statistics pass, from a
    producer's octet entries and from the pair entries of two concatenated producers, with bias / residual / output
    scale, every strips-per-group count; every statistics entry it emits is recomputed from the output it stored."""
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    if kern == 33 and (Ci < 64 or Co % 64):
        pytest.skip("outside the ping-pong kernel's shapes")
    if kern == 33 and mode == "gn_oct_nores":
        pytest.skip("covered by the other modes")
    # tile cfg 27 = the tall kernel (conv_f16x2_tall.hip: kept halo rows, transposed accumulators, 16-byte epilogue);
    # shapes / modes it does not take (Ci not 32 or 64, pair entries) run on the pipelined kernel by its launcher's
    # fallback -- same statistics partition either way
    cfg = kern + 100 * ns
    x = (seeded_randn(B, Ci, H, W, seed=401) * 1.3 + 0.4).to(dev)
    w = (seeded_randn(Co, Ci, 3, 3, seed=402) / (Ci * 9) ** 0.5).to(dev)
    bias = seeded_randn(Co, seed=403).to(dev)
    res = seeded_randn(B, Co, H, W, seed=404).to(dev)
    ga, be = (1 + 0.1 * seeded_randn(Ci, seed=405)).to(dev), (0.1 * seeded_randn(Ci, seed=406)).to(dev)
    ss = (0.3 * seeded_randn(B, 2 * Ci, seed=407)).to(dev)
    small = B * Ci * H * W <= (1 << 21)
    if mode == "plain":
        kw = dict(bias=bias, out_scale=0.7071)
        ref = D.conv_ring(x.cpu(), w.cpu(), bias.cpu()) * 0.7071 if small else None
        emit = False
    elif mode == "gn_silu_res_oct":
        kw = dict(bias=bias, res=res, out_scale=0.7071, gn_silu=True)
        gn = lambda: K.groupnorm_stats(x, 8, 1e-6, ga, be)
        ref = (D.conv_ring(D.silu(D.group_norm(x.cpu(), 8, ga.cpu(), be.cpu(), 1e-6)), w.cpu(), bias.cpu())
               + res.cpu()) * 0.7071 if small else None
        emit = True
    elif mode == "gn_oct_nores":
        kw = dict(bias=bias, gn_silu=False, out_scale=1.25)
        gn = lambda: K.groupnorm_stats(x, 8, 1e-6, ga, be)
        ref = D.conv_ring(D.group_norm(x.cpu(), 8, ga.cpu(), be.cpu(), 1e-6), w.cpu(), bias.cpu()) * 1.25 if small else None
        emit = True
    elif mode == "gn_res_pairs":
        kw = dict(res=res, gn_silu=False)
        gn = lambda: K.groupnorm_stats(x, 32, 1e-6, ga, be)
        ref = D.conv_ring(D.group_norm(x.cpu(), 32, ga.cpu(), be.cpu(), 1e-6), w.cpu(), None) + res.cpu() if small else None
        emit = 2
    else:
        # the input is a concat of two producers that left statistics (octet entries; different tile shapes)
        if Ci % 64:
            pytest.skip("two producers of Ci / 2 channels, 8 channels per group")
        src = seeded_randn(B, 32, H, W, seed=408).to(dev)
        w1 = (seeded_randn(Ci // 2, 32, 3, 3, seed=409) / 17.0).to(dev)
        w2 = (seeded_randn(Ci // 2, 32, 3, 3, seed=410) / 11.0).to(dev)
        x = torch.empty(B, Ci, H, W, device=dev)
        K.conv2d_ring(src, K.PackedConv(), w1, bias[:1].repeat(Ci // 2), out=x[:, :Ci // 2], tile_cfg=23, emit_stats=True)
        K.conv2d_ring(src, K.PackedConv(), w2, None, out=x[:, Ci // 2:], tile_cfg=13, emit_stats=True)
        kw = dict(bias=bias, gn_silu=True)
        G2 = Ci // 8
        gn = lambda: K.groupnorm_stats(x, G2, 1e-6, ga, be, ss[:, :Ci], ss[:, Ci:])
        assert gn()._struct.partials is None
        xc = x.cpu()
        a = D.silu(D.group_norm(xc, G2, ga.cpu(), be.cpu(), 1e-6) * (1 + ss.cpu()[:, :Ci, None, None])
                   + ss.cpu()[:, Ci:, None, None])
        ref = D.conv_ring(a, w.cpu(), bias.cpu()) if small else None
        emit = True
    outs = {}
    for c in (cfg, 23):
        if mode != "plain":
            kw["gn_coeffs"] = gn()
        outs[c] = K.conv2d_ring(x, K.PackedConv(), w, tile_cfg=c, emit_stats=emit, **kw)
    y = outs[cfg]
    if ref is not None:
        assert rel_l2(y, ref) < 3e-6, rel_l2(y, ref)
    if kern == 33:
        assert torch.equal(y, outs[23]), rel_l2(y, outs[23])
    else:   # the transposed MFMA sums the same products in the same order per K step; the epilogue's fma matches too
        assert rel_l2(y, outs[23]) < 5e-7, rel_l2(y, outs[23])
    if emit:
        unit = 8 if emit is True else 2
        h = y._lc_gnstats[(0, Co)]
        assert h.unit == unit and h.slots == (H // 4) * (W // 64) * 4
        e = h.buf.double()                                             # [B, Co / unit, slots, 4]
        # slot = (strip_row * tiles_w + tile_col) * 4 + row; a wave owns one image row of the strip
        yv = y.double().view(B, Co // unit, unit, H // 4, 4, W // 64, 64).permute(0, 1, 3, 5, 4, 2, 6)
        rv = yv.reshape(B, Co // unit, h.slots, unit * 64)
        rs, rq = rv.sum(-1), (rv * rv).sum(-1)
        pv, n, s_, q = e[..., 0], e[..., 1], e[..., 2], e[..., 3]
        assert torch.equal(n, torch.full_like(n, unit * 64.0))
        es, eq = pv * n + s_, q + 2 * pv * s_ + pv * pv * n
        assert float((es - rs).abs().max()) < 4e-3 and float(((eq - rq).abs() / rq.clamp(min=1.0)).max()) < 1e-4
        # ... and a consumer GroupNorm that folds them agrees with the statistics pass
        g1 = K.groupnorm(y, 32 if unit == 2 else 8, 1e-6, act_silu=True) if unit == 8 else None
        if g1 is not None:
            assert rel_l2(g1, K.groupnorm(y.clone(), 8, 1e-6, act_silu=True)) < 2e-6


def test_groupnorm_large_mean(dev):
    """fp64 partial sums: no catastrophic cancellation when |mean| >> std."""
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    x = seeded_randn(1, 64, 32, 1024, seed=12) * 0.01 + 30.0
    ref = D.group_norm(x.double(), 8, None, None, 1e-6)
    y = K.groupnorm(x.to(dev), 8, 1e-6)
    ref32 = D.group_norm(x, 8, None, None, 1e-6)
    r_hip, r_torch = rel_l2(y, ref), rel_l2(ref32, ref)
    assert r_hip < 1e-4, (r_hip, r_torch)  # pivot-shifted sums: only input quantisation left
    # ... and by (sample, group), row and column: the two conditions of DESIGN.md "Error profiles"
    from tests._profile_cases import GN_KEEPS, check_profiles, gn_views

    lines, fails = check_profiles(gn_views(y, 8), gn_views(ref32, 8), gn_views(ref, 8), GN_KEEPS, 1e-4,
                                  name="groupnorm large mean, full width")
    print("\n".join(lines))
    assert not fails, fails


# ------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("B,C,H,W", [(2, 3, 4, 16), (1, 128, 32, 1024), (2, 64, 2, 8), (2, 7, 6, 10),
                                     (2, 5, 6, 256), (1, 4, 8, 512)])
def test_resample(dev, B, C, H, W, golden):
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    x = seeded_randn(B, C, H, W, seed=12)
    xd = x.to(dev)
    assert rel_l2(K.resample2x(xd, up=False), D.resample_down2(x)) < 1e-6
    assert rel_l2(K.resample2x(xd, up=True), D.resample_up2(x)) < 1e-6
    if W % 256 == 0:
        # the vector kernels (aligned rows, W % 256 == 0) against the scalar ones (the same values at a 4-byte-offset address):
        # same arithmetic order, bit for bit
        flat = torch.empty(x.numel() + 1, device=dev)
        xu = flat[1:].view(B, C, H, W)
        xu.copy_(xd)
        assert xu.data_ptr() % 16 != 0
        assert torch.equal(K.resample2x(xd, up=True), K.resample2x(xu, up=True))
        assert torch.equal(K.resample2x(xd, up=False), K.resample2x(xu, up=False))
    if (B, C, H, W) == (2, 3, 4, 16):
        g = golden("ops")
        assert rel_l2(K.resample2x(xd, up=False), T(g["down_y"])) < 1e-6
        assert rel_l2(K.resample2x(xd, up=True), T(g["up_y"])) < 1e-6


@pytest.mark.parametrize("B,C,H,W,G", [(2, 128, 8, 512, 8), (1, 64, 32, 1024, 8), (2, 32, 4, 256, 4), (1, 128, 16, 768, 32)])
def test_resample_down_statistics_feed_groupnorm(dev, B, C, H, W, G):
    """The x2 down-sampler's per-channel statistics entries (resample.hip, where its vector kernel runs): every entry
    recomputed from the plane the same launch stored, and each GroupNorm consumer -- apply, apply + fp16 split for
    the pre-split convolutions, the convolution's fused input norm -- fed from them against the same consumer behind a
    statistics pass (<= 2e-6) and against the oracle."""
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    x = (seeded_randn(B, C, H, W, seed=77) * 1.2 + 0.35)
    y = K.resample2x(x.to(dev), up=False)
    h = y._lc_gnstats[(0, C)]
    assert h.unit == 1 and h.slots == (H // 2) * (W // 2 // 128) and tuple(h.buf.shape) == (B, C, h.slots, 4)
    e = h.buf.double()
    rv = y.double().view(B, C, H // 2, W // 2 // 128, 128).reshape(B, C, h.slots, 128)
    pv, n, s_, q = e[..., 0], e[..., 1], e[..., 2], e[..., 3]
    assert bool((n == 128.0).all())
    assert float(((pv * n + s_) - rv.sum(-1)).abs().max()) < 2e-3
    rq = (rv * rv).sum(-1)
    assert float((((q + 2 * pv * s_ + pv * pv * n) - rq).abs() / rq.clamp(min=1.0)).max()) < 1e-4

    ga, be = (1 + 0.1 * seeded_randn(C, seed=78)).to(dev), (0.1 * seeded_randn(C, seed=79)).to(dev)
    y2 = y.clone()                                   # (no entries follow a clone: the statistics-pass route)
    assert not getattr(y2, "_lc_gnstats", None)
    ref = D.group_norm(D.resample_down2(x), G, ga.cpu(), be.cpu(), 1e-6)
    a1, a2 = K.groupnorm(y, G, 1e-6, ga, be), K.groupnorm(y2, G, 1e-6, ga, be)
    assert rel_l2(a1, a2) < 2e-6 and rel_l2(a1, ref) < 2e-6
    w = (seeded_randn(64, C, 3, 3, seed=80) / (C * 9) ** 0.5).to(dev)
    c1 = K.conv2d_ring(y, K.PackedConv(), w, None, gn_coeffs=K.groupnorm_stats(y, G, 1e-6, ga, be), gn_silu=True)
    c2 = K.conv2d_ring(y2, K.PackedConv(), w, None, gn_coeffs=K.groupnorm_stats(y2, G, 1e-6, ga, be), gn_silu=True)
    assert rel_l2(c1, c2) < 2e-6
    if (C // G) % 8 == 0:
        pk1, pk2 = K.PackedConv(), K.PackedConv()
        s1 = K.conv2d_ring(K.groupnorm(y, G, 1e-6, ga, be, act_silu=True, split_for=pk1), pk1, w, None)
        s2 = K.conv2d_ring(K.groupnorm(y2, G, 1e-6, ga, be, act_silu=True, split_for=pk2), pk2, w, None)
        assert rel_l2(s1, s2) < 2e-6 and rel_l2(s1, c1) < 2e-6


# ------------------------------------------------------------------------------------- dense
def test_linear_sinusoid(dev, golden):
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    x = seeded_randn(11, 256, seed=13)
    w = seeded_randn(300, 256, seed=14) / 16
    b = seeded_randn(300, seed=15)
    ref = torch.nn.functional.linear(D.silu(x), w, b)
    assert rel_l2(K.linear(x.to(dev), w.to(dev), b.to(dev), act_in=True), ref) < 2e-6
    ref = D.silu(torch.nn.functional.linear(x, w, b))
    assert rel_l2(K.linear(x.to(dev), w.to(dev), b.to(dev), act_out=True), ref) < 2e-6
    lam = torch.tensor([-15.0, -3.25, 0.0, 7.5, 15.0])
    y = K.sinusoid(lam.to(dev), 64)
    assert torch.allclose(y.cpu(), T(golden("ops")["sin_y"]), atol=2e-6)


# ------------------------------------------------------------------------------------- attention
# rel-L2 vs the fp32 / fp64 reference: fp32 MFMA kernel and the f16x2-split kernel (hi/lo fp16
# operands, fp32 accumulation) are held to the same fp32-class bound
ATTN_TOL = {"f32": 2e-6, "f16x2": 2e-6}


@pytest.mark.parametrize("B,heads,d,L", [(2, 4, 8, 32), (1, 8, 64, 512), (2, 8, 32, 512),
                                         (1, 2, 16, 100), (1, 8, 64, 2048),
                                         # >= 128 blocks of 256 queries with d_v <= 32: the 8-wave block of the f16x2 kernel
                                         (4, 16, 32, 512), (2, 8, 32, 2000), (8, 8, 16, 300)])
@pytest.mark.parametrize("prec", ["f32", "f16x2"])
def test_attention_mha(dev, B, heads, d, L, prec):
    from lidarcrafter_amd import ops as K

    C = heads * d
    qkv = seeded_randn(B, 3 * C, L, seed=16)
    q, k, v = [t.reshape(B, heads, d, L) for t in qkv.chunk(3, dim=1)]
    s = torch.einsum("bhct,bhcs->bhts", q, k) / d ** 0.5
    ref = torch.einsum("bhts,bhcs->bhct", s.softmax(-1), v).reshape(B, C, L)
    t = qkv.to(dev)
    o = K.attention_cm(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], heads, scale=1 / d ** 0.5,
                       precision=prec)
    assert rel_l2(o, ref) < ATTN_TOL[prec], rel_l2(o, ref)


@pytest.mark.parametrize("prec", ["f32", "f16x2"])
@pytest.mark.parametrize("B,heads,L1", [(2, 4, 200), (8, 8, 500)])   # (the second: the 8-wave block, ragged last block)
def test_attention_two_segments_and_spike(dev, prec, B, heads, L1):
    """Layout-style second key segment (13 tokens), d_qk = 2 d_v, and a forced online-softmax
    rescale (one huge score late in the key sequence)."""
    from lidarcrafter_amd import ops as K

    dqk, dv, L2 = 64, 32, 13
    q = seeded_randn(B, heads * dqk, L1, seed=17)
    k = seeded_randn(B, heads * dqk, L1, seed=18)
    v = seeded_randn(B, heads * dv, L1, seed=19)
    k2 = seeded_randn(B, heads * dqk, L2, seed=20)
    v2 = seeded_randn(B, heads * dv, L2, seed=21)
    k[:, :, 170] = q[:, :, 5] * 3.0  # spike: key 170 matches query 5 strongly
    scale = dqk ** -0.5
    qh = q.reshape(B, heads, dqk, L1)
    kh = torch.cat([k.reshape(B, heads, dqk, L1), k2.reshape(B, heads, dqk, L2)], -1)
    vh = torch.cat([v.reshape(B, heads, dv, L1), v2.reshape(B, heads, dv, L2)], -1)
    s = torch.einsum("bhct,bhcs->bhts", qh.double(), kh.double()) * scale
    ref = torch.einsum("bhts,bhcs->bhct", s.softmax(-1), vh.double()).reshape(B, heads * dv, L1)
    o = K.attention_cm(q.to(dev), k.to(dev), v.to(dev), heads, scale, k2=k2.to(dev), v2=v2.to(dev),
                       precision=prec)
    assert rel_l2(o, ref) < ATTN_TOL[prec], rel_l2(o, ref)


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("B,C,H,W,G", [(2, 64, 16, 512, 8), (2, 64, 8, 64, 8), (1, 256, 4, 256, 32)])
@pytest.mark.parametrize("producer_stats", [True, False])
def test_groupnorm_resample_pair(dev, up, B, C, H, W, G, producer_stats):
    """op(SiLU(GroupNorm(x))) and op(x) of a resampling ResBlock (layout_unet_v1.py:81-150) in one pass over x
    (lc_groupnorm_coeffs_os + lc_resample2x_pair_fwd) against GroupNorm apply + two resampling passes."""
    from lidarcrafter_amd import ops as K

    src = seeded_randn(B, 32, H, W, seed=81).to(dev)
    w = seeded_randn(C, 32, 3, 3, seed=82).to(dev) / 17.0
    x = K.conv2d_ring(src, K.PackedConv(), w, None, emit_stats=True)        # octet entries: groups of 8 channels
    if not producer_stats:
        x = x.clone()                                   # carries no entries: the coefficient rows come from a statistics pass
    assert (K._find_stats(x, G) is not None) == producer_stats
    ga, be = seeded_randn(C, seed=83).to(dev), seeded_randn(C, seed=84).to(dev)
    want_a = K.resample2x(K.groupnorm(x, G, 1e-5, ga, be, act_silu=True), up)
    want_x = K.resample2x(x, up)
    a, xr = K.groupnorm_resample_pair(x, G, 1e-5, ga, be, up)
    assert torch.equal(xr, want_x)
    assert rel_l2(a, want_a) < 1e-6, rel_l2(a, want_a)
    assert float((a - want_a).abs().max()) < 2e-5 * max(1.0, float(want_a.abs().max()))


@pytest.mark.parametrize("B,heads,Lq,Lk0,Lk1,dqk,dpos,dv", [
    (2, 3, 192, 192, 13, 32, 32, 32),      # ObjectAwareCrossAttention's shape in small: image keys ++ 13 layout keys
    (8, 8, 512, 512, 13, 32, 32, 32),      # the 8-wave block (ds 8 of the layout model)
    (2, 2, 100, 128, 0, 40, 16, 24),       # ragged queries, no second segment, channels a head does not fill
    (1, 2, 64, 64, 32, 64, 0, 8),          # no positional part, a full second tile
])
def test_attention_units_bit_equal(dev, B, heads, Lq, Lk0, Lk1, dqk, dpos, dv):
    """Keys / values in unit form (csrc/attention_units.hip: split once by lc_attention_pack_units, staged by LDS-DMA)
    against lc_attention_f16x2_fwd on the same operands: the same arithmetic, so the same bits -- and both within the
    f16x2 tolerance of the float64 softmax."""
    from lidarcrafter_amd import ops as K

    mk = lambda c, L, seed: seeded_randn(B, heads * c, L, seed=seed).to(dev)
    q, k, v = mk(dqk, Lq, 61), mk(dqk, Lk0, 62), mk(dv, Lk0, 63)
    qp = mk(dpos, Lq, 64) if dpos else None
    kp = seeded_randn(1, heads * dpos, Lk0, seed=65).to(dev).expand(B, -1, -1) if dpos else None   # stride-0 batch
    k2 = mk(dqk, Lk1, 66) if Lk1 else None
    v2 = mk(dv, Lk1, 67) if Lk1 else None
    k2p = mk(dpos, Lk1, 68) if (Lk1 and dpos) else None
    k[:, :, Lk0 - 7] = 2.5 * q[:, :, 3] if Lq == Lk0 else k[:, :, Lk0 - 7]     # a late spike: the running maximum moves
    scale = (dqk + dpos) ** -0.5
    want = K.attention_cm(q, k, v, heads, scale, k2=k2, v2=v2, q_pos=qp, k_pos=kp, k2_pos=k2p, precision="f16x2")
    assert K.AttnUnits.eligible(heads, Lk0, Lk1, dqk, dpos, dv)
    u = K.AttnUnits(B, heads, Lk0, Lk1, dqk, dpos, dv, dev)
    K.attention_pack_units(u, k, "k"), K.attention_pack_units(u, v, "v")
    if dpos:
        K.attention_pack_units(u, kp, "k_pos")
    if Lk1:
        K.attention_pack_units(u, k2, "k", segment=1), K.attention_pack_units(u, v2, "v", segment=1)
        if dpos:
            K.attention_pack_units(u, k2p, "k_pos", segment=1)
    got = K.attention_units(q, u, heads, scale, q_pos=qp)
    assert torch.equal(got, want)
    # a second step: new content keys / values over the old ones, the static parts stay
    k_, v_ = mk(dqk, Lk0, 72), mk(dv, Lk0, 73)
    K.attention_pack_units(u, k_, "k"), K.attention_pack_units(u, v_, "v")
    assert torch.equal(K.attention_units(q, u, heads, scale, q_pos=qp),
                       K.attention_cm(q, k_, v_, heads, scale, k2=k2, v2=v2, q_pos=qp, k_pos=kp, k2_pos=k2p))
    qh = torch.cat([t.reshape(B, heads, -1, Lq) for t in (q, qp) if t is not None], 2).double().cpu()
    k0 = torch.cat([t.reshape(B, heads, -1, Lk0) for t in (k, kp) if t is not None], 2)
    kh, vh = k0, v.reshape(B, heads, dv, Lk0)
    if Lk1:
        k1 = torch.cat([t.reshape(B, heads, -1, Lk1) for t in (k2, k2p) if t is not None], 2)
        kh, vh = torch.cat([k0, k1], -1), torch.cat([vh, v2.reshape(B, heads, dv, Lk1)], -1)
    sc = torch.einsum("bhct,bhcs->bhts", qh, kh.double().cpu()) * scale
    ref = torch.einsum("bhts,bhcs->bhct", sc.softmax(-1), vh.double().cpu()).reshape(B, heads * dv, Lq)
    assert rel_l2(want, ref) < ATTN_TOL["f16x2"]


@pytest.mark.parametrize("B,C,L,L2", [(2, 256, 512, 13), (8, 256, 2048, 13), (1, 128, 96, 0), (2, 512, 128, 13)])
def test_qkv_projection_writes_units(dev, monkeypatch, B, C, L, L2):
    """lc_conv1x1_f16x2_ps_qkv_fwd: the qkv projection whose key / value rows leave the kernel in the attention kernel's
    unit form (values through transposed accumulators) against the plain projection + lc_attention_f16x2_fwd."""
    from lidarcrafter_amd import ops as K
    from lidargen.models.unets.nn import GroupNorm32, PointwiseConv1d

    monkeypatch.setattr(K, "PS1X1_MIN_CO", 128)
    heads, d = C // 32, 32
    norm = seeded_fill(GroupNorm32(32, C), salt=41).to(dev)
    proj = seeded_fill(PointwiseConv1d(C, 3 * C), salt=42).to(dev)
    x = seeded_randn(B, C, L, seed=43).to(dev)
    pos = seeded_randn(1, heads * d, L, seed=44).to(dev).expand(B, -1, -1)
    k2 = seeded_randn(B, C, L2, seed=45).to(dev) if L2 else None
    v2 = seeded_randn(B, C, L2, seed=46).to(dev) if L2 else None
    k2p = seeded_randn(B, C, L2, seed=47).to(dev) if L2 else None
    scale = (2 * d) ** -0.5
    with torch.no_grad():
        assert K.presplit_1x1(C, 3 * C, 32) and K.qkv_units_ok(C, heads, L)
        qkv = proj(norm(x, split_for=proj._packed))
        want = K.attention_cm(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], heads, scale, k2=k2, v2=v2, q_pos=pos, k_pos=pos,
                              k2_pos=k2p)
        u = K.AttnUnits(B, heads, L, L2, d, d, d, dev)
        K.attention_pack_units(u, pos, "k_pos")
        if L2:
            K.attention_pack_units(u, k2, "k", 1), K.attention_pack_units(u, v2, "v", 1), K.attention_pack_units(u, k2p, "k_pos", 1)
        q = K.qkv_project_units(norm(x, split_for=proj._packed), proj._packed, proj.weight, proj.bias, u)
        assert torch.equal(q, qkv[:, :C])
        # the units the epilogue wrote == the units packed from the fp32 rows of the plain projection
        u2 = K.AttnUnits(B, heads, L, L2, d, d, d, dev)
        K.attention_pack_units(u2, pos, "k_pos"), K.attention_pack_units(u2, qkv[:, C:2 * C], "k"), K.attention_pack_units(u2, qkv[:, 2 * C:], "v")
        if L2:
            K.attention_pack_units(u2, k2, "k", 1), K.attention_pack_units(u2, v2, "v", 1), K.attention_pack_units(u2, k2p, "k_pos", 1)
        assert torch.equal(u.buf, u2.buf)
        got = K.attention_units(q, u, heads, scale, q_pos=pos)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------- sampler
def test_pstep_golden(dev, golden):
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion

    g = golden("diffusion")
    x_t = seeded_randn(3, 2, 4, 16, seed=31)
    pred = seeded_randn(3, 2, 4, 16, seed=32)
    st, ss = torch.tensor([1.0, 0.6, 0.1]), torch.tensor([0.9, 0.5, 0.0])

    class Stub(torch.nn.Module):
        resolution, in_channels = (4, 16), 2

        def forward(self, x, c):
            return pred.to(x.device)

    for obj in ("eps", "v", "x_0"):
        ddpm = ContinuousTimeGaussianDiffusion(Stub(), torch.nn.Identity(), prediction_type=obj).to(dev)
        for mode, eta in (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)):
            rng = [torch.Generator().manual_seed(100 + i) for i in range(3)]
            y = ddpm.p_step(x_t.to(dev), st, ss, rng=rng, mode=mode, ddim_eta=eta)
            ref = T(g[f"pstep_{obj}_{mode}_{eta}"])
            assert torch.allclose(y.cpu(), ref, rtol=2e-6, atol=2e-6), (obj, mode, eta)


# ------------------------------------------------------------------------------------- modules
def _uncond(base, res, dev):
    from lidargen.models.unets import EfficientUNet
    from lidargen.utils.lidar import get_linear_ray_angles

    m = EfficientUNet(2, res, base_channels=base, coords_encoding="fourier_features",
                      num_residual_blocks=(3, 3, 3, 3), gn_num_groups=8, gn_eps=1e-6,
                      attn_num_heads=8, ring=True)
    m.coords = get_linear_ray_angles(res[0], res[1], 10.0, -30.0)
    seeded_fill(m, salt=100)
    return m.eval().to(dev)


def test_blocks_golden(dev, golden):
    from lidargen.models.unets import efficient_unet as eu

    g = golden("ops")
    x = seeded_randn(2, 32, 4, 8, seed=15).to(dev)
    temb = seeded_randn(2, 64, seed=16).to(dev)
    rb = seeded_fill(eu.ResidualBlock(32, 32, 64, 8, 1e-6, ring=True), salt=5).to(dev)
    assert rel_l2(rb(x, temb), T(g["rb_same_y"])) < 5e-6
    rb = seeded_fill(eu.ResidualBlock(32, 16, 64, 8, 1e-6, ring=True), salt=6).to(dev)
    assert rel_l2(rb(x, temb), T(g["rb_skip_y"])) < 5e-6
    sa = seeded_fill(eu.SelfAttentionBlock(32, 4, 1e-6, 8), salt=7).to(dev)
    assert rel_l2(sa(x), T(g["sa_y"])) < 5e-6


def test_unet_small_golden(dev, golden):
    m = _uncond(16, (8, 64), dev)
    x = seeded_randn(2, 2, 8, 64, seed=21).to(dev)
    with torch.no_grad():
        y = m(x, torch.tensor([-4.0, 2.5], device=dev))
    assert rel_l2(y, T(golden("unet_small")["y"])) < 2e-5, rel_l2(y, T(golden("unet_small")["y"]))


def test_unet_full_golden(dev, golden, gn_stats_route):
    """32x1024, base 64 (31.1 M params) -- the C1/C2 denoiser -- vs the reference's own output."""
    m = _uncond(64, (32, 1024), dev)
    x = seeded_randn(1, 2, 32, 1024, seed=22).to(dev)
    with torch.no_grad():
        y = m(x, torch.tensor([-1.5], device=dev))
    r = rel_l2(y, T(golden("unet_full")["y"]))
    assert r < 2e-5, r


def test_prepare_model_packs_every_conv_weight_once(dev, monkeypatch):
    """ops.prepare_model (called by inference.setup_model on a GPU): every conv weight of the denoiser is packed and the
    code objects are loaded up front; the first forward then packs nothing, and gives the bits of an unprepared model."""
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd._lib import lib

    x = seeded_randn(2, 2, 8, 64, seed=23).to(dev)
    lam = torch.tensor([-1.0, 0.7], device=dev)
    with torch.no_grad():
        ref = _uncond(16, (8, 64), dev)(x, lam).clone()
    m = _uncond(16, (8, 64), dev)
    n_conv = sum(1 for mod in m.modules() if isinstance(mod.__dict__.get("_packed"), K.PackedConv)) + \
        2 * sum(1 for mod in m.modules() if isinstance(mod.__dict__.get("_pk_in"), K.PackedConv))
    assert K.prepare_model(m) == n_conv > 40
    assert lib().lc_load_code_objects() == 0            # idempotent
    calls = []
    real = lib().lc_pack_conv_weight_f16x2
    monkeypatch.setattr(lib(), "lc_pack_conv_weight_f16x2", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        y = m(x, lam)
    assert not calls, f"{len(calls)} weights were packed again by the first forward"
    assert torch.equal(y, ref)


def test_unet_batch_invariance(dev):
    m = _uncond(16, (8, 64), dev)
    x = seeded_randn(3, 2, 8, 64, seed=23).to(dev)
    lam = torch.tensor([-4.0, 2.5, 0.1], device=dev)
    with torch.no_grad():
        y3 = m(x, lam).clone()
        y1 = m(x[1:2].contiguous(), lam[1:2]).clone()
    assert rel_l2(y1, y3[1:2]) < 1e-6


def test_trajectory_small_golden(dev, golden):
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion

    g = golden("trajectory")
    m = _uncond(16, (8, 64), dev)
    ddpm = ContinuousTimeGaussianDiffusion(m, torch.nn.Identity()).eval().to(dev)
    for mode in ("ddim", "ddpm"):
        rng = [torch.Generator().manual_seed(i) for i in range(2)]
        xs = ddpm.sample(2, 10, progress=False, rng=rng, return_all=True, mode=mode).cpu()
        ref = T(g[f"small_{mode}"])
        assert torch.equal(xs[0], ref[0])
        for i in range(1, 11):
            assert rel_l2(xs[i], ref[i]) < 1e-3, (mode, i, rel_l2(xs[i], ref[i]))


def test_c1_trajectory_golden(dev, golden):
    """Config C1: 32x1024, DDIM 10 steps, B=1, CPU generator seed 0 (x_T bit-identical)."""
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion

    g = golden("trajectory")
    m = _uncond(64, (32, 1024), dev)
    ddpm = ContinuousTimeGaussianDiffusion(m, torch.nn.Identity()).eval().to(dev)
    rng = [torch.Generator().manual_seed(0)]
    xs = ddpm.sample(1, 10, progress=False, rng=rng, return_all=True, mode="ddim").cpu()
    for key, i in (("c1_x1", 1), ("c1_x2", 2), ("c1_x10", 10)):
        r = rel_l2(xs[i], T(g[key]))
        assert r < 1e-3, (key, r)


# ------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("N,H,W,seed", [(4096, 16, 256, 0), (34720, 32, 1024, 1),
                                        (131072, 32, 1024, 2), (0, 8, 64, 3), (7, 8, 64, 4)])
def test_projection_bit_exact(dev, N, H, W, seed):
    from lidarcrafter_amd import ops as K
    from oracle import lidar as L

    pts = synth_points(N, seed) if N else np.zeros((0, 4), np.float32)
    if N == 7:  # duplicates -> equal-depth ties: lowest index wins
        pts[3] = pts[1]
        pts[5] = pts[1]
    # both dtype contracts: "native" (default: float64 elevation arithmetic, the reference under
    # numpy >= 2) and "f32" (the reference's pinned numpy 1.23.5), bit-exact vs the oracle
    for mode, omode in (("native", "native_cr"), ("f32", "f32")):
        img_r, win_r = L.load_points_as_images(pts, H, W, mode=omode)
        gh, gw, _ = L.project_cells(pts, H, W, 10.0, -30.0, omode)
        img, win, cells = K.project_points(T(pts).to(dev), H, W, 10.0, -30.0, 1.45, 80.0,
                                           return_cells=True, dtype_mode=mode)
        assert np.array_equal(cells.cpu().numpy(), np.stack([gh, gw], 1).reshape(-1, 2)), mode
        assert np.array_equal(win.cpu().numpy(), win_r), mode
        assert np.array_equal(img.cpu().numpy(), img_r), mode


@pytest.mark.parametrize("H,W", [(32, 1024), (64, 2048), (16, 250)])
def test_projection_cells_at_boundaries(dev, H, W):
    """The cell of a point comes from an fp32 bracket of asin / atan2 when both ends of the bracket give one cell, and from
    the exact path (fp64 asin / atan2 rounded once: the definition) otherwise (geometry.hip cell_of, round 5).  Points
    constructed ON the row / column boundaries and a few float32 steps either side of them, on the azimuth wrap (y = +-0,
    x < 0), on the axes, at the poles and at the origin, plus a large uniform cloud: every cell equals the oracle's."""
    from lidarcrafter_amd import ops as K
    from oracle import lidar as L

    g = np.random.default_rng(5)
    up, down = np.deg2rad(10.0), np.deg2rad(-30.0)
    rows = down + (up - down) * (1.0 - np.arange(0, H + 1) / H)          # elevation of the row boundaries
    cols = -np.pi * (2.0 * np.arange(0, W + 1) / W - 1.0)                # azimuth of the column boundaries
    pts = []
    for _ in range(6):
        el = np.repeat(rows, 8) + g.uniform(-3e-7, 3e-7, 8 * (H + 1))
        az = g.uniform(-np.pi, np.pi, el.size)
        r = np.exp(g.uniform(np.log(0.8), np.log(95.0), el.size))
        pts.append(np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1))
        az = np.repeat(cols, 4) + g.uniform(-6e-7, 6e-7, 4 * (W + 1))
        el = g.uniform(down, up, az.size)
        r = np.exp(g.uniform(np.log(0.8), np.log(95.0), az.size))
        pts.append(np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1))
    special = np.array([[-1, 0.0, 0], [-1, -0.0, 0], [-5, 1e-7, 0.1], [-5, -1e-7, 0.1], [-5, 1e-38, 0], [-5, -1e-38, 0],
                        [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [1e-20, 1e-20, 1e-20],
                        [3, 4, 1e-30], [3, 4, -1e-30], [1e-3, 0, 50], [1e-3, 0, -50], [np.nan, 1, 1], [1, np.inf, 1]])
    pts.append(special)
    pts.append(synth_points(1 << 20, 11)[:, :3].astype(np.float64))
    p3 = np.concatenate(pts).astype(np.float32)
    # float32 neighbours of every constructed point (x or y one step up / down): lands on both sides of a boundary
    nb = p3[: 8 * (H + 1) + 4 * (W + 1)].copy()
    nb[:, 0] = np.nextafter(nb[:, 0], np.float32(np.inf))
    nb2 = p3[: 8 * (H + 1) + 4 * (W + 1)].copy()
    nb2[:, 1] = np.nextafter(nb2[:, 1], np.float32(-np.inf))
    p3 = np.concatenate([p3, nb, nb2])
    p4 = np.concatenate([p3, np.ones((p3.shape[0], 1), np.float32)], 1)
    for mode, omode in (("native", "native_cr"), ("f32", "f32")):
        with np.errstate(all="ignore"):
            gh, gw, _ = L.project_cells(p4, H, W, 10.0, -30.0, omode)
        cells = K.project_points(T(p4).to(dev), H, W, 10.0, -30.0, 1.45, 80.0, return_cells=True, dtype_mode=mode)[2]
        got = cells.cpu().numpy()
        ok = np.isfinite(p4).all(1)           # (a NaN / inf point never wins a cell; its reported cell is unspecified)
        bad = np.nonzero(((got[:, 0] != gh) | (got[:, 1] != gw)) & ok)[0]
        assert bad.size == 0, (mode, bad[:8], got[bad[:8]], gh[bad[:8]], gw[bad[:8]], p4[bad[:8]])


@pytest.mark.parametrize("tag,N,H,W,seed", [("a", 4096, 16, 256, 0), ("b", 34720, 32, 1024, 1)])
def test_projection_vs_reference_golden(dev, golden, tag, N, H, W, seed):
    """Against the reference AS RUN in the build container (numpy 2.2 promotion, fixture
    tests/golden/lidar.npz): 0 differing cells, all four stored channels bit-identical.  (The
    kernel's asin / atan2 are correctly rounded, numpy's SIMD float32 ones are not; a difference
    could only appear in a cell reachable by a point whose cell depends on that last bit --
    oracle.lidar.ulp_ambiguous -- and these fixtures have none that matters.)"""
    from lidarcrafter_amd import ops as K
    from oracle import lidar as L

    g = golden("lidar")
    pts = synth_points(N, seed)
    img = K.project_points(T(pts).to(dev), H, W, 10.0, -30.0, 1.45, 80.0)[0].cpu().numpy()
    diff = np.argwhere(img[..., 4] != g[f"proj_{tag}_depth"]).tolist()
    _, cells = L.ulp_ambiguous(pts, H, W, 10.0, -30.0)
    assert all((a, b) in cells for a, b in diff), diff
    assert diff == [], diff
    assert np.array_equal(img[..., 5].astype(np.uint8), g[f"proj_{tag}_mask"])
    assert np.array_equal(img[..., 0], g[f"proj_{tag}_x"])
    assert np.array_equal(img[..., 3], g[f"proj_{tag}_i"])


# ------------------------------------------------------------------------------------- conditional
@pytest.mark.parametrize("prec", ["f32", "f16x2"])
def test_attention_positional_parts(dev, prec):
    """q/k = content ++ positional parts passed as separate operands (no cat), stride-0 batch."""
    from lidarcrafter_amd import ops as K

    B, heads, d, L1, L2 = 2, 4, 32, 96, 13
    C = heads * d
    q, k, v = [seeded_randn(B, C, L1, seed=30 + i) for i in range(3)]
    pos = seeded_randn(1, C, L1, seed=33)
    k2, v2, p2 = [seeded_randn(B, C, L2, seed=34 + i) for i in range(3)]
    hv = lambda t: t.expand(B, -1, -1).reshape(B, heads, d, -1)
    qm = torch.cat([hv(q), hv(pos)], 2)
    km = torch.cat([torch.cat([hv(k), hv(pos)], 2), torch.cat([hv(k2), hv(p2)], 2)], 3)
    vm = torch.cat([hv(v), hv(v2)], 3)
    scale = (2 * d) ** -0.5
    s = torch.einsum("bhct,bhcs->bhts", qm.double(), km.double()) * scale
    ref = torch.einsum("bhts,bhcs->bhct", s.softmax(-1), vm.double()).reshape(B, C, L1)
    posd = pos.to(dev).expand(B, -1, -1)
    o = K.attention_cm(q.to(dev), k.to(dev), v.to(dev), heads, scale, k2=k2.to(dev),
                       v2=v2.to(dev), q_pos=posd, k_pos=posd, k2_pos=p2.to(dev), precision=prec)
    assert rel_l2(o, ref) < ATTN_TOL[prec], rel_l2(o, ref)


def _to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


def test_cond_small_golden(dev, golden):
    from lidarcrafter_amd.testing import synth_layout_batch
    from tests.test_oracle_vs_golden import build_cond_pair

    g = golden("cond_small")
    m, enc = build_cond_pair((8, 64), 8, 32)
    m, enc = m.to(dev), enc.to(dev)
    batch = _to_dev(synth_layout_batch(2, 8, 64, seed=51), dev)
    with torch.no_grad():
        cond = enc(batch)
        for k in ("xf_proj", "xf_out", "obj_class_embedding", "obj_bbox_embedding"):
            assert rel_l2(cond[k], T(g["cond_" + k])) < 5e-6, k
        x = seeded_randn(2, 2, 8, 64, seed=52).to(dev)
        lam = torch.tensor([-3.0, 1.5], device=dev)
        y = m(x, {"time_condition": lam, "other_condition": cond})
    r = rel_l2(y, T(g["y"]))
    assert r < 2e-5, r


@pytest.mark.parametrize("tag", ["mask", "nf", "scale"])
def test_cond_attention_options_golden(dev, golden, tag):
    """The ObjectAwareCrossAttention constructor options no shipped configuration sets (normalisation before the
    projectors, extra norm of xf_out, positional channels = channels / 2, masked layout keys -- also inside the layout
    encoder) vs the reference's output (tests/golden/cond_options.npz)."""
    from lidarcrafter_amd.testing import synth_layout_batch
    from tests.test_oracle_vs_golden import COND_OPTION_VARIANTS, build_cond_pair

    g = golden("cond_options")
    ukw, ekw = COND_OPTION_VARIANTS[tag]
    m, enc = build_cond_pair((8, 64), 8, 32, unet_kw=ukw, enc_kw=ekw)
    m, enc = m.to(dev), enc.to(dev)
    batch = _to_dev(synth_layout_batch(2, 8, 64, seed=51), dev)
    with torch.no_grad():
        cond = enc(batch)
        assert rel_l2(cond["xf_out"], T(g[tag + "_xf_out"])) < 5e-6
        x = seeded_randn(2, 2, 8, 64, seed=52).to(dev)
        lam = torch.tensor([-3.0, 1.5], device=dev)
        y = m(x, {"time_condition": lam, "other_condition": cond})
        y2 = m(x, {"time_condition": lam, "other_condition": cond})      # cached condition operands: same bits
    r = rel_l2(y, T(g[tag + "_y"]))
    assert r < 2e-5, r
    assert torch.equal(y, y2)


def test_cond_attention_extra_output(dev):
    """return_attention_embeddings (layout_unet_v1.py:512-530): the layer hands its positional operands back."""
    from lidargen.models.unets.layout_unet_v1 import ObjectAwareCrossAttention

    at = seeded_fill(ObjectAwareCrossAttention(64, num_head_channels=32, encoder_channels=64, ds=4, resolution=2,
                                               type="input", return_attention_embeddings=True), salt=9).to(dev).eval()
    B, L1, L2 = 2, 2 * 16, 13
    cond = {"image_patch_bbox_embedding_for_resolution2": seeded_randn(B, 64, L1, seed=1).to(dev),
            "obj_bbox_embedding": seeded_randn(B, 64, L2, seed=2).to(dev),
            "xf_out": seeded_randn(B, 64, L2, seed=3).to(dev),
            "obj_class_embedding": seeded_randn(B, 64, L2, seed=4).to(dev)}
    with torch.no_grad():
        y, extra = at(seeded_randn(B, 64, 2, 16, seed=5).to(dev), cond)
    assert y.shape == (B, 64, 2, 16)
    assert extra["type"] == "input" and extra["ds"] == 4 and extra["resolution"] == 2 and extra["num_heads"] == 2
    assert extra["image_query_embeddings"].shape == (B, 64, L1) and extra["layout_key_embeddings"].shape == (B, 64, L2)


def test_cond_full_golden(dev, golden, gn_stats_route):
    """box-layout-v6 (70.1 M params) forward + 3-step conditional DDIM vs the reference."""
    from lidargen.utils import inference
    from lidargen.utils.configs import __all__ as C
    from lidarcrafter_amd.testing import synth_layout_batch

    g = golden("cond_full")
    cfg = C["nuscenes-box-layout-v6"]()
    ddpm, model, _ = inference.load_model_duffusion_training(cfg)
    seeded_fill(model, salt=200), seeded_fill(ddpm.condition_model, salt=201)
    ddpm = ddpm.eval().to(dev)
    batch = _to_dev(synth_layout_batch(1, 32, 1024, seed=53), dev)
    with torch.no_grad():
        cond = ddpm.condition_model(batch)
        x = seeded_randn(1, 2, 32, 1024, seed=54).to(dev)
        y = ddpm.model(x, {"time_condition": torch.tensor([-0.5], device=dev),
                           "other_condition": cond})
    r = rel_l2(y, T(g["y"]))
    assert r < 2e-5, r
    rng = [torch.Generator().manual_seed(7)]
    xs = ddpm.sample(batch, 1, 3, progress=False, rng=rng, return_all=True, mode="ddim").cpu()
    assert rel_l2(xs[1], T(g["traj_x1"])) < 1e-3, rel_l2(xs[1], T(g["traj_x1"]))
    assert rel_l2(xs[3], T(g["traj_x3"])) < 1e-3, rel_l2(xs[3], T(g["traj_x3"]))


# ------------------------------------------------------------------------------------- boxes
def test_points_in_boxes_bit_exact(dev, golden):
    from lidarcrafter_amd.testing import synth_boxes
    from lidargen.ops.roiaware_pool3d import roiaware_pool3d_utils as R
    from oracle import boxes as OB

    g = golden("boxes")
    pts = synth_points(32768, 5)[:, :3].copy()
    bx = synth_boxes(12, pts, 6)
    keep = bx.copy()
    mask = R.points_in_boxes_cpu(pts, bx)          # numpy in -> numpy out, runs on the GPU
    assert isinstance(mask, np.ndarray) and mask.shape == (12, 32768)
    assert np.array_equal(np.packbits(mask.astype(np.uint8), axis=1), g["mask_packed"])
    # batched first-hit variant (GPU margin 1e-5), incl. an empty / far box and B=2
    pts2 = np.stack([pts, synth_points(32768, 8)[:, :3]])
    bx2 = np.stack([keep, synth_boxes(12, pts2[1], 11)])
    bx2[1, 3, :3] = 1e4
    idx = R.points_in_boxes_gpu(T(pts2).to(dev), T(bx2).to(dev))
    assert np.array_equal(idx.cpu().numpy(), OB.points_in_boxes_index(pts2, bx2, 1e-5))


def test_points_in_boxes_more_boxes_than_one_launch(dev):
    """a launch holds 1250 boxes in LDS; the ops chunk larger sets (mask rows per slab, counts added, first
    containing box across slabs) -- bit-exact against the C restatement at 2600 boxes."""
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd.testing import synth_boxes
    from oracle import boxes as OB

    pts = synth_points(4096, 15)[:, :3].copy()
    bx = np.concatenate([synth_boxes(13, pts, 20 + i) for i in range(200)])
    assert bx.shape[0] == 2600 > K.PIB_MAX_BOXES
    ref = OB.points_in_boxes_mask(pts, bx, 1e-2)
    p4 = np.concatenate([pts, np.zeros((4096, 1), np.float32)], 1)
    m4, cnt = K.points_in_boxes_mask4(T(p4).to(dev), T(bx).to(dev), 1e-2)
    assert np.array_equal(m4.cpu().numpy(), ref) and np.array_equal(cnt.cpu().numpy(), ref.sum(0))
    m = K.points_in_boxes_mask(T(pts).to(dev), T(bx).to(dev), 1e-2)
    assert np.array_equal(m.cpu().numpy(), ref)
    idx = K.points_in_boxes_index(T(pts[None]).to(dev), T(bx[None]).to(dev), 1e-5)
    assert np.array_equal(idx.cpu().numpy(), OB.points_in_boxes_index(pts[None], bx[None], 1e-5))


def test_load_points_as_images_api(dev, golden):
    from lidargen.dataset.transforms_3d.common import load_points_as_images
    from oracle import lidar as L

    pts = synth_points(4096, 0)
    img = load_points_as_images(points=pts, scan_unfolding=False, H=16, W=256)
    ref, _ = L.load_points_as_images(pts, 16, 256, mode="native_cr")
    assert isinstance(img, np.ndarray) and np.array_equal(img, ref)


# ------------------------------------------------------------------------------------- other configs
def test_unet_64x2048(dev):
    """C4 resolution: the same denoiser at 64x2048 (H, W are parameters of every kernel)."""
    from oracle import denoiser as D

    m = _uncond(32, (64, 2048), dev)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x = seeded_randn(1, 2, 64, 2048, seed=60)
    lam = torch.tensor([0.7])
    with torch.no_grad():
        y = m(x.to(dev), lam.to(dev))
    r = rel_l2(y, D.efficient_unet_forward(sd, x, lam))
    assert r < 2e-5, r


def test_autoregressive_cond_config(dev):
    """nuscenes-auto-reg-v2 shapes (11 condition channels = concat_cond 10 + autoregressive 1),
    reduced width, DDPM mode like sample_and_save_temporal.py:189, vs the oracle sampler."""
    from lidarcrafter_amd.testing import synth_layout_batch
    from lidargen.models.diffusion import CondContinuousTimeGaussianDiffusion
    from oracle import denoiser as D
    from oracle import diffusion as DF
    from tests.test_oracle_vs_golden import build_cond_pair

    m, enc = build_cond_pair((8, 64), 8, 32, cond_out=11)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sde = {k: v.clone() for k, v in enc.state_dict().items()}
    batch = synth_layout_batch(2, 8, 64, seed=61, n_extra=1)
    ddpm = CondContinuousTimeGaussianDiffusion(m, enc, cond_mode="concat").eval().to(dev)
    assert ddpm.sampling_shape == (2, 8, 64)
    rng = [torch.Generator().manual_seed(70 + i) for i in range(2)]
    xs = ddpm.sample({k: v.to(dev) for k, v in batch.items()}, 2, 4, progress=False, rng=rng,
                     return_all=True, mode="ddpm").cpu()
    cond = D.layout_encoder_forward(sde, batch, feature_map_size=[8, 64],
                                    resolution_to_attention=[4, 8])
    den = lambda x, lam: D.layout_unet_v1_forward(sd, x, lam, cond, image_size=8, model_channels=32)
    rng = [torch.Generator().manual_seed(70 + i) for i in range(2)]
    ref = DF.sample(den, (2, 2, 8, 64), 4, rng, mode="ddpm", return_all=True)
    assert torch.equal(xs[0], ref[0])
    for i in range(1, 5):
        assert rel_l2(xs[i], ref[i]) < 1e-3, (i, rel_l2(xs[i], ref[i]))


def test_hip_graph_equals_eager(dev):
    """Graph-replayed steps produce the same states as eager launches (DDPM: noise is an input)."""
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion

    m = _uncond(16, (8, 64), dev)
    ddpm = ContinuousTimeGaussianDiffusion(m, torch.nn.Identity()).eval().to(dev)
    outs = []
    for flag in (True, False):
        ddpm.use_hip_graph = flag
        rng = [torch.Generator().manual_seed(i) for i in range(2)]
        outs.append(ddpm.sample(2, 6, progress=False, rng=rng, return_all=True, mode="ddpm").cpu())
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------- roi pooling
@pytest.mark.parametrize("method", ["max", "avg"])
def test_roiaware_pool3d_vs_restatement_voxel_index_slot_order_pooling_unpinned(dev, method):
    """Forward bit-exact vs the numpy restatement of the reference kernels (incl. a voxel that
    overflows max_pts_each_voxel), backward within fp32 atomics tolerance.  The restatement's inside test is pinned on
    the compiled reference (tests/test_oracle_vs_golden.py::test_roipool_inside_test_vs_reference_cpp).  The voxel
    index arithmetic, slot order / overflow rule, the pooling and the backward, which this restatement only follows
    from the CUDA text (hence the test name), are now pinned on the reference's own CUDA kernels, hipified and
    compiled for gfx950 with and without FP contraction (tests/test_reference_kernels.py)."""
    from lidarcrafter_amd.testing import synth_boxes
    from lidargen.ops.roiaware_pool3d.roiaware_pool3d_utils import RoIAwarePool3d
    from oracle import roipool as O

    g = np.random.default_rng(3)
    pts = synth_points(3000, 12)[:, :3].copy()
    bx = synth_boxes(5, pts, 13)
    bx[:, 3:6] *= 1.5
    pts[:200] = bx[0, :3] + g.normal(0, 0.01, (200, 3)).astype(np.float32)  # overflow one voxel
    feat = g.normal(size=(3000, 4)).astype(np.float32)
    out_size, cap = (3, 2, 2), 16
    pooled_r, vox_r, am_r = O.forward(bx, pts, feat, out_size, cap, 0 if method == "max" else 1)
    assert vox_r[..., 0].max() == cap - 1
    pool = RoIAwarePool3d(out_size, cap)
    ft = T(feat).to(dev).requires_grad_(True)
    y = pool(T(bx).to(dev), T(pts).to(dev), ft, pool_method=method)
    assert np.array_equal(y.detach().cpu().numpy(), pooled_r)
    go = g.normal(size=pooled_r.shape).astype(np.float32)
    y.backward(T(go).to(dev))
    gin_r = O.backward(vox_r, am_r, go, 3000, 0 if method == "max" else 1)
    assert np.allclose(ft.grad.cpu().numpy(), gin_r, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------- pre/post
def test_fused_pre_post_processing(dev):
    from lidargen.utils.lidar import LiDARUtility, get_linear_ray_angles
    from oracle import denoiser as D
    from oracle import lidar as L

    H, W = 32, 1024
    ang = get_linear_ray_angles(H, W, 10.0, -30.0)
    lu = LiDARUtility((H, W), "log_depth", 1.45, 80.0, ray_angles=ang).to(dev)
    x = (seeded_randn(3, 2, H, W, seed=80) * 0.6).clamp(-1, 1)
    y = lu.postprocess(x.to(dev)).cpu()
    dn = (x + 1) / 2
    metric = L.revert_depth(dn[:, [0]], 1.45, 80.0)
    ref = torch.cat([metric, L.to_xyz(metric, D.linear_ray_angles(H, W, 10.0, -30.0), 1.45, 80.0),
                     dn[:, [1]]], dim=1)
    # a depth within a few ulp of min/max_depth may flip its mask: compare away from the edges
    edge = ((metric - 1.45).abs() < 1e-4) | ((metric - 80.0).abs() < 1e-3)
    ok = ~edge.expand_as(ref)
    assert torch.allclose(y[ok], ref[ok], rtol=2e-5, atol=2e-5)
    g = torch.Generator().manual_seed(81)
    cm = torch.stack([torch.randint(0, 9, (3, H, W), generator=g).float(),
                      torch.rand(3, H, W, generator=g) * 90], dim=1)
    z = lu.preprocess_condition_mask(cm.to(dev), 9).cpu()
    ref = torch.cat([torch.nn.functional.one_hot(cm[:, 0].long(), 9).permute(0, 3, 1, 2).float(),
                     L.convert_depth(cm[:, [1]], 1.45, 80.0)], dim=1)
    assert torch.equal(z[:, :9], ref[:, :9])
    assert torch.allclose(z[:, 9:], ref[:, 9:], rtol=2e-6, atol=2e-6)


def test_cli_generate(dev, tmp_path):
    from lidarcrafter_amd import cli

    cli.main(["--cfg", "nuscenes-unet-uncond", "--batch_size", "2", "--sampling_steps", "3",
              "--out", str(tmp_path)])
    out = torch.load(tmp_path / "samples.pt")
    assert out.shape == (2, 5, 32, 1024) and torch.isfinite(out).all()
    cli.main(["--cfg", "nuscenes-auto-reg-v2", "--batch_size", "1", "--sampling_steps", "3",
              "--mode", "ddpm", "--out", str(tmp_path)])
    out = torch.load(tmp_path / "samples.pt")
    assert out.shape == (1, 5, 32, 1024) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------- layout raster
@pytest.mark.parametrize("tag,n,H,W,seed", [("a", 9, 32, 1024, 0), ("b", 13, 32, 1024, 1),
                                            ("c", 5, 64, 2048, 2)])
def test_layout_condition_device(dev, golden, tag, n, H, W, seed):
    """3-D boxes -> class/depth condition mask on the device, bit-exact vs the reference's own
    output (fixture) and the numpy restatement, incl. the +-pi wrap-around box; batched call with
    padded rows; chained into the fused preprocess kernel."""
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd.testing import synth_scene_boxes
    from lidargen.dataset.transforms_3d.common import convert_boxes_to_2d
    from oracle import layout as OL

    g = golden("layout_cond")
    boxes = synth_scene_boxes(n, seed)
    c2d, mask, wmap = convert_boxes_to_2d(boxes, H=H, W=W)
    assert np.array_equal(mask[0].astype(np.uint8), g[f"{tag}_class"])
    assert np.array_equal(mask[1], g[f"{tag}_depth"])
    assert np.allclose(c2d, g[f"{tag}_corners2d"], atol=1e-7)
    _, _, wref = OL.convert_boxes_to_2d(boxes, H, W)
    assert np.allclose(wmap, wref, rtol=1e-5)
    pad = np.zeros((2, 13, 8), np.float32)
    pad[0, :n], pad[1, :4] = boxes, boxes[:4]
    nv = torch.tensor([n, 4], dtype=torch.int32, device=dev)
    c2, m2 = K.layout_condition(T(pad).to(dev), nv, H, W, 10.0, -30.0)
    assert np.array_equal(m2[0].cpu().numpy(), mask)
    assert np.array_equal(m2[1].cpu().numpy(), OL.convert_boxes_to_2d(boxes[:4], H, W)[1])
    assert float(c2[0, n:].abs().max()) == 0.0 if n < 13 else True


# ------------------------------------------------------------------------------------- temporal glue
@pytest.mark.parametrize("N", [0, 1, 255, 1023, 1024, 1025, 34720, 300001])
def test_compact_points(dev, N):
    from lidarcrafter_amd import ops as K

    g = np.random.default_rng(N)
    rows = torch.from_numpy(g.normal(size=(N, 4)).astype(np.float32)).to(dev)
    flags = torch.from_numpy((g.random(N) < 0.37).astype(np.int32) * g.integers(1, 5, N).astype(np.int32)).to(dev)
    out, idx = K.compact_points(rows, flags, return_index=True)
    sel = np.nonzero(flags.cpu().numpy())[0]
    assert np.array_equal(idx.cpu().numpy(), sel)
    assert torch.equal(out.cpu(), rows.cpu()[sel])
    out0 = K.compact_points(rows, flags, keep_if_zero=True)
    assert torch.equal(out0.cpu(), rows.cpu()[np.nonzero(flags.cpu().numpy() == 0)[0]])


def test_transform_points_bit_exact(dev, golden):
    from lidarcrafter_amd import ops as K
    from lidarcrafter_amd.testing import synth_points
    from oracle import temporal as OT

    g = golden("temporal")
    P = synth_points(5000, seed=7)
    d = torch.from_numpy(P).to(dev)
    for T in list(g["Ts"]) + [OT.warp_lidar_matrix(g["ego_xy"], 2), OT.box_frame_matrix(g["boxes"][1], False),
                              OT.box_frame_matrix(g["boxes"][1], True)]:
        assert np.array_equal(K.transform_points(d, T).cpu().numpy(), OT.apply_T(P, T))
    # against the reference's own float64 result (warp_lidar_future on float64 points)
    w = K.transform_points(torch.from_numpy(synth_points(800, seed=7)).to(dev),
                           OT.warp_lidar_matrix(g["ego_xy"], 3)).cpu().numpy()
    assert np.abs(w - g["warp_lidar64"][3]).max() < 1e-5


from tests._scenes import temporal_scene as _temporal_scene  # noqa: E402


def test_custom_dataset_item_vs_oracle(dev):
    """CustomDataset.__getitem__ + pre_process on the device vs the oracle (itself pinned on the
    reference's own CustomDataset, tests/golden/pipe_next.npz): float32 and float64 point sets."""
    import lidargen  # noqa: F401
    from lidargen.dataset import __all__ as DS
    from oracle import temporal as OT

    first, pts, ref = _temporal_scene(3)
    ds = DS["custom"]([dict(points=pts, gt_boxes=first["gt_boxes"].copy(), gt_names=first["gt_names"])])
    it = ds[0]
    for k in ("xyz", "reflectance", "depth", "mask", "condition_mask"):
        assert np.array_equal(it[k].cpu().numpy(), ref[k]), k
    # float map exp(sum of per-box weights): device expf / summation order vs numpy's, 2 ulps
    assert np.allclose(it["scene_loss_weight_map"].cpu().numpy(), ref["scene_loss_weight_map"], rtol=2.4e-7, atol=0)
    for k in ("scaled_gt_boxes", "gt_boxes_2d", "fg_encoding_box", "is_valid_obj"):
        assert np.allclose(np.asarray(it[k]), ref[k], rtol=1e-6, atol=1e-6), k
    ds.task = "autoregressive_generation"
    it2 = ds[0]
    ref2 = OT.custom_item(pts, first["gt_boxes"].copy(), first["gt_names"], task="autoregressive_generation")
    assert np.array_equal(it2["autoregressive_cond"].cpu().numpy(), ref2["autoregressive_cond"])
    assert "xyz" not in it2
    batch = ds.collate_fn([it2, ds[0]])
    assert batch["autoregressive_cond"].shape == (2, 2, 32, 1024) and batch["batch_size"] == 2
    assert batch["scaled_gt_boxes"].shape == (2, 13, 9) and batch["is_valid_obj"].shape == (2, 13)
    # float64 points: projected in float64 (numpy and device-tensor inputs)
    p64 = pts.astype(np.float64) * 1.0000001
    ref3 = OT.custom_item(p64, first["gt_boxes"].copy(), first["gt_names"], task="autoregressive_generation")
    for src in (p64, torch.from_numpy(p64).to(dev)):
        ds3 = DS["custom"]([dict(points=src, gt_boxes=first["gt_boxes"].copy(), gt_names=first["gt_names"])])
        ds3.task = "autoregressive_generation"
        assert np.array_equal(ds3[0]["autoregressive_cond"].cpu().numpy(), ref3["autoregressive_cond"])


def test_custom_dataset_item_vs_reference_golden(dev, golden):
    """The device item vs outputs of the REFERENCE's own CustomDataset.__getitem__ /
    NuscDataset.pre_process (tests/golden/pipe_next.npz): images bit-identical outside the <= 2
    cells a float32 asin / atan2 last-bit-ambiguous point can reach (numpy's float32 ufuncs are not
    correctly rounded), everything else bit-identical; float64 point sets and the
    boxes-only item bit-identical."""
    import lidargen  # noqa: F401
    from lidargen.dataset.custom_dataset import CustomDataset
    from oracle import lidar as OLD

    g = golden("pipe_next")
    for seed in (0, 1):
        first, pts, _ = _temporal_scene(seed)
        t = f"s{seed}_"
        info = lambda p: dict(points=p, gt_boxes=first["gt_boxes"].copy(), gt_names=list(first["gt_names"]))
        it = CustomDataset([info(pts.copy())])[0]
        assert sorted(it.keys()) == list(g[t + "item_keys"])
        _, cells = OLD.ulp_ambiguous(pts, 32, 1024, 10.0, -30.0)
        free = np.ones((32, 1024), bool)
        for (r, c) in cells:
            free[r, c] = False
        for k in ("xyz", "reflectance", "depth", "mask", "condition_mask", "scene_loss_weight_map"):
            if t + "item_" + k not in g:
                continue
            a, ref = it[k].cpu().numpy(), g[t + "item_" + k]
            assert a.dtype == ref.dtype and a.shape == ref.shape, k
            if k == "condition_mask":
                assert np.array_equal(a, ref), k
            elif k == "scene_loss_weight_map":      # float exp(): 2 ulps (expf vs numpy's exp)
                assert np.allclose(a, ref, rtol=2.4e-7, atol=0), k
            else:
                assert np.array_equal(a[..., free], ref[..., free]), k
        for k in ("gt_boxes", "scaled_gt_boxes", "gt_boxes_2d", "fg_encoding_box", "is_valid_obj"):
            assert np.allclose(np.asarray(it[k], np.float64), g[t + "item_" + k], rtol=0, atol=1e-12), k
        p64 = pts.astype(np.float64) * 1.0000001
        ds = CustomDataset([info(p64.copy())])
        i64 = ds[0]
        ds.task = "autoregressive_generation"
        iar = ds[0]
        assert sorted(iar.keys()) == list(g[t + "itemar_keys"])
        if seed == 0:
            assert np.array_equal(i64["xyz"].cpu().numpy(), g[t + "item64_xyz"])
            assert np.array_equal(iar["autoregressive_cond"].cpu().numpy(), g[t + "itemar_cond"])
        else:
            wts = np.arange(1, 2 * 32 * 1024 + 1, dtype=np.float64).reshape(2, 32, 1024)
            dig = np.array([float((iar["autoregressive_cond"].cpu().numpy() * wts).sum()),
                            float(np.abs(i64["xyz"].cpu().numpy()).sum(dtype=np.float64))])
            assert np.array_equal(dig, g[t + "itemar_cond_digest"])
        itb = CustomDataset([dict(gt_boxes=first["gt_boxes"].copy(), gt_names=list(first["gt_names"]))])[0]
        assert sorted(itb.keys()) == list(g[t + "itemb_keys"])
        assert np.array_equal(itb["condition_mask"].cpu().numpy(), g[t + "itemb_condition_mask"])


def test_next_frame_points_vs_reference_golden(dev, golden):
    """refine_next_frame_points / get_next_frame_points on the device vs outputs of the REFERENCE's
    own pipe_related.py run through its own CustomDataset (tests/golden/pipe_next.npz), chained over
    two future frames like sample_and_save_temporal.py:296-327.  Each call gets the inputs the
    reference's call got (rebuilt with the oracle's reference flow, which the CPU suite proves
    bit-exact): the re-projected background -- float64 `Ts @ homo`, float64 projection, mask,
    compaction -- is BIT-IDENTICAL (count, order, values); the re-posed object rows (the
    reference's float32 library matmuls vs correctly rounded values) agree to two float32 ulps."""
    import lidargen  # noqa: F401
    from lidargen.utils import temporal as T
    from lidarcrafter_amd import ops as K
    from oracle import temporal as OT

    g = golden("pipe_next")
    for seed in (0, 1):
        first, pts, _ = _temporal_scene(seed)
        t = f"s{seed}_"
        rfirst = dict(first)
        rfirst["xyz"], rfirst["reflectance"] = g[t + "item_xyz"], g[t + "item_reflectance"]
        _, rfut_bg, _, fut_boxes, Ts, robj_pts, robj_int = OT.get_temporal_boxes_3d(rfirst, f32=False)
        dfirst = dict(rfirst)
        for k in ("xyz", "reflectance", "condition_mask"):
            dfirst[k] = torch.from_numpy(np.ascontiguousarray(rfirst[k])).to(dev)
        _, fut_bg, _, dfut_boxes, dTs, obj_pts, obj_int = T.get_temporal_boxes_3d(dfirst)
        assert np.allclose(dfut_boxes, g[t + "fut_boxes"], rtol=0, atol=1e-11)
        assert np.allclose(dTs, g[t + "Ts"], rtol=0, atol=1e-11)
        xyz, refl = rfirst["xyz"], rfirst["reflectance"]
        cur = np.stack([xyz[0], xyz[1], xyz[2], refl[0]], -1).reshape(-1, 4)
        dcur_chain = torch.from_numpy(cur).to(dev)
        for f in range(2):
            ref = g[t + f"next{f}"]
            n = int(g[t + f"refine{f}_n"][0])
            dcur = torch.from_numpy(np.ascontiguousarray(cur, np.float32)).to(dev)
            moved = K.transform_points(dcur, Ts[f], f64="keep")
            assert moved.dtype == torch.float64
            rbg = T.refine_next_frame_points([dict(
                points=moved, gt_boxes=np.concatenate([np.zeros((1, 7)), fut_boxes[:, f]]),
                gt_names=list(first["gt_names"]))])
            assert rbg.dtype == torch.float32 and np.array_equal(rbg.cpu().numpy(), ref[:n])
            nxt = T.get_next_frame_points(dcur, obj_pts, obj_int, fut_boxes[:, f],
                                          list(first["gt_names"]), Ts[f])
            assert nxt.dtype == torch.float64 and tuple(nxt.shape) == ref.shape
            a = nxt.cpu().numpy()
            assert np.array_equal(a[:n], ref[:n])
            assert ref.shape[0] - n > 1000 and np.abs(a[n:] - ref[n:]).max() <= 1.6e-5
            assert np.array_equal(a[n:, 3], ref[n:, 3])
            # the same call on the reference's own float32 object points: only the float32
            # rotation of get_next_frame_points itself is left between the two -> one ulp
            nx2 = T.get_next_frame_points(
                dcur, [torch.from_numpy(p).to(dev) for p in robj_pts],
                [torch.from_numpy(i).to(dev) for i in robj_int], fut_boxes[:, f],
                list(first["gt_names"]), Ts[f]).cpu().numpy()
            assert np.abs(nx2[n:] - ref[n:]).max() <= 7.7e-6
            gen = synth_points(32 * 1024, seed=300 + 10 * seed + f)
            cur = OT.delete_fg_points(np.concatenate([rfut_bg[f], gen], axis=0), fut_boxes[:, f])
            assert cur.dtype == np.float32 and cur.shape[0] == int(g[t + f"cur{f}_n"][0])
            # device-only chain: every stage on the device, never re-seeded from the oracle
            dnx = T.get_next_frame_points(dcur_chain, obj_pts, obj_int, fut_boxes[:, f],
                                          list(first["gt_names"]), Ts[f])
            assert abs(dnx.shape[0] - ref.shape[0]) <= 8
            comb = torch.cat([fut_bg[f], torch.from_numpy(gen).to(dev)], dim=0).contiguous()
            dcur_chain = T.delete_fg_points(comb, fut_boxes[:, f])
            assert abs(dcur_chain.shape[0] - cur.shape[0]) <= 8


@pytest.mark.parametrize("seed", [0, 1])
def test_temporal_frame_glue_vs_oracle(dev, seed):
    """get_temporal_boxes_3d -> get_next_frame_points -> delete_fg_points for two frames, device
    vs the oracle's device-contract flow (oracle/temporal.py header; the oracle's reference flow is
    pinned bit-exactly on the reference's outputs): identical point selections and order,
    coordinates bit-equal (same float64 4x4s)."""
    import lidargen  # noqa: F401
    from lidargen.utils import temporal as T
    from oracle import temporal as OT

    first, _, _ = _temporal_scene(seed)
    dfirst = dict(first)
    for k in ("xyz", "reflectance", "condition_mask"):
        dfirst[k] = torch.from_numpy(np.ascontiguousarray(first[k])).to(dev)
    names = first["gt_names"]
    bg, fut_bg, boxes, fut_boxes, Ts, obj_pts, obj_int = T.get_temporal_boxes_3d(dfirst, M=None)
    rbg, rfut_bg, rboxes, rfut_boxes, rTs, robj_pts, robj_int = OT.get_temporal_boxes_3d(first, M=None)
    assert np.array_equal(bg.cpu().numpy(), rbg)
    assert np.array_equal(fut_bg.cpu().numpy(), rfut_bg)
    assert np.allclose(fut_boxes, rfut_boxes, rtol=0, atol=1e-12) and np.array_equal(Ts, rTs)
    assert sum(p.shape[0] for p in obj_pts) > 50            # the scene does have object points
    for k in range(len(obj_pts)):
        assert np.array_equal(obj_pts[k].cpu().numpy(), robj_pts[k]), k
        assert np.array_equal(obj_int[k].cpu().numpy(), robj_int[k]), k
    cur, rcur = bg, rbg
    for t in range(2):
        nxt = T.get_next_frame_points(cur, obj_pts, obj_int, rfut_boxes[:, t], names, rTs[t])
        rnxt = OT.get_next_frame_points(rcur, robj_pts, robj_int, rfut_boxes[:, t], names, rTs[t])
        assert np.array_equal(nxt.cpu().numpy(), rnxt), t
        assert nxt.dtype == torch.float64 and rnxt.dtype == np.float64
        # (the rounded set stands in for the sampled frame, which is float32 in the reference)
        comb = torch.cat([fut_bg[t], nxt.float()], dim=0).contiguous()
        rcomb = np.concatenate([rfut_bg[t], rnxt.astype(np.float32)], axis=0)
        cur = T.delete_fg_points(comb, rfut_boxes[:, t])
        rcur = OT.delete_fg_points(rcomb, rfut_boxes[:, t])
        assert np.array_equal(cur.cpu().numpy(), rcur), t
        assert 0 < cur.shape[0] < comb.shape[0]


def test_temporal_glue_vs_reference_golden(dev, golden):
    """Device get_temporal_boxes_3d / delete_fg_points vs outputs of the REFERENCE's own
    pipe_related.py (tests/golden/pipe.npz): identical point selections and order; coordinates within
    one float32 ulp (the device keeps float32 rows and rounds once, the reference carries float64
    between stages -- DESIGN section 5b)."""
    import lidargen  # noqa: F401
    from lidargen.utils import temporal as T

    g = golden("pipe")
    for seed in (0, 1):
        first, _, _ = _temporal_scene(seed, H=8, W=256, n_pts=6000)
        t = f"s{seed}_"
        dfirst = dict(first)
        for k in ("xyz", "reflectance", "condition_mask"):
            dfirst[k] = torch.from_numpy(np.ascontiguousarray(first[k])).to(dev)
        bg, fut_bg, boxes, fut_boxes, Ts, obj_pts, obj_int = T.get_temporal_boxes_3d(dfirst, M=None)
        assert np.array_equal(bg.cpu().numpy(), g[t + "bg"])
        # host float64 trigonometry: last-ulp differences between numpy builds / CPUs are allowed
        assert np.allclose(np.asarray(fut_boxes), g[t + "fut_boxes"], rtol=0, atol=1e-11)
        assert np.allclose(np.asarray(Ts), g[t + "Ts"], rtol=0, atol=1e-11)
        assert np.abs(fut_bg[0].cpu().numpy() - g[t + "fut_bg_first"]).max() <= 7.7e-6
        assert np.abs(fut_bg[-1].cpu().numpy() - g[t + "fut_bg_last"]).max() <= 7.7e-6
        assert np.array_equal(np.array([p.shape[0] for p in obj_pts]), g[t + "obj_n"])
        assert np.abs(torch.cat(obj_pts).cpu().numpy() - g[t + "obj_pts"]).max() <= 1e-6
        assert np.array_equal(torch.cat(obj_int).cpu().numpy(), g[t + "obj_int"])
        comb = torch.cat([fut_bg[0], bg], dim=0).contiguous()
        kept = T.delete_fg_points(comb, g[t + "fut_boxes"][:, 0])
        assert kept.shape[0] == g[t + "delete_fg"].shape[0]
        assert np.abs(kept.cpu().numpy() - g[t + "delete_fg"]).max() <= 7.7e-6
        m9 = T.get_temporal_boxes_3d(dfirst, M=9)
        assert np.allclose(np.asarray(m9[3]), g[t + "M9_fut_boxes"], rtol=0, atol=1e-11)
        assert np.allclose(np.asarray(m9[4]), g[t + "M9_Ts"], rtol=0, atol=1e-11)


def test_generate_sequence_device_loop(dev):
    """sample_and_save_temporal.py:198-331 as one device-resident loop (reduced-width models at
    8x64): frame 0 layout-conditioned, frames 1-2 autoregressive; deterministic under per-sample
    generators, finite, and frame t+1's autoregressive condition really is the re-projected,
    ego-motion-compensated frame t (checked against the oracle glue for sample 0)."""
    import lidargen  # noqa: F401
    from lidargen.dataset.custom_dataset import CustomDataset, DataConfig
    from lidargen.models.diffusion import CondContinuousTimeGaussianDiffusion
    from lidargen.utils import temporal as T
    from lidargen.utils.lidar import LiDARUtility
    from lidarcrafter_amd.testing import synth_scene_boxes, synth_temporal_inputs
    from tests.test_oracle_vs_golden import build_cond_pair

    H, W, B, K_ = 8, 64, 2, 4
    m0, e0 = build_cond_pair((H, W), 8, 32, cond_out=10)
    m1, e1 = build_cond_pair((H, W), 8, 32, cond_out=11)
    ddpm = CondContinuousTimeGaussianDiffusion(m0, e0, cond_mode="concat").eval().to(dev)
    auto = CondContinuousTimeGaussianDiffusion(m1, e1, cond_mode="concat").eval().to(dev)
    lu = LiDARUtility(resolution=(H, W), depth_format="log_depth", min_depth=1.45, max_depth=80.0,
                      ray_angles=m0.coords).to(dev)

    class Cfg(DataConfig):
        resolution = (H, W)

    infos = []
    for b in range(B):
        sb = synth_scene_boxes(K_, seed=40 + b)
        names = ["ego"] + [DataConfig.class_names[int(c) - 1] for c in sb[:, 7]]
        infos.append(dict(gt_boxes=np.concatenate([np.zeros((1, 7)), sb[:, :7].astype(np.float64)]),
                          gt_names=names, gt_fut_trajs=synth_temporal_inputs(50 + b, K=K_)[0]))
    ds = CustomDataset([dict(d) for d in infos], cfg=Cfg())
    batch = ds.collate_fn([ds[i] for i in range(B)])
    batch["gt_fut_trajs"] = [d["gt_fut_trajs"] for d in infos]

    def run():
        rng = [torch.Generator().manual_seed(90 + i) for i in range(B)]
        return T.generate_sequence(ddpm, auto, lu, dict(batch), num_frames=3, num_steps=3,
                                   mode="ddpm", traj_length=6, rng=rng, data_cfg=Cfg())

    frames, points = run()
    frames2, _ = run()
    assert len(frames) == 3 and all(f.shape == (B, 5, H, W) for f in frames)
    assert all(torch.isfinite(f).all() for f in frames)
    assert all(torch.equal(a, b) for a, b in zip(frames, frames2))
    assert not torch.equal(frames[1], frames[2])
    assert points[1][0].shape == (H * W, 4)


def test_condition_caches_follow_the_condition(dev):
    """Step-invariant condition operands are cached per sampling run.  A second run whose condition
    tensors land on the addresses the first run freed (caching allocator) must not see the first
    run's operands: sample(A); sample(B) == a fresh model's sample(B)."""
    from lidarcrafter_amd.testing import synth_layout_batch
    from lidargen.models.diffusion import CondContinuousTimeGaussianDiffusion
    from tests.test_oracle_vs_golden import build_cond_pair

    def fresh():
        m, e = build_cond_pair((8, 64), 8, 32)
        return CondContinuousTimeGaussianDiffusion(m, e, cond_mode="concat").eval().to(dev)

    def run(ddpm, seed):
        batch = {k: v.to(dev) for k, v in synth_layout_batch(2, 8, 64, seed=seed).items()}
        rng = [torch.Generator().manual_seed(5 + i) for i in range(2)]
        return ddpm.sample(batch, 2, 4, progress=False, rng=rng, mode="ddim").cpu()

    a = fresh()
    run(a, 71)
    second = run(a, 72)
    assert torch.equal(second, run(fresh(), 72))
    assert not torch.equal(second, run(fresh(), 71))


# ------------------------------------------------------------------------------------- BEV metrics
def test_bev_metrics_vs_reference_golden(dev, golden):
    """lidargen.metrics.bev on the device vs the reference's own bev.py outputs: histogram counts
    bit-exact (incl. points on the range edges), JSD / MMD to 1e-6."""
    import lidargen  # noqa: F401
    from lidargen.metrics import bev
    from oracle import metrics as OM
    from tests.test_oracle_vs_golden import _bev_clouds

    g = golden("bev")
    hs = []
    for cl, key in zip(_bev_clouds(), ("hist_a", "hist_b")):
        h = torch.stack([bev.point_cloud_to_histogram(torch.from_numpy(p).to(dev)) for p in cl])
        assert np.array_equal(h.cpu().numpy(), g[key].astype(np.float32)), key
        hs.append(h)
    small = bev.point_cloud_to_histogram(
        torch.from_numpy(synth_points(3000, seed=5)[:, :3] * np.float32(0.02)).to(dev),
        min_depth=1e-6, max_depth=1e3, field_size=2.0)
    assert np.array_equal(small.cpu().numpy(), g["hist_small"].astype(np.float32))
    # [N,4] rows (the sampler's point format) bin like [N,3]
    p4 = torch.from_numpy(synth_points(5000, seed=9)).to(dev)
    assert torch.equal(bev.point_cloud_to_histogram(p4), bev.point_cloud_to_histogram(p4[:, :3].contiguous()))
    assert abs(bev.compute_jsd_2d(hs[0], hs[1]) - float(g["jsd"])) < 1e-6
    assert abs(bev.compute_mmd_2d(hs[0], hs[1]) - float(g["mmd"])) < 1e-6
    # ragged pair counts (M, Mq not multiples of the 16 x 16 pair tile) against float64: each
    # kernel mean to 1e-6 relative (fp32 exp); their difference (the MMD, ~1e-4 out of terms ~1)
    # only to the absolute error of the terms
    gen = torch.Generator().manual_seed(11)
    a = torch.rand(37, 300, generator=gen)
    b = torch.rand(21, 300, generator=gen)
    a, b = a / a.sum(1, keepdim=True), b / b.sum(1, keepdim=True)

    def kmean(u, v):
        d2 = ((u.double()[:, None, :] - v.double()[None, :, :]) ** 2).sum(-1)
        return float(torch.exp(-2.0 * d2).mean())            # gamma = 1 / (2 * 0.5^2)

    ad, bd = a.to(dev), b.to(dev)
    for u, v, ud, vd in ((a, a, ad, ad), (b, b, bd, bd), (a, b, ad, bd)):
        got = bev.cdist_rbf_mean(ud, vd).item()
        assert abs(got - kmean(u, v)) < 1e-6 * kmean(u, v)
    mmd = (bev.cdist_rbf_mean(ad, ad) + bev.cdist_rbf_mean(bd, bd) - 2 * bev.cdist_rbf_mean(ad, bd)).item()
    assert abs(mmd - OM.compute_mmd_2d(a.numpy(), b.numpy())) < 5e-7


# ------------------------------------------------------------------------------------- sampler extras
def test_sampler_extras_golden(dev, golden):
    """q_step_from_x_0, q_step, RePaint, conditional inpaint and the training-loss VALUE of the HIP
    path vs the reference's own outputs (tests/golden/sampler_extras.npz)."""
    from lidarcrafter_amd.testing import synth_layout_batch
    from lidargen.models.diffusion import (CondContinuousTimeGaussianDiffusion,
                                           ContinuousTimeGaussianDiffusion)
    from tests.test_oracle_vs_golden import build_cond_pair

    g = golden("sampler_extras")
    m = _uncond(16, (8, 64), dev)
    ddpm = ContinuousTimeGaussianDiffusion(m, torch.nn.Identity()).eval().to(dev)
    x0 = seeded_randn(2, 2, 8, 64, seed=71).clamp(-1, 1).to(dev)
    steps = torch.tensor([0.8, 0.3], device=dev)
    rng = [torch.Generator().manual_seed(300 + i) for i in range(2)]
    xt, noise = ddpm.q_step_from_x_0(x0, steps, rng=rng)
    assert torch.equal(noise.cpu(), T(g["q0_noise"])) and rel_l2(xt, T(g["q0_xt"])) < 1e-6
    rng = [torch.Generator().manual_seed(310 + i) for i in range(2)]
    qs = ddpm.q_step(T(g["q0_xt"]).to(dev), torch.tensor([0.9, 0.5], device=dev), steps, rng=rng)
    assert rel_l2(qs, T(g["q_step"])) < 1e-6
    mask = T(g["mask"]).to(dev)
    rng = [torch.Generator().manual_seed(320 + i) for i in range(2)]
    rp = ddpm.repaint(x0, mask, num_steps=4, num_resample_steps=2, jump_length=2, progress=False,
                      rng=rng, return_all=True).cpu()
    ref = T(g["repaint"])
    assert rp.shape == ref.shape and torch.equal(rp[0], ref[0])
    for i in range(1, rp.shape[0]):
        assert rel_l2(rp[i], ref[i]) < 1e-3, (i, rel_l2(rp[i], ref[i]))
    for obj, lt, msw in (("eps", "l2", True), ("v", "l2", True), ("x_0", "l2", True),
                         ("eps", "l1", False), ("v", "huber", True)):
        d2 = ContinuousTimeGaussianDiffusion(m, torch.nn.Identity(), prediction_type=obj, loss_type=lt,
                                             min_snr_loss_weight=msw).eval().to(dev)
        torch.manual_seed(5)
        # the reference draws the loss noise from the global CPU generator on CPU tensors; draw
        # the same numbers here and hand them over through a per-sample-free generator call
        noise = torch.randn(2, 2, 8, 64)
        a, s = d2.log_snr(steps.cpu()).sigmoid().sqrt(), (-d2.log_snr(steps.cpu())).sigmoid().sqrt()
        x_t = (x0.cpu() * a + noise * s).to(dev)
        with torch.no_grad():
            pred = d2.model(x_t, d2.get_network_condition(steps))
        got = d2._masked_loss(pred, d2.get_target(x0, steps, noise.to(dev)), torch.ones_like(x0), steps)
        want = float(g[f"loss_{obj}_{lt}_{int(msw)}"])
        assert abs(float(got) - want) < 1e-4 * max(1.0, abs(want)), (obj, lt, float(got), want)
    mc, enc = build_cond_pair((8, 64), 8, 32)
    dc = CondContinuousTimeGaussianDiffusion(mc, enc, cond_mode="concat").eval().to(dev)
    batch = {k: v.to(dev) for k, v in synth_layout_batch(2, 8, 64, seed=73).items()}
    rng = [torch.Generator().manual_seed(330 + i) for i in range(2)]
    ip = dc.inpaint(x0, mask, batch, num_steps=3, num_resample_steps=1, jump_length=2, progress=False,
                    rng=rng, return_all=True).cpu()
    ref = T(g["inpaint"])
    assert ip.shape == ref.shape and torch.equal(ip[0], ref[0])
    for i in range(1, ip.shape[0]):
        assert rel_l2(ip[i], ref[i]) < 1e-3, (i, rel_l2(ip[i], ref[i]))


def test_discrete_time_sampler_golden(dev, golden):
    """DiscreteTimeGaussianDiffusion.sample (integer timesteps into the same HIP denoiser) vs the
    reference's states 0, 1, 25, 50 of a 50-step run (T = 50), both update rules, two beta schedules."""
    from lidargen.models.diffusion import DiscreteTimeGaussianDiffusion

    g = golden("discrete_trajectory")
    m = _uncond(16, (8, 64), dev)
    for kind in ("linear", "cosine"):
        dd = DiscreteTimeGaussianDiffusion(m, None, num_training_steps=50, noise_schedule=kind).eval().to(dev)
        for mode in ("ddpm", "ddim"):
            rng = [torch.Generator().manual_seed(400 + i) for i in range(2)]
            xs = dd.sample(2, 50, progress=False, rng=rng, return_all=True, mode=mode).cpu()[[0, 1, 25, 50]]
            ref = T(g[f"{kind}_{mode}"])
            assert torch.equal(xs[0], ref[0])
            for i in range(1, 4):
                assert rel_l2(xs[i], ref[i]) < 1e-3, (kind, mode, i, rel_l2(xs[i], ref[i]))


@pytest.mark.parametrize("B,N,M", [(2, 1000, 777), (1, 1, 5), (1, 512, 1024), (3, 300, 513)])
def test_chamfer3d_vs_unpinned_restatement(dev, B, N, M):
    """lc_chamfer3d_fwd vs the float32 numpy restatement: distances and indices identical,
    duplicates resolved to the first minimum; compute_pairwise_cd(_batch) on top of it.  The
    restatement itself is unpinned; the kernel is pinned on the reference's own chamfer3D.cu,
    hipified and compiled for gfx950 with and without FP contraction
    (tests/test_reference_kernels.py::test_chamfer3d_vs_reference_kernel)."""
    import lidargen  # noqa: F401
    from lidargen.metrics import chamfer
    from oracle import metrics as OM

    g = np.random.default_rng(B * 1000 + N)
    a = g.normal(0, 20, (B, N, 3)).astype(np.float32)
    b = g.normal(0, 20, (B, M, 3)).astype(np.float32)
    if M > 4:
        b[:, 3] = b[:, 1]                                   # a duplicated target: index 1 must win
    d1, d2, i1, i2 = chamfer.chamfer_3DDist()(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    r1, r2, j1, j2 = OM.chamfer3d(a, b)
    assert np.array_equal(d1.cpu().numpy(), r1) and np.array_equal(i1.cpu().numpy(), j1)
    assert np.array_equal(d2.cpu().numpy(), r2) and np.array_equal(i2.cpu().numpy(), j2)
    cd = chamfer.compute_pairwise_cd(a[0], b[0])
    assert abs(cd - float((r1[0].mean() + r2[0].mean()) / 2)) < 1e-4 * max(1.0, cd)
    res = chamfer.compute_pairwise_cd_batch(a[0], [b[0], b[0][: max(1, M // 2)]])
    assert abs(res[0] - cd) < 1e-4 * max(1.0, cd) and len(res) == 2
