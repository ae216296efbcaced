"""Kernel parity resolved by slice (DESIGN.md "Error profiles").  `pytest -m gpu`.

The other kernel tests judge a kernel by one relative-L2 figure over the whole output, which dilutes a fault confined to
n of N outputs by sqrt(n / N).  The paths in which these kernels differ from the textbook -- halo rows and the ring-wrap
column, the kept halo rows of the tall kernel, the variant border rows of the stride-2 fold, the border taps of the
up-fold, the last partial 64-channel chunk, split-K partial sums, the ragged last query block, the clamped rows of the
neighbourhood attention, the K tail of the skinny GEMM -- are all thin slices.  Here the same figure is computed per
sample, channel, row, column and pixel (`lidarcrafter_amd.testing.error_profiles`) and every slice is held to

  bound        slice error <= tol * max(1, r_ref)          tol: the whole-tensor tolerance of the kernel's existing test
  uniformity   worst slice / median slice <= 2 * u_ref

with r_ref (worst slice / whole tensor) and u_ref (worst / median slice) measured at run time on the CPU float32
evaluation of the same operation against its float64 twin, at the same shape and slicing (tests/_profile_cases.py, which
tests/test_error_profiles_host.py checks on its own).  No test here reads anything outside the repository.

Measured on the MI355X (the figures `assert_profiles` prints; per family the maximum over its cases and profiles, so a
kernel's ratio and the reference's ratio in one row may come from different profiles -- each profile is held to its own):

  family                                          whole    tol  worst/whole r_ref  worst/median u_ref
  conv, bias + residual + scale (cfg matrix)    2.9e-07  2e-06         1.91  1.61          1.95  1.61
  conv, fused GroupNorm + AdaGN + SiLU          2.8e-07  3e-06         1.85  1.56          1.88  1.95
  conv, statistics-emitting epilogue            2.9e-07  2e-06         1.72  1.61          1.74  1.61
  conv, pre-split routes (3x3, 1x1)             1.7e-07  2e-06         1.66  1.56          1.67  1.95
  conv, split-K forced                          1.5e-07  2e-06         1.58  1.53          1.60  1.55
  stride-2 fold-down, default form              1.5e-07  2e-06         3.31  2.49          2.88  2.19
  stride-2 fold-down, LC_S2_FORM=1 (child)      1.5e-07  2e-06         3.31  2.49          2.88  2.19
  up-fold                                       1.5e-07  2e-06         1.72  1.66          1.57  1.56
  up-fold, xup output                           5.1e-08  1e-06         1.44  1.44          1.46  1.46
  resample2x                                    6.9e-08  1e-06         1.17  1.17          1.15  1.15
  groupnorm_resample_pair                       7.2e-08  1e-06         1.20  1.19          1.21  1.20
  GroupNorm, statistics pass                    8.7e-08  2e-06         1.61  2.23          1.67  2.40
  GroupNorm, large mean                         5.5e-05  1e-04         1.55  1.64          2.24  2.26
  GroupNorm from producer entries               1.1e-07  2e-06         1.89  3.16          2.16  4.10
  attention_cm f32 / f16x2                      5.5e-07  2e-06         2.20  2.13          2.13  2.08
  attention_units (8, 8, 64, 512)               5.3e-07  2e-06         2.41  2.71          2.35  2.66
  neighbourhood attention                       9.1e-07  1e-05         2.04  1.99          3.77  3.98
  skinny linear                                 2.9e-07  2e-06         1.27  1.39          1.23  1.35
  rowprep                                       8.6e-08  2e-06         1.13  1.16          1.13  1.17
  conv dx                                       4.2e-07  2e-06         1.16  1.16          1.17  1.15
  conv dw                                       2.3e-07  2e-06         1.15  1.16          1.16  1.17
  flash attention dq / dk / dv                  8.6e-07  3e-06         2.61  2.05          3.13  2.14
  GroupNorm dx                                  8.8e-08  5e-06         1.64  1.78          1.69  1.96
  neighbourhood attention dq / dk / dv          4.6e-06  5e-05         2.37  3.14          2.98  4.33

No kernel failed a condition; the two forms of the stride-2 fold give the same figures in every profile (the same bits).
Profiles left out by the 64-element rule are printed as NOT CHECKED: only the skinny-linear / rowprep profiles over
fewer than 64 rows or columns.  Closest to the uniformity limit 2 u_ref: flash attention dv / dk by key with the f32
backward (3.06 of 3.94, 3.13 of 4.28), dq by query with the f16x2 backward (2.91 of 3.81); the stride-2 fold by output
channel (2.88 of 4.38); the conv cfg matrix on the pixel map (1.95 of 3.23).
"""
import pytest
import torch

from lidarcrafter_amd.testing import seeded_randn
from tests import _profile_cases as PC
from tests import test_presplit as _TP

pytestmark = pytest.mark.gpu
_L = PC.existing_lists()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def assert_profiles(got, ref32, ref64, keeps, tol, name, margins=None):
    """Both conditions on every profile; prints every figure before it asserts (as near_reference in test_layout_gen)."""
    lines, fails = PC.check_profiles(got, ref32, ref64, keeps, tol, margins=margins, name=name)
    print("\n".join(lines))
    assert not fails, "\n".join(fails)


def _conv_ids(cfgs):
    """(prec, cfg) with test_conv's rule: the pipelined tile configurations exist for the f16x2 kernel only."""
    return [("f32", c) for c in cfgs if c <= 5] + [("f16x2", c) for c in cfgs]


def _pp_ok(shape):
    B, Ci, Co, H, W, ks = shape
    return ks == 3 and Ci % 16 == 0 and Ci >= 64 and Co % 64 == 0 and H % 8 == 0 and W % 64 == 0


# ------------------------------------------------------------------------------------------------ forward conv
@pytest.mark.parametrize("prec,cfg", _conv_ids(_L["conv_cfgs"]))
@pytest.mark.parametrize("shape", PC.CONV_SHAPES, ids=str)
def test_conv_bias_residual_scale(dev, shape, prec, cfg):
    from lidarcrafter_amd import ops as K

    if cfg == 33 and not _pp_ok(shape):
        pytest.skip("outside the ping-pong kernel's shapes (the launcher refuses them: test_abi)")
    c = PC.conv_case(shape, "plain")
    t = c.dev(dev)
    y = K.conv2d_ring(t["x"], K.PackedConv(), t["w"], t["b"], res=t["res"], out_scale=0.7071, tile_cfg=cfg, precision=prec)
    assert_profiles(y, c.ref32, c.ref64, PC.NCHW_KEEPS, PC.TOL_CONV, f"conv {shape} {prec} cfg {cfg}")


@pytest.mark.parametrize("cfg", _L["gn_cfgs"])
@pytest.mark.parametrize("shape", PC.CONV_SHAPES, ids=str)
def test_conv_fused_groupnorm_adagn_silu(dev, shape, cfg):
    from lidarcrafter_amd import ops as K

    B, Ci = shape[:2]
    c = PC.conv_case(shape, "gn")
    t = c.dev(dev)
    co = K.groupnorm_coeffs(t["x"], PC.gn_groups(Ci), 1e-6, t["ga"], t["be"], t["ss"][:, :Ci], t["ss"][:, Ci:])
    y = K.conv2d_ring(t["x"], K.PackedConv(), t["w"], t["b"], res=t["res"], out_scale=0.7071, tile_cfg=cfg,
                      precision="f16x2", gn_coeffs=co, gn_silu=True)
    assert_profiles(y, c.ref32, c.ref64, PC.NCHW_KEEPS, PC.TOL_CONV_GN, f"conv+gn {shape} cfg {cfg}")


@pytest.mark.parametrize("cfg", [0, 13, 23, 27, 33])
@pytest.mark.parametrize("unit", [True, 2])
@pytest.mark.parametrize("shape", [s for s in PC.CONV_SHAPES if s[5] == 3 and s[2] % 8 == 0], ids=str)
def test_conv_emitting_statistics(dev, shape, unit, cfg):
    """The epilogue that also leaves GroupNorm statistics entries (octets, pairs) stores the same output."""
    from lidarcrafter_amd import ops as K

    if cfg == 33 and not _pp_ok(shape):
        pytest.skip("outside the ping-pong kernel's shapes (the launcher refuses them: test_abi)")
    c = PC.conv_case(shape, "plain")
    t = c.dev(dev)
    y = K.conv2d_ring(t["x"], K.PackedConv(), t["w"], t["b"], res=t["res"], out_scale=0.7071, tile_cfg=cfg, emit_stats=unit)
    assert_profiles(y, c.ref32, c.ref64, PC.NCHW_KEEPS, PC.TOL_CONV, f"conv emit_stats={unit} {shape} cfg {cfg}")


def _presplit(K, c, t, Ci, pk):
    return K.groupnorm(t["x"], PC.gn_groups(Ci), 1e-6, t["ga"], t["be"], t["ss"][:, :Ci], t["ss"][:, Ci:], act_silu=True,
                       split_for=pk)


# 3x3: every tile configuration of test_presplit::test_conv_presplit_vs_oracle; the pre-split 1x1 kernel has one
_PS_CASES = [(s, cfg) for s in PC.CONV_SHAPES if s[1] % 16 == 0
             for cfg in (PC._marks(_TP.test_conv_presplit_vs_oracle, "cfg") if s[5] == 3 else [0])]


@pytest.mark.parametrize("shape,cfg", _PS_CASES, ids=str)
def test_conv_presplit_routes(dev, shape, cfg):
    """GroupNorm apply + fp16 split, then the LDS-DMA kernels: 3x3 (every tile configuration of test_presplit) and 1x1."""
    from lidarcrafter_amd import ops as K

    Ci = shape[1]
    c = PC.conv_case(shape, "gn")
    t = c.dev(dev)
    pk = K.PackedConv("ps")
    sa = _presplit(K, c, t, Ci, pk)
    assert isinstance(sa, K.SplitAct)
    y = K.conv2d_ring(sa, pk, t["w"], t["b"], res=t["res"], out_scale=0.7071, tile_cfg=cfg)
    assert not K.range_poll(dev)
    assert_profiles(y, c.ref32, c.ref64, PC.NCHW_KEEPS, PC.TOL_CONV_PS, f"conv presplit {shape} cfg {cfg}")


@pytest.mark.parametrize("ksplit", [2, 4])
@pytest.mark.parametrize("shape", [s for s in PC.CONV_SHAPES if s[1] % 16 == 0 and s[5] == 3], ids=str)
def test_conv_split_k_forced(dev, shape, ksplit, monkeypatch):
    """Split-K forced on (the developer switch LC_SPLITK_FORCE = "ks:cfg"): partial sums over disjoint K ranges + the
    reduce pass, with its statistics output."""
    from lidarcrafter_amd import ops as K

    Ci = shape[1]
    monkeypatch.setattr(K, "_SPLITK_FORCE", (ksplit, 0, 0))
    c = PC.conv_case(shape, "gn")
    t = c.dev(dev)
    pk = K.PackedConv("splitk")
    sa = _presplit(K, c, t, Ci, pk)
    y = K.conv2d_ring(sa, pk, t["w"], t["b"], res=t["res"], out_scale=0.7071, emit_stats=True)
    assert_profiles(y, c.ref32, c.ref64, PC.NCHW_KEEPS, PC.TOL_CONV_PS, f"conv split-K {ksplit} {shape}")


# ------------------------------------------------------------------------------------------------ the two folds
@pytest.mark.parametrize("shape", PC.FOLD_SHAPES, ids=str)
def test_fold_down(dev, shape):
    """FIR pre-filter + stride-2 conv against the unfolded float64 conv + FIR, in the default form of LC_S2_FORM (the
    launcher reads it once per process: test_fold_down_first_form runs the other form in a child process)."""
    from lidarcrafter_amd import ops as K

    c = PC.fold_case(shape, "down")
    t = c.dev(dev)
    y = K.conv_down2(t["x"], K.PackedConv("down"), t["w"], t["b"], emit_stats=True)
    assert not K.range_poll(dev)
    assert_profiles(y, c.ref32, c.ref64, PC.NCHW_KEEPS, PC.TOL_FOLD, f"fold-down {shape}")


def test_fold_down_first_form(dev, tmp_path):
    """LC_S2_FORM=1, the first form of the stride-2 conv (conv_f16x2_ps_kernel<.., S2>, weights re-loaded per tile), in a
    fresh child process (tests/_fold_down_child.py); the same conditions on what it hands back."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.environ.get("LC_S2_FORM", "2") != "1", "this process must run the default form"
    res = tmp_path / "fold_down_form1.pt"
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_fold_down_child.py"), str(res)], cwd=root,
                       env=dict(os.environ, LC_S2_FORM="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout.decode(), r.stdout.decode()[-2000:]
    got = torch.load(res)
    assert got["form"] == "1"
    for shape in PC.FOLD_SHAPES:
        c = PC.fold_case(shape, "down")
        assert_profiles(got[str(shape)], c.ref32, c.ref64, PC.NCHW_KEEPS, PC.TOL_FOLD, f"fold-down form 1 {shape}")


@pytest.mark.parametrize("xup", [False, True])
@pytest.mark.parametrize("shape", PC.FOLD_SHAPES, ids=str)
def test_fold_up(dev, shape, xup, monkeypatch):
    from lidarcrafter_amd import ops as K

    monkeypatch.setattr(K, "FOLD_UP_MIN_CI", 32)
    c = PC.fold_case(shape, "up")
    t = c.dev(dev)
    pk = K.PackedConv("up9")
    y = K.conv_up2(K.split_act(t["x"], pk), pk, K.up9_weight(t["w"]), t["b"], emit_stats=True, up_also=t["x2"] if xup else None)
    assert not K.range_poll(dev)
    if xup:
        y, y2 = y
        assert_profiles(y2, c.ref32[1], c.ref64[1], PC.NCHW_KEEPS, PC.TOL_RESAMPLE, f"fold-up xup {shape}")
    assert_profiles(y, c.ref32[0], c.ref64[0], PC.NCHW_KEEPS, PC.TOL_FOLD, f"fold-up {shape} xup={xup}")


# ------------------------------------------------------------------------------------------------ resampling
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("shape", PC.RESAMPLE_SHAPES, ids=str)
def test_resample2x(dev, shape, up):
    from lidarcrafter_amd import ops as K

    c = PC.resample_case(shape, up)
    y = K.resample2x(c.t["x"].to(dev), up=up)
    assert_profiles(y, c.ref32, c.ref64, ((2,), (3,)), PC.TOL_RESAMPLE, f"resample up={up} {shape}")


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("producer_stats", [True, False])
def test_groupnorm_resample_pair(dev, up, producer_stats):
    """op(SiLU(GroupNorm(x))) in one pass over a conv's output x (statistics from the producer's entries, or from a pass):
    against the CPU evaluation on that same x."""
    from lidarcrafter_amd import ops as K
    from oracle import denoiser as D

    B, C, H, W, G = 2, 64, 8, 128, 8
    src = seeded_randn(B, 32, H, W, seed=81).to(dev)
    w = seeded_randn(C, 32, 3, 3, seed=82).to(dev) / 17.0
    x = K.conv2d_ring(src, K.PackedConv(), w, None, emit_stats=True)
    if not producer_stats:
        x = x.clone()
    assert (K._find_stats(x, G) is not None) == producer_stats
    ga, be = seeded_randn(C, seed=83), seeded_randn(C, seed=84)
    a, xr = K.groupnorm_resample_pair(x, G, 1e-5, ga.to(dev), be.to(dev), up)
    op = D.resample_up2 if up else D.resample_down2
    xc = x.cpu()
    refs = [op(D.silu(D.group_norm(xc.to(dt), G, ga.to(dt), be.to(dt), 1e-5))) for dt in (torch.float32, torch.float64)]
    assert_profiles(a, refs[0], refs[1], ((2,), (3,)), PC.TOL_RESAMPLE, f"gn+resample pair up={up} producer={producer_stats}")
    assert_profiles(xr, op(xc), op(xc.double()), ((2,), (3,)), PC.TOL_RESAMPLE, f"resample of the pair up={up}")


# ------------------------------------------------------------------------------------------------ GroupNorm
def _gn_assert(y, x_cpu, p, G, tol, name):
    """y against SiLU(AdaGN(GroupNorm(x_cpu))) on the CPU: (sample, group), row, column profiles and the channel profile."""
    refs = [PC.gn_apply({k: (v.to(dt) if v is not None else None) for k, v in dict(x=x_cpu, **p).items()}, G)
            for dt in (torch.float32, torch.float64)]
    assert_profiles(PC.gn_views(y, G), PC.gn_views(refs[0], G), PC.gn_views(refs[1], G), PC.GN_KEEPS, tol, name)
    assert_profiles(y, refs[0], refs[1], ((1,),), tol, name + " by channel")


@pytest.mark.parametrize("shape", PC.GN_SHAPES, ids=str)
def test_groupnorm_statistics_pass(dev, shape):
    from lidarcrafter_amd import ops as K

    B, C, H, W, G = shape
    c = PC.gn_case(shape)
    t = c.dev(dev)
    y = K.groupnorm(t["x"], G, 1e-6, t["ga"], t["be"], t["ss"][:, :C], t["ss"][:, C:], act_silu=True)
    assert_profiles(PC.gn_views(y, G), PC.gn_views(c.ref32, G), PC.gn_views(c.ref64, G), PC.GN_KEEPS, PC.TOL_GN, f"gn {shape}")
    assert_profiles(y, c.ref32, c.ref64, ((1,),), PC.TOL_GN, f"gn {shape} by channel")


def test_groupnorm_large_mean(dev):
    from lidarcrafter_amd import ops as K

    c = PC.gn_large_mean_case()
    y = K.groupnorm(c.t["x"].to(dev), 8, 1e-6)
    assert_profiles(PC.gn_views(y, 8), PC.gn_views(c.ref32, 8), PC.gn_views(c.ref64, 8), PC.GN_KEEPS, PC.TOL_GN_LARGE_MEAN,
                    "gn large mean")


@pytest.mark.parametrize("producer,G", [("octet", 8), ("quad", 16), ("pair", 32), ("per_channel", 8), ("conv1x1", 8)])
def test_groupnorm_from_producer_entries(dev, producer, G):
    """lc_groupnorm_apply_os from the entries of each unit a producer leaves (octets and pairs: the fp32-input 3x3 conv;
    quads: the pre-split conv; per channel: the down-sampler; octets of a 1x1 conv), at (2, 64, 8, 128): against the CPU
    GroupNorm of the tensor the producer stored.  The other GroupNorm shape, (3, 96, 5, 50, G = 32), has 3 channels per
    group: a group must be a whole number of entries (ops._find_stats), so only per-channel entries could feed it, and
    their two producers write whole 128-column segments (the down-sampler's vector kernel: input W % 256; the up-fold's
    combine pass: output W % 256) -- no producer leaves entries at W = 50, that shape runs the statistics pass only."""
    from lidarcrafter_amd import ops as K

    B, C, H, W = PC.GN_SHAPES[1][:4]
    src = (seeded_randn(B, 32, H, W, seed=91) + 0.2).to(dev)
    w3 = (seeded_randn(C, 32, 3, 3, seed=92) / 17.0).to(dev)
    bias = (seeded_randn(C, seed=93) * 2.0).to(dev)                 # means far from the pivot
    if producer == "octet":
        x = K.conv2d_ring(src, K.PackedConv(), w3, bias, tile_cfg=23, emit_stats=True)
    elif producer == "pair":
        x = K.conv2d_ring(src, K.PackedConv(), w3, bias, tile_cfg=13, emit_stats=2)
    elif producer == "quad":
        pk = K.PackedConv("q")
        x = K.conv2d_ring(K.groupnorm(src, 4, 1e-6, act_silu=True, split_for=pk), pk, w3, bias, tile_cfg=23, emit_stats=4)
    elif producer == "per_channel":
        big = (seeded_randn(B, C, 2 * H, 2 * W, seed=94) * 1.2 + 0.35).to(dev)
        x = K.resample2x(big, up=False)
    else:
        w1 = (seeded_randn(C, 32, 1, 1, seed=95) / 32 ** 0.5).to(dev)
        x = K.conv2d_ring(src, K.PackedConv(), w1, bias, emit_stats=True)
    assert K._find_stats(x, G) is not None, "the producer left no entries this GroupNorm can fold"
    p = PC.gn_params(B, C)
    y = K.groupnorm(x, G, 1e-6, p["ga"].to(dev), p["be"].to(dev), p["ss"].to(dev)[:, :C], p["ss"].to(dev)[:, C:], act_silu=True)
    _gn_assert(y, x.cpu(), p, G, PC.TOL_GN, f"gn from {producer} entries")


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("prec", ["f32", "f16x2"])
@pytest.mark.parametrize("case", PC.ATTN_CASES, ids=str)
def test_attention_cm(dev, case, prec):
    """Query position, (sample, head) and value channel; the two-segment case keeps its late spike."""
    from lidarcrafter_amd import ops as K

    kind, B, heads, d, L = case
    c = PC.attn_case(*case)
    t = c.dev(dev)
    o = K.attention_cm(t["q"], t["k"], t["v"], heads, c.scale, k2=t["k2"], v2=t["v2"], precision=prec)
    assert_profiles(o.reshape(B, heads, c.dv, L), c.ref32, c.ref64, PC.ATTN_KEEPS, _L["attn_tol"][prec], f"attention {case} {prec}")


def test_attention_units(dev):
    """Keys / values in unit form need whole 32-key tiles of image keys: the two-segment operands of the 8-wave block at
    L = 512 (_profile_cases.ATTN_UNITS_CASE) instead of 500."""
    from lidarcrafter_amd import ops as K

    kind, B, heads, d, L = PC.ATTN_UNITS_CASE
    c = PC.attn_case(*PC.ATTN_UNITS_CASE)
    t = c.dev(dev)
    assert K.AttnUnits.eligible(heads, L, 13, d, 0, c.dv)
    u = K.AttnUnits(B, heads, L, 13, d, 0, c.dv, dev)
    K.attention_pack_units(u, t["k"], "k"), K.attention_pack_units(u, t["v"], "v")
    K.attention_pack_units(u, t["k2"], "k", segment=1), K.attention_pack_units(u, t["v2"], "v", segment=1)
    o = K.attention_units(t["q"], u, heads, c.scale)
    assert_profiles(o.reshape(B, heads, c.dv, L), c.ref32, c.ref64, PC.ATTN_KEEPS, _L["attn_tol"]["f16x2"], "attention units")


@pytest.mark.parametrize("d", PC.NA_D)
@pytest.mark.parametrize("grid", PC.NA_GRIDS, ids=str)
def test_neighbourhood_attention(dev, grid, d):
    from lidarcrafter_amd import ops as K

    h, w, kh, kw = grid
    c = PC.na_case(grid, d)
    t = c.dev(dev)
    o = K.hdit_na(t["q"], t["k"], t["v"], PC.NA_HEADS, h, w, (kh, kw), scale=1.0)
    assert_profiles(PC.na_view(o, grid), PC.na_view(c.ref32, grid), PC.na_view(c.ref64, grid), PC.NA_KEEPS, PC.TOL_NA,
                    f"neighbourhood attention {grid} d {d}")


# ------------------------------------------------------------------------------------------------ skinny GEMM / rowprep
@pytest.mark.parametrize("M,Kd,N", PC.SKINNY_CASES)
def test_skinny_linear(dev, M, Kd, N):
    """Row and output-column profiles.  Slices under 64 elements are left out by the helper's rule, which stays: at
    (7, 20, 512) and (33, 1664, 256) the columns (7 / 33 rows), at (37, 512, 20) rows (20) and columns (37) alike, so
    that case keeps only the whole-tensor figure here."""
    from lidarcrafter_amd import ops_skinny as S

    c = PC.skinny_case(M, Kd, N)
    t = c.dev(dev)
    y = S.skinny_linear([(t["x"], 0, Kd, None)], M, t["w"], t["b"], "relu", vec=(t["vec"], 0, t["vidx"]), res=(t["res"], 8))
    assert_profiles(y, c.ref32, c.ref64, PC.SKINNY_KEEPS, PC.TOL_SKINNY, f"skinny linear {(M, Kd, N)}")


def test_skinny_linear_gathered_geglu(dev):
    from lidarcrafter_amd import ops_skinny as S

    c = PC.skinny_geglu_case()
    t = c.dev(dev)
    y = S.skinny_linear([(t["obj"], 0, 768, t["s"]), (t["pred"], 5, 128, None), (t["obj"], 0, 768, t["o"])], 23, t["w"], None, "geglu")
    assert_profiles(y, c.ref32, c.ref64, PC.SKINNY_KEEPS, PC.TOL_SKINNY, "skinny linear gathered GEGLU")


def test_rowprep(dev):
    from lidarcrafter_amd import ops_skinny as S

    M, C, G = 37, 1024, 32
    c = PC.rowprep_case(M, C, G)
    t = c.dev(dev)
    y = S.rowprep([(t["a"], 0, C // 2, None), (t["b"], 4, C // 2, None)], M, G, 1e-5, t["ga"], t["be"], True)
    assert_profiles(y, c.ref32, c.ref64, PC.SKINNY_KEEPS, PC.TOL_SKINNY, "rowprep")


# ------------------------------------------------------------------------------------------------ backward kernels
@pytest.mark.parametrize("shape", PC.CONV_BWD_SHAPES, ids=str)
def test_conv_backward(dev, shape):
    """dx by row, column and channel; dw by tap (border handling shows in the kh = 0 / 2 taps), output and input channel."""
    from lidarcrafter_amd import autograd as AG

    c = PC.conv_bwd_case(shape)
    t = c.dev(dev)

    class M:
        pass

    m = M()
    m.weight, m.bias = t["w"].requires_grad_(), t["b"].requires_grad_()
    xd = t["x"].requires_grad_()
    AG.conv(m, xd).backward(t["g"])
    assert_profiles(xd.grad, c.ref32[0], c.ref64[0], PC.DX_KEEPS, PC.TOL_CONV_BWD, f"conv dx {shape}")
    assert_profiles(m.weight.grad, c.ref32[1], c.ref64[1], PC.DW_KEEPS, PC.TOL_CONV_BWD, f"conv dw {shape}")


@pytest.mark.parametrize("fwd,bwd", [("f16x2", "f16x2"), ("f32", "f32")])
def test_flash_attention_backward(dev, fwd, bwd, monkeypatch):
    """dq by query, dk / dv by key, both backward precisions."""
    from lidarcrafter_amd import autograd as AG

    monkeypatch.setattr(AG, "TRAIN_ATTN_FWD_PRECISION", fwd)
    monkeypatch.setattr(AG, "TRAIN_ATTN_BWD_PRECISION", bwd)
    c = PC.attn_bwd_case()
    t = c.dev(dev)
    qd, kd, vd = (t[n].requires_grad_() for n in ("q", "k", "v"))
    AG.FlashAttention.apply(qd, kd, vd, c.scale).backward(t["g"])
    for i, (n, g) in enumerate((("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)), 1):
        assert_profiles(g, c.ref32[i], c.ref64[i], ((3,),), PC.TOL_ATTN_BWD, f"flash attention {n} bwd {bwd}")


def test_groupnorm_backward(dev):
    from lidarcrafter_amd import autograd as AG

    B, C, H, W, G = PC.GN_BWD_SHAPE
    c = PC.gn_bwd_case()
    t = c.dev(dev)
    xd = t["x"].requires_grad_()
    AG.GroupNormAct.apply(xd, None, None, t["scale"], t["shift"], G, 1e-6, True).backward(t["g"])
    assert_profiles(PC.gn_views(xd.grad, G), PC.gn_views(c.ref32, G), PC.gn_views(c.ref64, G), ((0, 1),), PC.TOL_GN_BWD, "gn dx")


@pytest.mark.parametrize("d", PC.NA_D)
@pytest.mark.parametrize("grid", PC.NA_GRIDS, ids=str)
def test_neighbourhood_attention_backward(dev, grid, d):
    from lidarcrafter_amd import ops as K

    h, w, kh, kw = grid
    c = PC.na_case(grid, d, True)
    t = c.dev(dev)
    o, lse = K.hdit_na_train(t["q"], t["k"], t["v"], PC.NA_HEADS, h, w, (kh, kw))
    grads = K.hdit_na_bwd(t["q"], t["k"], t["v"], o, t["do"], lse, PC.NA_HEADS, h, w, (kh, kw))
    for i, (n, g) in enumerate(zip(("dq", "dk", "dv"), grads), 1):
        assert_profiles(PC.na_view(g, grid), PC.na_view(c.ref32[i], grid), PC.na_view(c.ref64[i], grid), PC.NA_KEEPS[:2],
                        PC.TOL_NA_BWD, f"neighbourhood attention {n} {grid} d {d}")
