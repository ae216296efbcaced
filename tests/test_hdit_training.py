"""HDiT training on the MI355X: the backward kernels of csrc/hdit_bwd.hip against float64 torch autograd of restatements
written here, the training graph (lidarcrafter_amd/autograd_hdit.py) against the reference's own loss and gradients
(tests/golden/hdit_train.npz, make_hdit_train_fixtures.py), end-to-end AdamW steps, the caches after an optimizer step,
deepcopy and DDP."""
import copy
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lidarcrafter_amd.testing import rel_l2, seeded_fill, seeded_fill_hdit, seeded_randn

pytestmark = pytest.mark.gpu

SALT = 100
PARAMS = dict(time_embed_channels=256, depths=(3, 3, 3, 3), dilation=(1, 1, 1, 1),
              positional_embedding="learnable_embedding", ring=True)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def T(a, dev="cuda"):
    return torch.as_tensor(a).to(dev)


def _close(got, ref, tol):
    err = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert err <= tol, err


# ---- kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["grid", "rows"])
@pytest.mark.parametrize("mode", ["plain", "mod", "gain"])
def test_rmsnorm_backward_against_float64(dev, form, mode):
    from lidarcrafter_amd import ops as K

    B, C = 3, 96
    x = (seeded_randn(B, C, 4, 20, seed=131) if form == "grid" else seeded_randn(B, C, seed=131)).to(dev) * 3.0
    mod = seeded_randn(B, 2 * C, seed=132).to(dev)[:, C:] if mode == "mod" else None
    gain = (1 + 0.1 * seeded_randn(C, seed=133)).to(dev) if mode == "gain" else None
    dy = seeded_randn(*x.shape, seed=134).to(dev)
    dx, df = K.hdit_rmsnorm_bwd(x, dy, mod=mod, gain=gain)
    xd = x.double().requires_grad_()
    y = xd * torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + 1e-6)
    fd = None
    if mode != "plain":
        fd = (mod if mode == "mod" else gain).double().requires_grad_()
        f = (1 + fd) if mode == "mod" else fd[None]
        y = y * (f if form == "rows" else f[:, :, None, None])
    y.backward(dy.double())
    _close(dx, xd.grad, 2e-6)
    if fd is None:
        assert df is None
    else:
        assert df.shape == fd.shape
        _close(df, fd.grad, 2e-6)


@pytest.mark.parametrize("form", ["grid", "rows"])
def test_geglu_backward_against_float64(dev, form):
    from lidarcrafter_amd import ops as K

    x = (seeded_randn(2, 2 * 48, 3, 17, seed=141) if form == "grid" else seeded_randn(5, 2 * 48, seed=141)).to(dev) * 2
    dy = seeded_randn(*((2, 48, 3, 17) if form == "grid" else (5, 48)), seed=142).to(dev)
    dx = K.hdit_geglu_bwd(x, dy)
    xd = x.double().requires_grad_()
    h, g = xd[:, :48], xd[:, 48:]
    (h * 0.5 * g * (1 + torch.erf(g / math.sqrt(2)))).backward(dy.double())
    _close(dx, xd.grad, 2e-6)


def _rope_tables(coords_hw, heads, d, harmonics):
    from lidargen.models.dits.hdit import AxialRoPE

    rope = AxialRoPE(d, heads, harmonics)
    ch, cw = coords_hw[0].reshape(-1).double(), coords_hw[1].reshape(-1).double()
    return torch.cat([ch[None, None] * rope.freqs_h.double()[:, :, None],
                      cw[None, None] * rope.freqs_w.double()[:, :, None]], 1)


@pytest.mark.parametrize("d", [32, 64])
def test_qk_prep_backward_against_float64(dev, d):
    """Heads below, above (d(scale) exactly 0) and exactly at the clamp ln 100 (torch's rule: the gradient passes)."""
    from lidarcrafter_amd import ops as K
    from lidargen.utils.lidar import get_linear_ray_angles

    heads, B, h, w = 4, 2, 8, 64
    C, L = heads * d, h * w
    coords = F.avg_pool2d(get_linear_ray_angles(h, 4 * w, 10.0, -30.0), (1, 4))[0]
    th = _rope_tables(coords, heads, d, (4, 32))
    cos_t, sin_t = th.cos().float().contiguous().to(dev), th.sin().float().contiguous().to(dev)
    qkv = seeded_randn(B, 3 * C, L, seed=950 + d).to(dev)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    ln100 = torch.tensor(math.log(100), dtype=torch.float32).item()
    scale = torch.tensor([[2.3], [5.2], [ln100], [0.7]], device=dev)
    gq = seeded_randn(B, C, L, seed=960 + d).to(dev)
    gk = seeded_randn(B, C, L, seed=970 + d).to(dev)
    dq, dk, ds = K.hdit_qk_prep_bwd(q, k, gq, gk, heads, scale, cos_t, sin_t)
    # torch's own rule for the float32 parameter
    s32 = scale.clone().requires_grad_()
    s32.clamp(max=math.log(100)).sum().backward()
    passes = s32.grad.double().reshape(1, heads, 1, 1)
    assert float(passes[0, 2]) == 1.0 and float(passes[0, 1]) == 0.0
    sd = scale.double().requires_grad_()
    eff = (passes.reshape(heads, 1) * sd + (1 - passes.reshape(heads, 1)) * sd.detach().clamp(max=math.log(100)))
    sc = eff.exp().sqrt().reshape(1, heads, 1, 1)
    c, s = th.cos().to(dev)[None], th.sin().to(dev)[None]
    xs = [src.double().requires_grad_() for src in (q, k)]
    loss = 0.0
    for x, g in zip(xs, (gq, gk)):
        v = x.reshape(B, heads, d, L)
        v = v / v.norm(dim=2, keepdim=True).clamp_min(1e-6) * sc
        x1, x2 = v[:, :, :d // 2], v[:, :, d // 2:]
        loss = loss + (torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], 2).reshape(B, C, L) * g.double()).sum()
    loss.backward()
    _close(dq, xs[0].grad, 2e-6)
    _close(dk, xs[1].grad, 2e-6)
    assert ds.shape == scale.shape
    assert float(ds[1]) == 0.0
    _close(ds, sd.grad, 1e-5)


def _na_f64(q, k, v, heads, h, w, kh, kw):
    B, C, L = q.shape
    d = C // heads
    r0 = (torch.arange(h) - kh // 2).clamp(0, h - kh)
    rows = r0[:, None] + torch.arange(kh)[None]
    cols = (torch.arange(w)[:, None] - kw // 2 + torch.arange(kw)[None]) % w
    key = (rows[:, None, :, None] * w + cols[None, :, None, :]).reshape(L, kh * kw).to(q.device)
    f = lambda t: t.reshape(B, heads, d, L)  # noqa: E731
    qd, kd, vd = f(q), f(k), f(v)
    kg, vg = kd[..., key], vd[..., key]
    s = torch.einsum("bhdl,bhdln->bhln", qd, kg)
    return torch.einsum("bhln,bhdln->bhdl", s.softmax(-1), vg).reshape(B, C, L)


def _na_case(dev, kh, kw, d, h, w):
    h = max(h, kh)
    heads, B = 3, 2
    C, L = heads * d, h * w
    qkv = seeded_randn(B, 3 * C + 4, L, seed=1800 + d + h * w + kh).to(dev)
    q, k, v = qkv[:, :C] * 3.0, qkv[:, C + 4:2 * C + 4], qkv[:, 2 * C + 4:]
    do = seeded_randn(B, C, L, seed=1900 + d + h * w + kh).to(dev)
    return q.contiguous(), k, v, do, heads, h, w


@pytest.mark.parametrize("kh,kw", [(3, 9), (5, 7)])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("h,w", [(3, 20), (5, 12), (8, 64), (6, 5)])
def test_neighbourhood_backward_against_float64(dev, kh, kw, d, h, w):
    """The forward test's grid matrix: h == kh (5 x 12 at kh = 5, 3 x 20 at kh = 3) and w < kw (6 x 5: keys twice)."""
    from lidarcrafter_amd import ops as K

    q, k, v, do, heads, h, w = _na_case(dev, kh, kw, d, h, w)
    o, lse = K.hdit_na_train(q, k, v, heads, h, w, (kh, kw))
    dq, dk, dv = K.hdit_na_bwd(q, k, v, o, do, lse, heads, h, w, (kh, kw))
    ts = [t.double().requires_grad_() for t in (q, k, v)]
    ref = _na_f64(*ts, heads, h, w, kh, kw)
    ref.backward(do.double())
    _close(o, ref.detach(), 1e-5)
    # the recomputed P carries the fp32 rounding of scores up to ~60, as the forward does (its bound: 1e-5)
    for got, t in zip((dq, dk, dv), ts):
        _close(got, t.grad, 5e-5)


def test_neighbourhood_train_forward_bit_identical_and_backward_deterministic(dev):
    from lidarcrafter_amd import ops as K

    for kh, kw, d, h, w in ((3, 9, 64, 32, 64), (5, 7, 32, 6, 5)):
        q, k, v, do, heads, h, w = _na_case(dev, kh, kw, d, h, w)
        o, lse = K.hdit_na_train(q, k, v, heads, h, w, (kh, kw))
        assert torch.equal(o, K.hdit_na(q, k, v, heads, h, w, (kh, kw)))
        a = K.hdit_na_bwd(q, k, v, o, do, lse, heads, h, w, (kh, kw))
        b = K.hdit_na_bwd(q, k, v, o, do, lse, heads, h, w, (kh, kw))
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_lerp_backward_against_float64(dev):
    from lidarcrafter_amd import ops as K

    B, C, H, W = 2, 6, 8, 20
    y = seeded_randn(B, 4 * C, H // 2, W // 2, seed=151).to(dev)
    skip = seeded_randn(B, C, H, W, seed=152).to(dev)
    alpha = torch.tensor([-3.0, -0.5, 0.0, 0.4, 1.5, 6.0], device=dev)
    dout = seeded_randn(B, C, H, W, seed=153).to(dev)
    dy, dskip, da = K.hdit_lerp_bwd(dout, y, skip, alpha, 2, 2)
    yd, sd, ad = (t.double().requires_grad_() for t in (y, skip, alpha))
    z = yd.reshape(B, 2, 2, C, H // 2, W // 2).permute(0, 3, 4, 1, 5, 2).reshape(B, C, H, W)
    torch.lerp(sd, z, torch.sigmoid(ad)[None, :, None, None]).backward(dout.double())
    _close(dy, yd.grad, 1e-6)
    _close(dskip, sd.grad, 1e-6)
    _close(da, ad.grad, 1e-6)


# ---- model ------------------------------------------------------------------------------------------------------
def _build(base, res, ray_angles, dev, clamped_heads=True):
    from lidargen.models.dits import HDiT
    from lidargen.utils.lidar import get_linear_ray_angles

    m = HDiT(res, 2, base_channels=base, **PARAMS)
    if ray_angles:
        m.coords = get_linear_ray_angles(res[0], res[1], 10.0, -30.0)
    seeded_fill(m, salt=SALT)
    seeded_fill_hdit(m, salt=SALT, clamped_heads=clamped_heads)
    return m.train().to(dev)


def _ddpm(m):
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion

    return ContinuousTimeGaussianDiffusion(m, torch.nn.Identity()).train().to(m.coords.device)


def _pinned_loss(ddpm, res, g, prefix, dev):
    x = seeded_randn(2, 2, *res, seed=int(g[f"{prefix}_x_seed"])).to(dev)
    noise = seeded_randn(2, 2, *res, seed=int(g[f"{prefix}_n_seed"])).to(dev)
    ddpm.randn_like = lambda x_, rng=None: noise
    try:
        return ddpm.p_loss(x, T(g["steps"]))
    finally:
        del ddpm.randn_like


def _role(name):
    """A parameter's role: its name without level / block indices (every down-level block's qkv_proj.weight is one)."""
    return re.sub(r"\d+", "#", name)


# Tolerances.  The well-conditioned model (no clamped heads) meets the issue's rule as it stands: each gradient norm within
# the larger of twice the reference's own float32 deviation for that parameter and 3e-4.  With logits up to 100 the
# float32 deviation is rounding noise of up to 2.5e-2 (the level-0 logit scales), and one parameter's single float32
# sample of it can fall far below what another evaluation order gives (the reference run on 8 and on 16 CPU threads
# differs by 2.48e-2 / 2.52e-2 on the same parameter).  For the clamped models the yardstick is therefore the largest own
# deviation over the parameter's role, with a floor of 1e-3.
def _check_grads(model, g, prefix, heads, by_role):
    """Each gradient against the reference's float64 one (see the tolerances above)."""
    grads = {k: p.grad for k, p in model.named_parameters()}
    names = [str(n) for n in g[f"{prefix}_names"]]
    assert set(names) == set(grads) and all(grads[n] is not None for n in names)
    n32, n64 = g[f"{prefix}_norms32"], g[f"{prefix}_norms64"]
    top = float(n64.max())
    own = np.abs(n32 - n64) / np.maximum(n64, 1e-30)
    scale = np.maximum(n64, 1e-3 * top)
    own_h = None
    if heads:
        h32, h64 = g[f"{prefix}_heads32"], g[f"{prefix}_heads64"]
        own_h = np.abs(h32 - h64).max(1) / scale
    if by_role:
        roles = [_role(k) for k in names]
        worst_own = {r: max(own[i] for i in range(len(names)) if roles[i] == r) for r in set(roles)}
        own = np.array([worst_own[r] for r in roles])
        if heads:
            worst_h = {r: max(own_h[i] for i in range(len(names)) if roles[i] == r) for r in set(roles)}
            own_h = np.array([worst_h[r] for r in roles])
    floor = 1e-3 if by_role else 3e-4
    worst = 0.0
    for i, k in enumerate(names):
        gr = grads[k].detach().double().cpu().flatten()
        n_ = float(n64[i])
        tol = max(2 * own[i], floor)
        err = abs(float(gr.norm()) - n_)
        assert err <= tol * n_ + 1e-6 * top, (k, float(gr.norm()), n_, tol)
        if n_ > 1e-4 * top:
            worst = max(worst, err / n_)
        if heads:
            m = min(8, gr.numel())
            atol = max(2 * own_h[i], floor) * scale[i]
            assert np.allclose(gr[:m].numpy(), g[f"{prefix}_heads64"][i][:m], rtol=0, atol=atol), k
    return worst


def test_train_mode_forward_matches_reference(dev, golden):
    g = golden("hdit")
    m = _build(64, (32, 256), False, dev)
    x = seeded_randn(2, 2, 32, 256, seed=601).to(dev)
    y = m(x, torch.tensor([-4.0, 2.5], device=dev))
    assert y.requires_grad and y.grad_fn is not None
    r = rel_l2(y.detach(), T(g["y_small64"]).float())
    assert r < 2 * float(g["ref_err_small"]), (r, float(g["ref_err_small"]))


def test_small_loss_and_gradients_without_clamped_heads(dev, golden):
    """Logit scales near ln 10: the float32 rounding stays small, and every gradient is held to the reference's
    float64 within the larger of twice the reference's own float32 deviation for that parameter and 3e-4."""
    g = golden("hdit_train")
    m = _build(64, (32, 256), False, dev, clamped_heads=False)
    loss = _pinned_loss(_ddpm(m), (32, 256), g, "u", dev)
    l64 = float(g["u_loss64"])
    assert abs(float(loss.detach()) - l64) <= 1e-5 * l64, (float(loss.detach()), l64)
    loss.backward()
    worst = _check_grads(m, g, "u", heads=True, by_role=False)
    print(f"worst gradient-norm deviation vs the reference's float64: {worst:.2e}")


def test_small_loss_and_gradients_against_reference(dev, golden):
    g = golden("hdit_train")
    m = _build(64, (32, 256), False, dev)
    loss = _pinned_loss(_ddpm(m), (32, 256), g, "s", dev)
    l64, l32 = float(g["s_loss64"]), float(g["s_loss32"])
    assert abs(float(loss.detach()) - l64) <= max(1e-5, 2 * abs(l32 - l64) / l64) * l64, (float(loss.detach()), l64)
    loss.backward()
    worst = _check_grads(m, g, "s", heads=True, by_role=True)
    print(f"worst gradient-norm deviation vs the reference's float64: {worst:.2e}")
    # the clamped heads (scale 5.0 > ln 100) get exactly zero gradient
    n_clamped = 0
    for k, p in m.named_parameters():
        if k.endswith("residual_attn.scale"):
            for i in range(p.shape[0]):
                if float(p[i]) > math.log(100):
                    assert float(p.grad[i]) == 0.0, k
                    n_clamped += 1
    assert n_clamped > 0


def test_full_loss_and_gradient_norms_against_reference(dev, golden):
    g = golden("hdit_train")
    m = _build(128, (32, 1024), True, dev)
    loss = _pinned_loss(_ddpm(m), (32, 1024), g, "f", dev)
    l64, l32 = float(g["f_loss64"]), float(g["f_loss32"])
    assert abs(float(loss.detach()) - l64) <= max(1e-5, 2 * abs(l32 - l64) / l64) * l64, (float(loss.detach()), l64)
    loss.backward()
    _check_grads(m, g, "f", heads=False, by_role=True)


def _gens(seeds):
    return [torch.Generator().manual_seed(s) for s in seeds]


def test_adamw_step_caches_and_deepcopy(dev):
    """ddpm(x0).backward() in train mode reaches every parameter with finite values; an AdamW step moves the loss; then
    sampling (replayed graph) equals an eager sample with the updated weights bit for bit, and so does a deepcopy."""
    m = _build(64, (32, 256), False, dev)
    ddpm = _ddpm(m)
    ddpm.eval()
    before = ddpm.sample(2, 3, progress=False, rng=_gens([3, 4]), mode="ddim")        # captures the step graph
    ddpm.train()
    x0 = seeded_randn(2, 2, 32, 256, seed=2001).clamp(-1, 1).to(dev)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    torch.manual_seed(11)
    loss0 = ddpm(x0)
    loss0.backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    opt.step()
    opt.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    loss1 = ddpm(x0)
    assert bool(torch.isfinite(loss1)) and float(loss1) != float(loss0), (float(loss0), float(loss1))
    loss1.backward()
    opt.step()
    ddpm.eval()
    a = ddpm.sample(2, 3, progress=False, rng=_gens([3, 4]), mode="ddim")
    b = ddpm.sample(2, 3, progress=False, rng=_gens([3, 4]), mode="ddim")
    ddpm.use_hip_graph = False
    c = ddpm.sample(2, 3, progress=False, rng=_gens([3, 4]), mode="ddim")
    ddpm.use_hip_graph = True
    assert not torch.equal(a, before)
    assert torch.equal(a, c) and torch.equal(b, c)
    twin = copy.deepcopy(ddpm)
    d = twin.sample(2, 3, progress=False, rng=_gens([3, 4]), mode="ddim")
    assert torch.equal(d, c)


def test_ddp_wraps_the_training_graph(dev):
    """A single-rank DistributedDataParallel around the train-mode ddpm: the same draws give the unwrapped gradients."""
    import os
    import socket

    import torch.distributed as dist

    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ddpm = _ddpm(_build(64, (32, 256), False, dev))
        x0 = seeded_randn(2, 2, 32, 256, seed=2101).to(dev)
        torch.manual_seed(7)
        ddpm(x0).backward()
        ref = {k: p.grad.clone() for k, p in ddpm.named_parameters() if p.grad is not None}
        ddpm.zero_grad(set_to_none=True)
        wrapped = torch.nn.parallel.DistributedDataParallel(ddpm, device_ids=[0], bucket_cap_mb=1)
        torch.manual_seed(7)
        wrapped(x0).backward()
        got = {k: p.grad for k, p in ddpm.named_parameters() if p.grad is not None}
        assert got.keys() == ref.keys() and len(ref) > 100
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
    finally:
        dist.destroy_process_group()
