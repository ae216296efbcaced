"""MeanFlow training on the MI355X: the tangent kernels (csrc/flow_jvp.hip) against float64 torch.func.jvp / autograd of
the reference formulas, and MeanFlow.loss / its gradients against the reference's own loss on the CPU
(tests/golden/meanflow_train.npz, make_meanflow_train_fixtures.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lidarcrafter_amd.testing import rel_l2, seeded_fill, seeded_fill_qk_gains, seeded_randn

pytestmark = pytest.mark.gpu

SALT = 100


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def T(a, dev="cuda"):
    return torch.as_tensor(np.asarray(a)).to(dev)


def _model(base, res, dev):
    from lidargen.models.unets.efficient_mf_unet import MFEfficientUNet
    from lidargen.utils.lidar import get_linear_ray_angles

    m = MFEfficientUNet(2, res, base_channels=base, coords_encoding="fourier_features", num_residual_blocks=(3, 3, 3, 3),
                        gn_num_groups=8, gn_eps=1e-6, attn_num_heads=8, ring=True)
    m.coords = get_linear_ray_angles(res[0], res[1], 10.0, -30.0)
    seeded_fill(m, salt=SALT)
    seeded_fill_qk_gains(m, salt=SALT)
    return m.to(dev)


def _flow(m):
    from lidargen.models.flows import MeanFlow

    return MeanFlow(m, channels=2, image_size=tuple(m.resolution), time_dist=["lognorm", -0.4, 1], flow_ratio=0.5)


def _rel_max(got, ref):
    return float((got.double().cpu() - ref.cpu()).abs().max() / ref.abs().max().clamp_min(1e-30))


# ---- kernels ------------------------------------------------------------------------------------------------------------
def _qk_ref(x, g, heads):
    B, C, L = x.shape
    d = C // heads
    xh = x.reshape(B, heads, d, L)
    return (F.normalize(xh, dim=2) * d ** 0.5 * g).reshape(B, C, L)


@pytest.mark.parametrize("d,L", [(32, 7), (64, 130), (32, 512), (64, 512)])
def test_qk_norm_jvp_and_backward_against_float64(dev, d, L):
    from lidarcrafter_amd import autograd as AG

    heads, B = 4, 3
    C = heads * d
    qkv = seeded_randn(B, 3 * C, L, seed=800 + d + L)
    x = qkv[:, C:2 * C]                                  # a strided slice, as in the attention
    dx = seeded_randn(B, C, L, seed=801 + d + L)
    gy = seeded_randn(B, C, L, seed=802 + d + L)
    g = torch.tensor([-1.75])
    x64, g64 = x.double(), g.double()
    y_ref, dy_ref = torch.func.jvp(lambda a: _qk_ref(a, g64, heads), (x64,), (dx.double(),))
    xr, gr = x64.clone().requires_grad_(True), g64.clone().requires_grad_(True)
    _qk_ref(xr, gr, heads).backward(gy.double())
    qkv_d, g_d = qkv.to(dev), g.to(dev).requires_grad_(True)
    x_d = qkv_d[:, C:2 * C].clone().requires_grad_(True)
    y, dy = AG.QKNormJvp.apply(x_d, g_d, heads, dx.to(dev))
    assert not dy.requires_grad
    assert _rel_max(y.detach(), y_ref) <= 1e-6 and _rel_max(dy, dy_ref) <= 1e-6
    y.backward(gy.to(dev))
    assert _rel_max(x_d.grad, xr.grad) <= 1e-6
    assert abs(float(g_d.grad) - float(gr.grad)) <= 1e-6 * abs(float(gr.grad))
    # the out-of-place primal is bit-identical to the in-place inference kernel
    from lidarcrafter_amd import ops as K

    inplace = qkv_d[:, C:2 * C].clone()
    K.qk_norm_cm(inplace, inplace.clone(), heads, g.to(dev), g.to(dev))
    assert torch.equal(AG.QKNorm.apply(qkv_d[:, C:2 * C], g.to(dev), heads), inplace)


def _gn_ref(x, G, eps, gamma, beta, sc, sh, act):
    y = F.group_norm(x, G, None, None, eps)
    if gamma is not None:
        y = y * gamma[None, :, None, None] + beta[None, :, None, None]
    if sc is not None:
        y = y * (1 + sc[:, :, None, None]) + sh[:, :, None, None]
    return F.silu(y) if act else y


@pytest.mark.parametrize("shape,affine,ada,act", [((2, 64, 32, 1024), False, True, True),
                                                  ((8, 128, 16, 512), True, True, True),
                                                  ((4, 512, 4, 128), True, False, False),
                                                  ((3, 48, 5, 37), False, False, True),
                                                  ((2, 256, 8, 256), True, True, False)])
def test_groupnorm_jvp_against_float64(dev, shape, affine, ada, act):
    from lidarcrafter_amd import autograd as AG

    B, C, H, W = shape
    G, eps = 8, 1e-6
    x = seeded_randn(*shape, seed=901) * 3 + 0.5
    dx = seeded_randn(*shape, seed=902)
    gamma = seeded_randn(C, seed=903) if affine else None
    beta = seeded_randn(C, seed=904) if affine else None
    sc = seeded_randn(B, C, seed=905) * 0.3 if ada else None
    sh = seeded_randn(B, C, seed=906) if ada else None
    dsc = seeded_randn(B, C, seed=907) * 0.3 if ada else None
    dsh = seeded_randn(B, C, seed=908) if ada else None
    d64 = lambda t: None if t is None else t.double()
    prim = (x.double(),) + ((d64(sc), d64(sh)) if ada else ())
    tang = (dx.double(),) + ((d64(dsc), d64(dsh)) if ada else ())

    def f(x_, *ss):
        return _gn_ref(x_, G, eps, d64(gamma), d64(beta), ss[0] if ada else None, ss[1] if ada else None, act)

    y_ref, dy_ref = torch.func.jvp(f, prim, tang)
    cu = lambda t: None if t is None else t.to(dev)
    xg = x.to(dev).requires_grad_(True)
    y, dy = AG.GroupNormActJvp.apply(xg, cu(gamma), cu(beta), cu(sc), cu(sh), G, eps, act, cu(dx), cu(dsc), cu(dsh))
    assert rel_l2(y, y_ref) <= 1e-6 and rel_l2(dy, dy_ref) <= 1e-6, (rel_l2(y, y_ref), rel_l2(dy, dy_ref))
    # primal y and the saved (mean, rstd) are GroupNormAct's
    y0 = AG.GroupNormAct.apply(xg, cu(gamma), cu(beta), cu(sc), cu(sh), G, eps, act)
    assert rel_l2(y, y0) <= 1e-7
    assert torch.equal(y.grad_fn.saved_tensors[1], y0.grad_fn.saved_tensors[1])


def _attn_ref(q, k, v, scale):
    s = torch.einsum("bhct,bhcs->bhts", q, k) * scale
    return torch.einsum("bhts,bhcs->bhct", s.softmax(-1), v)


@pytest.mark.parametrize("d,Lq,Lk", [(64, 512, 512), (32, 200, 77), (64, 33, 300), (48, 130, 64)])
@pytest.mark.parametrize("mag", [1.0, 1e-3, 30.0])
def test_attention_jvp_against_float64(dev, d, Lq, Lk, mag):
    from lidarcrafter_amd import autograd as AG

    B, h = 2, 3
    q = seeded_randn(B, h, d, Lq, seed=1001) * mag
    k = seeded_randn(B, h, d, Lk, seed=1002) * mag
    v = seeded_randn(B, h, d, Lk, seed=1003) * mag
    dq, dk, dv = (seeded_randn(*t.shape, seed=1004 + i) * mag for i, t in enumerate((q, k, v)))
    scale = d ** -0.5 / max(mag, 1.0) ** 2             # keep the softmax away from one-hot at large magnitudes
    o_ref, do_ref = torch.func.jvp(lambda a, b, c: _attn_ref(a, b, c, scale), (q.double(), k.double(), v.double()),
                                   (dq.double(), dk.double(), dv.double()))
    o, lse, do = AG.attention_jvp_launch(*(t.to(dev).contiguous() for t in (q, k, v, dq, dk, dv)), scale)
    # bound 2e-6; 5e-6 at the small magnitude, where the softmax is near uniform over zero-mean values and o cancels to
    # ~3 % of |v| (the error is ~1e-7 of |v| there: one rounding of a 512-term sum)
    tol = 2e-6 if mag >= 1.0 else 5e-6
    assert rel_l2(o, o_ref) <= tol and rel_l2(do, do_ref) <= tol, (rel_l2(o, o_ref), rel_l2(do, do_ref))
    s = torch.einsum("bhct,bhcs->bhts", q.double(), k.double()) * scale
    lse_ref = torch.logsumexp(s, -1) / np.log(2.0)                       # base 2, as lc_attention_train_fwd's
    assert float((lse.cpu().double() - lse_ref.reshape(B * h, Lq)).abs().max()) <= 1e-5 * max(1.0, float(lse_ref.abs().max()))


def test_attention_jvp_backward_matches_flash_attention(dev):
    """The paired Function's backward (lc_attention_bwd* on the saved o, lse) gives FlashAttention's gradients."""
    from lidarcrafter_amd import autograd as AG

    q, k, v = (seeded_randn(2, 8, 64, 512, seed=1100 + i).to(dev) for i in range(3))
    go = seeded_randn(2, 8, 64, 512, seed=1104).to(dev)
    z = torch.zeros_like(q)
    a = [t.clone().requires_grad_(True) for t in (q, k, v)]
    b = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o1, _ = AG.FlashAttentionJvp.apply(*a, z, z, z, 0.125)
    o2 = AG.FlashAttention.apply(*b, 0.125)
    assert rel_l2(o1, o2) <= 2e-5
    o1.backward(go)
    o2.backward(go)
    for x1, x2 in zip(a, b):
        assert rel_l2(x1.grad, x2.grad) <= 2e-5


# ---- whole network --------------------------------------------------------------------------------------------------------
def _digest_check(named_params, names, norms, heads, tol):
    grads = {k: p.grad for k, p in named_params if p.grad is not None}
    assert set(grads) == {str(k) for k in names}
    top = float(norms.max())
    worst = 0.0
    for i, (k, n_) in enumerate(zip(names, norms)):
        gr = grads[str(k)].detach().double().cpu().flatten()
        err = abs(float(gr.norm()) - n_)
        assert err <= tol * n_ + 1e-6 * top, (k, float(gr.norm()), n_)
        if heads is not None:
            m = min(8, gr.numel())
            assert np.allclose(gr[:m].numpy(), heads[i][:m], rtol=0, atol=tol * max(n_, 1e-3 * top)), k
        if n_ > 1e-4 * top:
            worst = max(worst, err / n_)
    return worst


def test_loss_small_against_reference(dev, golden):
    g = golden("meanflow_train")
    m = _model(16, (8, 64), dev)
    flow = _flow(m)
    loss, mse, u, dudt = flow.loss_terms(T(g["s_x"]), T(g["s_t"]), T(g["s_r"]), T(g["s_e"]))
    assert rel_l2(u, T(g["s_u"], "cpu")) <= 2e-5, rel_l2(u, T(g["s_u"], "cpu"))
    assert rel_l2(dudt, T(g["s_dudt"], "cpu")) <= 5e-5, rel_l2(dudt, T(g["s_dudt"], "cpu"))
    assert abs(float(loss) - float(g["s_loss"])) <= 1e-5 * float(g["s_loss"])
    assert abs(float(mse) - float(g["s_mse"])) <= 1e-5 * float(g["s_mse"])
    assert u.requires_grad and not dudt.requires_grad
    loss.backward()
    worst = _digest_check(m.named_parameters(), g["s_names"], g["s_norms"], g["s_heads"], 3e-4)
    print(f"worst gradient-norm deviation vs the reference: {worst:.2e}")
    for name in ("end_time_embedding.1.weight", "d_block4.self_attn_block.attn.q_norm.g",
                 "u_block4.self_attn_block.attn.k_norm.g"):
        p = dict(m.named_parameters())[name]
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_loss_full_against_reference(dev, golden):
    g = golden("meanflow_train")
    m = _model(64, (32, 1024), dev)
    flow = _flow(m)
    x = seeded_randn(2, 2, 32, 1024, seed=int(g["f_x_seed"]))
    torch.manual_seed(int(g["f_e_seed"]))
    e = torch.randn_like(x)
    loss, mse, u, dudt = flow.loss_terms(x.to(dev), T(g["f_t"]), T(g["f_r"]), e.to(dev))
    for prefix, a, tol in (("f_u", u, 2e-5), ("f_dudt", dudt, 5e-5)):
        st = 8
        r = (rel_l2(a[..., ::st], T(g[f"{prefix}_cols"], "cpu")), rel_l2(a.norm(dim=-1), T(g[f"{prefix}_rownorm"], "cpu")),
             rel_l2(a.flatten(1).norm(dim=1), T(g[f"{prefix}_norm"], "cpu")))
        assert max(r) <= tol, (prefix, r)
    assert abs(float(loss) - float(g["f_loss"])) <= 1e-5 * float(g["f_loss"])
    loss.backward()
    _digest_check(m.named_parameters(), g["f_names"], g["f_norms"], None, 3e-4)


def test_seeded_loss_draws_as_the_reference(dev, golden):
    g = golden("meanflow_train")
    m = _model(16, (8, 64), dev)
    flow = _flow(m)
    x = seeded_randn(4, 2, 8, 64, seed=int(g["e2e_x_seed"])).to(dev)
    np.random.seed(int(g["e2e_np_seed"]))
    t, r = flow.sample_t_r(4, "cpu")
    assert torch.equal(t, T(g["e2e_t"], "cpu")) and torch.equal(r, T(g["e2e_r"], "cpu"))
    np.random.seed(int(g["e2e_np_seed"]))
    torch.manual_seed(int(g["e2e_torch_seed"]))
    loss, mse = flow({"x_0": x})
    assert abs(float(loss) - float(g["e2e_loss"])) <= 1e-5 * float(g["e2e_loss"])
    assert abs(float(mse) - float(g["e2e_mse"])) <= 1e-5 * float(g["e2e_mse"])


def test_dudt_against_finite_differences(dev):
    """An independent check of signs and factors: dudt against central differences of the INFERENCE forward along
    (v, 1, 0), the rows with t away from 1."""
    m = _model(16, (8, 64), dev)
    z = seeded_randn(2, 2, 8, 64, seed=1201).to(dev)
    v = seeded_randn(2, 2, 8, 64, seed=1202).to(dev)
    t, r = torch.tensor([0.6, 0.4], device=dev), torch.tensor([0.1, 0.4], device=dev)
    _, dudt = m.forward_jvp(z, t, r, v, torch.ones_like(t), torch.zeros_like(r))
    eps = 1e-2
    with torch.no_grad():
        up = m(z + eps * v, t + eps, r).double()
        dn = m(z - eps * v, t - eps, r).double()
    fd = (up - dn) / (2 * eps)
    assert rel_l2(dudt, fd) <= 1e-2, rel_l2(dudt, fd)


def test_grad_mode_forward_matches_inference(dev):
    m = _model(16, (8, 64), dev)
    z = seeded_randn(2, 2, 8, 64, seed=1301).to(dev)
    t, r = torch.tensor([0.9, 0.5], device=dev), torch.tensor([0.2, 0.5], device=dev)
    u = m(z, t, r)
    assert u.requires_grad
    with torch.no_grad():
        ref = m(z, t, r)
    assert rel_l2(u, ref) <= 2e-5
    u2, _ = m.forward_jvp(z, t, r, torch.zeros_like(z), torch.ones_like(t), torch.zeros_like(r))
    assert rel_l2(u2, ref) <= 2e-5


def test_adamw_steps_lower_the_loss(dev):
    m = _model(16, (8, 64), dev).train()
    flow = _flow(m)
    x = seeded_randn(4, 2, 8, 64, seed=1401).to(dev)
    t, r = torch.tensor([0.9, 0.7, 0.5, 1.0]), torch.tensor([0.2, 0.3, 0.5, 0.0])
    e = seeded_randn(4, 2, 8, 64, seed=1402).to(dev)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = flow.loss_terms(x, t, r, e)[0]
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses


def test_ddp_wraps_the_flow(dev):
    """A single-rank DistributedDataParallel around `flow`: the same draws give the unwrapped module's gradients."""
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
        flow = _flow(_model(16, (8, 64), dev).train())
        x0 = seeded_randn(4, 2, 8, 64, seed=1501).to(dev)
        np.random.seed(3)
        torch.manual_seed(7)
        flow({"x_0": x0})[0].backward()
        ref = {k: p.grad.clone() for k, p in flow.named_parameters() if p.grad is not None}
        flow.zero_grad(set_to_none=True)
        wrapped = torch.nn.parallel.DistributedDataParallel(flow, device_ids=[0], bucket_cap_mb=1)
        np.random.seed(3)
        torch.manual_seed(7)
        wrapped({"x_0": x0})[0].backward()
        got = {k: p.grad for k, p in flow.named_parameters() if p.grad is not None}
        assert got.keys() == ref.keys() and len(ref) > 100
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
    finally:
        dist.destroy_process_group()
