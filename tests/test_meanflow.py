"""MeanFlow generator on the MI355X: the q / k normalisation and flow-step kernels against float64 restatements, the
model and the sampler against the reference's outputs (tests/golden/meanflow.npz, make_meanflow_fixtures.py)."""
import pytest
import torch

from lidarcrafter_amd.testing import rel_l2, seeded_fill, seeded_fill_qk_gains, seeded_randn

pytestmark = pytest.mark.gpu

SALT = 100


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def T(a, dev="cuda"):
    return torch.as_tensor(a).to(dev)


def _match(g, prefix, x, step, tol=2e-5):
    """x against the fixture's summary of the reference's output: every `step`-th column, the L2 norm of every row over
    all its columns, and the per-sample norms (tests/golden/make_meanflow_fixtures.py summary)."""
    r_cols = rel_l2(x[..., ::step], T(g[f"{prefix}_cols"]))
    r_rows = rel_l2(x.norm(dim=-1), T(g[f"{prefix}_rownorm"]))
    r_norm = rel_l2(x.flatten(1).norm(dim=1), T(g[f"{prefix}_norm"]))
    assert r_cols < tol and r_rows < tol and r_norm < tol, (prefix, r_cols, r_rows, r_norm)


def _qk_norm_f64(v, heads, g):
    """F.normalize(v, dim=head channels) * sqrt(d) * g in float64; v [B, heads*d, L]."""
    B, C, L = v.shape
    d = C // heads
    x = v.double().reshape(B, heads, d, L)
    n = x.norm(dim=2, keepdim=True).clamp_min(1e-12)
    return (x / n * d ** 0.5 * float(g)).reshape(B, C, L)


@pytest.mark.parametrize("d,L", [(32, 7), (64, 130), (32, 512), (64, 512)])
def test_qk_norm_cm_against_float64(dev, d, L):
    from lidarcrafter_amd import ops as K

    heads, B = 4, 3
    C = heads * d
    qkv = seeded_randn(B, 3 * C + 5, L, seed=700 + d + L).to(dev)        # channel pitch != 3C: strided slices
    q, k = qkv[:, :C], qkv[:, C + 5:2 * C + 5]
    k[1, 2 * d:3 * d, 3] = 0.0                                             # an all-zero k token (head 2): eps path -> 0
    gq, gk = torch.tensor([1.75], device=dev), torch.tensor([-2.25], device=dev)
    q0, k0 = q.clone(), k.clone()
    gap, rest = qkv[:, C:C + 5].clone(), qkv[:, 2 * C + 5:].clone()
    K.qk_norm_cm(q, k, heads, gq, gk)
    for got, src, g in ((q, q0, 1.75), (k, k0, -2.25)):
        ref = _qk_norm_f64(src, heads, g)
        err = (got.double() - ref).abs() / ref.abs().clamp_min(1e-30)
        err[ref == 0] = got.double()[ref == 0].abs()
        assert float(err.max()) <= 1e-6, float(err.max())
    assert float(k[1, 2 * d:3 * d, 3].abs().max()) == 0.0
    assert torch.equal(qkv[:, C:C + 5], gap) and torch.equal(qkv[:, 2 * C + 5:], rest)   # gap and v untouched
    # deterministic: a second call on the same input gives the same bits
    q2, k2 = q0.clone(), k0.clone()
    K.qk_norm_cm(q2, k2, heads, gq, gk)
    assert torch.equal(q2, q) and torch.equal(k2, k)


def test_flow_step(dev):
    from lidarcrafter_amd import ops as K

    z = seeded_randn(3, 2, 8, 96, seed=710).to(dev)
    u = seeded_randn(3, 2, 8, 96, seed=711).to(dev)
    dt = torch.tensor([1.0, 0.5, 0.3], device=dev)
    ref = z - dt[:, None, None, None] * u
    assert torch.equal(K.flow_step(z, u, dt), ref)
    zz = z.clone()
    assert K.flow_step(zz, u, dt, out=zz).data_ptr() == zz.data_ptr()
    assert torch.equal(zz, ref)


def _model(base, res, dev):
    from lidargen.models.unets.efficient_mf_unet import MFEfficientUNet
    from lidargen.utils.lidar import get_linear_ray_angles

    m = MFEfficientUNet(2, res, base_channels=base, coords_encoding="fourier_features", num_residual_blocks=(3, 3, 3, 3),
                        gn_num_groups=8, gn_eps=1e-6, attn_num_heads=8, ring=True)
    m.coords = get_linear_ray_angles(res[0], res[1], 10.0, -30.0)
    seeded_fill(m, salt=SALT)
    seeded_fill_qk_gains(m, salt=SALT)
    return m.eval().to(dev)


def _flow(dev):
    from lidargen.models.flows import MeanFlow

    return MeanFlow(_model(64, (32, 1024), dev), channels=2, image_size=(32, 1024))


def test_model_small_golden(dev, golden, gn_stats_route):
    g = golden("meanflow")
    m = _model(16, (8, 64), dev)
    x = seeded_randn(2, 2, 8, 64, seed=501).to(dev)
    with torch.no_grad():
        y = m(x, torch.tensor([0.9, 0.6], device=dev), torch.tensor([0.2, 0.6], device=dev))
    r = rel_l2(y, T(g["y_small"]))
    assert r < 2e-5, r


def test_model_full_golden(dev, golden, gn_stats_route):
    g = golden("meanflow")
    m = _model(64, (32, 1024), dev)
    x = seeded_randn(2, 2, 32, 1024, seed=502).to(dev)
    with torch.no_grad():
        y0 = m(x, torch.tensor([1.0, 0.35], device=dev), torch.tensor([0.0, 0.35], device=dev))
        y1 = m(x, torch.tensor([0.75, 0.5], device=dev), torch.tensor([0.25, 0.0], device=dev))
    _match(g, "y_full0", y0, 8)
    _match(g, "y_full1", y1, 8)


def test_reference_sample_formula(dev, golden):
    """`torch.manual_seed(s); flow.sample()` == the reference's `torch.manual_seed(s); flow.sample(device="cpu")`."""
    g = golden("meanflow")
    flow = _flow(dev)
    torch.manual_seed(int(g["ref_seed"]))
    z = flow.sample()
    assert z.shape == (1, 2, 32, 1024) and z.is_cuda
    _match(g, "ref_sample", z, 8)


@pytest.mark.parametrize("steps", [1, 2])
def test_batch8_samples(dev, golden, steps):
    g = golden("meanflow")
    flow = _flow(dev)
    rng = [torch.Generator().manual_seed(i) for i in range(8)]
    z = flow.sample(batch_size=8, num_steps=steps, rng=rng)
    _match(g, f"b8_s{steps}", z, 16)
    if steps == 2:
        zs = flow.sample(batch_size=8, num_steps=2, rng=[torch.Generator().manual_seed(i) for i in range(8)],
                         return_all=True)
        assert zs.shape == (3, 8, 2, 32, 1024) and torch.equal(zs[-1], z)


def test_sample_i_depends_on_generator_i_only(dev):
    flow = _flow(dev)
    zb = flow.sample(batch_size=8, rng=[torch.Generator().manual_seed(i) for i in range(8)])
    for i in (0, 5):
        z1 = flow.sample(batch_size=1, rng=[torch.Generator().manual_seed(i)])
        r = rel_l2(zb[i:i + 1], z1)
        assert r < 1e-5, (i, r)


def test_precomputed_time_features_bit_equal(dev):
    m = _model(16, (8, 64), dev)
    x = seeded_randn(2, 2, 8, 64, seed=503).to(dev)
    t, r = torch.tensor([0.8, 0.3], device=dev), torch.tensor([0.1, 0.3], device=dev)
    with torch.no_grad():
        y = m(x, t, r)
        y2 = m(x, t, r, time_features=m.time_features(t, r))
        y0d = m(x, torch.tensor(0.8, device=dev), torch.tensor(0.1, device=dev))
        y0r = m(x, torch.tensor([0.8, 0.8], device=dev), torch.tensor([0.1, 0.1], device=dev))
    assert torch.equal(y, y2)
    assert torch.equal(y0d, y0r)                                          # 0-d times broadcast over the batch
