"""Golden vectors of the MeanFlow generator (reference lidargen/models/unets/efficient_mf_unet.py and
lidargen/models/flows/mean_flow.py), run on the CPU from the read-only reference tree.

Run in the build container only:   python tests/golden/make_meanflow_fixtures.py
Output: tests/golden/meanflow.npz (committed).  Weights come from lidarcrafter_amd.testing.seeded_fill followed by
seeded_fill_qk_gains, inputs from seeded_randn / torch generators, so the file holds outputs and key lists only.

timm is not a dependency of this project.  The reference model takes one class from it,
`timm.models.vision_transformer.Attention`, which is restated below from timm 0.9.12 (the version the reference's
environment pins) and registered in sys.modules before the reference module is imported.  The attention internals of
these fixtures are therefore pinned only as far as that restatement goes: qkv Linear -> (3, heads, head_dim) split ->
q_norm / k_norm -> q * head_dim^-0.5 -> softmax(q k^T) v -> proj (the `fused_attn = False` branch; dropout p = 0).
"""
import os
import sys
import types
import warnings

import numpy as np
import torch
from torch import nn

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import as R  # noqa: E402

R.install()
from lidarcrafter_amd.testing import seeded_fill, seeded_fill_qk_gains, seeded_randn  # noqa: E402

torch.set_num_threads(int(os.environ.get("LC_FIXTURE_THREADS", "8")))
torch.manual_seed(0)


class Attention(nn.Module):
    """timm 0.9.12 timm/models/vision_transformer.py Attention (third-party semantics, restated)."""

    fused_attn = False

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_norm=False, attn_drop=0., proj_drop=0.,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        q, k = self.q_norm(q), self.k_norm(k)
        if self.fused_attn:
            x = torch.nn.functional.scaled_dot_product_attention(q, k, v, dropout_p=0.)
        else:
            q = q * self.scale
            attn = q @ k.transpose(-2, -1)
            attn = attn.softmax(dim=-1)
            attn = self.attn_drop(attn)
            x = attn @ v
        x = x.transpose(1, 2).reshape(B, N, C)
        x = self.proj(x)
        x = self.proj_drop(x)
        return x


def _install_timm():
    for name in ("timm", "timm.models", "timm.models.vision_transformer"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["timm.models.vision_transformer"].Attention = Attention
    flows = types.ModuleType("lidargen.models.flows")
    flows.__path__ = [R.REF + "/lidargen/models/flows"]
    flows.__package__ = "lidargen.models.flows"
    sys.modules["lidargen.models.flows"] = flows


_install_timm()
MF = R.ref("models.unets.efficient_mf_unet")
MEAN_FLOW = R.ref("models.flows.mean_flow")
LIDAR = R.ref("utils.lidar")

# the config's model params (option_meanflow_nusc.py:8-21) at base 64; the small model at base 16
PARAMS = dict(temb_channels=None, channel_multiplier=(1, 2, 4, 8), num_residual_blocks=(3, 3, 3, 3), gn_num_groups=8,
              gn_eps=1e-6, attn_num_heads=8, coords_encoding="fourier_features", ring=True)
SALT = 100
T_SMALL, R_SMALL = [0.9, 0.6], [0.2, 0.6]            # one r < t, one r = t
TR_FULL = [([1.0, 0.35], [0.0, 0.35]), ([0.75, 0.5], [0.25, 0.0])]
REF_SEED = 7
COL_STEP_FULL, COL_STEP_B8 = 8, 16         # stored columns of the 32 x 1024 outputs (file size: about 0.5 MB in all)


def build(base, res):
    m = MF.MFEfficientUNet(2, res, base_channels=base, **PARAMS)
    m.coords = LIDAR.get_linear_ray_angles(res[0], res[1], 10.0, -30.0)     # inference.py:409-410
    seeded_fill(m, salt=SALT)
    seeded_fill_qk_gains(m, salt=SALT)
    return m.eval()


def keys_of(module):
    return np.array(sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items()))


def summary(prefix, x, step):
    """A full-size output in a few hundred KB: every `step`-th column, the L2 norm of every row over ALL its columns (a
    mistake in a column that is not stored still shows) and the per-sample norms."""
    return {f"{prefix}_cols": x[..., ::step].contiguous(), f"{prefix}_rownorm": x.norm(dim=-1),
            f"{prefix}_norm": x.flatten(1).norm(dim=1)}


def flow_sample(m, z, num_steps):
    """The build's multi-step update on the reference model: t_i = 1 - i / S, z <- z - (t_i - t_{i+1}) u(z, t_i, t_{i+1})
    (float32 time grid, as MeanFlow.time_grid; S = 1 is the reference's `z - model(z, 1, 0)`)."""
    tg = (1.0 - torch.arange(num_steps + 1, dtype=torch.float64) / num_steps).float()
    B = z.shape[0]
    for i in range(num_steps):
        u = m(z, tg[i].repeat(B), tg[i + 1].repeat(B))
        z = z - (tg[i] - tg[i + 1]) * u
    return z


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: a rerun writes the same bytes."""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    out = {}
    with torch.no_grad():
        # small: base 16, 8 x 64, B = 2
        ms = build(16, (8, 64))
        x = seeded_randn(2, 2, 8, 64, seed=501)
        y_small = ms(x, torch.tensor(T_SMALL), torch.tensor(R_SMALL))
        out["y_small"] = y_small
        # the gains are not degenerate: zeroing them must change the output visibly
        saved = {k: v.clone() for k, v in ms.state_dict().items() if k.endswith(".g")}
        for name, p in ms.named_parameters():
            if name.endswith(".g"):
                p.zero_()
        y0 = ms(x, torch.tensor(T_SMALL), torch.tensor(R_SMALL))
        ms.load_state_dict(saved, strict=False)
        change = float((y0 - y_small).norm() / y_small.norm())
        assert change > 0.05, f"zeroing the q / k gains changes y_small by only {change:.4f}"
        out["gain_sensitivity"] = np.float64(change)

        # full size: the config's params, 32 x 1024, B = 2, two (t, r) pairs
        m = build(64, (32, 1024))
        out["keys_model"] = keys_of(m)
        assert sum(p.numel() for p in m.parameters()) == 31_180_934
        x = seeded_randn(2, 2, 32, 1024, seed=502)
        for j, (t, r) in enumerate(TR_FULL):
            out.update(summary(f"y_full{j}", m(x, torch.tensor(t), torch.tensor(r)), COL_STEP_FULL))

        flow = MEAN_FLOW.MeanFlow(m, channels=2, image_size=(32, 1024), normalizer=["minmax", None, None],
                                  time_dist=["lognorm", -0.4, 1], flow_ratio=0.5, cfg_ratio=0.1, cfg_scale=None,
                                  jvp_api="autograd")
        out["keys_flow"] = keys_of(flow)
        # the reference's own sampler: torch.manual_seed(s); flow.sample(device="cpu")
        torch.manual_seed(REF_SEED)
        out.update(summary("ref_sample", flow.sample(device="cpu"), COL_STEP_FULL))
        out["ref_seed"] = np.int64(REF_SEED)

        # batch 8: one- and two-step samples from per-sample generators
        z = torch.stack([torch.randn(2, 32, 1024, generator=torch.Generator().manual_seed(i)) for i in range(8)])
        for S in (1, 2):
            out.update(summary(f"b8_s{S}", flow_sample(m, z, S), COL_STEP_B8))

    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "meanflow.npz")
    save_npz(path, arrays)
    assert os.path.getsize(path) < 600 * 1024, "meanflow.npz grew: store fewer columns"
    print(f"meanflow.npz  {os.path.getsize(path) / 1024:.1f} KiB  gain sensitivity {change:.3f}  keys={list(arrays)}")


if __name__ == "__main__":
    main()
