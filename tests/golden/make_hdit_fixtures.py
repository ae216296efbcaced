"""Golden vectors of the Hourglass Diffusion Transformer (reference lidargen/models/dits/hdit.py), run on the CPU from
the read-only reference tree.

Run in the build container only:   python tests/golden/make_hdit_fixtures.py
Output: tests/golden/hdit.npz (committed).  Weights come from lidarcrafter_amd.testing.seeded_fill followed by
seeded_fill_hdit, inputs from seeded_randn / torch generators, so the file holds outputs and key lists only.

natten, the CUDA neighbourhood-attention library the reference imports, is not a dependency of this project.  A stub
module is registered in sys.modules before the reference module is imported: `natten.context.is_fna_enabled()` returns
False, which selects the reference's unfused branch, and `natten.functional.na2d_qk` / `na2d_av` are restated below with
natten's non-dilated semantics -- the window of query (i, j) on an H x W grid is rows clamp(i - kh//2, 0, H - kh) + r and
columns clamp(j - kw//2, 0, W - kw) + s (clamped at every border, never padded), the scores in row-major (r, s) order.
The neighbourhood attention of these fixtures is therefore pinned only as far as that restatement goes.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import as R  # noqa: E402

R.install()
from lidarcrafter_amd.testing import seeded_fill, seeded_fill_hdit, seeded_randn  # noqa: E402

torch.set_num_threads(int(os.environ.get("LC_FIXTURE_THREADS", "8")))
torch.manual_seed(0)


def _window_index(n, k):
    """[n, k] indices of natten's clamped window along one axis (no dilation)."""
    start = (torch.arange(n) - k // 2).clamp(0, n - k)
    return start[:, None] + torch.arange(k)[None, :]


def na2d_qk(q, k, kernel_size, dilation=1):
    """q, k [B, N, H, W, D] -> scores [B, N, H, W, kh * kw]."""
    kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
    B, N, H, W, D = k.shape
    ri, ci = _window_index(H, kh), _window_index(W, kw)
    kg = k[:, :, ri][:, :, :, :, ci]                          # [B, N, H, kh, W, kw, D]
    s = torch.einsum("bnhwd,bnhrwsd->bnhwrs", q, kg)
    return s.reshape(B, N, H, W, kh * kw)


def na2d_av(a, v, kernel_size, dilation=1):
    """a [B, N, H, W, kh * kw], v [B, N, H, W, D] -> [B, N, H, W, D]."""
    kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
    B, N, H, W, D = v.shape
    ri, ci = _window_index(H, kh), _window_index(W, kw)
    vg = v[:, :, ri][:, :, :, :, ci]
    return torch.einsum("bnhwrs,bnhrwsd->bnhwd", a.reshape(B, N, H, W, kh, kw), vg)


def _install_natten():
    nat = types.ModuleType("natten")
    nat.context = types.SimpleNamespace(is_fna_enabled=lambda: False)
    nat.functional = types.SimpleNamespace(na2d_qk=na2d_qk, na2d_av=na2d_av)
    sys.modules["natten"] = nat
    dits = types.ModuleType("lidargen.models.dits")
    dits.__path__ = [R.REF + "/lidargen/models/dits"]
    dits.__package__ = "lidargen.models.dits"
    sys.modules["lidargen.models.dits"] = dits


_install_natten()
HD = R.ref("models.dits.hdit")
DF = R.ref("models.diffusion")
LIDAR = R.ref("utils.lidar")

# the config's model params (option_dit_nusc.py); the small model at base 64, 32 x 256
PARAMS = dict(time_embed_channels=256, depths=(3, 3, 3, 3), dilation=(1, 1, 1, 1),
              positional_embedding="learnable_embedding", ring=True)
SALT = 100
LAM_SMALL, LAM_FULL = [-4.0, 2.5], [12.5, -9.0]
COL_STEP = 8                  # stored columns of the 32 x 1024 output
DDIM_STEPS = 4


def build(base, res, ray_angles, clamped_heads=True):
    m = HD.HDiT(res, 2, base_channels=base, **PARAMS)
    if ray_angles:
        m.coords = LIDAR.get_linear_ray_angles(res[0], res[1], 10.0, -30.0)     # inference._build_denoiser
    seeded_fill(m, salt=SALT)
    seeded_fill_hdit(m, salt=SALT, clamped_heads=clamped_heads)
    return m.eval()


def keys_of(module):
    return np.array(sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items()))


def summary(prefix, x, step):
    """A full-size output in a few hundred KB: every `step`-th column, the L2 norm of every row over ALL its columns and
    the per-sample norms."""
    return {f"{prefix}_cols": x[..., ::step].contiguous(), f"{prefix}_rownorm": x.norm(dim=-1),
            f"{prefix}_norm": x.flatten(1).norm(dim=1)}


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
        # small: base 64, 32 x 256 (token grid 32 x 64, mid level 4 x 8), polar coords, B = 2
        ms = build(64, (32, 256), ray_angles=False)
        x = seeded_randn(2, 2, 32, 256, seed=601)
        out["y_small"] = ms(x, torch.tensor(LAM_SMALL))
        # the clamp of the logit scale is exercised: without it the output moves visibly
        saved = {k: v.clone() for k, v in ms.state_dict().items() if k.endswith("residual_attn.scale")}
        for name, p in ms.named_parameters():
            if name.endswith("residual_attn.scale"):
                p.clamp_(max=float(np.log(100.0)) - 0.5)
        y0 = ms(x, torch.tensor(LAM_SMALL))
        ms.load_state_dict(saved, strict=False)
        change = float((y0 - out["y_small"]).norm() / out["y_small"].norm())
        assert change > 1e-3, f"lowering the clamped scales changes y_small by only {change:.2e}"
        out["clamp_sensitivity"] = np.float64(change)

        # the same forward in float64: the reference's own float32 rounding.  Logits of up to 100 make this model
        # ill-conditioned; the GPU test bounds its error against the float64 output by twice the reference's.
        y64 = ms.double()(x.double(), torch.tensor(LAM_SMALL).double())
        ms.float()
        out["y_small64"] = y64
        out["ref_err_small"] = np.float64((out["y_small"].double() - y64).norm() / y64.norm())

        # a short DDIM run of the reference's continuous-time diffusion (per-sample generators) around the small model
        # without the clamped heads: the first step divides the prediction by alpha(lambda_max), which would amplify
        # the rounding of the ill-conditioned forward past any useful bound
        mt = build(64, (32, 256), ray_angles=False, clamped_heads=False)
        ddpm = DF.ContinuousTimeGaussianDiffusion(mt, torch.nn.Identity()).eval()
        rng = [torch.Generator().manual_seed(i) for i in range(2)]
        out["ddim_small"] = ddpm.sample(2, DDIM_STEPS, progress=False, rng=rng, mode="ddim")

        # full size: the config's params, 32 x 1024, ray-angle coords, B = 2
        m = build(128, (32, 1024), ray_angles=True)
        out["keys_model"] = keys_of(m)
        assert sum(p.numel() for p in m.parameters()) == 79_859_844
        x = seeded_randn(2, 2, 32, 1024, seed=602)
        y = m(x, torch.tensor(LAM_FULL))
        out.update(summary("y_full", y, COL_STEP))
        y64 = m.double()(x.double(), torch.tensor(LAM_FULL).double())
        out.update(summary("y_full64", y64, COL_STEP))
        out["ref_err_full"] = np.float64((y.double() - y64).norm() / y64.norm())

    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "hdit.npz")
    save_npz(path, arrays)
    assert os.path.getsize(path) < 1000 * 1024, "hdit.npz grew: store fewer columns"
    print(f"hdit.npz  {os.path.getsize(path) / 1024:.1f} KiB  clamp sensitivity {change:.3e}  reference float32 error "
          f"{float(out['ref_err_small']):.2e} / {float(out['ref_err_full']):.2e}  keys={list(arrays)}")


if __name__ == "__main__":
    main()
