"""CPU-side checks of tests/test_glue_kernels.py, on the inputs its own builders make: the float32 restatement of each
reference stays inside the bound the GPU test holds the kernel to (so the bound is one the reference's own arithmetic
meets), the edge-exclusion caps hold for the chosen seeds, and the planted pixels decide what the GPU tests say they
decide.  Figures measured by these tests are quoted in their docstrings."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_glue_kernels as G  # noqa: E402


@pytest.mark.parametrize("H,W", G.IMAGES)
@pytest.mark.parametrize("fmt", G.FORMATS)
def test_postprocess_restatement_within_bounds(fmt, H, W):
    """float32 against float64 restatement of denormalize -> revert_depth -> to_xyz.  Measured here: depth and reflectance
    reach at most 0.18 of their bound (log_depth, 8 x 256), xyz 0.021 of theirs; at most one pixel of 4096 is an edge pixel
    (share 0.0002 against the cap of 0.005)."""
    x, ang = G.post_input(fmt, H, W), G.ray_angles(H, W)
    assert float(x.max()) > 1.0 and float(x.min()) < -1.0, "some values lie outside [-1, 1]"
    got, _ = G.post_ref(x, ang, fmt, G.MIN_D, G.MAX_D, torch.float32)
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    kept = float((got[:, 0] > 0).float().mean())
    assert 0.2 < kept < 0.95, "both sides of the mask are populated"
    G.check_post(got, x, ang, fmt)


@pytest.mark.parametrize("H,W", G.IMAGES)
def test_postprocess_boundary_pixels(H, W):
    """The three planted inputs are exact in float32 and land on 80.0, on 2.5 and one step above 2.5."""
    x, ang = G.boundary_input(H, W), G.ray_angles(H, W)
    f = np.float32
    for (b, h, w), v in G.BOUNDARY_PIXELS.items():
        assert float(x[b, 0, h, w]) == v, "representable in float32"
    m = [(f(v) + f(1)) / f(2) * f(80) for v in G.BOUNDARY_PIXELS.values()]
    assert [float(v) for v in m] == [80.0, 2.5, 2.5 + 5 * 2.0 ** -17]
    got, _ = G.post_ref(x, ang, G.BOUNDARY["fmt"], G.BOUNDARY["min_d"], G.BOUNDARY["max_d"], torch.float32)
    assert float(got[0, :4, 0, 0].abs().max()) == 0.0 and float(got[0, :4, 1, 7].abs().max()) == 0.0
    assert float(got[1, 0, 2, 49]) == 2.5 + 5 * 2.0 ** -17
    G.check_post(got, x, ang, G.BOUNDARY["fmt"], G.BOUNDARY["min_d"], G.BOUNDARY["max_d"], planted=G.BOUNDARY_PIXELS)


@pytest.mark.parametrize("ncls", [1, 9])
@pytest.mark.parametrize("H,W", G.IMAGES)
@pytest.mark.parametrize("fmt", G.FORMATS)
def test_condition_restatement_within_bounds(fmt, H, W, ncls):
    """float32 against float64 restatement of convert_depth.  Measured here: at most 0.025 of the bound (inverse_depth,
    8 x 256), at most one unplanted edge pixel of 4096 (share 0.0002 against the cap of 0.005).  In float32 the pixel planted at
    float32(1.45) is not above min_depth (the comparison is made in float32, as the kernel makes it)."""
    cm = G.cond_input(fmt, H, W, ncls)
    assert float(cm[:, 0].max()) < ncls and float(cm[:, 0].min()) >= 0
    got = G.cond_depth_ref(cm, fmt, G.MIN_D, G.MAX_D, torch.float32)
    assert got.dtype == torch.float32
    G.check_cond_depth(got, cm, fmt)
    if fmt == "depth":      # torch's float32 division by a Python scalar is a true division, not a reciprocal multiply
        d = cm[:, 1].numpy()
        ref = np.clip(d / np.float32(G.MAX_D), 0, 1) * ((d > np.float32(G.MIN_D)) & (d < np.float32(G.MAX_D)))
        assert np.array_equal(got[:, 0].numpy(), ref.astype(np.float32))


@pytest.mark.parametrize("shape", G.SHAPES, ids=["second_trip", "small"])
def test_pstep_restatement_within_bounds(shape):
    """float32 against float64 restatement of every (objective, mode, noise, clip) single step.  Measured here: the worst
    element of the worst combination reaches 0.25 of the bound at 2 x 1048833 elements, 0.07 at 3 x 30; with clip = 1
    more than 5 % of the x0 estimates are clamped in every combination."""
    pred, x_t, noise = G.operands(shape)
    w = 0.0
    for objective in (0, 1, 2):
        for mode in (0, 1, 2, 3):
            for clip in (0.0, 1.0):
                coef = G.pstep_coef(shape[0], clip)
                assert G.clipped_share(x_t, pred, coef, objective, mode) > 0.05
                for nz in (noise, None):
                    got = G.pstep_ref(x_t, pred, nz, coef, objective, mode, torch.float32)
                    assert got.dtype == torch.float32
                    w = max(w, G.check_pstep(got, x_t, pred, nz, coef, objective, mode))
    print(f"pstep {shape}: float32 restatement at {w:.3f} of the bound")


def test_second_trip_shape():
    """n = 1048576 + 257 exceeds the 4096 * 256 threads of the capped grid; the small shape fits one block."""
    n = [s[1] * s[2] * s[3] for s in G.SHAPES]
    assert n[0] > 4096 * 256 and (n[0] + 255) // 256 > 4096 and n[1] < 256


@pytest.mark.parametrize("H,W", G.IMAGES)
def test_image_to_points_planted_pixels(H, W):
    frame, refl, cond = G.points_frame(H, W)
    xyz = frame[1, 1:4]
    assert (cond > 0).any() and (cond < 0).any() and (cond == 0).any()
    at = lambda flags, h, w: int(flags[h * W + w])               # noqa: E731
    _, k = G.image_to_points_ref(xyz, refl, None, 1.0, 5.0, 0.0)
    assert (at(k, 0, 0), at(k, 0, 1), at(k, 1, 3), at(k, 0, 2)) == (0, 0, 0, 1)
    nrm = xyz.double().pow(2).sum(0).sqrt().reshape(-1)
    others = torch.ones(H * W, dtype=torch.bool)
    others[[0 * W + 1, 1 * W + 3]] = False
    assert float((nrm[others] - 5.0).abs().min()) > 1e-4, "no other pixel has a norm within an ulp of the threshold"
    _, k = G.image_to_points_ref(xyz, refl, None, 1.0, -1.0, 2.0)
    assert (at(k, 1, 0), at(k, 1, 1), at(k, 1, 2), at(k, 2, 0), at(k, 2, 1)) == (1, 1, 1, 0, 0)
    assert 0 < int(k.sum()) < H * W
    rows, k = G.image_to_points_ref(xyz, refl, cond, 255.0, -1.0, 0.0)
    assert k.all() and not rows[(cond.reshape(-1) > 0).numpy()].any() and rows[(cond.reshape(-1) < 0).numpy()].all()
