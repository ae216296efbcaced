"""CPU part of the error-profile tests (DESIGN.md "Error profiles"): the helper against hand-computed profiles, the
demonstration that a fault confined to one slice passes the whole-tensor bound and fails the profile conditions, and the
float32 reference alone inside the conditions at every shape and slicing tests/test_error_profiles.py uses on the GPU."""
import math

import pytest
import torch

from lidarcrafter_amd.testing import error_profiles, rel_l2, seeded_randn
from tests import _profile_cases as PC


def test_helper_against_hand_computed_profiles():
    ref = torch.tensor([[3.0, 4.0], [6.0, 8.0], [5.0, 12.0]], dtype=torch.float64)
    got = ref.clone().float()
    got[0, 0] += 0.3            # row 0: 0.3 / 5
    got[2, 1] -= 1.3            # row 2: 1.3 / 13; column 1: 1.3 / sqrt(16 + 64 + 144)
    p = error_profiles(got, ref, [(0,), (1,)], min_elems=2)
    assert p["whole"] == pytest.approx(math.sqrt(0.09 + 1.69) / math.sqrt(294.0), rel=1e-6)
    rows = p["profiles"][(0,)]
    assert rows["err"].tolist() == pytest.approx([0.06, 0.0, 0.1], rel=1e-6, abs=1e-9)
    assert rows["index"] == (2,) and rows["worst"] == pytest.approx(0.1, rel=1e-6) and rows["median"] == pytest.approx(0.06, rel=1e-6)
    cols = p["profiles"][(1,)]
    assert cols["err"].tolist() == pytest.approx([0.3 / math.sqrt(70.0), 1.3 / math.sqrt(224.0)], rel=1e-6)
    assert cols["index"] == (1,)
    # two kept axes: every element its own slice; the index is a tuple over the kept axes
    e = error_profiles(got, ref, [(0, 1)], min_elems=1)["profiles"][(0, 1)]
    assert e["index"] == (2, 1) and tuple(e["err"].shape) == (3, 2) and e["worst"] == pytest.approx(1.3 / 12, rel=1e-6)


def test_helper_refuses_small_slices_and_float32_references():
    ref = seeded_randn(4, 8, 16, seed=1).double()
    got = ref.float()
    error_profiles(got, ref, [(0,), (1,)])               # 128 and 64 elements per slice
    with pytest.raises(ValueError, match="hold 32 < 64"):
        error_profiles(got, ref, [(2,)])
    with pytest.raises(ValueError):
        error_profiles(got, ref, [(0, 1)])               # 16 per slice
    with pytest.raises(TypeError):
        error_profiles(got, ref.float(), [(0,)])
    with pytest.raises(ValueError):
        error_profiles(got[:2], ref, [(0,)])
    assert PC.usable(ref.shape, [(0,), (1,), (2,), (0, 1)]) == ((0,), (1,))


@pytest.fixture(scope="module")
def big_conv():
    """ref32 / ref64 of test_conv's (1, 32, 64, 32, 1024): the shape of the dilution argument."""
    c = PC.conv_case((1, 32, 64, 32, 1024, 3), "plain")
    return c.ref32, c.ref64


def test_reference_alone_at_the_sensitivity_shape(big_conv):
    ref32, ref64 = big_conv
    lines, fails = PC.check_profiles(ref32, ref32, ref64, PC.NCHW_KEEPS, PC.TOL_CONV, name="ref32")
    print("\n".join(lines))
    assert not fails


@pytest.mark.parametrize("what", ["column", "tile_row"])
def test_planted_fault_passes_the_whole_tensor_bound_and_fails_the_profiles(big_conv, what):
    """A relative fault of 2e-5 in one column (the ring-wrap column, say), and in one row of one 64-column tile of the
    64-channel block: diluted by sqrt(n / N) to 6e-7 and 9e-7, inside test_conv's 2e-6; the profiles name the slice.
    (A whole image row of the block is 1 / 32 of this output: 2e-5 / sqrt(32) = 3.5e-6 fails the old bound already.)"""
    ref32, ref64 = big_conv
    got = ref32.clone()
    if what == "column":
        got[..., 517] *= 1 + 2e-5
        where = ["axes (3,) slice (517,)", "axes (2, 3) slice"]
    else:
        got[:, :, 13, 128:192] *= 1 + 2e-5
        where = ["axes (2,) slice (13,)", "axes (2, 3) slice (13, 1"]
    assert rel_l2(got, ref64) < PC.TOL_CONV                       # what the suite saw so far
    lines, fails = PC.check_profiles(got, ref32, ref64, PC.NCHW_KEEPS, PC.TOL_CONV, name=what)
    print("\n".join(lines))
    for w in where:
        assert any(w in f and "bound" in f for f in fails), (w, fails)
        assert any(w in f and "median" in f for f in fails), (w, fails)
    # sample and channel profiles cannot see it: the fault crosses every channel
    assert not any("axes (0,)" in f or "axes (1,)" in f for f in fails), fails


_HOST = dict(PC.host_cases())


@pytest.mark.parametrize("name", list(_HOST))
def test_reference_alone_stays_inside_the_conditions(name):
    """ref32 against ref64 at every listed shape and slicing: inside the bound with the existing tolerance, and u_ref is
    finite (no slice with a zero reference norm, no slice the float32 reference evaluates exactly)."""
    ref32, ref64, keeps, tol = _HOST[name]()
    keeps = PC.usable(ref64.shape, keeps)
    # skinny (37, 512, 20): rows hold 20 and columns 37 elements, both under the helper's rule -- only the whole-tensor
    # figure is left there, and the rule stays
    assert keeps or name == "skinny-(37, 512, 20)", "no profile has slices of 64 elements at this shape"
    lines, fails = PC.check_profiles(ref32, ref32, ref64, keeps, tol, name=name)
    print("\n".join(lines))
    assert not fails, fails
    r = error_profiles(ref32, ref64, keeps)
    for keep in keeps:
        p = r["profiles"][keep]
        assert math.isfinite(p["worst"]) and p["median"] > 0 and math.isfinite(p["worst"] / p["median"]), (keep, p["worst"], p["median"])
