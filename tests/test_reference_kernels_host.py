"""The recipe that compiles the reference's own GPU kernels for gfx950 (oracle/build_ref_gpu.py):
where the reference sources exist, build() yields every stamped module, each imports without a GPU
and exposes the reference's functions; a second build() compiles nothing."""
import os

import pytest

from oracle import build_ref_gpu as R


def _have_reference():
    return all(os.path.exists(s) for base in R.EXTENSIONS for s in R._sources(base))


@pytest.fixture(scope="module")
def built():
    if not _have_reference():
        pytest.skip("the reference sources are not on this machine")
    return R.build(verbose=False)


def test_recipe_builds_and_stamps_every_module(built):
    st = R.stamp()
    assert built == R.STAMP and st is not None
    assert sorted(st["modules"]) == sorted(R.module_names())
    assert {st["modules"][n]["fp_contract"] for n in R.module_names()} == {"off", "default"}
    for name in R.module_names():
        assert st["modules"][name]["fp_contract"] == ("default" if name.endswith("_fc") else "off")


@pytest.mark.parametrize("name", R.module_names())
def test_reference_module_imports_and_exposes_its_functions(built, name):
    mod = R.load_gpu_ref(name)
    assert mod is not None
    for fn in R.expected_functions(name):
        assert callable(getattr(mod, fn)), f"{name} lacks {fn}"


def test_second_build_compiles_nothing(built):
    before = {n: os.path.getmtime(os.path.join(R.REF_DIR, n + ".so")) for n in R.module_names()}
    assert R.build(verbose=False) == R.STAMP
    after = {n: os.path.getmtime(os.path.join(R.REF_DIR, n + ".so")) for n in R.module_names()}
    assert before == after


def test_names_do_not_collide_with_the_cpu_reference_module():
    from oracle import build_c

    assert os.path.splitext(os.path.basename(build_c.REF_SO))[0] not in R.module_names()
