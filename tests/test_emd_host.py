"""CPU-side checks of the EMD feature (csrc/emd.hip, lidargen/metrics/emd.py, eval_utils.py): the numpy restatement the GPU
tests compare against (tests/_emd_oracle.py) is itself checked -- against the auction's eps-optimality with scipy's
optimum, and against the plain arg-max at one iteration; the inputs of the bit-exact GPU tests are free of the two
kinds of ties the reference leaves to a race; the Python layers refuse CPU tensors and bad shapes; evaluate() dispatches."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _emd_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, seed) of every bit-exact GPU comparison at eps = 0.005 (tests/test_emd.py)
BIT_EXACT = [(1024, 0), (1024, 2), (1024, 3), (96, 0), (2500, 0)]


def test_restatement_is_eps_optimal():
    """Once every point is assigned before the last iteration the auction's matching costs at most n * eps more than the
    optimal one (Bertsekas); scipy's linear_sum_assignment on the float64 distances gives the optimum."""
    n, eps = 1024, 0.05
    r = O.case(n, 0, eps, 1500)
    assert 0 in r.unassigned[:-1], "some point was still unassigned before the last iteration"
    assert sorted(r.assignment.tolist()) == list(range(n))
    a, b = O.clouds(n, 0)
    cost = float(np.sqrt(r.dist.astype(np.float64)).sum())
    opt = O.optimum(a, b)
    print(f"auction {cost:.4f}  optimum {opt:.4f}  gap {cost - opt:.4f}  bound {n * eps:.1f}  all assigned at iteration "
          f"{r.unassigned.index(0)}")
    assert opt - 1e-3 <= cost <= opt + n * eps
    assert r.ties_best == 0 and r.ties_window == 0


def test_restatement_one_iteration_is_the_argmax():
    """iters = 1 is the forced last pass alone: at zero prices every point takes the object of the largest 3 - distance."""
    n = 1024
    a, b = O.clouds(n, 0)
    r = O.case(n, 0, 0.005, 1)
    d = b[None, :, :] - a[:, None, :]
    s = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=np.float32)
    want = np.argmax((3.0 - s.astype(np.float64)).astype(np.float32), axis=1)
    assert r.unassigned == [n]
    assert np.array_equal(r.assignment, want)
    dd = a - b[want]
    assert np.array_equal(r.dist, (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])


@pytest.mark.parametrize("n,seed", BIT_EXACT)
def test_bit_exact_inputs_have_no_ties(n, seed):
    r = O.case(n, seed, 0.005, 50)
    assert (r.ties_best, r.ties_window) == (0, 0)
    assert len(r.unassigned) == 50 and r.unassigned[0] == n and r.unassigned[-1] > 0   # the forced last pass has work
    if (n, seed) == (1024, 0):
        for iters in (1, 2):
            q = O.case(n, seed, 0.005, iters)
            assert (q.ties_best, q.ties_window) == (0, 0)


def test_seed_one_has_the_window_tie():
    """What the counters are for: seed 1 at n = 1024 has one object with two bidders inside the 1e-6 window."""
    r = O.case(1024, 1, 0.005, 50)
    assert (r.ties_best, r.ties_window) == (0, 1)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from lidarcrafter_amd import ops

    a = torch.zeros(1, 1024, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.emd_forward(a, a, 0.005, 50)
    with pytest.raises((RuntimeError, ValueError)):
        ops.emd_forward(a, torch.zeros(1, 512, 3), 0.005, 50)
    meta = torch.zeros(1, 8, 3, device="meta")   # .is_cuda is False: refused before anything is dereferenced
    with pytest.raises(RuntimeError):
        ops.emd_forward(meta, meta, 0.005, 50)


def test_pairwise_emd_refuses_cpu_tensors_and_bad_shapes():
    from lidargen.metrics.emd import compute_pairwise_emd, compute_pairwise_emd_batch, emdModule

    x = torch.rand(2048, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_pairwise_emd(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        emdModule()(x[None], x[None], 0.005, 50)
    with pytest.raises(ValueError):
        compute_pairwise_emd(torch.rand(2048, 3), torch.rand(2048, 2))
    with pytest.raises(ValueError):
        compute_pairwise_emd(np.zeros((2048, 3), np.float32), np.zeros((3, 2048), np.float32))
    with pytest.raises(ValueError):
        compute_pairwise_emd(np.zeros((1000, 3), np.float32), np.zeros((2048, 3), np.float32))   # < 1024 in common
    with pytest.raises(AssertionError):
        emdModule()(torch.rand(1, 1024, 3), torch.rand(1, 2048, 3), 0.005, 50)
    with pytest.raises(ValueError):
        compute_pairwise_emd_batch([x], [x, x])


def test_c_entry_refuses_bad_arguments():
    """lc_emd_fwd validates before any launch (callable without a GPU); lc_emd_scratch_bytes is host-only."""
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    LC_EINVAL, LC_EUNSUP = -1, -2
    p = 4096
    ok = dict(B=1, n=1024, eps=0.005, iters=50, tb=0)

    def call(xyz1=p, xyz2=p, dist=p, asg=p, scratch=p, **kw):
        a = dict(ok, **kw)
        return h.lc_emd_fwd(xyz1, xyz2, a["B"], a["n"], a["eps"], a["iters"], a["tb"], dist, asg, scratch, None)

    for null in ("xyz1", "xyz2", "dist", "asg", "scratch"):
        assert call(**{null: None}) == LC_EINVAL, null
    assert call(n=0) == LC_EINVAL and call(B=0) == LC_EINVAL and call(iters=0) == LC_EINVAL
    assert call(eps=-1.0) == LC_EINVAL and call(eps=float("nan")) == LC_EINVAL
    assert call(tb=-1) == LC_EINVAL and call(tb=2049) == LC_EINVAL and call(B=64, tb=65) == LC_EINVAL
    assert call(n=(1 << 24) + 1) == LC_EUNSUP and call(B=65536) == LC_EUNSUP
    assert h.lc_emd_scratch_bytes(0, 1024) == 0 and h.lc_emd_scratch_bytes(1, 0) == 0
    small, big = h.lc_emd_scratch_bytes(1, 1024), h.lc_emd_scratch_bytes(1, 32768)
    assert 0 < small < big < 16 << 20
    assert h.lc_emd_scratch_bytes(16, 8192) < 64 << 20


def test_evaluate_dispatch(monkeypatch):
    from lidargen.metrics import eval_utils as E
    from lidargen.metrics.eval_utils import evaluate

    for m in ("frid", "fsvd", "fpvd", "mmd"):
        with pytest.raises(NotImplementedError, match=f"'{m}'"):
            evaluate([], [], [m], "32")
        with pytest.raises(NotImplementedError, match=f"'{m}'"):
            evaluate([], [], ["cd", m], "32")
    calls = []
    monkeypatch.setattr(E, "compute_cd", lambda r, s: calls.append(("cd", r, s)) or 1.0)
    monkeypatch.setattr(E, "compute_emd", lambda r, s: calls.append(("emd", r, s)) or 2.0)
    monkeypatch.setattr(E, "compute_jsd", lambda r, s, d: calls.append(("jsd", r, s, d)) or 3.0)
    ref, smp = [object()], [object()]
    assert evaluate(ref, smp, ["cd", "emd", "jsd"], "32") == {"cd": 1.0, "emd": 2.0, "jsd": 3.0}
    assert calls == [("cd", ref, smp), ("emd", ref, smp), ("jsd", ref, smp, "32")]
    del calls[:]
    assert evaluate(ref, smp, ["emd"], "64") == {"emd": 2.0}
    assert calls == [("emd", ref, smp)]
    assert evaluate(ref, smp, [], "64") == {}


def test_score_line_wording(capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE

    line = OUTPUT_TEMPLATE.format("EMD ", 0.0123456)
    rule = "-" * 50
    assert line == rule + "\n|" + " " * 16 + "EMD :1.2346E-02" + " " * 17 + "|\n" + rule
    assert all(len(row) == 50 for row in line.split("\n"))


def test_symbols_in_header_binding_and_library():
    from lidarcrafter_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "lidarcrafter_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    h = _lib.lib()
    for name in ("lc_emd_scratch_bytes", "lc_emd_fwd"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(h, name)
    assert "emd.hip" in build.SOURCES
    assert h.lc_abi_version() == 6 and _lib.ABI_VERSION == 6
