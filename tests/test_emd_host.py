"""CPU-side checks of the EMD feature (csrc/emd.hip, lidargen/metrics/emd.py, eval_utils.py): the numpy restatement the GPU
tests compare against (tests/_emd_oracle.py) is itself checked -- against the auction's eps-optimality with scipy's
optimum, and against the plain arg-max at one iteration; the inputs of the bit-exact GPU tests are free of the two
kinds of ties the reference leaves to a race; the restatement under the rule the kernels take where the reference races
(rule="device") agrees with it on those inputs, makes only choices the reference permits on inputs made of ties, and those
inputs have the ties they are there for; a replica of the bid pass's split keeps the triples inside the scratch and says
which splits the tie cases visit; the Python layers refuse CPU tensors and bad shapes; evaluate() dispatches."""
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


# ------------------------------------------------------------------------------------------------- the device rule under ties
def _dev(fam, n, seed, eps=0.005, iters=50):
    return O.case(n, seed, eps, iters, fam, "device")


@pytest.mark.parametrize("n,seed", BIT_EXACT)
def test_rules_agree_on_tie_free_inputs(n, seed):
    """Without ties the two rules are one: same assignment, same dist bits, same trajectory."""
    ref, dev = O.case(n, seed, 0.005, 50), _dev("clouds", n, seed)
    assert np.array_equal(ref.assignment, dev.assignment)
    assert np.array_equal(ref.dist.view(np.uint32), dev.dist.view(np.uint32))
    assert ref.unassigned == dev.unassigned
    assert (dev.ties_best, dev.ties_window, dev.ties_inc) == (0, 0, 0)


MEMBERSHIP = [c[:3] + (0.005, 50) for c in O.TIE_CASES if c[1] <= 1024] + [O.EPS_ZERO, O.EPS_OPT[1]]


@pytest.mark.parametrize("fam,n,seed,eps,iters", MEMBERSHIP, ids=lambda v: str(v))
def test_device_rule_is_a_member_of_the_permitted_set(fam, n, seed, eps, iters):
    """Every choice of a device-rule run is one the reference could have made: the object a point bids for is a maximiser of
    its values (recomputed here in float64 steps from the prices of that iteration), every object that received a bid has
    exactly one winner, and the winner's increment lies inside the reference's 1e-6 window of the object's largest."""
    a, b = O.FAMILIES[fam](n, seed)
    seen = []

    def observe(it, U, bid, inc, price, won):
        d = b[None, :, :] - a[U][:, None, :]
        ss = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        v = (3.0 - np.sqrt(ss, dtype=np.float32).astype(np.float64) - price.astype(np.float64)[None, :]).astype(np.float32)
        assert np.array_equal(v[np.arange(U.size), bid], v.max(axis=1)), it
        if it == iters - 1:
            assert won.all()
            return
        m = np.zeros(n, np.float32)            # max_increments is 0 or -1e9f when an iteration starts, every inc is >= 0
        assert (inc >= 0).all()
        np.maximum.at(m, bid, inc)
        assert np.array_equal(np.bincount(bid[won], minlength=n), (np.bincount(bid, minlength=n) > 0).astype(np.int64)), it
        mw, iw = m[bid[won]].astype(np.float64), inc[won].astype(np.float64)
        assert ((iw - 1e-6 <= mw) & (mw <= iw + 1e-6)).all(), it
        assert np.array_equal(inc[won], m[bid[won]]), it      # and it is the exact largest
        seen.append(it)

    res = O.emd_forward(a, b, eps, iters, "device", observe)
    want = _dev(fam, n, seed, eps, iters)
    assert np.array_equal(res.assignment, want.assignment) and res.unassigned == want.unassigned
    assert seen and seen[0] == 0


# (ties_best, ties_window, ties_inc) with the last pass's share taken off the last two, and the points the forced last pass
# hands out, at eps = 0.005 and 50 iterations
TIE_FIGURES = {
    ("lattice", 96): ((195, 85, 81), 6), ("lattice", 513): ((1802, 1781, 1777), 119),
    ("lattice", 1024): ((7897, 2443, 2443), 220), ("lattice", 2500): ((34538, 3666, 3666), 291),
    ("padded", 96): ((140, 392, 322), 18), ("padded", 1024): ((1391, 1874, 1662), 91),
    ("padded", 2500): ((3273, 3322, 2958), 165),
}


@pytest.mark.parametrize("fam,n,seed,mid", O.TIE_CASES, ids=lambda v: str(v))
def test_tie_cases_have_their_ties(fam, n, seed, mid):
    """A tie case keeps the kind of tie it is there for, whatever is done to its seed later."""
    r = _dev(fam, n, seed)
    decided = (r.ties_best, r.ties_window - r.last_window, r.ties_inc - r.last_inc)
    print(f"{fam}({n}, {seed}): ties (best, window, inc) {decided}, last pass ({r.last_window}, {r.last_inc}), "
          f"unassigned at the last pass {r.unassigned[-1]}")
    assert len(r.unassigned) == 50 and r.unassigned[0] == n
    if fam in ("lattice", "one_object"):
        assert r.ties_best > 0
    if fam in ("lattice", "padded", "one_object"):
        assert r.ties_inc - r.last_inc > 0
    if fam == "padded":
        assert r.ties_window - r.last_window > r.ties_inc - r.last_inc
    if (fam, n) in TIE_FIGURES:
        assert (decided, r.unassigned[-1]) == TIE_FIGURES[(fam, n)]
        assert r.unassigned[-1] > 0                      # the forced last pass has work, and hands out repeated objects
    if fam == "one_object":                              # one point wins per iteration, everything assigned at iteration n
        assert decided == (819, 39, 39) and r.unassigned == list(range(40, 0, -1)) + [0] * 10
    if fam == "clouds":
        assert decided == (0, 1, 0) and (r.last_window, r.last_inc) == (0, 0)
    if fam.startswith("self_pair"):
        a, _ = O.FAMILIES[fam](n, seed)
        assert len(np.unique(a, axis=0)) == n            # no repeated point: a point's own copy is its only best object
        assert r.unassigned == [n] + [0] * 49
        assert not r.dist.any()
        want = np.arange(n) if fam == "self_pair" else np.argsort(O.self_pair_perm(n, seed))
        assert np.array_equal(r.assignment, want)


def test_tie_case_without_an_increment_floor():
    """eps = 0 on the lattice: every tied increment is +0.0, prices of contested objects never move, and the same points
    lose every iteration; the last pass then hands out repeated objects."""
    fam, n, seed, eps, iters = O.EPS_ZERO
    r = _dev(fam, n, seed, eps, iters)
    assert r.unassigned[0] == n and r.unassigned[1:] == [391] * (iters - 1)
    assert r.ties_best > 0 and r.ties_inc - r.last_inc > 0
    assert len(set(r.assignment.tolist())) < n


@pytest.mark.parametrize("fam,n,seed,eps,iters", O.EPS_OPT, ids=lambda v: str(v))
def test_eps_optimal_under_ties(fam, n, seed, eps, iters):
    """The condition of the GPU test of the same cases (everything assigned before the last iteration) and the bound itself,
    on the device-rule restatement."""
    r = _dev(fam, n, seed, eps, iters)
    assert 0 in r.unassigned[:-1]
    assert r.ties_inc > 0 and sorted(r.assignment.tolist()) == list(range(n))
    a, b = O.FAMILIES[fam](n, seed)
    cost, opt = float(np.sqrt(r.dist.astype(np.float64)).sum()), O.optimum(a, b)
    print(f"{fam}({n}, {seed}): auction {cost:.4f}  optimum {opt:.4f}  bound {n * eps:.2f}  all assigned at iteration "
          f"{r.unassigned.index(0)}")
    assert opt - 1e-3 <= cost <= opt + n * eps


def test_ladder_and_batch_inputs():
    """The size ladder and the batch edge cases need no seed picking; what they are there for holds: n = 1 has no second
    best (the increment is the value's distance to the floor), and the rows of a batch differ in their trajectories."""
    r = _dev("clouds", 1, 1)
    assert r.assignment.tolist() == [0] and r.unassigned == [1] + [0] * 49
    assert _dev("clouds", 1, 1, iters=1).assignment.tolist() == [0]
    for n in O.LADDER:
        q = _dev("clouds", n, n)
        assert ((0 <= q.assignment) & (q.assignment < n)).all()
    for B in (33, 40):
        assert O.emd_auto_target(B) == 64 and O.emd_auto_target(32) == 64 and O.emd_auto_target(31) == 66
        for n in (96, 600):
            rows = O.batch_rows(B, n)
            assert {f for f, _, _ in rows} == {"clouds", "lattice", "padded"}
            assert len({tuple(_dev(f, m, s).unassigned) for f, m, s in rows}) == B


def test_plan_replica_keeps_the_triples_inside_the_scratch():
    """csrc/emd.hip emd_plan: cnt * nspans <= max(256 * tgt, cnt) <= emd_cap for every split, so one (best, better, index)
    triple per point and span fits the scratch sized from the auto target.  A handful by hand, then a sweep."""
    assert O.emd_plan(2500, 2500, 24) == O.Plan(1, 10, 2, 3, 5)          # ten groups, spans of 3 + 2 chunks
    assert O.emd_plan(2500, 2500, 2048) == O.Plan(64, 625, 3, 2, 5)
    assert O.emd_plan(2500, 2500, 1) == O.Plan(1, 10, 1, 5, 5)
    assert O.emd_plan(20, 32768, 2048) == O.Plan(64, 5, 64, 1, 64)       # 20 bidders: a wave per point, every chunk a span
    assert O.emd_plan(32768, 32768, 2048) == O.Plan(1, 128, 16, 4, 64)   # 32 k bidders: one lane per point
    assert O.emd_plan(1, 1, 2048) == O.Plan(64, 1, 1, 1, 1)
    assert O.emd_plan(512, 512, 64) == O.Plan(64, 128, 1, 1, 1)          # 256 * groups = 32768 > emd_cap(32, 512) = 16896
    assert (O.emd_auto_target(1), O.emd_auto_target(8), O.emd_auto_target(33), O.emd_auto_target(65535)) == (2048, 256, 64, 64)
    for B in (1, 3, 32, 33, 40, 4096):
        auto = O.emd_auto_target(B)
        for n in (1, 3, 96, 511, 512, 513, 600, 1024, 2500, 32768):
            cap = O.emd_cap(B, n)
            for tgt in sorted({1, 2, 7, 24, 63, 64, auto // 2, auto}):
                if tgt > auto:
                    continue
                for cnt in sorted({1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, n // 3 + 1, n - 1, n}):
                    if not 1 <= cnt <= n:
                        continue
                    p = O.emd_plan(cnt, n, tgt)
                    assert p.T in (1, 4, 16, 64) and p.groups * (O.BLK // p.T) >= cnt
                    assert 1 <= p.nspans <= p.nch and p.nspans * p.cps >= p.nch > (p.nspans - 1) * p.cps
                    assert cnt * p.nspans <= max(O.BLK * tgt, cnt) <= cap, (B, n, tgt, cnt, p)
                    assert cnt * p.nspans <= O.BLK * max(tgt, p.groups)


def test_split_coverage():
    """Under ties the GPU cases visit every T and merge several spans: from the replica over the restatement's trajectory."""
    seen = set()
    for fam, n, seed, mid in O.TIE_CASES:
        r = _dev(fam, n, seed)
        for tb in (0, mid, 1):
            s = O.splits(r.unassigned, n, 1, tb)
            print(f"{fam}({n}, {seed}) target_blocks {tb}: (T, spans) {sorted(s)}")
            if (r.ties_best, r.ties_window, r.ties_inc) != (0, 0, 0):
                seen |= s
        assert 1 < mid < O.emd_auto_target(1)
        assert O.splits(r.unassigned, n, 1, 1) == {(1, 1)}
    assert {T for T, _ in seen} == {1, 4, 16, 64}
    for T in (1, 4, 16, 64):
        assert any(t == T and ns > 1 for t, ns in seen), T    # the span merge behind every lane count
    fam, n, seed, eps, iters = O.EPS_ZERO
    assert O.splits(_dev(fam, n, seed, eps, iters).unassigned, n, 1, 6) == {(1, 2), (4, 1)}
    for B in (33, 40):                                        # the batch edges run at the floor of the auto target
        rows = O.batch_rows(B, 600)
        s = set().union(*(O.splits(_dev(f, m, q).unassigned, m, B, 0) for f, m, q in rows))
        print(f"B = {B}, n = 600: (T, spans) {sorted(s)}")
        assert {T for T, _ in s} >= {16, 64} and any(ns > 1 for _, ns in s)


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
