"""Earth Mover's Distance on the MI355X (csrc/emd.hip, ops.emd_forward, lidargen/metrics/emd.py, eval_utils.evaluate).
`pytest -m gpu`.  Three pins:
  * bit for bit against the numpy restatement of the reference's kernels (tests/_emd_oracle.py), on inputs for which the
    restatement counted none of the ties the reference leaves to a race (asserted here, case by case);
  * bit for bit against the same restatement under the rule the kernels take where the reference races (rule="device"), on
    inputs made of ties (a lattice, padded clouds, one repeated object, a cloud against itself), on every route of the bid
    pass, twice each; on the size ladder n = 1 ... 1025; and on batches of more than 32 pairs;
  * independent of the restatement: the auction's eps-optimality against scipy's optimal matching, with and without ties."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _emd_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, ITERS = 0.005, 50


def _run(pairs, eps=EPS, iters=ITERS, target_blocks=0):
    """ops.emd_forward on clouds(n, seed) for every (n, seed) of `pairs` (one n) -> numpy dist, assignment."""
    from lidarcrafter_amd import ops

    cl = [O.clouds(n, s) for n, s in pairs]
    a = torch.from_numpy(np.stack([c[0] for c in cl])).cuda()
    b = torch.from_numpy(np.stack([c[1] for c in cl])).cuda()
    dist, asg = ops.emd_forward(a, b, eps, iters, target_blocks=target_blocks)
    assert dist.dtype == torch.float32 and asg.dtype == torch.int32 and dist.shape == asg.shape == a.shape[:2]
    return dist.cpu().numpy(), asg.cpu().numpy()


def _check(pairs, dist, asg, eps=EPS, iters=ITERS):
    for row, (n, seed) in enumerate(pairs):
        want = O.case(n, seed, eps, iters)
        assert (want.ties_best, want.ties_window) == (0, 0), "pick another seed: the reference's outcome is a race here"
        bad = np.flatnonzero(asg[row] != want.assignment)
        assert bad.size == 0, (n, seed, f"{bad.size} assignments differ, first at point {bad[:1]}")
        assert np.array_equal(dist[row].view(np.uint32), want.dist.view(np.uint32)), (n, seed)


# the bid pass splits its work by the number of bidders: 1 / 4 / 16 / 64 lanes per point, 1 ... all chunks of 512 objects per
# span.  Auto (2048 blocks per pair) runs these small shapes at 64 lanes per point throughout; target_blocks = 24 starts
# n = 2500 at one lane per point with two spans (3 + 2 chunks) and walks through 4, 16 and 64 lanes as the bidders thin out;
# target_blocks = 1 keeps one lane per point, one span and one block for the whole run.
@pytest.mark.parametrize("n,seed,target_blocks", [
    (1024, 0, 0),        # the base shape: two whole chunks
    (96, 0, 0),          # fewer points than a block, one ragged chunk
    (2500, 0, 0),        # five chunks, the last one ragged (452 objects)
    (2500, 0, 24),
    (2500, 0, 1),
    (1024, 2, 6),
])
def test_bit_exact_against_restatement(n, seed, target_blocks):
    dist, asg = _run([(n, seed)], target_blocks=target_blocks)
    _check([(n, seed)], dist, asg)


@pytest.mark.parametrize("iters", [1, 2])
def test_forced_last_pass_and_one_eviction_round(iters):
    dist, asg = _run([(1024, 0)], iters=iters)
    _check([(1024, 0)], dist, asg, iters=iters)


BATCH = [(1024, 0), (1024, 2), (1024, 3)]


def test_batch_of_three_pairs():
    """Pairs whose unassigned counts differ at every iteration share each launch."""
    dist, asg = _run(BATCH)
    _check(BATCH, dist, asg)
    counts = [O.case(n, s, EPS, ITERS).unassigned for n, s in BATCH]
    assert len({tuple(c) for c in counts}) == 3


def test_batch_rows_equal_single_calls():
    dist, asg = _run(BATCH)
    for row, pair in enumerate(BATCH):
        d1, a1 = _run([pair])
        assert np.array_equal(asg[row], a1[0]) and np.array_equal(dist[row].view(np.uint32), d1[0].view(np.uint32))


def test_eps_optimality_against_scipy():
    """Independent of the restatement: with every point assigned before the last iteration the assignment is a permutation
    whose cost is within n * eps of the optimal matching's."""
    n, eps = 1024, 0.05
    dist, asg = _run([(n, 0)], eps=eps, iters=1500)
    assert sorted(asg[0].tolist()) == list(range(n))
    a, b = O.clouds(n, 0)
    d = a - b[asg[0]]
    assert np.array_equal(dist[0], (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    cost = float(np.sqrt(dist[0].astype(np.float64)).sum())
    opt = O.optimum(a, b)
    print(f"auction {cost:.4f}  optimum {opt:.4f}  gap {cost - opt:.4f}  bound {n * eps:.1f}")
    assert opt - 1e-3 <= cost <= opt + n * eps


# ------------------------------------------------------------------------------------------------------------ under ties
# Bit for bit against the restatement under the DEVICE rule (tests/_emd_oracle.py rule="device": the lowest object index
# among equal best values, the largest (increment bits, j) pair among an object's bidders), which is defined for every
# input; test_emd_host.py shows that every choice it makes is one the reference permits, and that these inputs have ties.
def _forward(a, b, eps=EPS, iters=ITERS, target_blocks=0):
    """ops.emd_forward on numpy clouds [B, n, 3] -> numpy dist, assignment; range and consistency checked on every run."""
    from lidarcrafter_amd import ops

    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    dist, asg = ops.emd_forward(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), eps, iters, target_blocks=target_blocks)
    assert dist.dtype == torch.float32 and asg.dtype == torch.int32 and dist.shape == asg.shape == a.shape[:2]
    dist, asg = dist.cpu().numpy(), asg.cpu().numpy()
    n = a.shape[1]
    assert ((0 <= asg) & (asg < n)).all(), "assignment out of range"
    d = a - np.take_along_axis(b, asg.astype(np.int64)[..., None], axis=1)
    want = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert np.array_equal(dist.view(np.uint32), want.view(np.uint32)), "dist is not the distance to the assigned object"
    return dist, asg


def _same(got, want_dist, want_asg, what):
    dist, asg = got
    bad = np.flatnonzero(asg != want_asg)
    assert bad.size == 0, (what, f"{bad.size} assignments differ, first at point {bad[:1]}: {asg[bad[:1]]} for {want_asg[bad[:1]]}")
    assert np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32)), what


def _routes(fam, n, seed, mid, eps=EPS, iters=ITERS):
    """One pair at target_blocks auto, `mid` and 1, each twice: all six equal to the device-rule restatement, hence to each
    other and to themselves (the order of the bidder list, which varies from run to run, does not reach the result)."""
    a, b = O.FAMILIES[fam](n, seed)
    want = O.case(n, seed, eps, iters, fam, "device")
    print(f"{fam}({n}, {seed}) eps {eps}: ties (best, window, inc) {(want.ties_best, want.ties_window, want.ties_inc)}, of these in the "
          f"last pass {(want.last_window, want.last_inc)}; unassigned at the last pass {want.unassigned[-1]}")
    first = None
    for tb in (0, mid, 1):
        print(f"  target_blocks {tb}: (T, spans) visited {sorted(O.splits(want.unassigned, n, 1, tb))}")
        for rep in range(2):
            got = _forward(a[None], b[None], eps, iters, tb)
            got = (got[0][0], got[1][0])
            _same(got, want.dist, want.assignment, (fam, n, seed, "target_blocks", tb, "run", rep))
            first = got if first is None else first
            _same(got, first[0], first[1], (fam, n, seed, "route", tb, "run", rep, "against the first run"))
    return first


@pytest.mark.parametrize("fam,n,seed,mid", O.TIE_CASES, ids=lambda v: str(v))
def test_ties_bit_exact_on_every_route(fam, n, seed, mid):
    dist, asg = _routes(fam, n, seed, mid)
    if fam.startswith("self_pair"):
        assert not dist.view(np.uint32).any()            # +0.0 exactly
        want = np.arange(n) if fam == "self_pair" else np.argsort(O.self_pair_perm(n, seed))
        assert np.array_equal(asg, want)


def test_ties_without_an_increment_floor():
    """eps = 0: every tied increment is +0.0 and the packed word orders by j + 1 alone."""
    fam, n, seed, eps, iters = O.EPS_ZERO
    _routes(fam, n, seed, 6, eps, iters)


@pytest.mark.parametrize("n", O.LADDER)
def test_size_ladder(n):
    """n = 1 (no second best), n < 4, and one below / at / one above the wave, the block and the object chunk."""
    a, b = O.clouds(n, n)
    for iters in (ITERS, 1) if n == 1 else (ITERS,):
        want = O.case(n, n, EPS, iters, "clouds", "device")
        for tb in (0, 1):
            got = _forward(a[None], b[None], EPS, iters, tb)
            _same((got[0][0], got[1][0]), want.dist, want.assignment, (n, "iters", iters, "target_blocks", tb))


@pytest.mark.parametrize("B,n,target_blocks", [(33, 96, 0), (33, 600, 0), (40, 96, 0), (40, 600, 0), (40, 600, 64)])
def test_batch_edges(B, n, target_blocks):
    """More than 32 pairs: the auto target sits at its floor of 64 blocks per pair and the triple scratch is sized from it.
    Rows of three families share every launch; each equals the restatement and its own single-pair call (auto target 2048)."""
    assert O.emd_auto_target(B) == 64
    rows = O.batch_rows(B, n)
    cl = [O.FAMILIES[f](m, s) for f, m, s in rows]
    a, b = np.stack([c[0] for c in cl]), np.stack([c[1] for c in cl])
    dist, asg = _forward(a, b, target_blocks=target_blocks)
    for r, (f, m, s) in enumerate(rows):
        want = O.case(m, s, EPS, ITERS, f, "device")
        _same((dist[r], asg[r]), want.dist, want.assignment, ("row", r, f, m, s))
        if target_blocks == 0:
            one = _forward(a[r:r + 1], b[r:r + 1])
            _same((dist[r], asg[r]), one[0][0], one[1][0], ("row", r, "against its single-pair call"))


@pytest.mark.parametrize("fam,n,seed,eps,iters", O.EPS_OPT, ids=lambda v: str(v))
def test_eps_optimality_under_ties(fam, n, seed, eps, iters):
    """Independent of any restatement: a permutation within n * eps (Bertsekas) of scipy's optimal matching.  That everything
    is assigned before the last iteration is a condition on the inputs, taken from the device-rule restatement."""
    assert 0 in O.case(n, seed, eps, iters, fam, "device").unassigned[:-1]
    a, b = O.FAMILIES[fam](n, seed)
    dist, asg = _forward(a[None], b[None], eps, iters)
    assert sorted(asg[0].tolist()) == list(range(n))
    d = a - b[asg[0]]
    assert np.array_equal(dist[0], (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    cost = float(np.sqrt(dist[0].astype(np.float64)).sum())
    opt = O.optimum(a, b)
    print(f"{fam}({n}, {seed}): auction {cost:.4f}  optimum {opt:.4f}  gap {cost - opt:.4f}  bound {n * eps:.2f}")
    assert opt - 1e-3 <= cost <= opt + n * eps


def test_front_ends_under_ties():
    from lidargen.metrics.emd import compute_pairwise_emd, compute_pairwise_emd_batch

    x = O.clouds(2048, 21)[0]
    assert compute_pairwise_emd(x, x) == 0.0
    for fam in ("padded", "lattice"):
        a, b = O.FAMILIES[fam](2048, 2048)
        want = O.case(2048, 2048, EPS, ITERS, fam, "device")
        assert want.ties_inc > 0
        ref = float(np.sqrt(want.dist.astype(np.float64)).mean())
        got = compute_pairwise_emd(a, b)
        assert abs(got - ref) <= 16 * 2.0 ** -23 * ref, (fam, got, ref)   # the bound of test_compute_pairwise_emd_truncates_and_matches
    # 34 pairs, 33 of truncated length 1024 (one launch sequence at the floor of the auto target) around one of 2048
    refs, smps = [], []
    for r in range(34):
        fam = ("clouds", "lattice", "padded", "self_pair")[r % 4]
        a, b = O.FAMILIES[fam](2100 if r == 17 else 1100 + 2 * r, 300 + r)
        refs.append(a)
        smps.append(b[:len(b) - 30])      # cut to 2048 (row 17) and to 1024: a padded cloud keeps part of its repeat
    assert sorted(min(len(r), len(s)) // 1024 for r, s in zip(refs, smps)) == [1] * 33 + [2]
    assert compute_pairwise_emd_batch(refs, smps) == [compute_pairwise_emd(r, s) for r, s in zip(refs, smps)]


def test_call_sequence():
    """Scratch is initialised by every call: the same call twice, and shape A, a smaller shape B, then A again."""
    a1 = _run([(1024, 0)])
    a2 = _run([(1024, 0)])
    b1 = _run([(96, 0)])
    a3 = _run([(1024, 0)])
    for other in (a2, a3):
        assert np.array_equal(a1[1], other[1]) and np.array_equal(a1[0].view(np.uint32), other[0].view(np.uint32))
    _check([(1024, 0)], *a3)
    _check([(96, 0)], *b1)


def test_ops_refuse_bad_shapes_and_arguments():
    from lidarcrafter_amd import ops

    a = torch.zeros(1, 1024, 3, device="cuda")
    for other in (torch.zeros(1, 512, 3, device="cuda"), torch.zeros(2, 1024, 3, device="cuda"),
                  torch.zeros(1, 1024, 2, device="cuda"), torch.zeros(1024, 3, device="cuda")):
        with pytest.raises(ValueError):
            ops.emd_forward(a, other, EPS, ITERS)
    with pytest.raises(ValueError):
        ops.emd_forward(a, a, EPS, 0)
    with pytest.raises(ValueError):
        ops.emd_forward(a, a, -0.1, ITERS)
    with pytest.raises(TypeError):
        ops.emd_forward(a.double(), a.double(), EPS, ITERS)


def _ragged(seed):
    rng = np.random.default_rng(seed)
    return rng.random((2500, 3), np.float32), rng.random((2300, 3), np.float32)


def test_compute_pairwise_emd_truncates_and_matches():
    from lidargen.metrics.emd import compute_pairwise_emd, compute_pairwise_emd_batch

    x, y = _ragged(14)
    want = O.emd_forward(x[:2048], y[:2048], EPS, ITERS)
    assert (want.ties_best, want.ties_window) == (0, 0)
    ref = float(np.sqrt(want.dist.astype(np.float64)).mean())
    got = compute_pairwise_emd(x, y)
    # float32 sqrt within 1 ulp (2^-23), a blocked / tree float32 sum of 2048 positive terms (<= 25 additions on any path,
    # 2^-24 each), one division: 16 * 2^-23 relative covers it
    assert abs(got - ref) <= 16 * 2.0 ** -23 * ref, (got, ref)
    assert compute_pairwise_emd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) == got
    # the batch: two pairs of truncated length 2048 around one of 1024, one launch per length, the per-pair values exactly
    x2, y2 = _ragged(16)
    refs, smps = [x, x2[:1500], x2], [y, y2[:1100], y2]
    assert compute_pairwise_emd_batch(refs, smps) == [compute_pairwise_emd(r, s) for r, s in zip(refs, smps)]


def test_emd_function_backward():
    from lidargen.metrics.emd import emdModule

    a, b = (torch.from_numpy(c).cuda()[None] for c in O.clouds(1024, 0))
    a.requires_grad_(True)
    b.requires_grad_(True)
    dist, asg = emdModule()(a, b, EPS, ITERS)
    assert not asg.requires_grad
    g = torch.linspace(-1.0, 2.0, 1024, device="cuda")[None]
    ga, gb = torch.autograd.grad(dist, (a, b), g)
    want = 2 * g[..., None] * (a.detach() - b.detach()[0, asg[0].long()][None])
    assert torch.equal(ga, want)
    assert torch.equal(gb, torch.zeros_like(b))
    assert np.array_equal(asg[0].cpu().numpy(), O.case(1024, 0, EPS, ITERS).assignment)


def test_evaluate_returns_the_individual_scores(capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, metric_utils
    from lidargen.metrics.chamfer import compute_pairwise_cd
    from lidargen.metrics.emd import compute_pairwise_emd
    from lidargen.metrics.eval_utils import evaluate

    rng = np.random.default_rng(20)
    ref = [rng.random((2048, 3), np.float32) for _ in range(2)]
    smp = [rng.random((2048, 3), np.float32) for _ in range(2)]
    got = evaluate(ref, smp, ["cd", "emd", "jsd"], "32")
    assert sorted(got) == ["cd", "emd", "jsd"]
    assert got["cd"] == sum(compute_pairwise_cd(r, s) for r, s in zip(ref, smp)) / 2
    assert got["emd"] == sum(compute_pairwise_emd(r, s) for r, s in zip(ref, smp)) / 2
    assert got["jsd"] == metric_utils.compute_jsd(ref, smp, "32")
    assert 0 < got["cd"] and 0 < got["emd"] < 3 ** 0.5 and 0 <= got["jsd"] <= 1
    out = capsys.readouterr().out
    for name in ("CD  ", "EMD ", "JSD "):
        assert OUTPUT_TEMPLATE.format(name, got[name.strip().lower()]) in out
