"""Earth Mover's Distance on the MI355X (csrc/emd.hip, ops.emd_forward, lidargen/metrics/emd.py, eval_utils.evaluate).
`pytest -m gpu`.  Two pins:
  * bit for bit against the numpy restatement of the reference's kernels (tests/_emd_oracle.py), on inputs for which the
    restatement counted none of the ties the reference leaves to a race (asserted here, case by case);
  * independent of the restatement: the auction's eps-optimality against scipy's optimal matching."""
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
