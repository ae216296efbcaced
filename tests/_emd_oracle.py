"""CPU restatement of the reference's auction EMD (lidargen/metrics/modules/emd/emd_cuda.cu emd_cuda_forward, state of
emd_module.py:59-70), written from the kernel text: numpy, float32 with the reference's float64 steps.

  value of object k for point j   (float)(3.0 - (double)sqrtf((x*x + y*y) + z*z) - (double)price[k]),  (x, y, z) = xyz2[k] - xyz1[j]
  best / better                   the largest and the second largest value of the multiset, floor -1e9f
  increment                       (best - better) + eps in float32; max_increments[best_i] = max(., increment)
  winner of an object             a bidder whose increment lies within 1e-6 (float64) of the object's max_increments
  assignment                      the winner evicts the previous owner, price += increment, max_increments = -1e9f
  last iteration                  every still-unassigned point takes its own bid, no eviction

Where the reference races the restatement decides, by one of two rules:

  rule="reference"  the LOWEST object index among equal best values, the HIGHEST point index among an object's bidders
                    inside the 1e-6 window.  A bit-exact comparison against it is meaningful only for inputs where
                    `ties_best` and `ties_window` are both zero.
  rule="device"     what csrc/emd.hip takes ("Permitted outcomes"): the lowest object index among
                    equal best values, and for an object the bidder of the largest (float32 bits of the increment, j)
                    pair -- the exact largest increment, the highest j among equal ones.  Defined for every input.

All three kinds of ties are counted under either rule: `ties_best` (point, iteration) cases whose best value occurs twice,
`ties_window` (object, iteration) cases with two or more bidders inside the window, `ties_inc` (object, iteration) cases
with two or more bidders holding exactly the object's largest increment.  The forced last pass is counted like every other
(the condition `ties == (0, 0)` of the reference-rule comparisons is the stricter for it) although it picks no winner;
`last_window` and `last_inc` are its share, so `ties_window - last_window` and `ties_inc - last_inc` count decisions only.

The module also holds the seeded input families of the tie tests, the list of tie cases shared by the host and the GPU
tests, and a plain-Python replica of the bid pass's split (emd_plan, emd_auto_target, emd_cap of csrc/emd.hip).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "dist assignment unassigned ties_best ties_window ties_inc last_window last_inc")
FLOOR = np.float32(-1e9)


# ---------------------------------------------------------------------------------------------------------- input families
def clouds(n: int, seed: int):
    """Cloud 1, then cloud 2, from one generator: [n, 3] float32 in [0, 1)."""
    rng = np.random.default_rng(seed)
    return rng.random((n, 3), np.float32), rng.random((n, 3), np.float32)


def lattice(n: int, seed: int):
    """Both clouds drawn from the 125 points of {0, 1/4, 1/2, 3/4, 1}^3: equal values, equal increments, repeated points."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 5, (n, 3)).astype(np.float32) / np.float32(4)
    b = rng.integers(0, 5, (n, 3)).astype(np.float32) / np.float32(4)
    return a, b


def padded(n: int, seed: int):
    """clouds(n // 2, seed), each cloud concatenated with itself (a cloud padded to length by repeating its points)."""
    assert n % 2 == 0
    a, b = clouds(n // 2, seed)
    return np.concatenate([a, a]), np.concatenate([b, b])


def one_object(n: int, seed: int):
    """Cloud 2 is n copies of one point: every point ties over all n objects, every increment is eps exactly."""
    a, b = clouds(n, seed)
    return a, np.repeat(b[:1], n, axis=0)


def self_pair(n: int, seed: int):
    """Cloud 2 is cloud 1."""
    a, _ = clouds(n, seed)
    return a, a.copy()


def self_pair_perm(n: int, seed: int):
    """The permutation of self_pair_permuted: cloud 2 [k] = cloud 1 [perm[k]]."""
    return np.random.default_rng(seed + 1000).permutation(n)


def self_pair_permuted(n: int, seed: int):
    """Cloud 2 is a fixed permutation of cloud 1."""
    a, _ = clouds(n, seed)
    return a, a[self_pair_perm(n, seed)].copy()


FAMILIES = {"clouds": clouds, "lattice": lattice, "padded": padded, "one_object": one_object, "self_pair": self_pair,
            "self_pair_permuted": self_pair_permuted}

# (family, n, seed, a target_blocks between 1 and auto) of every tie case the GPU tests run at eps = 0.005, 50 iterations;
# the middle value is picked with the plan replica below (test_emd_host.py test_split_coverage says what each one reaches)
TIE_CASES = [
    ("lattice", 96, 96, 2),
    ("lattice", 513, 513, 6),
    ("lattice", 1024, 1024, 30),
    ("lattice", 2500, 2500, 24),
    ("padded", 96, 96, 2),
    ("padded", 1024, 1024, 14),
    ("padded", 2500, 2500, 24),
    ("one_object", 40, 40, 2),
    ("clouds", 1024, 1, 8),
    ("self_pair", 1024, 7, 8),
    ("self_pair_permuted", 1024, 7, 8),
]

# the one tie case at eps = 0 (every tied increment is +0.0) and the two eps-optimality cases under ties:
# (family, n, seed, eps, iterations)
EPS_ZERO = ("lattice", 513, 513, 0.0, 50)
EPS_OPT = [("lattice", 513, 513, 0.05, 1500), ("padded", 512, 5, 0.05, 400)]
# clouds(n, n) of the size ladder: 1 (no second best), below 4, around the 64-lane wave, the 256-thread block and the
# 512-object chunk, and one past two chunks
LADDER = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]


def batch_rows(B: int, n: int):
    """(family, n, seed) of the rows of a batch edge case: the three families in turn, a seed per row."""
    return [(("clouds", "lattice", "padded")[r % 3], n, 100 + r) for r in range(B)]


# ------------------------------------------------------------------------------------------------------------ restatement
def _values(p1, xyz2, price):
    """[u, n] float32 values of every object for the points p1 [u, 3]."""
    d = xyz2[None, :, :] - p1[:, None, :]
    ss = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    s = np.sqrt(ss, dtype=np.float32)
    return ((np.float64(3.0) - s.astype(np.float64)) - price.astype(np.float64)[None, :]).astype(np.float32)


def emd_forward(xyz1: np.ndarray, xyz2: np.ndarray, eps: float, iters: int, rule: str = "reference", observe=None) -> Result:
    """observe(it, U, bid, inc, price, won): called once per iteration that has bidders, with the unassigned points U, their
    bids and increments, the prices they bid at, and the mask of the bidders that take their object (in the last
    iteration: all of them)."""
    assert rule in ("reference", "device")
    xyz1 = np.ascontiguousarray(xyz1, np.float32)
    xyz2 = np.ascontiguousarray(xyz2, np.float32)
    n = xyz1.shape[0]
    assert xyz1.shape == xyz2.shape == (n, 3) and iters >= 1
    eps = np.float32(eps)
    assignment = np.full(n, -1, np.int32)
    assignment_inv = np.full(n, -1, np.int32)
    price = np.zeros(n, np.float32)
    max_inc = np.zeros(n, np.float32)
    max_idx = np.zeros(n, np.int32)
    unassigned, ties_best, ties_window, ties_inc, last_window, last_inc = [], 0, 0, 0, 0, 0
    for it in range(iters):
        last = it == iters - 1
        U = np.flatnonzero(assignment == -1)
        unassigned.append(int(U.size))
        if U.size == 0:
            continue
        bid = np.empty(U.size, np.int64)
        inc = np.empty(U.size, np.float32)
        for lo in range(0, U.size, 512):
            v = _values(xyz1[U[lo:lo + 512]], xyz2, price)
            r = np.arange(v.shape[0])
            bi = np.argmax(v, axis=1)
            best = v[r, bi]
            v[r, bi] = FLOOR
            better = np.maximum(v.max(axis=1), FLOOR)
            ties_best += int(np.count_nonzero(better == best))
            bid[lo:lo + 512] = bi
            inc[lo:lo + 512] = (best - better) + eps
        np.maximum.at(max_inc, bid, inc)
        m = max_inc[bid].astype(np.float64)
        b64 = inc.astype(np.float64)
        inside = (b64 - 1e-6 <= m) & (m <= b64 + 1e-6)
        window = int(np.count_nonzero(np.bincount(bid[inside], minlength=n) > 1))
        exact = int(np.count_nonzero(np.bincount(bid[inc == max_inc[bid]], minlength=n) > 1))
        ties_window += window
        ties_inc += exact
        if last:
            last_window, last_inc = window, exact
            if observe is not None:
                observe(it, U, bid, inc, price.copy(), np.ones(U.size, bool))
            assignment[U] = bid
            continue
        if rule == "reference":
            for j, k in zip(U[inside], bid[inside]):   # ascending j: the highest qualifying j stays
                max_idx[k] = j
            won = max_idx[bid] == U
        else:
            # sorted by object, then increment bits (inc >= 0: the bits order like the value), then j: the last bidder of
            # every object's run holds the largest (bits, j) pair
            order = np.lexsort((U, inc.view(np.uint32), bid))
            ends = np.flatnonzero(np.append(bid[order][1:] != bid[order][:-1], True))
            won = np.zeros(U.size, bool)
            won[order[ends]] = True
        if observe is not None:
            observe(it, U, bid, inc, price.copy(), won)
        for j, k, g in zip(U[won], bid[won], inc[won]):
            prev = assignment_inv[k]
            if prev != -1:
                assignment[prev] = -1
            assignment_inv[k] = j
            assignment[j] = k
            price[k] = price[k] + g
            max_inc[k] = FLOOR
    d = xyz1 - xyz2[assignment]
    dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return Result(dist.astype(np.float32), assignment, unassigned, ties_best, ties_window, ties_inc, last_window, last_inc)


@functools.lru_cache(maxsize=None)
def case(n: int, seed: int, eps: float, iters: int, family: str = "clouds", rule: str = "reference") -> Result:
    """The restatement on FAMILIES[family](n, seed), computed once per session and shared (treat as read-only)."""
    a, b = FAMILIES[family](n, seed)
    res = emd_forward(a, b, eps, iters, rule=rule)
    for arr in (res.dist, res.assignment):
        arr.setflags(write=False)
    return res


def optimum(xyz1: np.ndarray, xyz2: np.ndarray) -> float:
    """Cost of the optimal one-to-one matching under the float64 Euclidean distance."""
    from scipy.optimize import linear_sum_assignment

    a, b = np.asarray(xyz1, np.float64), np.asarray(xyz2, np.float64)
    cost = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    r, c = linear_sum_assignment(cost)
    return float(cost[r, c].sum())


# ------------------------------------------------------------------------------- the bid pass's split (csrc/emd.hip), replica
Plan = namedtuple("Plan", "T groups nspans cps nch")
BLK, CH = 256, 512


def emd_auto_target(B: int) -> int:
    return max(64, 2048 // B)


def emd_cap(B: int, n: int) -> int:
    """Triples of scratch per pair."""
    return BLK * emd_auto_target(B) + n


def emd_plan(cnt: int, n: int, tgt: int) -> Plan:
    """The split of one pair's bid pass for `cnt` bidders of `n` at `tgt` blocks per pair."""
    assert 1 <= cnt <= n and tgt >= 1
    nch = (n + CH - 1) // CH
    T = 1
    while T < 64 and ((cnt * T + BLK - 1) // BLK) * nch < tgt:
        T *= 4
    groups = (cnt * T + BLK - 1) // BLK
    ns = min(max(tgt // groups, 1), nch)
    cps = (nch + ns - 1) // ns
    return Plan(T, groups, (nch + cps - 1) // cps, cps, nch)


def splits(unassigned, n: int, B: int, target_blocks: int):
    """The set of (T, nspans) a run with this `unassigned` trajectory visits."""
    tgt = target_blocks or emd_auto_target(B)
    return {(p.T, p.nspans) for p in (emd_plan(c, n, tgt) for c in unassigned if c > 0)}
