"""The coordinate hash of csrc/spconv_hash.h restated in numpy uint64 (the key, `sp_slot`, `sp_capacity`), a checker that
reads a built table back and asserts what an open-addressing table with linear probing must satisfy, a vectorised
neighbour oracle for scenes too large for the dictionary of _spconv_oracle (pinned on it by tests/test_spconv_host.py),
and the scenes the GPU tests of the hash share (tests/test_spconv.py, tests/test_spvoxel.py).

The restatement of the slot function is pinned on the GPU by invariant (ii) of `table_invariants`: a key that does not sit
in the run of occupied slots that starts at its restated home slot fails it at once."""
import numpy as np
import torch

import _spconv_oracle as O

MAX_COORD = (1 << 18) - 1          # include/lidarcrafter_hip.h LC_SPCONV_MAX_COORD (tests/test_spconv_host.py compares)
MAX_BATCH = 510                    # LC_SPCONV_MAX_BATCH
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _np(coords):
    return coords.cpu().numpy() if isinstance(coords, torch.Tensor) else np.asarray(coords)


def sp_key(coords):
    """uint64 [N]: batch << 54 | x << 36 | y << 18 | z of rows (x, y, z, batch) inside the fields."""
    c = _np(coords).astype(np.uint64)
    return (c[:, 3] << np.uint64(54)) | (c[:, 0] << np.uint64(36)) | (c[:, 1] << np.uint64(18)) | c[:, 2]


def sp_slot(keys, cap):
    """The home slot of every key in a table of `cap` slots: the 64-bit finaliser of spconv_hash.h, low bits."""
    k = np.asarray(keys, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.int64) & (cap - 1)


def sp_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def read_table(table, n):
    """(keys uint64 [cap], values int32 [cap]) of the int64 tensor `hash_build` returns for n rows."""
    cap = sp_capacity(n)
    raw = table.cpu().numpy()
    assert raw.dtype == np.int64 and raw.size == cap + cap // 2, (raw.dtype, raw.size, cap)
    return raw[:cap].view(np.uint64), raw[cap:].view(np.int32)


def displacements(keys, cap):
    """For every occupied slot h: (h - home slot of its key) mod cap; and the slots themselves."""
    occ = np.nonzero(keys != EMPTY)[0]
    return (occ - sp_slot(keys[occ], cap)) % cap, occ


def ordered_table(coords):
    """(keys uint64 [cap], values int32 [cap]): the one arrangement of the rows' keys in which every key has only smaller
    keys between its home slot and its own (ordered hashing: where two keys meet the smaller stays, the larger moves on),
    here by inserting the distinct keys one after the other; value = the largest row of a key."""
    cap = sp_capacity(len(coords))
    k = sp_key(coords)
    last = dict(zip(k.tolist(), range(len(k))))                      # ascending rows: the largest stays
    home = dict(zip(k.tolist(), sp_slot(k, cap).tolist()))
    empty = int(EMPTY)
    keys = [empty] * cap
    for key in last:
        h, carry = home[key], key
        while keys[h] != empty:
            if keys[h] > carry:
                keys[h], carry = carry, keys[h]
            h = (h + 1) & (cap - 1)
        keys[h] = carry
    return np.array(keys, np.uint64), np.array([last.get(key, -1) for key in keys], np.int32)


def table_invariants(table, coords):
    """Reads the table of `coords` back and asserts (i) every distinct input key occurs exactly once and its value is the
    largest row that has it, (ii) for every occupied slot h holding key k all slots from sp_slot(k) cyclically up to h are
    occupied, (iii) nothing else is there: as many occupied slots as distinct keys, every other key the empty marker,
    every other value -1, and (iv) the table is `ordered_table(coords)` slot for slot: its bytes are a function of the
    rows, not of the order in which the threads arrived.  -> (keys, values, displacement of every occupied slot, the
    occupied slots)."""
    n = len(coords)
    cap = sp_capacity(n)
    keys, vals = read_table(table, n)
    want = {}
    for i, k in enumerate(sp_key(coords).tolist()):
        want[k] = i                                                  # ascending rows: the largest stays
    occ = keys != EMPTY
    got = dict(zip(keys[occ].tolist(), vals[occ].tolist()))
    assert int(occ.sum()) == len(got) == len(want), (int(occ.sum()), len(got), len(want))      # (i) once, (iii) count
    assert got == want                                                                        # (i) keys and values
    assert bool((vals[~occ] == -1).all())                                                     # (iii)
    disp, slots = displacements(keys, cap)
    # (ii): run[h] = occupied slots in a row ending at h, cyclically (two passes over the doubled table; cap = all full)
    run = np.zeros(2 * cap, np.int64)
    o2 = np.concatenate([occ, occ])
    for h in range(2 * cap):
        run[h] = (run[h - 1] + 1 if h else 1) if o2[h] else 0
    run = np.minimum(run[cap:], cap)
    bad = np.nonzero(disp + 1 > run[slots])[0]
    assert len(bad) == 0, ("a key is not reachable from its home slot", slots[bad][:8], disp[bad][:8])
    want_keys, want_vals = ordered_table(coords)                                              # (iv)
    moved = np.nonzero(keys != want_keys)[0]
    assert len(moved) == 0, ("not the ordered arrangement", moved[:8], keys[moved][:8], want_keys[moved][:8])
    assert np.array_equal(vals, want_vals)
    return keys, vals, disp, slots


# ---- a vectorised neighbour oracle --------------------------------------------------------------------------------------
def lookup_sorted(table_coords, query_coords, offs):
    """[M, K] int64: O._lookup(O._index(table_coords), query_coords, offs) by sorted packed keys and searchsorted.  A
    query with a component outside [0, MAX_COORD] is absent: no table row has one (asserted)."""
    t, q = _np(table_coords).astype(np.int64), _np(query_coords).astype(np.int64)
    assert t[:, :3].min() >= 0 and t[:, :3].max() <= MAX_COORD and t[:, 3].min() >= 0 and t[:, 3].max() <= MAX_BATCH
    tk = sp_key(t).astype(np.int64)                                  # non-negative: the batch has 9 bits
    order = np.argsort(tk, kind="stable")
    sk = tk[order]
    out = np.full((len(q), len(offs)), -1, np.int64)
    for k, off in enumerate(offs):
        p = q.copy()
        p[:, :3] += np.asarray(off, np.int64)
        ok = ((p[:, :3] >= 0) & (p[:, :3] <= MAX_COORD)).all(1) & (p[:, 3] >= 0) & (p[:, 3] <= MAX_BATCH)
        pk = sp_key(np.where(ok[:, None], p, 0)).astype(np.int64)
        at = np.searchsorted(sk, pk, side="right") - 1               # the last of equal keys: the largest row
        hit = ok & (at >= 0) & (sk[np.maximum(at, 0)] == pk)
        out[hit, k] = order[at[hit]]
    return torch.from_numpy(out)


class SortedOracle:
    """nbr_same / nbr_down / nbr_up of _spconv_oracle through `lookup_sorted`."""

    @staticmethod
    def nbr_same(coords, s):
        return lookup_sorted(coords, coords, O.offsets3(s))

    @staticmethod
    def nbr_down(fine, coarse, s):
        return lookup_sorted(fine, coarse, O.offsets2(s))

    @staticmethod
    def nbr_up(fine, coarse, s):
        return lookup_sorted(coarse, fine, [(-dx, -dy, -dz) for dx, dy, dz in O.offsets2(s)])


# ---- scenes -------------------------------------------------------------------------------------------------------------
CAPACITY_NS = (1, 511, 512, 513, 1024, 1025)
CAPACITIES = (1024, 1024, 1024, 2048, 2048, 4096)


def _shuffled(rows, seed):
    c = torch.as_tensor(np.asarray(rows, np.int64)).reshape(-1, 4)
    return c[torch.randperm(len(c), generator=torch.Generator().manual_seed(seed))]


def capacity_scene(n):
    """n unique rows drawn from three clouds' boxes of side ceil((2 n)^(1/3)): about one cell in six is taken, so most
    rows have neighbours."""
    side = int(np.ceil((2 * n) ** (1.0 / 3.0) - 1e-9))
    g = np.random.default_rng(n)
    cells = g.permutation(3 * side ** 3)[:n]
    b, r = cells // side ** 3, cells % side ** 3
    return torch.from_numpy(np.stack([r // side ** 2, r // side % side, r % side, b], 1).astype(np.int64))


CLUSTER_CAP, CLUSTER_SIDE, CLUSTER_KEYS, CLUSTER_PLAIN, CLUSTER_ABSENT = 1024, 36, 300, 100, 50


def clustered_scene():
    """(coords [400, 4] shuffled, absent [50, 4]).  From the 36^3 lattice of cloud 0 the first 300 keys whose home slot in
    a table of 1024 lies in the last 8 slots: they can only be stored by wrapping to slot 0 and on.  100 ordinary rows:
    the +x neighbours of the first 50 clustered voxels (so the scene has neighbours at all) and 50 lattice points of
    clouds 1 and 2.  `absent`: 50 lattice points of cloud 0 that are not in the scene and whose home slot is one of the
    last 8 or the first 200 -- inside the chain, so a query for one walks over foreign keys to the chain's end."""
    S = CLUSTER_SIDE
    lat = np.stack(np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij"), -1).reshape(-1, 3)
    lat = np.concatenate([lat, np.zeros((len(lat), 1), np.int64)], 1).astype(np.int64)
    home = sp_slot(sp_key(lat), CLUSTER_CAP)
    tail = np.nonzero(home >= CLUSTER_CAP - 8)[0]
    assert len(tail) >= CLUSTER_KEYS, len(tail)
    chosen = lat[tail[:CLUSTER_KEYS]]
    taken = {tuple(r) for r in chosen.tolist()}
    plain = []
    for x, y, z, b in chosen.tolist():
        if len(plain) < CLUSTER_PLAIN // 2 and (x + 1, y, z, b) not in taken:
            plain.append((x + 1, y, z, b))
            taken.add(plain[-1])
    g = np.random.default_rng(7)
    for i in g.permutation(len(lat))[:CLUSTER_PLAIN - len(plain)]:
        plain.append(tuple(lat[i, :3].tolist()) + (1 + len(plain) % 2,))
    assert len(plain) == CLUSTER_PLAIN and len(set(plain)) == CLUSTER_PLAIN
    inside = np.nonzero((home >= CLUSTER_CAP - 8) | (home < 200))[0]
    absent = [tuple(lat[i].tolist()) for i in inside if tuple(lat[i].tolist()) not in taken][-CLUSTER_ABSENT:]
    assert len(absent) == CLUSTER_ABSENT
    return _shuffled(chosen.tolist() + plain, 11), torch.tensor(absent, dtype=torch.int64)


def duplicate_scene():
    """64 coordinates of two clouds' 5^3 boxes, each 2 to 5 times, and 40 single ones, the rows shuffled."""
    g = np.random.default_rng(5)
    cells = g.permutation(2 * 125)[:104]
    rows = np.stack([cells % 125 // 25, cells % 25 // 5, cells % 5, cells // 125], 1)
    times = np.concatenate([2 + np.arange(64) % 4, np.ones(40, np.int64)])
    return _shuffled(np.repeat(rows, times, axis=0), 13)


def top_scene(s):
    """Rows at the largest coordinate (a multiple of s) of every axis, in cloud 0 and in the two last clouds the key
    takes, each with its -s neighbour; the row of the largest key of all, (top, top, top) of cloud MAX_BATCH, and the same
    place one cloud before; and where a +s step from a top row would land if it carried out of its field of the key: x
    carries into the batch -- (0, y, z) of the next cloud --, y into x + 1, z into y + 1.  Every cloud below MAX_BATCH with a
    top voxel is followed by a cloud with a voxel at the origin; no cloud follows MAX_BATCH."""
    top = MAX_COORD // s * s
    B = MAX_BATCH
    rows = []
    for b in (0, B - 1):
        rows += [(top, 0, 0, b), (top - s, 0, 0, b), (0, top, 0, b), (0, top - s, 0, b), (0, 0, top, b), (0, 0, top - s, b),
                 (top, top, top, b), (top, top, top - s, b),
                 (0, 0, 0, b + 1), (0, top, top, b + 1),              # x + s of (top, 0, 0, b) and (top, top, top, b)
                 (1, 0, 0, b), (0, 1, 0, b), (s, 0, 0, b), (0, s, 0, b), (0, 0, s, b)]
    rows += [(top, top, top, B), (top - s, top, top, B), (top, top - s, top, B), (top, 0, 0, B), (s, s, s, B), (0, 0, 0, 2)]
    rows = sorted(set(rows))
    return _shuffled(rows, 17 + s)


def sweep_scene():
    """30 000 unique rows, 15 000 in each of two clouds' 40 x 40 x 36 boxes: one cell in four."""
    g = np.random.default_rng(3)
    out = []
    for b in range(2):
        cells = g.permutation(40 * 40 * 36)[:15000]
        out.append(np.stack([cells // (40 * 36), cells // 36 % 40, cells % 36, np.full(15000, b)], 1))
    return _shuffled(np.concatenate(out), 19)
