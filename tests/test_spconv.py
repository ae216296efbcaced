"""GPU tests of the sparse 3-D convolution (csrc/spconv.hip), the MinkUNet extractor built on it and the Frechet Sparse
Volume Distance front-end, against the float64 restatement of tests/_spconv_oracle.py (itself pinned on conv3d /
conv_transpose3d by tests/test_spconv_host.py).  `pytest -m gpu`.

The coordinate hash is tested on its own: the table is read back and checked against the hash restated in numpy
(tests/_spconv_hash.py `table_invariants`) and the three neighbour tables against the oracle's dictionary, exactly, on scenes
at the capacity boundaries, with a probe chain that wraps the end of the table, with repeated rows, at the top of every
field of the key and at one sweep's size.

Tolerances: the oracle runs the same arithmetic in float32; the row-wise rel-L2 of that against float64 is measured at run
time and the kernel may be 4 x as far off (another summation order over up to 27 x 192 terms), never less than TOL_CONV."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spconv_hash as H  # noqa: E402
import _spconv_oracle as O  # noqa: E402

from lidarcrafter_amd import ops_spconv as KS  # noqa: E402
from lidarcrafter_amd.testing import seeded_randn, synth_points  # noqa: E402
from tests._profile_cases import TOL_CONV  # noqa: E402   2e-6: the project's tolerance for its fp32-accurate convolutions

pytestmark = pytest.mark.gpu
T = KS.TILE
DEPTH_RANGE = [1.0, 45.0]            # nuScenes ('32')


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _limit(ref32, ref64, what):
    base = float(O.rel_l2_rows(ref32, ref64).max())
    return max(4.0 * base, TOL_CONV), base


def _check_rows(got, ref32, ref64, what):
    limit, base = _limit(ref32, ref64, what)
    err = float(O.rel_l2_rows(got, ref64).max())
    print(f"{what}: worst row rel-L2 {err:.2e}; float32 oracle {base:.2e}; ratio {err / max(base, 1e-30):.2f}; "
          f"limit {limit:.2e}")
    assert bool(torch.isfinite(got).all()) and err < limit, (what, err, limit)


# ---- maps -----------------------------------------------------------------------------------------------------------
def _map_scene(s):
    """Coordinates at stride s (multiples of s), rows shuffled.  Cloud 0: a solid 4 x 4 x 4 block at the origin (all 27
    neighbours inside, coordinate 0 on every axis, coarse cells of 8 children), an isolated voxel (a coarse cell of one
    child), a pair along x (a cell of two) and a voxel at the largest supported x.  Clouds 1 and 2: the same coordinates
    as each other, among them (0, 0, 0) -- where the voxel of cloud 0 at the largest x would land if x + s wrapped out of
    its field of the key."""
    top = KS.MAX_COORD // s
    block = [(x, y, z) for x in range(4) for y in range(4) for z in range(4)]
    c0 = block + [(20, 21, 22), (30, 30, 30), (31, 30, 30), (top, 0, 0), (top - 1, 0, 0)]
    c12 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (5, 5, 5), (6, 5, 5), (6, 6, 6), (9, 0, 3)]
    rows = [(x * s, y * s, z * s, 0) for x, y, z in c0] + [(x * s, y * s, z * s, b) for b in (1, 2) for x, y, z in c12]
    c = torch.tensor(rows, dtype=torch.int64)
    return c[torch.randperm(len(c), generator=torch.Generator().manual_seed(s))]


@pytest.mark.parametrize("s", [1, 2, 4])
def test_maps_equal_the_oracles(dev, s):
    c = _map_scene(s)
    cd = c.to(torch.int32).to(dev)
    want_same = O.nbr_same(c, s)
    assert int((want_same >= 0).sum(1).max()) == 27 and int((want_same >= 0).sum(1).min()) == 1
    table = KS.hash_build(cd, int(c[:, :3].max()), 3)
    same = KS.kernel_map(cd, KS.KIND_SAME, s, table, len(c))
    assert torch.equal(same.cpu().long(), want_same)
    coarse = O.down_coords(c, s)
    got_coarse = KS.downsample_coords(cd, s)
    assert torch.equal(got_coarse.cpu().long(), coarse)
    want_down = O.nbr_down(c, coarse, s)
    assert sorted(set((want_down >= 0).sum(1).tolist())) == [1, 2, 4, 8]
    down = KS.kernel_map(got_coarse, KS.KIND_DOWN, s, table, len(c))
    assert torch.equal(down.cpu().long(), want_down)
    ctable = KS.hash_build(got_coarse, int(c[:, :3].max()), 3)
    up = KS.kernel_map(cd, KS.KIND_UP, s, ctable, len(coarse))
    assert torch.equal(up.cpu().long(), O.nbr_up(c, coarse, s))
    # the voxel at the largest x: its +s neighbours are absent, not cloud 1's voxel at x = 0
    i = int((c[:, 0] == (KS.MAX_COORD // s) * s).nonzero()[0])
    assert bool((same[i].cpu().reshape(3, 3, 3)[:, :, 2] == -1).all())
    lv = KS.CoordLevels(cd, 3, stride=s)
    assert torch.equal(lv.same(0), same) and torch.equal(lv.down(0), down) and torch.equal(lv.up(0), up)
    assert lv.same(0) is lv.same(0)                                  # built once


# ---- the coordinate hash: load, probing, duplicates, the top of every field ---------------------------------------------
def _check_hash_scene(dev, c, s, n_batch, oracle=O, extra=None):
    """The table of c [N, 4] int64 read back (`H.table_invariants`), and the three kinds of neighbour table exactly as the
    oracle has them -- a dictionary over the rows, never the hash.  `extra`: further query rows (not in the table) for
    the kinds that take any query.  -> what table_invariants returns, and the `same` table."""
    cd = c.to(torch.int32).to(dev)
    n = len(c)
    table = KS.hash_build(cd, int(c[:, :3].max()), n_batch)
    read = H.table_invariants(table, c)
    same = KS.kernel_map(cd, KS.KIND_SAME, s, table, n)
    assert torch.equal(same.cpu().long(), oracle.nbr_same(c, s))
    coarse = O.down_coords(c, s)
    got_coarse = KS.downsample_coords(cd, s)
    assert torch.equal(got_coarse.cpu().long(), coarse)
    down = KS.kernel_map(got_coarse, KS.KIND_DOWN, s, table, n)
    assert torch.equal(down.cpu().long(), oracle.nbr_down(c, coarse, s))
    ctable = KS.hash_build(got_coarse, int(c[:, :3].max()), n_batch)
    H.table_invariants(ctable, coarse)
    up = KS.kernel_map(cd, KS.KIND_UP, s, ctable, len(coarse))
    assert torch.equal(up.cpu().long(), oracle.nbr_up(c, coarse, s))
    if extra is not None:
        index = O._index(c)
        q = torch.cat([c, extra])
        qd = q.to(torch.int32).to(dev)
        for kind, offs in ((KS.KIND_SAME, O.offsets3(s)), (KS.KIND_DOWN, O.offsets2(s))):
            got = KS.kernel_map(qd, kind, s, table, n)
            assert torch.equal(got.cpu().long(), O._lookup(index, q, offs))
    return read, same


@pytest.mark.parametrize("n,cap", list(zip(H.CAPACITY_NS, H.CAPACITIES)))
def test_hash_at_the_capacity_boundaries(dev, n, cap):
    """N = 512 rows fill half of 1024 slots, the highest load the table takes; row 513 doubles it."""
    c = H.capacity_scene(n)
    assert H.sp_capacity(n) == cap and int(KS.hash_build(c.to(torch.int32).to(dev), 64, 3).numel()) == cap + cap // 2
    (keys, vals, disp, slots), same = _check_hash_scene(dev, c, 1, 3)
    if n >= 511:
        assert int((same >= 0).sum(1).median()) >= 3 and int(disp.max()) >= 1      # neighbours, and collisions, at all


def test_hash_clustered_chain_wraps_the_table_end(dev):
    """300 keys whose home slot is one of the last 8 of 1024: the chain wraps to slot 0 and runs on for hundreds of
    slots, through the ordinary rows' home slots.  Queries for absent coordinates whose home slot lies in the chain walk
    it to its end and find nothing."""
    c, absent = H.clustered_scene()
    (keys, vals, disp, slots), same = _check_hash_scene(dev, c, 1, 3, extra=absent)
    home = H.sp_slot(keys[slots], H.CLUSTER_CAP)
    wrapped = int((slots < home).sum())
    print(f"clustered table: {wrapped} keys below their home slot, longest displacement {int(disp.max())}")
    assert wrapped >= 250 and int(disp.max()) >= 250                  # the chain really wrapped, and is long
    assert int(((same >= 0).sum(1) >= 2).sum()) >= 80


def test_hash_duplicate_rows_the_last_wins_every_run(dev):
    """Rows that repeat: one slot per coordinate, its value the largest row (atomicMax), whichever thread came first.  The
    dictionary of the oracle has the same rule by construction: a later row overwrites an earlier one.  The table's bytes
    are the same every run: the ordered insertion leaves one arrangement (with a first-come compare-and-swap two keys
    of one home slot swapped places between runs, and this failed in one run of two on an MI355X)."""
    c = H.duplicate_scene()
    (keys, vals, disp, slots), same = _check_hash_scene(dev, c, 1, 2)
    last = {}
    for i, r in enumerate(map(tuple, c.tolist())):
        last[r] = i
    want = torch.tensor([last[tuple(r)] for r in c.tolist()])
    assert int((want != torch.arange(len(c))).sum()) >= 100           # most rows are not the last of their coordinate
    assert torch.equal(same[:, 13].cpu().long(), want)
    cd = c.to(torch.int32).to(dev)
    first = KS.hash_build(cd, 4, 2).cpu()
    for _ in range(3):
        assert torch.equal(KS.hash_build(cd, 4, 2).cpu(), first)      # the same table bytes every run


@pytest.mark.parametrize("s", [1, 4])
def test_hash_at_the_top_of_every_field(dev, s):
    """The largest coordinate on every axis, the largest batch, and the largest key of all.  A +s step from a top voxel
    is absent: not the voxel the sum would name if it carried into the next field of the key (H.top_scene puts one
    there: the origin of the next cloud behind x, x + 1 behind y, y + 1 behind z).  No cloud follows MAX_BATCH."""
    c = H.top_scene(s)
    top = KS.MAX_COORD // s * s
    (keys, vals, disp, slots), same = _check_hash_scene(dev, c, s, KS.MAX_BATCH + 1)
    big = int(H.sp_key(torch.tensor([[top, top, top, KS.MAX_BATCH]]))[0])
    assert big in keys.tolist() and int(keys[keys != H.EMPTY].max()) == big and big >> 62 == 1
    cube = same.cpu().reshape(len(c), 3, 3, 3)                       # [row, iz, iy, ix]
    want = O.nbr_same(c, s).reshape(len(c), 3, 3, 3)
    n_top = 0
    for axis, plane in ((0, (slice(None), slice(None), 2)), (1, (slice(None), 2)), (2, (2,))):
        at = (c[:, axis] == top).nonzero()[:, 0]
        n_top += len(at)
        for i in at.tolist():
            assert bool((cube[i][plane] == -1).all()) and bool((want[i][plane] == -1).all())
            assert int(cube[i, 1, 1, 1]) == i
    assert n_top >= 15
    assert int((same >= 0).sum()) > len(c) + 10                      # the -s neighbours of the top voxels are found


def test_hash_one_sweep(dev):
    """30 000 rows in 65 536 slots.  The oracle is H.SortedOracle (tests/test_spconv_host.py pins it on the dictionary)."""
    c = H.sweep_scene()
    want = H.SortedOracle.nbr_same(c, 1)
    assert int((want >= 0).sum(1).median()) >= 6                     # of 27, itself included
    (keys, vals, disp, slots), same = _check_hash_scene(dev, c, 1, 2, oracle=H.SortedOracle)
    assert len(keys) == 65536 and int(disp.max()) >= 4
    print(f"one sweep: longest displacement {int(disp.max())}, mean {float(disp.mean()):.2f}")


# ---- the convolution kernel -------------------------------------------------------------------------------------------
def _conv_weights(K, Ci, Co, seed):
    """Mixed signs, output columns of very different scale (as tests/test_pointnet.py draws W3)."""
    w = seeded_randn(K, Ci, Co, seed=seed) / (0.4 * K * Ci) ** 0.5 * torch.exp(seeded_randn(1, 1, Co, seed=seed + 1))
    return w.contiguous(), (0.3 * seeded_randn(Co, seed=seed + 2)).contiguous()


def _conv_table(M, n_in, K, transposed, seed):
    g = torch.Generator().manual_seed(seed)
    if K == 1:
        return None
    nbr = torch.randint(0, n_in, (M, K), generator=g)
    if transposed:
        keep = torch.zeros((M, K), dtype=torch.bool)
        keep[torch.arange(M), torch.randint(0, K, (M,), generator=g)] = True
    else:
        keep = torch.rand((M, K), generator=g) < 0.4
    return torch.where(keep, nbr, torch.full_like(nbr, -1))


CONV_CASES_EVERY_M = [(4, 16, 27, False), (16, 16, 27, False), (16, 32, 1, False), (192, 128, 27, False),
                      (64, 48, 27, False), (48, 48, 8, False), (128, 128, 8, True)]
# the other (Ci, Co, K) of the MinkUNet and the SPVCNN of O.CONFIG, at M = 1 and T + 1 (tests/test_spconv_host.py asserts
# that CONV_CASES has every one): Co = 64 is an instance of the kernel of its own, Ci = 96 is staged as 64 + 32
CONV_CASES_USED = [(16, 32, 27, False), (32, 32, 27, False), (32, 64, 27, False), (48, 48, 27, False), (64, 64, 27, False),
                   (64, 128, 27, False), (96, 64, 27, False), (128, 128, 27, False),
                   (16, 16, 8, False), (32, 32, 8, False), (64, 64, 8, False), (128, 128, 8, False),
                   (128, 64, 8, True), (64, 48, 8, True), (48, 48, 8, True),
                   (32, 64, 1, False), (64, 128, 1, False), (64, 48, 1, False), (96, 64, 1, False), (192, 128, 1, False)]
CONV_CASES = CONV_CASES_EVERY_M + CONV_CASES_USED


@pytest.mark.parametrize("M", [1, T + 1])
@pytest.mark.parametrize("Ci,Co,K,transposed", CONV_CASES_USED)
def test_conv_vs_float64_every_width_in_use(dev, Ci, Co, K, transposed, M):
    test_conv_vs_float64(dev, Ci, Co, K, transposed, M)


@pytest.mark.parametrize("M", [1, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("Ci,Co,K,transposed", CONV_CASES_EVERY_M)
def test_conv_vs_float64(dev, Ci, Co, K, transposed, M):
    n_in = M if K == 1 else M + 5
    x = seeded_randn(n_in, Ci, seed=3 * M + Ci)
    w, b = _conv_weights(K, Ci, Co, 10 * Ci + Co + K)
    nbr = _conv_table(M, n_in, K, transposed, M + K)
    res = seeded_randn(M, Co, seed=M + Co)
    xd, wd, bd, resd = x.to(dev), w.to(dev), b.to(dev), res.to(dev)
    nd = None if nbr is None else nbr.to(torch.int32).to(dev)
    col, wide = 16, Co + 16 + 12
    for with_res in (False, True):
        for relu in (False, True):
            r = res if with_res else None
            ref64 = O.conv(x.double(), nbr, w.double(), b.double(), None if r is None else r.double(), relu)
            ref32 = O.conv(x, nbr, w, b, r, relu)
            out = torch.full((M, wide), -7.25, device=dev)
            y = KS.sparse_conv(xd, nd, wd, bd, residual=resd if with_res else None, relu=relu, out=out, out_col=col)
            torch.cuda.synchronize()
            assert y is out
            assert bool((out[:, :col] == -7.25).all()) and bool((out[:, col + Co:] == -7.25).all())
            _check_rows(out[:, col:col + Co], ref32, ref64, f"conv Ci={Ci} Co={Co} K={K} M={M} res={with_res} relu={relu}")
    # strided operands: x and the residual as column slices of wider buffers, no bias
    xw = torch.full((n_in, Ci + 8), float("nan"), device=dev)
    xw[:, 4:4 + Ci] = xd
    rw = torch.full((M, Co + 4), float("nan"), device=dev)
    rw[:, 4:] = resd
    y = KS.sparse_conv(xw[:, 4:4 + Ci], nd, wd, None, residual=rw[:, 4:], relu=True)
    _check_rows(y, O.conv(x, nbr, w, None, res, True), O.conv(x.double(), nbr, w.double(), None, res.double(), True),
                f"conv Ci={Ci} Co={Co} K={K} M={M} strided operands")


def test_centre_only_table_is_the_dense_product(dev):
    """A table of -1 except the centre column equals the K = 1 product with the centre weight bit for bit, and the NaN
    rows 0 and n - 1 of x, which no entry names, never reach the output (-1 is not row 0, nor the last row)."""
    M, n_in, Ci, Co = 2 * T + 3, 2 * T + 9, 64, 48
    x = seeded_randn(n_in, Ci, seed=1)
    x[0] = float("nan")
    x[-1] = float("nan")
    w, b = _conv_weights(27, Ci, Co, 2)
    idx = torch.randint(1, n_in - 1, (M,), generator=torch.Generator().manual_seed(3))
    nbr = torch.full((M, 27), -1, dtype=torch.int64)
    nbr[:, 13] = idx
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    y27 = KS.sparse_conv(xd, nbr.to(torch.int32).to(dev), wd, bd, relu=False)
    y1 = KS.sparse_conv(xd[idx.to(dev)].contiguous(), None, wd[13:14].contiguous(), bd, relu=False)
    y1t = KS.sparse_conv(xd, idx.to(torch.int32).to(dev)[:, None].contiguous(), wd[13:14].contiguous(), bd, relu=False)
    assert bool(torch.isfinite(y27).all())
    assert torch.equal(y27, y1) and torch.equal(y27, y1t)
    _check_rows(y27, O.conv(x[idx], None, w[13:14], b), O.conv(x[idx].double(), None, w[13:14].double(), b.double()),
                "centre-only table")
    # an entry outside [0, n_in) is absent too
    bad = nbr.clone()
    bad[0, 0], bad[1, 26] = n_in, -5
    assert torch.equal(KS.sparse_conv(xd, bad.to(torch.int32).to(dev), wd, bd), y27)


def _structured_table(n_in, seed):
    """[2 T + 3, 27]: which offsets a row has is decided by its wave and tile, so that the kernel's skipping of an offset
    no row of the block has, and of one no row of the WAVE has while another wave has it, is at work in every tile.
    Tile 0: wave w has only offsets with k % 4 == w.  Tile 1: offsets 0 .. 12 in its first 16 rows only, no offset at all
    in the next 16, the centre alone in the third 16, nothing but k = 26 in the last 16.  The ragged tile 2: one row with
    all 27 offsets, two with none."""
    g = torch.Generator().manual_seed(seed)
    M = 2 * T + 3
    keep = torch.zeros((M, 27), dtype=torch.bool)
    k = torch.arange(27)
    for wv in range(4):
        rows = slice(16 * wv, 16 * wv + 16)
        keep[rows] = (torch.rand((16, 27), generator=g) < 0.6) & (k % 4 == wv)
        keep[16 * wv] = k % 4 == wv                                   # one row of the wave has all of them
    keep[T:T + 16] = (torch.rand((16, 27), generator=g) < 0.7) & (k <= 12)
    keep[T] = k <= 12
    keep[T + 32:T + 48, 13] = True
    keep[T + 48:2 * T, 26] = True
    keep[2 * T] = True
    nbr = torch.randint(0, n_in, (M, 27), generator=g)
    return torch.where(keep, nbr, torch.full_like(nbr, -1)), keep


def test_structured_table_skipping_and_row_independence(dev):
    M, Ci, Co, K = 2 * T + 3, 96, 64, 27
    n_in = M + 5
    nbr, keep = _structured_table(n_in, 5)
    for wv in range(4):                                               # the table is what it says
        has = keep[16 * wv:16 * wv + 16].any(0)
        assert has.tolist() == [k % 4 == wv for k in range(27)]
    assert keep[T:T + 16].any(0).tolist() == [k <= 12 for k in range(27)] and not bool(keep[T + 16:T + 32].any())
    assert not bool(keep[T + 16:2 * T, :13].any()) and keep[T + 48:2 * T].sum(0).tolist() == [0] * 26 + [16]
    assert bool(keep[2 * T].all()) and not bool(keep[2 * T + 1:].any())
    x = seeded_randn(n_in, Ci, seed=41)
    w, b = _conv_weights(K, Ci, Co, 42)
    res = seeded_randn(M, Co, seed=43)
    xd, wd, bd, resd, nd = x.to(dev), w.to(dev), b.to(dev), res.to(dev), nbr.to(torch.int32).to(dev)
    # every wave of tile 0, two rows of tile 1, the row with all 27 offsets, a row with none
    chosen = [0, 16, 37, 48, T + 5, 2 * T - 1, 2 * T, 2 * T + 1]
    for with_res, relu in ((False, False), (True, True), (True, False)):
        r = res if with_res else None
        rd = resd if with_res else None
        ref64 = O.conv(x.double(), nbr, w.double(), b.double(), None if r is None else r.double(), relu)
        ref32 = O.conv(x, nbr, w, b, r, relu)
        y = KS.sparse_conv(xd, nd, wd, bd, residual=rd, relu=relu)
        _check_rows(y, ref32, ref64, f"structured table res={with_res} relu={relu}")
        # rows without any offset: exactly act(b + res), nothing of x
        plain = b[None].expand(M, Co) if r is None else b[None] + r
        plain = torch.relu(plain) if relu else plain
        empty = (~keep.any(1)).nonzero()[:, 0]
        assert len(empty) == 18 and torch.equal(y.cpu()[empty], plain[empty])
        # a row's bits depend on its own neighbours only: alone in a call of one row, the same bits
        for j in chosen:
            alone = KS.sparse_conv(xd, nd[j:j + 1], wd, bd, residual=None if rd is None else rd[j:j + 1], relu=relu)
            assert torch.equal(alone[0], y[j]), (j, with_res, relu)


# ---- the network ------------------------------------------------------------------------------------------------------
def _cloud(seed, n=2000, lo=1.0, hi=3.2, scale=0.25):
    """About 1 500 voxels: a shell of a synthetic sweep, shrunk so that voxels have neighbours."""
    p = synth_points(20000, seed)[:, :3]
    d = np.linalg.norm(p, axis=1)
    return (p[(d > lo) & (d < hi)][:n] * np.float32(scale)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _state(seed):
    from lidargen.metrics.models.minkowskinet.model import Model

    return O.seeded_state(Model(O.CONFIG), seed)


def _model(dev, seed):
    from lidargen.metrics.models.minkowskinet.model import Model

    m = Model(O.CONFIG)
    m.load_state_dict(_state(seed))
    return m.eval().to(dev)


@functools.lru_cache(maxsize=None)
def _net_case(weights_seed, cloud_seeds):
    """(feats, coords, logits float32 mode, logits float64) of the oracle, computed once."""
    feats, coords = O.collate([O.pcd2voxel(_cloud(s)) for s in cloud_seeds])
    sd = _state(weights_seed)
    return feats, coords, O.network(sd, feats, coords, torch.float32), O.network(sd, feats, coords, torch.float64)


def test_network_vs_float64(dev):
    feats, coords, ref32, ref64 = _net_case(1, (11, 12))
    assert 2400 < len(coords) < 4000
    m = _model(dev, 1)
    out = m(feats.to(dev), coords.to(torch.int32).to(dev))
    assert out["logits"].shape == (len(coords), 48) and out["logits"].dtype == torch.float32
    assert torch.equal(out["coords"].cpu().long(), coords[:, :3]) and torch.equal(out["batch_indices"].cpu().long(), coords[:, 3])
    assert float(ref64.abs().max()) > 1e-3 and float((ref64 == 0).double().mean()) < 0.9     # a live output
    _check_rows(out["logits"], ref32, ref64, "MinkUNet logits")
    deep = m(feats.to(dev), coords.to(torch.int32).to(dev), return_logits=True)
    lv = O.levels(coords)
    assert deep["logits"].shape == (len(lv[4]), 128) and torch.equal(deep["batch_indices"].cpu().long(), lv[4][:, 3])


def test_batch_independence_through_the_network(dev):
    """Cloud A alone and as the middle one of three: the same bits in every row, twice."""
    m = _model(dev, 1)
    items = [O.pcd2voxel(_cloud(s)) for s in (21, 11, 22)]
    fa, ca = O.collate(items[1:2])
    f3, c3 = O.collate(items)
    ya = m(fa.to(dev), ca.to(torch.int32).to(dev))["logits"]
    y3 = m(f3.to(dev), c3.to(torch.int32).to(dev))["logits"]
    lo = len(items[0][1])
    assert torch.equal(y3[lo:lo + len(ca)], ya)
    assert torch.equal(m(f3.to(dev), c3.to(torch.int32).to(dev))["logits"], y3)


def test_call_sequence_maps_and_weights_belong_to_their_call(dev):
    """A second cloud with the SAME number of voxels at other places must get its own maps; load_state_dict and an
    in-place edit of a BatchNorm buffer between calls fold again; nothing of an earlier call stays."""
    feats, coords, ref32, ref64 = _net_case(1, (11,))
    mirrored = coords.clone()
    mirrored[:, 0] = coords[:, 0].max() - coords[:, 0]               # the same count, other neighbours
    sd = _state(1)
    m = _model(dev, 1)
    run = lambda c: m(feats.to(dev), c.to(torch.int32).to(dev))["logits"]
    first = run(coords)
    _check_rows(first, ref32, ref64, "first cloud")
    r32, r64 = O.network(sd, feats, mirrored, torch.float32), O.network(sd, feats, mirrored, torch.float64)
    assert float(O.rel_l2_rows(r64, ref64).median()) > 1e-3           # the other places are visible at all
    _check_rows(run(mirrored), r32, r64, "same voxel count, other coordinates")
    m.load_state_dict(_state(2))
    _, _, s32, s64 = _net_case(2, (11,))
    _check_rows(run(coords), s32, s64, "after load_state_dict")
    with torch.no_grad():
        m.up4[1][1].net[4].running_var.mul_(1.7)
        m.stem[1].running_mean.add_(0.2)
    sd2 = dict(_state(2))
    sd2["up4.1.1.net.4.running_var"] = sd2["up4.1.1.net.4.running_var"] * 1.7
    sd2["stem.1.running_mean"] = sd2["stem.1.running_mean"] + 0.2
    e32, e64 = O.network(sd2, feats, coords, torch.float32), O.network(sd2, feats, coords, torch.float64)
    assert float(O.rel_l2_rows(e64, s64).median()) > 1e-3
    _check_rows(run(coords), e32, e64, "after in-place edits")
    m.load_state_dict(_state(1))
    assert torch.equal(run(coords), first)


# ---- aggregation, compute_logits, compute_fsvd ------------------------------------------------------------------------
def _metre_cloud(seed, n=600, hi=14.0):
    """A sweep cropped to 14 m: nothing beyond, so its far depth sectors are empty."""
    p = synth_points(8000, seed)[:, :3]
    d = np.linalg.norm(p, axis=1)
    return p[(d > 1.0) & (d < hi)][:n]


def _oracle_features(sd, clouds, dtype):
    items = [O.pcd2voxel(O.preprocess_pcd(c, DEPTH_RANGE)) for c in clouds]
    feats, coords = O.collate(items)
    return O.sector_means(O.network(sd, feats, coords, dtype), coords, DEPTH_RANGE, len(clouds))


def test_pcd2voxel_on_the_device_equals_the_host_route(dev):
    from lidargen.metrics import metric_utils as MU

    p = _metre_cloud(5, n=3000)
    p[7] = p[2] + np.float32(0.003)
    host = MU.pcd2voxel(p)["lidar"]
    on_dev = MU.pcd2voxel(torch.from_numpy(p).to(dev))["lidar"]
    assert on_dev.F.is_cuda and torch.equal(on_dev.F.cpu(), host.F) and torch.equal(on_dev.C.cpu(), host.C)


def test_sector_means_and_compute_logits(dev):
    from lidargen.metrics import metric_utils as MU

    clouds = [_metre_cloud(31), _metre_cloud(32, n=450), _metre_cloud(33, hi=40.0)]
    sd = _state(1)
    ref32, ref64 = _oracle_features(sd, clouds, torch.float32), _oracle_features(sd, clouds, torch.float64)
    (got,) = MU.compute_logits("32", "voxel", clouds, model=_model(dev, 1))
    assert got.shape == (3, 16 * 48) and got.dtype == np.float32
    got = torch.from_numpy(got)
    empty = ref64.reshape(3, 16, 48).abs().sum(2) == 0
    assert bool(empty[0, 6:].all()) and not bool(empty[0, :3].any()) and not bool(empty[2, :12].any())
    assert bool((got.reshape(3, 16, 48)[empty] == 0).all())          # an empty sector is exact zeros
    _check_rows(got, ref32, ref64, "depth-sector features")
    # the kernel alone, on oracle logits: every row lands in the oracle's sector
    items = [O.pcd2voxel(O.preprocess_pcd(c, DEPTH_RANGE)) for c in clouds]
    feats, coords = O.collate(items)
    logits = seeded_randn(len(coords), 48, seed=9)
    offsets = torch.tensor([0] + [len(c) for _, c in items]).cumsum(0).to(torch.int32)
    agg = KS.sector_means(logits.to(dev), coords.to(torch.int32).to(dev), offsets.to(dev),
                          MU.sector_edges(DEPTH_RANGE).to(dev), 0.05)
    _check_rows(agg, O.sector_means(logits, coords, DEPTH_RANGE), O.sector_means(logits.double(), coords, DEPTH_RANGE),
                "sector means of given rows")
    assert torch.equal(agg, KS.sector_means(logits.to(dev), coords.to(torch.int32).to(dev), offsets.to(dev),
                                            MU.sector_edges(DEPTH_RANGE).to(dev), 0.05))


def test_compute_fsvd_vs_float64_features(dev, capsys):
    from lidargen.metrics import OUTPUT_TEMPLATE, eval_utils

    real = [_metre_cloud(40 + i, n=300) for i in range(6)]
    fake = [_metre_cloud(60 + i, n=300) * np.float32(0.8) for i in range(6)]
    sd = _state(1)
    f64 = [_oracle_features(sd, s, torch.float64).numpy() for s in (real, fake)]
    f32 = [_oracle_features(sd, s, torch.float32).numpy() for s in (real, fake)]
    want, want32 = O.compute_fd(*f64), O.compute_fd(*f32)
    limit = 4.0 * abs(want32 - want) / abs(want)
    m = _model(dev, 1)
    score = eval_utils.compute_fsvd(real, fake, "32", model=m)
    out = capsys.readouterr().out
    rel = abs(score - want) / abs(want)
    print(f"FSVD {score!r} against {want!r}: relative {rel:.2e}; float32 oracle {limit / 4:.2e}; limit {limit:.2e}")
    assert "Evaluating (FSVD) ..." in out and OUTPUT_TEMPLATE.format("FSVD", score) in out
    assert rel < limit
    same = eval_utils.compute_fsvd(real, real, "32", model=m)
    assert abs(same) < 1e-6 * float(np.trace(np.cov(f64[0], rowvar=False)))
