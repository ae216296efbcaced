"""GPU tests of lidargen.ops.iou3d_nms (csrc/iou3d_nms.hip): the three pairwise modes bit for bit on
axis-aligned quarter-grid boxes and within the float32 restatement's own error of the float64 restatement on rotated ones,
the 3-D epilogue against the reference's torch expressions bit for bit, the NMS mask and the device-side greedy walk on
constructions whose answer is known, on hand-built masks and against the float64 restatement's IoU."""
import numpy as np
import pytest
import torch

import _iou3d_oracle as O

pytestmark = pytest.mark.gpu

NMS_SEED = 2         # chosen on the CPU: no float64 IoU of these boxes lies within 1e-4 of 0.1 or of 0.7 (asserted below)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host_overlap(a, b):
    """overlap [N,M] of lc_boxes_overlap_bev_host: csrc/iou3d_box.h on the CPU."""
    from lidarcrafter_amd import _lib

    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    out = np.zeros((a.shape[0], b.shape[0]), np.float32)
    assert _lib.lib().lc_boxes_overlap_bev_host(a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], out.ctypes.data,
                                                None) == 0
    return out


def _U():
    from lidargen.ops.iou3d_nms import iou3d_nms_utils

    return iou3d_nms_utils


def _K():
    from lidarcrafter_amd import ops

    return ops


@pytest.fixture(scope="module")
def yardstick():
    """The float32 restatement's largest deviation from the float64 restatement over the 3000 pairs of the host test."""
    rng = np.random.default_rng(0)
    a, b = O.general_boxes(rng, 3000), O.general_boxes(rng, 3000)
    s32, c32 = O.box_overlap(a, b, np.float32)
    s64, c64 = O.box_overlap(a, b, np.float64)
    yard = float(np.abs(s32.astype(np.float64) - s64)[c32 == c64].max())
    assert 0 < yard < 1e-4
    return yard


def clustered_boxes(seed, n=200):
    rng = np.random.default_rng(seed)
    hubs = rng.uniform(-20, 20, (10, 2))
    centres = hubs[rng.integers(0, 10, n)] + rng.normal(0, 1.0, (n, 2))
    return O.general_boxes(rng, n, centres=centres), rng.permutation(n).astype(np.float32) / n


@pytest.fixture(scope="module")
def nms_case():
    boxes, scores = clustered_boxes(NMS_SEED)
    pa, pb = O.all_pairs(boxes, boxes)
    n = boxes.shape[0]
    return boxes, scores, O.iou_bev(pa, pb, np.float64).reshape(n, n), O.iou_normal(pa, pb, np.float64).reshape(n, n)


# ---------------------------------------------------------------------------------------------- pairwise modes
def _iou3d_f32(a, b, s):
    """The epilogue in numpy float32 (exact on the quarter grid up to the final, correctly rounded, division)."""
    f = np.float32
    h = np.maximum(np.minimum(a[:, 2] + a[:, 5] / 2, b[:, 2] + b[:, 5] / 2) -
                   np.maximum(a[:, 2] - a[:, 5] / 2, b[:, 2] - b[:, 5] / 2), f(0))
    o3 = s * h
    return o3 / np.maximum(a[:, 3] * a[:, 4] * a[:, 5] + b[:, 3] * b[:, 4] * b[:, 5] - o3, f(1e-6))


def test_axis_aligned_quarter_grid_is_exact_in_all_three_modes():
    K = _K()
    rng = np.random.default_rng(1)
    named = list(O.NAMED_EXACT.values())
    a = np.concatenate([O.exact_boxes(rng, 24), np.array([c[0] for c in named], np.float32)])
    b = np.concatenate([O.exact_boxes(rng, 21), np.array([c[1] for c in named], np.float32)])
    pa, pb = O.all_pairs(a, b)
    s, iou = O.rect_overlap_f32(pa, pb)
    shape = (a.shape[0], b.shape[0])
    got_s = K.boxes_overlap_bev(_dev(a), _dev(b)).cpu().numpy()
    got_i = K.boxes_iou_bev(_dev(a), _dev(b)).cpu().numpy()
    got_3 = K.boxes_iou3d(_dev(a), _dev(b)).cpu().numpy()
    assert np.array_equal(_bits(got_s), _bits(s.reshape(shape)))
    assert np.array_equal(_bits(got_i), _bits(iou.reshape(shape)))
    assert np.array_equal(_bits(got_3), _bits(_iou3d_f32(pa, pb, s).reshape(shape)))
    for k, (_, _, overlap, value) in enumerate(named):
        assert got_s[24 + k, 21 + k] == overlap and got_i[24 + k, 21 + k] == value


@pytest.mark.parametrize("N,M", [(1, 1), (17, 33), (64, 65)])
def test_rotated_pairs_within_the_restatements_own_error(yardstick, N, M):
    """|device - float64 restatement| <= 4 x yardstick on the pairs where the float32 and float64 restatements find the same
    number of points (at most 1 % may differ), the host entry and the device within the same bound of each other, and a
    non-contiguous input gives the bits of its contiguous copy."""
    K, U = _K(), _U()
    rng = np.random.default_rng(100 + N)
    a, b = O.general_boxes(rng, N), O.general_boxes(rng, M)
    if N == 1:
        b[0, :2] = a[0, :2] + np.float32(0.3)          # the one pair overlaps
    pa, pb = O.all_pairs(a, b)
    s32, c32 = O.box_overlap(pa, pb, np.float32)
    s64, c64 = O.box_overlap(pa, pb, np.float64)
    same = (c32 == c64).reshape(N, M)
    assert (~same).mean() <= 0.01
    s64 = s64.reshape(N, M)
    ta, tb = _dev(a), _dev(b)
    got = K.boxes_overlap_bev(ta, tb).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - s64)[same].max())
    print(f"{N}x{M}: yardstick {yardstick:.3e}, device overlap error {err:.3e}, non-empty {(s64 > 0).sum()}")
    assert (s64 > 0).any()
    assert err <= 4 * yardstick
    host = _host_overlap(a, b).astype(np.float64)
    assert float(np.abs(got - host)[same].max()) <= 4 * yardstick
    # the IoU is the header's expression over that overlap, each operation rounded on its own: the same bits from numpy
    got_i = U.boxes_iou_bev(ta, tb)
    assert got_i.shape == (N, M) and got_i.is_cuda
    s = got.astype(np.float32)
    union = (pa[:, 3] * pa[:, 4] + pb[:, 3] * pb[:, 4]).reshape(N, M) - s
    assert np.array_equal(_bits(got_i.cpu().numpy()), _bits(s / np.maximum(union, np.float32(1e-8))))
    wide_a = torch.zeros((N, 9), device="cuda")
    wide_a[:, 1:8] = ta
    wide_b = torch.zeros((7, M), device="cuda")
    wide_b[:] = tb.t()
    va, vb = wide_a[:, 1:8], wide_b.t()
    assert (not va.is_contiguous() or N == 1) and (not vb.is_contiguous() or M == 1)
    assert torch.equal(U.boxes_iou_bev(va, vb).view(torch.int32), got_i.view(torch.int32))
    assert torch.equal(U.boxes_iou3d_gpu(va, vb).view(torch.int32), U.boxes_iou3d_gpu(ta, tb).view(torch.int32))


# ---------------------------------------------------------------------------------------------- 3-D epilogue
def _torch_iou3d(a, b, overlaps_bev, aligned):
    """The reference's torch lines over a given BEV overlap."""
    def col(t):
        return t.view(-1, 1)

    row = col if aligned else (lambda t: t.view(1, -1))          # how b's per-box values meet a's
    roof = torch.min(col(a[:, 2] + a[:, 5] / 2), row(b[:, 2] + b[:, 5] / 2))
    floor = torch.max(col(a[:, 2] - a[:, 5] / 2), row(b[:, 2] - b[:, 5] / 2))
    shared = overlaps_bev * torch.clamp(roof - floor, min=0)
    volumes = col(a[:, 3] * a[:, 4] * a[:, 5]) + row(b[:, 3] * b[:, 4] * b[:, 5])
    return shared / torch.clamp(volumes - shared, min=1e-6)


def test_epilogue_equals_the_torch_expressions_bit_for_bit():
    K, U = _K(), _U()
    rng = np.random.default_rng(7)
    hubs = rng.uniform(-3, 3, (70, 2))
    a, b = O.general_boxes(rng, 70, centres=hubs + rng.normal(0, 0.5, (70, 2))), O.general_boxes(rng, 70, centres=hubs)
    a[:6, 2] += 5.0                        # disjoint heights
    a[6:9, 5] = 0.0                        # zero volumes: flat boxes ...
    b[6:8, 5] = 0.0
    b[8, 3:6] = 0.0                        # ... and a point
    a[9, 2], a[9, 5], b[9, 2], b[9, 5] = 0.0, 1.0, 1.0, 1.0      # touching in height
    ta, tb = _dev(a), _dev(b[:65])
    bev = K.boxes_overlap_bev(ta, tb)
    assert (bev > 0).sum() > 65
    want = _torch_iou3d(ta, tb, bev, aligned=False)
    got = U.boxes_iou3d_gpu(ta, tb)
    assert got.shape == (70, 65) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (want[:6] == 0).all() and (want[6:9] == 0).all() and (want > 0).sum() > 30
    tb = _dev(b)
    diag = K.boxes_aligned_iou3d(ta, tb, overlap_only=True)
    assert torch.equal(diag.view(torch.int32), K.boxes_overlap_bev(ta, tb).diagonal().contiguous().view(torch.int32))
    assert (diag > 0).sum() > 40
    want = _torch_iou3d(ta, tb, diag.view(-1, 1), aligned=True)
    got_a, got_p = U.boxes_aligned_iou3d_gpu(ta, tb), U.paired_boxes_iou3d_gpu(ta, tb)
    assert got_a.shape == (70, 1) and got_p.shape == (70,)
    assert torch.equal(got_a.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got_p.view(torch.int32), want.view(-1).view(torch.int32))


# ---------------------------------------------------------------------------------------------- NMS by construction
def _row_of_boxes(n):
    """Heading-0 boxes of 2 x 1 at x = i: neighbours overlap with IoU exactly 1/3, boxes two apart only touch."""
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, 0] = np.arange(n)
    boxes[:, 3:6] = (2.0, 1.0, 1.0)
    return boxes


@pytest.mark.parametrize("normal", [False, True], ids=["rotated", "normal"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 200])
def test_nms_row_keeps_the_even_ranks(n, normal):
    U = _U()
    fn = U.nms_normal_gpu if normal else U.nms_gpu
    boxes = _dev(_row_of_boxes(n))
    scores = torch.arange(n, 0, -1, device="cuda", dtype=torch.float32)
    keep, second = fn(boxes, scores, 0.25)
    assert second is None and keep.dtype == torch.int64 and keep.is_cuda and keep.is_contiguous()
    assert keep.tolist() == list(range(0, n, 2))


def test_nms_row_with_permuted_scores_and_pre_maxsize():
    U = _U()
    n = 200
    perm = np.random.default_rng(5).permutation(n)
    boxes = _row_of_boxes(n)
    scores = np.empty(n, np.float32)
    scores[perm] = np.arange(n, 0, -1)              # box perm[r] has rank r; the boxes sit at x = their RANK
    placed = np.empty_like(boxes)
    placed[perm] = boxes
    keep, _ = U.nms_gpu(_dev(placed), _dev(scores), 0.25)
    assert keep.tolist() == perm[0:n:2].tolist()       # original indices, descending score
    keep, _ = U.nms_gpu(_dev(placed), _dev(scores), 0.25, pre_maxsize=70)
    assert keep.tolist() == perm[0:70:2].tolist()
    keep, _ = U.nms_normal_gpu(_dev(placed), _dev(scores), 0.25)
    assert keep.tolist() == perm[0:n:2].tolist()


def test_nms_chain_across_words():
    """Box 70 is suppressed by box 3 (two words earlier); box 130 overlaps only box 70, which is gone: 130 is kept."""
    U = _U()
    n = 140
    boxes = _row_of_boxes(n)
    boxes[:, 0] *= 10                       # everything apart ...
    boxes[70, 0] = boxes[3, 0] + 1          # ... but 70 on 3 (IoU 1/3)
    boxes[130, 0] = boxes[70, 0] + 1        # and 130 on 70, touching 3 (IoU 0)
    scores = torch.arange(n, 0, -1, device="cuda", dtype=torch.float32)
    keep, _ = U.nms_gpu(_dev(boxes), scores, 0.25)
    assert keep.tolist() == [i for i in range(n) if i != 70]
    mask = _K().nms_mask(_dev(boxes), 0.25).cpu().numpy().view(np.uint64)
    assert mask.shape == (140, 3) and mask[3, 1] == 1 << 6 and mask[70, 2] == 1 << 2 and mask[3, 2] == 0
    assert np.count_nonzero(mask) == 2


def _pack(bits):
    n = bits.shape[0]
    words = (n + 63) // 64
    padded = np.zeros((n, words * 64), np.uint64)
    padded[:, :n] = bits
    return (padded.reshape(n, words, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


@pytest.mark.parametrize("n,p", [(1, 0.5), (64, 0.05), (65, 0.5), (200, 0.01), (200, 0.2), (333, 0.004)])
def test_select_walks_hand_built_masks(n, p):
    """The device-side walk over random suppression matrices equals the sequential walk; the words left of the diagonal
    are filled with ones to show that they are not read."""
    K = _K()
    rng = np.random.default_rng(n)
    bits = np.triu(rng.random((n, n)) < p, 1)
    words = _pack(bits)
    for r in range(n):
        words[r, :r // 64] = np.uint64(0xFFFFFFFFFFFFFFFF)
    keep = K.nms_select(_dev(words.view(np.int64)))
    want = O.greedy_keep_mask(bits)
    assert keep.dtype == torch.int64 and keep.tolist() == want
    assert 0 < len(want) <= n


def test_mask_bits_equal_the_threshold_test(nms_case):
    K = _K()
    boxes, _, iou64, _ = nms_case
    mask = K.nms_mask(_dev(boxes), 0.1).cpu().numpy().view(np.uint64)
    assert np.array_equal(mask, _pack(np.triu(iou64 > 0.1, 1)))


# ---------------------------------------------------------------------------------------------- NMS, rotated boxes
@pytest.mark.parametrize("thresh", [0.1, 0.7])
def test_nms_random_rotated_boxes(nms_case, thresh):
    U = _U()
    boxes, scores, iou64, normal64 = nms_case
    order = np.argsort(-scores, kind="stable")
    for fn, iou in ((U.nms_gpu, iou64), (U.nms_normal_gpu, normal64)):
        assert np.abs(iou - thresh).min() > 1e-4              # no decision hangs on a rounding
        want = order[O.greedy_keep(iou[order][:, order], thresh)]
        keep, _ = fn(_dev(boxes), _dev(scores), thresh)
        assert keep.tolist() == want.tolist()
        assert 10 < len(want) < len(boxes)                    # some are suppressed, some are kept


# ---------------------------------------------------------------------------------------------- streams, repeats, edges
def test_same_bits_twice_and_on_another_stream(nms_case):
    K, U = _K(), _U()
    boxes, scores, _, _ = nms_case
    tb, ts = _dev(boxes), _dev(scores)
    first = (K.boxes_overlap_bev(tb, tb), K.boxes_iou_bev(tb, tb), K.boxes_iou3d(tb, tb), K.boxes_aligned_iou3d(tb, tb.flip(0)))
    keep = U.nms_gpu(tb, ts, 0.3)[0]
    again = (K.boxes_overlap_bev(tb, tb), K.boxes_iou_bev(tb, tb), K.boxes_iou3d(tb, tb), K.boxes_aligned_iou3d(tb, tb.flip(0)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        third = (K.boxes_overlap_bev(tb, tb), K.boxes_iou_bev(tb, tb), K.boxes_iou3d(tb, tb),
                 K.boxes_aligned_iou3d(tb, tb.flip(0)))
        keep3 = U.nms_gpu(tb, ts, 0.3)[0]
    stream.synchronize()
    for x, y, z in zip(first, again, third):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    assert keep.tolist() == U.nms_gpu(tb, ts, 0.3)[0].tolist() == keep3.tolist()


def test_empty_inputs():
    K, U = _K(), _U()
    none, some = torch.zeros((0, 7), device="cuda"), _dev(_row_of_boxes(3))
    assert U.boxes_iou_bev(none, some).shape == (0, 3) and U.boxes_iou3d_gpu(some, none).shape == (3, 0)
    assert U.boxes_aligned_iou3d_gpu(none, none).shape == (0, 1) and U.paired_boxes_iou3d_gpu(none, none).shape == (0,)
    for fn in (U.nms_gpu, U.nms_normal_gpu):
        keep, second = fn(none, torch.zeros((0,), device="cuda"), 0.5)
        assert second is None and keep.dtype == torch.int64 and keep.is_cuda and keep.numel() == 0
    assert K.nms_mask(none, 0.5).shape == (0, 0)


def test_the_cpu_entry_refuses_device_tensors_like_the_reference():
    U = _U()
    some = _dev(_row_of_boxes(3))
    for a, b in ((some, some), (some.cpu(), some), (some, some.cpu())):
        with pytest.raises(AssertionError, match="Only support CPU tensors"):
            U.boxes_bev_iou_cpu(a, b)
    got = U.boxes_bev_iou_cpu(some.cpu(), some.cpu())              # and agrees with the device on these exact boxes
    assert torch.equal(got, U.boxes_iou_bev(some, some).cpu())
    assert float(got[0, 1]) == float(np.float32(1) / np.float32(3)) and float(got[0, 2]) == 0 and float(got[1, 1]) == 1


def test_more_than_65536_boxes_are_refused_with_the_limit_named():
    K, U = _K(), _U()
    boxes = torch.zeros((65537, 7), device="cuda")
    for call in (lambda: U.nms_gpu(boxes, torch.zeros(65537, device="cuda"), 0.5), lambda: K.nms(boxes, 0.5),
                 lambda: K.nms_mask(boxes, 0.5)):
        with pytest.raises(ValueError, match="65536"):
            call()
