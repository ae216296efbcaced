"""Numpy restatement of the chamfer backward (csrc/chamfer_bwd.hip) and the scenes of its tests.

`backward` adds the reference's terms (chamfer3D.cu:155-195: g = grad * 2, t = g * (own - other), the neighbour receives
-(t)) in the order the kernel documents, every operation rounded to float32:

    a = +0 + d                                       d the row's direct term
    L <= SERIAL:  row = (((a + s_0) + s_1) + ...)    s_i its scattered terms in ascending source index
    L  > SERIAL:  row = a + T,  q_t = ((+0 + s_t) + s_{t+LANES}) + ...  for lane t of LANES (q_t = +0 for t >= L),
                  T = q_0 after  for h = LANES/2, ..., 1:  q_t = q_t + q_{t+h}  (t < h)

`terms64` gives, per output element, the float64 sum of the same terms, their count c (the direct term included) and
sum |t_i|: what the summation-order bounds of the tests are made of."""
import numpy as np

F32 = np.float32
SERIAL = 32     # CB_SERIAL of csrc/chamfer_bwd.hip
LANES = 256     # CB_BLOCK


def scene(B, N, M, kind, seed, dim=3):
    """float32 clouds a [B,N,dim], b [B,M,dim]; the recipes of the forward's reference-kernel test (rand / same / dups /
    large) and two of this test's own: `funnel` (every row of a nearest to ONE row of b) and `hubs` (the rows of a
    shared among three rows of b: two in one wave of a block, one in another)."""
    g = np.random.default_rng(seed)
    if kind == "large":
        base = g.uniform(-1e4, 1e4, (B, 1, dim))
        a = (base + g.uniform(-1, 1, (B, N, dim)) * 1e-2).astype(F32)
        b = (base + g.uniform(-1, 1, (B, M, dim)) * 1e-2).astype(F32)
        return a, b
    a = g.normal(0, 5, (B, N, dim)).astype(F32)
    if kind == "same":
        assert N == M
        return a, a.copy()
    b = g.normal(0, 5, (B, M, dim)).astype(F32)
    if kind == "dups":
        # duplicated targets within a group of four and across the forward's 512-target chunk boundary; queries sit
        # next to them, so that the duplicate pair is the nearest (the first must win)
        pairs = [(k, k + d) for k in (0, 4, 9, 100, 508) for d in (1, 2, 3)] + \
                [(1, 513), (511, 512), (100, 612), (3, 1027), (600, 1536)]
        used = []
        for i, j in pairs:
            if j < M:
                b[:, j] = b[:, i]
                used.append(i)
        for r in range(min(N, 4 * len(used)) if used else 0):
            a[:, r] = b[:, used[r % len(used)]] + g.normal(0, 1e-3, (B, dim)).astype(F32)
    elif kind in ("funnel", "hubs"):
        # targets far apart (a lattice of pitch 10 with a small jitter), sources within 1e-2 of their hub
        side = int(np.ceil(M ** (1.0 / dim))) + 1
        b = (10.0 * np.stack(np.unravel_index(np.arange(M), (side,) * dim), -1)[None]
             + g.uniform(-1, 1, (B, M, dim))).astype(F32)
        hubs = [M // 2] if kind == "funnel" else [5, 6, 130]
        assert max(hubs) < M
        owner = np.asarray(hubs)[np.arange(N) * len(hubs) // N]
        a = (b[:, owner] + g.uniform(-1, 1, (B, N, dim)) * 1e-2).astype(F32)
    else:
        assert kind == "rand", kind
    return a, b


def grads(B, N, M, seed, zero_rows=False):
    """Seeded normal grad_dist1 [B,N], grad_dist2 [B,M]; zero_rows: batch entry 0 of the first and every third column of
    the second are zero."""
    g = np.random.default_rng(seed + 7)
    g1, g2 = g.normal(0, 1, (B, N)).astype(F32), g.normal(0, 1, (B, M)).astype(F32)
    if zero_rows:
        g1[0] = 0
        g2[:, ::3] = 0
    return g1, g2


def nearest(q, t):
    """int32 index of the first float32-nearest row of t [B,M,D] for every row of q [B,N,D] (a host stand-in for the
    forward: the properties of the restatement hold for any index)."""
    d = (t[:, None] - q[:, :, None]).astype(F32)
    return np.argmin((d * d).sum(-1, dtype=F32), axis=-1).astype(np.int32)


def _inverse(idx, targets):
    order = np.argsort(idx, kind="stable")
    seg = np.searchsorted(idx[order], np.arange(targets + 1))
    return order, seg


def _one_way(own, other, g_own, idx_own, g_other, idx_other):
    """grad of `own` [n,D] for one batch entry, float32, in the documented order.  An index outside its cloud adds no
    term (the forward writes none)."""
    n, m = own.shape[0], other.shape[0]
    ok = (idx_own >= 0) & (idx_own < m)
    acc = F32(0) + np.where(ok[:, None], (g_own * F32(2))[:, None] * (own - other[np.where(ok, idx_own, 0)]), F32(0))
    src = np.nonzero((idx_other >= 0) & (idx_other < n))[0]                # the sources that scatter, ascending
    s = -((g_other[src] * F32(2))[:, None] * (other[src] - own[idx_other[src]]))
    order, seg = _inverse(idx_other[src], n)
    length = seg[1:] - seg[:-1]
    short = length <= SERIAL
    for i in range(int(length[short].max(initial=0))):
        rows = np.nonzero(short & (length > i))[0]
        acc[rows] = acc[rows] + s[order[seg[rows] + i]]
    for r in np.nonzero(~short)[0]:
        q = np.zeros((LANES, own.shape[1]), F32)
        for c in range(seg[r], seg[r + 1], LANES):
            chunk = s[order[c:min(c + LANES, seg[r + 1])]]
            q[:len(chunk)] = q[:len(chunk)] + chunk
        h = LANES // 2
        while h:
            q[:h] = q[:h] + q[h:2 * h]
            h //= 2
        acc[r] = acc[r] + q[0]
    assert acc.dtype == F32
    return acc


def backward(a, b, g1, g2, i1, i2):
    """(grad_xyz1, grad_xyz2) float32 of clouds a [B,N,D], b [B,M,D]."""
    ga, gb = np.empty_like(a), np.empty_like(b)
    for k in range(a.shape[0]):
        ga[k] = _one_way(a[k], b[k], g1[k], i1[k], g2[k], i2[k])
        gb[k] = _one_way(b[k], a[k], g2[k], i2[k], g1[k], i1[k])
    return ga, gb


def direct(a, b, g1, i1):
    """+0 + the direct term of every row of a, float32: what a row that receives nothing must hold."""
    return F32(0) + (g1 * F32(2))[..., None] * (a - np.take_along_axis(b, i1[..., None].astype(np.int64), 1))


def terms64(a, b, g1, g2, i1, i2):
    """Per element of (grad_xyz1, grad_xyz2): (float64 sum, count of terms, float64 sum of |term|)."""
    out = []
    for own, other, g_own, i_own, g_other, i_other in ((a, b, g1, i1, g2, i2), (b, a, g2, i2, g1, i1)):
        own, other, g_own, g_other = (v.astype(np.float64) for v in (own, other, g_own, g_other))
        val, cnt, mag = np.empty_like(own), np.empty_like(own), np.empty_like(own)
        for k in range(own.shape[0]):
            ok = (i_own[k] >= 0) & (i_own[k] < other.shape[1])
            d = np.where(ok[:, None], 2 * g_own[k][:, None] * (own[k] - other[k][np.where(ok, i_own[k], 0)]), 0.0)
            src = np.nonzero((i_other[k] >= 0) & (i_other[k] < own.shape[1]))[0]
            tgt = i_other[k][src]
            s = -(2 * g_other[k][src][:, None] * (other[k][src] - own[k][tgt]))
            v, c, m = d.copy(), np.broadcast_to(ok[:, None], d.shape).astype(np.float64), np.abs(d)
            np.add.at(v, tgt, s)
            np.add.at(c, tgt, 1)
            np.add.at(m, tgt, np.abs(s))
            val[k], cnt[k], mag[k] = v, c, m
        out.append((val, cnt, mag))
    return out


def bits_equal(x, y):
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    return bool(np.array_equal(x.view(np.int32), y.view(np.int32)))
