"""CPU oracle of lidargen.ops.pointnet2.pointnet2_stack (tests only; nothing here touches the product's kernels): numpy
restatements of every operator in float32 with separately rounded operations, and a float64 variant of the distances.
Stacked layout: cloud b is rows start_b .. start_b + n_b - 1."""
import numpy as np

F32 = np.float32


def offsets(cnt):
    cnt = np.asarray(cnt, np.int64)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


def batch_of(cnt):
    return np.repeat(np.arange(len(cnt)), np.asarray(cnt, np.int64))


def sqdist(p, q, dtype=F32):
    """(dx dx + dy dy) + dz dz of every row of p [n,3] to the point q, every operation rounded to `dtype`."""
    p = np.asarray(p, dtype).reshape(-1, 3)
    q = np.asarray(q, dtype)
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == dtype
    return d


def radius2(radius, dtype=F32):
    """The kernels' radius^2: the float32 product (in float64: the square of the float32 radius)."""
    r = F32(radius)
    return r * r if dtype == F32 else np.float64(r) * np.float64(r)


def _rows(hits, nsample):
    row = np.zeros(nsample, np.int32)
    if len(hits) == 0:
        row[0] = -1
    else:
        row[:] = hits[0]
        row[:min(len(hits), nsample)] = hits[:nsample]
    return row


def ball_query(xyz, xyz_cnt, new_xyz, new_cnt, radius, nsample, dtype=F32, sizes=None):
    """The kernel's rows [M, nsample] int32 (local indices; an empty ball is [-1, 0, ...]).  sizes (a list): receives the
    number of points inside every ball."""
    xo, no = offsets(xyz_cnt), offsets(new_cnt)
    r2 = radius2(radius, dtype)
    out = np.zeros((no[-1], nsample), np.int32)
    for b in range(len(xyz_cnt)):
        p = np.asarray(xyz)[xo[b]:xo[b + 1]]
        for m in range(no[b], no[b + 1]):
            hits = np.nonzero(sqdist(p, new_xyz[m], dtype) < r2)[0]
            if sizes is not None:
                sizes.append(len(hits))
            out[m] = _rows(hits, nsample)
    return out


def finish_query(raw):
    """(idx with the empty rows set to 0, empty_ball_mask): what the public ball_query / voxel_query return."""
    mask = raw[:, 0] == -1
    idx = raw.copy()
    idx[mask] = 0
    return idx, mask


def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices, inclusive=True):
    """new_coords [M,4] = (batch, z, y, x); the kernel's rows (global rows of xyz), d <= r2 (inclusive=False: d < r2, what
    the kernel does NOT compute)."""
    B, Z, Y, X = point_indices.shape
    zr, yr, xr = max_range
    r2 = radius2(radius)
    out = np.zeros((len(new_coords), nsample), np.int32)
    for m, (b, z0, y0, x0) in enumerate(np.asarray(new_coords)):
        hits = []
        for dz in range(-zr, zr + 1):
            for dy in range(-yr, yr + 1):
                for dx in range(-xr, xr + 1):
                    z, y, x = z0 + dz, y0 + dy, x0 + dx
                    if not (0 <= z < Z and 0 <= y < Y and 0 <= x < X):
                        continue
                    k = int(point_indices[b, z, y, x])
                    if k < 0:
                        continue
                    d = sqdist(xyz[k], new_xyz[m])[0]
                    if d <= r2 if inclusive else d < r2:
                        hits.append(k)
        out[m] = _rows(np.asarray(hits, np.int64), nsample)
    return out


def global_rows(idx, f_cnt, i_cnt):
    """[M, nsample] int64: the global row every entry reads, -1 where the index lies outside its cloud."""
    fo = offsets(f_cnt)
    b = batch_of(i_cnt)[:, None]
    n = np.asarray(f_cnt, np.int64)[b]
    idx = np.asarray(idx, np.int64)
    return np.where((idx >= 0) & (idx < n), fo[b] + idx, -1)


def group(features, f_cnt, idx, i_cnt):
    """[M, C, nsample]: features[start + idx[m, s], c], zero for an index outside its cloud."""
    rows = global_rows(idx, f_cnt, i_cnt)
    f = np.asarray(features)
    out = f[np.maximum(rows, 0)]                                   # [M, nsample, C]
    out = np.where(rows[:, :, None] >= 0, out, 0).astype(f.dtype)
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def group_bwd(grad_out, N, f_cnt, idx, i_cnt):
    """[N, C]: the sum of grad_out [M, C, nsample] into the rows read, in ascending (m, s) order, in grad_out's dtype."""
    rows = global_rows(idx, f_cnt, i_cnt)
    g = np.asarray(grad_out)
    out = np.zeros((N, g.shape[1]), g.dtype)
    for m in range(rows.shape[0]):
        for s in range(rows.shape[1]):
            if rows[m, s] >= 0:
                out[rows[m, s]] = out[rows[m, s]] + g[m, :, s]
    return out


def fps_stack(xyz, cnt, npoints, bs=1024):
    """The reference's stack_farthest_point_sampling_kernel: a block of `bs` threads whatever n is -- thread t scans points
    t, t + bs, ... and keeps its first strict maximum, the tree keeps the left operand on ties.  Global rows."""
    xyz = np.ascontiguousarray(xyz, F32)
    o = offsets(cnt)
    out = []
    for b, M in enumerate(npoints):
        p = xyz[o[b]:o[b + 1]]
        N = len(p)
        rows = (N + bs - 1) // bs
        temp = np.full(N, 1e10, F32)
        pick = np.zeros(M, np.int64)
        old = 0
        for j in range(1, M):
            temp = np.minimum(sqdist(p, p[old]), temp)
            grid = np.concatenate([temp, np.full(rows * bs - N, -2.0, F32)]).reshape(rows, bs)
            r = np.argmax(grid, axis=0)
            dists = grid[r, np.arange(bs)].copy()
            dists_i = r * bs + np.arange(bs)
            s = bs // 2
            while s >= 1:
                v1, v2 = dists[:s].copy(), dists[s:2 * s].copy()
                i1, i2 = dists_i[:s].copy(), dists_i[s:2 * s].copy()
                dists[:s] = np.maximum(v1, v2)
                dists_i[:s] = np.where(v2 > v1, i2, i1)
                s //= 2
            old = int(dists_i[0])
            pick[j] = old
        out.append(pick + o[b])
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)


def three_nn(unknown, u_cnt, known, k_cnt, dtype=F32):
    """(dist2 [N,3] `dtype`, idx [N,3] int32 global rows): ascending (distance, index) under strict <; a slot never filled
    holds +inf and the cloud's start row."""
    uo, ko = offsets(u_cnt), offsets(k_cnt)
    N = uo[-1]
    dist2 = np.full((N, 3), np.inf, dtype)
    idx = np.zeros((N, 3), np.int32)
    for b in range(len(u_cnt)):
        p = np.asarray(known)[ko[b]:ko[b + 1]]
        for n in range(uo[b], uo[b + 1]):
            d = sqdist(p, unknown[n], dtype)
            order = np.argsort(d, kind="stable")[:3]               # ascending (distance, index)
            idx[n] = ko[b]
            idx[n, :len(order)] = ko[b] + order
            dist2[n, :len(order)] = d[order]
    return dist2, idx


def three_interpolate(features, idx, weight):
    """[N, C] = (w0 f0 + w1 f1) + w2 f2 in the dtype of `features`; an index outside [0, M) adds 0."""
    f = np.asarray(features)
    M = f.shape[0]
    idx = np.asarray(idx, np.int64)
    w = np.asarray(weight, f.dtype)
    if M == 0:
        return np.zeros((idx.shape[0], f.shape[1]), f.dtype)
    ok = (idx >= 0) & (idx < M)
    t = [np.where(ok[:, j:j + 1], w[:, j:j + 1] * f[np.clip(idx[:, j], 0, M - 1)], 0).astype(f.dtype) for j in range(3)]
    return (t[0] + t[1]) + t[2]


def three_interpolate_bwd(grad_out, idx, weight, M):
    """[M, C]: grad_out[n] weight[n, j] summed into row idx[n, j] in ascending (n, j) order, in grad_out's dtype."""
    g = np.asarray(grad_out)
    w = np.asarray(weight, g.dtype)
    out = np.zeros((M, g.shape[1]), g.dtype)
    for n in range(g.shape[0]):
        for j in range(3):
            i = int(idx[n, j])
            if 0 <= i < M:
                out[i] = out[i] + g[n] * w[n, j]
    return out


def grouped_operand(xyz, xyz_cnt, new_xyz, new_cnt, features, raw_idx, use_xyz=True):
    """The operand of QueryAndGroup [M, C (+3), nsample] from the ball query's raw rows, in the dtype of `xyz`."""
    idx, mask = finish_query(raw_idx)
    xyz = np.asarray(xyz)
    gx = group(xyz, xyz_cnt, idx, new_cnt) - np.asarray(new_xyz, xyz.dtype)[:, :, None]
    gx[mask] = 0
    if features is None:
        return gx
    gf = group(np.asarray(features, xyz.dtype), xyz_cnt, idx, new_cnt)
    gf[mask] = 0
    return np.concatenate([gx, gf], axis=1) if use_xyz else gf


def rel_l2_rows(got, ref):
    """Per-row relative L2 error of [rows, C] against `ref` (float64); a zero row of `ref` counts with norm 1."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = np.linalg.norm(ref, axis=1)
    return np.linalg.norm(got - ref, axis=1) / np.where(den > 0, den, 1.0)
