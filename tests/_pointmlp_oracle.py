"""CPU oracle of the PointMLP extractor (tests only; nothing here touches the product's kernels): a numpy restatement of the
reference's farthest point sampling kernel, the (distance, index) k nearest neighbours, the grouped operand and the whole
network in any dtype from a state dict."""
import numpy as np
import torch

TOL_CONV = 2e-6
"""Per-sample relative L2 bound of one dense layer / one grouped operand against float64: the bound of
tests/_rangenet_oracle.py, whose kernel has the same k chunking (chunks of 32, fma chains from zero, added in order)."""
EPS = 1e-5


def block_size(N):
    """The reference launcher's thread count: the largest power of two <= min(N, 1024)."""
    bs = 1
    while bs * 2 <= min(N, 1024):
        bs *= 2
    return bs


def fps(xyz, M):
    """The reference's farthest_point_sampling_kernel on one cloud [N,3] float32, step by step: a strided scan per thread
    that keeps the first strict maximum, then the tree that takes the right operand only when it is strictly larger.
    float32 operations, each rounded on its own."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    N = xyz.shape[0]
    bs = block_size(N)
    rows = (N + bs - 1) // bs
    temp = np.full(N, 1e10, np.float32)
    out = np.zeros(M, np.int32)
    old = 0
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pad = rows * bs - N
    for j in range(1, M):
        dx, dy, dz = x - x[old], y - y[old], z - z[old]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        temp = np.minimum(d, temp)
        grid = np.concatenate([temp, np.full(pad, -2.0, np.float32)]).reshape(rows, bs)   # thread t scans column t
        r = np.argmax(grid, axis=0)                                                       # first maximum: `d2 > best`
        dists = grid[r, np.arange(bs)].copy()
        dists_i = (r * bs + np.arange(bs)).astype(np.int64)
        s = bs // 2
        while s >= 1:
            v1, v2 = dists[:s].copy(), dists[s:2 * s].copy()
            i1, i2 = dists_i[:s].copy(), dists_i[s:2 * s].copy()
            dists[:s] = np.maximum(v1, v2)
            dists_i[:s] = np.where(v2 > v1, i2, i1)
            s //= 2
        old = int(dists_i[0])
        out[j] = old
    return out


def fps_batch(xyz, M):
    return np.stack([fps(c, M) for c in np.asarray(xyz)])


def sqdist(xyz, q):
    """float32 (dx dx + dy dy) + dz dz of every point of [N,3] to the point q."""
    xyz = np.asarray(xyz, np.float32)
    dx, dy, dz = xyz[:, 0] - q[0], xyz[:, 1] - q[1], xyz[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def knn(xyz, query_idx, K):
    """[S,K] int32: the K nearest points of every query, ascending (distance, index)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    out = np.zeros((len(query_idx), K), np.int32)
    for s, q in enumerate(query_idx):
        out[s] = np.argsort(sqdist(xyz, xyz[q]), kind="stable")[:K]
    return out


def knn_batch(xyz, query_idx, K):
    return np.stack([knn(c, q, K) for c, q in zip(np.asarray(xyz), np.asarray(query_idx))])


def geometry(xyz, groups, kneighbors):
    """[(fps_idx [B,S], knn_idx [B,S,K])] per stage from xyz [B,N,3] float32, as Model.geometry builds them."""
    xyz = np.asarray(xyz, np.float32)
    tables = []
    for S, K in zip(groups, kneighbors):
        f = fps_batch(xyz, S)
        tables.append((f, knn_batch(xyz, f, K)))
        xyz = np.stack([c[i] for c, i in zip(xyz, f)])
    return tables


def same_neighbour_coordinates(xyz, a, b):
    """True when the index rows a, b [S,K] of one cloud name the same multiset of coordinates on every query."""
    xyz = np.asarray(xyz, np.float32)
    for ra, rb in zip(np.asarray(a), np.asarray(b)):
        pa, pb = xyz[ra], xyz[rb]
        if not np.array_equal(pa[np.lexsort(pa.T)], pb[np.lexsort(pb.T)]):
            return False
    return True


def group(x, fps_idx, knn_idx, alpha, beta, eps=EPS):
    """x [B,d,N] -> [B,2d,S K] in x's dtype: (alpha (x[knn] - x[anchor]) / (std + eps) + beta, x[anchor]), std the unbiased
    deviation over all differences of a cloud; also returns std [B]."""
    B, d, N = x.shape
    f = torch.as_tensor(np.asarray(fps_idx)).long()
    k = torch.as_tensor(np.asarray(knn_idx)).long()
    S, K = k.shape[1], k.shape[2]
    anchor = torch.gather(x, 2, f[:, None, :].expand(B, d, S))                             # [B,d,S]
    nb = torch.gather(x, 2, k.reshape(B, 1, S * K).expand(B, d, S * K)).reshape(B, d, S, K)
    diff = nb - anchor[..., None]
    std = diff.reshape(B, -1).std(dim=1)
    norm = alpha.reshape(1, d, 1, 1) * (diff / (std.reshape(B, 1, 1, 1) + eps)) + beta.reshape(1, d, 1, 1)
    out = torch.cat([norm, anchor[..., None].expand(B, d, S, K)], 1).reshape(B, 2 * d, S * K)
    return out, std


def dense(x, w, b, act, res=None):
    y = torch.einsum("oc,bcl->bol", w, x) + b[None, :, None]
    if res is not None:
        y = y + res
    return torch.relu(y) if act else y


def fold(sd, conv, bn, dtype):
    """(w [Co,Ci], b [Co]) of state-dict layer `conv` followed by BatchNorm `bn` (None: plain), in float64, cast to dtype."""
    w = sd[conv + ".weight"].double()
    w = w.reshape(w.shape[0], -1)
    b = sd[conv + ".bias"].double() if conv + ".bias" in sd else torch.zeros(w.shape[0], dtype=torch.float64)
    if bn is not None:
        s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
        w = w * s[:, None]
        b = (b - sd[bn + ".running_mean"].double()) * s + sd[bn + ".bias"].double()
    return w.to(dtype), b.to(dtype)


def config_of(model):
    """(anchors, neighbours, pre blocks, pos blocks) per stage of a Model of either tree."""
    return ([g.groups for g in model.local_grouper_list], [g.kneighbors for g in model.local_grouper_list],
            [len(p.operation) for p in model.pre_blocks_list], [len(p.operation) for p in model.pos_blocks_list])


def forward(sd, cfg, x, tables, dtype=torch.float64, mutate=None):
    """(features [B,C], logits [B,classes]) of the network with state dict `sd` on x [B,3,N] and the index tables
    `tables`, computed in `dtype` with BatchNorm as an eval-mode fold.  mutate: None, or 'eps' (the + 1e-5 dropped)."""
    groups, kn, pre, pos = cfg
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    eps = 0.0 if mutate == "eps" else EPS

    def layer(t, conv, bn, act, res=None):
        w, b = fold(sd, conv, bn, dtype)
        return dense(t, w, b, act, res)

    def block(t, stem):
        u = layer(t, stem + ".net1.0", stem + ".net1.1", True)
        return layer(u, stem + ".net2.0", stem + ".net2.1", True, res=t)

    feat = layer(torch.as_tensor(x).to(dtype), "embedding.net.0", "embedding.net.1", True)
    for i, (f, k) in enumerate(tables):
        g, _ = group(feat, f, k, sd[f"local_grouper_list.{i}.affine_alpha"].to(dtype),
                     sd[f"local_grouper_list.{i}.affine_beta"].to(dtype), eps)
        t = layer(g, f"pre_blocks_list.{i}.transfer.net.0", f"pre_blocks_list.{i}.transfer.net.1", True)
        for j in range(pre[i]):
            t = block(t, f"pre_blocks_list.{i}.operation.{j}")
        B, C, L = t.shape
        feat = t.reshape(B, C, L // kn[i], kn[i]).amax(3)
        for j in range(pos[i]):
            feat = block(feat, f"pos_blocks_list.{i}.operation.{j}")
    f = feat.amax(2)
    h = f.t()[None]
    h = layer(h, "classifier.0", "classifier.1", True)
    h = layer(h, "classifier.4", "classifier.5", True)
    h = layer(h, "classifier.8", None, False)
    return f, h[0].t()


def rel_l2_per_sample(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    B = ref.shape[0]
    e = (got - ref).reshape(B, -1).norm(dim=1) / ref.reshape(B, -1).norm(dim=1)
    return [float(v) for v in e]


def clouds(B, N, seed, real=None):
    """[B,N,3] float32 in [0,1]^3; real = a list of B counts: cloud b keeps its first real[b] points, the rest are zero
    padding (NuscObject.__getitem__)."""
    g = np.random.default_rng(seed)
    c = g.random((B, N, 3), dtype=np.float32)
    if real is not None:
        for b, n in enumerate(real):
            c[b, n:] = 0.0
    return c
