"""Voxel scatter of the weight-free metrics -- mirror of the reference's
lidargen/metrics/metric_utils.py: `ravel_hash` :28-40, `sparse_quantize` :43-66, `pcd2bev_sum`
:233-258 (the BEV occupancy volume the JSD of eval_utils.compute_jsd :84-95 is computed from), `pcd2bev_bin` :261-284
(the BEV cell sets the MMD of eval_utils.compute_mmd is computed from; one bitmap per cloud, csrc/bev_chamfer.hip).
The point sets stay on the device: sweeps are scattered with atomics (lc_bev_occupancy_accumulate),
unique voxels come from a device radix sort (lc_sparse_quantize).  numpy in -> numpy out, CUDA
tensors in -> CUDA tensors out.  Of the feature-extractor front-ends of that module the sparse-volume one is built
(`preprocess_pcd` :310-314, `pcd2voxel` :157-167, a collate, `compute_logits` :374-412 for 'voxel' with the depth-sector
aggregation of `batch2list` :351-365 on the device) and the point-voxel one (`compute_point_voxel_logits`: the same
input and aggregation around the SPVCNN) and the range-image one (`pcd2range` :69-122, `range2xyz` :125-154,
`preprocess_range` :317-322 in numpy on the host, `compute_range_logits`: RangeNet over 5-channel range images, row-band
means on the device).  `compute_logits` still refuses 'point_voxel' and 'range' by name (its callers rely on that) and
points at `compute_point_voxel_logits` / `compute_range_logits`.
With `preprocess_device='cuda'` the three front-ends prepare a whole batch of clouds on the device instead of cloud by cloud
on the host (`preprocess_range_batch`, `pcd2voxel_batch`; csrc/metric_preprocess.hip); None, the
default, is the host route, unchanged."""
from __future__ import annotations

import math

import numpy as np
import torch

from lidarcrafter_amd import ops as K
from lidarcrafter_amd import ops_metric_pre as KP
from lidarcrafter_amd import ops_spconv as KS

# lidargen/metrics/__init__.py:28-33
VOXEL_SIZE = 0.05
DATA_CONFIG = {"64": {"x": [-50, 50], "y": [-50, 50], "z": [-3, 1]},
               "32": {"x": [-30, 30], "y": [-30, 30], "z": [-3, 6]}}


def _dev(a):
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("metric_utils needs the MI355X: no CPU fallback on the hot path")
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda(), True
    return a.float().contiguous(), False


def ravel_hash(x):
    """[N, D] integer coordinates -> uint64 hash, row-major over (x - min) with extents max + 1."""
    t = torch.as_tensor(x)
    t = (t - t.min(dim=0).values).to(torch.int64)
    ext = t.max(dim=0).values + 1
    h = torch.zeros(t.shape[0], dtype=torch.int64, device=t.device)
    for k in range(t.shape[1] - 1):
        h = (h + t[:, k]) * ext[k + 1]
    h = h + t[:, -1]
    return h.cpu().numpy().astype(np.uint64) if isinstance(x, np.ndarray) else h


def sparse_quantize(coords, voxel_size=1, *, return_index: bool = False, return_inverse: bool = False):
    c, is_np = _dev(coords)
    out = K.sparse_quantize(c, voxel_size, return_index=return_index, return_inverse=return_inverse)
    if not is_np:
        return out
    if isinstance(out, (list, tuple)):
        return [o.cpu().numpy() for o in out]
    return out.cpu().numpy()


def pcd2bev_sum(data_type, *args, voxel_size=VOXEL_SIZE):
    """For every set of sweeps in `args`: float32 [nx, ny] volume whose cell (i, j) counts the
    sweeps that have at least one point in voxel (i, j) of the BEV range of `data_type`."""
    cfg = DATA_CONFIG[data_type]
    output = tuple()
    for data in args:
        acc, is_np = None, False
        for pcd in data:
            p, is_np = _dev(pcd)
            if acc is None:
                acc = K.BevOccupancy(cfg["x"], cfg["y"], voxel_size, p.device)
            acc.add(p)
        if acc is None:
            vol = torch.zeros((math.ceil((cfg["x"][1] - cfg["x"][0]) / voxel_size),
                               math.ceil((cfg["y"][1] - cfg["y"][0]) / voxel_size)))
            output += (vol.numpy(),)
        else:
            output += (acc.grid.cpu().numpy() if is_np else acc.grid,)
    return output


def bev_bin(x_range, y_range, voxel_size, *args):
    """pcd2bev_bin on any range: for every list of clouds in `args` a list of float32 [k, 2] arrays, the unique cells
    (strict mask, floor(xy / voxel) - ceil(min / voxel)) in row-major order with x major, each divided by (nx, ny) in
    float64 and rounded to float32.  A cloud with no point in range gives a [0, 2] array."""
    output = tuple()
    for data in args:
        data = list(data)
        if not data:
            output += ([],)
            continue
        devd = [_dev(pcd) for pcd in data]
        cells, (nx, ny) = K.bev_cells([p for p, _ in devd], x_range, y_range, voxel_size)
        shape = torch.tensor([nx, ny], dtype=torch.float64, device=cells[0].device)
        vals = [(c.to(torch.float64) / shape).to(torch.float32) for c in cells]
        output += ([v.cpu().numpy() if is_np else v for v, (_, is_np) in zip(vals, devd)],)
    return output


def pcd2bev_bin(data_type, *args, voxel_size=0.5):
    """For every set of sweeps in `args`: per sweep the float32 [k, 2] unique BEV cells of `data_type`'s range, as
    cell / (nx, ny) (metric_utils.py:261-284)."""
    cfg = DATA_CONFIG[data_type]
    return bev_bin(cfg["x"], cfg["y"], voxel_size, *args)


def compute_jsd(reference, samples, data):
    """eval_utils.compute_jsd :84-95 (value returned instead of printed)."""
    from scipy.spatial.distance import jensenshannon

    r, s = pcd2bev_sum(data, reference, samples)
    r = r.cpu().numpy() if isinstance(r, torch.Tensor) else r
    s = s.cpu().numpy() if isinstance(s, torch.Tensor) else s
    return float(jensenshannon((r / np.sum(r)).flatten(), (s / np.sum(s)).flatten()))


# ---- the sparse-volume front-end (FSVD) ---------------------------------------------------------------------------
class SparseTensor:
    """Rows `F` [N, C] over integer coordinates `C` [N, 3] (one cloud) or [N, 4] = (x, y, z, batch) (a collated batch)."""

    def __init__(self, feats, coords, stride=1):
        self.F, self.C, self.s = feats, coords, stride


def preprocess_pcd(pcd, **kwargs):
    """The rows with depth_range[0] < |p| < depth_range[1] (metric_utils.py:310-314)."""
    lo, hi = kwargs["depth_range"]
    if isinstance(pcd, torch.Tensor):
        depth = torch.linalg.vector_norm(pcd, 2, dim=1)
        return pcd[(depth > lo) & (depth < hi)]
    depth = np.linalg.norm(pcd, 2, axis=1)
    return pcd[np.logical_and(depth > lo, depth < hi)]


def pcd2voxel(pcd):
    """One cloud [N, 3] -> {'lidar': SparseTensor(F [n, 4] float32 = (x, y, z, -1) of each voxel's first point, C [n, 3]
    = round(p / 0.05) - min, unique, in np.unique(ravel_hash) order)} (metric_utils.py:157-167).  A numpy cloud is
    quantized on the host in numpy's own arithmetic (round half to even in the dtype of pcd / 0.05) and gives CPU tensors;
    a CUDA tensor is quantized by lc_sparse_quantize and stays on the device."""
    if pcd.ndim != 2 or pcd.shape[1] != 3:
        raise ValueError(f"pcd2voxel: a cloud must be [N, 3], got {tuple(pcd.shape)}")
    if isinstance(pcd, torch.Tensor):
        if not pcd.is_cuda:
            raise RuntimeError("pcd2voxel: a tensor must be a CUDA(HIP) tensor (a numpy cloud is quantized on the host)")
        if pcd.shape[0] == 0:
            return {"lidar": SparseTensor(pcd.new_zeros((0, 4), dtype=torch.float32),
                                          torch.zeros((0, 3), dtype=torch.int64, device=pcd.device))}
        v = torch.round(pcd / VOXEL_SIZE)
        v = (v - v.min(dim=0, keepdim=True).values).float().contiguous()
        _, inds = K.sparse_quantize(v, 1, return_index=True)
        feat = torch.cat([pcd[inds].float(), -torch.ones((inds.numel(), 1), device=pcd.device)], dim=1)
        return {"lidar": SparseTensor(feat, v[inds].long())}
    if pcd.shape[0] == 0:
        return {"lidar": SparseTensor(torch.zeros((0, 4)), torch.zeros((0, 3), dtype=torch.int64))}
    v = np.round(pcd / VOXEL_SIZE)
    v = v - v.min(0, keepdims=True)
    ext = v.max(0).astype(np.uint64) + 1
    q = v.astype(np.uint64)
    h = (q[:, 0] * ext[1] + q[:, 1]) * ext[2] + q[:, 2]         # ravel_hash: row-major over the extents
    _, inds = np.unique(h, return_index=True)
    feat = np.concatenate((pcd[inds], -np.ones((inds.shape[0], 1))), axis=1)
    return {"lidar": SparseTensor(torch.from_numpy(feat.astype(np.float32)), torch.from_numpy(v[inds].astype(np.int64)))}


def sparse_collate(batch, device=None):
    """[pcd2voxel(...)] -> (feats [N, 4] float32, coords [N, 4] int32 = (x, y, z, batch), offsets int32 [len + 1]) on
    `device` (default: where the first cloud is): torchsparse's sparse_collate_fn, batch index last."""
    ts = [b["lidar"] for b in batch]
    if not ts:
        raise ValueError("sparse_collate: an empty batch")
    device = ts[0].F.device if device is None else device
    feats = torch.cat([t.F.to(device) for t in ts]).float().contiguous()
    coords = torch.cat([torch.cat([t.C.to(device).to(torch.int32),
                                   torch.full((t.C.shape[0], 1), i, dtype=torch.int32, device=device)], dim=1)
                        for i, t in enumerate(ts)]).contiguous()
    counts = torch.tensor([0] + [t.C.shape[0] for t in ts], dtype=torch.int64)
    return feats, coords, torch.cumsum(counts, 0).to(torch.int32).to(device)


def pcd2voxel_batch(clouds, device="cuda", depth_range=None, **kwargs):
    """A list of [N, 3] clouds -> the triple `sparse_collate([pcd2voxel(preprocess_pcd(c, depth_range=...)) for c in
    clouds], device)` returns, bit for bit, computed on the device in one pass over the batch: one upload (numpy clouds; CUDA
    tensors are concatenated on the device), one sort, one device->host read (lc_voxel_batch_fwd).  Depth filter and
    rint(p / 0.05) run in the clouds' own dtype, float32 or float64, as numpy runs them; the quotient is the IEEE division.
    (The per-cloud route of a CUDA tensor through `pcd2voxel` divides as torch does, by multiplying with 1 / 0.05 = 20: the
    two agree wherever p * 20 is exact.)  There is no fallback: without a GPU, or for a `device` that is not a CUDA(HIP)
    device, it raises; an empty list raises as `sparse_collate` does.  Further keywords are ignored, as by `preprocess_pcd`:
    a whole DATASET_CONFIG entry may be passed."""
    if depth_range is None:
        raise TypeError("pcd2voxel_batch: `depth_range` is required (DATASET_CONFIG[...]['depth_range'])")
    clouds = list(clouds)
    if not clouds:
        raise ValueError("pcd2voxel_batch: an empty batch")
    KP.voxel_key_bits(len(clouds), float(depth_range[1]), VOXEL_SIZE)
    pts, offsets = KP.ragged(clouds, device)
    return KP.voxelize(pts, offsets, depth_range, VOXEL_SIZE)


def check_preprocess_device(preprocess_device, need_gpu=True):
    """None: the host route.  Otherwise the CUDA(HIP) device of the batched route; anything else raises ValueError, a
    missing GPU RuntimeError (`need_gpu=False` checks the value alone)."""
    if preprocess_device is None:
        return None
    return KP._device(preprocess_device, need_gpu)


def sector_edges(depth_range):
    """The 17 float32 edges of the 16 depth sectors (batch2list 'depth', metric_utils.py:357-358)."""
    from . import NUM_SECTORS

    e = torch.linspace(depth_range[0] + 3, depth_range[1], NUM_SECTORS + 1)
    e[0] = 0.0
    return e


def _sector_features(data_type, modality, model, sets, preprocess_device=None):
    """Per list of [N, 3] clouds in `sets` the float32 [n, 16 * width] depth-sector means of `model`'s features,
    MODAL2BATCHSIZE[modality] clouds at a time.  `preprocess_device`: None quantizes cloud by cloud (`pcd2voxel`), 'cuda' a
    batch at a time on the device (`pcd2voxel_batch`)."""
    from . import DATASET_CONFIG, MODAL2BATCHSIZE, TYPE2DATASET

    cfg = DATASET_CONFIG[TYPE2DATASET[data_type]]
    bs = MODAL2BATCHSIZE[modality]
    dev = next(model.parameters()).device
    edges = sector_edges(cfg["depth_range"]).to(dev)
    pre = check_preprocess_device(preprocess_device)
    output = tuple()
    for data in sets:
        rows = []
        for i in range(math.ceil(len(data) / bs)):
            if pre is None:
                batch = [pcd2voxel(preprocess_pcd(pcd, **cfg)) for pcd in data[i * bs:(i + 1) * bs]]
                feats, coords, offsets = sparse_collate(batch, dev)
            else:
                feats, coords, offsets = pcd2voxel_batch(data[i * bs:(i + 1) * bs], dev, depth_range=cfg["depth_range"])
            out = model(feats, coords, return_final_logits=True)
            rows.append(KS.sector_means(out["logits"], coords, offsets, edges, VOXEL_SIZE).cpu().numpy())
        output += (np.concatenate(rows) if rows else np.zeros((0, 0), np.float32),)
    return output


def compute_logits(data_type, modality, *args, model=None, root=None, preprocess_device=None):
    """For every list of [N, 3] clouds in `args` the float32 [n, 16 * width] matrix of depth-sector means of the
    extractor's features (metric_utils.py:374-412), MODAL2BATCHSIZE clouds at a time.  Only 'voxel' (MinkowskiNet, FSVD)
    is dispatched from here; 'point_voxel' (SPVCNN, FPVD) is `compute_point_voxel_logits`, 'range' (RangeNet, FRID) is
    `compute_range_logits`.  `model`: a minkowskinet Model
    in eval mode on the GPU; None builds the pretrained one (build_model).  `preprocess_device`: None quantizes on the host,
    'cuda' on the device a batch at a time (`pcd2voxel_batch`: the same bits)."""
    from . import MODALITY2MODEL, TYPE2DATASET, build_model

    assert data_type in ["32", "64"]
    assert modality in ["range", "voxel", "point_voxel"]
    if modality == "point_voxel":
        raise NotImplementedError(f"compute_logits: modality '{modality}' ({MODALITY2MODEL[modality]}) is not dispatched "
                                  "from here; call metric_utils.compute_point_voxel_logits(data_type, *sets)")
    if modality != "voxel":
        raise NotImplementedError(f"compute_logits: modality '{modality}' ({MODALITY2MODEL[modality]}) is not dispatched "
                                  "from here; call metric_utils.compute_range_logits(data_type, *sets)")
    check_preprocess_device(preprocess_device, need_gpu=False)
    if not torch.cuda.is_available():
        raise RuntimeError("compute_logits needs the MI355X: no CPU fallback on the hot path")
    if model is None:
        model = build_model(TYPE2DATASET[data_type], MODALITY2MODEL[modality], device="cuda", root=root)
    return _sector_features(data_type, modality, model, args, preprocess_device)


def compute_point_voxel_logits(data_type, *sets, model=None, root=None, preprocess_device=None):
    """For every list of [N, 3] clouds in `sets` the float32 [n, 16 * 48 = 768] matrix of depth-sector means of the
    SPVCNN's per-point features (the reference's compute_logits for 'point_voxel'), 25 clouds at a time.  The points are
    the unique voxels of pcd2voxel; their sector is decided from the integer voxel coordinate (the
    reference feeds the float coordinate, which is that integer or 1 ulp above it).  `model`: a spvcnn Model in eval mode
    on the GPU; None loads the pretrained one (models.spvcnn.pretrained).  `preprocess_device`: as in `compute_logits`."""
    from . import TYPE2DATASET
    from .models import spvcnn

    assert data_type in ["32", "64"]
    check_preprocess_device(preprocess_device, need_gpu=False)
    if not torch.cuda.is_available():
        raise RuntimeError("compute_point_voxel_logits needs the MI355X: no CPU fallback on the hot path")
    if model is None:
        model = spvcnn.pretrained(TYPE2DATASET[data_type], device="cuda", root=root)
    return _sector_features(data_type, "point_voxel", model, sets, preprocess_device)


# ---- the range-image front-end (FRID) -----------------------------------------------------------------------------
def pcd2range(pcd, size, fov, depth_range, remission=None, labels=None, **kwargs):
    """One cloud [N, 3] -> (float32 [H, W] depth image with -1 where no point falls, feature image or None): spherical
    projection, the nearest point of a pixel wins (metric_utils.py:69-122).  numpy on the host, in the cloud's dtype."""
    fov_up, fov_down = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
    fov_range = abs(fov_down) + abs(fov_up)
    depth = np.linalg.norm(pcd, 2, axis=1)
    mask = np.logical_and(depth > depth_range[0], depth < depth_range[1])
    depth, pcd = depth[mask], pcd[mask]
    yaw = -np.arctan2(pcd[:, 1], pcd[:, 0])
    pitch = np.arcsin(pcd[:, 2] / depth)
    proj_x = 0.5 * (yaw / np.pi + 1.0)
    proj_y = 1.0 - (pitch + abs(fov_down)) / fov_range
    proj_x *= size[1]
    proj_y *= size[0]
    proj_x = np.maximum(0, np.minimum(size[1] - 1, np.floor(proj_x))).astype(np.int32)
    proj_y = np.maximum(0, np.minimum(size[0] - 1, np.floor(proj_y))).astype(np.int32)
    order = np.argsort(depth)[::-1]                      # far first: the nearest point is written last
    proj_x, proj_y, depth = proj_x[order], proj_y[order], depth[order]
    proj_range = np.full(size, -1, dtype=np.float32)
    proj_range[proj_y, proj_x] = depth
    proj_feature = None
    if remission is not None:
        proj_feature = np.full(size, -1, dtype=np.float32)
        proj_feature[proj_y, proj_x] = remission[mask][order]
    elif labels is not None:
        proj_feature = np.full(size, 0, dtype=np.float32)
        proj_feature[proj_y, proj_x] = labels[mask][order]
    return proj_range, proj_feature


def range2xyz(range_img, fov, depth_range, depth_scale=None, log_scale=True, **kwargs):
    """[H, W] depth image -> float64 [3, H, W] points of the pixel centres' rays, -1 where the depth is outside
    `depth_range` (metric_utils.py:125-154).  `depth_scale` is read only with `log_scale` (depth = 2^(img * scale) - 1);
    it has a default here because the nuScenes settings carry none and preprocess_range never uses it."""
    size = range_img.shape
    fov_up, fov_down = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
    fov_range = abs(fov_down) + abs(fov_up)
    depth = (np.exp2(range_img * depth_scale) - 1) if log_scale else range_img
    scan_x, scan_y = np.meshgrid(np.arange(size[1]), np.arange(size[0]))
    scan_x = scan_x.astype(np.float64) / size[1]
    scan_y = scan_y.astype(np.float64) / size[0]
    yaw = np.pi * (scan_x * 2 - 1)
    pitch = (1.0 - scan_y) * fov_range - abs(fov_down)
    xyz = -np.ones((3, *size))
    xyz[0] = np.cos(yaw) * np.cos(pitch) * depth
    xyz[1] = -np.sin(yaw) * np.cos(pitch) * depth
    xyz[2] = np.sin(pitch) * depth
    mask = np.logical_and(depth > depth_range[0], depth < depth_range[1])
    xyz[:, ~mask] = -1
    return xyz


def preprocess_range(pcd, **kwargs):
    """One cloud -> float64 [4, H, W]: the depth image on top of its back-projection (metric_utils.py:317-322)."""
    depth_img = pcd2range(pcd, **kwargs)[0]
    xyz_img = range2xyz(depth_img, log_scale=False, **kwargs)
    return np.vstack([depth_img[None], xyz_img])


def preprocess_range_batch(clouds, device="cuda", remission=None, labels=None, **cfg):
    """A list of [N, 3] clouds -> float32 [B, 4, H, W] on the device: depth on top of its back-projection, computed by
    lc_range_batch_fwd in one pass over the batch (`cfg`: size, fov, depth_range as for `preprocess_range`).
    The contract: the result is `torch.from_numpy(np.stack([preprocess_range(c.astype(np.float64), **cfg) for c in
    clouds])).float()` -- the host route applied to the clouds WIDENED TO FLOAT64.  For float64 clouds that is the host route
    itself; for float32 clouds numpy evaluates norm / arctan2 / arcsin in float32, which no device routine reproduces bit for
    bit: a few points per 100 000 fall into a neighbouring pixel and about one depth in ten differs by one float32 ulp
    (DESIGN.md section 5u has the figures).  The pixel of a point
    whose float64 coordinate lies within about 1e-12 px of a pixel boundary depends on the library's atan2 / asin.
    `remission=` / `labels=` images depend on the order of equal depths on the host and are refused.  No fallback: without
    a GPU, or for a `device` that is not a CUDA(HIP) device, it raises; an empty list raises."""
    if remission is not None:
        raise NotImplementedError("preprocess_range_batch: `remission=` is not built on the device route (the host writes "
                                  "the feature of the last of equally deep points); use preprocess_range / pcd2range")
    if labels is not None:
        raise NotImplementedError("preprocess_range_batch: `labels=` is not built on the device route (the host writes the "
                                  "label of the last of equally deep points); use preprocess_range / pcd2range")
    clouds = list(clouds)
    if not clouds:
        raise ValueError("preprocess_range_batch: an empty batch")
    pts, offsets = KP.ragged([np.asarray(c) if not isinstance(c, torch.Tensor) else c for c in clouds], device)
    return KP.range_images(pts, offsets, cfg["size"], cfg["fov"], cfg["depth_range"])


def compute_range_logits(data_type, *sets, model=None, root=None, size=None, preprocess_device=None):
    """For every list of [N, 3] clouds in `sets` the float32 [n, 16 * 32 = 512] matrix of row-band means of RangeNet's
    decoder map over the clouds' range images (the reference's compute_logits for 'range'), MODAL2BATCHSIZE['range']
    clouds at a time.  The projection runs in numpy on the host.  `model`: a models.rangenet Model in eval mode on the
    GPU; None loads the pretrained one (build_model).  `size`: (H, W) instead of the dataset's image size.
    `preprocess_device`: None projects on the host, 'cuda' on the device a batch at a time (`preprocess_range_batch`: the
    host route's bits for float64 clouds, the host route of the widened cloud for float32 ones)."""
    from . import AGG_TYPE, DATASET_CONFIG, MODAL2BATCHSIZE, TYPE2DATASET, build_model

    assert data_type in ["32", "64"]
    check_preprocess_device(preprocess_device, need_gpu=False)
    if not torch.cuda.is_available():
        raise RuntimeError("compute_range_logits needs the MI355X: no CPU fallback on the hot path")
    cfg = dict(DATASET_CONFIG[TYPE2DATASET[data_type]])
    if size is not None:
        cfg["size"] = [int(size[0]), int(size[1])]
    if model is None:
        model = build_model(TYPE2DATASET[data_type], "rangenet", device="cuda", root=root)
    bs = MODAL2BATCHSIZE["range"]
    dev = next(model.parameters()).device
    pre = check_preprocess_device(preprocess_device)
    output = tuple()
    for data in sets:
        rows = []
        for i in range(math.ceil(len(data) / bs)):
            if pre is None:
                batch = np.stack([preprocess_range(np.asarray(pcd), **cfg) for pcd in data[i * bs:(i + 1) * bs]])
                x = torch.from_numpy(batch).float().to(dev)
            else:
                x = preprocess_range_batch(data[i * bs:(i + 1) * bs], dev, **cfg)
            with torch.no_grad():
                rows.append(model(x, return_final_logits=True, agg_type=AGG_TYPE))
        output += (np.vstack(rows) if rows else np.zeros((0, 0), np.float32),)
    return output
