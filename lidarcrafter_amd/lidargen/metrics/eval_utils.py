"""Evaluation front-end -- mirror of the reference's `lidargen/metrics/eval_utils.py`: `evaluate(reference, samples,
metrics, data)` and the weight-free scores behind it (`compute_cd` :40-51, `compute_emd` :54-65, `compute_mmd` :68-82,
`compute_jsd` :85-95).  Every score is printed through the reference's OUTPUT_TEMPLATE and also returned; `evaluate`
returns {metric: score}.  Of the perceptual metrics FSVD and FPVD are built (`compute_fd` :98-102, `compute_fsvd` :116-124:
MinkUNet features, sparse convolution in csrc/spconv.hip; `compute_fpvd` :127-135: SPVCNN features, point <-> voxel
exchanges in csrc/spvoxel.hip) and FRID (`compute_frid` :105-113: RangeNet features of range images, dense convolutions
in csrc/rangenet.hip).  `evaluate` still refuses all three and 'mmd' (its callers rely on that): call `compute_frid` /
`compute_fsvd` / `compute_fpvd` / `compute_mmd` directly.

`extract_point_features` / `compute_fpd` are the Frechet Point Distance of the reference's own evaluator
(tools/evaluation/evaluate_our.py `EvaluationEngine`: PointNet1 features of every cloud, `distribution.
compute_frechet_distance` on the two feature sets); `extract_range_features` / `compute_frd` are its FRD (RangeNet
'lidargen' features of 5-channel range images).  `evaluate` does not dispatch them."""
from __future__ import annotations

import numpy as np
import torch

from . import OUTPUT_TEMPLATE
from . import distribution, metric_utils
from .chamfer import bev_min_matching, compute_pairwise_cd
from .emd import compute_pairwise_emd_batch

_NOT_BUILT = {"frid": "a direct call of eval_utils.compute_frid(reference, samples, data)",
              "fpvd": "a direct call of eval_utils.compute_fpvd(reference, samples, data)",
              "fsvd": "a direct call of eval_utils.compute_fsvd(reference, samples, data)",
              "mmd": "a direct call of eval_utils.compute_mmd(reference, samples, data)"}


def evaluate(reference, samples, metrics, data):
    scores = {}
    for m in ("frid", "fsvd", "fpvd"):   # perceptual
        if m in metrics:
            raise NotImplementedError(f"evaluate: metric '{m}' is not dispatched from here; it needs {_NOT_BUILT[m]}")
    if "mmd" in metrics:
        raise NotImplementedError(f"evaluate: metric 'mmd' is not dispatched from here; it needs {_NOT_BUILT['mmd']}")
    # reconstruction
    if "cd" in metrics:
        scores["cd"] = compute_cd(reference, samples)
    if "emd" in metrics:
        scores["emd"] = compute_emd(reference, samples)
    # statistical
    if "jsd" in metrics:
        scores["jsd"] = compute_jsd(reference, samples, data)
    return scores


def compute_cd(reference, samples):
    """Score of Chamfer Distance (CD): the mean over the pairs."""
    print("Evaluating (CD) ...")
    results = [compute_pairwise_cd(x, y) for x, y in zip(reference, samples)]
    score = sum(results) / len(results)
    print(OUTPUT_TEMPLATE.format("CD  ", score))
    return score


def compute_emd(reference, samples):
    """Score of Earth Mover's Distance (EMD): the mean over the pairs, pairs of one length in one launch."""
    print("Evaluating (EMD) ...")
    results = compute_pairwise_emd_batch(list(reference), list(samples))
    score = sum(results) / len(results)
    print(OUTPUT_TEMPLATE.format("EMD ", score))
    return score


def compute_mmd(reference, samples, data, dist="cd", verbose=True):
    """Score of Minimum Matching Distance (MMD): the mean over the reference clouds of the smallest chamfer distance
    between the cloud's BEV cell set and a sample's.  `verbose` is accepted for the reference's signature (its progress
    bar has nothing to show: the references are not looped over on the host)."""
    print("Evaluating (MMD) ...")
    assert dist in ["cd", "emd"]
    if dist == "emd":
        raise NotImplementedError("compute_mmd: dist='emd' is not built (the reference's own call on that branch passes a "
                                  "list where compute_pairwise_emd needs an array)")
    cfg = metric_utils.DATA_CONFIG[data]
    results, _ = bev_min_matching(reference, samples, cfg["x"], cfg["y"], 0.5)
    score = float(sum(results.tolist()) / len(results))
    print(OUTPUT_TEMPLATE.format("MMD ", score))
    return score


def compute_jsd(reference, samples, data):
    """Score of Jensen-Shannon Divergence (JSD) of the BEV occupancy sums."""
    print("Evaluating (JSD) ...")
    score = metric_utils.compute_jsd(reference, samples, data)
    print(OUTPUT_TEMPLATE.format("JSD ", score))
    return score


def _cloud_cm(a, scale):
    """[N,3] array or tensor -> CUDA float32 [3,N] scaled (the evaluator's `xyz / DATASET_MAX_DEPTH`, channel-major)."""
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("extract_point_features needs the MI355X: no CPU fallback on the hot path")
        a = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    elif not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise RuntimeError("extract_point_features: tensors must be CUDA(HIP) tensors -- no CPU fallback on the hot path")
    if a.dim() != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"extract_point_features: a cloud must be [N, 3] with N >= 1, got {tuple(a.shape)}")
    return (a.float() * scale).t()


def extract_point_features(model, clouds, batch_size=16, scale=1 / 80.0):
    """Features of `model` (extractor.PointNet1, eval mode, on the GPU) for a list of [N,3] clouds -> [n, width] float64
    numpy array in input order.  Clouds of one length go through the model together, `batch_size` at a time; `scale`
    multiplies the coordinates first."""
    clouds = list(clouds)
    by_len = {}
    for i, c in enumerate(clouds):
        by_len.setdefault(int(c.shape[0]), []).append(i)
    rows = [None] * len(clouds)
    for idx in by_len.values():
        for lo in range(0, len(idx), batch_size):
            part = idx[lo:lo + batch_size]
            x = torch.stack([_cloud_cm(clouds[i], scale) for i in part]).contiguous()
            f = model(x).double().cpu().numpy()
            for row, i in enumerate(part):
                rows[i] = f[row]
    return np.stack(rows) if rows else np.zeros((0, 0))


def _stats(stats_device, key="device"):
    """Keyword for the functions of `distribution` (or, as `stats_device`, for compute_fd): nothing for the host route (the
    default, so those calls stay as they were), the device for the float64 kernels (distribution's docstring)."""
    return {} if stats_device is None else {key: stats_device}


def _as_features(a, model, batch_size):
    if isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[1] != 3:
        return a                                    # already a feature matrix (the evaluator caches the real set's)
    return extract_point_features(model, a, batch_size)


def compute_fpd(reference, samples, model, batch_size=16, columns=None, stats_device=None):
    """Score of Frechet Point Distance (FPD): the Frechet distance of the PointNet features of the two sets.  Either set
    may be a feature matrix ([n, width] numpy array) instead of a list of clouds.  `columns` (a slice or index array)
    restricts the distance to those feature columns.  `stats_device`: None the host statistics, 'cuda' the device route."""
    print("Evaluating (FPD) ...")
    fr, fs = _as_features(reference, model, batch_size), _as_features(samples, model, batch_size)
    if columns is not None:
        fr, fs = fr[:, columns], fs[:, columns]
    score = distribution.compute_frechet_distance(fr, fs, **_stats(stats_device))
    print(OUTPUT_TEMPLATE.format("FPD ", score))
    return score


def compute_fd(reference, samples, stats_device=None):
    """Frechet distance of two feature matrices as the reference's evaluator computes it (eval_utils.py:98-102).
    `stats_device`: None the host statistics; 'cuda' the device route on the feature matrices themselves."""
    if stats_device is not None:
        return distribution.compute_frechet_distance(reference, samples, device=stats_device)
    mu1, mu2 = np.mean(reference, axis=0), np.mean(samples, axis=0)
    sigma1, sigma2 = np.cov(reference, rowvar=False), np.cov(samples, rowvar=False)
    return distribution.calculate_frechet_distance(mu1, sigma1, mu2, sigma2)


def compute_fsvd(reference, samples, data, model=None, stats_device=None, preprocess_device=None):
    """Score of Frechet Sparse Volume Distance (FSVD): the Frechet distance of the depth-sector means of the MinkUNet
    features of the two sets of [N, 3] clouds.  `model`: the extractor to use instead of the pretrained one.
    `preprocess_device`: None quantizes the clouds on the host, 'cuda' a batch at a time on the device (the same bits)."""
    print("Evaluating (FSVD) ...")
    gt_logits, samples_logits = metric_utils.compute_logits(data, "voxel", reference, samples, model=model,
                                                            preprocess_device=preprocess_device)
    score = compute_fd(gt_logits, samples_logits, **_stats(stats_device, "stats_device"))
    print(OUTPUT_TEMPLATE.format("FSVD", score))
    return score


def compute_fpvd(reference, samples, data, model=None, stats_device=None, preprocess_device=None):
    """Score of Frechet Point-Voxel Distance (FPVD): the Frechet distance of the depth-sector means of the SPVCNN
    features of the two sets of [N, 3] clouds.  `model`: the extractor to use instead of the pretrained one.
    `preprocess_device`: as for `compute_fsvd`."""
    print("Evaluating (FPVD) ...")
    gt_logits, samples_logits = metric_utils.compute_point_voxel_logits(data, reference, samples, model=model,
                                                                        preprocess_device=preprocess_device)
    score = compute_fd(gt_logits, samples_logits, **_stats(stats_device, "stats_device"))
    print(OUTPUT_TEMPLATE.format("FPVD", score))
    return score


def compute_frid(reference, samples, data, model=None, size=None, stats_device=None, preprocess_device=None):
    """Score of Frechet Range Image Distance (FRID): the Frechet distance of the row-band means of RangeNet's decoder map
    over the range images of the two sets of [N, 3] clouds.  `model`: the extractor to use instead of the pretrained one;
    `size`: (H, W) of the range images instead of the dataset's.  `preprocess_device`: None projects the clouds on the host,
    'cuda' a batch at a time on the device -- the host's bits for float64 clouds, the host route of the cloud widened to
    float64 for float32 ones (metric_utils.preprocess_range_batch)."""
    print("Evaluating (FRID) ...")
    gt_logits, samples_logits = metric_utils.compute_range_logits(data, reference, samples, model=model, size=size,
                                                                  preprocess_device=preprocess_device)
    score = compute_fd(gt_logits, samples_logits, **_stats(stats_device, "stats_device"))
    print(OUTPUT_TEMPLATE.format("FRID", score))
    return score


def extract_range_features(model, preprocess, imgs, masks=None, batch_size=16):
    """'lidargen' features of `model` (extractor.rangenet.RangeNet, eval mode, on the GPU) for [n, C, H, W] range images
    (a CUDA tensor or a numpy array; `masks` [n, 1, H, W] or None) -> [n, 4096] float64 numpy array, `batch_size` images
    at a time through `preprocess` (extractor.rangenet.Preprocess; None: the images as they are)."""
    if isinstance(imgs, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("extract_range_features needs the MI355X: no CPU fallback on the hot path")
        imgs = torch.from_numpy(np.ascontiguousarray(imgs, np.float32)).cuda()
    elif not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
        raise RuntimeError("extract_range_features: tensors must be CUDA(HIP) tensors -- no CPU fallback on the hot path")
    if masks is not None:
        masks = torch.as_tensor(masks).to(imgs.device).float()
    rows = []
    with torch.no_grad():
        for lo in range(0, imgs.shape[0], batch_size):
            x = imgs[lo:lo + batch_size].float()
            if preprocess is not None:
                x = preprocess(x, None if masks is None else masks[lo:lo + batch_size])
            rows.append(model(x, feature="lidargen").double().cpu().numpy())
    return np.concatenate(rows) if rows else np.zeros((0, 0))


def compute_frd(reference, samples, model, preprocess=None, batch_size=16, columns=None, stats_device=None):
    """Score of Frechet Range Distance (FRD) of the reference's own evaluator: the Frechet distance of the RangeNet
    'lidargen' features of the two sets of range images.  Either set may be a feature matrix ([n, width] numpy array)
    instead of [n, C, H, W] images.  `columns` (a slice or index array) restricts the distance to those feature columns."""
    print("Evaluating (FRD) ...")
    feats = [a if isinstance(a, np.ndarray) and a.ndim == 2 else extract_range_features(model, preprocess, a,
                                                                                         batch_size=batch_size)
             for a in (reference, samples)]
    if columns is not None:
        feats = [f[:, columns] for f in feats]
    score = distribution.compute_frechet_distance(feats[0], feats[1], **_stats(stats_device))
    print(OUTPUT_TEMPLATE.format("FRD ", score))
    return score


def compute_obj_scores(real_set, gen_set, class_name="car", stats_device=None):
    """The evaluator's 'obj' block (tools/evaluation/evaluate_our.py:424-439) on two object sets of
    `fg_object.get_fg_object_set_feature`: {'frechet_distance', 'squared_mmd'} of the PointMLP features and {'jsd', 'mmd'} of
    the object BEV histograms of `class_name`.  One score line per number.  `stats_device`: None the host statistics, 'cuda'
    the device route for the first two."""
    from . import bev

    real, gen = real_set[class_name], gen_set[class_name]
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    hists = [torch.from_numpy(np.asarray(s["bev_hists"])).to(dev).float() for s in (real, gen)]
    out = {"frechet_distance": float(distribution.compute_frechet_distance(real["pts_feat"], gen["pts_feat"], **_stats(stats_device))),
           "squared_mmd": float(distribution.compute_squared_mmd(real["pts_feat"], gen["pts_feat"], **_stats(stats_device))),
           "jsd": float(bev.compute_jsd_2d(*hists)),
           "mmd": float(bev.compute_mmd_2d(*hists))}
    for name, key in (("OFD ", "frechet_distance"), ("OMMD", "squared_mmd"), ("OJSD", "jsd"), ("OBMD", "mmd")):
        print(OUTPUT_TEMPLATE.format(name, out[key]))
    return out
