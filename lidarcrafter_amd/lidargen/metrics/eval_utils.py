"""Evaluation front-end -- mirror of the reference's `lidargen/metrics/eval_utils.py`: `evaluate(reference, samples,
metrics, data)` and the weight-free scores behind it (`compute_cd` :40-51, `compute_emd` :54-65, `compute_mmd` :68-82,
`compute_jsd` :85-95).  Every score is printed through the reference's OUTPUT_TEMPLATE and also returned; `evaluate`
returns {metric: score}.  The perceptual metrics (FRID / FSVD / FPVD: pretrained extractors) are not built here and raise;
`evaluate` also still refuses 'mmd' (its callers rely on that): call `compute_mmd` directly."""
from __future__ import annotations

from . import OUTPUT_TEMPLATE
from . import metric_utils
from .chamfer import bev_min_matching, compute_pairwise_cd
from .emd import compute_pairwise_emd_batch

_NOT_BUILT = {"frid": "the pretrained range-image extractor", "fsvd": "the pretrained sparse-volume extractor",
              "fpvd": "the pretrained point-voxel extractor",
              "mmd": "a direct call of eval_utils.compute_mmd(reference, samples, data)"}


def evaluate(reference, samples, metrics, data):
    scores = {}
    for m in ("frid", "fsvd", "fpvd"):   # perceptual
        if m in metrics:
            raise NotImplementedError(f"evaluate: metric '{m}' needs {_NOT_BUILT[m]}, which this build does not have")
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
