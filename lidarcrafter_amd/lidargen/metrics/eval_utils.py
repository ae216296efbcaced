"""Evaluation front-end -- mirror of the reference's `lidargen/metrics/eval_utils.py`: `evaluate(reference, samples,
metrics, data)` and the weight-free scores behind it (`compute_cd` :40-51, `compute_emd` :54-65, `compute_jsd` :85-95).
Every score is printed through the reference's OUTPUT_TEMPLATE and also returned; `evaluate` returns {metric: score}.
The perceptual metrics (FRID / FSVD / FPVD: pretrained extractors) and MMD (`pcd2bev_bin`) are not built here and raise."""
from __future__ import annotations

from . import OUTPUT_TEMPLATE
from . import metric_utils
from .chamfer import compute_pairwise_cd
from .emd import compute_pairwise_emd_batch

_NOT_BUILT = {"frid": "the pretrained range-image extractor", "fsvd": "the pretrained sparse-volume extractor",
              "fpvd": "the pretrained point-voxel extractor", "mmd": "pcd2bev_bin"}


def evaluate(reference, samples, metrics, data):
    scores = {}
    for m in ("frid", "fsvd", "fpvd"):   # perceptual
        if m in metrics:
            raise NotImplementedError(f"evaluate: metric '{m}' needs {_NOT_BUILT[m]}, which this build does not have")
    if "mmd" in metrics:
        raise NotImplementedError(f"evaluate: metric 'mmd' needs {_NOT_BUILT['mmd']}, which this build does not have")
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


def compute_jsd(reference, samples, data):
    """Score of Jensen-Shannon Divergence (JSD) of the BEV occupancy sums."""
    print("Evaluating (JSD) ...")
    score = metric_utils.compute_jsd(reference, samples, data)
    print(OUTPUT_TEMPLATE.format("JSD ", score))
    return score
