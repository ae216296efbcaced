"""Front-end of the object scores and CGF -- mirror of the reference's `lidargen/metrics/fg_object.py` for the parts that rest
on the PointMLP extractor (`extractor.pointmlp`) and for the pure host code next to them.  The
functions take what the reference builds inside them from a method name (loader, network) as arguments.  RGF, the
regression fidelity, rests on the GLENet box sampler (`models.glenet`): `pretrained_glenet`,
`compute_rgf_fold` (all draws of a fold in one batched plan, scored on the device), `compute_rgf_from_results` (the
reference's fixed-bin table without pandas) and `compute_rgf` over the folds.  The detector behind DCF's input is not
built; the sklearn / pandas per-class tables are left out."""
import os
from collections import defaultdict

import numpy as np
import torch

from . import bev
from .extractor.pointmlp import pointMLP
from .models.glenet.model import DEFAULT_MODEL_CFG, Generator

FIXED_BINS = (0, 100, 200, 300, 400, 500, np.inf)
FIXED_LABELS = ("<100", "100-200", "200-300", "300-400", "400-500", ">500")
RGF_BINS = (0, 150, 300, np.inf)
RGF_LABELS = ("<150", "150-300", ">300")


def pretrained_pointmlp(checkpoint, device="cuda", num_classes=4):
    """pointMLP(num_classes) with `checkpoint['net']` (a `module.` prefix of DataParallel is stripped), in eval mode on
    `device`.  The file is never fetched: when it is absent this raises FileNotFoundError naming the path."""
    path = os.fspath(checkpoint)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"pretrained_pointmlp: no checkpoint at {path} -- place the reference's "
                                "nusc_object_classification_model.pth there; this build does not fetch it")
    state = torch.load(path, map_location="cpu", weights_only=False)["net"]
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    net = pointMLP(num_classes=num_classes)
    net.load_state_dict(state)
    net.eval().requires_grad_(False)
    return net.to(device)


def _device_of(net):
    return next(net.parameters()).device


def get_fg_object_set_feature(loader, net, class_names=("car", "truck", "bus")):
    """{class: {'pts_feat': [n,1024], 'bev_hists': [n,100,100]}} over the batches (data [b,N,3], label [b], points in gt)
    of `loader`; label 0 is collected under 'unkonw' as lists, as the reference leaves it."""
    names = ["unkonw"] + list(class_names)
    out = {n: defaultdict(list) for n in names}
    dev = _device_of(net)
    with torch.no_grad():
        for data, label, _ in loader:
            data = torch.as_tensor(data).to(dev).float()
            label = np.asarray(torch.as_tensor(label).cpu()).reshape(-1)
            feats = net(data.permute(0, 2, 1), return_features=True).cpu()
            for i in range(data.shape[0]):
                name = names[int(label[i])]
                out[name]["pts_feat"].append(feats[i])
                out[name]["bev_hists"].append(
                    bev.point_cloud_to_histogram(data[i], min_depth=1e-6, max_depth=1e3, field_size=2.0).cpu())
    for name, d in out.items():
        if name == "unkonw":
            continue
        for key, empty in (("pts_feat", (0, 1024)), ("bev_hists", (0, 100, 100))):
            d[key] = torch.stack(d[key], dim=0).numpy() if len(d[key]) else np.zeros(empty, np.float32)
    return out


def validate_classification(net, loader, class_names=None):
    """{'class_names', 'test_true', 'test_pred', 'num_points_in_gt'} over `loader` (the reference's result dict)."""
    if class_names is None:
        class_names = list(loader.dataset.class_name)
    dev = _device_of(net)
    true, pred, pts = [], [], []
    with torch.no_grad():
        for data, label, n in loader:
            data = torch.as_tensor(data).to(dev).float()
            logits = net(data.permute(0, 2, 1))
            true.append(np.asarray(torch.as_tensor(label).cpu()).reshape(-1))
            pred.append(logits.max(dim=1)[1].cpu().numpy())
            pts.append(np.asarray(torch.as_tensor(n).cpu()).reshape(-1))
    return {"class_names": ["unknow"] + list(class_names), "test_true": np.concatenate(true),
            "test_pred": np.concatenate(pred), "num_points_in_gt": np.concatenate(pts)}


def compute_cgf_from_results(result_dict, bins=None):
    """{'overall': {'accuracy'}, 'partitions': {label: {'accuracy', 'count'}}}: the overall accuracy and the accuracy per
    fixed bin of the object's point count (pandas.cut with include_lowest: [0, 100], (100, 200], ... (500, inf)); empty
    bins are left out, as the reference skips them."""
    bins = list(FIXED_BINS if bins is None else bins)
    labels = list(FIXED_LABELS) if len(bins) == len(FIXED_BINS) else [f"({bins[i]}, {bins[i + 1]}]" for i in range(len(bins) - 1)]
    y_true, y_pred = np.asarray(result_dict["test_true"]), np.asarray(result_dict["test_pred"])
    pts = np.asarray(result_dict["num_points_in_gt"])
    out = {"overall": {"accuracy": float(np.mean(y_true == y_pred))}, "partitions": {}}
    for i, lbl in enumerate(labels):
        lo, hi = bins[i], bins[i + 1]
        mask = ((pts >= lo) if i == 0 else (pts > lo)) & (pts <= hi)
        if mask.any():
            out["partitions"][lbl] = {"accuracy": float(np.mean(y_true[mask] == y_pred[mask])), "count": int(mask.sum())}
    return out


def compute_dcf(detection_results_dict):
    """{class: mean detection score rounded to 4 places} over the 'car', 'truck', 'bus', 'pedestrian' entries, keyed by
    every detection's own name."""
    scores = defaultdict(list)
    for class_name, infos in detection_results_dict.items():
        if class_name in ("car", "truck", "bus", "pedestrian"):
            for det in infos:
                scores[det["name"]].append(det["score"])
    print("Average confidence per class:")
    out = {}
    for cls, vals in scores.items():
        avg = np.mean(vals)
        print(f"{cls}: {avg:.6f}")
        out[cls] = float(round(avg, 4))
    return out


def pretrained_glenet(checkpoint, model_cfg=None, device="cuda"):
    """Generator(model_cfg or exp20.yaml's MODEL block, input_channels, scale=1) with `checkpoint['model_state']` loaded
    strictly, in eval mode on `device`.  The file is never fetched: when it is absent this raises FileNotFoundError naming
    the path."""
    path = os.fspath(checkpoint)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"pretrained_glenet: no checkpoint at {path} -- place the reference's "
                                "nusc_object_uncertainty_model.pth there; this build does not fetch it")
    cfg = DEFAULT_MODEL_CFG if model_cfg is None else model_cfg
    state = torch.load(path, map_location="cpu", weights_only=False)["model_state"]
    net = Generator(cfg, input_channels=cfg["INPUT_CHANNELS"] if "INPUT_CHANNELS" in cfg else 4, scale=1)
    net.load_state_dict(state, strict=True)
    net.eval().requires_grad_(False)
    return net.to(device)


def compute_rgf_fold(dataset, net, draws=30, generator=None, batch_size=2048):
    """{key: {'variance' [7], 'overlap', 'pointnum'}} over the objects of `dataset` (datasets.object_uncertainty_dataset.
    NuscObjUncertainty): `draws` boxes per object from `net` (Generator.sample_boxes, every draw with its own 512 indices
    from the dataset's generator and its own eps from `generator`, a torch.Generator; default: seed 0), decoded and scored
    against the object's box on the device (ops_glenet.glenet_score): the variance over the draws of the seven box columns,
    the heading as the sine of its offset from the gt heading, and the mean IoU.  What the reference spreads over `draws`
    evaluation runs, their pickles and single_fold_data."""
    from lidarcrafter_amd import ops_glenet as KG

    dev = _device_of(net)
    if generator is None:
        generator = torch.Generator().manual_seed(0)
    out = {}
    for batch in dataset.batches(batch_size):
        B = len(batch["key"])
        counts = np.diff(batch["offsets"])
        choice = torch.from_numpy(dataset.choice(counts, draws)).to(dev)
        eps = torch.randn((draws, B, net.latent_dim), generator=generator, dtype=torch.float32).to(dev)
        box = net.sample_boxes(torch.from_numpy(batch["points"]).to(dev), torch.from_numpy(batch["offsets"]).to(dev),
                               torch.from_numpy(batch["text_feat"]).to(dev), choice, eps)
        _, _, variance, mean_overlap = KG.glenet_score(box, torch.from_numpy(batch["gt_boxes"]).to(dev))
        variance, mean_overlap = variance.cpu().numpy(), mean_overlap.cpu().numpy()
        for i, key in enumerate(batch["key"]):
            out[key] = {"variance": variance[i], "overlap": float(mean_overlap[i]), "pointnum": batch["num_points_in_gt"][i]}
    return out


def compute_rgf_from_results(result_json, bins=None):
    """{'overall': {'variance' [7], 'overlap'}, 'partitions': {label: {'variance', 'overlap'}}}: the reference's
    compute_regression_metrics_fixed_bins without pandas -- the means over all objects and per fixed bin of the object's
    point count (pandas.cut with include_lowest: [0, 150], (150, 300], (300, inf)); empty bins are skipped; prints what the
    reference prints."""
    bins = list(RGF_BINS if bins is None else bins)
    labels = list(RGF_LABELS)
    rows = list(result_json.values())
    for r in rows:
        assert {"variance", "overlap", "pointnum"}.issubset(r.keys()), "every entry needs variance, overlap, pointnum"
    var = np.stack([np.asarray(r["variance"], np.float64) for r in rows])
    ov = np.asarray([r["overlap"] for r in rows], np.float64)
    pts = np.asarray([r["pointnum"] for r in rows])
    overall_var, overall_overlap = var.mean(axis=0), ov.mean()
    print(f"整体 variance 均值: {overall_var}")
    print(f"整体 overlap 均值:  {overall_overlap:.4f}\n")
    partitions = {}
    for i, lbl in enumerate(labels):
        lo, hi = bins[i], bins[i + 1]
        mask = ((pts >= lo) if i == 0 else (pts > lo)) & (pts <= hi)
        if not mask.any():
            print(f"分区 {lbl}: 无样本，已跳过\n")
            continue
        var_mean, overlap_mean = var[mask].mean(axis=0), ov[mask].mean()
        print(f"分区 {lbl} (样本数 {int(mask.sum())}):")
        print(f"  variance 均值: {var_mean}")
        print(f"  overlap 均值:  {overlap_mean:.4f}\n")
        partitions[lbl] = {"variance": var_mean.tolist(), "overlap": overlap_mean}
    return {"overall": {"variance": overall_var.tolist(), "overlap": overall_overlap}, "partitions": partitions}


def compute_rgf(datasets_by_fold, nets_by_fold, draws=30, generator=None):
    """The RGF table over the folds: compute_rgf_fold of every (dataset, net) pair -- a single net serves every fold -- merged
    by key, then compute_rgf_from_results.  The keys are the objects' indices in the fold's source list: the datasets must be
    folds of ONE list (`fold_idx` = 0 ... 9), and a key that two datasets share raises ValueError instead of overwriting an
    object.  One `generator` runs through all folds; with generator=None every fold draws its eps from seed 0 again."""
    datasets_by_fold = list(datasets_by_fold)
    nets = list(nets_by_fold) if isinstance(nets_by_fold, (list, tuple)) else [nets_by_fold] * len(datasets_by_fold)
    if len(nets) != len(datasets_by_fold):
        raise ValueError(f"compute_rgf: {len(datasets_by_fold)} datasets and {len(nets)} networks")
    result_json = {}
    for dataset, net in zip(datasets_by_fold, nets):
        fold = compute_rgf_fold(dataset, net, draws=draws, generator=generator)
        shared = result_json.keys() & fold.keys()
        if shared:
            raise ValueError(f"compute_rgf: {len(shared)} object keys occur in two datasets (e.g. {sorted(shared)[0]!r}) -- the "
                             "datasets must be folds of one list")
        result_json.update(fold)
    return compute_rgf_from_results(result_json)
