"""Front-end of the object scores and CGF -- mirror of the reference's `lidargen/metrics/fg_object.py` for the parts that rest
on the PointMLP extractor (`extractor.pointmlp`) and for the pure host code next to them.  The
functions take what the reference builds inside them from a method name (loader, network) as arguments.  GLENet / RGF and
the detector behind DCF's input are not built; the sklearn / pandas per-class tables are left out."""
import os
from collections import defaultdict

import numpy as np
import torch

from . import bev
from .extractor.pointmlp import pointMLP

FIXED_BINS = (0, 100, 200, 300, 400, 500, np.inf)
FIXED_LABELS = ("<100", "100-200", "200-300", "300-400", "400-500", ">500")


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
