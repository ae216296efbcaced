"""Evaluation front-end on the device (SURVEY.md section 8f-3 ii): `bev`, `chamfer`, `emd`, `eval_utils.evaluate`, the
Frechet Point Distance (`extractor.pointnet`, `distribution`, `eval_utils.compute_fpd`), the Frechet Sparse Volume
Distance (`models.minkowskinet`, `metric_utils.compute_logits`, `eval_utils.compute_fsvd`; sparse 3-D convolution in
csrc/spconv.hip) and the Frechet Point-Voxel Distance (`models.spvcnn`, `metric_utils.compute_point_voxel_logits`,
`eval_utils.compute_fpvd`; point <-> voxel exchanges in csrc/spvoxel.hip) and the Frechet Range Image Distance
(`models.rangenet`, `metric_utils.compute_range_logits`, `eval_utils.compute_frid`; dense convolutions in
csrc/rangenet.hip), with its sibling FRD of the reference's own evaluator (`extractor.rangenet`, `eval_utils.compute_frd`),
and the object half: the PointMLP extractor (`extractor.pointmlp`; farthest point sampling, k nearest neighbours and grouped
dense layers in csrc/pointmlp.hip), `datasets.nuscenes_object_dataset.NuscObject`, `fg_object` and
`eval_utils.compute_obj_scores`, and RGF on the GLENet box sampler (`models.glenet`, `datasets.object_uncertainty_dataset`,
`fg_object.compute_rgf`; gathered trunk, rotated IoU and the score reduction in csrc/glenet.hip); the sequence metrics TTCE and
TCD (`temporal`; point-to-point ICP in csrc/icp.hip)."""
import os

# a score line as the reference prints it: a 50-column rule above and below `|<16 blanks>NAME:1.2345E+00<17 blanks>|`
_RULE = "-" * 50
OUTPUT_TEMPLATE = f"{_RULE}\n|{'':16}{{}}:{{:.4E}}{'':17}|\n{_RULE}"

# the reference's settings (lidargen/metrics/__init__.py:23-36)
DEFAULT_ROOT = "../pretrained_models/evaluation"
MODAL2BATCHSIZE = {"range": 100, "voxel": 50, "point_voxel": 25}
VOXEL_SIZE = 0.05
NUM_SECTORS = 16
AGG_TYPE = "depth"
TYPE2DATASET = {"32": "nuscenes", "64": "kitti"}
MODALITY2MODEL = {"range": "rangenet", "voxel": "minkowskinet", "point_voxel": "spvcnn"}
DATASET_CONFIG = {"kitti": {"size": [64, 1024], "fov": [3, -25], "depth_range": [1.0, 56.0], "depth_scale": 6},
                  "nuscenes": {"size": [32, 1024], "fov": [10, -30], "depth_range": [1.0, 45.0]}}


def _load_pretrained(who, dataset_name, model_name, model_cls, device, root):
    """`model_cls(config.yaml)` with `model.ckpt`'s state dict from <root>/<dataset_name>/<model_name>/, in eval mode on
    `device`; `who` names the caller in the errors."""
    import torch
    import yaml

    folder = os.path.join(DEFAULT_ROOT if root is None else os.fspath(root), dataset_name, model_name)
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"{who}: no pretrained weights folder at {folder} -- place the reference's "
                                "config.yaml and model.ckpt there or pass root=<path>; this build does not fetch them")
    paths = [os.path.join(folder, n) for n in ("config.yaml", "model.ckpt")]
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(f"{who}: {p} is missing; this build does not fetch it")
    with open(paths[0], "r") as f:
        model = model_cls(yaml.safe_load(f))
    state = torch.load(paths[1], map_location="cpu", weights_only=False)["state_dict"]
    own = model.state_dict()
    missing = [k for k in own if k not in state]
    if missing:
        raise KeyError(f"{who}: {paths[1]} lacks {len(missing)} keys of the model, the first: {missing[:4]}")
    model.load_state_dict({k: state[k] for k in own})
    model.eval().requires_grad_(False)
    return model.to(device)


def _load_rangenet(dataset_name, device, root):
    import yaml

    from .models.rangenet.model import Model

    folder = os.path.join(DEFAULT_ROOT if root is None else os.fspath(root), dataset_name, "rangenet")
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"build_model: no pretrained weights folder at {folder} -- place the reference's "
                                "config.yaml, backbone and segmentation_decoder there or pass root=<path>; this build "
                                "does not fetch them")
    for n in ("config.yaml", "backbone", "segmentation_decoder"):
        if not os.path.isfile(os.path.join(folder, n)):
            raise FileNotFoundError(f"build_model: {os.path.join(folder, n)} is missing; this build does not fetch it")
    with open(os.path.join(folder, "config.yaml"), "r") as f:
        model = Model(yaml.safe_load(f))
    model.load_pretrained_weights(folder)
    model.eval().requires_grad_(False)
    return model.to(device)


def build_model(dataset_name, model_name, device="cpu", root=None):
    """The pretrained extractor `model_name` of `dataset_name` from <root>/<dataset_name>/<model_name>/{config.yaml,
    model.ckpt} (root: DEFAULT_ROOT), in eval mode on `device`.  'minkowskinet' is built here and 'rangenet' (config.yaml
    and the state dicts `backbone` and `segmentation_decoder` of its folder); 'spvcnn' has its own loader,
    models.spvcnn.pretrained.  Nothing is fetched: a missing folder or file raises FileNotFoundError naming the
    path.  Unlike the reference's `strict=False` a model key missing from the checkpoint raises; keys the model does not
    have are ignored."""
    if model_name == "spvcnn":
        raise NotImplementedError("build_model: 'spvcnn' is not dispatched from here; the extractor of FPVD is loaded by "
                                  "models.spvcnn.pretrained(dataset_name, device, root)")
    if model_name == "rangenet":
        return _load_rangenet(dataset_name, device, root)
    if model_name != "minkowskinet":
        raise NotImplementedError(f"build_model: '{model_name}' is not built (only 'minkowskinet', the extractor of FSVD, "
                                  "and 'rangenet', the extractor of FRID)")
    from .models.minkowskinet.model import Model

    return _load_pretrained("build_model", dataset_name, model_name, Model, device, root)


from . import bev, chamfer, distribution, emd, eval_utils, extractor, models  # noqa: E402,F401
