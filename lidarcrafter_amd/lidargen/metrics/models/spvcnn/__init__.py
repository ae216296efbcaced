"""SPVCNN feature extractor of the Frechet Point-Voxel Distance: `model.Model` and `pretrained`."""


def pretrained(dataset_name, device="cuda", root=None):
    """The pretrained SPVCNN of `dataset_name` from <root>/<dataset_name>/spvcnn/{config.yaml, model.ckpt} (root: the
    metrics package's DEFAULT_ROOT), in eval mode on `device`, by build_model's rules: nothing is fetched, a missing folder
    or file raises FileNotFoundError naming the path, a model key missing from the checkpoint raises KeyError."""
    from ... import _load_pretrained
    from .model import Model

    return _load_pretrained("models.spvcnn.pretrained", dataset_name, "spvcnn", Model, device, root)
