"""GLENet box sampler of the RGF object metric -- mirror of the reference's `lidargen/metrics/models/glenet`: `point_net`
(PointNetfeat, SimPointNetfeat), `model` (Encoder_x, Encoder_xy, Object_feat_encoder, Generator) and `eval_utils` (iou3d).
Inference only; kernels in csrc/glenet.hip."""
from . import eval_utils, model, point_net  # noqa: F401
from .model import DEFAULT_MODEL_CFG, Generator  # noqa: F401
