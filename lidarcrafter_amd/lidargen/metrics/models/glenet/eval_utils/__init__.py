"""`glenet.eval_utils`: the paired rotated 3-D IoU of the reference's eval_utils/eval_utils.py."""
from . import eval_utils  # noqa: F401
from .eval_utils import iou3d  # noqa: F401
