"""Pretrained feature extractors of the perceptual scores (the reference's `lidargen/metrics/models`): MinkowskiNet for
FSVD, SPVCNN for FPVD, RangeNet for FRID (`models.rangenet`; dense convolutions in csrc/rangenet.hip), GLENet for RGF (`models.glenet`; csrc/glenet.hip)."""
from . import rangenet  # noqa: E402,F401
from . import spvcnn  # noqa: E402,F401  (models.spvcnn.pretrained)
from . import glenet  # noqa: E402,F401  (models.glenet.Generator)
