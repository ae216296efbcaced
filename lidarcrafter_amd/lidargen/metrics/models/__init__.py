"""Pretrained feature extractors of the perceptual scores (the reference's `lidargen/metrics/models`): MinkowskiNet for
FSVD, SPVCNN for FPVD.  RangeNet (FRID) is not built."""
from . import spvcnn  # noqa: E402,F401  (models.spvcnn.pretrained)
