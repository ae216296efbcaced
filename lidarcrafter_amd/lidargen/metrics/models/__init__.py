"""Pretrained feature extractors of the perceptual scores (the reference's `lidargen/metrics/models`): MinkowskiNet for
FSVD.  RangeNet (FRID) and SPVCNN (FPVD) are not built."""
