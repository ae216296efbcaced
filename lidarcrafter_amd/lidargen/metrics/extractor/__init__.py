"""Learned feature extractors of the evaluation (mirror of the reference's `lidargen/metrics/extractor`): PointNet (FPD) and
RangeNet (FRD; `rangenet.rangenet53` / `rangenet21` / `build_rangenet`); PointMLP (the object scores and CGF) is
`extractor.pointmlp`, imported where it is used."""
from . import rangenet  # noqa: F401
from .pointnet import PointNet1, PointNetfeat, STN3d, pretrained_pointnet  # noqa: F401
