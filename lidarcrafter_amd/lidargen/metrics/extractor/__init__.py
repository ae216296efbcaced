"""Learned feature extractors of the evaluation (mirror of the reference's `lidargen/metrics/extractor`): PointNet only."""
from .pointnet import PointNet1, PointNetfeat, STN3d, pretrained_pointnet  # noqa: F401
