"""Flow-matching generators (reference lidargen/models/flows/__init__.py): the MeanFlow sampler."""
from .mean_flow import MeanFlow

__all__ = {
    "mean": MeanFlow,
}
