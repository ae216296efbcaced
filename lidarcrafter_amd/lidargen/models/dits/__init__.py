"""Diffusion transformers (reference lidargen/models/dits/__init__.py): the Hourglass Diffusion Transformer."""
from .hdit import HDiT

__all__ = {
    "hdit": HDiT,
}
