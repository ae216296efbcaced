"""RangeNet++ (DarkNet-21 / -53), the extractor of the Frechet Range Image Distance: `model.Model` under the reference's
state-dict names, `plan.Plan` the forward both module trees run."""
from .model import Backbone, BasicBlock, Decoder, Model  # noqa: F401
