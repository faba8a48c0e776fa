"""Training of the heatmap head on frozen trunk features."""
from .trainer import Trainer

__all__ = ["Trainer"]
