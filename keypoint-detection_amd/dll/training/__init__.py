"""Training on frozen trunk features: the heatmap head and the person detector (§3j)."""
from .detector_trainer import DetectorTrainer
from .trainer import Trainer

__all__ = ["DetectorTrainer", "Trainer"]
