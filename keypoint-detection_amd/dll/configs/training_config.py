"""Training configuration.  Only ``pck_thresholds`` is read on the inference
hot path and ``augmentation`` by the device augmentation
(``dll.data.KeypointAugmentation``); the remaining fields are kept so the
reference's constructor call ``TrainingConfig()`` and YAML dicts keep working
(reference: dll/configs/training_config.py:94-133).  ``dll.training.Trainer``
reads ``optimizer``, ``lr_scheduler``, ``num_epochs``, ``batch_size`` (through
``scripts/train.py``), ``checkpoint_interval`` and ``pck_thresholds``."""
from dataclasses import dataclass, field
from typing import Any, Dict, List, Union

from .base_config import BaseConfig, DeviceConfig


@dataclass
class OptimizerConfig(BaseConfig):
    name: str = "adam"
    learning_rate: float = 0.001
    weight_decay: float = 1e-4
    momentum: float = 0.9
    beta1: float = 0.9
    beta2: float = 0.999


@dataclass
class AugmentationConfig(BaseConfig):
    """The reference's fields (its YAML block constructs this class), plus
    ``color`` and ``fill``.  Each enabled transform is applied on its own with
    probability ``prob`` (``KeypointAugmentation.sample``)."""
    enabled: bool = False
    prob: float = 0.5
    flip: Dict[str, bool] = field(default_factory=lambda: {"enabled": True, "horizontal": True})
    rotate: Dict[str, Union[bool, float]] = field(default_factory=lambda: {"enabled": True, "max_angle": 30.0})
    scale: Dict[str, Any] = field(default_factory=lambda: {"enabled": True, "range": [0.8, 1.2]})
    color: Dict[str, Union[bool, float]] = field(
        default_factory=lambda: {"enabled": False, "brightness": 0.2, "contrast": 0.2})
    fill: Any = 0   # colour of a tap outside the source image: one value or three

    def validate(self) -> None:
        assert 0 <= self.prob <= 1, "prob must be between 0 and 1"
        assert float(self.rotate.get("max_angle", 0.0)) >= 0, "rotate.max_angle must not be negative"
        lo, hi = self.scale.get("range", [1.0, 1.0])
        assert 0 < lo <= hi, "scale.range must satisfy 0 < range[0] <= range[1]"


@dataclass
class LossConfig(BaseConfig):
    keypoint_loss_weight: float = 15.0
    visibility_loss_weight: float = 5.0


@dataclass
class LRSchedulerConfig(BaseConfig):
    factor: float = 0.1
    patience: int = 3
    min_lr: float = 1e-6
    mode: str = "min"
    threshold: float = 1e-4
    metric: str = "loss"


@dataclass
class TrainingConfig(BaseConfig):
    num_epochs: int = 50
    batch_size: int = 32
    num_workers: int = 4
    optimizer: OptimizerConfig = field(default_factory=OptimizerConfig)
    augmentation: AugmentationConfig = field(default_factory=AugmentationConfig)
    loss: LossConfig = field(default_factory=LossConfig)
    lr_scheduler: LRSchedulerConfig = field(default_factory=LRSchedulerConfig)
    device: DeviceConfig = field(default_factory=DeviceConfig)
    checkpoint_interval: int = 5
    validation_interval: int = 1
    lr_factor: float = 0.1
    patience: int = 3
    min_lr: float = 1e-6
    lambda_keypoint: float = 15.0
    lambda_visibility: float = 5.0
    l2_lambda: float = 0.0003
    default_validation_threshold: float = 0.5
    pck_thresholds: List[float] = field(default_factory=lambda: [0.002, 0.05, 0.2])
