"""MI355X-native drop-in for the reference's ``dll`` inference path.

The hot path (``dll.models`` + configs) with what stands around it on the
device: ``dll.data`` (``ITransform``, the YOLO-pose dataset and its targets, and
the training augmentation ``KeypointAugmentation`` / ``augment_batch``: flip,
rotate, scale with the labels moved along by ``kpd_augment_batch``),
``dll.losses``, ``dll.ops`` and ``dll.utils`` (metrics and ``draw_poses``, the
pose overlay the prediction CLI saves: boxes, skeleton, joints and a heatmap
underlay drawn in place by ``kpd_draw_poses``) and ``dll.training`` (the
``Trainer`` of the heatmap head on frozen trunk features).
Training anything but the heatmap head, feature-map plotting and the
reference's matplotlib panels are out of scope.
"""
from .configs import ModelConfig, TrainingConfig
from .models import MultiPersonKeypointModel

__version__ = "1.0.0+mi355x"

__all__ = ["MultiPersonKeypointModel", "ModelConfig", "TrainingConfig"]
