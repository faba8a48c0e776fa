"""Evaluation helpers (reference ``dll.utils.metric`` / Trainer metrics) and
the device-drawn pose overlay (``draw_poses``, csrc/draw.hip)."""
from .draw import COCO_SKELETON, DrawStyle, draw_poses, format_pose_labels
from .metric import calculate_validation_metrics, get_default_metrics

__all__ = ["calculate_validation_metrics", "get_default_metrics", "COCO_SKELETON", "DrawStyle", "draw_poses",
           "format_pose_labels"]
