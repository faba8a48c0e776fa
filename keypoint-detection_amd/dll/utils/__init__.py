"""Evaluation helpers (reference ``dll.utils.metric`` / Trainer metrics), the
device-drawn pose overlay (``draw_poses``, csrc/draw.hip) and COCO keypoint AP
on the device (``OksEvaluator``, csrc/oks.hip)."""
from .draw import COCO_SKELETON, DrawStyle, draw_poses, format_pose_labels
from .metric import calculate_validation_metrics, get_default_metrics
from .oks import COCO_OKS_THRESHOLDS, COCO_SIGMAS, OksEvaluator, oks_match, pose_scores

__all__ = ["calculate_validation_metrics", "get_default_metrics", "COCO_SKELETON", "DrawStyle", "draw_poses",
           "format_pose_labels", "COCO_SIGMAS", "COCO_OKS_THRESHOLDS", "OksEvaluator", "oks_match", "pose_scores"]
