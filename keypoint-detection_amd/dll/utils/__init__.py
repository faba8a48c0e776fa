"""Evaluation helpers (reference ``dll.utils.metric`` / Trainer metrics), the
device-drawn pose overlay (``draw_poses``, csrc/draw.hip), COCO keypoint AP
on the device (``OksEvaluator``, csrc/oks.hip), OKS pose-NMS on the device
(``oks_nms`` / ``suppress_poses``, csrc/pose_nms.hip) and the flip-test merge
on the device (``flip_merge``, csrc/flip_merge.hip), and OKS pose tracking across
frames on the device (``PoseTracker``, csrc/track.hip)."""
from .draw import COCO_SKELETON, DrawStyle, draw_poses, format_pose_labels
from .flip import COCO_FLIP_PAIRS, flip_index, flip_merge, mirror_boxes, mirror_images
from .metric import calculate_validation_metrics, get_default_metrics
from .oks import COCO_OKS_THRESHOLDS, COCO_SIGMAS, OksEvaluator, keypoint_peaks, oks_match, pose_scores
from .pose_nms import POSE_NMS_MODES, oks_nms, suppress_poses
from .track import PoseTracker

__all__ = ["calculate_validation_metrics", "get_default_metrics", "COCO_SKELETON", "DrawStyle", "draw_poses",
           "format_pose_labels", "COCO_SIGMAS", "COCO_OKS_THRESHOLDS", "OksEvaluator", "oks_match", "pose_scores",
           "keypoint_peaks", "POSE_NMS_MODES", "oks_nms", "suppress_poses", "COCO_FLIP_PAIRS", "flip_index",
           "flip_merge", "mirror_boxes", "mirror_images", "PoseTracker"]
