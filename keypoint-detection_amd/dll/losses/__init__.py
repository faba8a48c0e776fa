from .detection_loss import DetectionLoss
from .keypoint_loss import (AdaptiveHeatmapLoss, DynamicLossBalancer, ImprovedKeypointLoss, KeypointLoss, LossMetrics,
                            SoftArgmaxCoordinateLoss, SpatialCoordinateLoss)

__all__ = ["AdaptiveHeatmapLoss", "DetectionLoss", "DynamicLossBalancer", "ImprovedKeypointLoss", "KeypointLoss",
           "LossMetrics", "SoftArgmaxCoordinateLoss", "SpatialCoordinateLoss"]
