"""Training loss of the person detector.

The reference has no detection loss, no anchor matching and no box encoding,
so the rules are build-defined, like the eval detector's glue (§C3), and pinned
to the float64 restatement tests/det_train_ref.py; parity with any external
detector trainer is unpinned.  The work runs native in one fused pass over the
pooled trunk features (``dll.ops.detector_loss``: kpd_detector_targets +
kpd_detector_loss); this module only holds the hyper-parameters.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops


class DetectionLoss(nn.Module):
    """Focal classification + smooth-L1 box regression over the 28,224 anchors
    of ``PERSON_HEAD``, normalised by the number of positive anchors.

    Matching: an anchor whose best IoU over the labelled boxes is at least
    ``pos_thr`` is positive for that box, in [``neg_thr``, ``pos_thr``) ignored,
    below negative; every labelled box also claims the anchors within
    min(``tie_eps``, half its own best IoU) of that best IoU, so a sub-pixel
    box keeps to the anchors that tie for it.  Class term: focal loss (``alpha``,
    ``gamma``) of the sigmoid logits; box term: smooth-L1 (``beta``) of the raw
    deltas against the decode's inverse, weighted by ``box_weight``."""

    def __init__(self, pos_thr: float = 0.5, neg_thr: float = 0.4, tie_eps: float = 1e-5, alpha: float = 0.25,
                 gamma: float = 2.0, beta: float = 1.0 / 9, box_weight: float = 1.0):
        super().__init__()
        if not 0.0 < pos_thr <= 1.0 or not 0.0 <= neg_thr <= pos_thr:
            raise ValueError(f"need 0 <= neg_thr <= pos_thr <= 1 and pos_thr > 0, got {neg_thr}, {pos_thr}")
        if tie_eps < 0 or not 0.0 <= alpha <= 1.0 or gamma < 0 or beta <= 0 or box_weight < 0:
            raise ValueError("need tie_eps >= 0, alpha in [0, 1], gamma >= 0, beta > 0 and box_weight >= 0")
        self.pos_thr, self.neg_thr, self.tie_eps = float(pos_thr), float(neg_thr), float(tie_eps)
        self.alpha, self.gamma, self.beta, self.box_weight = float(alpha), float(gamma), float(beta), float(box_weight)

    def forward(self, person_head: nn.Module, pooled: torch.Tensor, gt_boxes: Optional[torch.Tensor],
                image_size) -> torch.Tensor:
        """pooled [B, 3136, 128] (``Plan.detector_features``), gt_boxes
        [B, G, 4] cxcywh normalised (all-zero rows are padding), image_size
        (H, W) -> the 0-d loss with gradients to ``person_head.box_heads[0]``
        and ``cls_heads[0]``; ``loss.cls_part`` / ``loss.box_part`` /
        ``loss.n_pos`` ride along detached."""
        box, cls = person_head.box_heads[0], person_head.cls_heads[0]
        return ops.detector_loss(pooled, box.weight, box.bias, cls.weight, cls.bias, person_head.anchors, gt_boxes,
                                 image_size, pos_thr=self.pos_thr, neg_thr=self.neg_thr, tie_eps=self.tie_eps,
                                 alpha=self.alpha, gamma=self.gamma, beta=self.beta,
                                 box_weight_factor=self.box_weight)

    def extra_repr(self) -> str:
        return (f"pos_thr={self.pos_thr}, neg_thr={self.neg_thr}, tie_eps={self.tie_eps}, alpha={self.alpha}, "
                f"gamma={self.gamma}, beta={self.beta:.6g}, box_weight={self.box_weight}")
