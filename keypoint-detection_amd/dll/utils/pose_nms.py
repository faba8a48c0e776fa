"""OKS pose-NMS on the device: the step of a top-down pose pipeline between
pose scoring and evaluation or drawing.  Two person boxes on one person give
two poses; the one whose object keypoint similarity (OKS) with a
higher-scoring pose of the same image is too high is suppressed (``hard``) or
has its score decayed (``soft``: Gaussian, ``soft_linear``: linear).

``kpd_pose_nms`` (csrc/pose_nms.hip) does the whole batch in one launch behind
the forward; nothing returns to the host.  The rules are written out in
DESIGN.md §3d and include/kpd.h; ``tests/pose_nms_ref.py`` restates them in
numpy.  The defaults (OKS threshold 0.9, visibility cut 0.2) are the values the
common top-down evaluation protocol uses; nothing here has been measured with
trained weights, and parity with any external implementation is not pinned
(DESIGN.md §5g).

There is no CPU fallback: a CPU tensor raises ``KpdNativeError``.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import _native
from .draw import keypoints_tensor, person_boxes
from .oks import COCO_SIGMAS, _f32, keypoint_peaks, pose_scores

POSE_NMS_MODES = {"hard": _native.POSE_NMS_HARD, "soft": _native.POSE_NMS_SOFT,
                  "soft_linear": _native.POSE_NMS_SOFT_LINEAR}


def oks_nms(kpts: torch.Tensor, scores: torch.Tensor, area: torch.Tensor, scale: torch.Tensor,
            kconf: Optional[torch.Tensor] = None, *, sigmas: Sequence[float] = COCO_SIGMAS, threshold: float = 0.9,
            mode: str = "hard", vis_threshold: float = 0.2, max_keep: int = 20, min_score: float = 0.0,
            return_oks: bool = False) -> Dict[str, torch.Tensor]:
    """``kpd_pose_nms`` on device tensors: kpts [B,D,K,2], scores [B,D] (a
    score not > 0 marks an absent slot), area [B,D] in scaled units squared,
    scale [B,2], kconf [B,D,K] or None.  Returns the output tensors of
    include/kpd.h by name (``keep``, ``n_keep``, ``scores_out``,
    ``suppressed_by`` and, with ``return_oks``, ``oks``), all on the device;
    the call does not synchronise."""
    if not isinstance(kpts, torch.Tensor):
        raise TypeError("kpts must be a tensor")
    _native._require_cuda(kpts, "kpts")
    dev = kpts.device
    if kpts.dim() != 4 or kpts.shape[-1] != 2:
        raise ValueError(f"kpts must be [B, D, K, 2], got {list(kpts.shape)}")
    if mode not in POSE_NMS_MODES:
        raise ValueError(f"unknown mode {mode!r}; choose from {sorted(POSE_NMS_MODES)}")
    B, D, K, _ = kpts.shape
    pk = _f32(kpts, dev, "kpts", (B, D, K, 2))
    ps = _f32(scores, dev, "scores", (B, D))
    pa = _f32(area, dev, "area", (B, D))
    sc = _f32(scale, dev, "scale", (B, 2))
    kc = None if kconf is None else _f32(kconf, dev, "kconf", (B, D, K))
    sig = [float(v) for v in sigmas]
    if len(sig) != K:
        raise ValueError(f"{len(sig)} sigmas for {K} keypoints")
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"keep": torch.empty(B, D, **i32), "n_keep": torch.empty(B, **i32),
           "scores_out": torch.empty(B, D, device=dev), "suppressed_by": torch.empty(B, D, **i32)}
    if return_oks:
        out["oks"] = torch.empty(B, D, D, dtype=torch.float64, device=dev)
    p = _native._ptr
    with torch.cuda.device(dev):
        rc = _native.load().kpd_pose_nms(p(pk), p(ps), p(pa), p(kc), p(sc), (ctypes.c_float * max(K, 1))(*sig),
                                         B, D, K, POSE_NMS_MODES[mode], float(threshold), float(vis_threshold),
                                         float(min_score), int(max_keep), p(out.get("oks")), p(out["keep"]),
                                         p(out["n_keep"]), p(out["scores_out"]), p(out["suppressed_by"]),
                                         _native._stream(dev))
    _native.check(rc, "kpd_pose_nms")
    return out


def _scale_tensor(sizes, B: int, dev) -> torch.Tensor:
    """(W, H) per image as [B, 2] fp32 on the device; one pair serves every image."""
    if isinstance(sizes, torch.Tensor):
        s = sizes.to(torch.float32)
    else:
        s = torch.from_numpy(np.asarray(sizes, dtype=np.float32))
    if s.numel() % 2:
        raise ValueError(f"sizes must be (W, H) pairs, got shape {list(s.shape)}")
    s = s.reshape(-1, 2)
    if s.shape[0] == 1 and B != 1:
        s = s.expand(B, 2)
    if s.shape[0] != B:
        raise ValueError(f"sizes describe {s.shape[0]} images, the outputs {B}")
    s = s.contiguous()
    return s.to(dev) if s.is_cuda else s.pin_memory().to(dev, non_blocking=True)


def suppress_poses(outputs: Dict, sizes, *, area_factor: float = 1.0, rescore: bool = True, **nms) -> Dict:
    """OKS pose-NMS of a forward's ``outputs``; ``sizes`` is (W, H) of the
    images, one pair or one per image; ``nms`` are ``oks_nms``'s options.

    Input scores are ``pose_scores(outputs, rescore)``, the per-keypoint
    confidences the heatmap-plane maxima (``keypoint_peaks``; outputs without a
    heatmap: every keypoint counts), areas ``w h W H area_factor`` of the
    person boxes in output-slot order (``draw.person_boxes``) and scale =
    (W, H).  Outputs without boxes raise ``ValueError``.

    Returns a shallow copy of ``outputs``; no input tensor is modified.  In the
    copy ``boxes`` is the [B, P, 4] tensor in slot order and ``box_scores`` the
    base score (``pose_scores(outputs, rescore=False)``) where the pose is kept
    and 0 where it is not, so ``draw_poses``, ``format_pose_labels`` and
    ``person_boxes`` drop suppressed persons through their ``box_scores`` rule;
    ``pose_scores`` [B, P] (``scores_out``: the ``scores`` of
    ``OksEvaluator.update``), ``pose_keep`` [B, P] and ``pose_n_keep`` [B] are
    new keys, with ``return_oks`` also ``pose_oks`` [B, P, P]."""
    k = torch.as_tensor(outputs["keypoints"])
    _native._require_cuda(k, "outputs['keypoints']")
    dev, B = k.device, k.shape[0]
    pk = keypoints_tensor(outputs, B)
    P = pk.shape[1]
    boxes = person_boxes(outputs, B, P, dev)
    if boxes is None:
        raise ValueError("suppress_poses needs outputs['boxes']: the pose areas come from the person boxes")
    scale = _scale_tensor(sizes, B, dev)
    area = boxes[..., 2] * boxes[..., 3] * scale[:, 0:1] * scale[:, 1:2] * float(area_factor)
    kconf = keypoint_peaks(outputs) if outputs.get("heatmap") is not None else None
    res = oks_nms(pk, pose_scores(outputs, rescore), area, scale, kconf, **nms)
    base = pose_scores(outputs, rescore=False)
    out = dict(outputs)
    out["boxes"] = boxes
    out["box_scores"] = torch.where(res["scores_out"] > 0, base, torch.zeros_like(base))
    out["pose_scores"], out["pose_keep"], out["pose_n_keep"] = res["scores_out"], res["keep"], res["n_keep"]
    if "oks" in res:
        out["pose_oks"] = res["oks"]
    return out
