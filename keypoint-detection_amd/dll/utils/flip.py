"""Flip-test on the device: the standard step of top-down pose evaluation that
runs the network on the image and on its left-right mirror, mirrors the second
pass's heatmaps back, swaps the left / right joint planes, averages the two and
decodes the average.

``kpd_flip_merge`` (csrc/flip_merge.hip) does the merge and the decode of a
whole batch in one launch behind the two forwards; nothing returns to the host.
The rules are written out in DESIGN.md §3e and include/kpd.h;
``tests/flip_ref.py`` restates them in numpy.  The one-pixel misalignment of
mirrored strided features is not compensated, and the accuracy effect with
trained weights is unmeasured (no checkpoint exists).

There is no CPU fallback: a CPU tensor raises ``KpdNativeError``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from .. import _native

# COCO joints: nose, then (left, right) eye, ear, shoulder, elbow, wrist, hip, knee, ankle
COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
_TINY = float(torch.finfo(torch.float32).tiny)   # the smallest positive normal float


def flip_index(K: int = 17, pairs: Sequence = COCO_FLIP_PAIRS) -> List[int]:
    """The joint whose mirrored plane merges into joint k, for k < K: ``pairs``
    swapped, every other joint (the nose) paired with itself -- an involution."""
    idx = list(range(K))
    for a, b in pairs:
        if not (0 <= a < K and 0 <= b < K):
            raise ValueError(f"flip pair ({a}, {b}) does not fit {K} keypoints")
        idx[a], idx[b] = b, a
    if any(idx[idx[k]] != k for k in range(K)):
        raise ValueError("the flip pairs overlap: the joint map is not an involution")
    return idx


def mirror_boxes(boxes: torch.Tensor) -> torch.Tensor:
    """cxcywh boxes [..., 4] of the left-right mirrored image: cx' = 1 - cx, the
    rest unchanged.  All-zero rows (padding) stay all-zero; a non-zero row whose
    mirror would be all-zero (cx == 1, cy = w = h = 0) gets cx' = the smallest
    positive normal float, so both passes compact their boxes identically."""
    if boxes.shape[-1] != 4:
        raise ValueError(f"boxes must be [..., 4] cxcywh, got {list(boxes.shape)}")
    zero = (boxes == 0).all(-1)
    cx = 1.0 - boxes[..., 0]
    rest_zero = (boxes[..., 1:] == 0).all(-1)
    cx = torch.where((cx == 0) & rest_zero, torch.full_like(cx, _TINY), cx)
    cx = torch.where(zero, torch.zeros_like(cx), cx)
    return torch.cat([cx.unsqueeze(-1), boxes[..., 1:]], dim=-1)


def mirror_images(x: torch.Tensor) -> torch.Tensor:
    """The left-right mirror of [..., H, W] images."""
    return x.flip(-1)


def flip_merge(heat_a: torch.Tensor, heat_b: torch.Tensor, boxes: torch.Tensor,
               pairs: Optional[Sequence[int]] = None, inplace: bool = False) -> Dict[str, torch.Tensor]:
    """Merge and decode the heatmaps of a straight (``heat_a``) and a mirrored
    (``heat_b``) forward, both [n, P, K, H, W] in the forward's person-slot
    order; ``boxes`` [n, P, 4] are the straight pass's boxes in caller order
    (zero rows included); ``pairs`` the joint map (default ``flip_index(K)``).
    Returns ``heatmap`` [n,P,K,H,W] (``heat_a`` itself with ``inplace``),
    ``keypoints`` [n,P,1,K,2], ``visibilities`` [n,P,1,K,3] and
    ``keypoint_peaks`` [n,P,K] -- the forward's output shapes -- on the device;
    the call does not synchronise."""
    if not isinstance(heat_a, torch.Tensor) or not isinstance(heat_b, torch.Tensor):
        raise TypeError("heat_a and heat_b must be tensors")
    _native._require_cuda(heat_a, "heat_a")
    _native._require_cuda(heat_b, "heat_b")
    if heat_a.dim() != 5 or tuple(heat_a.shape) != tuple(heat_b.shape):
        raise ValueError(f"heat_a / heat_b must be equal [n, P, K, H, W], got {list(heat_a.shape)} and "
                         f"{list(heat_b.shape)}")
    dev = heat_a.device
    n, P, K, _, _ = heat_a.shape
    if inplace and not (heat_a.dtype == torch.float32 and heat_a.is_contiguous()):
        raise ValueError("inplace needs a contiguous float32 heat_a")
    a = _native._dev_f32(heat_a, "heat_a")
    b = _native._dev_f32(heat_b, "heat_b")
    bx = _native._dev_f32(torch.as_tensor(boxes), "boxes")
    if tuple(bx.shape) != (n, P, 4) or bx.device != dev:
        raise ValueError(f"boxes must be [{n}, {P}, 4] on {dev}, got {list(bx.shape)} on {bx.device}")
    out = {"heatmap": a if inplace else torch.empty_like(a),
           "keypoints": torch.empty(n, P, 1, K, 2, device=dev),
           "visibilities": torch.empty(n, P, 1, K, 3, device=dev),
           "keypoint_peaks": torch.empty(n, P, K, device=dev)}
    _native.flip_merge(a, b, bx, flip_index(K) if pairs is None else pairs, out["heatmap"], out["keypoints"],
                       out["visibilities"], out["keypoint_peaks"])
    return out
