"""COCO keypoint AP on the device: object keypoint similarity (OKS), greedy
matching by score at the ten OKS thresholds, 101-point interpolated precision
and AP / AP50 / AP75 / AR.

Per batch, ``kpd_oks_match`` (csrc/oks.hip) computes the OKS of every
(predicted pose, labelled person) pair of every image and matches them under
COCOeval's rules in one launch behind the forward; nothing returns to the
host.  ``OksEvaluator.summarize`` then runs COCOeval's ``accumulate`` over the
kept device tensors with a handful of float64 torch ops and transfers the four
numbers.  The rules are written out in DESIGN.md §3c and include/kpd.h;
``tests/oks_ref.py`` restates them in numpy.  Parity with pycocotools itself
is not pinned.

Unlike the slot-wise ADE / PCK of ``dll.utils.metric``, this matches predicted
poses to labelled persons, so it scores detector boxes (any order, any count,
duplicates and misses) as well as ground-truth boxes.

There is no CPU fallback: a CPU tensor raises ``KpdNativeError``.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _native
from .draw import keypoints_tensor, person_boxes

# the published per-keypoint constants of the COCO keypoint evaluation (COCOeval.Params.kpt_oks_sigmas)
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
COCO_OKS_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_GRID = np.linspace(0, 1, 101)
_EPS = float(np.spacing(1))   # 2^-52

METRIC_KEYS = ("oks_AP", "oks_AP50", "oks_AP75", "oks_AR")


def _f32(t, dev, name: str, shape) -> torch.Tensor:
    t = torch.as_tensor(t).to(dev, torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return t


def oks_match(pred_kpts: torch.Tensor, pred_scores: torch.Tensor, gt_kpts: torch.Tensor, gt_vis: torch.Tensor,
              gt_boxes: torch.Tensor, gt_area: torch.Tensor, n_gt: torch.Tensor, scale: torch.Tensor,
              sigmas: Sequence[float] = COCO_SIGMAS, thresholds: Sequence[float] = COCO_OKS_THRESHOLDS,
              max_dets: int = 20, return_oks: bool = False) -> Dict[str, torch.Tensor]:
    """``kpd_oks_match`` on device tensors: pred_kpts [B,D,K,2], pred_scores
    [B,D] (a score not > 0 marks an absent slot), gt_kpts [B,G,K,2], gt_vis
    [B,G,K], gt_boxes [B,G,4] cxcywh, gt_area [B,G], n_gt [B], scale [B,2].
    Returns the output tensors of include/kpd.h by name (``det_score``,
    ``det_slot``, ``det_match``, ``det_ignore``, ``gt_match``, ``counts`` and,
    with ``return_oks``, ``oks``), all on the device; the call does not
    synchronise."""
    if not isinstance(pred_kpts, torch.Tensor):
        raise TypeError("pred_kpts must be a tensor")
    _native._require_cuda(pred_kpts, "pred_kpts")
    dev = pred_kpts.device
    if pred_kpts.dim() != 4 or pred_kpts.shape[-1] != 2:
        raise ValueError(f"pred_kpts must be [B, D, K, 2], got {list(pred_kpts.shape)}")
    B, D, K, _ = pred_kpts.shape
    if gt_kpts.dim() != 4:
        raise ValueError(f"gt_kpts must be [B, G, K, 2], got {list(gt_kpts.shape)}")
    G = gt_kpts.shape[1]
    pk = _f32(pred_kpts, dev, "pred_kpts", (B, D, K, 2))
    ps = _f32(pred_scores, dev, "pred_scores", (B, D))
    gk = _f32(gt_kpts, dev, "gt_kpts", (B, G, K, 2))
    gv = _f32(gt_vis, dev, "gt_vis", (B, G, K))
    gb = _f32(gt_boxes, dev, "gt_boxes", (B, G, 4))
    ga = _f32(gt_area, dev, "gt_area", (B, G))
    sc = _f32(scale, dev, "scale", (B, 2))
    ng = torch.as_tensor(n_gt).to(dev, torch.int32).contiguous()
    if tuple(ng.shape) != (B,):
        raise ValueError(f"n_gt must be [{B}], got {list(ng.shape)}")
    sig = [float(v) for v in sigmas]
    thr = [float(v) for v in thresholds]
    if len(sig) != K:
        raise ValueError(f"{len(sig)} sigmas for {K} keypoints")
    T = len(thr)
    M = max(min(int(max_dets), D), 0)
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"det_score": torch.empty(B, M, device=dev), "det_slot": torch.empty(B, M, **i32),
           "det_match": torch.empty(B, T, M, **i32), "det_ignore": torch.empty(B, T, M, dtype=torch.uint8, device=dev),
           "gt_match": torch.empty(B, T, G, **i32), "counts": torch.empty(B, 2, **i32)}
    if return_oks:
        out["oks"] = torch.empty(B, D, G, dtype=torch.float64, device=dev)
    p = _native._ptr
    with torch.cuda.device(dev):
        rc = _native.load().kpd_oks_match(p(pk), p(ps), p(gk), p(gv), p(gb), p(ga), p(ng), p(sc),
                                          (ctypes.c_float * max(K, 1))(*sig), (ctypes.c_float * max(T, 1))(*thr),
                                          B, D, G, K, T, int(max_dets), p(out.get("oks")), p(out["det_score"]),
                                          p(out["det_slot"]), p(out["det_match"]), p(out["det_ignore"]),
                                          p(out["gt_match"]), p(out["counts"]), _native._stream(dev))
    _native.check(rc, "kpd_oks_match")
    return out


def keypoint_peaks(outputs: Dict) -> torch.Tensor:
    """The maximum of every heatmap plane of a forward's ``outputs``, [B, P, K]:
    one confidence per keypoint (``outputs['heatmap']`` is a sigmoid).  Outputs
    that carry ``keypoint_peaks`` (a flip-test forward: ``kpd_flip_merge``
    writes them with the merged map) return that tensor -- the same values
    with one pass over the heatmap fewer."""
    k = torch.as_tensor(outputs["keypoints"])
    B, dev = k.shape[0], k.device
    if outputs.get("keypoint_peaks") is not None:
        return torch.as_tensor(outputs["keypoint_peaks"]).to(dev, torch.float32)
    P = keypoints_tensor(outputs, B).shape[1]
    heat = outputs.get("heatmap")
    if heat is None:
        raise ValueError("the keypoint peaks need outputs['heatmap']")
    heat = torch.as_tensor(heat).to(dev, torch.float32)
    return heat.reshape(B, P, -1, heat.shape[-2] * heat.shape[-1]).amax(-1)


def pose_scores(outputs: Dict, rescore: bool = True) -> torch.Tensor:
    """One score per person slot of a forward's ``outputs``, [B, P].  The base
    is the detector's ``box_scores`` when the outputs carry them; otherwise 1
    for a slot whose box is not all zero and 0 for an absent slot, the
    renderer's rule (``draw.person_boxes``; outputs without boxes: every slot
    1).  With ``rescore`` the base is multiplied by the mean over keypoints of
    the heatmap plane's maximum; ``outputs['heatmap']`` is a sigmoid, so a
    present person keeps a score > 0."""
    k = torch.as_tensor(outputs["keypoints"])
    B, dev = k.shape[0], k.device
    P = keypoints_tensor(outputs, B).shape[1]
    if outputs.get("box_scores") is not None:
        base = torch.as_tensor(outputs["box_scores"]).to(dev, torch.float32).reshape(B, P)
    else:
        boxes = person_boxes(outputs, B, P, dev)
        base = torch.ones(B, P, device=dev) if boxes is None else (boxes != 0).any(-1).to(torch.float32)
    if not rescore:
        return base
    if outputs.get("heatmap") is None:
        raise ValueError("rescore=True needs outputs['heatmap']")
    return base * keypoint_peaks(outputs).mean(-1)


class OksEvaluator:
    """COCO keypoint AP / AP50 / AP75 / AR over a dataset, accumulated on the
    device.  ``update`` launches ``kpd_oks_match`` for one batch and keeps its
    output tensors; ``summarize`` is COCOeval's ``accumulate`` + ``summarize``
    (area range "all", one category) in float64 torch ops with one host
    transfer, of the four numbers.

    ``area_factor`` scales the ground-truth area ``w h W H`` (the labelled box
    in pixels): COCO's ``area`` is the segment's, commonly taken as 0.53 of the
    box when only boxes are labelled; the default 1.0 uses the box."""

    def __init__(self, sigmas: Sequence[float] = COCO_SIGMAS, thresholds: Sequence[float] = COCO_OKS_THRESHOLDS,
                 max_dets: int = 20, area_factor: float = 1.0):
        self.sigmas = np.asarray(sigmas, np.float64)
        self.thresholds = np.asarray(thresholds, np.float64)
        if self.thresholds.ndim != 1 or not 1 <= len(self.thresholds) <= _native.OKS_MAX_T:
            raise ValueError(f"between 1 and {_native.OKS_MAX_T} thresholds")
        if int(max_dets) < 1:
            raise ValueError("max_dets must be at least 1")
        self.max_dets, self.area_factor = int(max_dets), float(area_factor)
        self.results: List[Dict[str, torch.Tensor]] = []

    def reset(self) -> None:
        self.results = []

    def inputs(self, outputs: Dict, batch: Dict, scores: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The device tensors ``update`` hands to ``oks_match`` for a forward's
        ``outputs`` and a collated ``batch`` ('keypoints' [B,G,K,2],
        'visibilities' [B,G,K], 'bboxes' ([boxes] or a tensor, [B,G,4] cxcywh
        normalised), 'num_persons' [B], 'orig_size': (W, H) per image):
        scale = (W, H) per image, gt_area = w h W H area_factor; the
        [B,P,1,K,2] prediction layout is squeezed; ``scores`` defaults to
        ``pose_scores(outputs)``."""
        k = torch.as_tensor(outputs["keypoints"])
        _native._require_cuda(k, "outputs['keypoints']")
        dev, B = k.device, k.shape[0]
        pk = keypoints_tensor(outputs, B)
        P = pk.shape[1]
        ps = pose_scores(outputs) if scores is None else torch.as_tensor(scores).to(dev, torch.float32).reshape(B, P)
        bb = batch["bboxes"]
        bb = (bb[0] if isinstance(bb, (list, tuple)) else bb).to(dev, torch.float32)
        gk = batch["keypoints"].to(dev, torch.float32)
        if gk.shape[0] != B or bb.shape[:2] != gk.shape[:2]:
            raise ValueError(f"batch keypoints {list(gk.shape)} / bboxes {list(bb.shape)} do not describe the "
                             f"{B} images of the outputs")
        sizes = torch.tensor([[float(w), float(h)] for w, h in batch["orig_size"]], dtype=torch.float32).reshape(-1, 2)
        if sizes.shape[0] != B:
            raise ValueError(f"orig_size describes {sizes.shape[0]} images, the outputs {B}")
        scale = sizes.pin_memory().to(dev, non_blocking=True)
        area = bb[..., 2] * bb[..., 3] * scale[:, 0:1] * scale[:, 1:2] * self.area_factor
        return {"pred_kpts": pk, "pred_scores": ps, "gt_kpts": gk, "gt_vis": batch["visibilities"].to(dev),
                "gt_boxes": bb, "gt_area": area, "n_gt": batch["num_persons"].to(dev), "scale": scale}

    def update(self, outputs: Dict, batch: Dict, scores: Optional[torch.Tensor] = None) -> None:
        """Match one batch on the device and keep the result.  No ``.item()``,
        ``.cpu()`` or synchronisation: the launch queues behind the forward."""
        self.results.append(oks_match(**self.inputs(outputs, batch, scores), sigmas=self.sigmas,
                                      thresholds=self.thresholds, max_dets=self.max_dets))

    def summarize(self) -> Dict[str, float]:
        """COCOeval ``accumulate``: the ranked detections of all images in
        update order, a stable descending sort on the scores (its mergesort of
        the negated scores), cumulative true / false positives per threshold,
        recall = tp / counted gts, precision = tp / (tp + fp + 2^-52) made
        non-increasing from the right, sampled at the 101 recall points by
        ``searchsorted`` (left; 0 past the end).  AP = the mean over thresholds
        and recall points, AP50 / AP75 the rows of the thresholds nearest 0.5
        and 0.75, AR the mean over thresholds of the last recall.  Every value
        is -1 without a counted ground truth; AP and AR are 0 with counted
        ground truths and no detection.

        Ranks past an image's ``n_det`` are not dropped (their number lives on
        the device) but kept as ignored entries with score -inf: the sort puts
        them last, where they count as neither true nor false positive and
        change no value."""
        if not self.results:
            return {k: -1.0 for k in METRIC_KEYS}
        dev = self.results[0]["counts"].device
        T = len(self.thresholds)
        f64 = dict(dtype=torch.float64, device=dev)
        score, match, ignore = [], [], []
        for r in self.results:
            ranked = r["det_slot"] >= 0                                              # [B, M]
            score.append(torch.where(ranked, r["det_score"], r["det_score"].new_tensor(-np.inf)).reshape(-1))
            match.append((r["det_match"] >= 0).permute(1, 0, 2).reshape(T, -1))
            ignore.append(((r["det_ignore"] != 0) | ~ranked[:, None, :]).permute(1, 0, 2).reshape(T, -1))
        # one more ignored entry, so the arrays are never empty
        score.append(torch.full((1,), -np.inf, device=dev))
        match.append(torch.zeros(T, 1, dtype=torch.bool, device=dev))
        ignore.append(torch.ones(T, 1, dtype=torch.bool, device=dev))
        npig = torch.cat([r["counts"][:, 1] for r in self.results]).sum().to(torch.float64)
        order = torch.sort(torch.cat(score), stable=True, descending=True).indices
        m, ig = torch.cat(match, 1)[:, order], torch.cat(ignore, 1)[:, order]
        tp = (m & ~ig).to(torch.float64).cumsum(1)
        fp = (~m & ~ig).to(torch.float64).cumsum(1)
        rc = tp / npig
        pr = tp / (tp + fp + _EPS)
        pr = pr.flip(1).cummax(1).values.flip(1)
        n = rc.shape[1]
        grid = torch.as_tensor(RECALL_GRID, **f64).expand(T, -1).contiguous()
        idx = torch.searchsorted(rc.contiguous(), grid, right=False)
        q = torch.where(idx < n, pr.gather(1, idx.clamp(max=n - 1)), torch.zeros((), **f64))   # [T, 101]
        i50 = int(np.abs(self.thresholds - 0.5).argmin())
        i75 = int(np.abs(self.thresholds - 0.75).argmin())
        vals = torch.stack([q.mean(), q[i50].mean(), q[i75].mean(), rc[:, -1].mean()])
        vals = torch.where(npig > 0, vals, torch.full_like(vals, -1.0))
        return dict(zip(METRIC_KEYS, vals.tolist()))   # the one host transfer
