"""OKS pose tracking across frames on the device: identity and temporal
stability for a frame sequence that runs through a top-down pose pipeline.
Person slot ``p`` of frame ``t`` has no relation to slot ``p`` of frame
``t + 1`` (detector and NMS order change), and per-frame soft-argmax output
jitters.  ``PoseTracker`` associates every frame's poses with the live tracks
of its sequence by greedy OKS matching and, on request, runs a One-Euro filter
per joint along each track.

``kpd_track_poses`` (csrc/track.hip) does the frames of a call in one launch
behind the forward, one workgroup per sequence; the state between calls lives
in a device tensor the tracker owns, and nothing returns to the host.  The
rules are written out in DESIGN.md §3m and include/kpd.h;
``tests/track_ref.py`` restates them in numpy.

The defaults (OKS threshold 0.3, ``max_age`` 10, the One-Euro constants
``min_cutoff`` 1.0, ``beta`` 0.05, ``d_cutoff`` 1.0 at 30 fps) are unmeasured:
no trained checkpoint and no sequence data exist here, so neither their effect
on identity switches nor on jitter has been evaluated, and parity with any
external tracker is not pinned.

There is no CPU fallback: a CPU tensor raises ``KpdNativeError``.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import torch

from .. import _native
from .draw import keypoints_tensor, person_boxes
from .oks import COCO_SIGMAS, _f32, keypoint_peaks, pose_scores
from .pose_nms import _scale_tensor


class PoseTracker:
    """Tracks of ``num_sequences`` independent frame sequences with
    ``num_keypoints`` joints per pose, at most ``_native.TRACK_MAX_T`` live
    tracks per sequence.  ``threshold``: the OKS a pose needs with a track to
    continue it; ``vis_threshold``: keypoints whose confidence is not above it
    count neither in the OKS nor in the filter; ``max_age``: frames a track
    survives without a match; ``smooth``: run the One-Euro filter
    (``min_cutoff``, ``beta``, ``d_cutoff`` in its usual meaning, ``fps`` the
    frame rate).  All defaults are unmeasured (module docstring)."""

    def __init__(self, num_keypoints: int = 17, num_sequences: int = 1, *, device, sigmas: Sequence[float] = COCO_SIGMAS,
                 threshold: float = 0.3, vis_threshold: float = 0.2, max_age: int = 10, smooth: bool = True,
                 min_cutoff: float = 1.0, beta: float = 0.05, d_cutoff: float = 1.0, fps: float = 30.0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _native.KpdNativeError(f"PoseTracker needs a HIP device (got {self.device}); the native path has "
                                         f"no CPU fallback")
        self.K, self.S = int(num_keypoints), int(num_sequences)
        self.sigmas = [float(v) for v in sigmas]
        if len(self.sigmas) != self.K:
            raise ValueError(f"{len(self.sigmas)} sigmas for {self.K} keypoints")
        if self.S < 1:
            raise ValueError("num_sequences must be at least 1")
        nbytes = int(_native.load().kpd_track_state_bytes(self.K))
        if nbytes == 0:
            raise ValueError(f"num_keypoints must be in [1, {_native.TRACK_MAX_K}], got {self.K}")
        self.threshold, self.vis_threshold, self.max_age = float(threshold), float(vis_threshold), int(max_age)
        self.smooth = bool(smooth)
        self.min_cutoff, self.beta, self.d_cutoff, self.fps = float(min_cutoff), float(beta), float(d_cutoff), float(fps)
        self._words, self._state = nbytes // 8, None

    @property
    def state(self) -> torch.Tensor:
        """The tracker's own state tensor, [num_sequences, state bytes / 8]
        int64 (the state holds doubles: 8-byte elements keep it aligned
        whatever the allocator does), zero-initialised at first use."""
        if self._state is None:
            self._state = torch.zeros(self.S, self._words, dtype=torch.int64, device=self.device)
        return self._state

    def reset(self) -> None:
        """Forget every track: the all-zero state (no tracks, next id 0)."""
        self.state.zero_()

    def update(self, kpts: torch.Tensor, scores: torch.Tensor, area: torch.Tensor, scale: torch.Tensor,
               kconf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """``kpd_track_poses`` on device tensors: kpts [S,B,D,K,2] ([B,D,K,2]
        with one sequence), scores [S,B,D] (a score not > 0 marks an absent
        slot), area [S,B,D] in scaled units squared, scale [S,B,2], kconf
        [S,B,D,K] or None: B consecutive frames of every sequence, continuing
        where the last call ended.  Returns ``track_id`` and ``track_hits``
        [S,B,D] int32, ``track_oks`` [S,B,D] float64, ``counts`` [S,B,4] int32
        (matched, born, dropped, live) and ``keypoints`` [S,B,D,K,2] (the
        smoothed poses; the input tensor itself without smoothing), in the
        input's leading shape, all on the device; the call does not
        synchronise."""
        if not isinstance(kpts, torch.Tensor):
            raise TypeError("kpts must be a tensor")
        _native._require_cuda(kpts, "kpts")
        single = kpts.dim() == 4
        if kpts.dim() not in (4, 5) or kpts.shape[-1] != 2:
            raise ValueError(f"kpts must be [S, B, D, K, 2] or [B, D, K, 2], got {list(kpts.shape)}")
        dev = kpts.device
        if dev != self.state.device:
            raise ValueError(f"kpts is on {dev}, the tracker's state on {self.state.device}")
        lead = tuple(kpts.shape[:-3])
        S = 1 if single else kpts.shape[0]
        B, D, K = kpts.shape[-4], kpts.shape[-3], kpts.shape[-2]
        if S != self.S or K != self.K:
            raise ValueError(f"the tracker holds {self.S} sequence(s) of {self.K} keypoints, got {S} of {K}")
        pk = _f32(kpts, dev, "kpts", lead + (D, K, 2))
        ps = _f32(scores, dev, "scores", lead + (D,))
        pa = _f32(area, dev, "area", lead + (D,))
        sc = _f32(scale, dev, "scale", lead + (2,))
        kc = None if kconf is None else _f32(kconf, dev, "kconf", lead + (D, K))
        i32 = dict(dtype=torch.int32, device=dev)
        out = {"track_id": torch.empty(lead + (D,), **i32), "track_hits": torch.empty(lead + (D,), **i32),
               "track_oks": torch.empty(lead + (D,), dtype=torch.float64, device=dev),
               "counts": torch.empty(lead + (4,), **i32),
               "keypoints": torch.empty_like(pk) if self.smooth else pk}
        p = _native._ptr
        with torch.cuda.device(dev):
            rc = _native.load().kpd_track_poses(
                p(pk), p(ps), p(pa), p(kc), p(sc), (ctypes.c_float * max(K, 1))(*self.sigmas), S, B, D, K,
                self.threshold, self.vis_threshold, self.max_age, int(self.smooth), self.min_cutoff, self.beta,
                self.d_cutoff, self.fps, p(self.state), p(out["track_id"]), p(out["track_hits"]), p(out["track_oks"]),
                p(out["keypoints"]) if self.smooth else None, p(out["counts"]), _native._stream(dev))
        _native.check(rc, "kpd_track_poses")
        return out

    def track(self, outputs: Dict, sizes, *, area_factor: float = 1.0, rescore: bool = True) -> Dict:
        """Track a forward's ``outputs`` as B consecutive frames of the single
        sequence; ``sizes`` is (W, H) of the frames, one pair or one per frame.

        The inputs are built as ``suppress_poses`` builds them: scores
        ``pose_scores(outputs, rescore)`` (so a pose that pose-NMS suppressed
        is absent), per-keypoint confidences the heatmap-plane maxima
        (``keypoint_peaks``; outputs without a heatmap and without
        ``keypoint_peaks``: every keypoint counts), areas ``w h W H
        area_factor`` of the person boxes in output-slot order and scale =
        (W, H).  Outputs without boxes raise ``ValueError``.

        Returns a shallow copy of ``outputs``; no input tensor is modified.
        In the copy ``track_ids`` and ``track_hits`` [B, P] int32 (-1 / 0 for
        an absent slot or a pose without a table entry), ``track_oks`` [B, P],
        ``track_counts`` [B, 4] and ``track_scores`` [B, P] (the scores the
        tracker saw) are new keys; with smoothing ``keypoints`` holds the
        smoothed values in the input's own shape and ``keypoints_raw`` the
        forward's."""
        if self.S != 1:
            raise ValueError("track() serves a tracker of one sequence; use update() for several")
        k = torch.as_tensor(outputs["keypoints"])
        _native._require_cuda(k, "outputs['keypoints']")
        dev, B = k.device, k.shape[0]
        pk = keypoints_tensor(outputs, B)
        P = pk.shape[1]
        boxes = person_boxes(outputs, B, P, dev)
        if boxes is None:
            raise ValueError("PoseTracker.track needs outputs['boxes']: the pose areas come from the person boxes")
        scale = _scale_tensor(sizes, B, dev)
        area = boxes[..., 2] * boxes[..., 3] * scale[:, 0:1] * scale[:, 1:2] * float(area_factor)
        peaks = outputs.get("heatmap") is not None or outputs.get("keypoint_peaks") is not None
        kconf = keypoint_peaks(outputs) if peaks else None
        if rescore and outputs.get("heatmap") is None and kconf is not None:
            scores = pose_scores(outputs, rescore=False) * kconf.mean(-1)    # pose_scores' product on the given peaks
        else:
            scores = pose_scores(outputs, rescore)
        res = self.update(pk, scores, area, scale, kconf)
        out = dict(outputs)
        out["track_ids"], out["track_hits"], out["track_oks"] = res["track_id"], res["track_hits"], res["track_oks"]
        out["track_counts"], out["track_scores"] = res["counts"], scores
        if self.smooth:
            out["keypoints_raw"] = outputs["keypoints"]
            out["keypoints"] = res["keypoints"].reshape(k.shape).to(k.dtype)
        return out
