"""Pose overlays drawn on the device (``kpd_draw_poses``, csrc/draw.hip) and
the YOLO-pose label text of a prediction.

``draw_poses`` takes the images a forward ran on and that forward's output
dict and returns the overlays as uint8 HWC device tensors: person boxes,
skeleton limbs, joints and, on request, the max-over-keypoints heatmap as an
underlay in a "hot" colour map.  The output tensors are read in place, the
images may have different sizes, and nothing returns to the host.  The
drawing rules are integer arithmetic; ``tests/draw_ref.py``
restates them in numpy.

There is no CPU fallback: drawing needs the HIP device.  ``person_boxes``,
``joint_classes`` and ``format_pose_labels`` are plain tensor code and run
anywhere.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native

# COCO-17 skeleton, 0-based joint indices (the 19 limbs of the COCO keypoint annotation)
COCO_SKELETON: Tuple[Tuple[int, int], ...] = (
    (15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10),
    (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))

_LEG, _TORSO, _ARM, _HEAD = (60, 200, 90), (240, 200, 40), (60, 150, 255), (255, 110, 180)
_COCO_LIMB_COLORS = (_LEG,) * 4 + (_TORSO,) * 4 + (_ARM,) * 4 + (_HEAD,) * 7

LAYERS = {"boxes": _native.DRAW_BOXES, "limbs": _native.DRAW_LIMBS, "joints": _native.DRAW_JOINTS,
          "heat": _native.DRAW_HEAT}
DEFAULT_LAYERS = ("boxes", "limbs", "joints")


@dataclass(frozen=True)
class DrawStyle:
    """Tables and integers of ``kpd_draw_poses``.  Lengths are in 1/16-pixel
    units (at most 512 = 32 px), alphas in [0, 256].  ``joint_colors`` holds
    one colour per visibility class; joints below ``min_class`` (and the limbs
    that touch them) are not drawn."""
    limbs: Tuple[Tuple[int, int], ...] = COCO_SKELETON
    limb_colors: Optional[Tuple[Tuple[int, int, int], ...]] = None   # None: the COCO palette / one colour
    joint_colors: Tuple[Tuple[int, int, int], ...] = ((128, 128, 128), (255, 160, 0), (255, 40, 40))
    box_color: Tuple[int, int, int] = (0, 255, 0)
    joint_radius: int = 40        # 2.5 px
    limb_half_width: int = 16     # a 2 px line
    box_half_width: int = 12      # a 1.5 px outline
    alpha: int = 256
    heat_alpha: int = 160
    min_class: int = 1

    def resolved_limb_colors(self) -> Tuple[Tuple[int, int, int], ...]:
        if self.limb_colors is not None:
            if len(self.limb_colors) != len(self.limbs):
                raise ValueError("DrawStyle: limb_colors needs one colour per limb")
            return tuple(tuple(c) for c in self.limb_colors)
        if tuple(map(tuple, self.limbs)) == COCO_SKELETON:
            return _COCO_LIMB_COLORS
        return (_ARM,) * len(self.limbs)


def layer_flags(layers: Sequence[str]) -> int:
    flags = 0
    for name in layers:
        if name not in LAYERS:
            raise ValueError(f"unknown layer {name!r}; choose from {sorted(LAYERS)}")
        flags |= LAYERS[name]
    return flags


def keypoints_tensor(outputs: Dict, n: int) -> torch.Tensor:
    """[n, P, K, 2] fp32: the memory of the forward's [n, P, 1, K, 2]."""
    k = torch.as_tensor(outputs["keypoints"])
    if k.shape[-1] != 2 or k.dim() < 3:
        raise ValueError(f"keypoints must end in [K, 2], got {tuple(k.shape)}")
    return k.reshape(n, -1, k.shape[-2], 2).to(torch.float32).contiguous()


def visibilities_tensor(outputs: Dict, n: int, P: int, K: int, device) -> torch.Tensor:
    """[n, P, K, 3] fp32 one-hot rows.  Class indices ([n, P, K], the label
    files' ``v``) become one-hot rows; without visibilities every joint is class 2."""
    v = outputs.get("visibilities")
    if v is None:
        v = torch.full((n, P, K), 2, device=device)
    v = torch.as_tensor(v).to(device)
    if v.numel() == n * P * K * 3 and v.shape[-1] == 3:
        return v.reshape(n, P, K, 3).to(torch.float32).contiguous()
    if v.numel() != n * P * K:
        raise ValueError(f"visibilities {tuple(v.shape)} do not match keypoints [{n}, {P}, {K}, 2]")
    cls = v.reshape(n, P, K).to(torch.int64).clamp(0, 2)
    return torch.nn.functional.one_hot(cls, 3).to(torch.float32).contiguous()


def person_boxes(outputs: Dict, n: int, P: int, device) -> Optional[torch.Tensor]:
    """The box of every person slot, [n, P, 4] cxcywh, or None when the
    outputs carry no boxes.  The forward compacts all-zero caller boxes out of
    the person slots, so all-zero rows are dropped here the same way (order
    kept, zero rows at the end); with detector outputs the slots whose
    ``box_scores`` is 0 get zero boxes.  A person is drawn if and only if its
    row here is not all zero."""
    b = outputs.get("boxes")
    if b is None:
        return None
    if isinstance(b, (list, tuple)):
        rows = [torch.as_tensor(x, dtype=torch.float32).to(device).reshape(-1, 4) for x in b]
        if len(rows) != n:
            raise ValueError(f"boxes describe {len(rows)} images, the outputs {n}")
        q = max([r.shape[0] for r in rows] + [1])
        if all(r.shape[0] == q for r in rows):   # the forward's list: equal lengths, one copy
            bt = torch.stack(rows)
        else:
            bt = torch.zeros(n, q, 4, device=device)
            for i, r in enumerate(rows):
                bt[i, :r.shape[0]] = r
    else:
        bt = torch.as_tensor(b).to(device, torch.float32).reshape(n, -1, 4)
    scores = outputs.get("box_scores")
    if scores is not None:   # detector slots are already in output order
        keep = torch.as_tensor(scores).to(device).reshape(n, -1, 1) > 0
        bt = torch.where(keep, bt, torch.zeros_like(bt))
    else:
        zero = ~(bt != 0).any(-1)
        order = torch.argsort(zero.to(torch.int8), dim=1, stable=True)
        bt = torch.gather(bt, 1, order[..., None].expand(-1, -1, 4))
    out = torch.zeros(n, P, 4, device=device)
    q = min(P, bt.shape[1])
    out[:, :q] = bt[:, :q]
    return out


def joint_classes(vis: torch.Tensor) -> torch.Tensor:
    """Visibility class of one-hot rows [..., 3]: the index of the first
    maximum, -1 for an all-zero row (a padding person) -- the renderer's rule."""
    a, b, c = vis[..., 0], vis[..., 1], vis[..., 2]
    k = torch.zeros_like(a, dtype=torch.int64)
    m = a.clone()
    k = torch.where(b > m, torch.ones_like(k), k)
    m = torch.where(b > m, b, m)
    k = torch.where(c > m, torch.full_like(k, 2), k)
    return torch.where((a == 0) & (b == 0) & (c == 0), torch.full_like(k, -1), k)


def _device_image(img, device, inplace: bool) -> torch.Tensor:
    """uint8 [H, W, 3] on ``device`` whose pixels are dense within a row."""
    if inplace:
        ok = (isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.device == device and img.dim() == 3
              and img.shape[2] == 3 and img.stride(2) == 1 and img.stride(1) == 3
              and (img.shape[0] == 1 or img.stride(0) >= 3 * img.shape[1]))
        if not ok:
            raise ValueError("inplace=True needs uint8 [H, W, 3] tensors on the outputs' device with dense rows "
                             "(strides (pitch, 3, 1), pitch >= 3 * W)")
        return img
    if isinstance(img, torch.Tensor):
        t = img
    else:   # PIL image or array-like
        if hasattr(img, "convert") and getattr(img, "mode", "RGB") not in ("RGB", "L"):
            img = img.convert("RGB")
        t = torch.from_numpy(np.array(img, copy=True))
    if t.dtype != torch.uint8:
        raise TypeError("draw_poses expects 8-bit images")
    if t.dim() == 2:
        t = t[:, :, None]
    if t.dim() != 3 or t.shape[2] not in (1, 3):
        raise ValueError(f"draw_poses expects [H, W], [H, W, 1] or [H, W, 3] images, got {tuple(t.shape)}")
    t = t.to(device, non_blocking=True)
    return t.expand(-1, -1, 3).contiguous() if t.shape[2] == 1 else t.clone(memory_format=torch.contiguous_format)


def draw_poses(images, outputs: Dict, *, style: Optional[DrawStyle] = None,
               layers: Sequence[str] = DEFAULT_LAYERS, inplace: bool = False) -> List[torch.Tensor]:
    """Draw a forward's ``outputs`` onto its ``n`` images in one native call.

    ``images``: PIL images, numpy arrays or uint8 tensors, on host or device,
    of any sizes; [H, W] and 1-channel inputs are replicated to RGB.
    ``outputs``: the forward's dict for those images ('keypoints',
    'visibilities', and for the box and heat layers 'boxes' (+ 'box_scores')
    and 'heatmap').  ``layers``: any of "boxes", "limbs", "joints", "heat".
    ``inplace=True`` draws into the caller's device tensors (pitched views
    included) instead of copies.  Returns the uint8 [H, W, 3] device tensors."""
    if isinstance(images, torch.Tensor) and images.dim() <= 3 or not isinstance(images, (list, tuple, torch.Tensor)):
        images = [images]
    images = list(images)
    n = len(images)
    if n == 0:
        raise ValueError("draw_poses needs at least one image")
    style = style or DrawStyle()
    flags = layer_flags(layers)
    kp = torch.as_tensor(outputs["keypoints"])
    _native._require_cuda(kp, "outputs['keypoints']")
    dev = kp.device
    kp = keypoints_tensor(outputs, n)
    P, K = kp.shape[1], kp.shape[2]
    vis = visibilities_tensor(outputs, n, P, K, dev)
    boxes = person_boxes(outputs, n, P, dev)
    heat = None
    hh = hw = 0
    if flags & _native.DRAW_HEAT:
        heat = outputs.get("heatmap")
        if heat is None:
            raise ValueError("the heat layer needs outputs['heatmap']")
        heat = torch.as_tensor(heat).to(dev, torch.float32)
        hh, hw = heat.shape[-2:]
        heat = heat.reshape(n, P, K, hh, hw).contiguous()
    imgs = [_device_image(im, dev, inplace) for im in images]
    limbs = [int(v) for ab in style.limbs for v in ab]
    L = len(style.limbs)
    lcol = [int(v) for c in style.resolved_limb_colors() for v in c]
    jcol = [int(v) for c in style.joint_colors for v in c]
    if len(jcol) != 9 or len(style.box_color) != 3:
        raise ValueError("DrawStyle: joint_colors is three RGB colours, box_color one")
    ints = ctypes.c_int * n
    u8 = ctypes.c_uint8
    lib = _native.load()
    with torch.cuda.device(dev):
        rc = lib.kpd_draw_poses((ctypes.c_void_p * n)(*[t.data_ptr() for t in imgs]),
                                ints(*[t.shape[0] for t in imgs]), ints(*[t.shape[1] for t in imgs]),
                                ints(*[t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1] for t in imgs]), n,
                                _native._ptr(kp), _native._ptr(vis), _native._ptr(boxes), _native._ptr(heat),
                                P, K, hh, hw, (ctypes.c_int * max(2 * L, 1))(*limbs), L,
                                (u8 * max(3 * L, 1))(*lcol), (u8 * 9)(*jcol), (u8 * 3)(*[int(v) for v in style.box_color]),
                                int(style.joint_radius), int(style.limb_half_width), int(style.box_half_width),
                                int(style.alpha), int(style.heat_alpha), int(style.min_class), flags,
                                _native._stream(dev))
    _native.check(rc, "kpd_draw_poses")
    return imgs


def format_pose_labels(outputs: Dict) -> str:
    """One image's prediction as YOLO-pose label text, the format
    ``OptimizedKeypointsDataset`` parses: per drawn person one line
    ``0 cx cy w h`` followed by K groups ``x y v`` -- coordinates as %.6f, v the
    visibility class (0 for a joint without one).  A person counts as drawn
    under the renderer's rule (``person_boxes``): zero-box persons and detector
    slots with score 0 are absent."""
    kp = keypoints_tensor(outputs, 1).cpu()
    P, K = kp.shape[1], kp.shape[2]
    cls = joint_classes(visibilities_tensor(outputs, 1, P, K, "cpu")).clamp(min=0)
    boxes = person_boxes(outputs, 1, P, "cpu")
    lines = []
    for p in range(P):
        b = boxes[0, p] if boxes is not None else torch.zeros(4)
        if boxes is not None and not bool((b != 0).any()):
            continue
        vals = ["0"] + [f"{float(v):.6f}" for v in b]
        for k in range(K):
            vals += [f"{float(kp[0, p, k, 0]):.6f}", f"{float(kp[0, p, k, 1]):.6f}", str(int(cls[0, p, k]))]
        lines.append(" ".join(vals))
    return "".join(line + "\n" for line in lines)
