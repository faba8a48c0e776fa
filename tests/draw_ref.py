"""Numpy restatement of the pose-overlay drawing rules (DESIGN.md §3b,
kpd_draw_poses).  A helper for tests/test_draw.py and
tests/test_predict_outputs.py, not a test module.

Every primitive is evaluated on the whole image from the written rule -- no
bounding boxes, no tiles, no culling -- in int64, so nothing here shares the
kernel's structure.  The only floating-point steps are the ones the rules
name: the fp32 multiply + round-half-even of the quantisation, the fp32 box
corners, and floor(m * 256) of the heat.
"""
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

BOXES, LIMBS, JOINTS, HEAT = 1, 2, 4, 8
ALL = BOXES | LIMBS | JOINTS | HEAT
QMAX = 1 << 20


@dataclass
class Style:
    limbs: Sequence[Tuple[int, int]] = ()
    limb_colors: Sequence[Tuple[int, int, int]] = ()
    joint_colors: Sequence[Tuple[int, int, int]] = ((128, 128, 128), (255, 160, 0), (255, 40, 40))
    box_color: Tuple[int, int, int] = (0, 255, 0)
    joint_radius: int = 40
    limb_half_width: int = 16
    box_half_width: int = 12
    alpha: int = 256
    heat_alpha: int = 160
    min_class: int = 0


def style_of(draw_style) -> Style:
    """The package's DrawStyle as a Style (limb colours resolved)."""
    return Style(limbs=tuple(draw_style.limbs), limb_colors=tuple(draw_style.resolved_limb_colors()),
                 joint_colors=tuple(draw_style.joint_colors), box_color=tuple(draw_style.box_color),
                 joint_radius=draw_style.joint_radius, limb_half_width=draw_style.limb_half_width,
                 box_half_width=draw_style.box_half_width, alpha=draw_style.alpha,
                 heat_alpha=draw_style.heat_alpha, min_class=draw_style.min_class)


def quantise(v, size) -> Optional[int]:
    """clamp(int(rint(fp32(v) * fp32(16 * size))), -2^20, 2^20); None for a non-finite v."""
    v = np.float32(v)
    if not np.isfinite(v):
        return None
    with np.errstate(over="ignore"):
        t = np.rint(v * np.float32(16 * size))      # one fp32 multiply, round half to even
    return int(min(max(float(t), -float(QMAX)), float(QMAX)))


def quantise_box(b, W, H):
    """(X0, Y0, X1, Y1) of a cxcywh row, or None: non-finite corner or an empty quantised box."""
    cx, cy, w, h = (np.float32(v) for v in b)
    with np.errstate(all="ignore"):
        hw, hh = np.float32(0.5) * w, np.float32(0.5) * h
        q = (quantise(cx - hw, W), quantise(cy - hh, H), quantise(cx + hw, W), quantise(cy + hh, H))
    if any(v is None for v in q) or q[2] <= q[0] or q[3] <= q[1]:
        return None
    return q


def joint_class(row) -> int:
    row = np.asarray(row, np.float32)
    return -1 if not row.any() else int(np.argmax(row))     # argmax: the first maximum


def blend(out, mask, color, a):
    """v' = (v * (256 - a) + c * a + 128) >> 8 on the masked pixels; color and a may be per-pixel arrays."""
    color = np.broadcast_to(np.asarray(color, np.int64), out.shape)
    a = np.broadcast_to(np.asarray(a, np.int64)[..., None] if np.ndim(a) else np.int64(a), out.shape)
    new = (out * (256 - a) + color * a + 128) >> 8
    out[mask] = new[mask]


def draw_one(img, kp, vis, boxes, heat, st: Style, flags: int) -> np.ndarray:
    """img [H,W,3] u8; kp [P,K,2]; vis [P,K,3]; boxes [P,4] or None; heat [P,K,hh,hw] or None."""
    H, W = img.shape[:2]
    out = img.astype(np.int64)
    Cx = (16 * np.arange(W, dtype=np.int64) + 8)[None, :]
    Cy = (16 * np.arange(H, dtype=np.int64) + 8)[:, None]
    P, K = kp.shape[:2]
    person = [boxes is None or bool((np.asarray(boxes[p], np.float32) != 0).any()) for p in range(P)]
    qbox = [quantise_box(boxes[p], W, H) if boxes is not None and person[p] else None for p in range(P)]
    if flags & HEAT:
        hh, hw = heat.shape[-2:]
        for p in range(P):
            if qbox[p] is None:
                continue
            X0, Y0, X1, Y1 = qbox[p]
            mask = (Cx >= X0) & (Cx < X1) & (Cy >= Y0) & (Cy < Y1)
            col = np.clip(((Cx - X0) * hw) // (X1 - X0), 0, hw - 1)
            row = np.clip(((Cy - Y0) * hh) // (Y1 - Y0), 0, hh - 1)
            with np.errstate(all="ignore"):
                m = np.fmax.reduce(np.asarray(heat[p], np.float32), axis=0)        # NaN entries ignored
                q = np.where(m > 0, np.minimum(np.floor(m * np.float32(256)), 255), 0)
            q = np.nan_to_num(q, nan=0.0).astype(np.int64)
            qv = q[np.broadcast_to(row, mask.shape), np.broadcast_to(col, mask.shape)]
            color = np.stack([np.minimum(255, 3 * qv), np.clip(3 * qv - 255, 0, 255), np.clip(3 * qv - 510, 0, 255)],
                             axis=-1)
            blend(out, mask, color, (qv * st.heat_alpha) >> 8)
    r, h, hb = st.joint_radius, st.limb_half_width, st.box_half_width
    for p in range(P):
        if not person[p]:
            continue
        if flags & BOXES and qbox[p] is not None:
            X0, Y0, X1, Y1 = qbox[p]
            outer = (Cx >= X0 - hb) & (Cx <= X1 + hb) & (Cy >= Y0 - hb) & (Cy <= Y1 + hb)
            inner = (Cx > X0 + hb) & (Cx < X1 - hb) & (Cy > Y0 + hb) & (Cy < Y1 - hb)
            blend(out, outer & ~inner, st.box_color, st.alpha)
        joints = []     # (X, Y, class) of the drawn joints, else None
        for k in range(K):
            c = joint_class(vis[p, k])
            X, Y = quantise(kp[p, k, 0], W), quantise(kp[p, k, 1], H)
            joints.append((X, Y, c) if c >= 0 and c >= st.min_class and X is not None and Y is not None else None)
        if flags & LIMBS:
            for (a, b), color in zip(st.limbs, st.limb_colors):
                if joints[a] is None or joints[b] is None:
                    continue
                ax, ay = joints[a][:2]
                dx, dy = joints[b][0] - ax, joints[b][1] - ay
                dd = dx * dx + dy * dy
                if dd <= 0:
                    continue
                T = math.isqrt(h * h * dd)          # (p x d)^2 <= h^2 dd  <=>  |p x d| <= isqrt(h^2 dd)
                px, py = Cx - ax, Cy - ay
                dot, cross = px * dx + py * dy, px * dy - py * dx
                blend(out, (dot >= 0) & (dot <= dd) & (np.abs(cross) <= T), color, st.alpha)
        if flags & JOINTS:
            for j in joints:
                if j is not None:
                    blend(out, (Cx - j[0]) ** 2 + (Cy - j[1]) ** 2 <= r * r, st.joint_colors[j[2]], st.alpha)
    return out.astype(np.uint8)


def draw_ref(images, keypoints, visibilities, boxes, heatmap, st: Style, flags: int = ALL):
    """images: list of [H,W,3] u8; keypoints [n,P,K,2]; visibilities [n,P,K,3]; boxes [n,P,4] or None;
    heatmap [n,P,K,hh,hw] or None -> list of drawn copies."""
    return [draw_one(np.asarray(img), np.asarray(keypoints[i], np.float32), np.asarray(visibilities[i], np.float32),
                     None if boxes is None else np.asarray(boxes[i], np.float32),
                     None if heatmap is None else np.asarray(heatmap[i], np.float32), st, flags)
            for i, img in enumerate(images)]
