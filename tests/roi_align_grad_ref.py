"""Plain fp64 reference of kpd_roi_align_backward (csrc/roi_align_grad.hip):
the exact adjoint of tests/ops_ref.py:roi_align_ref, built from the same
``_axis`` -- the fp32 sample coordinates and decisions the forward reference is
pinned with -- as  dF[c] = sum over an image's ROIs of My^T . G[c] . Mx / count,
scattered through topk.  No device code.

The device tolerance is derived, not measured.  A gfeat element is a sum of N
terms  My[p,y] Mx[q,x] G[c,p,q] / count  (the non-zero weights only); the
kernel rounds the two weights to fp32 once each (1 / count folded into one of
them, from doubles), multiplies them (one rounding) and adds the products by
fma in a fixed order (one rounding per term), so
    |got - want| <= (N + 3) 2^-24 S  <=  (N + 2) 2^-23 S,   S = sum |term|,
the fixed-order fp32 sum bound in the spirit of ops_ref.roi_align_bound.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ops_ref import F32, _axis

SIDE = 56


def boxes_to_rois(boxes, rows, H: int, W: int) -> torch.Tensor:
    """cxcywh boxes [B,P,4] -> rois [n,5] (image, x1, y1, x2, y2) on an H x W map
    for the rows ``rows`` by the forward's rule (roi_row_sample): corners clamped
    to [0, 1] and scaled, every operation in fp32."""
    bx = np.asarray(torch.as_tensor(boxes).detach().cpu().float().numpy(), F32)
    P = bx.shape[1]
    flat = bx.reshape(-1, 4)
    out = np.zeros((len(rows), 5), F32)
    for i, r in enumerate(int(v) for v in rows):
        cx, cy, bw, bh = flat[r]
        half_w, half_h = F32(bw / F32(2)), F32(bh / F32(2))
        clamp = lambda v: min(max(F32(v), F32(0)), F32(1))   # noqa: E731
        out[i] = (r // P, F32(clamp(cx - half_w) * F32(W)), F32(clamp(cy - half_h) * F32(H)),
                  F32(clamp(cx + half_w) * F32(W)), F32(clamp(cy + half_h) * F32(H)))
    return torch.from_numpy(out)


def roi_matrices(roi, H: int, W: int):
    """(My [56,H], Mx [56,W], count, (gh, gw)) of one roi (image, x1, y1, x2, y2), fp32 decisions."""
    x1, y1, x2, y2 = (F32(v) for v in np.asarray(roi, F32)[1:])
    rw, rh = max(F32(x2 - x1), F32(1.0)), max(F32(y2 - y1), F32(1.0))
    bh, bw = F32(rh / F32(SIDE)), F32(rw / F32(SIDE))
    gh, gw = int(math.ceil(F32(rh / F32(SIDE)))), int(math.ceil(F32(rw / F32(SIDE))))
    My, _ = _axis(y1, bh, SIDE, gh, H)
    Mx, _ = _axis(x1, bw, SIDE, gw, W)
    return My, Mx, max(gh * gw, 1), (gh, gw)


def roi_align_grad_ref(gout, boxes, rows, topk, C: int, H: int, W: int):
    """gout [n,Cs,56,56], boxes [B,P,4], rows (ascending indices into B*P), topk
    [B,Cs] or None -> (gfeat [B,C,H,W] fp64, S [B,C,H,W] = sum |term|, N [B,C,H,W]
    = the number of terms), ROIs of an image summed in row order."""
    g = torch.as_tensor(gout).detach().cpu().double().numpy()
    B, P = torch.as_tensor(boxes).shape[:2]
    rows = [int(v) for v in rows]
    rois = boxes_to_rois(boxes, rows, H, W).numpy()
    tk = None if topk is None else torch.as_tensor(topk).detach().cpu().long().numpy()
    gfeat = np.zeros((B, C, H, W), np.float64)
    S = np.zeros_like(gfeat)
    N = np.zeros((B, C, H, W), np.int64)
    for i, r in enumerate(rows):
        b = r // P
        My, Mx, count, _ = roi_matrices(rois[i], H, W)
        d = np.einsum("ph,cpq,qw->chw", My, g[i], Mx) / count
        s = np.einsum("ph,cpq,qw->chw", My, np.abs(g[i]), Mx) / count
        nn = np.outer((My != 0).sum(axis=0), (Mx != 0).sum(axis=0))
        ch = np.arange(g.shape[1]) if tk is None else tk[b]
        gfeat[b, ch] += d
        S[b, ch] += s
        N[b, ch] += nn
    return gfeat, S, N


def roi_align_grad_bound(S: np.ndarray, N: np.ndarray) -> np.ndarray:
    """(N + 2) 2^-23 S per element (module docstring)."""
    return (N + 2) * 2.0 ** -23 * S


# ------------------------------------------------------------------ the shared cases
def edge_boxes() -> torch.Tensor:
    """[2,3,4]: image 0 = the whole image, a box thinner than a pixel in both axes
    (a size-1 ROI: all 56 x 56 bins on a patch of at most 3 x 3 pixels), a box hanging over the
    top-left corner; image 1 = a box over the bottom-right corner, a small box
    inside it at the very corner (overlap; samples past the edge are skipped, the
    lo >= size - 1 clamp), an all-zero padding box (the size-1 ROI at the origin)."""
    return torch.tensor([[[0.5, 0.5, 1.0, 1.0], [0.4, 0.6, 0.001, 0.002], [0.05, 0.05, 0.4, 0.3]],
                         [[0.9, 0.92, 0.4, 0.3], [0.97, 0.96, 0.02, 0.03], [0.0, 0.0, 0.0, 0.0]]], dtype=torch.float32)


ROW_SETS = {"labelled": [0, 1, 2, 3, 4], "with_padding": [0, 1, 2, 3, 4, 5], "image0_empty": [3, 4],
            "image1_empty": [0, 1, 2]}


def shuffled_topk(B: int, Cs: int, C: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(C, generator=g)[:Cs] for _ in range(B)]).to(torch.int32)


def sweep_boxes(H: int, W: int, count: int) -> torch.Tensor:
    """[1,count,4]: extents swept over [1, W] (ascending) and [1, H] (descending)
    at shifting sub-pixel offsets -- every band length and footprint size the
    compact tables of the kernel can meet on this map."""
    out = []
    for k in range(count):
        t = k / max(count - 1, 1)
        sx, sy = 1.0 + t * (W - 1), H - t * (H - 1)
        x1 = (0.37 * (k + 1)) % 1.0 * (W - sx)
        y1 = (0.61 * (k + 1)) % 1.0 * (H - sy)
        out.append([(x1 + sx / 2) / W, (y1 + sy / 2) / H, sx / W, sy / H])
    return torch.tensor([out], dtype=torch.float32)


def compact_table_size(M: np.ndarray) -> int:
    """footprint x longest band of one axis matrix M [56,size], as the kernel
    lays its table out: bin p covers the columns from its first sample's lo to
    its last sample's hi (lo + 1 also where the weight there is 0)."""
    size = M.shape[1]
    first = np.full(size, 10 ** 9)
    last = np.full(size, -1)
    for p in range(M.shape[0]):
        nz = np.nonzero(M[p])[0]
        if len(nz) == 0:
            continue
        a, b = nz[0], min(nz[-1] + 1, size - 1)
        first[a:b + 1] = np.minimum(first[a:b + 1], p)
        last[a:b + 1] = np.maximum(last[a:b + 1], p)
    cols = np.nonzero(last >= 0)[0]
    if len(cols) == 0:
        return 0
    return int(cols[-1] - cols[0] + 1) * int((last[cols] - first[cols] + 1).max())
