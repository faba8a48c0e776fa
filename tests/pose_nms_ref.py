"""Numpy float64 restatement of OKS pose-NMS as kpd_pose_nms
(csrc/pose_nms.hip) implements it, written as plain loops from the rules in
DESIGN.md §3d: per image, per pick, per pose, per keypoint.  Deliberately not
shaped like the kernel: no matrix is kept for the decisions, the loop is the
classic ``while order:`` of greedy NMS, which recomputes the overlaps of the
remaining poses against the current pick.

Inputs are the arrays the kernel receives (fp32); every difference, sum of
squares and score product is formed in float64 from them, in the rules'
operation order.  threshold, vis_threshold and min_score are taken as the fp32
values the C call receives.
"""
import math

import numpy as np

EPS = float(np.spacing(1))   # 2^-52
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
MODES = ("hard", "soft", "soft_linear")


def _as32(a):
    """What the kernel sees of a table or a scalar: fp32 values, here widened to float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def pair_oks(ki, kj, ci, cj, area_i, area_j, scale, sigmas, vis_threshold):
    """OKS of two poses [K,2]; ci / cj: their keypoint confidences [K] or None."""
    sx, sy = float(scale[0]), float(scale[1])
    den = (float(area_i) + float(area_j)) / 2.0 + EPS
    vt = np.float32(vis_threshold)
    total, n = 0.0, 0
    for k in range(len(sigmas)):
        if ci is not None and not (ci[k] > vt and cj[k] > vt):
            continue
        dx = sx * float(ki[k][0]) - sx * float(kj[k][0])
        dy = sy * float(ki[k][1]) - sy * float(kj[k][1])
        s2 = 2.0 * float(sigmas[k])
        var = s2 * s2
        e = (dx * dx + dy * dy) / var / den / 2.0
        total += math.exp(-e)
        n += 1
    return total / n if n else 0.0


def nms_img(kpts, scores, area, kconf, scale, sigmas=COCO_SIGMAS, threshold=0.9, mode="hard", vis_threshold=0.2,
            max_keep=20, min_score=0.0):
    """One image.  Returns the kernel's outputs for it (oks [D,D], keep [D],
    n_keep, scores_out [D], suppressed_by [D]) and ``gaps``: per soft-mode pick
    the relative gap between the best and the second-best current score."""
    assert mode in MODES
    sig = _as32(sigmas)
    thr, smin = float(np.float32(threshold)), float(np.float32(min_score))
    D = len(scores)
    present = [d for d in range(D) if scores[d] > 0]            # a NaN is not > 0

    def overlap(i, j):     # the same operands in the same order whichever way it is asked
        a, b = min(i, j), max(i, j)
        return pair_oks(kpts[a], kpts[b], None if kconf is None else kconf[a], None if kconf is None else kconf[b],
                        area[a], area[b], scale, sig, vis_threshold)

    oks = np.zeros((D, D))
    for i in present:
        for j in present:
            if i != j:
                oks[i, j] = overlap(i, j)
    keep, out, sup, gaps = [], np.zeros(D, np.float32), -np.ones(D, np.int32), []
    if mode == "hard":
        order = sorted(present, key=lambda d: -float(scores[d]))       # stable: ties keep slot order
        rank = {d: r for r, d in enumerate(order)}
        # the walk reaches the ranks below `end`: up to the first score that is not > min_score ...
        end = next((r for r, d in enumerate(order) if not float(scores[d]) > smin), len(order))
        while order:
            d = order.pop(0)
            if not float(scores[d]) > smin:
                break
            keep.append(d)
            out[d] = scores[d]
            if len(keep) == max_keep:         # ... or to the pose that fills the list
                end = rank[d] + 1
                break
            rest = []
            for j in order:     # what the pick suppresses leaves the list now: its earliest-kept suppressor
                if overlap(d, j) > thr:
                    sup[j] = d
                else:
                    rest.append(j)
            order = rest
        for j in present:       # a pose the walk never reached was not examined
            if rank[j] >= end:
                sup[j] = -1
    else:
        cur = {d: float(scores[d]) for d in present}
        order = list(present)
        while order and len(keep) < max_keep:
            d = max(order, key=lambda j: (cur[j], -j))           # highest current score, ties to the lower slot
            if not cur[d] > smin:
                break
            second = [cur[j] for j in order if j != d]
            if second and max(second) != cur[d]:
                gaps.append((cur[d] - max(second)) / abs(cur[d]))
            order.remove(d)
            keep.append(d)
            out[d] = np.float32(cur[d])
            for j in order:
                o = overlap(d, j)
                if mode == "soft":
                    cur[j] = cur[j] * math.exp(-(o * o) / thr)
                else:
                    cur[j] = cur[j] * ((1.0 - o) if o >= thr else 1.0)
    keep_arr = -np.ones(D, np.int32)
    keep_arr[:len(keep)] = keep
    return {"oks": oks, "keep": keep_arr, "n_keep": np.int32(len(keep)), "scores_out": out, "suppressed_by": sup,
            "gaps": gaps, "present": np.array([d in present for d in range(D)], bool)}


def nms_batch(kpts, scores, area, scale, kconf=None, **kw):
    """nms_img per image of a batch, stacked: the output arrays of one kpd_pose_nms call (+ gaps, present)."""
    B, D = scores.shape
    imgs = [nms_img(kpts[b], scores[b], area[b], None if kconf is None else kconf[b], scale[b], **kw)
            for b in range(B)]
    empty = {"oks": ((0, D, D), np.float64), "keep": ((0, D), np.int32), "n_keep": ((0,), np.int32),
             "scores_out": ((0, D), np.float32), "suppressed_by": ((0, D), np.int32), "present": ((0, D), bool)}
    res = {k: np.stack([i[k] for i in imgs]) if imgs else np.zeros(s, t) for k, (s, t) in empty.items()}
    res["gaps"] = [g for i in imgs for g in i["gaps"]]
    return res


def margins(ref, threshold, mode):
    """How far a case is from a decision that rounding could flip: (the
    smallest |OKS - threshold| over the pairs of present poses, for the soft
    modes the smallest relative gap between the best and the second-best
    current score at any pick, an exact tie excluded -- it is decided by the
    slot).  inf where nothing qualifies."""
    thr = float(np.float32(threshold))
    a = np.inf
    for o, p in zip(ref["oks"], ref["present"]):
        pair = p[:, None] & p[None, :] & ~np.eye(len(p), dtype=bool)
        if pair.any():
            a = min(a, float(np.abs(o[pair] - thr).min()))
    gap = min(ref["gaps"]) if mode != "hard" and ref["gaps"] else np.inf
    return a, gap
