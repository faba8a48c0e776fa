"""Numpy float64 restatement of COCO keypoint evaluation as kpd_oks_match
(csrc/oks.hip) and dll.utils.OksEvaluator implement it: COCOeval's computeOks,
evaluateImg (keypoints, area range "all", no crowd annotations), accumulate
and summarize, written as plain loops in COCOeval's own structure from the
rules in DESIGN.md §3c.  Deliberately not shaped like the kernel: per image,
per detection, per ground truth, per keypoint.

Inputs are the arrays the kernel receives (fp32); every difference and sum of
squares is formed in float64 from them, in the rules' operation order.
"""
import numpy as np

EPS = float(np.spacing(1))   # 2^-52
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
COCO_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_GRID = np.linspace(0, 1, 101)


def _as32(a):
    """What the kernel sees of a table: fp32 values, here widened to float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def labelled(gt_vis_row):
    return [k for k in range(len(gt_vis_row)) if gt_vis_row[k] > 0]


def oks_one(dk, gk, gv, box, area, scale, sigmas):
    """OKS of one detection [K,2] against one ground truth (computeOks' inner loop)."""
    sx, sy = float(scale[0]), float(scale[1])
    K = len(sigmas)
    lab = labelled(gv)
    k1 = len(lab)
    pos = lambda v: v if v > 0 else 0.0     # noqa: E731
    if k1 == 0:
        cx, cy, w, h = (float(v) for v in box)
        xtl, ytl = (cx - w / 2.0) * sx, (cy - h / 2.0) * sy
        W, H = w * sx, h * sy
        x0, x1, y0, y1 = xtl - W, xtl + 2.0 * W, ytl - H, ytl + 2.0 * H
    total, n = 0.0, 0
    for k in (lab if k1 > 0 else range(K)):
        xd, yd = sx * float(dk[k][0]), sy * float(dk[k][1])
        if k1 > 0:
            dx = xd - sx * float(gk[k][0])
            dy = yd - sy * float(gk[k][1])
        else:
            dx = pos(x0 - xd) + pos(xd - x1)
            dy = pos(y0 - yd) + pos(yd - y1)
        s2 = 2.0 * float(sigmas[k])
        var = s2 * s2
        e = (dx * dx + dy * dy) / var / (float(area) + EPS) / 2.0
        total += float(np.exp(-e))
        n += 1
    return total / n


def evaluate_img(pred_kpts, pred_scores, gt_kpts, gt_vis, gt_boxes, gt_area, n_gt, scale, sigmas, thresholds,
                 max_dets):
    """One image.  Returns the kernel's outputs for it: oks [D,G], det_score
    [M], det_slot [M], det_match [T,M], det_ignore [T,M], gt_match [T,G],
    counts (n_det, n_gt_counted)."""
    sig, thr = _as32(sigmas), _as32(thresholds)
    D, G, T = len(pred_scores), len(gt_kpts), len(thr)
    M = min(max_dets, D)
    n_gt = min(max(int(n_gt), 0), G)
    present = [d for d in range(D) if pred_scores[d] > 0]            # a NaN is not > 0
    dt = sorted(present, key=lambda d: -float(pred_scores[d]))[:max_dets]     # stable: ties keep slot order
    ign = [len(labelled(gt_vis[g])) == 0 for g in range(n_gt)]
    gorder = sorted(range(n_gt), key=lambda g: ign[g])                # stable: counted first, slot order within
    oks = np.zeros((D, G))
    for d in present:
        for g in range(n_gt):
            oks[d, g] = oks_one(pred_kpts[d], gt_kpts[g], gt_vis[g], gt_boxes[g], gt_area[g], scale, sig)
    dtm = -np.ones((T, M), np.int32)
    dtig = np.zeros((T, M), np.uint8)
    gtm = -np.ones((T, G), np.int32)
    for ti in range(T):
        for r, d in enumerate(dt):
            best = min(float(thr[ti]), 1 - 1e-10)
            m = -1
            for g in gorder:
                if gtm[ti, g] >= 0:
                    continue
                if m > -1 and not ign[m] and ign[g]:
                    break
                if oks[d, g] < best:
                    continue
                best = oks[d, g]
                m = g
            if m == -1:
                continue
            dtig[ti, r] = ign[m]
            dtm[ti, r] = m
            gtm[ti, m] = d
    score = np.zeros(M, np.float32)
    slot = -np.ones(M, np.int32)
    for r, d in enumerate(dt):
        score[r], slot[r] = pred_scores[d], d
    return {"oks": oks, "det_score": score, "det_slot": slot, "det_match": dtm, "det_ignore": dtig, "gt_match": gtm,
            "counts": np.array([len(dt), n_gt - sum(ign)], np.int32)}


def evaluate_batch(pred_kpts, pred_scores, gt_kpts, gt_vis, gt_boxes, gt_area, n_gt, scale, sigmas=COCO_SIGMAS,
                   thresholds=COCO_THRESHOLDS, max_dets=20):
    """evaluate_img per image of a batch, stacked: the output arrays of one kpd_oks_match call."""
    B = len(pred_kpts)
    imgs = [evaluate_img(pred_kpts[b], pred_scores[b], gt_kpts[b], gt_vis[b], gt_boxes[b], gt_area[b], n_gt[b],
                         scale[b], sigmas, thresholds, max_dets) for b in range(B)]
    D, G, T = pred_scores.shape[1], gt_kpts.shape[1], len(thresholds)
    M = min(max_dets, D)
    empty = {"oks": (0, D, G), "det_score": (0, M), "det_slot": (0, M), "det_match": (0, T, M),
             "det_ignore": (0, T, M), "gt_match": (0, T, G), "counts": (0, 2)}
    return {k: np.stack([i[k] for i in imgs]) if imgs else np.zeros(s) for k, s in empty.items()}


def accumulate(batches, thresholds=COCO_THRESHOLDS):
    """COCOeval.accumulate over evaluate_batch results in order: precision
    [T,101] and recall [T], -1 everywhere without a counted ground truth."""
    T, R = len(thresholds), len(RECALL_GRID)
    precision = -np.ones((T, R))
    recall = -np.ones(T)
    scores, dtm, dtig, npig = [np.zeros(0)], [np.zeros((T, 0), bool)], [np.zeros((T, 0), bool)], 0
    for res in batches:
        for b in range(len(res["counts"])):
            nd = int(res["counts"][b][0])
            scores.append(res["det_score"][b][:nd])
            dtm.append(res["det_match"][b][:, :nd] >= 0)
            dtig.append(res["det_ignore"][b][:, :nd] != 0)
            npig += int(res["counts"][b][1])
    if npig == 0:
        return precision, recall
    scores = np.concatenate(scores)
    inds = np.argsort(-scores, kind="mergesort")
    dtm = np.concatenate(dtm, axis=1)[:, inds]
    dtig = np.concatenate(dtig, axis=1)[:, inds]
    tps = np.logical_and(dtm, np.logical_not(dtig))
    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
    tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
    fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
        nd = len(tp)
        rc = tp / npig
        pr = (tp / (fp + tp + EPS)).tolist()
        q = [0.0] * R
        recall[t] = rc[-1] if nd else 0
        for i in range(nd - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        for ri, pi in enumerate(np.searchsorted(rc, RECALL_GRID, side="left")):
            if pi >= nd:
                break
            q[ri] = pr[pi]
        precision[t] = q
    return precision, recall


def summarize(precision, recall, thresholds=COCO_THRESHOLDS):
    """COCOeval.summarize's four keypoint numbers we report."""
    thr = np.asarray(thresholds, np.float64)

    def mean(a):
        a = a[a > -1]
        return float(np.mean(a)) if a.size else -1.0

    i50, i75 = int(np.abs(thr - 0.5).argmin()), int(np.abs(thr - 0.75).argmin())
    return {"oks_AP": mean(precision), "oks_AP50": mean(precision[i50]), "oks_AP75": mean(precision[i75]),
            "oks_AR": mean(recall)}


def average_precision(batches, thresholds=COCO_THRESHOLDS):
    return summarize(*accumulate(batches, thresholds), thresholds)


def margins(oks, thresholds=COCO_THRESHOLDS):
    """How far a case is from a decision that rounding could flip: (the
    smallest |oks - min(t, 1 - 1e-10)| over all entries and thresholds, the
    smallest gap between two different OKS values of one detection's row that
    both reach the lowest threshold).  inf where nothing qualifies."""
    oks = np.asarray(oks, np.float64)
    thr = np.minimum(_as32(thresholds), 1 - 1e-10)
    a = float(np.abs(oks[..., None] - thr).min()) if oks.size else np.inf
    gap = np.inf
    for row in oks.reshape(-1, oks.shape[-1]) if oks.size else []:
        v = np.unique(row[row >= thr.min()])
        if len(v) > 1:
            gap = min(gap, float(np.diff(v).min()))
    return a, gap
