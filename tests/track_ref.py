"""Numpy float64 restatement of OKS pose tracking as kpd_track_poses
(csrc/track.hip) implements it, written as plain loops from the rules in
DESIGN.md §3m: per frame, per pick, per track, per pose, per keypoint.
Deliberately not shaped like the kernel: the tracks are a list of dicts that
grows and shrinks (no table, no matrix kept for the decisions), every pick
recomputes the similarities of the tracks and poses that are left, and the
filter state hangs on its track.

Inputs are the arrays the kernel receives (fp32); every difference, sum of
squares and filter term is formed in float64 from them, in the rules' operation
order.  threshold, vis_threshold and the filter constants are taken as the
fp32 values the C call receives.

``track_frames`` also returns what the tests need to show that rounding cannot
flip a decision: per greedy pick its distance to the threshold and to the best
other candidate, and the smallest distance of any examined pair to the
threshold.
"""
import math

import numpy as np

EPS = float(np.spacing(1))   # 2^-52
MAX_TRACKS = 64
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
DEFAULTS = dict(threshold=0.3, vis_threshold=0.2, max_age=10, smooth=True, min_cutoff=1.0, beta=0.05, d_cutoff=1.0,
                fps=30.0)


def _f(v):
    """A scalar as the C call receives it: fp32, widened to float64."""
    return float(np.float32(v))


def new_state():
    """No tracks, next id 0, no frame seen."""
    return {"tracks": [], "next_id": 0, "frames": 0}


def track_pose_oks(track, kj, cj, area_j, scale_j, sigmas, vis_threshold):
    """OKS of a track's last matched raw pose and pose j of the current frame."""
    tsx, tsy = float(track["scale"][0]), float(track["scale"][1])
    sx, sy = float(scale_j[0]), float(scale_j[1])
    den = (float(track["area"]) + float(area_j)) / 2.0 + EPS
    vt = np.float32(vis_threshold)
    total, n = 0.0, 0
    for k in range(len(sigmas)):
        if cj is not None and not (track["kconf"][k] > vt and cj[k] > vt):
            continue
        dx = tsx * float(track["kpts"][k][0]) - sx * float(kj[k][0])
        dy = tsy * float(track["kpts"][k][1]) - sy * float(kj[k][1])
        s2 = 2.0 * float(sigmas[k])
        var = s2 * s2
        e = (dx * dx + dy * dy) / var / den / 2.0
        total += math.exp(-e)
        n += 1
    return total / n if n else 0.0


def _alpha(fc, te):
    r = 2.0 * math.pi * fc * te
    return r / (r + 1.0)


def one_euro_step(x, prev, te, min_cutoff, d_cutoff, beta):
    """(x^, dx^) of one coordinate; ``prev`` = (x^prev, dx^prev) or None."""
    if prev is None:
        return x, 0.0
    xp, dp = prev
    dx = (x - xp) / te
    ad = _alpha(d_cutoff, te)
    dxh = ad * dx + (1.0 - ad) * dp
    fc = min_cutoff + beta * abs(dxh)
    a = _alpha(fc, te)
    return a * x + (1.0 - a) * xp, dxh


def track_frames(kpts, scores, area, scale, kconf=None, state=None, sigmas=COCO_SIGMAS, threshold=0.3,
                 vis_threshold=0.2, max_age=10, smooth=True, min_cutoff=1.0, beta=0.05, d_cutoff=1.0, fps=30.0):
    """B consecutive frames of one sequence: kpts [B,D,K,2], scores [B,D], area
    [B,D], scale [B,2], kconf [B,D,K] or None.  ``state`` (``new_state()`` when
    None) is updated in place and returned with the outputs: track_id,
    track_hits [B,D] int32, track_oks [B,D] float64, keypoints [B,D,K,2] fp32
    (the input without ``smooth``), counts [B,4] int32; ``picks``: per greedy
    pick (distance to the threshold, distance to the best other candidate --
    0.0 marks a bit-equal one); ``pair_margin``: the smallest |OKS - threshold|
    over the examined pairs with a non-zero OKS; ``events``: how often each of
    match, birth, death, reid (a match after a gap) and drop happened."""
    state = new_state() if state is None else state
    sig = np.asarray(sigmas, np.float32).astype(np.float64)
    thr, vt = _f(threshold), np.float32(vis_threshold)
    mc, bt, dc, rate = _f(min_cutoff), _f(beta), _f(d_cutoff), _f(fps)
    B, D = scores.shape
    K = len(sig)
    ids, hits = -np.ones((B, D), np.int32), np.zeros((B, D), np.int32)
    oks_out, counts = np.zeros((B, D)), np.zeros((B, 4), np.int32)
    out = np.array(kpts, np.float32, copy=True)
    picks, pair_margin = [], np.inf
    events = dict(match=0, birth=0, death=0, reid=0, drop=0)
    for f in range(B):
        tracks = state["tracks"]
        poses = [j for j in range(D) if scores[f, j] > 0]            # a NaN is not > 0
        conf = (lambda j: None) if kconf is None else (lambda j: kconf[f, j])

        def candidates(open_tracks, open_poses):
            found = []
            for tr in open_tracks:
                for j in open_poses:
                    o = track_pose_oks(tr, kpts[f, j], conf(j), area[f, j], scale[f], sig, vis_threshold)
                    found.append((o, tr, j))
            return found

        for o, _, _ in candidates(tracks, poses):
            if o != 0.0:
                pair_margin = min(pair_margin, abs(o - thr))
        open_tracks, open_poses, matched = list(tracks), list(poses), []
        while True:
            cand = [c for c in candidates(open_tracks, open_poses) if c[0] > thr]
            if not cand:
                break
            best = max(cand, key=lambda c: (c[0], -c[1]["id"], -c[2]))   # ties: the lower track id, then the lower slot
            others = [c[0] for c in cand if c is not best]
            picks.append((best[0] - thr, best[0] - max(others) if others else np.inf))
            matched.append(best)
            open_tracks = [t for t in open_tracks if t is not best[1]]
            open_poses.remove(best[2])
        updated = []                                                   # (track, slot, frames since its last match or None)
        for o, tr, j in matched:
            step = tr["age"] + 1
            events["match"] += 1
            events["reid"] += tr["age"] > 0
            tr["age"], tr["hits"] = 0, tr["hits"] + 1
            ids[f, j], hits[f, j], oks_out[f, j] = tr["id"], tr["hits"], o
            updated.append((tr, j, step))
        for tr in open_tracks:
            tr["age"] += 1
        dead = [tr for tr in open_tracks if tr["age"] > max_age]
        events["death"] += len(dead)
        state["tracks"] = tracks = [tr for tr in tracks if not any(tr is d for d in dead)]
        born = dropped = 0
        for j in open_poses:                                           # slot order
            if len(tracks) >= MAX_TRACKS:
                dropped += 1
                continue
            tr = {"id": state["next_id"], "age": 0, "hits": 1, "filter": {}}
            state["next_id"] += 1
            tracks.append(tr)
            born += 1
            ids[f, j], hits[f, j] = tr["id"], 1
            updated.append((tr, j, None))
        events["birth"] += born
        events["drop"] += dropped
        for tr, j, step in updated:
            tr["kpts"], tr["area"], tr["scale"] = np.array(kpts[f, j]), area[f, j], np.array(scale[f])
            tr["kconf"] = None if kconf is None else np.array(kconf[f, j])
            if not smooth:
                continue
            for k in range(K):
                if kconf is not None and not kconf[f, j, k] > vt:
                    tr["filter"].pop(k, None)                          # passes through, loses its state
                    continue
                prev = tr["filter"].get(k) if step is not None else None
                te = None if prev is None else float(step) / rate
                new = []
                for c in range(2):
                    s = float(scale[f, c])
                    x = float(kpts[f, j, k, c]) * s
                    xh, dxh = one_euro_step(x, None if prev is None else prev[c], te, mc, dc, bt)
                    new.append((xh, dxh))
                    out[f, j, k, c] = np.float32(xh / s)
                tr["filter"][k] = new
        counts[f] = (len(matched), born, dropped, len(tracks))
        state["frames"] += 1
    return {"track_id": ids, "track_hits": hits, "track_oks": oks_out, "keypoints": out, "counts": counts,
            "picks": picks, "pair_margin": pair_margin, "events": events, "state": state}


def track_sequences(kpts, scores, area, scale, kconf=None, states=None, **kw):
    """track_frames per sequence of [S, B, ...] arrays, stacked: the output arrays of one kpd_track_poses call."""
    S = scores.shape[0]
    states = [new_state() for _ in range(S)] if states is None else states
    seqs = [track_frames(kpts[s], scores[s], area[s], scale[s], None if kconf is None else kconf[s], states[s], **kw)
            for s in range(S)]
    res = {k: np.stack([q[k] for q in seqs]) for k in ("track_id", "track_hits", "track_oks", "keypoints", "counts")}
    res["picks"] = [p for q in seqs for p in q["picks"]]
    res["pair_margin"] = min([q["pair_margin"] for q in seqs] + [np.inf])
    res["events"] = {k: sum(q["events"][k] for q in seqs) for k in ("match", "birth", "death", "reid", "drop")}
    res["states"] = states
    return res
