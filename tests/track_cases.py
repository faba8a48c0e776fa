"""Seeded frame sequences for kpd_track_poses, shared by tests/test_track_cpu.py
(which asserts their margins and coverage on tests/track_ref.py alone) and
tests/test_track.py (which runs the kernel on them).  Every case is built and
restated once and never modified.

A case is a layout: per frame and slot the person shown there, or -1 for an
absent slot.  Persons sit in the cells of a grid over the unit square, far
enough apart that the OKS of two different persons stays orders of magnitude
below the threshold; a person's pose in a frame is its base pose plus a slow
drift plus a jitter of 0.02 sqrt(area) per keypoint in a random direction, its
box sides vary by +-5 %.  Coordinates are normalised, the scale (W, H) is
non-unit and unequal and, where ``wobble`` is set, changes a little from frame
to frame, so the scale a track remembers differs from the current one.
Keypoint confidences are uniform in (0.05, 1): about one in six is not above
the visibility cut 0.2 on either side of a pair.
"""
import functools
import math

import numpy as np

import track_ref as R

f32 = np.float32
VIS_THRESHOLD = 0.2
THRESHOLD = 0.3
FILTER = dict(min_cutoff=1.0, beta=0.05, d_cutoff=1.0, fps=30.0)
_ = -1


def build(seed, layout, K=17, grid=(4, 2), box=(0.12, 0.2), wobble=0.002, nan_slots=(), copies=(), blind=()):
    """Arrays of one sequence.  nan_slots: (frame, slot) absent slots whose score is NaN; copies: (frame, from
    slot, to slot) makes a slot a bit-identical copy; blind: (frame, slot) poses whose confidences are all 0.1."""
    rng = np.random.default_rng(seed)
    layout = np.asarray(layout, int)
    B, D = layout.shape
    n = max(int(layout.max()) + 1, 1)
    cols, rows = grid
    assert n <= cols * rows
    cell = rng.permutation(cols * rows)[:n]
    centre = np.stack([(cell % cols + 0.5) / cols, (cell // cols + 0.5) / rows], -1)
    wh = rng.uniform(box[0], box[1], (n, 2))
    base = centre[:, None] + rng.uniform(-0.5, 0.5, (n, K, 2)) * wh[:, None]
    drift = rng.uniform(-0.002, 0.002, (n, 1, 2)) * wh[:, None]
    scale0 = rng.uniform(200, 700, 2)
    scale = np.stack([scale0 * (1.0 + wobble * rng.uniform(-1, 1, 2)) for _f in range(B)]).astype(f32)
    kp, area = np.zeros((B, D, K, 2)), np.zeros((B, D))
    scores, kconf = np.zeros((B, D), f32), rng.uniform(0.05, 1.0, (B, D, K)).astype(f32)
    for f in range(B):
        for j in range(D):
            p = layout[f, j]
            if p < 0:
                kp[f, j] = rng.uniform(0, 1, (K, 2))         # garbage in an absent slot must not matter
                area[f, j] = rng.uniform(100, 1000)
                continue
            w = wh[p] * rng.uniform(0.95, 1.05, 2)
            side = math.sqrt(float(wh[p, 0] * wh[p, 1]))
            ang = rng.uniform(0, 2 * math.pi, K)
            kp[f, j] = base[p] + drift[p] * f + 0.02 * side * np.stack([np.cos(ang), np.sin(ang)], -1)
            area[f, j] = w[0] * w[1] * float(scale[f, 0]) * float(scale[f, 1])
            scores[f, j] = rng.uniform(0.3, 1.0)
    kp, area = kp.astype(f32), area.astype(f32)
    for f, j in nan_slots:
        assert layout[f, j] < 0
        scores[f, j] = np.nan
    for f, j in blind:
        kconf[f, j] = 0.1
    for f, a, b in copies:
        kp[f, b], area[f, b], kconf[f, b], scores[f, b] = kp[f, a], area[f, a], kconf[f, a], scores[f, a]
    return dict(kpts=kp, scores=scores, area=area, scale=scale, kconf=kconf)


def _swap(B, D=5):
    return [[(f % 2) if j == 0 else (1 - f % 2) if j == 3 % D else _ for j in range(D)] for f in range(B)]


def _exhaust():
    first, second = list(range(64)), list(range(64, 128))
    return [first, second, second, second[::-1]]


# name -> (build arguments, options beyond the shared ones, the person ids the restatement must give per frame and slot
# or None).  In the id tables -1 is an absent or dropped slot.
CASES = {
    # two persons change slots every frame and keep their ids
    "swap": (dict(seed=1, layout=_swap(8)), dict(max_age=2),
             [[0, _, _, 1, _] if f % 2 == 0 else [1, _, _, 0, _] for f in range(8)]),
    # person 1 is away for g = max_age frames and returns with its id ...
    "gap2_age2": (dict(seed=2, layout=[[_, 0, 1, _, _]] * 2 + [[_, 0, _, _, _]] * 2 + [[_, 0, _, _, 1]] * 4), dict(max_age=2),
                  [[_, 0, 1, _, _]] * 2 + [[_, 0, _, _, _]] * 2 + [[_, 0, _, _, 1]] * 4),
    # ... and after g = max_age + 1 frames it gets a new one
    "gap3_age2": (dict(seed=3, layout=[[_, 0, 1, _, _]] * 2 + [[_, 0, _, _, _]] * 3 + [[_, 0, _, _, 1]] * 3), dict(max_age=2),
                  [[_, 0, 1, _, _]] * 2 + [[_, 0, _, _, _]] * 3 + [[_, 0, _, _, 2]] * 3),
    # max_age 0, one slot: g = 0 keeps the id, one frame without any present pose kills the track
    "gap0_age0": (dict(seed=4, layout=[[0]] * 4), dict(max_age=0), [[0]] * 4),
    "gap1_age0": (dict(seed=5, layout=[[0], [_], [0], [0]]), dict(max_age=0), [[0], [_], [1], [1]]),
    # frames without any present pose age the tracks; both return at g = max_age
    "empty_frames": (dict(seed=6, layout=[[0, _, 1, _, _]] + [[_] * 5] * 2 + [[_, 1, _, _, 0]] * 2), dict(max_age=2),
                     [[0, _, 1, _, _]] + [[_] * 5] * 2 + [[_, 1, _, _, 0]] * 2),
    # births in slot order, ids never repeat; a NaN score is an absent slot
    "births": (dict(seed=7, layout=[[_, 0, 1, _, 2], [3, 0, 1, 4, 2], [4, 3, _, 5, _], [6, 5, 7, 3, 4]], nan_slots=((0, 0),)),
               dict(max_age=2), [[_, 0, 1, _, 2], [3, 0, 1, 4, 2], [4, 3, _, 5, _], [6, 5, 7, 3, 4]]),
    # the table fills: 64 births, 64 drops, and once the old tracks have died 64 births and 64 matches
    "exhaust": (dict(seed=8, layout=_exhaust(), grid=(16, 8), box=(0.02, 0.03), wobble=0.0), dict(max_age=1),
                [list(range(64)), [_] * 64, list(range(64, 128)), list(range(64, 128))[::-1]]),
    # person 1 shows no confident keypoint in frame 1: OKS 0 with its own track, a birth; frame 2 finds the old track
    "masks": (dict(seed=9, layout=[[0, _, 1, _, _]] * 4, blind=((1, 2),)), dict(max_age=2),
              [[0, _, 1, _, _], [0, _, 2, _, _], [0, _, 1, _, _], [0, _, 1, _, _]]),
    # frame 1: two bit-identical poses against track 0 -> the lower slot, the other is born as track 1 with the same
    # last pose; frame 2: tracks 0 and 1 against one pose -> the lower id
    "ties": (dict(seed=10, layout=[[_, _, 0, _, _], [_, 0, _, 0, _], [_, _, _, _, 0]], copies=((1, 1, 3),)), dict(max_age=2),
             [[_, _, 0, _, _], [_, 0, _, 1, _], [_, _, _, _, 0]]),
    # edge sizes of K
    "k1": (dict(seed=11, layout=_swap(4), K=1), dict(max_age=2, sigmas=(0.05,)), None),
    "k32": (dict(seed=12, layout=_swap(4), K=32),
            dict(max_age=2, sigmas=tuple(np.random.default_rng(1).uniform(0.025, 0.107, 32))), None),
}
NAMES = tuple(CASES)
STACKED = ("swap", "gap2_age2", "gap3_age2")     # one S = 3 call: equal B, D, K and options


def options(name):
    opts = dict(sigmas=tuple(R.COCO_SIGMAS), threshold=THRESHOLD, vis_threshold=VIS_THRESHOLD, smooth=True, **FILTER)
    opts.update(CASES[name][1])
    return opts


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, options, the restatement's outputs from an empty state): computed once, shared, never modified."""
    inputs = build(**CASES[name][0])
    ref = R.track_frames(**inputs, **options(name))
    for a in list(inputs.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inputs, options(name), ref
