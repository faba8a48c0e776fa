"""Inputs for tests/golden/ops_edges.npz (shared by make_ops_edges_golden.py
and the tests): everything is regenerated from seeds, the fixture stores the
reference's outputs only.

* target_cases():  generate_target_heatmap / _adaptive at sigmas fp32 cannot
  represent, at sub-unit sigma, on maps smaller than the Gaussian, and at
  every W % 4 (the float4 and the scalar store path of target_heatmap_kernel);
* decode_jobs():   the edge planes of the decoders (sizes around the
  256-thread stride, ties across the reduction, NaN, sub-pixel windows,
  soft-argmax temperatures) with the decoder and parameter to run on each;
* metric_cases():  validation metrics at n around the workgroup's stride.
"""
import math

import numpy as np
import torch

ARGMAX, SUBPIXEL, SOFTARGMAX, MODEL = 0, 1, 2, 3
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ targets
def _below_one():
    return float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def target_cases():
    """(name, keypoints [B,K,2], (H, W), sigma or base_sigma, adaptive)."""
    g = torch.Generator().manual_seed(31)
    wide = lambda *s: torch.rand(*s, 2, generator=g) * 1.2 - 0.1     # noqa: E731  some outside [0, 1)
    cases = [
        ("s2p4", wide(2, 6), (30, 41), 2.4, False),                  # 2.4 is no fp32 value; 13 x 13
        ("adaptive56", wide(1, 6), (56, 56), 3.0, True),             # sigma 3.0
        ("adaptive48", wide(1, 6), (64, 48), 3.0, True),             # 3 * 48 / 56 = 2.5714...
        ("adaptive30", wide(2, 5), (30, 41), 3.0, True),             # 3 * 0.8 = 2.4000000000000004
        ("s0p8", wide(2, 6), (9, 10), 0.8, False),                   # kernel size 1: a single 1.0
        ("s3_8x8", wide(2, 6), (8, 8), 3.0, False),                  # 19 x 19 Gaussian on an 8 x 8 map
        ("s2p9999999", wide(1, 6), (20, 24), 2.9999999, False),      # rounds to 3.0f: 13 x 13, not 19 x 19
        ("s1p016", wide(1, 6), (12, 16), 1.016, False),
    ]
    for W in (1, 2, 3, 5, 8, 41):                                    # W % 4 = 1, 2, 3, 1, 0, 1
        kp = torch.rand(1, 8, 2, generator=g)
        kp[0, 0] = torch.tensor([_below_one(), 0.5])                 # x*W just below W in fp32: last column
        kp[0, 1] = torch.tensor([1.0, 0.5])                          # x*W == W: outside
        kp[0, 2] = torch.tensor([0.5, _below_one()])
        kp[0, 3] = torch.tensor([0.5, 1.0])
        kp[0, 4] = torch.tensor([0.0, 0.0])
        kp[0, 5] = torch.tensor([-1e-9, 0.3])                        # just below 0: outside
        cases.append((f"w{W}", kp, (7, W), 1.3, False))
    return cases


def target_nan_case():
    """A NaN keypoint: the reference raises on int(NaN), so no fixture entry;
    the project's contract is a zero plane."""
    kp = torch.tensor([[[0.5, 0.5], [NAN, 0.5], [0.5, NAN], [NAN, NAN], [0.25, 0.75]]])
    return kp, (9, 10), 1.3


# ----------------------------------------------------------------- decoders
SIZES = [(2, 2), (2, 3), (3, 2), (5, 51), (16, 16), (3, 86), (2, 300), (300, 2), (96, 72), (128, 128)]
TEMPS = [0.01, 0.5, 1.0, 100.0, -1.0]
WINDOWS = [3, 5, 7, 0, 2, 4, -1, -3]


def _size_planes(H, W, g):
    n = H * W
    last = torch.zeros(n)
    last[n - 1] = 0.7                                                # the maximum at the last index
    planes = [torch.rand(n, generator=g), torch.randn(n, generator=g), torch.rand(n, generator=g) ** 8, last,
              torch.full((n,), 0.25), torch.full((n,), -INF)]        # all-equal; all -inf
    return torch.stack(planes).view(1, len(planes), H, W)


def _tie_planes(H, W, i, g):
    """Equal maxima at every non-empty subset of size >= 2 of the flat indices
    {i, i+1, i+256, i+257} that fit: neighbours in one wave, the same thread's
    next element, and pairs whose lower index sits in the higher thread."""
    n = H * W
    idx = [j for j in (i, i + 1, i + 256, i + 257) if j < n]
    planes = []
    for mask in range(1, 1 << len(idx)):
        sel = [idx[b] for b in range(len(idx)) if mask >> b & 1]
        if len(sel) < 2:
            continue
        p = torch.rand(n, generator=g) * 0.5
        for j in reversed(sel):                                      # placed from the highest index down
            p[j] = 0.9
        planes.append(p)
    return torch.stack(planes).view(1, len(planes), H, W)


def _nan_planes(H, W, g):
    n = H * W
    base = lambda: torch.rand(n, generator=g) * 0.5                  # noqa: E731
    a, b = n // 7, (5 * n) // 7
    one = base(); one[a] = NAN                                       # one NaN
    after = base(); after[a] = 0.9; after[b] = NAN                   # a NaN after the maximum
    before = base(); before[a] = NAN; before[b] = 0.9                # a NaN before it
    two = base(); two[a + 1] = NAN; two[min(a + 256, n - 1)] = NAN   # two NaNs: the first wins
    inf_nan = base(); inf_nan[a] = INF; inf_nan[b] = NAN             # NaN beats +inf
    planes = [one, after, before, two, inf_nan, torch.full((n,), NAN)]
    return torch.stack(planes).view(1, len(planes), H, W)


def _subpixel_planes(g):
    """9 x 11: the maximum in each corner, on each edge and inside; then planes
    whose window mass is not positive, and a mixed-sign window with positive mass."""
    H, W = 9, 11
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 5), (H - 1, 5), (4, 0), (4, W - 1), (4, 5), (1, 1),
             (H - 2, W - 2)]
    planes = []
    for y, x in spots:
        p = torch.rand(H, W, generator=g) * 0.3
        p[y, x] = 1.0
        planes.append(p)
    planes.append(-torch.rand(H, W, generator=g) - 0.1)              # all negative: mass < 0
    planes.append(torch.zeros(H, W))                                 # mass 0
    mixed = torch.randn(H, W, generator=g) * 0.05
    mixed[4, 5] = 1.0
    mixed[4, 4] = mixed[3, 5] = -0.2                                  # negative neighbours, mass stays > 0.5
    planes.append(mixed)
    neg_mass = torch.full((H, W), -0.5)
    neg_mass[2, 3] = 1.0                                             # positive maximum, window mass negative
    planes.append(neg_mass)
    return torch.stack(planes).view(1, len(planes), H, W)


def decode_jobs():
    """(key, heat [1,K,H,W], mode, param) -- one decoder call each.  Keys name
    the fixture entries of the three reference decoders; MODEL jobs (no
    fixture: the model's decode_heatmap is compared with decode_ref only) carry
    a key too so failures name their case."""
    g = torch.Generator().manual_seed(77)
    jobs = []

    def add(name, heat, temps=(1.0,), windows=(3,)):
        jobs.append((f"{name}_argmax", heat, ARGMAX, 0.0))
        for w in windows:
            jobs.append((f"{name}_sub{w}", heat, SUBPIXEL, float(w)))
        for t in temps:
            jobs.append((f"{name}_sa{t}", heat, SOFTARGMAX, t))
        jobs.append((f"{name}_model", heat, MODEL, 0.0))
    for H, W in SIZES:
        add(f"size{H}x{W}", _size_planes(H, W, g), temps=TEMPS)
    add("tie16x16", _tie_planes(16, 16, 100, g))                     # 256: only i, i+1 fit
    add("tie3x86", _tie_planes(3, 86, 0, g))                         # 258: 0, 1, 256, 257
    add("tie96x72_3", _tie_planes(96, 72, 3, g))
    add("tie96x72_255", _tie_planes(96, 72, 255, g))                 # i+1 wraps to thread 0
    add("tie96x72_end", _tie_planes(96, 72, 96 * 72 - 258, g))       # ... up to the last index
    add("nan2x3", _nan_planes(2, 3, g))
    add("nan3x86", _nan_planes(3, 86, g))
    add("nan96x72", _nan_planes(96, 72, g))
    sub = _subpixel_planes(g)
    add("subpix9x11", sub, windows=[w for w in WINDOWS if w >= 0])
    # negative windows: pad = w // 2 < 0 makes the window empty -> zeros.  With
    # the maximum at (0, 0) and w = -3 the reference's slice end turns negative,
    # its window is not empty and its torch.arange raises: those two planes
    # (the top-left peak and the zero plane) have no reference value and stay out.
    keep = [k for k in range(sub.shape[1]) if int(sub[0, k].argmax()) != 0]
    add("subpixneg9x11", sub[:, keep], windows=[w for w in WINDOWS if w < 0])
    small = torch.rand(1, 3, 4, 4, generator=g)
    add("subpix4x4", small, windows=(9, 3))                          # a window larger than the plane
    logits = torch.rand(1, 4, 16, 16, generator=g) * 160 - 80        # +-80 logits at T = 1
    logits[0, 3] = -80.0
    logits[0, 3, 5, 9] = 80.0
    add("logits80", logits)
    return jobs


# ------------------------------------------------------------------ metrics
DEFAULT_THRESHOLDS = [0.002, 0.05, 0.2]
EXACT_THRESHOLDS = [0.25, 0.3125, 0.5]
SIXTEEN = [round(0.01 * (i + 1), 2) for i in range(16)]


def metric_cases():
    """(name, pred [1,n,2], gt [1,n,2], vis [1,n], thresholds)."""
    g = torch.Generator().manual_seed(41)
    cases = []
    for n in (1, 255, 256, 257, 5000):
        gt = torch.rand(1, n, 2, generator=g)
        pred = gt + torch.randn(1, n, 2, generator=g) * 0.05
        vis = torch.tensor([2.0, 0.5, -1.0, 0.0, 1.0])[torch.randint(0, 5, (1, n), generator=g)]
        if n == 1:
            vis[:] = 0.5
        cases.append((f"n{n}", pred, gt, vis, DEFAULT_THRESHOLDS))
    # distances exactly on a threshold (<=): dyadic offsets, 3-4-5 triangles
    gt = torch.tensor([[[0.5, 0.5]] * 8])
    d = torch.tensor([[[0.25, 0.0], [0.0, -0.25], [0.1875, 0.25], [-0.25, 0.1875], [0.5, 0.0], [0.375, 0.5],
                       [0.2500001, 0.0], [0.0, 0.0]]])
    vis = torch.tensor([[2.0, 0.5, 1.0, 2.0, 2.0, 2.0, 2.0, -1.0]])
    cases.append(("exact", gt + d, gt, vis, EXACT_THRESHOLDS))
    n = 300
    gt = torch.rand(1, n, 2, generator=g)
    pred = gt + torch.randn(1, n, 2, generator=g) * 0.08
    cases.append(("sixteen", pred, gt, torch.ones(1, n), SIXTEEN))
    cases.append(("hidden", pred, gt, -torch.ones(1, n), DEFAULT_THRESHOLDS))       # nothing visible
    return cases


assert all(math.isfinite(t) for t in TEMPS)
