"""Inputs and exact expectations for the detector-training kernels at their
value, slot and grid edges: shared by
tests/test_det_train_edges_cpu.py (every precondition: the fp32 and float64
matchings agree, each case reaches what it is named for) and
tests/test_det_train_edges.py (the device).  CPU tensors only; nothing here
runs the model: features, head parameters and labels come from seeded
generators, the anchors from PERSON_HEAD's buffer."""
import functools

import torch

import det_train_ref as R

MAIN = (256, 192)
A, GP = R.A, R.GRID * R.GRID
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
NAN, INF = float("nan"), float("inf")

# person-sized boxes, and one small enough (59 px^2: gmax 0.058) to live on its low-quality set
P = (0.4, 0.45, 0.3, 0.5)
Q = (0.62, 0.55, 0.25, 0.6)
SMALL = (0.41, 0.37, 0.03, 0.04)
ZERO = (0.0, 0.0, 0.0, 0.0)
# the four kinds of absent row
ABSENT = (ZERO, (0.5, 0.5, 0.0, 0.4), (0.5, 0.5, 0.3, -0.1), (0.5, NAN, 0.3, 0.4))
# rows that are present by the rule and overlap no anchor: infinite width, infinite centre, far outside the image
W_INF, CX_INF, FAR = (0.5, 0.5, INF, 0.4), (INF, 0.5, 0.3, 0.4), (5.0, 0.5, 0.3, 0.4)

# the sub-pixel GT of the capped band: a normal person in slot 0, a dot of the given side in slot 1
TINY_PERSON, TINY_AT = (0.42, 0.55, 0.3, 0.5), (0.8131, 0.2077)
TINY_SIDES = (1e-3, 5e-4, 3e-4, 1e-5)
N0 = (20 * 56 + 30) * 9 + 4      # cell (20, 30), the 64 x 64 anchor


@functools.lru_cache(maxsize=None)
def anchors():
    from dll.configs import PersonDetectionConfig
    from dll.models import PERSON_HEAD
    return PERSON_HEAD(PersonDetectionConfig()).anchors.detach().clone()


def abox(n, size=MAIN):
    """Anchor n as a normalised cxcywh box (float64 -> fp32)."""
    return tuple(R.anchor_boxes(anchors(), size[0], size[1], torch.float64)[n].to(torch.float32).tolist())


def image(G, rows):
    """[G,4]: zero rows except rows[slot]."""
    t = torch.zeros(G, 4)
    for slot, box in rows.items():
        t[slot] = torch.tensor(box, dtype=torch.float32)
    return t


def tiny_boxes(side):
    return image(2, {0: TINY_PERSON, 1: TINY_AT + (side, side)})[None]


def _synthetic(B, G, seed):
    from dll.models.synthetic import synthetic_boxes
    return synthetic_boxes(B, G, seed=seed)


THREE = torch.stack([image(3, {0: P, 1: Q, 2: SMALL}), image(3, {0: Q, 2: P})])
BR = (0.985, 0.985, 0.03, 0.03)     # hard against the bottom-right corner
TL = (0.015, 0.015, 0.03, 0.03)     # and the top-left one


def _matching_cases():
    c = {}
    for s in TINY_SIDES:
        c[f"tiny_{s:g}"] = dict(B=1, size=MAIN, gt=tiny_boxes(s), kw={})
    c["thr_equal"] = dict(B=2, size=MAIN, gt=THREE, kw=dict(pos_thr=0.5, neg_thr=0.5))
    c["neg_zero"] = dict(B=2, size=MAIN, gt=torch.stack([THREE[0], image(3, {})]), kw=dict(neg_thr=0.0))
    c["tie_wide"] = dict(B=1, size=MAIN, gt=THREE[:1], kw=dict(tie_eps=0.05))
    # (neg_thr 0.43: at 0.4 the same anchor eight cells along sits on the threshold, (1 - 3/7) / (1 + 3/7), and
    # at 0.45 every 64 x 256 anchor around Q does, 48 x 153.6 / (64 x 256))
    c["pos_09"] = dict(B=1, size=MAIN, gt=image(2, {0: abox(N0), 1: Q})[None], kw=dict(pos_thr=0.9, neg_thr=0.43))
    c["slot63_only"] = dict(B=1, size=MAIN, gt=image(64, {63: P})[None], kw={})
    c["dup_0_63"] = dict(B=1, size=MAIN, gt=image(64, {0: P, 63: P})[None], kw={})
    rows = {s: ABSENT[s % 4] for s in range(62)}
    rows.update({62: P, 63: Q})
    c["slots_62_63"] = dict(B=1, size=MAIN, gt=image(64, rows)[None], kw={})
    c["nonfinite"] = dict(B=2, size=MAIN, kw={}, gt=torch.stack([
        image(5, {0: P, 1: W_INF, 2: CX_INF, 3: FAR, 4: Q}), image(5, {0: W_INF, 1: CX_INF, 3: FAR})]))
    c["corners"] = dict(B=3, size=MAIN, kw={}, gt=torch.stack([
        image(2, {0: BR, 1: P}), image(2, {}), image(2, {0: ABSENT[3], 1: TL})]))
    for (h, w), seed in (((64, 512), 31), ((512, 64), 32), ((34, 34), 33)):
        c[f"size_{h}x{w}"] = dict(B=2, size=(h, w), gt=_synthetic(2, 3, seed), kw={})
    return c


MATCHING = _matching_cases()
# tie_eps = 0: fp32 bits may differ between torch and the device, so the device is held to a sandwich
TIE_ZERO = dict(B=2, size=MAIN, gt=THREE, kw=dict(tie_eps=0.0))


@functools.lru_cache(maxsize=None)
def ref_match(name, dtype=torch.float64):
    c = TIE_ZERO if name == "tie_zero" else MATCHING[name]
    return R.match(anchors(), c["gt"], c["B"], *c["size"], dtype=dtype, **c["kw"])


def default_assign():
    """The labels of most loss cases: THREE matched at the default thresholds (positives, ignored, negatives)."""
    return ref_match("thr_default")["assign"]


def present_iou_zero(m, gt):
    """[B,A] bool: the anchor's float64 IoU with every present GT is 0 (all True for an image without one)."""
    out = torch.ones(gt.shape[0], A, dtype=torch.bool)
    for b, iou in enumerate(m["iou"]):
        pres = R.present(gt[b])
        if bool(pres.any()):
            out[b] = (iou[:, pres] == 0).all(dim=1)
    return out


# ---------------------------------------------------------------- loss
GRADS = ("g_box_w", "g_box_b", "g_cls_w", "g_cls_b")


@functools.lru_cache(maxsize=None)
def features(B, seed=77):
    return torch.randn(B, GP, 128, generator=torch.Generator().manual_seed(seed + B))


def params(seed=5, box_scale=0.05, cls_scale=0.05, bias_scale=0.1):
    """(box_w [36,128], box_b [36], cls_w [9,128], cls_b [9]), fp32."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(36, 128, generator=g) * box_scale, torch.randn(36, generator=g) * bias_scale,
            torch.randn(9, 128, generator=g) * cls_scale, torch.randn(9, generator=g) * bias_scale]


def _case(x, prm, gt, assign, n_pos=None, size=MAIN, **hyper):
    assign = assign.to(torch.int32).contiguous()
    if n_pos is None:
        n_pos = (assign >= 0).sum(dim=1)
    n_pos = torch.as_tensor(n_pos, dtype=torch.int32)
    return dict(x=x, prm=prm, gt=gt, assign=assign, n_pos=n_pos, size=size, hyper=hyper)


def _matched(gt, B, size=MAIN):
    return R.match(anchors(), gt, B, *size)["assign"]


@functools.lru_cache(maxsize=None)
def grid_case(B):
    """Random features, G = 3, assign from the restatement.  B = 4: 224 workgroups, one block each, the reduce
    loop's last chunk of 64 half full; B = 10: 560 blocks, workgroups 0-47 own three."""
    gt = _synthetic(B, 3, 40 + B)
    return _case(features(B), params(), gt, _matched(gt, B))


# planted placement: (image, cell row, cell column); row blocks 264 and 524 are a workgroup's second and third
PLANT_B = 10
PLANT_CELLS = {"b0_i0_j0": (0, 0, 0), "b0_i0_j55": (0, 0, 55), "b0_i55_j55": (0, 55, 55), "b9_i55_j0": (9, 55, 0),
               "block264": (4, 40, 17), "block524": (9, 20, 38)}
PLANT_CHANNELS = (0, 15, 16, 127)
PLANT_X = 2.5
PLANT_LABELS = (0, 1, 2, -1, -2, 0, -1, 1, 2)    # the nine anchors of every planted cell
assert [b * 56 + i for b, i, _ in PLANT_CELLS.values()][-2:] == [264, 524]


@functools.lru_cache(maxsize=None)
def planted_base():
    """Zero weights, random biases (so z and d are the biases), hand-made labels with every planted cell holding
    positives of all three GTs, a negative pair and an ignored anchor.  x is all zero: planted_case() sets one value."""
    g = torch.Generator().manual_seed(91)
    gt = _synthetic(PLANT_B, 3, 92)
    u = torch.rand(PLANT_B, A, generator=g)
    slot = torch.randint(0, 3, (PLANT_B, A), generator=g)
    assign = torch.where(u < 0.03, slot, torch.where(u < 0.06, torch.full_like(slot, -2), torch.full_like(slot, -1)))
    for b, i, j in PLANT_CELLS.values():
        n = (i * 56 + j) * 9
        assign[b, n:n + 9] = torch.tensor(PLANT_LABELS)
    prm = [torch.zeros(36, 128), torch.randn(36, generator=g) * 0.5, torch.zeros(9, 128), torch.randn(9, generator=g)]
    return _case(torch.zeros(PLANT_B, GP, 128), prm, gt, assign)


def planted_case(cell, channel, value=PLANT_X):
    b, i, j = PLANT_CELLS[cell]
    c = dict(planted_base())
    c["x"] = torch.zeros(PLANT_B, GP, 128)
    c["x"][b, i * 56 + j, channel] = value
    return c


SAT_BASE = 0.7                       # class-weight scale: z ~ N(0, 7.9^2) before the factor
SAT_FACTORS = (3.0, 10.0)
SAT_GAMMAS = (0.0, 0.5, 1.0, 2.0, 3.0)
SAT_ALPHAS = (0.0, 0.25, 1.0)


def saturation_case(factor, gamma=2.0, alpha=0.25):
    """|z| passes 88 (expf overflows) at x3 and 104 (fp32 sigmoid underflows to 0) at x10, with both signs
    among positives, negatives and ignored anchors."""
    return _case(features(2), params(cls_scale=SAT_BASE * factor), THREE, default_assign(), gamma=gamma,
                 alpha=alpha)


def logits(case):
    """float64 z [B,A] of a case."""
    return R.heads(case["x"].double(), *[p.double() for p in case["prm"]])[1]


def box_residuals(case):
    """float64 |d - target| of the positives, [n,4]."""
    d, _ = R.heads(case["x"].double(), *[p.double() for p in case["prm"]])
    t = R.box_targets(anchors(), case["gt"], case["assign"], *case["size"], torch.float64)
    return (d - t)[case["assign"] >= 0].abs()


def smooth_l1_case(kind):
    kw = {"quadratic": dict(beta=10.0), "linear": dict(beta=1e-3), "both": dict(beta=1.0 / 9),
          "no_box": dict(box_weight=0.0)}[kind]
    prm = params(box_scale=0.01, bias_scale=0.02) if kind == "both" else params()
    return _case(features(2), prm, THREE, default_assign(), **kw)


def label_case(kind):
    """Hand-made labels on B = 2, G = 3.  -> the case, or for the two out-of-range kinds (case, canonical case)."""
    x, prm = features(2), params()
    base = default_assign().clone()
    n_pos = (base >= 0).sum(dim=1)
    if kind == "all_ignored":
        return _case(x, prm, THREE, torch.full((2, A), -2))
    if kind == "image_all_positive":
        a = base.clone()
        a[0] = 0
        return _case(x, prm, THREE, a)
    idx = torch.arange(A)
    if kind == "too_large":      # G, 1000, INT32_MAX act as -2
        where, values, canon = idx % 7 == 3, (3, 1000, INT32_MAX), -2
    elif kind == "too_small":    # -3, INT32_MIN act as -1
        where, values, canon = idx % 11 == 5, (-3, INT32_MIN), -1
    else:
        raise KeyError(kind)
    odd, plain = base.clone(), base.clone()
    k = int(where.sum())
    odd[:, where] = torch.tensor(values, dtype=torch.int32).repeat(k // len(values) + 1)[:k]
    plain[:, where] = canon
    return _case(x, prm, THREE, odd, n_pos), _case(x, prm, THREE, plain, n_pos)


def extreme_target_case():
    """Positives assigned to a GT of side 1e-6 (log targets near -12) and to one of side 50 (near +6)."""
    g = torch.Generator().manual_seed(93)
    gt = torch.stack([image(3, {0: (0.5, 0.5, 1e-6, 1e-6), 1: (0.5, 0.5, 50.0, 50.0), 2: P})] * 2)
    u = torch.rand(2, A, generator=g)
    slot = torch.randint(0, 3, (2, A), generator=g)
    assign = torch.where(u < 0.05, slot, torch.where(u < 0.08, torch.full_like(slot, -2), torch.full_like(slot, -1)))
    return _case(features(2), params(), gt, assign)


def n_pos_case(n_pos):
    """N comes from n_pos, not from assign: B = 3, assign from the restatement."""
    gt = _synthetic(3, 3, 43)
    return _case(features(3), params(), gt, _matched(gt, 3), n_pos=list(n_pos))


MATCHING["thr_default"] = dict(B=2, size=MAIN, gt=THREE, kw={})   # the loss cases' labels, matched at the defaults
