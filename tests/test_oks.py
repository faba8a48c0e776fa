"""kpd_oks_match (csrc/oks.hip) and dll.utils.OksEvaluator: COCO keypoint AP.

CPU part: the ABI, the argument checks (made-up device addresses: every call
here returns before any device work), the numpy restatement tests/oks_ref.py
against values known without it, and the margin condition of the seeded cases.
GPU part: the kernel against oks_ref.

Tolerances.  OKS within 1e-12 absolute: both sides use double and the same
operation order, device and host exp() may differ by a few ulp, at most ~1e-15
on each term (e * exp(-e) <= 0.37); 1e-12 is three orders above that and three
below the 1e-9 margin every seeded case keeps from a threshold and between the
candidates of one detection, so no match can flip.  Every integer output is
compared exactly; AP / AR within 1e-12 (the same decisions, sums of at most a
few thousand terms in a different order).
"""
import ctypes
import functools
import math
import re

import numpy as np
import pytest
import torch

import oks_ref as R
from conftest import ROOT

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
c_int, c_void_p, c_float = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
f32 = np.float32
INPUTS = ("pred_kpts", "pred_scores", "gt_kpts", "gt_vis", "gt_boxes", "gt_area", "n_gt", "scale")
INT_OUTPUTS = ("det_slot", "det_match", "det_ignore", "gt_match", "counts")


# ------------------------------------------------------------------ ABI
def test_symbol_declared_bound_exported():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    assert re.search(r"\bint\s+kpd_oks_match\s*\(", hdr)
    assert "kpd_oks_match" in _native.EXPORTS
    lib = _native.load()
    assert hasattr(lib, "kpd_oks_match") and lib.kpd_oks_match.restype is c_int
    assert len(lib.kpd_oks_match.argtypes) == 24


def test_header_constants_match_native():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+KPD_OKS_(\w+)\s+(\d+)", hdr)}
    mine = {k[4:]: v for k, v in vars(_native).items() if k.startswith("OKS_")}
    assert defs == mine == {"MAX_K": 32, "MAX_T": 16, "MAX_D": 64, "MAX_G": 64}


def test_python_constants():
    from dll.utils import COCO_OKS_THRESHOLDS, COCO_SIGMAS
    from dll.utils import oks
    assert np.array_equal(COCO_SIGMAS, R.COCO_SIGMAS) and len(COCO_SIGMAS) == 17
    assert np.array_equal(COCO_OKS_THRESHOLDS, np.linspace(.5, .95, 10))
    assert np.array_equal(oks.RECALL_GRID, np.linspace(0, 1, 101))


# ------------------------------------------------------------------ argument checks
def _args(**over):
    a = dict(pred_kpts=c_void_p(0x10000), pred_scores=c_void_p(0x20000), gt_kpts=c_void_p(0x30000),
             gt_vis=c_void_p(0x40000), gt_boxes=c_void_p(0x50000), gt_area=c_void_p(0x60000), n_gt=c_void_p(0x70000),
             scale=c_void_p(0x80000), sigmas=(c_float * 32)(*([0.05] * 32)), thresholds=(c_float * 16)(*([0.5] * 16)),
             B=2, D=5, G=4, K=17, T=10, max_dets=20, oks=c_void_p(0x90000), det_score=c_void_p(0xa0000),
             det_slot=c_void_p(0xb0000), det_match=c_void_p(0xc0000), det_ignore=c_void_p(0xd0000),
             gt_match=c_void_p(0xe0000), counts=c_void_p(0xf0000), stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


NULLABLE = ("pred_kpts", "pred_scores", "gt_kpts", "gt_vis", "gt_boxes", "gt_area", "n_gt", "scale", "sigmas",
            "thresholds", "det_score", "det_slot", "det_match", "det_ignore", "gt_match", "counts")


@pytest.mark.parametrize("over, word", [(({name: None}), name) for name in NULLABLE] + [
    (dict(K=0), "K"), (dict(K=33), "K"), (dict(K=-1), "K"),
    (dict(T=0), "T"), (dict(T=17), "T"), (dict(T=-2), "T"),
    (dict(D=65), "D"), (dict(D=-1), "D"),
    (dict(G=65), "G"), (dict(G=-1), "G"),
    (dict(B=-1), "B"),
    (dict(max_dets=0), "max_dets"), (dict(max_dets=-5), "max_dets"),
    (dict(oks=None, counts=None), "counts"),          # a null oks is not what is complained about
])
def test_argument_checks(over, word):
    from dll import _native
    lib = _native.load()
    assert lib.kpd_oks_match(*_args(**over)) == -1          # KPD_EINVAL
    msg = lib.kpd_last_error().decode()
    assert msg.startswith("kpd_oks_match") and re.search(rf"\b{word}\b", msg), msg
    assert "oks is null" not in msg


def test_empty_batch_and_null_oks_accepted():
    from dll import _native
    lib = _native.load()
    assert lib.kpd_oks_match(*_args(B=0)) == 0               # KPD_OK, no launch
    assert lib.kpd_oks_match(*_args(B=0, oks=None)) == 0
    assert lib.kpd_oks_match(*_args(B=0, K=33)) == -1        # sizes are checked even then


def test_cpu_tensor_raises():
    from dll import _native
    from dll.utils import OksEvaluator, oks_match
    z = torch.zeros
    with pytest.raises(_native.KpdNativeError):
        oks_match(z(1, 2, 17, 2), z(1, 2), z(1, 1, 17, 2), z(1, 1, 17), z(1, 1, 4), z(1, 1), z(1), z(1, 2))
    with pytest.raises(_native.KpdNativeError):
        OksEvaluator().update({"keypoints": z(1, 2, 1, 17, 2)}, {})
    assert OksEvaluator().summarize() == {"oks_AP": -1.0, "oks_AP50": -1.0, "oks_AP75": -1.0, "oks_AR": -1.0}


# ------------------------------------------------------------------ the restatement against known values
def _people(G, K=17, seed=0):
    """G labelled persons in pixel units (scale 1), every keypoint labelled: integers, so differences are exact."""
    rng = np.random.default_rng(seed)
    c = rng.integers(100, 400, (G, 1, 2)).astype(np.float64)
    kp = (c + rng.integers(-40, 41, (G, K, 2))).astype(f32)
    boxes = np.concatenate([c[:, 0], np.full((G, 2), 100.0)], -1).astype(f32)
    return kp, np.full((G, K), 2, f32), boxes, np.full(G, 1e4, f32)


def _img(pred, scores, gt, max_dets=20, sigmas=R.COCO_SIGMAS, thresholds=R.COCO_THRESHOLDS, n_gt=None):
    kp, vis, boxes, area = gt
    return R.evaluate_img(np.asarray(pred, f32), np.asarray(scores, f32), kp, vis, boxes, area,
                          len(kp) if n_gt is None else n_gt, (1.0, 1.0), sigmas, thresholds, max_dets)


def test_ref_identical_pose_is_one_and_matches_everywhere():
    gt = _people(1)
    r = _img(gt[0], [0.7], gt)
    assert r["oks"][0, 0] == 1.0
    assert (r["det_match"][:, 0] == 0).all() and (r["gt_match"][:, 0] == 0).all() and not r["det_ignore"].any()
    assert r["det_match"].shape == (10, 1) and tuple(r["counts"]) == (1, 1)


def test_ref_uniform_displacement_formula():
    kp, vis, boxes, area = _people(1, seed=1)
    vis[0, [2, 5, 11]] = 0                                 # unlabelled keypoints do not count
    pred = kp.copy()
    pred[0, :, 0] += 3.0                                   # (3, 4): 5 px, exact in fp32
    pred[0, :, 1] -= 4.0
    pred[0, 5] += 1000.0                                   # and may be anywhere
    r = _img(pred, [0.5], (kp, vis, boxes, area))
    sig = np.asarray(R.COCO_SIGMAS, f32).astype(np.float64)
    lab = [k for k in range(17) if vis[0, k] > 0]
    want = sum(math.exp(-25.0 / (2.0 * (2.0 * sig[k]) ** 2 * 1e4)) for k in lab) / len(lab)
    assert len(lab) == 14 and 0.5 < want < 1.0
    assert abs(r["oks"][0, 0] - want) <= 1e-14


def test_ref_unlabelled_gt_uses_doubled_box_and_is_ignored():
    kp, vis, boxes, area = _people(1, seed=2)
    vis[:] = 0
    cx, cy = boxes[0, :2]
    pred = np.zeros((2, 17, 2), f32)
    pred[0] = [cx + 140.0, cy - 149.0]                     # inside the doubled box [c - 150, c + 150]
    pred[1] = [cx + 150.0 + 30.0, cy]                      # 30 px right of it
    r = _img(pred, [0.9, 0.8], (kp, vis, boxes, area))
    assert r["oks"][0, 0] == 1.0
    sig = np.asarray(R.COCO_SIGMAS, f32).astype(np.float64)
    want = np.mean([math.exp(-900.0 / (2.0 * (2.0 * s) ** 2 * 1e4)) for s in sig])
    assert abs(r["oks"][1, 0] - want) <= 1e-14
    assert tuple(r["counts"]) == (2, 0)
    assert (r["det_match"][:, 0] == 0).all() and (r["det_ignore"][:, 0] == 1).all()
    assert (r["det_match"][:, 1] == -1).all() and (r["det_ignore"][:, 1] == 0).all()     # already matched: skipped


def test_ref_two_dets_one_gt_higher_score_wins():
    gt = _people(1, seed=3)
    near = gt[0] + f32(1.0)
    r = _img(np.concatenate([near, gt[0]]), [0.4, 0.6], gt)          # slot 1 scores higher
    assert list(r["det_slot"]) == [1, 0]
    assert (r["det_match"][:, 0] == 0).all() and (r["det_match"][:, 1] == -1).all()
    assert (r["gt_match"][:, 0] == 1).all() and not r["det_ignore"].any()


def test_ref_identical_gts_later_one_first():
    kp, vis, boxes, area = _people(1, seed=4)
    gt2 = tuple(np.concatenate([a, a]) for a in (kp, vis, boxes, area))
    r = _img(np.concatenate([kp, kp]), [0.9, 0.8], gt2)
    assert r["oks"][0, 0] == r["oks"][0, 1] == 1.0
    assert (r["det_match"][:, 0] == 1).all() and (r["det_match"][:, 1] == 0).all()


def test_ref_counted_gt_beats_better_ignored_gt():
    kp, vis, boxes, area = _people(2, seed=5)
    kp[1], boxes[1] = kp[0], boxes[0]
    vis[1] = 0                                             # gt 1: ignored, OKS 1.0 by its box
    pred = kp[:1] + f32(3.0)                               # against gt 0: below 0.95, above 0.5
    r = _img(pred, [0.9], (kp, vis, boxes, area))
    assert r["oks"][0, 1] == 1.0 and 0.5 < r["oks"][0, 0] < 1.0
    for ti, t in enumerate(R.COCO_THRESHOLDS):
        if r["oks"][0, 0] >= t:
            assert r["det_match"][ti, 0] == 0 and r["det_ignore"][ti, 0] == 0
        else:                                              # no counted gt reaches t: the ignored one is taken
            assert r["det_match"][ti, 0] == 1 and r["det_ignore"][ti, 0] == 1
    assert r["det_match"][0, 0] == 0 and r["det_match"][-1, 0] == 1      # both branches occur


def test_ref_max_dets_cuts_lowest_scores():
    gt = _people(4, seed=6)
    scores = [0.2, 0.9, 0.1, 0.5]
    r = _img(gt[0], scores, gt, max_dets=2)
    assert list(r["det_slot"]) == [1, 3] and list(r["det_score"]) == [f32(0.9), f32(0.5)]
    assert list(r["det_match"][0]) == [1, 3] and list(r["gt_match"][0]) == [-1, 1, -1, 3]
    assert tuple(r["counts"]) == (2, 4)


def test_ref_score_tie_keeps_slot_order():
    gt = _people(3, seed=7)
    r = _img(gt[0], [0.5, 0.7, 0.5], gt)
    assert list(r["det_slot"]) == [1, 0, 2]


def test_ref_absent_slots_never_ranked():
    gt = _people(4, seed=8)
    r = _img(gt[0], [0.0, np.nan, 0.3, -1.0], gt)
    assert list(r["det_slot"]) == [2, -1, -1, -1] and list(r["det_score"]) == [f32(0.3), 0, 0, 0]
    assert tuple(r["counts"]) == (1, 4) and (r["det_match"][:, 1:] == -1).all()
    assert (r["oks"][[0, 1, 3]] == 0).all()


# ------------------------------------------------------------------ AP
def _batch(pred, scores, gt, **kw):
    r = _img(pred, scores, gt, **kw)
    return {k: v[None] for k, v in r.items()}


def test_ap_all_perfect_is_one():
    gt = _people(3, seed=9)
    assert R.average_precision([_batch(gt[0], [0.9, 0.8, 0.7], gt)]) == \
        {"oks_AP": 1.0, "oks_AP50": 1.0, "oks_AP75": 1.0, "oks_AR": 1.0}


def test_ap_false_positive_above_true_positive():
    gt = _people(1, seed=10)
    far = gt[0] + f32(5000.0)
    got = R.average_precision([_batch(np.concatenate([far, gt[0]]), [0.9, 0.6], gt)])
    assert got == {"oks_AP": 0.5, "oks_AP50": 0.5, "oks_AP75": 0.5, "oks_AR": 1.0}


def test_ap_no_counted_gt_is_minus_one():
    kp, vis, boxes, area = _people(1, seed=11)
    vis[:] = 0
    assert set(R.average_precision([_batch(kp, [0.9], (kp, vis, boxes, area))]).values()) == {-1.0}
    assert set(R.average_precision([_batch(kp, [0.9], (kp, vis, boxes, area), n_gt=0)]).values()) == {-1.0}


def test_ap_gts_without_dets_is_zero():
    gt = _people(2, seed=12)
    got = R.average_precision([_batch(gt[0], [0.0, 0.0], gt)])
    assert got == {"oks_AP": 0.0, "oks_AP50": 0.0, "oks_AP75": 0.0, "oks_AR": 0.0}


# ------------------------------------------------------------------ seeded cases (shared with the GPU tests)
LEVELS = np.array([0.02, 0.05, 0.1, 0.2])


def _seeded(seed, B, D, G, K, n_det, n_gt, sigmas, thresholds, max_dets, cluster=1, ignored=(), twins=()):
    """Normalised coordinates with a non-unit, unequal scale per image.  Detection d aims at gt d % n_gt: its
    keypoints are the gt's plus noise of a magnitude drawn per keypoint from LEVELS * sqrt(area), mostly the
    detection's own level, in a random direction.  cluster > 1: groups of gts that are small perturbations of one
    pose, so a detection has several candidates.  ignored: (b, g) gts without a labelled keypoint; twins:
    (b, g, h) makes gt h an exact copy of gt g -- an exact tie."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(200, 700, (B, 2)).astype(f32)
    c, wh = rng.uniform(0.3, 0.7, (B, G, 2)), rng.uniform(0.2, 0.5, (B, G, 2))
    kp = c[:, :, None] + rng.uniform(-0.5, 0.5, (B, G, K, 2)) * wh[:, :, None]
    for g in range(G):
        lead = g - g % cluster
        if lead != g:
            c[:, g], wh[:, g] = c[:, lead], wh[:, lead]
            kp[:, g] = kp[:, lead] + rng.normal(0, 0.02, (B, K, 2)) * wh[:, g, None]
    boxes = np.concatenate([c, wh], -1).astype(f32)
    kp = kp.astype(f32)
    vis = rng.integers(0, 3, (B, G, K)).astype(f32)
    vis[..., 0] = 2
    for b, g in ignored:
        vis[b, g] = 0
    for b, g, h in twins:
        kp[b, h], vis[b, h], boxes[b, h] = kp[b, g], vis[b, g], boxes[b, g]
    area = boxes[..., 2] * boxes[..., 3] * scale[:, 0:1] * scale[:, 1:2]
    pred = rng.uniform(0, 1, (B, D, K, 2))
    scores = rng.uniform(0.05, 1.0, (B, D)).astype(f32)
    for b in range(B):
        for d in range(D):
            if d >= n_det[b]:
                scores[b, d] = 0
            if n_gt[b] == 0:
                continue
            g = d % n_gt[b]
            own = (d // n_gt[b] + d + b) % 4
            lev = np.where(rng.uniform(size=K) < 0.8, own, rng.integers(0, 4, K))
            mag = LEVELS[lev] * math.sqrt(float(area[b, g]))
            ang = rng.uniform(0, 2 * math.pi, K)
            pred[b, d] = kp[b, g] + np.stack([mag * np.cos(ang) / scale[b, 0], mag * np.sin(ang) / scale[b, 1]], -1)
    inputs = dict(pred_kpts=pred.astype(f32), pred_scores=scores, gt_kpts=kp, gt_vis=vis, gt_boxes=boxes,
                  gt_area=area.astype(f32), n_gt=np.asarray(n_gt, np.int32), scale=scale)
    return dict(inputs=inputs, sigmas=np.asarray(sigmas), thresholds=np.asarray(thresholds), max_dets=max_dets)


_MAIN = dict(seed=21, B=3, D=5, G=4, K=17, n_det=(5, 2, 0), n_gt=(4, 1, 3), sigmas=R.COCO_SIGMAS,
             thresholds=R.COCO_THRESHOLDS, ignored=((0, 2), (2, 1)), twins=((0, 1, 3),))
CASES = {
    # ragged counts, ignored gts, det 4 of image 0 shares gt 0 with det 0, gts 1 and 3 of image 0 tie exactly
    "main_top3": lambda: _seeded(max_dets=3, **_MAIN),
    "main_top20": lambda: _seeded(max_dets=20, **_MAIN),
    # one image at the limits: the whole LDS matrix, every wave and every lane busy
    "limits": lambda: _seeded(seed=22, B=1, D=64, G=64, K=32, n_det=(64,), n_gt=(64,),
                              sigmas=np.random.default_rng(1).uniform(0.025, 0.107, 32),
                              thresholds=np.linspace(0.5, 0.95, 16), max_dets=100, cluster=4,
                              ignored=((0, 5), (0, 17), (0, 40), (0, 41)), twins=((0, 8, 9),)),
    "mixed": lambda: _seeded(seed=23, B=4, D=6, G=5, K=17, n_det=(6, 4, 6, 1), n_gt=(5, 5, 2, 3), sigmas=R.COCO_SIGMAS,
                             thresholds=R.COCO_THRESHOLDS, max_dets=20, cluster=2, ignored=((1, 0), (2, 1))),
    "no_det_slots": lambda: _seeded(seed=24, B=2, D=0, G=3, K=17, n_det=(0, 0), n_gt=(3, 2), sigmas=R.COCO_SIGMAS,
                                    thresholds=R.COCO_THRESHOLDS, max_dets=20),
    "no_gt_slots": lambda: _seeded(seed=25, B=2, D=3, G=0, K=17, n_det=(3, 1), n_gt=(0, 0), sigmas=R.COCO_SIGMAS,
                                   thresholds=R.COCO_THRESHOLDS, max_dets=20),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, the restatement's outputs): computed once, shared, never modified."""
    case = CASES[name]()
    ref = R.evaluate_batch(**case["inputs"], sigmas=case["sigmas"], thresholds=case["thresholds"],
                           max_dets=case["max_dets"])
    for a in list(case["inputs"].values()) + list(ref.values()):
        a.setflags(write=False)
    return case, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_seeded_cases_keep_their_margins(name):
    case, ref = _case(name)
    a, gap = R.margins(ref["oks"], case["thresholds"])
    assert a >= 1e-9 and gap >= 1e-9, (a, gap)


def test_seeded_cases_exercise_every_threshold_and_feature():
    for name, T in (("main_top20", 10), ("limits", 16), ("mixed", 10)):
        case, ref = _case(name)
        ranked = ref["det_slot"] >= 0
        for t in range(T):
            m = ref["det_match"][:, t][ranked]
            assert (m >= 0).any() and (m < 0).any(), (name, t)
        assert ref["det_ignore"].any(), name
    case, ref = _case("main_top20")
    o = ref["oks"]
    assert 0.25 < o[o > 0.2].min() < 0.5 and o.max() > 0.95                    # spread over the thresholds
    assert np.array_equal(o[0, :, 1], o[0, :, 3]) and (o[0, :, 1] >= 0.5).any()     # the exact tie
    assert list(ref["counts"][:, 0]) == [5, 2, 0] and list(ref["counts"][:, 1]) == [3, 1, 2]
    assert list(_case("main_top3")[1]["counts"][:, 0]) == [3, 2, 0]
    sc = case["inputs"]["scale"]
    assert (sc != 1).all() and (sc[:, 0] != sc[:, 1]).all()
    # the shared gt: detections 0 and 4 of image 0 both have their best OKS, above 0.5, on gt 0
    cnt = [0, 1, 3]                                                              # its counted gts
    assert o[0, 0, cnt].argmax() == 0 and o[0, 4, cnt].argmax() == 0 and o[0, 0, 0] >= 0.5 and o[0, 4, 0] >= 0.5
    limits = _case("limits")[1]
    assert limits["counts"][0, 0] == 64 and limits["counts"][0, 1] == 60
    assert (limits["det_match"][0] >= 0).sum(1).max() > 32


# ------------------------------------------------------------------ GPU
def _gpu_match(case, return_oks=True):
    from dll.utils import oks_match
    t = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in case["inputs"].items()}
    out = oks_match(**t, sigmas=case["sigmas"], thresholds=case["thresholds"], max_dets=case["max_dets"],
                    return_oks=return_oks)
    torch.cuda.synchronize()
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, with_oks=True):
    if with_oks:
        assert got["oks"].dtype == np.float64 and got["oks"].shape == ref["oks"].shape
        err = float(np.abs(got["oks"] - ref["oks"]).max()) if ref["oks"].size else 0.0
        print("max |oks - ref| =", err)
        assert err <= 1e-12, err
    else:
        assert "oks" not in got
    assert np.array_equal(got["det_score"], ref["det_score"])          # copies of the input scores
    for k in INT_OUTPUTS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_kernel_matches_restatement(name):
    case, ref = _case(name)
    _compare(_gpu_match(case), ref)


@gpu
def test_gpu_null_oks():
    case, ref = _case("main_top20")
    _compare(_gpu_match(case, return_oks=False), ref, with_oks=False)


@gpu
def test_gpu_non_default_stream():
    from dll.utils import oks_match
    case, ref = _case("mixed")
    t = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in case["inputs"].items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        out = oks_match(**t, sigmas=case["sigmas"], thresholds=case["thresholds"], max_dets=case["max_dets"],
                        return_oks=True)
    s.synchronize()
    _compare({k: v.cpu().numpy() for k, v in out.items()}, ref)


def _forward_like(rng, case, P_heat=6, detector=True):
    """A forward's output dict and a collated batch around a seeded case's arrays."""
    i = case["inputs"]
    B, D, K = i["pred_kpts"].shape[:3]
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)     # noqa: E731
    out = {"keypoints": dev(i["pred_kpts"])[:, :, None], "heatmap": dev(rng.uniform(0.05, 1, (B, D, K, P_heat, 5)).astype(f32))}
    boxes = rng.uniform(0.2, 0.6, (B, D, 4)).astype(f32)
    if detector:
        out["box_scores"] = dev(i["pred_scores"])
    else:                                                      # caller boxes: absent slots are all-zero rows at the end
        boxes[i["pred_scores"] == 0] = 0
    out["boxes"] = [dev(b) for b in boxes]
    batch = {"keypoints": dev(i["gt_kpts"]), "visibilities": dev(i["gt_vis"]), "bboxes": [dev(i["gt_boxes"])],
             "num_persons": dev(i["n_gt"]).long(), "orig_size": [(int(w), int(h)) for w, h in i["scale"]]}
    return out, batch


@gpu
def test_gpu_evaluator_two_batches_against_restatement():
    from dll.utils import OksEvaluator, pose_scores
    rng = np.random.default_rng(31)
    ev = OksEvaluator(max_dets=4, area_factor=0.53)
    assert ev.summarize() == {k: -1.0 for k in ("oks_AP", "oks_AP50", "oks_AP75", "oks_AR")}
    want_batches = []
    for name, detector in (("main_top20", True), ("mixed", False)):         # B = 3, P = 5 and B = 4, P = 6
        out, batch = _forward_like(rng, _case(name)[0], detector=detector)
        assert ev.update(out, batch) is None
        host = {k: v.cpu().numpy() for k, v in ev.inputs(out, batch).items()}
        sc = pose_scores(out).cpu().numpy()
        assert np.array_equal(host["pred_scores"], sc) and np.array_equal(sc > 0, _case(name)[0]["inputs"]["pred_scores"] > 0)
        assert (sc < 1).all()                                               # rescored by the heatmap peaks
        w, h = np.array(batch["orig_size"], f32).T
        gb = host["gt_boxes"]
        assert np.array_equal(host["scale"], np.stack([w, h], 1))
        assert np.allclose(host["gt_area"], gb[..., 2] * gb[..., 3] * (w * h)[:, None] * 0.53, rtol=1e-6, atol=0)
        want_batches.append(R.evaluate_batch(**host, sigmas=ev.sigmas, thresholds=ev.thresholds, max_dets=4))
        a, gap = R.margins(want_batches[-1]["oks"], ev.thresholds)
        assert a >= 1e-9 and gap >= 1e-9
    # update only queued work: it returned nothing and holds device tensors alone
    assert len(ev.results) == 2 and all(isinstance(v, torch.Tensor) and v.is_cuda for r in ev.results for v in r.values())
    got, want = ev.summarize(), R.average_precision(want_batches, ev.thresholds)
    print(got, want)
    assert set(got) == set(want) == {"oks_AP", "oks_AP50", "oks_AP75", "oks_AR"}
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    assert 0.0 < want["oks_AP"] < want["oks_AP50"] <= 1.0 and 0.0 < want["oks_AR"] < 1.0
    ev.reset()
    assert ev.results == [] and ev.summarize()["oks_AP"] == -1.0


@gpu
def test_gpu_evaluator_edge_values():
    """Labels fed back as predictions: 1.0 exactly; counted gts without detections: 0; no counted gt: -1."""
    from dll.utils import OksEvaluator
    case = _case("mixed")[0]
    i = case["inputs"]
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)     # noqa: E731
    batch = {"keypoints": dev(i["gt_kpts"]), "visibilities": dev(i["gt_vis"]), "bboxes": dev(i["gt_boxes"]),
             "num_persons": dev(i["n_gt"]).long(), "orig_size": [(640, 480)] * 4}
    G = i["gt_kpts"].shape[1]
    present = (torch.arange(G, device=DEV)[None] < dev(i["n_gt"])[:, None]).float()
    ev = OksEvaluator()
    ev.update({"keypoints": dev(i["gt_kpts"])[:, :, None]}, batch, scores=present)
    assert ev.summarize() == {"oks_AP": 1.0, "oks_AP50": 1.0, "oks_AP75": 1.0, "oks_AR": 1.0}
    ev.reset()
    ev.update({"keypoints": dev(i["gt_kpts"])[:, :, None]}, batch, scores=torch.zeros_like(present))
    assert ev.summarize() == {"oks_AP": 0.0, "oks_AP50": 0.0, "oks_AP75": 0.0, "oks_AR": 0.0}
    ev.reset()
    ev.update({"keypoints": dev(i["gt_kpts"])[:, :, None]}, dict(batch, visibilities=torch.zeros_like(batch["visibilities"])),
              scores=present)
    assert set(ev.summarize().values()) == {-1.0}
