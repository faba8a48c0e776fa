"""kpd_pose_nms (csrc/pose_nms.hip) and dll.utils.oks_nms / suppress_poses:
OKS pose-NMS.

CPU part: the ABI, the argument checks (made-up device addresses: every call
here returns before any device work), the numpy restatement
tests/pose_nms_ref.py against values known without it, and the margin and
coverage conditions of the seeded cases.  GPU part: the kernel against
pose_nms_ref, and suppress_poses on a real forward.

Tolerances.  OKS within 1e-12 absolute, for the reason tests/test_oks.py
gives: both sides use double and the same operation order, device and host
exp() may differ by a few ulp, at most ~1e-15 on each term (e * exp(-e) <=
0.37); 1e-12 is three orders above that and three below the 1e-9 margin every
seeded case keeps from its threshold and, in the soft modes, between the best
and the second-best current score of every pick (a product of at most 63 decay
factors, each within a few ulp: ~1e-13 relative), so no decision can flip.
keep, n_keep and suppressed_by are compared exactly; hard-mode scores_out bit
for bit (copies of the inputs); soft-mode scores_out within one fp32 ulp of the
restatement's fp32 cast: the double products differ by ~1e-13 relative, which
can only move the rounding to fp32 at a tie.
"""
import ctypes
import functools
import math
import re

import numpy as np
import pytest
import torch

import pose_nms_ref as R
from conftest import ROOT

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
c_int, c_void_p, c_float = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
f32 = np.float32
INT_OUTPUTS = ("keep", "n_keep", "suppressed_by")


# ------------------------------------------------------------------ ABI
def test_symbol_declared_bound_exported():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    assert re.search(r"\bint\s+kpd_pose_nms\s*\(", hdr)
    assert "kpd_pose_nms" in _native.EXPORTS
    lib = _native.load()
    assert hasattr(lib, "kpd_pose_nms") and lib.kpd_pose_nms.restype is c_int
    assert len(lib.kpd_pose_nms.argtypes) == 20


def test_header_constants_match_native():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+KPD_POSE_NMS_(\w+)\s+(\d+)", hdr)}
    mine = {k[len("POSE_NMS_"):]: v for k, v in vars(_native).items() if k.startswith("POSE_NMS_")}
    assert defs == mine == {"MAX_D": 64, "MAX_K": 32, "HARD": 0, "SOFT": 1, "SOFT_LINEAR": 2}


def test_python_constants():
    from dll.utils import COCO_SIGMAS, POSE_NMS_MODES
    assert POSE_NMS_MODES == {"hard": 0, "soft": 1, "soft_linear": 2} and tuple(POSE_NMS_MODES) == R.MODES
    assert np.array_equal(COCO_SIGMAS, R.COCO_SIGMAS) and len(COCO_SIGMAS) == 17


# ------------------------------------------------------------------ argument checks
def _args(**over):
    a = dict(kpts=c_void_p(0x10000), scores=c_void_p(0x20000), area=c_void_p(0x30000), kconf=c_void_p(0x40000),
             scale=c_void_p(0x50000), sigmas=(c_float * 32)(*([0.05] * 32)), B=2, D=5, K=17, mode=0, threshold=0.9,
             vis_threshold=0.2, min_score=0.0, max_keep=20, oks=c_void_p(0x60000), keep=c_void_p(0x70000),
             n_keep=c_void_p(0x80000), scores_out=c_void_p(0x90000), suppressed_by=c_void_p(0xa0000), stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


NULLABLE = ("kpts", "scores", "area", "scale", "sigmas", "keep", "n_keep", "scores_out", "suppressed_by")


@pytest.mark.parametrize("over, word", [(({name: None}), name) for name in NULLABLE] + [
    (dict(K=0), "K"), (dict(K=33), "K"), (dict(K=-1), "K"),
    (dict(D=65), "D"), (dict(D=-1), "D"),
    (dict(B=-1), "B"),
    (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
    (dict(threshold=0.0), "threshold"), (dict(threshold=-0.5), "threshold"), (dict(threshold=1.5), "threshold"),
    (dict(threshold=float("nan")), "threshold"),
    (dict(vis_threshold=float("nan")), "vis_threshold"), (dict(min_score=float("nan")), "min_score"),
    (dict(max_keep=0), "max_keep"), (dict(max_keep=-5), "max_keep"),
    (dict(oks=None, kconf=None, n_keep=None), "n_keep"),     # a null oks or kconf is not what is complained about
])
def test_argument_checks(over, word):
    from dll import _native
    lib = _native.load()
    assert lib.kpd_pose_nms(*_args(**over)) == -1          # KPD_EINVAL
    msg = lib.kpd_last_error().decode()
    assert msg.startswith("kpd_pose_nms") and re.search(rf"\b{word}\b", msg), msg
    assert "oks is null" not in msg and "kconf is null" not in msg


def test_empty_batch_accepted_without_launch():
    from dll import _native
    lib = _native.load()
    assert lib.kpd_pose_nms(*_args(B=0)) == 0               # KPD_OK, no launch
    assert lib.kpd_pose_nms(*_args(B=0, oks=None, kconf=None)) == 0
    assert lib.kpd_pose_nms(*_args(B=0, threshold=1.0)) == 0
    assert lib.kpd_pose_nms(*_args(B=0, K=33)) == -1        # sizes are checked even then
    assert lib.kpd_pose_nms(*_args(B=0, threshold=0.0)) == -1


def test_cpu_tensor_raises():
    from dll import _native
    from dll.utils import oks_nms, suppress_poses
    z = torch.zeros
    with pytest.raises(_native.KpdNativeError):
        oks_nms(z(1, 2, 17, 2), z(1, 2), z(1, 2), z(1, 2))
    with pytest.raises(_native.KpdNativeError):
        suppress_poses({"keypoints": z(1, 2, 1, 17, 2), "boxes": z(1, 2, 4)}, (640, 480))


# ------------------------------------------------------------------ the restatement against known values
def _poses(D, K=17, seed=0):
    """D well separated poses in pixel units (scale 1): integer coordinates, so differences are exact."""
    rng = np.random.default_rng(seed)
    c = (np.arange(D)[:, None, None] * 1000.0 + rng.integers(100, 400, (D, 1, 2))).astype(np.float64)
    kp = (c + rng.integers(-40, 41, (D, K, 2))).astype(f32)
    return kp, np.full(D, 1e4, f32)


def _img(kp, scores, area, kconf=None, **kw):
    return R.nms_img(np.asarray(kp, f32), np.asarray(scores, f32), np.asarray(area, f32),
                     None if kconf is None else np.asarray(kconf, f32), (1.0, 1.0), **kw)


def test_ref_identical_twin_with_equal_score():
    kp, area = _poses(2)
    kp[1] = kp[0]
    r = _img(kp, [0.7, 0.7], area)
    assert abs(r["oks"][0, 1] - 1.0) <= 1e-14 and r["oks"][0, 1] == r["oks"][1, 0]
    assert r["oks"][0, 0] == 0 and r["oks"][1, 1] == 0
    assert list(r["keep"]) == [0, -1] and r["n_keep"] == 1
    assert list(r["suppressed_by"]) == [-1, 0] and list(r["scores_out"]) == [f32(0.7), 0]


def test_ref_uniform_displacement_formula():
    kp, area = _poses(2, seed=1)
    area[:] = [1e4, 3e4]                                   # den = the mean of the two
    kp[1] = kp[0]
    kp[1, :, 0] += 3.0                                     # (3, 4): 5 px, exact in fp32
    kp[1, :, 1] -= 4.0
    r = _img(kp, [0.5, 0.4], area)
    sig = np.asarray(R.COCO_SIGMAS, f32).astype(np.float64)
    want = sum(math.exp(-25.0 / (2.0 * (2.0 * s) ** 2 * 2e4)) for s in sig) / 17
    assert 0.5 < want < 1.0
    assert abs(r["oks"][0, 1] - want) <= 1e-14 and r["oks"][0, 1] == r["oks"][1, 0]


def test_ref_kconf_counts_only_common_keypoints():
    kp, area = _poses(2, seed=2)
    kp[1] = kp[0]
    kp[1, 5:] += 1000.0                                    # only keypoints 0..4 agree
    conf = np.full((2, 17), 0.9, f32)
    conf[0, 5:] = 0.1                                      # ... and only they are confident in both
    conf[1, 3] = 0.2                                       # not > 0.2: keypoint 3 does not count either
    r = _img(kp, [0.9, 0.8], area, conf)
    assert abs(r["oks"][0, 1] - 1.0) <= 1e-14 and list(r["suppressed_by"]) == [-1, 0]
    assert _img(kp, [0.9, 0.8], area)["oks"][0, 1] < 0.5   # without kconf all 17 count
    conf[0, :5] = 0.1                                      # no common keypoint: OKS 0, nothing suppressed
    r = _img(kp, [0.9, 0.8], area, conf)
    assert r["oks"][0, 1] == 0 and list(r["keep"]) == [0, 1] and (r["suppressed_by"] == -1).all()


def test_ref_gaussian_decay_of_one_pair():
    kp, area = _poses(2, seed=3)
    kp[1] = kp[0] + f32(3.0)
    r = _img(kp, [0.9, 0.8], area, mode="soft", threshold=0.5)
    o, t = r["oks"][0, 1], float(f32(0.5))
    assert 0.5 < o < 1.0 and list(r["keep"]) == [0, 1] and (r["suppressed_by"] == -1).all()
    assert r["scores_out"][0] == f32(0.9)
    assert r["scores_out"][1] == f32(float(f32(0.8)) * math.exp(-(o * o) / t))


def test_ref_linear_decay_on_either_side_of_the_threshold():
    kp, area = _poses(2, seed=4)
    kp[1] = kp[0] + f32(3.0)
    o = _img(kp, [0.9, 0.8], area)["oks"][0, 1]
    assert 0.5 < o < 0.95
    below = _img(kp, [0.9, 0.8], area, mode="soft_linear", threshold=0.95)
    assert list(below["scores_out"]) == [f32(0.9), f32(0.8)]            # unchanged
    above = _img(kp, [0.9, 0.8], area, mode="soft_linear", threshold=0.5)
    assert above["scores_out"][1] == f32(float(f32(0.8)) * (1.0 - o))


def test_ref_soft_decay_reorders_the_picks():
    kp, area = _poses(3, seed=5)
    kp[1] = kp[0]                                          # slot 1: a twin of the best pose, decays by exp(-1/0.5)
    r = _img(kp, [0.9, 0.8, 0.3], area, mode="soft", threshold=0.5)
    assert list(r["keep"]) == [0, 2, 1]
    assert r["scores_out"][1] == f32(float(f32(0.8)) * math.exp(-1.0 / 0.5)) and r["scores_out"][2] == f32(0.3)


def test_ref_max_keep_cuts_the_list():
    kp, area = _poses(4, seed=6)
    scores = [0.2, 0.9, 0.1, 0.5]
    for mode in R.MODES:
        r = _img(kp, scores, area, mode=mode, max_keep=2)
        assert list(r["keep"]) == [1, 3, -1, -1] and r["n_keep"] == 2
        assert list(r["scores_out"]) == [0, f32(0.9), 0, f32(0.5)] and (r["suppressed_by"] == -1).all()
    kp[0] = kp[1]                                          # ranked after the cut: never examined, so not "suppressed"
    r = _img(kp, scores, area, max_keep=2)
    assert list(r["keep"]) == [1, 3, -1, -1] and (r["suppressed_by"] == -1).all()
    assert list(_img(kp, scores, area, max_keep=3)["suppressed_by"]) == [1, -1, -1, -1]


def test_ref_min_score_ends_the_picking():
    kp, area = _poses(4, seed=7)
    scores = [0.2, 0.9, 0.3, 0.5]
    for mode in R.MODES:
        r = _img(kp, scores, area, mode=mode, min_score=0.3)          # 0.3 is not > 0.3
        assert list(r["keep"]) == [1, 3, -1, -1] and list(r["scores_out"]) == [0, f32(0.9), 0, f32(0.5)]
    kp[3] = kp[1]                                          # soft: the twin decays to 0.5 exp(-1/0.9) = 0.165 < 0.25
    r = _img(kp, scores, area, mode="soft", min_score=0.25)
    assert list(r["keep"]) == [1, 2, -1, -1] and list(r["scores_out"]) == [0, f32(0.9), f32(0.3), 0]


def test_ref_absent_and_nan_scores_never_ranked():
    kp, area = _poses(4, seed=8)
    kp[:] = kp[2]                                          # all four identical: only presence separates them
    for mode in R.MODES:
        r = _img(kp, [0.0, np.nan, 0.3, -1.0], area, mode=mode)
        assert list(r["keep"]) == [2, -1, -1, -1] and r["n_keep"] == 1
        assert list(r["scores_out"]) == [0, 0, f32(0.3), 0] and (r["suppressed_by"] == -1).all()
        assert (r["oks"] == 0).all()


def test_ref_score_tie_goes_to_the_lower_slot():
    kp, area = _poses(3, seed=9)
    for mode in R.MODES:
        assert list(_img(kp, [0.5, 0.7, 0.5], area, mode=mode)["keep"]) == [1, 0, 2]


def test_ref_suppressor_is_the_earliest_kept():
    kp, area = _poses(3, seed=10)
    kp[1] = kp[0] + f32(3.0)                               # 0 ~ 1 below the threshold (0.90): both kept
    kp[2] = kp[0] + f32(1.0)                               # 2 is over the threshold with both
    r = _img(kp, [0.8, 0.9, 0.7], area, threshold=0.94)
    o = r["oks"]
    assert o[0, 1] < 0.94 < min(o[0, 2], o[1, 2])
    assert list(r["keep"]) == [1, 0, -1] and list(r["suppressed_by"]) == [-1, -1, 1]


# ------------------------------------------------------------------ seeded cases (shared with the GPU tests)
LEVELS = np.array([0.02, 0.05, 0.1, 0.2])
SETTINGS = (("hard", 0.9), ("hard", 0.5), ("soft", 0.9), ("soft_linear", 0.5))
VIS_THRESHOLD = 0.2


def _seeded(seed, B, D, K, n_present, cluster, sigmas, twins=(), nan_slots=()):
    """Normalised coordinates with a non-unit, unequal scale per image.  The poses come in clusters of
    ``cluster`` slots: the first of a cluster is a random pose in a random box, the others copy it with every
    keypoint moved by a magnitude drawn from LEVELS * sqrt(area), mostly the copy's own level, in a random
    direction, and the box sides varied by +-10 %.  Slots from n_present[b] on are absent (score 0, or NaN for
    ``nan_slots``); twins: (b, i, j) makes slot j an exact copy of slot i with an equal score."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(200, 700, (B, 2)).astype(f32)
    c, wh = rng.uniform(0.3, 0.7, (B, D, 2)), rng.uniform(0.2, 0.5, (B, D, 2))
    kp = c[:, :, None] + rng.uniform(-0.5, 0.5, (B, D, K, 2)) * wh[:, :, None]
    for b in range(B):
        for d in range(D):
            lead = d - d % cluster
            if lead == d:
                continue
            side = math.sqrt(float(wh[b, lead, 0] * wh[b, lead, 1] * scale[b, 0] * scale[b, 1]))
            own = (d // cluster + d + b) % 4
            lev = np.where(rng.uniform(size=K) < 0.8, own, rng.integers(0, 4, K))
            mag, ang = LEVELS[lev] * side, rng.uniform(0, 2 * math.pi, K)
            kp[b, d] = kp[b, lead] + np.stack([mag * np.cos(ang) / scale[b, 0], mag * np.sin(ang) / scale[b, 1]], -1)
            wh[b, d] = wh[b, lead] * rng.uniform(0.9, 1.1, 2)
    scores = rng.uniform(0.05, 1.0, (B, D)).astype(f32)
    kconf = rng.uniform(0.05, 1.0, (B, D, K)).astype(f32)
    kp = kp.astype(f32)
    for b, i, j in twins:
        kp[b, j], wh[b, j], scores[b, j], kconf[b, j] = kp[b, i], wh[b, i], scores[b, i], kconf[b, i]
    for b in range(B):
        scores[b, n_present[b]:] = 0
    for b, d in nan_slots:
        assert d >= n_present[b]
        scores[b, d] = np.nan
    area = (wh[..., 0] * wh[..., 1]).astype(f32) * scale[:, 0:1] * scale[:, 1:2]
    return dict(kpts=kp, scores=scores, area=area.astype(f32), scale=scale, kconf=kconf), np.asarray(sigmas)


SIZES = {
    # ragged counts (6, 3 and 0 present poses), a NaN score, slots 1 and 2 of image 0 tie exactly
    "main": dict(seed=41, B=3, D=6, K=17, n_present=(6, 3, 0), cluster=3, sigmas=R.COCO_SIGMAS, twins=((0, 1, 2),),
                 nan_slots=((1, 4),)),
    # one image at the limits: the whole LDS matrix, every lane of the suppressing wave busy
    "limits": dict(seed=42, B=1, D=64, K=32, n_present=(64,), cluster=4,
                   sigmas=np.random.default_rng(1).uniform(0.025, 0.107, 32)),
    "no_slots": dict(seed=43, B=2, D=0, K=17, n_present=(0, 0), cluster=1, sigmas=R.COCO_SIGMAS),
}
CASES = [(size, mode, thr, with_kconf) for size in SIZES for mode, thr in SETTINGS for with_kconf in (True, False)]
CASE_IDS = [f"{s}-{m}-{t}-{'kconf' if c else 'nokconf'}" for s, m, t, c in CASES]


def _max_keep(size, mode):
    """20, the default, except that hard mode at the limits may keep all 64."""
    return 64 if (size, mode) == ("limits", "hard") else 20


@functools.lru_cache(maxsize=None)
def _inputs(size):
    inputs, sigmas = _seeded(**SIZES[size])
    for a in inputs.values():
        a.setflags(write=False)
    return inputs, sigmas


@functools.lru_cache(maxsize=None)
def _case(size, mode, thr, with_kconf):
    """(inputs, options, the restatement's outputs): computed once, shared, never modified."""
    inputs, sigmas = _inputs(size)
    inputs = dict(inputs, kconf=inputs["kconf"] if with_kconf else None)
    opts = dict(sigmas=sigmas, threshold=thr, mode=mode, vis_threshold=VIS_THRESHOLD, max_keep=_max_keep(size, mode),
                min_score=0.0)
    ref = R.nms_batch(**inputs, **opts)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inputs, opts, ref


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_seeded_cases_keep_their_margins(case):
    _, opts, ref = _case(*case)
    a, gap = R.margins(ref, opts["threshold"], opts["mode"])
    print(case, "threshold margin", a, "pick gap", gap)
    assert a >= 1e-9 and gap >= 1e-9, (a, gap)


def test_seeded_cases_exercise_the_feature():
    second_hand = 0
    for case in CASES:
        size, mode, thr, with_kconf = case
        inputs, opts, ref = _case(*case)
        present = ref["present"]
        kept = ref["scores_out"] > 0
        assert not (kept & ~present).any() and (ref["n_keep"] == kept.sum(1)).all()
        if size == "no_slots":
            assert ref["keep"].shape == (2, 0) and list(ref["n_keep"]) == [0, 0]
            continue
        if mode == "hard":
            assert kept.any() and (ref["suppressed_by"] >= 0).any(), case       # both keeps and suppresses
            assert ((ref["suppressed_by"] >= 0) == (present & ~kept)).all()
            for b in range(len(kept)):
                top = ref["keep"][b, 0]
                second_hand += int(((ref["suppressed_by"][b] >= 0) & (ref["suppressed_by"][b] != top)).sum())
        else:
            assert (ref["suppressed_by"] == -1).all()
            decayed = kept & (ref["scores_out"] != inputs["scores"])
            assert decayed.any() or size == "limits", case      # at the limits the 20 picks may all be undecayed
        if size == "limits" and mode != "hard":
            assert ref["n_keep"][0] == 20 and present.sum() == 64                # stops at max_keep
        if size == "limits" and mode == "hard":
            assert ref["n_keep"][0] > 20
        if size == "main":
            assert list(present.sum(1)) == [6, 3, 0] and ref["n_keep"][2] == 0
            assert np.isnan(inputs["scores"][1, 4]) and not present[1, 4]
            assert ref["oks"][0, 1, 2] == 1.0 and inputs["scores"][0, 1] == inputs["scores"][0, 2]   # the exact twin
            if mode == "hard":               # slot 2 falls to slot 1, or to whatever suppressed slot 1 before it
                sup = ref["suppressed_by"][0]
                assert not kept[0, 2] and sup[2] == (1 if kept[0, 1] else sup[1])
    assert second_hand > 0               # a pose suppressed by a pose other than the top-ranked one
    sc = _inputs("main")[0]["scale"]
    assert (sc != 1).all() and (sc[:, 0] != sc[:, 1]).all()


# ------------------------------------------------------------------ GPU
def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _gpu_nms(inputs, opts, return_oks=True, images=slice(None)):
    from dll.utils import oks_nms
    t = {k: None if v is None else _dev(v[images]) for k, v in inputs.items()}
    out = oks_nms(**t, **opts, return_oks=return_oks)
    torch.cuda.synchronize()
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, mode, with_oks=True, images=slice(None)):
    if with_oks:
        want = ref["oks"][images]
        assert got["oks"].dtype == np.float64 and got["oks"].shape == want.shape
        err = float(np.abs(got["oks"] - want).max()) if want.size else 0.0
        print("max |oks - ref| =", err)
        assert err <= 1e-12, err
        assert np.array_equal(got["oks"], got["oks"].transpose(0, 2, 1))                  # exactly symmetric
        assert (np.diagonal(got["oks"], axis1=1, axis2=2) == 0).all()
    else:
        assert "oks" not in got
    for k in INT_OUTPUTS:
        want = ref[k][images]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert np.array_equal(got[k], want), (k, got[k], want)
    want = ref["scores_out"][images]
    assert got["scores_out"].dtype == f32 and got["scores_out"].shape == want.shape
    if mode == "hard":
        assert np.array_equal(got["scores_out"], want)                                    # copies of the inputs
    else:
        ulps = np.abs(got["scores_out"].astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
        print("max soft score error in fp32 ulp =", float(ulps.max()) if ulps.size else 0.0)
        assert ((got["scores_out"] == 0) == (want == 0)).all() and (ulps <= 1.0).all()


@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_kernel_matches_restatement(case):
    inputs, opts, ref = _case(*case)
    _compare(_gpu_nms(inputs, opts), ref, opts["mode"])


@gpu
@pytest.mark.parametrize("mode, thr", [("hard", 0.9), ("soft", 0.9)])
def test_gpu_null_oks(mode, thr):
    inputs, opts, ref = _case("main", mode, thr, True)
    _compare(_gpu_nms(inputs, opts, return_oks=False), ref, mode, with_oks=False)


@gpu
def test_gpu_non_default_stream():
    from dll.utils import oks_nms
    inputs, opts, ref = _case("main", "soft_linear", 0.5, True)
    t = {k: _dev(v) for k, v in inputs.items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        out = oks_nms(**t, **opts, return_oks=True)
    s.synchronize()
    _compare({k: v.cpu().numpy() for k, v in out.items()}, ref, "soft_linear")


@gpu
@pytest.mark.parametrize("mode, thr", SETTINGS)
def test_gpu_image_alone_gives_the_same_bytes(mode, thr):
    inputs, opts, ref = _case("main", mode, thr, True)
    whole = _gpu_nms(inputs, opts)
    for b in range(3):
        alone = _gpu_nms(inputs, opts, images=slice(b, b + 1))
        for k, v in alone.items():
            assert v.tobytes() == whole[k][b:b + 1].tobytes(), (k, b)


@gpu
@pytest.mark.parametrize("mode", R.MODES)
def test_gpu_max_keep_and_min_score(mode):
    """The walk's two ends on the seeded main inputs: exact decisions on fp32 scores in hard mode; in the soft modes
    the cut score 0.3 is asserted to stay 1e-9 clear of every current score the restatement compares with it."""
    inputs, sigmas = _inputs("main")
    for extra in (dict(max_keep=2, min_score=0.0), dict(max_keep=20, min_score=0.3), dict(max_keep=1, min_score=0.3)):
        opts = dict(sigmas=sigmas, threshold=0.5, mode=mode, vis_threshold=VIS_THRESHOLD, **extra)
        ref = R.nms_batch(**inputs, **opts)
        a, gap = R.margins(ref, 0.5, mode)
        assert a >= 1e-9 and gap >= 1e-9
        assert (ref["n_keep"] <= extra["max_keep"]).all()
        _compare(_gpu_nms(inputs, opts), ref, mode)


def _forward_setup():
    from dll.configs import BackboneConfig, ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_images, synthetic_state_dict
    m = MultiPersonKeypointModel(ModelConfig(backbone=BackboneConfig(in_channels=1, input_size=64)), TrainingConfig())
    m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0))
    m = m.to(DEV).eval()
    x = synthetic_images(2, 1, 64, 64, seed=7).to(DEV)
    b0, b1 = [0.5, 0.5, 0.4, 0.8], [0.3, 0.4, 0.2, 0.3]
    twice = torch.tensor([[b0, b0], [b1, [0.0] * 4]], device=DEV)       # image 0: the same box twice
    once = torch.tensor([[b0], [b1]], device=DEV)
    with torch.no_grad():
        return m({"image": x, "bboxes": twice}), m({"image": x, "bboxes": once})


def _image_of(outputs, i):
    return {k: v[i:i + 1] if isinstance(v, torch.Tensor) else [v[i]] for k, v in outputs.items()}


@gpu
def test_gpu_suppress_poses_on_a_forward():
    from dll.utils import draw_poses, format_pose_labels, pose_scores, suppress_poses
    out2, out1 = _forward_setup()
    before = {k: v.clone() for k, v in out2.items() if isinstance(v, torch.Tensor)}
    keys = set(out2)
    sizes = [(128, 96), (90, 120)]
    got = suppress_poses(out2, sizes, mode="hard", return_oks=True)
    torch.cuda.synchronize()
    # the inputs are untouched
    assert set(out2) == keys and all(torch.equal(out2[k], v) for k, v in before.items())
    assert got is not out2 and got["keypoints"] is out2["keypoints"] and got["heatmap"] is out2["heatmap"]
    kp = out2["keypoints"]
    assert kp.shape[:3] == (2, 2, 1) and torch.equal(kp[0, 0], kp[0, 1])           # bit-identical poses
    sc = pose_scores(out2)
    assert sc[0, 0] == sc[0, 1] and (sc[:, 0] > 0).all() and sc[1, 1] == 0
    assert got["pose_oks"][0, 0, 1] == 1.0 and got["pose_oks"][0, 1, 0] == 1.0
    assert got["pose_keep"].tolist() == [[0, -1], [0, -1]] and got["pose_n_keep"].tolist() == [1, 1]
    assert torch.equal(got["pose_scores"], torch.stack([sc[:, 0], torch.zeros_like(sc[:, 0])], 1))   # slot 0 unchanged
    assert got["box_scores"].tolist() == [[1.0, 0.0], [1.0, 0.0]]
    assert got["boxes"].shape == (2, 2, 4) and torch.equal(got["boxes"][0, 0], got["boxes"][0, 1])
    # one label line for the image with the doubled box, as the single-box forward gives
    text = format_pose_labels(_image_of(got, 0))
    assert text.count("\n") == 1 and format_pose_labels(_image_of(out2, 0)).count("\n") == 2
    assert text == format_pose_labels(_image_of(out1, 0))
    # and the same overlay
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    drawn, want, doubled = draw_poses(images, got), draw_poses(images, out1), draw_poses(images, out2)
    for a, b in zip(drawn, want):
        assert torch.equal(a, b)
    assert (want[0].cpu().numpy() != images[0]).any() and all(a.shape == d.shape for a, d in zip(drawn, doubled))
    # the soft modes keep both poses of the pair, the twin with a decayed score
    soft = suppress_poses(out2, sizes, mode="soft", threshold=0.5)
    assert soft["pose_keep"].tolist() == [[0, 1], [0, -1]]
    want1 = np.float32(float(sc[0, 1]) * math.exp(-1.0 / 0.5))
    assert abs(float(soft["pose_scores"][0, 1]) - want1) <= np.spacing(want1) and soft["pose_scores"][0, 0] == sc[0, 0]
    assert soft["box_scores"].tolist() == [[1.0, 1.0], [1.0, 0.0]]
    with pytest.raises(ValueError):
        suppress_poses({k: v for k, v in out2.items() if k != "boxes"}, sizes)
    with pytest.raises(ValueError):
        suppress_poses(out2, [(128, 96)] * 3)
    one = suppress_poses(out2, (128, 96))                                          # one pair serves every image
    assert one["pose_keep"].tolist() == [[0, -1], [0, -1]]
