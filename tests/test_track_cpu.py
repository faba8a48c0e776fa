"""kpd_track_poses (csrc/track.hip), dll.utils.PoseTracker and predict.py
--track: everything that needs no GPU.

The ABI, the argument checks (made-up device addresses: every call here
returns before any device work), the numpy restatement tests/track_ref.py
against values known without it, and the margin and coverage conditions of the
seeded cases of tests/track_cases.py that tests/test_track.py runs on the GPU:
every greedy pick keeps 1e-9 from the threshold and from the best other
candidate unless that one is bit-equal (the designed ties, decided by id and
slot), and every examined pair keeps 1e-9 from the threshold, so the 1e-12 the
device's exp() may differ by cannot flip a decision.
"""
import argparse
import ctypes
import math
import re
import sys

import numpy as np
import pytest
import torch

import track_cases as C
import track_ref as R
from conftest import PKG, ROOT

c_int, c_void_p, c_float = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
f32 = np.float32


# ------------------------------------------------------------------ ABI
def test_symbols_declared_bound_exported():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    assert re.search(r"\bint\s+kpd_track_poses\s*\(", hdr) and re.search(r"\bsize_t\s+kpd_track_state_bytes\s*\(", hdr)
    assert "kpd_track_poses" in _native.EXPORTS and "kpd_track_state_bytes" in _native.EXPORTS
    lib = _native.load()
    assert lib.kpd_track_poses.restype is c_int and len(lib.kpd_track_poses.argtypes) == 25
    assert lib.kpd_track_state_bytes.restype is ctypes.c_size_t


def test_header_constants_match_native():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+KPD_TRACK_(\w+)\s+(\d+)", hdr)}
    mine = {k[len("TRACK_"):]: v for k, v in vars(_native).items() if k.startswith("TRACK_")}
    assert defs == mine == {"MAX_T": 64, "MAX_D": 64, "MAX_K": 32}
    assert R.MAX_TRACKS == 64


def test_state_bytes():
    from dll import _native
    lib = _native.load()
    n17 = lib.kpd_track_state_bytes(17)
    assert n17 > 0 and n17 % 8 == 0
    assert lib.kpd_track_state_bytes(0) == 0 and lib.kpd_track_state_bytes(33) == 0 and lib.kpd_track_state_bytes(-1) == 0
    sizes = [lib.kpd_track_state_bytes(k) for k in range(1, 33)]
    assert all(b > a and b % 8 == 0 for a, b in zip(sizes, sizes[1:]))
    # at least the last raw pose, its confidences and two doubles per coordinate for each of the 64 tracks
    assert n17 >= 64 * 17 * (2 * 4 + 4 + 4 * 8)


# ------------------------------------------------------------------ argument checks
def _args(**over):
    a = dict(kpts=c_void_p(0x10000), scores=c_void_p(0x20000), area=c_void_p(0x30000), kconf=c_void_p(0x40000),
             scale=c_void_p(0x50000), sigmas=(c_float * 32)(*([0.05] * 32)), S=2, B=3, D=5, K=17, threshold=0.3,
             vis_threshold=0.2, max_age=10, smooth=1, min_cutoff=1.0, beta=0.05, d_cutoff=1.0, fps=30.0,
             state=c_void_p(0x60000), track_id=c_void_p(0x70000), track_hits=c_void_p(0x80000),
             track_oks=c_void_p(0x90000), kpts_out=c_void_p(0xa0000), counts=c_void_p(0xb0000), stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


REQUIRED = ("kpts", "scores", "area", "scale", "sigmas", "state", "track_id", "track_hits", "kpts_out", "counts")
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("over, word", [(({name: None}), name) for name in REQUIRED] + [
    (dict(S=-1), "S"), (dict(B=-1), "B"),
    (dict(D=65), "D"), (dict(D=-1), "D"),
    (dict(K=0), "K"), (dict(K=33), "K"), (dict(K=-1), "K"),
    (dict(threshold=1.0), "threshold"), (dict(threshold=-0.1), "threshold"), (dict(threshold=1.5), "threshold"),
    (dict(threshold=NAN), "threshold"), (dict(vis_threshold=NAN), "vis_threshold"),
    (dict(max_age=-1), "max_age"),
    (dict(min_cutoff=0.0), "min_cutoff"), (dict(min_cutoff=-1.0), "min_cutoff"), (dict(min_cutoff=NAN), "min_cutoff"),
    (dict(min_cutoff=INF), "min_cutoff"),
    (dict(d_cutoff=0.0), "d_cutoff"), (dict(d_cutoff=NAN), "d_cutoff"), (dict(d_cutoff=INF), "d_cutoff"),
    (dict(beta=-0.1), "beta"), (dict(beta=NAN), "beta"), (dict(beta=INF), "beta"),
    (dict(fps=0.0), "fps"), (dict(fps=-30.0), "fps"), (dict(fps=NAN), "fps"), (dict(fps=INF), "fps"),
    (dict(track_oks=None, kconf=None, counts=None), "counts"),   # a null track_oks or kconf is not what is complained about
])
def test_argument_checks(over, word):
    from dll import _native
    lib = _native.load()
    assert lib.kpd_track_poses(*_args(**over)) == -1          # KPD_EINVAL
    msg = lib.kpd_last_error().decode()
    assert msg.startswith("kpd_track_poses") and re.search(rf"\b{word}\b", msg), msg
    assert "track_oks is null" not in msg and "kconf is null" not in msg


def test_range_edges_accepted():
    """The accepted side of every range edge, on an empty call (no launch)."""
    from dll import _native
    lib = _native.load()
    for over in (dict(threshold=0.0), dict(threshold=float(np.nextafter(f32(1), f32(0)))), dict(max_age=0), dict(beta=0.0),
                 dict(D=0), dict(D=64), dict(K=1), dict(K=32)):
        assert lib.kpd_track_poses(*_args(S=0, **over)) == 0, over


def test_empty_call_accepted_without_launch():
    from dll import _native
    lib = _native.load()
    for empty in (dict(S=0), dict(B=0), dict(S=0, B=0)):
        assert lib.kpd_track_poses(*_args(**empty)) == 0               # KPD_OK, no launch
        assert lib.kpd_track_poses(*_args(**empty, track_oks=None, kconf=None)) == 0
        assert lib.kpd_track_poses(*_args(**empty, K=33)) == -1        # sizes are checked even then
        assert lib.kpd_track_poses(*_args(**empty, D=65)) == -1
        assert lib.kpd_track_poses(*_args(**empty, threshold=1.0)) == -1
        assert lib.kpd_track_poses(*_args(**empty, fps=0.0)) == -1


def test_smoothing_off_needs_neither_kpts_out_nor_filter_constants():
    from dll import _native
    lib = _native.load()
    # S = 0: the checks that come before the early return; nothing is launched on the made-up addresses
    assert lib.kpd_track_poses(*_args(S=0, smooth=0, kpts_out=None)) == 0
    assert lib.kpd_track_poses(*_args(S=0, smooth=0, kpts_out=None, fps=0.0, min_cutoff=NAN)) == 0
    # with work to do a null kpts_out is complained about only when smoothing is on: smooth = 0 gets past every
    # pointer check, so the first complaint is about the one pointer that is null besides it
    assert lib.kpd_track_poses(*_args(smooth=0, kpts_out=None, counts=None)) == -1
    assert "counts is null" in lib.kpd_last_error().decode()
    assert lib.kpd_track_poses(*_args(smooth=1, kpts_out=None, counts=None)) == -1
    assert "kpts_out is null" in lib.kpd_last_error().decode()


def test_cpu_tensor_raises():
    from dll import _native
    from dll.utils import PoseTracker
    z = torch.zeros
    with pytest.raises(_native.KpdNativeError):
        PoseTracker(device="cpu")
    tr = PoseTracker(device="cuda")                                    # the state is allocated at first use
    with pytest.raises(_native.KpdNativeError):
        tr.update(z(2, 3, 17, 2), z(2, 3), z(2, 3), z(2, 2))
    with pytest.raises(_native.KpdNativeError):
        tr.track({"keypoints": z(1, 2, 1, 17, 2), "boxes": z(1, 2, 4)}, (640, 480))
    with pytest.raises(ValueError):
        PoseTracker(num_keypoints=33, device="cuda")
    with pytest.raises(ValueError):
        PoseTracker(num_keypoints=5, device="cuda")                    # 17 sigmas for 5 keypoints


# ------------------------------------------------------------------ the restatement against known values
SIG2 = (0.05, 0.1)


def _frames(poses, area=1e4, conf=None):
    """Hand-built frames, K = 2, scale 1, pixel units: poses[f][j] = [[x0, y0], [x1, y1]] or None."""
    B, D = len(poses), len(poses[0])
    kp, sc = np.zeros((B, D, 2, 2), f32), np.zeros((B, D), f32)
    for f in range(B):
        for j in range(D):
            if poses[f][j] is not None:
                kp[f, j], sc[f, j] = poses[f][j], 0.9
    return dict(kpts=kp, scores=sc, area=np.full((B, D), area, f32), scale=np.ones((B, 2), f32),
                kconf=None if conf is None else np.asarray(conf, f32))


A = [[100.0, 200.0], [140.0, 260.0]]
FAR = [[5100.0, 5200.0], [5140.0, 5260.0]]


def test_ref_identical_pose_twice():
    r = R.track_frames(**_frames([[A], [A]]), sigmas=SIG2)
    assert r["track_oks"][1, 0] == 1.0 and r["track_oks"][0, 0] == 0.0
    assert list(r["track_id"][:, 0]) == [0, 0] and list(r["track_hits"][:, 0]) == [1, 2]
    assert r["counts"].tolist() == [[0, 1, 0, 1], [1, 0, 0, 1]]
    assert r["picks"] == [(1.0 - float(f32(0.3)), np.inf)]


def test_ref_far_pose_is_born_with_the_next_id():
    r = R.track_frames(**_frames([[A, None], [A, FAR], [FAR, A]]), sigmas=SIG2)
    assert r["track_id"].tolist() == [[0, -1], [0, 1], [1, 0]] and r["track_hits"].tolist() == [[1, 0], [2, 1], [2, 3]]
    assert r["counts"].tolist() == [[0, 1, 0, 1], [1, 1, 0, 2], [2, 0, 0, 2]]
    assert r["track_oks"][1, 1] == 0.0 and r["track_oks"][2, 0] == 1.0


def test_ref_displacement_formula_and_threshold():
    moved = [[103.0, 204.0], [143.0, 264.0]]                            # (3, 4): 5 px, exact in fp32
    sig = np.asarray(SIG2, f32).astype(np.float64)
    want = sum(math.exp(-25.0 / ((2.0 * s) ** 2) / 1e4 / 2.0) for s in sig) / 2     # 2^-52 vanishes beside the area
    assert 0.3 < want < 0.95
    r = R.track_frames(**_frames([[A], [moved]]), sigmas=SIG2)
    assert abs(r["track_oks"][1, 0] - want) <= 1e-15 and r["track_id"][1, 0] == 0
    r = R.track_frames(**_frames([[A], [moved]]), sigmas=SIG2, threshold=0.95)   # below: a birth
    assert r["track_id"][1, 0] == 1 and r["track_oks"][1, 0] == 0.0 and r["counts"][1].tolist() == [0, 1, 0, 2]


def test_ref_one_euro_constant_input_returns_the_input():
    fr = _frames([[A, None], [A, None], [None, A]])
    fr["scale"][:] = (3.0, 7.0)                                         # x sx is exact in double
    r = R.track_frames(**fr, sigmas=SIG2)
    assert r["track_id"].tolist() == [[0, -1], [0, -1], [-1, 0]]
    assert r["keypoints"].tobytes() == fr["kpts"].tobytes()


def test_ref_one_euro_hand_computed_step():
    b = [[103.0, 200.0], [140.0, 260.0]]                                # x of joint 0 moves by 3 px in one frame
    r = R.track_frames(**_frames([[A], [b]]), sigmas=SIG2, min_cutoff=1.0, beta=0.05, d_cutoff=1.0, fps=30.0)
    te = 1.0 / 30.0
    rr = 2.0 * math.pi * 1.0 * te
    ad = rr / (rr + 1.0)
    dxh = ad * (3.0 / te)                                               # dx^prev = 0
    fc = 1.0 + float(f32(0.05)) * dxh
    r2 = 2.0 * math.pi * fc * te
    a = r2 / (r2 + 1.0)
    want = a * 103.0 + (1.0 - a) * 100.0
    assert 100.5 < want < 102.9
    assert r["keypoints"][1, 0, 0, 0] == f32(want)
    assert r["keypoints"][1, 0].tolist()[0][1] == 200.0 and r["keypoints"][1, 0, 1].tolist() == [140.0, 260.0]
    # after a gap of one frame te doubles
    r = R.track_frames(**_frames([[A], [None], [b]]), sigmas=SIG2)
    te = 2.0 / 30.0
    rr = 2.0 * math.pi * 1.0 * te
    ad = rr / (rr + 1.0)
    fc = 1.0 + float(f32(0.05)) * (ad * (3.0 / te))
    a = 2.0 * math.pi * fc * te / (2.0 * math.pi * fc * te + 1.0)
    assert r["keypoints"][2, 0, 0, 0] == f32(a * 103.0 + (1.0 - a) * 100.0) and r["track_id"][2, 0] == 0


def test_ref_unconfident_joint_passes_through_and_restarts_its_filter():
    b = [[103.0, 200.0], [146.0, 260.0]]
    conf = [[[0.9, 0.9]], [[0.9, 0.1]], [[0.9, 0.9]]]                   # joint 1 does not count in frame 1
    r = R.track_frames(**_frames([[A], [b], [A]], conf=conf), sigmas=SIG2)
    assert list(r["track_id"][:, 0]) == [0, 0, 0]
    assert r["keypoints"][1, 0, 1].tolist() == [146.0, 260.0]           # passed through
    assert r["keypoints"][2, 0, 1].tolist() == [140.0, 260.0]           # no state: x^ = x
    assert 100.0 < r["keypoints"][2, 0, 0, 0] < 103.0                   # joint 0 kept filtering


def test_ref_state_carries_between_calls():
    fr = _frames([[A, None], [A, FAR], [FAR, A], [None, A]])
    whole = R.track_frames(**fr, sigmas=SIG2, max_age=0)
    state = R.new_state()
    cut = lambda a, b: {k: None if v is None else v[a:b] for k, v in fr.items()}   # noqa: E731
    first = R.track_frames(**cut(0, 1), state=state, sigmas=SIG2, max_age=0)
    rest = R.track_frames(**cut(1, 4), state=state, sigmas=SIG2, max_age=0)
    for k in ("track_id", "track_hits", "track_oks", "keypoints", "counts"):
        assert np.concatenate([first[k], rest[k]]).tobytes() == whole[k].tobytes(), k
    assert whole["counts"][3].tolist() == [1, 0, 0, 1] and state["frames"] == 4


# ------------------------------------------------------------------ the seeded cases (run on the GPU by test_track.py)
@pytest.mark.parametrize("name", C.NAMES)
def test_seeded_cases_keep_their_margins(name):
    _, _, ref = C.case(name)
    to_thr = min([p[0] for p in ref["picks"]] + [np.inf])
    to_other = min([p[1] for p in ref["picks"] if p[1] != 0.0] + [np.inf])
    print(name, "picks", len(ref["picks"]), "threshold margin", to_thr, "competitor margin", to_other, "pair margin",
          ref["pair_margin"], "ties", sum(p[1] == 0.0 for p in ref["picks"]))
    assert to_thr >= 1e-9 and to_other >= 1e-9 and ref["pair_margin"] >= 1e-9
    if name != "ties":
        assert all(p[1] != 0.0 for p in ref["picks"])                   # bit-equal candidates only where designed


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.CASES[n][2] is not None])
def test_seeded_cases_give_the_designed_ids(name):
    inputs, _, ref = C.case(name)
    want = np.asarray(C.CASES[name][2], np.int32)
    assert np.array_equal(ref["track_id"], want), (ref["track_id"], want)
    assert ((ref["track_id"] >= 0) | ~(inputs["scores"] > 0) | (name == "exhaust")).all()


def test_seeded_cases_exercise_the_feature():
    events = {k: sum(C.case(n)[2]["events"][k] for n in C.NAMES) for k in ("match", "birth", "death", "reid", "drop")}
    print(events)
    assert all(v > 0 for v in events.values()), events
    ex = C.case("exhaust")[2]
    assert ex["counts"].tolist() == [[0, 64, 0, 64], [0, 0, 64, 64], [0, 64, 0, 64], [64, 0, 0, 64]]
    assert (ex["track_id"][1] == -1).all() and (ex["track_hits"][1] == 0).all()
    assert C.case("gap2_age2")[2]["events"]["reid"] == 1 and C.case("gap3_age2")[2]["events"]["death"] == 1
    assert C.case("empty_frames")[2]["counts"][1:3].tolist() == [[0, 0, 0, 2], [0, 0, 0, 2]]
    assert np.isnan(C.case("births")[0]["scores"][0, 0]) and C.case("births")[2]["track_id"][0, 0] == -1
    ties = C.case("ties")[2]
    assert sum(p[1] == 0.0 for p in ties["picks"]) == 2 and ties["track_oks"][2, 4] > 0.3
    masks_in, _, masks = C.case("masks")
    assert masks["track_oks"][1, 2] == 0.0 and masks["track_hits"][2, 2] == 2
    vt = f32(C.VIS_THRESHOLD)
    assert (masks_in["kconf"][0, 0] <= vt).any() and (masks_in["kconf"][1, 0] <= vt).any()     # masked on either side
    assert ((masks_in["kconf"][0, 0] <= vt) != (masks_in["kconf"][1, 0] <= vt)).any()
    sw_in, _, sw = C.case("swap")
    assert (sw_in["scale"][0] != sw_in["scale"][1]).all() and (sw_in["scale"][:, 0] != sw_in["scale"][:, 1]).all()
    assert (sw["keypoints"] != sw_in["kpts"]).any()                     # the filter does something
    assert {C.case(n)[0]["kpts"].shape[1] for n in C.NAMES} == {1, 5, 64}
    assert all(C.case(n)[0]["kpts"].shape[0] <= 8 for n in C.NAMES)
    assert len({C.case(n)[0]["kpts"].shape[:3] for n in C.STACKED}) == 1


# ------------------------------------------------------------------ CLI: parsed before any device use
def _predict():
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    return __import__("predict")


def test_track_with_a_file_input_is_rejected(tmp_path, capsys):
    predict = _predict()
    image = tmp_path / "one.png"
    image.write_bytes(b"not decoded: the option is rejected first")
    with pytest.raises(SystemExit) as e:
        predict.main(["--config", "nowhere.yaml", "--model", "synthetic", "--input", str(image), "--output",
                      str(tmp_path / "out"), "--track"])
    assert e.value.code == 2 and "--track" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_unknown_track_value_is_rejected(capsys):
    predict = _predict()
    with pytest.raises(SystemExit) as e:
        predict.main(["--config", "nowhere.yaml", "--model", "synthetic", "--input", "nowhere", "--output", "nowhere",
                      "--track", "maybe"])
    assert e.value.code == 2 and "--track" in capsys.readouterr().err


def test_option_helpers():
    predict = _predict()
    ap = argparse.ArgumentParser()
    predict.add_track_arguments(ap)
    assert predict.track_options(ap.parse_args([])) is None
    assert predict.track_options(ap.parse_args(["--track", "off", "--track-threshold", "0.5"])) is None
    assert predict.track_options(ap.parse_args(["--track"])) == {"threshold": 0.3, "max_age": 10, "fps": 30.0,
                                                                 "smooth": True}
    got = predict.track_options(ap.parse_args(["--track", "on", "--track-threshold", "0.5", "--track-max-age", "3",
                                               "--track-fps", "25", "--track-no-smooth"]))
    assert got == {"threshold": 0.5, "max_age": 3, "fps": 25.0, "smooth": False}
