"""kpd_track_poses (csrc/track.hip) and dll.utils.PoseTracker on the GPU: the
kernel against the numpy restatement tests/track_ref.py on the seeded cases of
tests/track_cases.py, the state carry, the independence of sequences, and
PoseTracker.track on a real forward.  tests/test_track_cpu.py asserts the
margins of the same cases without a GPU.

Tolerances (derived, none measured).  track_id, track_hits and counts: exact.
track_oks within 1e-12 absolute, for the reason tests/test_pose_nms.py gives:
both sides use double and the same operation order, device and host exp() may
differ by a few ulp, ~1e-15 on each term; every decision of every case keeps
1e-9 from its alternatives (test_track_cpu.py), so none can flip.  kpts_out
within one fp32 ulp of the restatement's fp32 cast: over <= 8 frames the double
filter values differ by ~1e-13 relative at most (division rounding, exp is not
involved), which can only move the rounding to fp32 at a tie.  A constant input
comes back bit-equal: x sx is exact in double, a x + (1 - a) x is within 2 ulp
(double) of it, and dividing by sx and rounding to fp32 returns x.
"""
import ctypes

import numpy as np
import pytest
import torch

import track_cases as C
import track_ref as R

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
OUTPUTS = ("track_id", "track_hits", "track_oks", "keypoints", "counts")


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _tracker(opts, K, S=1, **over):
    from dll.utils import PoseTracker
    return PoseTracker(K, S, device=DEV, **{**opts, **over})


def _update(tr, inputs, frames=slice(None)):
    out = tr.update(**{k: None if v is None else _dev(v[..., frames, :, :, :] if k == "kpts" else
                                                      v[..., frames, :, :] if k == "kconf" else v[..., frames, :])
                       for k, v in inputs.items()})
    torch.cuda.synchronize()
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref):
    for k in ("track_id", "track_hits", "counts"):
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert got["track_oks"].dtype == np.float64 and got["track_oks"].shape == ref["track_oks"].shape
    err = float(np.abs(got["track_oks"] - ref["track_oks"]).max()) if ref["track_oks"].size else 0.0
    want = ref["keypoints"]
    assert got["keypoints"].dtype == f32 and got["keypoints"].shape == want.shape
    ulps = np.abs(got["keypoints"].astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
    print("max |track_oks - ref| =", err, " max keypoint error in fp32 ulp =", float(ulps.max()) if ulps.size else 0.0)
    assert err <= 1e-12, err
    assert (ulps <= 1.0).all()


@gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_gpu_kernel_matches_restatement(name):
    inputs, opts, ref = C.case(name)
    got = _update(_tracker(opts, inputs["kpts"].shape[2]), inputs)
    _compare(got, ref)
    if C.CASES[name][2] is not None:
        assert np.array_equal(got["track_id"], np.asarray(C.CASES[name][2], np.int32))


@gpu
def test_gpu_table_exhaustion_counts():
    inputs, opts, _ = C.case("exhaust")
    got = _update(_tracker(opts, 17), inputs)
    assert got["counts"].tolist() == [[0, 64, 0, 64], [0, 0, 64, 64], [0, 64, 0, 64], [64, 0, 0, 64]]
    assert (got["track_id"][1] == -1).all() and (got["track_hits"][1] == 0).all()
    assert got["keypoints"][1].tobytes() == inputs["kpts"][1].tobytes()             # dropped poses pass through
    assert sorted(got["track_id"][2]) == list(range(64, 128)) and (got["track_hits"][3] == 2).all()


@gpu
def test_gpu_without_kconf_every_keypoint_counts():
    inputs, opts, _ = C.case("masks")
    inputs = dict(inputs, kconf=None)
    ref = R.track_frames(**inputs, **opts)
    assert min(p[0] for p in ref["picks"]) >= 1e-9 and ref["pair_margin"] >= 1e-9
    assert ref["track_id"][:, 2].tolist() == [1, 1, 1, 1]                           # nothing is blind without kconf
    _compare(_update(_tracker(opts, 17), inputs), ref)


@gpu
def test_gpu_state_carries_between_calls_and_reset():
    inputs, opts, ref = C.case("gap3_age2")
    tr = _tracker(opts, 17)
    whole = _update(tr, inputs, slice(0, 7))
    _compare(whole, {k: ref[k][:7] for k in OUTPUTS})
    tr2 = _tracker(opts, 17)
    a, b = _update(tr2, inputs, slice(0, 3)), _update(tr2, inputs, slice(3, 7))
    for k in OUTPUTS:
        assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes(), k
    assert tr2.state.cpu().numpy().tobytes() == tr.state.cpu().numpy().tobytes()
    again = _update(tr2, inputs, slice(0, 3))                                       # without a reset the ids go on
    assert again["track_id"].max() > whole["track_id"][:3].max()
    tr2.reset()
    assert not tr2.state.any()
    again = _update(tr2, inputs, slice(0, 3))
    for k in OUTPUTS:
        assert again[k].tobytes() == a[k].tobytes(), k


@gpu
def test_gpu_no_slots_still_age_the_tracks():
    inputs, opts, _ = C.case("gap0_age0")
    tr = _tracker(opts, 17, max_age=1)
    first = _update(tr, inputs, slice(0, 2))
    assert first["counts"].tolist() == [[0, 1, 0, 1], [1, 0, 0, 1]]
    z = lambda *s: torch.zeros(*s, device=DEV)    # noqa: E731
    out = tr.update(z(3, 0, 17, 2), z(3, 0), z(3, 0), torch.ones(3, 2, device=DEV), z(3, 0, 17))
    torch.cuda.synchronize()
    assert out["track_id"].shape == (3, 0) and out["keypoints"].shape == (3, 0, 17, 2)
    assert out["counts"].tolist() == [[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0]]     # age 1, then 2 > max_age
    after = _update(tr, inputs, slice(2, 4))
    assert after["track_id"].tolist() == [[1], [1]] and after["counts"].tolist() == [[0, 1, 0, 1], [1, 0, 0, 1]]


@gpu
def test_gpu_sequence_alone_gives_the_same_bytes():
    cases = [C.case(n) for n in C.STACKED]
    opts = cases[0][1]
    assert all(c[1] == opts for c in cases)
    stacked = {k: np.stack([c[0][k] for c in cases]) for k in cases[0][0]}
    tr = _tracker(opts, 17, S=3)
    whole = _update(tr, stacked)
    assert whole["track_id"].shape == (3, 8, 5) and whole["counts"].shape == (3, 8, 4)
    state = tr.state.cpu().numpy()
    for s, (inputs, _, ref) in enumerate(cases):
        one = _tracker(opts, 17)
        alone = _update(one, inputs)
        for k in OUTPUTS:
            assert alone[k].tobytes() == whole[k][s].tobytes(), (k, s)
        assert one.state.cpu().numpy().tobytes() == state[s:s + 1].tobytes()
        _compare({k: whole[k][s] for k in OUTPUTS}, ref)


@gpu
def test_gpu_smoothing_off_keeps_the_ids_and_writes_no_keypoints():
    from dll import _native
    inputs, opts, ref = C.case("swap")
    off = _update(_tracker(opts, 17, smooth=False), inputs)
    for k in ("track_id", "track_hits", "counts"):
        assert np.array_equal(off[k], ref[k]), k
    assert np.abs(off["track_oks"] - ref["track_oks"]).max() <= 1e-12
    assert off["keypoints"].tobytes() == inputs["kpts"].tobytes()                   # the input itself
    # the C call with smooth = 0 and a buffer: not a byte of it is written
    B, D, K = inputs["kpts"].shape[:3]
    t = {k: _dev(v) for k, v in inputs.items()}
    state = torch.zeros(_native.load().kpd_track_state_bytes(K) // 8, dtype=torch.int64, device=DEV)
    ids, hits = (torch.empty(B, D, dtype=torch.int32, device=DEV) for _ in range(2))
    counts = torch.empty(B, 4, dtype=torch.int32, device=DEV)
    sentinel = torch.full((B, D, K, 2), -12345.5, device=DEV)
    p = _native._ptr
    rc = _native.load().kpd_track_poses(
        p(t["kpts"]), p(t["scores"]), p(t["area"]), p(t["kconf"]), p(t["scale"]), (ctypes.c_float * K)(*opts["sigmas"]),
        1, B, D, K, opts["threshold"], opts["vis_threshold"], opts["max_age"], 0, 1.0, 0.05, 1.0, 30.0, p(state), p(ids),
        p(hits), None, p(sentinel), p(counts), _native._stream(DEV))
    _native.check(rc, "kpd_track_poses")
    torch.cuda.synchronize()
    assert (sentinel == -12345.5).all()
    assert np.array_equal(ids.cpu().numpy(), ref["track_id"]) and np.array_equal(counts.cpu().numpy(), ref["counts"])


@gpu
def test_gpu_two_runs_are_bit_identical():
    inputs, opts, _ = C.case("exhaust")
    a, b = _update(_tracker(opts, 17), inputs), _update(_tracker(opts, 17), inputs)
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k


@gpu
def test_gpu_non_default_stream():
    inputs, opts, ref = C.case("births")
    tr = _tracker(opts, 17)
    t = {k: _dev(v) for k, v in inputs.items()}
    tr.reset()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        out = tr.update(**t)
    s.synchronize()
    _compare({k: v.cpu().numpy() for k, v in out.items()}, ref)


def _forward_frames(n=3):
    """One synthetic image with two boxes, repeated as n frames."""
    from dll.configs import BackboneConfig, ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_images, synthetic_state_dict
    m = MultiPersonKeypointModel(ModelConfig(backbone=BackboneConfig(in_channels=1, input_size=64)), TrainingConfig())
    m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0))
    m = m.to(DEV).eval()
    x = synthetic_images(1, 1, 64, 64, seed=7).to(DEV).expand(n, -1, -1, -1).contiguous()
    boxes = torch.tensor([[[0.5, 0.5, 0.4, 0.8], [0.3, 0.4, 0.2, 0.3]]], device=DEV).expand(n, -1, -1).contiguous()
    with torch.no_grad():
        return m({"image": x, "bboxes": boxes})


@gpu
def test_gpu_track_on_a_forward():
    from dll.utils import PoseTracker
    out = _forward_frames(3)
    before = {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}
    keys = set(out)
    tr = PoseTracker(device=DEV)
    got = tr.track(out, (128, 96))
    torch.cuda.synchronize()
    assert set(out) == keys and all(torch.equal(out[k], v) for k, v in before.items())   # the inputs are untouched
    assert got is not out and got["heatmap"] is out["heatmap"] and got["keypoints_raw"] is out["keypoints"]
    assert got["track_ids"].dtype == torch.int32 and got["track_ids"].tolist() == [[0, 1]] * 3
    assert got["track_hits"].tolist() == [[1, 1], [2, 2], [3, 3]]
    assert got["track_counts"].tolist() == [[0, 2, 0, 2], [2, 0, 0, 2], [2, 0, 0, 2]]
    assert (got["track_oks"][1:] == 1.0).all() and (got["track_oks"][0] == 0).all()
    assert got["keypoints"].shape == out["keypoints"].shape and got["keypoints"] is not out["keypoints"]
    assert torch.equal(got["keypoints"], out["keypoints"])                           # a constant input, bit for bit
    # the next chunk goes on where this one ended; a suppressed pose is absent
    kept = dict(out, box_scores=torch.ones(3, 2, device=DEV))                        # what suppress_poses leaves
    more = tr.track(kept, (128, 96))
    assert more["track_ids"].tolist() == [[0, 1]] * 3 and more["track_hits"][2].tolist() == [6, 6]
    kept["box_scores"] = kept["box_scores"] * torch.tensor([1.0, 0.0], device=DEV)
    gone = tr.track(kept, (128, 96))
    assert gone["track_ids"].tolist() == [[0, -1]] * 3 and gone["track_counts"][:, 3].tolist() == [2, 2, 2]
    with pytest.raises(ValueError):
        tr.track({k: v for k, v in out.items() if k != "boxes"}, (128, 96))
    with pytest.raises(ValueError):
        PoseTracker(num_sequences=2, device=DEV).track(out, (128, 96))
