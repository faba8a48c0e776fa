"""decode_planes_kernel<MODE> (csrc/ops_kernels.hip), all four modes, against
tests/ops_ref.decode_ref and the reference's own outputs (ops_edges.npz) on
the planes of tests/golden/ops_edges_cases.decode_jobs():

* plane sizes around the 256-thread stride and the idle-thread sentinel
  (2x2 .. 3x86, 2x300 and 300x2 which divide by W-1 = 1 / H-1 = 1, 96x72,
  128x128);
* equal maxima at flat indices i, i+1, i+256, i+257 in every combination
  (better() across threads and across the tree), an all-equal and an
  all -inf plane, the maximum at the last index;
* NaN: one, after / before the maximum, two in different threads, NaN
  against +inf, all NaN;
* sub-pixel windows 3, 5, 7, 0, 2, 4, -1, -3 and 9 on 4x4 with the maximum in
  every corner and on every edge, planes whose window mass is not positive,
  a mixed-sign window;
* soft-argmax temperatures 0.01, 0.5, 1, 100, -1, logits of +-80; 0 raises.

Bars: argmax coordinates, all scores and the visibility classes bit for bit
(equal_nan where the reference yields NaN).  Sub-pixel: (n_window + 3) *
2^-23 * sum|v x| / |sum v| / (W - 1) from decode_ref's own condition number.
Soft-argmax: 4 x the error of the reference's own fp32 formula against
decode_ref on the same planes, evaluated on the CPU (both are fp32 sums in
different orders), floor 1e-6.  Measured reference-side errors: at most
2.93e-6 (128x128, the nearly uniform softmax of a plane with one raised pixel,
T = 1 and 100), 2.3e-6 (96x72, same plane), 2.0e-6 at T = 0.01 (16x16), below
7e-7 everywhere else -- so the bars lie between 1e-6 and 1.2e-5.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import ops_ref as R  # noqa: E402
from ops_edges_cases import ARGMAX, MODEL, SOFTARGMAX, SUBPIXEL, decode_jobs  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
JOBS = decode_jobs()
_REFS = {}


def ref_of(key, heat, mode, param):
    """decode_ref once per job, shared by the tests and left unchanged."""
    if key not in _REFS:
        _REFS[key] = R.decode_ref(heat, mode, param)
    return _REFS[key]


@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(golden_dir / "ops_edges.npz", allow_pickle=False)


def _jobs(mode):
    return [j for j in JOBS if j[2] == mode]


def _run(heat, mode, param):
    from dll import _native
    k, s, v = _native.decode_heatmaps(heat.to(DEV), mode, param)
    return k.cpu().numpy(), s.cpu().numpy(), None if v is None else v.cpu().numpy()


def test_jobs_cover_the_issue_cases():
    keys = {j[0] for j in JOBS}
    for H, W in [(2, 2), (2, 3), (3, 2), (5, 51), (16, 16), (3, 86), (2, 300), (300, 2), (96, 72), (128, 128)]:
        for t in (0.01, 0.5, 1.0, 100.0, -1.0):
            assert f"size{H}x{W}_sa{t}" in keys
    for w in (3, 5, 7, 0, 2, 4):
        assert f"subpix9x11_sub{w}" in keys
    assert {"subpixneg9x11_sub-1", "subpixneg9x11_sub-3", "subpix4x4_sub9", "logits80_sa1.0"} <= keys
    tie = [j[1] for j in JOBS if j[0] == "tie96x72_255_argmax"][0]
    assert tie.shape[1] == 11                                   # every subset of size >= 2 of four indices
    flat = tie.view(11, -1)
    assert sorted({tuple((flat[k] == 0.9).nonzero().view(-1).tolist()) for k in range(11)})[0] == (255, 256)


@gpu
def test_argmax_bit_exact(edges):
    for key, heat, mode, param in _jobs(ARGMAX):
        r = ref_of(key, heat, mode, param)
        k, s, _ = _run(heat, mode, param)
        assert np.array_equal(k, r["kpts"].astype(np.float32)), key
        assert np.array_equal(s, r["scores"], equal_nan=True), key
        assert np.array_equal(k, edges[f"dec_{key}_kpts"]), key
        assert np.array_equal(s, edges[f"dec_{key}_scores"], equal_nan=True), key


@gpu
def test_subpixel_within_condition_bound(edges):
    worst = 0.0
    for key, heat, mode, param in _jobs(SUBPIXEL):
        H, W = heat.shape[2:]
        r = ref_of(key, heat, mode, param)
        k, s, _ = _run(heat, mode, param)
        bound = R.subpixel_bound(r, H, W)
        err = np.abs(k - r["kpts"])
        worst = max(worst, float(np.max(err - bound)))
        print(f"{key}: max err {err.max():.3e} bound {bound.max():.3e}")
        assert not np.isnan(k).any() and (err <= bound).all(), key
        assert np.array_equal(s, r["scores"]), key
        assert np.array_equal(s, edges[f"dec_{key}_scores"]), key
        # two fp32 evaluations (the reference's and the device's) each within the bound of the fp64 value
        assert (np.abs(k - edges[f"dec_{key}_kpts"]) <= 2 * bound).all(), key
        empty = r["n_window"] == 0
        assert (k[empty] == 0).all() and (s[empty] == 0).all(), key
    assert worst <= 0


def _softargmax_bar(heat, ref, temperature):
    fp32 = R.soft_argmax_fp32(heat, temperature)
    e = np.nanmax(np.abs(fp32 - ref["kpts"]), initial=0.0)
    return max(1e-6, 4.0 * float(e)), float(e)


@gpu
def test_soft_argmax_within_measured_bar(edges):
    for key, heat, mode, param in _jobs(SOFTARGMAX):
        r = ref_of(key, heat, mode, param)
        bar, e_ref = _softargmax_bar(heat, r, param)
        k, s, _ = _run(heat, mode, param)
        nan = np.isnan(r["kpts"])
        err = np.abs(k - r["kpts"])[~nan]
        print(f"{key}: device {err.max(initial=0):.3e} reference fp32 {e_ref:.3e} bar {bar:.3e}")
        assert np.array_equal(np.isnan(k), nan), key
        assert (err <= bar).all(), key
        assert np.array_equal(s, r["scores"], equal_nan=True), key
        assert np.array_equal(np.isnan(k), np.isnan(edges[f"dec_{key}_kpts"])), key
        assert (np.abs(k - edges[f"dec_{key}_kpts"])[~nan] <= bar + e_ref).all(), key


@gpu
def test_model_mode_and_visibility_classes():
    for key, heat, mode, param in _jobs(MODEL):
        r = ref_of(key, heat, mode, param)
        bar, e_ref = _softargmax_bar(heat, r, None)
        k, s, v = _run(heat, mode, param)
        nan = np.isnan(r["kpts"])
        assert np.array_equal(np.isnan(k), nan), key
        assert (np.abs(k - r["kpts"])[~nan] <= bar).all(), key
        assert np.array_equal(s, r["scores"], equal_nan=True), key
        assert np.array_equal(v, r["vis"]), key
    # every class is reached, the NaN maximum lands in class 2 as in the reference's comparisons
    seen = np.concatenate([_REFS[j[0]]["vis"].reshape(-1, 3) for j in _jobs(MODEL)]).sum(axis=0)
    assert (seen > 0).all()


@gpu
def test_model_decode_heatmap_method(model_sd):
    """MultiPersonKeypointModel.decode_heatmap reaches the same kernel: one odd size."""
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig())
    m.load_state_dict(model_sd)
    m = m.to(DEV).eval()
    key, heat, mode, param = [j for j in _jobs(MODEL) if j[0] == "size3x86_model"][0]
    r = ref_of(key, heat, mode, param)
    k, v = m.decode_heatmap(heat.to(DEV))
    nan = np.isnan(r["kpts"])
    assert np.array_equal(np.isnan(k.cpu().numpy()), nan)
    assert (np.abs(k.cpu().numpy() - r["kpts"])[~nan] <= _softargmax_bar(heat, r, None)[0]).all()
    assert np.array_equal(v.cpu().numpy(), r["vis"])


@gpu
def test_zero_temperature_is_rejected():
    from dll import _native
    from dll.models import decode_heatmaps_soft_argmax
    with pytest.raises(_native.KpdNativeError):
        decode_heatmaps_soft_argmax(torch.rand(1, 2, 4, 4, device=DEV), temperature=0.0)


@gpu
def test_wrappers_keep_reference_shapes_and_empty_batches():
    from dll.models import decode_heatmaps, decode_heatmaps_soft_argmax, decode_heatmaps_subpixel
    h3 = torch.rand(5, 7, 9, generator=torch.Generator().manual_seed(8))            # [K, H, W], not a golden size
    a = R.decode_ref(h3[None], ARGMAX)
    k, s = decode_heatmaps(h3.to(DEV))
    assert k.shape == (5, 2) and s.shape == (5,)
    assert np.array_equal(k.cpu().numpy(), a["kpts"][0].astype(np.float32)) and np.array_equal(s.cpu().numpy(), a["scores"][0])
    k, s = decode_heatmaps_subpixel(h3.to(DEV), window_size=5)                       # the reference keeps the batch dim
    assert k.shape == (1, 5, 2) and s.shape == (1, 5)
    b = R.decode_ref(h3[None], SUBPIXEL, 5)
    assert (np.abs(k.cpu().numpy() - b["kpts"]) <= R.subpixel_bound(b, 7, 9)).all()
    k, s = decode_heatmaps_soft_argmax(h3.to(DEV), temperature=0.5)
    assert k.shape == (5, 2) and s.shape == (5,)
    np.testing.assert_allclose(k.cpu().numpy(), R.decode_ref(h3[None], SOFTARGMAX, 0.5)["kpts"][0], atol=1e-6)
    for shape in ((0, 17, 6, 5), (3, 0, 6, 5)):                                       # B*K = 0
        e = torch.empty(*shape, device=DEV)
        for fn in (decode_heatmaps, decode_heatmaps_subpixel, decode_heatmaps_soft_argmax):
            k, s = fn(e)
            assert k.shape == (*shape[:2], 2) and s.shape == shape[:2]
