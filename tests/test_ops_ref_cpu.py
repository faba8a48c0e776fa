"""tests/ops_ref.py against what the project already trusts, so the references
of the operator edge tests are not their own judges (no GPU).

* decode_ref reproduces tests/golden/decoders.npz (the reference's own
  outputs) at the bars of test_gpu_api.test_decoders_vs_golden, and the
  reference's three decoders on every edge plane of ops_edges.npz.
* roi_align_ref(aligned=False, sampling_ratio=-1) equals
  oracle.kpd_oracle.roi_align_loop on the oracle's boxes, on the three golden
  boxes, and the golden ROI slice.  There is no torchvision on these
  machines: the aligned=True and fixed-sampling-ratio paths rest on the
  restatement of torchvision's roi_align forward alone (they differ from the
  pinned path only by the half-pixel offset, the missing clamp of the ROI size
  to 1, and grid = sampling_ratio).
* target_heatmap_ref / keypoint_metrics_ref reproduce data.npz and
  ops_edges.npz; channel_select_ref reproduces ca_scores / ca_topk.

Measured here (and used as bars by the GPU tests, never the device's output):
the reference's fp32 Gaussian table against the fp64 table differs by at most
3.13e-7 relative over the ops_edges target cases (TABLE_REL_ERR below); the reference's fp32 soft-argmax against
decode_ref by at most 2.93e-6 (the nearly uniform softmax of the 128 x 128
plane with one raised pixel, T = 1 and 100; 2.3e-6 at 96 x 72), 2.0e-6 at
T = 0.01 (16 x 16) and below 7e-7 on every other edge plane.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import decoder_cases  # noqa: E402
import ops_ref as R  # noqa: E402
from data_cases import heatmap_cases, metric_cases  # noqa: E402
from ops_edges_cases import (ARGMAX, MODEL, SOFTARGMAX, SUBPIXEL, decode_jobs, target_cases,  # noqa: E402
                             metric_cases as edge_metric_cases)
from oracle import kpd_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(golden_dir / "ops_edges.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def dec(golden_dir):
    return np.load(golden_dir / "decoders.npz", allow_pickle=False), decoder_cases.inputs()


subpixel_bound = R.subpixel_bound


def test_decode_ref_reproduces_decoder_golden(dec):
    g, c = dec
    for name, h in (("", c["h"]), ("hr_", c["hr"])):
        r = R.decode_ref(h, ARGMAX)
        assert np.array_equal(r["kpts"].astype(np.float32), g[f"{name}argmax_kpts"])
        if not name:
            assert np.array_equal(r["scores"], g["argmax_scores"])
    for w in (3, 5):
        r = R.decode_ref(c["h"], SUBPIXEL, w)
        np.testing.assert_allclose(r["kpts"], g[f"sub{w}_kpts"], atol=1e-6)
        np.testing.assert_allclose(r["scores"], g[f"sub{w}_scores"], atol=0)
        # non-negative planes: sum|v x| / |sum v| <= W - 1, so the bound is at most (n + 3) ulp of 1
        assert (subpixel_bound(r, 56, 56) <= (w * w + 3) * 2.0 ** -23).all()
    for i, t in enumerate(g["sa_temps"]):
        r = R.decode_ref(c["h"], SOFTARGMAX, float(t))
        np.testing.assert_allclose(r["kpts"], g[f"sa{i}_kpts"], atol=1e-6)
        assert np.array_equal(r["scores"], g[f"sa{i}_scores"])
    np.testing.assert_allclose(R.decode_ref(c["hr"], SUBPIXEL, 3)["kpts"], g["hr_sub_kpts"], atol=1e-6)
    np.testing.assert_allclose(R.decode_ref(c["hr"], SOFTARGMAX, 1.0)["kpts"], g["hr_sa_kpts"], atol=1e-6)
    r = R.decode_ref(c["h"], MODEL)
    np.testing.assert_allclose(r["kpts"], g["model_kpts"], atol=1e-6)
    np.testing.assert_allclose(r["kpts"], g["model_sa"], atol=1e-6)
    assert np.array_equal(r["vis"], g["model_vis"])
    assert np.array_equal(r["vis"], O.visibility_classes(c["h"]).numpy())


def test_decode_ref_reproduces_edge_fixture(edges):
    worst_sa = {}
    for key, heat, mode, param in decode_jobs():
        if mode == MODEL:
            continue
        H, W = heat.shape[2:]
        r = R.decode_ref(heat, mode, param)
        want_k, want_s = edges[f"dec_{key}_kpts"], edges[f"dec_{key}_scores"]
        assert want_k.shape == r["kpts"].shape and want_s.shape == r["scores"].shape, key
        assert np.array_equal(r["scores"], want_s, equal_nan=True), key
        assert np.array_equal(np.isnan(r["kpts"]), np.isnan(want_k)), key
        if mode == ARGMAX:
            assert np.array_equal(r["kpts"].astype(np.float32), want_k), key
        elif mode == SUBPIXEL:
            assert (np.abs(r["kpts"] - want_k) <= subpixel_bound(r, H, W)).all(), key
        else:
            # the restated fp32 formula is the fixture's; its distance from decode_ref is the measured bar
            fp32 = R.soft_argmax_fp32(heat, param)
            assert np.array_equal(fp32, want_k, equal_nan=True), key
            e = np.nanmax(np.abs(fp32 - r["kpts"]), initial=0.0)
            worst_sa[param] = max(worst_sa.get(param, 0.0), float(e))
    print("soft-argmax, reference fp32 vs decode_ref, max |d| per temperature:", worst_sa)
    assert max(worst_sa.values()) <= 3.0e-6, worst_sa          # the measured maximum of the module docstring


def test_roi_align_ref_matches_oracle_loop(dec):
    g, c = dec
    feat = torch.randn(8, 20, 16, generator=torch.Generator().manual_seed(3))
    boxes = [(1.3, 2.2, 9.7, 17.9), (0.0, 0.0, 16.0, 20.0), (15.5, 19.5, 16.0, 20.0), (3.0, 3.0, 3.2, 3.1),
             (0.0, 0.0, 0.0, 0.0)]
    rois = torch.tensor([[0.0, *b] for b in boxes])
    got, info = R.roi_align_ref(feat[None], rois, 7)
    for i, b in enumerate(boxes):
        np.testing.assert_allclose(got[i], O.roi_align_loop(feat, *b, out=7).numpy(), atol=2e-6)
    # the three golden boxes (cxcywh -> pixel corners as extract_roi_features does) and the golden ROI slice
    feats = c["feats"]
    _, C, H, W = feats.shape
    corners = [O.box_center_to_corners(b) * torch.tensor([W, H, W, H], dtype=torch.float32) for b in c["boxes"]]
    rois = torch.stack([torch.cat([torch.zeros(1), cr]) for cr in corners])
    got, _ = R.roi_align_ref(feats[:1, :8], rois, 14)
    for i, cr in enumerate(corners):
        want = O.roi_align_loop(feats[0, :8], *[float(v) for v in cr], out=14).numpy()
        np.testing.assert_allclose(got[i], want, atol=2e-6)
    got, _ = R.roi_align_ref(feats[:1, :8], rois[1:2], (56, 56))
    np.testing.assert_allclose(got[0, :, 20:28, 10:18], g["roi_feat_slice"], atol=1e-6)


def test_roi_align_ref_exact_on_dyadic_grid():
    """Integer-valued features, a box on the pixel grid at dyadic coordinates:
    every weight is dyadic, the result is exact -- and known in closed form for
    a linear ramp (bilinear interpolation reproduces it inside the map)."""
    H, W = 20, 16
    ramp = (torch.arange(H).view(H, 1) * 3 + torch.arange(W).view(1, W) * 5).float().view(1, 1, H, W)
    rois = torch.tensor([[0.0, 2.0, 4.0, 10.0, 12.0]])
    got, info = R.roi_align_ref(ramp, rois, (4, 4), 1.0, 2, False)          # bins 2 x 2 pixels, samples at .5, 1.5
    cy = 4.0 + (np.arange(4) + 0.5) * 2.0
    cx = 2.0 + (np.arange(4) + 0.5) * 2.0
    assert np.array_equal(got[0, 0], cy[:, None] * 3 + cx[None, :] * 5)
    got, _ = R.roi_align_ref(ramp, rois, (4, 4), 1.0, 2, True)              # aligned: half a pixel up and left
    assert np.array_equal(got[0, 0], (cy[:, None] - 0.5) * 3 + (cx[None, :] - 0.5) * 5)
    got, _ = R.roi_align_ref(ramp, rois * torch.tensor([1.0, 2, 2, 2, 2]), (4, 4), 0.5, -1, False)
    assert np.array_equal(got[0, 0], cy[:, None] * 3 + cx[None, :] * 5)     # spatial_scale folds the box back


TABLE_REL_ERR = R.TABLE_REL_ERR


def _rel(a, b):
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def test_target_heatmap_ref_reproduces_goldens(golden_dir, edges):
    g = np.load(golden_dir / "data.npz", allow_pickle=False)
    for i, (kp, size, sigma) in enumerate(heatmap_cases()):
        want = g[f"hm_out{i}"]
        got = R.target_heatmap_ref(kp, size, sigma)
        assert got.shape == want.shape and np.array_equal(got == 0, want == 0), i
        assert np.abs(got - want).max() <= 4e-9, i
    worst = 0.0
    for name, kp, size, sigma, adaptive in target_cases():
        s = R.adaptive_sigma(size, sigma) if adaptive else sigma
        want = edges[f"hm_{name}"]
        got = R.target_heatmap_ref(kp, size, s)
        assert got.shape == want.shape and np.array_equal(got == 0, want == 0), name
        worst = max(worst, _rel(want.astype(np.float64), got))
    print("reference fp32 Gaussian table vs fp64 table, max relative difference:", worst)
    assert 0 < worst <= TABLE_REL_ERR
    assert edges["hm_s2p9999999"].astype(bool).sum(axis=(2, 3)).max() == 13 * 13      # int(2.9999999) = 2
    assert edges["hm_s0p8"].max() == 1.0 and set(np.unique(edges["hm_s0p8"])) == {0.0, 1.0}


def test_keypoint_metrics_ref_reproduces_goldens(golden_dir, edges):
    g = np.load(golden_dir / "data.npz", allow_pickle=False)
    for i, (pred, gt, vis) in enumerate(metric_cases()):
        pred = pred.squeeze(2) if pred.dim() == 5 else pred
        if pred.dim() == 4 and gt.dim() == 3:
            pred = pred[:, 0]
        if pred.shape != gt.shape:
            continue
        ade, pck, _ = R.keypoint_metrics_ref(pred, gt, vis, [0.002, 0.05, 0.2])
        np.testing.assert_allclose([ade] + pck, g[f"met_out{i}"], rtol=1e-6, atol=1e-7)
    for name, pred, gt, vis, thr in edge_metric_cases():
        ade, pck, counts = R.keypoint_metrics_ref(pred, gt, vis, thr)
        want = edges[f"met_{name}"]
        np.testing.assert_allclose([ade] + pck, want, rtol=1e-6, atol=1e-7, err_msg=name)
        n = vis.numel()
        assert [round(float(p) * n) for p in want[1:]] == counts[1:], name          # the PCK counts, exactly
    _, _, counts = R.keypoint_metrics_ref(*edge_metric_cases()[5][1:4], [0.25, 0.3125, 0.5])
    assert counts == [7, 2, 5, 6]           # on-threshold distances count (<=); 0.25000012 does not; vis -1 is hidden


def test_channel_select_ref_reproduces_golden(dec, model_sd):
    g, c = dec
    scores, topk, gap = R.channel_select_ref(c["feats"], model_sd)
    np.testing.assert_allclose(scores, g["ca_scores"], atol=1e-6)
    assert np.array_equal(topk, g["ca_topk"])
    assert (gap > 2e-6).all()
    # the stated order on ties and NaN: NaN first, then score descending, index ascending
    sd = {k: v.clone() for k, v in model_sd.items()}
    sd["channel_attention.fc.2.weight"][7] = sd["channel_attention.fc.2.weight"][90]
    sd["channel_attention.fc.2.bias"][7] = sd["channel_attention.fc.2.bias"][90]
    scores, topk, _ = R.channel_select_ref(c["feats"], sd)
    assert (scores[:, 7] == scores[:, 90]).all()
    for b in range(2):
        t = topk[b].tolist()
        assert (7 in t) == (90 in t) or t[-1] == 7
        if 90 in t:
            assert t.index(90) == t.index(7) + 1
    x = c["feats"].clone()
    x[1, 3, 2, 2] = float("nan")
    scores, topk, _ = R.channel_select_ref(x, model_sd)
    assert np.isnan(scores[1]).all() and topk[1].tolist() == list(range(64)) and not np.isnan(scores[0]).any()
