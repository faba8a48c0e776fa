"""target_heatmap_kernel and keypoint_metrics_kernel (csrc/data_kernels.hip)
against the reference's own outputs (tests/golden/ops_edges.npz) and
tests/ops_ref.target_heatmap_ref / keypoint_metrics_ref.

Targets: sigmas fp32 cannot represent (2.4, the adaptive 3 * 48 / 56 and
3 * 0.8, 1.016), 2.9999999 whose fp32 value is 3.0 (the kernel size follows
the double: 13 x 13), sigma 0.8 (kernel size 1), a 19 x 19 Gaussian on an
8 x 8 map, W of 1, 2, 3, 5, 8, 41 (the float4 and the scalar store path),
keypoints at x*W just below and exactly at W, a NaN keypoint (zero plane: the
reference raises there), planes = 0, generate_target_heatmap_adaptive.

Bar for the values: relative.  The reference's own fp32 table differs from
target_heatmap_ref's fp64 table by at most 3.13e-7 relative over these cases
(measured on the CPU by test_ops_ref_cpu.py, ops_ref.TABLE_REL_ERR); the device may
differ from the fixture by at most 4 x that = 1.25e-6, its normalising sum
being taken in another order.  The support (which pixels are zero) is exact.

Metrics: n of 1, 255, 256, 257 and 5000 (the single workgroup's strided
loop), distances exactly on a threshold (<=), 16 thresholds (17 raise),
visibilities of 0.5 and -1, nothing visible.  ADE / PCK within 1e-6 relative
of the reference's fp32 means (the bar of test_data.py); the PCK counts exact.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import ops_ref as R  # noqa: E402
from ops_edges_cases import metric_cases, target_cases, target_nan_case  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAR = 4 * R.TABLE_REL_ERR


@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(golden_dir / "ops_edges.npz", allow_pickle=False)


def _rel(a, b):
    nz = b != 0
    return float(np.max(np.abs(a[nz].astype(np.float64) - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def test_cases_reach_both_store_paths_and_the_border_columns(edges):
    names = [c[0] for c in target_cases()]
    assert {f"w{W}" for W in (1, 2, 3, 5, 8, 41)} <= set(names)
    for name, kp, (H, W), sigma, _ in target_cases():
        if not name.startswith("w"):
            continue
        want = edges[f"hm_{name}"]
        assert want[0, 0, :, W - 1].max() > 0            # x*W just below W: the last column is the centre
        assert (want[0, 1] == 0).all() and (want[0, 3] == 0).all() and (want[0, 5] == 0).all()   # at W / H, below 0
        assert want[0, 2, H - 1].max() > 0 and want[0, 4, 0, 0] > 0


@gpu
def test_targets_match_the_reference(edges):
    from dll.models.heatmap_head import generate_target_heatmap, generate_target_heatmap_adaptive
    for name, kp, size, sigma, adaptive in target_cases():
        fn = generate_target_heatmap_adaptive if adaptive else generate_target_heatmap
        got = fn(kp.to(DEV), size, sigma).cpu().numpy()
        want = edges[f"hm_{name}"]
        ref = R.target_heatmap_ref(kp, size, R.adaptive_sigma(size, sigma) if adaptive else sigma)
        assert got.shape == want.shape, name
        assert np.array_equal(got == 0, want == 0) and np.array_equal(got == 0, ref == 0), name      # the support
        print(f"{name}: device vs fixture {_rel(got, want.astype(np.float64)):.3e}, vs fp64 table {_rel(got, ref):.3e}")
        assert _rel(got, want.astype(np.float64)) <= BAR, name
        assert _rel(got, ref) <= BAR, name
    got = generate_target_heatmap_adaptive(target_cases()[0][1].to(DEV), (30, 41), 2.4, adaptive=False).cpu().numpy()
    assert _rel(got, edges["hm_s2p4"].astype(np.float64)) <= BAR


@gpu
def test_kernel_size_follows_the_double_sigma(edges):
    """int(2.9999999) = 2 -> 13 x 13; the fp32 value of that sigma is 3.0 (19 x 19)."""
    from dll.models.heatmap_head import generate_target_heatmap
    name, kp, size, sigma, _ = [c for c in target_cases() if c[0] == "s2p9999999"][0]
    assert np.float32(sigma) == np.float32(3.0) and int(sigma) == 2
    got = generate_target_heatmap(kp.to(DEV), size, sigma).cpu().numpy()
    assert (got != 0).sum(axis=(2, 3)).max() == 13 * 13
    assert np.array_equal(got == 0, edges[f"hm_{name}"] == 0)


@gpu
def test_nan_keypoints_empty_input_and_4d_layout():
    from dll.models.heatmap_head import generate_target_heatmap
    kp, size, sigma = target_nan_case()
    got = generate_target_heatmap(kp.to(DEV), size, sigma).cpu().numpy()
    ref = R.target_heatmap_ref(kp, size, sigma)
    assert (got[0, 1:4] == 0).all() and got[0, 0].max() > 0 and got[0, 4].max() > 0
    assert np.array_equal(got == 0, ref == 0) and _rel(got, ref) <= BAR
    assert generate_target_heatmap(torch.empty(0, 17, 2, device=DEV), (8, 8), 2.4).shape == (0, 17, 8, 8)
    assert generate_target_heatmap(torch.empty(2, 0, 2, device=DEV), (8, 8), 2.4).shape == (2, 0, 8, 8)
    kp4 = torch.rand(2, 3, 4, 2, generator=torch.Generator().manual_seed(2))        # [B,P,K,2]: the first B rows
    got = generate_target_heatmap(kp4.to(DEV), (9, 10), 1.3).cpu().numpy()
    ref = R.target_heatmap_ref(kp4, (9, 10), 1.3)
    assert got.shape == (2, 4, 9, 10) and np.array_equal(got == 0, ref == 0) and _rel(got, ref) <= BAR


@gpu
def test_metrics_match_the_reference(edges):
    from dll.utils import calculate_validation_metrics
    for name, pred, gt, vis, thr in metric_cases():
        m = calculate_validation_metrics({"keypoints": pred.to(DEV)},
                                         {"keypoints": gt.to(DEV), "visibilities": vis.to(DEV)}, pck_thresholds=thr)
        got = np.array([m["avg_ADE"]] + [m[f"pck_{t}"] for t in thr])
        ade, pck, counts = R.keypoint_metrics_ref(pred, gt, vis, thr)
        np.testing.assert_allclose(got, edges[f"met_{name}"], rtol=1e-6, atol=1e-7, err_msg=name)
        np.testing.assert_allclose(got, [ade] + pck, rtol=1e-6, atol=1e-7, err_msg=name)
        n = vis.numel()
        assert [int(round(p * n)) for p in got[1:]] == counts[1:], name              # the PCK counts, exactly
        assert all(abs(p * n - round(p * n)) < 1e-3 * max(1, p * n) for p in got[1:]), name
    assert set(np.unique(torch.cat([c[3].view(-1) for c in metric_cases()]).numpy())) >= {-1.0, 0.0, 0.5, 2.0}


@gpu
def test_seventeen_thresholds_raise():
    from dll import _native
    from dll.utils import calculate_validation_metrics
    name, pred, gt, vis, thr = metric_cases()[0]
    seventeen = [0.01 * (i + 1) for i in range(17)]
    with pytest.raises(_native.KpdNativeError):
        calculate_validation_metrics({"keypoints": pred.to(DEV)}, {"keypoints": gt.to(DEV), "visibilities": vis.to(DEV)},
                                     pck_thresholds=seventeen)
