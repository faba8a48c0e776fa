"""kpd_roi_targets on the device against the numpy restatement
(tests/roi_targets_ref.py): weights equal, planes within 4 x the float32
rule's own deviation from float64 (not below 1e-6), row gathering, n = 0, the
W % 4 != 0 tail, and the decode round trip through the device argmax decoder."""
import numpy as np
import pytest
import torch

import roi_targets_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = {"r6k17_56": (6, 17, 56, 56, 2.0), "r3k5_14x10": (3, 5, 14, 10, 1.0)}


def _inputs(R, K):
    kpts, vis, boxes, where = RR.cases(R, K, seed=3)
    # [B, P] = [R, 1]: generate_roi_targets flattens to R ROIs
    t = [torch.from_numpy(a).to(DEV) for a in (kpts[:, None], vis[:, None], boxes[:, None])]
    return kpts, vis, boxes, where, t


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("rows", [None, [2, 0, 1], [4, 0, 3]], ids=["all", "gather201", "gather403"])
def test_kernel_matches_restatement(shape, rows):
    from dll.models.heatmap_head import generate_roi_targets
    R, K, H, W, sigma = SHAPES[shape]
    if rows is not None and max(rows) >= R:
        rows = [r % R for r in rows]
    kpts, vis, boxes, where, (kd, vd, bd) = _inputs(R, K)
    heat, weight = generate_roi_targets(kd, vd, bd, rows, (H, W), sigma)
    torch.cuda.synchronize()
    r64, w64 = RR.roi_targets_ref(kpts, vis, boxes, rows, H, W, sigma)
    r32, _ = RR.roi_targets_ref(kpts, vis, boxes, rows, H, W, sigma, dtype=np.float32)
    n = R if rows is None else len(rows)
    assert tuple(heat.shape) == (n, K, H, W) and tuple(weight.shape) == (n, K)
    assert np.array_equal(weight.cpu().numpy(), w64)
    got = heat.double().cpu().numpy()
    err, e32 = float(np.abs(got - r64).max()), float(np.abs(r32 - r64).max())
    bound = max(4 * e32, 1e-6)
    print(f"{shape} rows={rows}: native {err:.3e}  fp32 restatement {e32:.3e}  bound {bound:.3e}")
    assert err <= bound
    off = w64 == 0
    assert off.any() and not got[off].any()          # every off plane is exactly zero
    if rows is None:
        for name, (r, k) in where.items():
            want = 1.0 if name in ("u0", "u1") else 0.0
            assert float(weight[r, k]) == want, name


def test_no_rows():
    from dll.models.heatmap_head import generate_roi_targets
    _, _, _, _, (kd, vd, bd) = _inputs(3, 5)
    heat, weight = generate_roi_targets(kd, vd, bd, torch.zeros(0, dtype=torch.int32, device=DEV), (14, 10), 1.0)
    assert tuple(heat.shape) == (0, 5, 14, 10) and tuple(weight.shape) == (0, 5)


def test_rows_as_device_tensor_and_python_errors():
    from dll.models.heatmap_head import generate_roi_targets
    _, _, _, _, (kd, vd, bd) = _inputs(6, 17)
    a = generate_roi_targets(kd, vd, bd, [4, 0, 3])
    b = generate_roi_targets(kd, vd, bd, torch.tensor([4, 0, 3], dtype=torch.int32, device=DEV))
    full = generate_roi_targets(kd, vd, bd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], full[0][[4, 0, 3]]) and tuple(full[0].shape) == (6, 17, 56, 56)
    with pytest.raises(ValueError):
        generate_roi_targets(kd, vd, bd, None, (1, 56))
    with pytest.raises(ValueError):
        generate_roi_targets(kd, vd[:, :, :5], bd)


def test_decode_round_trip_on_device():
    """decode_heatmaps (device argmax) of each `on` plane, its pixel read as
    i/(W-1) and mapped through the unclamped box, recovers the labelled joint
    within 0.5 heatmap pixels per axis."""
    from dll.models.heatmap_head import decode_heatmaps, generate_roi_targets
    kpts, vis, boxes, _ = RR.cases(24, 17, seed=11)
    kd, vd, bd = (torch.from_numpy(a).to(DEV) for a in (kpts[:, None], vis[:, None], boxes[:, None]))
    heat, weight = generate_roi_targets(kd, vd, bd)
    kp, score = decode_heatmaps(heat)
    on = weight.cpu().numpy() > 0
    idx = np.rint(kp.double().cpu().numpy() * 55)          # the decoder returns i / (W - 1) in float32
    assert float(np.abs(idx / 55 - kp.double().cpu().numpy()).max()) < 1e-6
    b = boxes.astype(np.float64)[:, None, :]
    got = idx / 55 * b[..., 2:] + (b[..., :2] - b[..., 2:] / 2)
    with np.errstate(all="ignore"):
        err = np.abs(got - kpts.astype(np.float64)) / b[..., 2:] * 55
    worst = float(err[on].max())
    print(f"device decode round trip: {worst:.3f} heatmap pixels over {int(on.sum())} joints")
    assert on.sum() > 300 and worst <= 0.5
    assert float(score.cpu().numpy()[on].min()) >= np.exp(-0.25 / 4.0) - 1e-6
