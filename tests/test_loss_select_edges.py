"""The adaptive heatmap loss (keypoint-detection_amd/csrc/loss_kernels.hip, kpd_adaptive_heatmap_loss)
at the edges of its threshold select and of its focal term.

Select: the threshold bit-exact against torch.clamp(torch.quantile(gt, 0.9),
0.05, 0.3) in fp32 on the CPU, on the inputs of tests/loss_select_cases.py --
negative values (the other branch of the order-preserving key), signed zeros
and denormals, planted order statistics whose key carries a 0xFF byte or whose
neighbours differ in one key byte alone, a selected value followed by a copy of
itself or by a larger value, n of 1, 2 and 3, constant tensors, and n around
the fixed grid's 1024 * 256 elements.  Every case first asserts on the CPU that
the clamp does not hide the quantile (check_band).

Loss and gradient: oracle/loss_oracle.py with autograd, at the tolerances of
tests/test_loss.py -- 2e-6 relative on the loss, rtol 1e-5 with atol 1e-6 *
max|grad| on the gradient.  A NaN in gt is outside the contract
(include/kpd.h) and is not tested."""
import numpy as np
import pytest
import torch

import loss_select_cases as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _native_loss(pred, gt, tw, alpha, want_grad=True):
    from dll import _native
    out = _native.adaptive_heatmap_loss(pred.to(DEV), gt.to(DEV), None if tw is None else tw.to(DEV), 50.0, 1.0, True,
                                        alpha, want_grad)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in out)


@pytest.mark.parametrize("name", list(S.CASES))
def test_threshold_is_torchs_quantile(name):
    want = S.check_band(name)
    x = S.build(name).view(1, 1, 1, -1)
    _, _, thr = _native_loss(x, x, None, 0.0, want_grad=False)
    print(f"{name}: n {x.numel()}, threshold {float(thr)!r}, torch {float(want)!r}")
    assert float(thr) == float(want)
    assert thr.view(torch.int32).item() == want.view(torch.int32).item()   # the sign of a zero included


@pytest.mark.parametrize("alpha", [1.0, 0.5, 3.0])
def test_focal_alpha_through_powf(alpha):
    pred, gt = S.loss_inputs()
    assert float((pred - gt).abs().min()) >= 1e-2
    want_loss, want_grad = S.oracle_loss_and_grad(pred, gt, None, alpha)
    assert bool(torch.isfinite(want_loss)) and bool(torch.isfinite(want_grad).all())
    loss, grad, _ = _native_loss(pred, gt, None, alpha)
    print(f"alpha {alpha}: loss {float(loss)!r} oracle {float(want_loss)!r}, "
          f"max|dgrad| {float((grad - want_grad).abs().max()):.3e} of max|grad| {float(want_grad.abs().max()):.3e}")
    assert float(loss) == pytest.approx(float(want_loss), rel=2e-6)
    np.testing.assert_allclose(grad.numpy(), want_grad.numpy(), rtol=1e-5, atol=1e-6 * float(want_grad.abs().max()))


@pytest.mark.parametrize("alpha", [0.0, 2.0, 1.5])
def test_pred_equal_to_gt_is_exactly_zero(alpha):
    _, gt = S.loss_inputs()
    loss, grad, _ = _native_loss(gt.clone(), gt, None, alpha)
    assert float(loss) == 0.0
    assert bool(torch.isfinite(grad).all()) and torch.count_nonzero(grad) == 0


def test_zero_target_weight_row():
    pred, gt = S.loss_inputs()
    tw = torch.ones(S.LOSS_SHAPE[:2])
    tw[1, 2] = 0.0
    want_loss, want_grad = S.oracle_loss_and_grad(pred, gt, tw, 2.0)
    loss, grad, _ = _native_loss(pred, gt, tw, 2.0)
    assert torch.count_nonzero(grad[1, 2]) == 0
    assert torch.count_nonzero(grad[1, 1]) > 0
    assert float(loss) == pytest.approx(float(want_loss), rel=2e-6)
    np.testing.assert_allclose(grad.numpy(), want_grad.numpy(), rtol=1e-5, atol=1e-6 * float(want_grad.abs().max()))


@pytest.mark.parametrize("name", ["negatives_4097", "copy_below_then_larger", "grid_plus_1"])
def test_without_the_gradient_the_same_bits(name):
    gt = S.build(name).view(1, 1, 1, -1)
    pred = (gt + 0.1).contiguous()
    l1, g1, t1 = _native_loss(pred, gt, None, 2.0, want_grad=True)
    l0, g0, t0 = _native_loss(pred, gt, None, 2.0, want_grad=False)
    assert g0 is None and g1 is not None
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    assert torch.equal(t0.view(torch.int32), t1.view(torch.int32))
