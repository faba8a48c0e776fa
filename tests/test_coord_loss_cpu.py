"""The float64 restatement of the coordinate loss (tests/coord_loss_ref.py)
checked without a GPU: torch.autograd.gradcheck of the composition, its
all-masked case, and the declaration of the two native entry points."""
import re

import pytest
import torch

import coord_loss_ref as CR
from conftest import ROOT

SHAPE = (3, 17, 5, 7)


@pytest.mark.parametrize("loss_type", ["smooth_l1", "mse", "huber"])
@pytest.mark.parametrize("temperature", [1.0, 0.02])
@pytest.mark.parametrize("tau", [5.0, 0.05])
def test_restatement_passes_gradcheck(loss_type, temperature, tau):
    """3 x 17 x 5 x 7 in float64, one gt at 1.8 (rho's linear branch), seeds
    at which no joint is within 1e-3 of a kink."""
    heat, gt, vis, _ = CR.make_case(SHAPE, temperature, tau)
    assert float(gt.max()) == pytest.approx(1.8)
    h = heat.double().requires_grad_(True)
    fn = lambda t: CR.coord_loss(t, gt, vis, temperature, loss_type, 100.0, tau)[0]   # noqa: E731
    assert torch.autograd.gradcheck(fn, (h,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_all_masked_is_zero():
    heat, gt, vis, _ = CR.make_case(SHAPE, 1.0, 5.0)
    loss, coords, grad = CR.loss_and_grad(heat, torch.full_like(gt, float("nan")), torch.zeros_like(vis))
    assert float(loss) == 0.0 and not grad.any() and torch.isfinite(coords).all()


def test_masked_nan_labels_reach_nothing():
    heat, gt, vis, _ = CR.make_case(SHAPE, 1.0, 5.0)
    want = CR.loss_and_grad(heat, gt, vis)
    got = CR.loss_and_grad(heat, torch.where((vis > 0).unsqueeze(-1), gt, torch.full_like(gt, float("nan"))), vis)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert not got[2][vis <= 0].any()


def test_entry_points_are_declared():
    """kpd_coord_loss and kpd_softargmax_backward: in include/kpd.h and in _native.EXPORTS."""
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    for name in ("kpd_coord_loss", "kpd_softargmax_backward"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in _native.EXPORTS, name
