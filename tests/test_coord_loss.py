"""kpd_coord_loss / kpd_softargmax_backward on the device
against the float64 restatement of tests/coord_loss_ref.py.

The tolerance is not a constant: every comparison also runs the same formulas
as a float32 torch chain on the device, and the native result's deviation from
float64 has to stay within

    max(4 x that chain's deviation, 4 x 2^-23 x max|reference|)      per output

(4: the two fp32 evaluations differ only in the order of their sums and in
their exp).  Both deviations are printed.

Measured on the MI355X, native / fp32 chain, each relative to the output's
maximum, worst case of its group: loss 7.2e-8 / 9.9e-8; coords 6.0e-8 / 5.6e-7;
gradient at T = 1 1.8e-7 / 4.6e-7 and at T = 0.02 1.7e-7 / 1.6e-6; soft_argmax
backward at T = 1 2.0e-7 / 2.5e-7 and at T = 0.02 1.1e-7 / 1.7e-6.  The native
result used at most 0.41 of its bound (on the 2 x 2 plane, where the bound is
its floor) and 0.26 on every other shape.
"""
from functools import lru_cache

import ctypes

import pytest
import torch

import coord_loss_ref as CR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SHAPES = [(1, 1, 2, 2),          # the minimum
          (3, 17, 5, 7),         # a plane smaller than a wave
          (2, 17, 9, 13),        # plane size no multiple of 64
          (3, 17, 56, 56),       # 51 planes, no multiple of the waves per workgroup, register path
          (2, 5, 64, 48),        # the head on a non-square map
          (40, 17, 56, 56)]      # 680 planes: more than one stride of the final sum, 8.5 MB
TEMPERATURES = [1.0, 0.02]
LOSS_TYPES = ["smooth_l1", "mse", "huber"]
TAUS = [5.0, 0.2]
SCALE = 100.0
EPS32 = 2.0 ** -23


def _dev(a, ref):
    return float((a.detach().double().cpu() - ref.double()).abs().max())


def _bound(chain_dev, ref):
    return max(4 * chain_dev, 4 * EPS32 * float(ref.double().abs().max()))


def _check(name, native, chain, ref):
    dn, dc = _dev(native, ref), _dev(chain, ref)
    bound = _bound(dc, ref)
    scale = max(float(ref.double().abs().max()), 1e-300)
    print(f"  {name}: native dev {dn:.3e} ({dn / scale:.2e} of max)  fp32 chain dev {dc:.3e} "
          f"({dc / scale:.2e})  bound {bound:.3e}")
    assert dn <= bound, f"{name}: native deviation {dn:.3e} > bound {bound:.3e} (fp32 chain {dc:.3e})"


@lru_cache(maxsize=None)
def _reference(shape, temperature, loss_type, tau):
    heat, gt, vis, seed = CR.make_case(shape, temperature, tau)
    kw = dict(temperature=temperature, loss_type=loss_type, pixel_weight_scale=SCALE, distance_threshold=tau)
    return CR.loss_and_grad(heat, gt, vis, **kw), kw, seed


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("temperature", TEMPERATURES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_coords_and_gradient_match_float64(shape, temperature, loss_type, tau):
    from dll.ops import soft_argmax_coord_loss
    heat, gt, vis, _ = CR.make_case(shape, temperature, tau)
    (loss64, coords64, grad64), kw, seed = _reference(shape, temperature, loss_type, tau)
    # on the float64 values: no visible joint near a kink; at tau = 0.2 the clamp band and the part beyond it
    # are populated (where the case has joints enough to ask)
    margin, q = CR.kink_distance(coords64, gt, vis, tau)
    assert margin > CR.KINK_MARGIN
    assert float(gt.max()) == pytest.approx(1.8)
    if tau == 0.2 and q.numel() >= 20:
        band, beyond = int(((q > 1) & (q < 3)).sum()), int((q > 3).sum())
        assert band >= q.numel() // 5 and beyond >= 1, (band, beyond, q.numel())
    h = heat.to(DEV).requires_grad_(True)
    loss, coords = soft_argmax_coord_loss(h, gt.to(DEV), vis.to(DEV), **kw)
    loss.backward()
    c_loss, c_coords, c_grad = CR.loss_and_grad(heat, gt, vis, dtype=torch.float32, device=DEV, **kw)
    print(f"\n{shape} T={temperature} {loss_type} tau={tau} seed={seed}: loss {float(loss64):.6e}")
    _check("loss", loss, c_loss, loss64)
    _check("coords", coords, c_coords, coords64)
    _check("grad", h.grad, c_grad, grad64)
    assert not coords.requires_grad and tuple(coords.shape) == (*shape[:2], 2)
    assert not h.grad[(vis <= 0).to(DEV)].any()          # masked planes: exactly zero


@pytest.mark.parametrize("temperature", TEMPERATURES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_soft_argmax_forward_is_the_decoder_and_backward_matches_float64(shape, temperature):
    from dll.models import decode_heatmaps_soft_argmax
    from dll.ops import soft_argmax
    heat, _, _, _ = CR.make_case(shape, temperature, 5.0)
    gc = torch.randn(*shape[:2], 2, generator=torch.Generator().manual_seed(7))
    h = heat.to(DEV).requires_grad_(True)
    coords = soft_argmax(h, temperature)
    assert torch.equal(coords.detach(), decode_heatmaps_soft_argmax(heat.to(DEV), temperature)[0])
    coords.backward(gc.to(DEV))
    _, grad64 = CR.softargmax_vjp(heat, gc, temperature)
    _, c_grad = CR.softargmax_vjp(heat, gc, temperature, dtype=torch.float32, device=DEV)
    print(f"\n{shape} T={temperature}")
    _check("grad_heat", h.grad, c_grad, grad64)


def _nan_masked(gt, vis):
    return torch.where((vis > 0).unsqueeze(-1), gt, torch.full_like(gt, float("nan")))


@pytest.mark.parametrize("shape", [(2, 17, 9, 13), (3, 17, 56, 56)], ids=lambda s: "x".join(map(str, s)))
def test_masked_joints_with_nan_labels(shape):
    """NaN gt on the masked joints: the loss is finite and the restatement's
    (which never sees those labels), the masked gradient planes exactly zero,
    and loss and gradient bit-identical to the call with finite labels there."""
    from dll.ops import soft_argmax_coord_loss
    heat, gt, vis, _ = CR.make_case(shape, 1.0, 0.2)
    (loss64, coords64, grad64), kw, _ = _reference(shape, 1.0, "smooth_l1", 0.2)
    assert int((vis <= 0).sum()) > 0
    out = []
    for g in (_nan_masked(gt, vis), gt):
        h = heat.to(DEV).requires_grad_(True)
        loss, _ = soft_argmax_coord_loss(h, g.to(DEV), vis.to(DEV), **kw)
        loss.backward()
        out.append((loss.detach(), h.grad))
    (loss, grad), (loss_f, grad_f) = out
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert torch.equal(loss, loss_f) and torch.equal(grad, grad_f)
    assert not grad[(vis <= 0).to(DEV)].any()
    c_loss, _, c_grad = CR.loss_and_grad(heat, gt, vis, dtype=torch.float32, device=DEV, **kw)
    _check("loss", loss, c_loss, loss64)
    _check("grad", grad, c_grad, grad64)


@pytest.mark.parametrize("shape", [(3, 17, 5, 7), (3, 17, 56, 56)], ids=lambda s: "x".join(map(str, s)))
def test_all_joints_masked(shape):
    from dll.ops import soft_argmax_coord_loss
    heat, gt, vis, _ = CR.make_case(shape, 1.0, 5.0)
    h = heat.to(DEV).requires_grad_(True)
    loss, coords = soft_argmax_coord_loss(h, torch.full_like(gt, float("nan")).to(DEV), torch.zeros_like(vis).to(DEV))
    loss.backward()
    assert float(loss.detach()) == 0.0 and not h.grad.any() and not torch.isnan(h.grad).any()
    assert torch.isfinite(coords).all()


@pytest.mark.parametrize("shape", [(2, 17, 9, 13), (3, 17, 56, 56)], ids=lambda s: "x".join(map(str, s)))
def test_constant_plane_decodes_to_the_centre(shape):
    from dll.ops import soft_argmax_coord_loss
    heat = torch.full(shape, 0.37)
    gt, vis = torch.zeros(*shape[:2], 2), torch.ones(shape[:2])
    _, coords = soft_argmax_coord_loss(heat.to(DEV), gt.to(DEV), vis.to(DEV))
    with torch.no_grad():
        chain = CR.soft_argmax(heat.to(DEV), 1.0)
    _check("coords", coords, chain, torch.full((*shape[:2], 2), 0.5, dtype=torch.float64))


@pytest.mark.parametrize("shape", [(2, 17, 9, 13), (3, 17, 56, 56), (40, 17, 56, 56)],
                         ids=lambda s: "x".join(map(str, s)))
def test_two_calls_are_bit_identical(shape):
    from dll.ops import soft_argmax_coord_loss
    heat, gt, vis, _ = CR.make_case(shape, 0.02, 0.2)
    runs = []
    for _ in range(2):
        h = heat.to(DEV).requires_grad_(True)
        loss, coords = soft_argmax_coord_loss(h, gt.to(DEV), vis.to(DEV), temperature=0.02, distance_threshold=0.2)
        loss.backward()
        runs.append((loss.detach(), coords, h.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_an_unaligned_view_takes_the_generic_path():
    """A 56 x 56 tensor that starts one element into its storage (planes not 16-byte aligned): same loss and
    coordinates within fp32 rounding of the aligned call's, nothing read or written out of place."""
    from dll import _native
    heat, gt, vis, _ = CR.make_case((3, 17, 56, 56), 1.0, 5.0)
    flat = torch.zeros(heat.numel() + 1, device=DEV)
    flat[1:] = heat.to(DEV).flatten()
    view = flat[1:].view(heat.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    a = _native.coord_loss(heat.to(DEV), gt.to(DEV), vis.to(DEV), 1.0, "smooth_l1", 100.0, 5.0, True)
    b = _native.coord_loss(view, gt.to(DEV), vis.to(DEV), 1.0, "smooth_l1", 100.0, 5.0, True)
    (loss64, coords64, grad64), _, _ = _reference((3, 17, 56, 56), 1.0, "smooth_l1", 5.0)
    for name, x, y, ref in zip(("loss", "coords", "grad"), b, a, (loss64, coords64, grad64)):
        _check(name, x, y, ref)


def test_module_and_no_grad():
    from dll import _native
    from dll.losses import SoftArgmaxCoordinateLoss
    heat, gt, vis, _ = CR.make_case((3, 17, 5, 7), 1.0, 5.0)
    fn = SoftArgmaxCoordinateLoss()
    with pytest.raises(_native.KpdNativeError):
        fn(heat, gt, vis)                                   # CPU tensors raise
    loss = fn(heat.to(DEV), gt.to(DEV), vis.to(DEV))
    assert not loss.requires_grad and tuple(fn.last_coords.shape) == (3, 17, 2)
    (loss64, _, _), _, _ = _reference((3, 17, 5, 7), 1.0, "smooth_l1", 5.0)
    assert float(loss) == pytest.approx(float(loss64), rel=1e-5)
    with pytest.raises(ValueError):
        SoftArgmaxCoordinateLoss(loss_type="l1")
    with pytest.raises(ValueError):
        SoftArgmaxCoordinateLoss(temperature=0.0)


def test_bad_arguments_raise():
    from dll import _native
    from dll.ops import soft_argmax, soft_argmax_coord_loss
    heat, gt, vis = torch.rand(2, 3, 4, 5, device=DEV), torch.rand(2, 3, 2, device=DEV), torch.ones(2, 3, device=DEV)
    for bad_t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            soft_argmax_coord_loss(heat, gt, vis, temperature=bad_t)
        with pytest.raises(ValueError):
            soft_argmax(heat, bad_t)
    with pytest.raises(ValueError):
        soft_argmax_coord_loss(heat, gt, vis, loss_type="l1")
    with pytest.raises(ValueError):
        soft_argmax_coord_loss(heat, gt, vis, distance_threshold=0.0)
    with pytest.raises(ValueError):
        soft_argmax_coord_loss(heat, gt[:, :2], vis)
    with pytest.raises(ValueError):
        soft_argmax_coord_loss(heat, gt, vis[:1])
    with pytest.raises(ValueError):
        soft_argmax_coord_loss(heat[:, :, :1], gt, vis)         # H = 1
    with pytest.raises(ValueError):
        soft_argmax(heat[..., :1])                              # W = 1
    with pytest.raises(ValueError):
        soft_argmax(heat[0])                                    # not [n, K, H, W]
    with pytest.raises(_native.KpdNativeError):
        soft_argmax(heat.cpu())
    # the C entry points themselves: KPD_EINVAL with a message, nothing launched
    lib, f = _native.load(), ctypes.c_float
    p = [_native._ptr(t) for t in (heat, gt, vis)]
    out = [_native._ptr(torch.empty(6, 2, device=DEV)), _native._ptr(torch.empty((), device=DEV)), None, None]
    for planes, H, W, T, kind, tau in ((-1, 4, 5, 1.0, 0, 5.0), (6, 1, 5, 1.0, 0, 5.0), (6, 4, 1, 1.0, 0, 5.0),
                                       (6, 4, 5, 0.0, 0, 5.0), (6, 4, 5, float("nan"), 0, 5.0),
                                       (6, 4, 5, float("inf"), 0, 5.0), (6, 4, 5, 1.0, 3, 5.0),
                                       (6, 4, 5, 1.0, 0, 0.0)):
        assert lib.kpd_coord_loss(*p, planes, H, W, f(T), kind, f(100.0), f(tau), *out) == -1
        assert b"kpd_coord_loss" in lib.kpd_last_error()
    for planes, H, W, T in ((-1, 4, 5, 1.0), (6, 1, 5, 1.0), (6, 4, 5, -2.0)):
        assert lib.kpd_softargmax_backward(p[0], p[1], planes, H, W, f(T), _native._ptr(torch.empty_like(heat)),
                                           None) == -1


def test_no_planes_is_a_noop_with_loss_zero():
    from dll.ops import soft_argmax, soft_argmax_coord_loss
    heat = torch.empty(0, 17, 56, 56, device=DEV, requires_grad=True)
    loss, coords = soft_argmax_coord_loss(heat, torch.empty(0, 17, 2, device=DEV), torch.empty(0, 17, device=DEV))
    assert float(loss.detach()) == 0.0 and tuple(coords.shape) == (0, 17, 2)
    loss.backward()
    assert heat.grad is None or heat.grad.numel() == 0
    assert tuple(soft_argmax(heat.detach()).shape) == (0, 17, 2)
