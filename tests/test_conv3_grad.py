"""The heatmap head's 3x3 convolution forward and backward (SURVEY §8(f)
rank 4, the backward of K6; kpd_conv3x3_forward / kpd_conv3x3_backward)
against torch autograd in float64 on the CPU.  Tolerance: 1e-5 of the
output's magnitude (fp32 sums of up to N*H*W = 6,272 products, exact
products on both sides).

The second half of the file moves the operands' magnitudes:
the split path picks its scales on the device -- per image for y and gx
(k6_amax_kernel -> k6_bound_kernel), tensor-global for the split wgrad -- so
y and gx are also judged per image, err_n <= 1e-5 * max|ref_n|: an image that
lost its precision next to a louder one must not pass on the louder one's
magnitude."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _ref(x, w, b, gy):
    x64, w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x64, w64, b64, padding=1)
    y.backward(gy.double().cpu())
    return y.detach(), x64.grad, w64.grad, b64.grad


def _close(got, want, rel=1e-5):
    got = got.detach().double().cpu()
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    assert err <= rel * scale, f"max|d| {err:.3e} > {rel} x {scale:.3e}"


@pytest.mark.parametrize("N,C,H,W,O", [(2, 64, 14, 14, 256), (1, 5, 9, 11, 7), (2, 256, 56, 56, 64), (1, 64, 56, 56, 256),
                                       (3, 17, 20, 13, 33)])
def test_conv3x3_forward_backward_vs_torch(N, C, H, W, O):
    from dll.ops import conv3x3
    g = torch.Generator().manual_seed(N * 1000 + C + O)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(O, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(O, generator=g) * 0.1
    gy = torch.randn(N, O, H, W, generator=g)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = conv3x3(xd, wd, bd)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    yr, gxr, gwr, gbr = _ref(x, w, b, gy)
    _close(y, yr)
    _close(xd.grad, gxr)
    _close(wd.grad, gwr)
    _close(bd.grad, gbr)


def test_conv3x3_deterministic_and_partial_grads():
    """Same inputs -> bit-identical gradients; gradients requested alone equal
    the ones computed together; no bias."""
    from dll import _native
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 32, 28, 28, generator=g).to(DEV)
    w = (torch.randn(48, 32, 3, 3, generator=g) * 0.1).to(DEV)
    gy = torch.randn(2, 48, 28, 28, generator=g).to(DEV)
    a = _native.conv3x3_backward(x, w, gy)
    b = _native.conv3x3_backward(x, w, gy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    gx, _, _ = _native.conv3x3_backward(x, w, gy, need_w=False, need_b=False)
    _, gw, _ = _native.conv3x3_backward(x, w, gy, need_x=False, need_b=False)
    assert torch.equal(gx, a[0]) and torch.equal(gw, a[1])
    y = _native.conv3x3_forward(x, w, None)
    _close(y, F.conv2d(x.double().cpu(), w.double().cpu(), None, padding=1))


def test_heatmap_head_conv_chain_grads():
    """The HeatmapHead conv chain shape (64 -> 256 -> 256 -> 64 at 56x56, BN
    folded, ReLU between): weight gradients of a loss through native convs
    equal torch autograd's.  The fp64 reference takes the ReLU masks of the
    native forward (a pre-activation within ~1e-6 of zero may fall on the
    other side of the kink in fp32; one flipped element moves a weight
    gradient by ~1e-4 of its magnitude), and the masks themselves agree with
    the fp64 forward's on all but a 1e-4 fraction of the elements."""
    from dll.ops import conv3x3
    g = torch.Generator().manual_seed(3)
    chans = [64, 256, 256, 64]
    ws = [torch.randn(chans[i + 1], chans[i], 3, 3, generator=g) * (2.0 / (9 * chans[i])) ** 0.5 for i in range(3)]
    bs = [torch.randn(chans[i + 1], generator=g) * 0.05 for i in range(3)]
    x = torch.rand(1, 64, 56, 56, generator=g)
    target = torch.rand(1, 64, 56, 56, generator=g)

    def run(conv, dev, dtype, masks):
        wp = [t.to(dev, dtype).requires_grad_(True) for t in ws]
        bp = [t.to(dev, dtype).requires_grad_(True) for t in bs]
        h = x.to(dev, dtype)
        own = []
        for i in range(3):
            pre = conv(h, wp[i], bp[i])
            own.append((pre > 0).cpu())
            h = pre * (own[i] if masks is None else masks[i]).to(dev, dtype)
        loss = ((h - target.to(dev, dtype)) ** 2).mean()
        loss.backward()
        return [p.grad for p in wp] + [p.grad for p in bp], own

    got, masks = run(conv3x3, DEV, torch.float32, None)
    want, masks64 = run(lambda h, w, b: F.conv2d(h, w, b, padding=1), "cpu", torch.float64, masks)
    for m, m64 in zip(masks, masks64):
        assert (m != m64).float().mean().item() <= 1e-4
    for u, v in zip(got, want):
        _close(u, v, rel=2e-5)


# ---------------------------------------------------------------- magnitudes
# (N, C, H, W, O): the split path (56 x 56, and the 64 -> 64 combination of
# k6_split_ok that no other test reaches) and the generic fp32 path
SHAPES = [(3, 64, 56, 56, 64), (3, 5, 9, 11, 7)]
SHAPE_IDS = ["split64to64", "generic"]
_DATA = {}


def _data(shape):
    """x, w, b, gy of a shape, drawn once and never modified."""
    if shape not in _DATA:
        N, C, H, W, O = shape
        g = torch.Generator().manual_seed(N * 1000 + C + O)
        _DATA[shape] = (torch.randn(N, C, H, W, generator=g), torch.randn(O, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5,
                        torch.randn(O, generator=g) * 0.1, torch.randn(N, O, H, W, generator=g))
    return _DATA[shape]


def _native_all(x, w, b, gy):
    """y, gx, gw, gb of the native forward and backward, on the host."""
    from dll import _native
    xd, wd, gyd = x.to(DEV), w.to(DEV), gy.to(DEV)
    y = _native.conv3x3_forward(xd, wd, None if b is None else b.to(DEV))
    gx, gw, gb = _native.conv3x3_backward(xd, wd, gyd)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (y, gx, gw, gb))


def _ref_all(x, w, b, gy):
    if b is not None:
        return _ref(x, w, b, gy)
    x64, w64 = (t.detach().double().requires_grad_(True) for t in (x, w))
    y = F.conv2d(x64, w64, None, padding=1)
    y.backward(gy.double())
    return y.detach(), x64.grad, w64.grad, gy.double().sum(dim=(0, 2, 3))


def _per_image(name, got, want, rel=1e-5):
    """err_n <= rel * max|ref_n| for every image n; the ratios err_n / (rel * max|ref_n|)."""
    assert torch.isfinite(got).all(), f"{name}: not finite"
    ratios = []
    for n in range(want.shape[0]):
        err = (got[n].double() - want[n]).abs().max().item()
        bar = rel * want[n].abs().max().item()
        ratios.append(err / bar if bar > 0 else (0.0 if err == 0 else float("inf")))
    print(f"{name} per-image error / bar: {[round(r, 4) for r in ratios]}")
    assert max(ratios) <= 1.0, f"{name}: per-image error / bar {ratios}"


def _check_all(label, got, want):
    _per_image(f"{label} y", got[0], want[0])
    _per_image(f"{label} gx", got[1], want[1])
    for name, u, v in (("gw", got[2], want[2]), ("gb", got[3], want[3])):
        assert torch.isfinite(u).all(), f"{label} {name}: not finite"
        _close(u, v)


def _pow2(t, k):
    return torch.ldexp(t, torch.tensor(k))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv3x3_per_image_bar(shape):
    """The plain draw, per image (the baseline of the cases below)."""
    x, w, b, gy = _data(shape)
    _check_all("plain", _native_all(x, w, b, gy), _ref_all(x, w, b, gy))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv3x3_mixed_magnitudes(shape):
    """x_n * {2^-20, 1, 2^12} with gy_n * {2^12, 2^-20, 1}, no bias (a bias would
    hide the quiet image's y behind itself): 2^32 between the images of one batch."""
    x, w, _, gy = _data(shape)
    fx = torch.tensor([2.0 ** -20, 1.0, 2.0 ** 12]).view(3, 1, 1, 1)
    fg = torch.tensor([2.0 ** 12, 2.0 ** -20, 1.0]).view(3, 1, 1, 1)
    _check_all("mixed", _native_all(x * fx, w, None, gy * fg), _ref_all(x * fx, w, None, gy * fg))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv3x3_zero_image_in_batch(shape):
    """Image 1 all zero in x and in gy: its y is the broadcast bias exactly, its gx zero exactly."""
    x, w, b, gy = _data(shape)
    x, gy = x.clone(), gy.clone()
    x[1] = 0
    gy[1] = 0
    got = _native_all(x, w, b, gy)
    _check_all("zero image", got, _ref_all(x, w, b, gy))
    assert torch.equal(got[0][1], b.view(-1, 1, 1).expand_as(got[0][1]))
    assert torch.count_nonzero(got[1][1]) == 0


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv3x3_zero_grad_y(shape):
    x, w, b, gy = _data(shape)
    _, gx, gw, gb = _native_all(x, w, b, torch.zeros_like(gy))
    for name, t in (("gx", gx), ("gw", gw), ("gb", gb)):
        assert torch.isfinite(t).all() and torch.count_nonzero(t) == 0, f"{name} must be exactly zero"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv3x3_zero_weights(shape):
    x, w, b, gy = _data(shape)
    got = _native_all(x, torch.zeros_like(w), b, gy)
    assert torch.equal(got[0], b.view(1, -1, 1, 1).expand_as(got[0]))
    assert torch.isfinite(got[1]).all() and torch.count_nonzero(got[1]) == 0
    want = _ref_all(x, torch.zeros_like(w), b, gy)
    _close(got[2], want[2])
    _close(got[3], want[3])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv3x3_tiny_products(shape):
    """x * 2^-40 with w * 2^-40 (forward) and gy * 2^-40 with w * 2^-40 (dgrad),
    no bias: max|x| * max|w| is below 2^-72, so k6_bound_kernel's a + we > 100
    branch lowers the input scale (split path); every result is ~2^-80."""
    x, w, _, gy = _data(shape)
    x, w, gy = _pow2(x, -40), _pow2(w, -40), _pow2(gy, -40)
    got, want = _native_all(x, w, None, gy), _ref_all(x, w, None, gy)
    assert want[0].abs().max() > 0 and want[1].abs().max() > 0
    _check_all("tiny", got, want)


@pytest.mark.parametrize("a,b", [(7, -3), (-20, 9)])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv3x3_scaling_law(shape, a, b):
    """The operator is linear and every scale a power of two: moving 2^a and 2^b
    onto the operands moves 2^(a+b) onto the result, bit for bit."""
    x, w, bias, gy = _data(shape)
    y0, gx0, gw0, gb0 = _native_all(x, w, bias, gy)
    y1, _, _, _ = _native_all(_pow2(x, a), _pow2(w, b), _pow2(bias, a + b), gy)
    assert torch.equal(y1, _pow2(y0, a + b)), "y"
    _, gx1, _, _ = _native_all(x, _pow2(w, b), bias, _pow2(gy, a))
    assert torch.equal(gx1, _pow2(gx0, a + b)), "gx"
    _, _, gw1, gb1 = _native_all(_pow2(x, a), w, bias, _pow2(gy, b))
    assert torch.equal(gw1, _pow2(gw0, a + b)), "gw"
    assert torch.equal(gb1, _pow2(gb0, b)), "gb"


def test_conv3x3_wgrad_dynamic_range():
    """The split wgrad's scale is tensor-global (max |gy|, max |x|): with gy's
    channel o scaled by 2^-(o mod 24) a quiet channel's hi keeps its 11 bits but
    its lo falls into f16 subnormals, so gw's rows of quiet channels are less
    accurate *relative to themselves* than the tensor-wide bar says.  A known
    property of the design (the training gradients of one conv are of one
    magnitude); only the tensor-wide bar is asserted.  Measured on MI355X
    (N = 3, 64 -> 64, 56 x 56): worst per-output-channel relative error 7.3e-5
    (the 2^-23 channels); 8.6e-7 at factor 1, 1.1e-6 at 2^-8, 1.3e-6 at 2^-16
    (DESIGN.md §5e)."""
    shape = SHAPES[0]
    x, w, b, gy = _data(shape)
    gy = gy * torch.tensor([2.0 ** -(o % 24) for o in range(shape[4])]).view(1, -1, 1, 1)
    got, want = _native_all(x, w, b, gy), _ref_all(x, w, b, gy)
    per = [(got[2][o].double() - want[2][o]).abs().max().item() / want[2][o].abs().max().item() for o in range(shape[4])]
    worst = max(range(shape[4]), key=lambda o: per[o])
    print(f"split wgrad, gy channel o x 2^-(o mod 24): worst per-output-channel relative error {per[worst]:.3e} "
          f"(channel {worst}, factor 2^-{worst % 24}); by factor: "
          f"{ {k: '%.1e' % max(per[o] for o in range(shape[4]) if o % 24 == k) for k in (0, 8, 16, 23)} }")
    assert torch.isfinite(got[2]).all()
    _close(got[2], want[2])
    _close(got[3], want[3])


def test_conv3x3_backward_checks_weight_shape():
    from dll import _native
    x = torch.zeros(1, 5, 9, 11, device=DEV)
    gy = torch.zeros(1, 7, 9, 11, device=DEV)
    for bad in ((7, 4, 3, 3), (7, 5, 3, 1), (7, 5, 9)):
        with pytest.raises(ValueError):
            _native.conv3x3_backward(x, torch.zeros(*bad, device=DEV), gy)
        with pytest.raises(ValueError):
            _native.conv3x3_forward(x, torch.zeros(*bad, device=DEV), None)
