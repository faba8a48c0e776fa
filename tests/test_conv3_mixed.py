"""dll.ops.conv3x3(..., precision="mixed") on the device (DESIGN.md §3i;
kpd_conv3x3_forward_prec / kpd_conv3x3_backward_prec with KPD_PRECISION_MIXED)
against its CPU restatement in float64 (tests/conv3_mixed_ref.py): every
product is of two operands each rounded to bf16 from its fp32 value, summed in
fp32.

Tolerance: 1e-5 of the output's magnitude, the bar and the reason of
tests/test_conv3_grad.py -- the device and the restatement multiply the same
rounded operands, a product of two bf16 values is exact in fp32, so the two
differ by the fp32 accumulation alone.  The split path cannot pass: its results
differ from the rounded-operand reference by ~2^-9 relative per operand.  y and
gx are also judged per image at the three-image shapes.

A second bar ties the results to the *unrounded* float64 convolution by the
elementwise cap (2^-8 + 2^-18) * (|w| (*) |x|) (tests/test_conv3_mixed_cpu.py)
plus the accumulation bar: a path that rounds worse than bf16, or twice,
fails it."""
import pytest
import torch

from conv3_mixed_ref import CAP, exact_all, mixed_all

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (N, C, H, W, O): the hmconv fast path (64 -> 256; 256 -> 64 with the output padded to a 128-column tile
# and a 64 -> 256 dgrad; 64 -> 64 with odd N and tiles that straddle two images; the 256 x 256 wgrad
# tile) and the generic kernels with ragged tiles
VS_REF = [(1, 64, 56, 56, 256), (2, 256, 56, 56, 64), (3, 64, 56, 56, 64), (1, 256, 56, 56, 256), (1, 5, 9, 11, 7),
          (3, 17, 20, 13, 33)]
SHAPES = [(3, 64, 56, 56, 64), (3, 5, 9, 11, 7)]
SHAPE_IDS = ["hm64to64", "generic"]
_DATA = {}
_REF = {}


def _data(shape):
    """x, w, b, gy of a shape, drawn once and never modified."""
    if shape not in _DATA:
        N, C, H, W, O = shape
        g = torch.Generator().manual_seed(N * 1000 + C + O)
        _DATA[shape] = (torch.randn(N, C, H, W, generator=g), torch.randn(O, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5,
                        torch.randn(O, generator=g) * 0.1, torch.randn(N, O, H, W, generator=g))
    return _DATA[shape]


def _plain_ref(shape):
    """The restatement of a shape's plain draw in float64, computed once."""
    if shape not in _REF:
        _REF[shape] = mixed_all(*_data(shape))
    return _REF[shape]


def _native_all(x, w, b, gy, precision="mixed"):
    """y, gx, gw, gb of the native forward and backward, on the host."""
    from dll import _native
    xd, wd, gyd = x.to(DEV), w.to(DEV), gy.to(DEV)
    y = _native.conv3x3_forward(xd, wd, None if b is None else b.to(DEV), precision=precision)
    gx, gw, gb = _native.conv3x3_backward(xd, wd, gyd, precision=precision)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (y, gx, gw, gb))


def _close(name, got, want, rel=1e-5):
    assert torch.isfinite(got).all(), f"{name}: not finite"
    scale = want.abs().max().item() + 1e-300
    err = (got.double() - want).abs().max().item()
    print(f"{name}: max|d| {err:.3e} = {err / scale:.3e} x max|ref|")
    assert err <= rel * scale, f"{name}: max|d| {err:.3e} > {rel} x {scale:.3e}"


def _per_image(name, got, want, rel=1e-5):
    """err_n <= rel * max|ref_n| for every image n."""
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
    _close(f"{label} gw", got[2], want[2])
    _close(f"{label} gb", got[3], want[3])


def _pow2(t, k):
    return torch.ldexp(t, torch.tensor(k))


@pytest.mark.parametrize("shape", VS_REF, ids=lambda s: "x".join(map(str, s)))
def test_mixed_forward_backward_vs_restatement(shape):
    """Through the autograd Function (dll.ops.conv3x3) against the float64 restatement."""
    from dll.ops import conv3x3
    x, w, b, gy = _data(shape)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = conv3x3(xd, wd, bd, precision="mixed")
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    want = _plain_ref(shape)
    got = tuple(t.detach().cpu() for t in (y, xd.grad, wd.grad, bd.grad))
    for name, u, v in zip(("y", "gx", "gw", "gb"), got, want):
        assert u.dtype == torch.float32
        _close(name, u, v)
    if shape[0] == 3:
        _per_image("y", got[0], want[0])
        _per_image("gx", got[1], want[1])


@pytest.mark.parametrize("shape", [(3, 64, 56, 56, 64), (1, 5, 9, 11, 7)], ids=["hm64to64", "generic1"])
def test_mixed_within_the_bf16_cap_of_unrounded_float64(shape):
    """|native - exact| <= (2^-8 + 2^-18) (|a| (*) |b|) + 1e-5 max|ref| elementwise,
    and the rounding is there at all (a path on unrounded operands would agree
    with the exact convolution to ~1e-7)."""
    x, w, b, gy = _data(shape)
    got = _native_all(x, w, b, gy)
    exact, caps = exact_all(x, w, b, gy)
    for name, u, v, cap in zip(("y", "gx", "gw"), got, exact, caps):
        d = (u.double() - v).abs()
        bar = CAP * cap + 1e-5 * v.abs().max()
        print(f"{name}: max|native - exact| {d.max().item():.3e} ({d.max().item() / v.abs().max().item():.3e} x max|ref|), "
              f"worst d / bar {(d / bar).max().item():.4f}")
        assert (d <= bar).all(), f"{name}: {(d / bar).max().item():.4f} x the cap"
        assert d.max() > 1e-4 * v.abs().max(), f"{name}: operands were not rounded to bf16"


@pytest.mark.parametrize("a,b", [(7, -3), (-20, 9)])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_scaling_law(shape, a, b):
    """bf16 rounding commutes with powers of two: moving 2^a and 2^b onto the
    operands moves 2^(a+b) onto the result, bit for bit (a hidden f16 conversion
    or a value-dependent scale breaks the equality)."""
    x, w, bias, gy = _data(shape)
    y0, gx0, gw0, gb0 = _native_all(x, w, bias, gy)
    y1, _, _, _ = _native_all(_pow2(x, a), _pow2(w, b), _pow2(bias, a + b), gy)
    assert torch.equal(y1, _pow2(y0, a + b)), "y"
    _, gx1, _, _ = _native_all(x, _pow2(w, b), bias, _pow2(gy, a))
    assert torch.equal(gx1, _pow2(gx0, a + b)), "gx"
    _, _, gw1, gb1 = _native_all(_pow2(x, a), w, bias, _pow2(gy, b))
    assert torch.equal(gw1, _pow2(gw0, a + b)), "gw"
    assert torch.equal(gb1, _pow2(gb0, b)), "gb"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_magnitudes_in_one_batch(shape):
    """x_n * {2^-20, 1, 2^12} with gy_n * {2^12, 2^-20, 1}, no bias: there are no
    scales in this mode, so every image keeps its own bf16 precision."""
    x, w, _, gy = _data(shape)
    fx = torch.tensor([2.0 ** -20, 1.0, 2.0 ** 12]).view(3, 1, 1, 1)
    fg = torch.tensor([2.0 ** 12, 2.0 ** -20, 1.0]).view(3, 1, 1, 1)
    _check_all("magnitudes", _native_all(x * fx, w, None, gy * fg), mixed_all(x * fx, w, None, gy * fg))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_tiny_products(shape):
    """Everything * 2^-40, no bias: results ~2^-80, finite, nonzero, within the per-image bar."""
    x, w, _, gy = _data(shape)
    x, w, gy = _pow2(x, -40), _pow2(w, -40), _pow2(gy, -40)
    got, want = _native_all(x, w, None, gy), mixed_all(x, w, None, gy)
    for t in got[:3]:
        assert torch.isfinite(t).all() and t.abs().max() > 0
    _check_all("tiny", got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_zero_image_in_batch(shape):
    """Image 1 all zero in x and in gy: its y is the broadcast bias exactly, its gx zero exactly."""
    x, w, b, gy = _data(shape)
    x, gy = x.clone(), gy.clone()
    x[1] = 0
    gy[1] = 0
    got = _native_all(x, w, b, gy)
    _check_all("zero image", got, mixed_all(x, w, b, gy))
    assert torch.equal(got[0][1], b.view(-1, 1, 1).expand_as(got[0][1]))
    assert torch.count_nonzero(got[1][1]) == 0


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_zero_grad_y(shape):
    x, w, b, gy = _data(shape)
    _, gx, gw, gb = _native_all(x, w, b, torch.zeros_like(gy))
    for name, t in (("gx", gx), ("gw", gw), ("gb", gb)):
        assert torch.isfinite(t).all() and torch.count_nonzero(t) == 0, f"{name} must be exactly zero"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_zero_weights(shape):
    x, w, b, gy = _data(shape)
    got = _native_all(x, torch.zeros_like(w), b, gy)
    assert torch.equal(got[0], b.view(1, -1, 1, 1).expand_as(got[0]))
    assert torch.isfinite(got[1]).all() and torch.count_nonzero(got[1]) == 0
    want = _plain_ref(shape)            # gw and gb do not depend on w
    _close("gw", got[2], want[2])
    _close("gb", got[3], want[3])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_deterministic_partial_grads_and_no_bias(shape):
    """Two calls give bit-identical gradients; gradients requested alone equal
    the joint ones; bias=None works through the Function."""
    from dll import _native
    from dll.ops import conv3x3
    x, w, _, gy = (t.to(DEV) for t in _data(shape))
    a = _native.conv3x3_backward(x, w, gy, precision="mixed")
    b = _native.conv3x3_backward(x, w, gy, precision="mixed")
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    gx, _, _ = _native.conv3x3_backward(x, w, gy, need_w=False, need_b=False, precision="mixed")
    _, gw, _ = _native.conv3x3_backward(x, w, gy, need_x=False, need_b=False, precision="mixed")
    _, _, gb = _native.conv3x3_backward(x, w, gy, need_x=False, need_w=False, precision="mixed")
    assert torch.equal(gx, a[0]) and torch.equal(gw, a[1]) and torch.equal(gb, a[2])
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = conv3x3(xr, wr, None, precision="mixed")
    y.backward(gy)
    assert torch.equal(xr.grad, a[0]) and torch.equal(wr.grad, a[1])
    want = mixed_all(x, w, None, gy)
    _close("y without bias", y.detach().cpu(), want[0])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_bias_gradient_is_the_split_paths(shape):
    """gb sums the unrounded gy on the kernels the split path uses: equal bits,
    computed with gw and alone."""
    from dll import _native
    x, w, b, gy = _data(shape)
    assert torch.equal(_native_all(x, w, b, gy, "mixed")[3], _native_all(x, w, b, gy, "split")[3])
    xd, wd, gyd = x.to(DEV), w.to(DEV), gy.to(DEV)
    alone = [_native.conv3x3_backward(xd, wd, gyd, need_x=False, need_w=False, precision=p)[2] for p in ("mixed", "split")]
    assert torch.equal(alone[0], alone[1])


@pytest.mark.parametrize("shape", [(1, 64, 56, 56, 256), (1, 5, 9, 11, 7)], ids=["hm64to256", "generic1"])
def test_split_is_undisturbed(shape):
    """conv3x3(x, w, b) and conv3x3(x, w, b, precision="split") give equal bits in
    y and all gradients, and they are not the mixed results."""
    from dll.ops import conv3x3
    x, w, b, gy = _data(shape)

    def run(**kw):
        xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
        y = conv3x3(xd, wd, bd, **kw)
        y.backward(gy.to(DEV))
        return [t.detach().cpu() for t in (y, xd.grad, wd.grad, bd.grad)]

    default, split, mixed = run(), run(precision="split"), run(precision="mixed")
    for name, u, v in zip(("y", "gx", "gw", "gb"), default, split):
        assert torch.equal(u, v), name
    for name, u, v in zip(("y", "gx", "gw"), split, mixed):
        assert not torch.equal(u, v), f"{name}: mixed equals split"


def test_native_rejects_unknown_precision():
    from dll import _native
    lib = _native.load()
    x = torch.zeros(1, 5, 9, 11, device=DEV)
    w = torch.zeros(7, 5, 3, 3, device=DEV)
    y = torch.zeros(1, 7, 9, 11, device=DEV)
    for prec in (_native.KPD_PRECISION_FP32, 7, -1):
        rc = lib.kpd_conv3x3_forward_prec(x.data_ptr(), w.data_ptr(), None, 1, 5, 9, 11, 7, y.data_ptr(), prec, None)
        assert rc == -1   # KPD_EINVAL
        rc = lib.kpd_conv3x3_backward_prec(x.data_ptr(), w.data_ptr(), y.data_ptr(), 1, 5, 9, 11, 7, x.data_ptr(), None,
                                           None, prec, None)
        assert rc == -1   # KPD_EINVAL
    with pytest.raises(ValueError):
        _native.conv3x3_forward(x, w, None, precision="bf16")
