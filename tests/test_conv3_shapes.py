"""The 3x3 convolution's forward, dgrad, wgrad and bias gradient
(keypoint-detection_amd/csrc/conv3_grad.hip, precisions "split" and "mixed") at the shapes where its
kernels change path or meet an edge (tests/conv3_shapes_cases.py names each):
the wgrad tile choice at C, O = 127 .. 129 and 257, grids of several tiles,
padded channel rows, maps 1 and 2 pixels wide or high, every class of W + 2
mod 4, padded planes that fill the 32-position K-step exactly, the generic
GEMM's tile edges and the near misses of the 56 x 56 fast path.

References: "split" against torch's conv2d with autograd in float64; "mixed"
against tests/conv3_mixed_ref.py.  The bar is the one of test_conv3_grad.py and
test_conv3_mixed.py: max|got - ref| <= 1e-5 max|ref| for gw and gb, and the
same per image for y and gx.

The placement tests are exact: one 1.0 in x and one in gy leave one 1.0 in gw
at the tap that joins them (or nothing); a one-hot x against dyadic weights
leaves those weights in y, a one-hot gy leaves them in gx.  A transposed tap,
a border that leaks and a read of the guard all change a value there."""
import pytest
import torch

import conv3_shapes_cases as K
from conv3_mixed_ref import mixed_all

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REL = 1e-5

_REF = {}


def _native_all(x, w, b, gy, precision):
    from dll import _native
    xd, wd, gyd = x.to(DEV), w.to(DEV), gy.to(DEV)
    y = _native.conv3x3_forward(xd, wd, None if b is None else b.to(DEV), precision=precision)
    gx, gw, gb = _native.conv3x3_backward(xd, wd, gyd, precision=precision)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (y, gx, gw, gb))


def _ref(shape, precision):
    """The reference of a shape's draw, computed once."""
    if (shape, precision) not in _REF:
        _REF[(shape, precision)] = (K.ref_split if precision == "split" else mixed_all)(*K.draw(shape))
    return _REF[(shape, precision)]


def _close(name, got, want):
    assert torch.isfinite(got).all(), f"{name}: not finite"
    err, scale = (got.double() - want).abs().max().item(), want.abs().max().item()
    print(f"{name}: max|d| {err:.3e} against {REL * scale:.3e}")
    assert err <= REL * scale, f"{name}: max|d| {err:.3e} > {REL} x {scale:.3e}"


def _per_image(name, got, want):
    assert torch.isfinite(got).all(), f"{name}: not finite"
    for n in range(want.shape[0]):
        err, scale = (got[n].double() - want[n]).abs().max().item(), want[n].abs().max().item()
        print(f"{name}[{n}]: max|d| {err:.3e} against {REL * scale:.3e}")
        assert err <= REL * scale, f"{name}, image {n}: max|d| {err:.3e} > {REL} x {scale:.3e}"


@pytest.mark.parametrize("precision", K.PRECISIONS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_shape_edges(shape, precision):
    got = _native_all(*K.draw(shape), precision)
    want = _ref(shape, precision)
    _per_image("y", got[0], want[0])
    _per_image("gx", got[1], want[1])
    _close("gw", got[2], want[2])
    _close("gb", got[3], want[3])


# ---------------------------------------------------------------- exact placements
def _channels(k, n):
    """A channel for the k-th placement: the last, the first, then a stride through the rest."""
    return (n - 1, 0)[k] if k < 2 else (k * 37) % n


@pytest.mark.parametrize("precision", K.PRECISIONS)
@pytest.mark.parametrize("shape", K.PLACEMENT_SHAPES, ids=K.shape_id)
def test_wgrad_places_one_tap(shape, precision):
    from dll import _native
    N, C, H, W, O = shape
    w = torch.zeros(O, C, 3, 3, device=DEV)
    k = 0
    for (y, x) in K.placements(H, W):
        for (yy, xx) in K.neighbours(H, W, y, x):
            xi, gi = (k % N, _channels(k, C), y, x), (k % N, _channels(k + 1, O), yy, xx)
            k += 1
            _, gw, gb = _native.conv3x3_backward(K.onehot((N, C, H, W), xi, DEV), w, K.onehot((N, O, H, W), gi, DEV),
                                                 need_x=False, precision=precision)
            assert torch.equal(gw.cpu(), K.expect_wgrad(shape, xi, gi)), f"x at {xi}, gy at {gi}"
            assert torch.equal(gb.cpu(), K.onehot((O,), gi[1])), f"gb, gy at {gi}"
    if N > 1:   # the two pixels in different images: nothing
        xi, gi = (0, C - 1, H - 1, W - 1), (1, O - 1, H - 1, W - 1)
        _, gw, _ = _native.conv3x3_backward(K.onehot((N, C, H, W), xi, DEV), w, K.onehot((N, O, H, W), gi, DEV),
                                            need_x=False, precision=precision)
        assert torch.count_nonzero(gw) == 0


@pytest.mark.parametrize("precision", K.PRECISIONS)
@pytest.mark.parametrize("shape", K.PLACEMENT_SHAPES, ids=K.shape_id)
def test_forward_places_the_weights(shape, precision):
    from dll import _native
    N, C, H, W, O = shape
    w, b = K.dyadic_weights(shape)
    wd, bd = w.to(DEV), b.to(DEV)
    for k, (y, x) in enumerate(K.placements(H, W)):
        xi = (k % N, _channels(k, C), y, x)
        got = _native.conv3x3_forward(K.onehot((N, C, H, W), xi, DEV), wd, bd, precision=precision)
        assert torch.equal(got.cpu(), K.expect_forward(shape, xi, w, b)), f"x at {xi}"


@pytest.mark.parametrize("precision", K.PRECISIONS)
@pytest.mark.parametrize("shape", K.PLACEMENT_SHAPES, ids=K.shape_id)
def test_dgrad_places_the_weights(shape, precision):
    from dll import _native
    N, C, H, W, O = shape
    w, _ = K.dyadic_weights(shape)
    wd, x0 = w.to(DEV), torch.zeros(N, C, H, W, device=DEV)
    for k, (y, x) in enumerate(K.placements(H, W)):
        gi = (k % N, _channels(k, O), y, x)
        gx, _, _ = _native.conv3x3_backward(x0, wd, K.onehot((N, O, H, W), gi, DEV), need_w=False, need_b=False,
                                            precision=precision)
        assert torch.equal(gx.cpu(), K.expect_dgrad(shape, gi, w)), f"gy at {gi}"


# ---------------------------------------------------------------- several tiles: determinism, gradients alone
@pytest.mark.parametrize("precision", K.PRECISIONS)
def test_multi_tile_deterministic_and_partial_grads(precision):
    from dll import _native
    x, w, _, gy = (t.to(DEV) for t in K.draw(K.MULTI_TILE))
    a = _native.conv3x3_backward(x, w, gy, precision=precision)
    b = _native.conv3x3_backward(x, w, gy, precision=precision)
    for name, u, v in zip(("gx", "gw", "gb"), a, b):
        assert torch.equal(u, v), f"{name} differs between two calls"
    gx, n1, n2 = _native.conv3x3_backward(x, w, gy, need_w=False, need_b=False, precision=precision)
    assert n1 is None and n2 is None and torch.equal(gx, a[0])
    _, gw, n2 = _native.conv3x3_backward(x, w, gy, need_x=False, need_b=False, precision=precision)
    assert n2 is None and torch.equal(gw, a[1])
    _, _, gb = _native.conv3x3_backward(x, w, gy, need_x=False, need_w=False, precision=precision)
    assert torch.equal(gb, a[2])
    want = _ref(K.MULTI_TILE, precision)
    _close("gw", a[1].cpu(), want[2])
