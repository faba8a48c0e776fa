"""CPU restatement of ``dll.ops.conv3x3(..., precision="mixed")`` (DESIGN.md
§3i), shared by the mixed-precision tests.

The rule: every product of the forward, the dgrad and the wgrad is the product
of its two operands *each rounded to bf16 (nearest even) from its own fp32
value*, accumulated without further rounding of the operands; the bias is added
unrounded and the bias gradient sums the unrounded gy.

    y  = sum bf16(w) * bf16(x) + b
    gx = sum bf16(w) * bf16(gy)
    gw = sum bf16(gy) * bf16(x)
    gb = sum gy

``conv3x3_mixed`` is a torch.autograd.Function in the dtype of its inputs.  The
rounding goes through float32 whatever that dtype is, so a float64 run sees the
same rounded operands as the device (whose tensors are fp32) and differs from
it by the accumulation order alone: a product of two bf16 values is exact in
fp32.  Deliberately not ``torch.autocast``: nothing but these products is
rounded.
"""
import torch
import torch.nn.functional as F
from torch.nn import grad as nn_grad


def bf16(t: torch.Tensor) -> torch.Tensor:
    """t rounded to bf16 from its fp32 value, in t's dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype)


class Conv3x3Mixed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.conv2d(bf16(x), bf16(w), b, padding=1)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        g = bf16(gy)
        gx = nn_grad.conv2d_input(x.shape, bf16(w), g, padding=1)
        gw = nn_grad.conv2d_weight(bf16(x), w.shape, g, padding=1)
        gb = gy.sum(dim=(0, 2, 3)) if ctx.has_bias else None
        return gx, gw, gb


def conv3x3_mixed(x, w, b=None):
    return Conv3x3Mixed.apply(x, w, b)


def mixed_all(x, w, b, gy, dtype=torch.float64):
    """(y, gx, gw, gb) of the restatement on ``dtype`` copies of fp32 tensors
    (b may be None: gb is then the plain sum of gy, as the device returns it)."""
    xr, wr = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (x, w))
    br = None if b is None else b.detach().cpu().to(dtype).requires_grad_(True)
    g = gy.detach().cpu().to(dtype)
    y = conv3x3_mixed(xr, wr, br)
    y.backward(g)
    gb = br.grad if br is not None else g.sum(dim=(0, 2, 3))
    return y.detach(), xr.grad, wr.grad, gb


def exact_all(x, w, b, gy):
    """(y, gx, gw) of the unrounded convolution in float64, and the elementwise
    caps (|w| (*) |x|, |w| (*) |gy|, |gy| (*) |x|): the same three convolutions
    of the absolute values."""
    def run(xx, ww, bb, gg):
        xr, wr = (t.detach().cpu().double().requires_grad_(True) for t in (xx, ww))
        y = F.conv2d(xr, wr, None if bb is None else bb.detach().cpu().double(), padding=1)
        y.backward(gg.detach().cpu().double())
        return y.detach(), xr.grad, wr.grad
    return run(x, w, b, gy), run(x.abs(), w.abs(), None, gy.abs())


# |bf16(a) bf16(b) - a b| <= ((1 + 2^-9)^2 - 1) |a b| = (2^-8 + 2^-18) |a b|: a
# bf16 rounding (8 significand bits, nearest) moves a value by at most 2^-9 of itself
CAP = 2.0 ** -8 + 2.0 ** -18


# ---------------------------------------------------------------- the head replica on the restatement
class _MixedFunctional:
    """torch.nn.functional with the 3x3 / padding-1 convolution replaced by the
    restatement: what tests/head_train_ref.py's forward sees as ``F`` inside
    ``head_forward_mixed``.  The 7x7 attention convolution and the final 1x1
    stay plain, as they do on the device."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def conv2d(x, w, b=None, padding=0):
        if tuple(w.shape[2:]) == (3, 3) and padding == 1:
            return conv3x3_mixed(x, w, b)
        return F.conv2d(x, w, b, padding=padding)


def head_forward_mixed(p, x, masks=None, momentum=0.1, eps=1e-5):
    """head_train_ref.forward with the head's three 3x3 convolutions on the
    restatement (HeatmapHead.train_precision = "mixed"); same arguments and returns."""
    import head_train_ref as HR
    plain = HR.F
    HR.F = _MixedFunctional()
    try:
        return HR.forward(p, x, masks, momentum, eps)
    finally:
        HR.F = plain
