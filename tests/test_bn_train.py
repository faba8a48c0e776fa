"""Train-mode BatchNorm + ReLU + Dropout2d on the device (kpd_bn_train_forward /
kpd_bn_train_backward through dll.ops.bn_relu_dropout2d) against the float64
restatement of its rules (tests/bn_train_ref.py)."""
import pytest
import torch

import bn_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-5   # the project's conv criterion: max|got - ref| <= 1e-5 * max|ref|


def _per_channel(name, got, ref):
    """The criterion per channel, so a quiet channel cannot hide behind a loud
    one; a channel whose reference is all zero must be exactly zero."""
    err = (got.double().cpu() - ref).abs().amax(dim=(0, 2, 3))
    scale = ref.abs().amax(dim=(0, 2, 3))
    worst = float((err / (REL * scale).clamp_min(1e-300)).max())
    print(f"{name}: worst channel at {worst:.3f} of the bound")
    bad = (err > REL * scale).nonzero().flatten().tolist()
    assert not bad, f"{name}: channels {bad[:8]} err {err[bad[:8]].tolist()} scale {scale[bad[:8]].tolist()}"


def _per_tensor(name, got, ref):
    err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{name}: {err:.3e} against {REL * scale:.3e}")
    assert err <= REL * scale, f"{name}: {err:.3e} > {REL * scale:.3e}"


def _run(c, with_drop, relu, running=True):
    """The operator with autograd on the case's inputs: y, gx, ggamma, gbeta, rm, rv."""
    from dll.ops import bn_relu_dropout2d
    x, ga, be = (c[k].to(DEV).requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = (c["rm"].to(DEV), c["rv"].to(DEV)) if running else (None, None)
    drop = c["drop"].to(DEV) if with_drop else None
    y = bn_relu_dropout2d(x, ga, be, rm, rv, momentum=0.1, eps=1e-5, relu=relu, drop=drop)
    y.backward(c["gy"].to(DEV))
    return y.detach(), x.grad, ga.grad, be.grad, rm, rv


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("with_drop", [True, False], ids=["drop", "nodrop"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_restatement(shape, with_drop, relu):
    from dll import _native
    c = R.case(shape)
    drop = c["drop"] if with_drop else None
    y, gx, gg, gb, rm, rv = _run(c, with_drop, relu)
    # the statistics as the C entry saves them, and the native ReLU mask: a forward without drop
    y0, mean, invstd = _native.bn_train_forward(c["x"].to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV), None, 1e-5, 0.1,
                                                None, None, relu)
    mask = (y0 > 0).cpu()
    fw64 = R.forward(c["x"], c["gamma"], c["beta"], drop, 1e-5, relu)
    if relu:   # the native mask against the float64 one (torch's own fp32 batch norm: 6.2e-7 at 2x256x56x56)
        flipped = float((mask.double() != fw64["mask"]).double().mean())
        print(f"mask: {flipped:.3e} of the elements differ from float64")
        assert flipped <= 1e-5
    fw = R.forward(c["x"], c["gamma"], c["beta"], drop, 1e-5, relu, mask=mask if relu else None)
    bw = R.backward(fw, c["gy"], c["gamma"])
    want_rm, want_rv = R.running_update(c["rm"], c["rv"], fw, 0.1)
    _per_channel("y", y, fw["y"])
    _per_channel("gx", gx, bw["gx"])
    _per_tensor("ggamma", gg, bw["ggamma"])
    _per_tensor("gbeta", gb, bw["gbeta"])
    _per_tensor("save_mean", mean, fw["mean"])
    _per_tensor("save_invstd", invstd, fw["invstd"])
    _per_tensor("running_mean", rm, want_rm)
    _per_tensor("running_var", rv, want_rv)


def test_special_channels():
    """One (3, 4, 6, 6) case.  Channel 1 is constant: y == relu(beta) * drop
    exactly and gx is finite.  Channel 2 has beta = -100: y, gx, ggamma and
    gbeta are exactly 0."""
    from dll.ops import bn_relu_dropout2d
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 4, 6, 6, generator=g) * 0.5 + 1.0
    x[:, 1] = 1.7
    gamma = torch.rand(4, generator=g) + 0.5
    beta = torch.tensor([0.2, 0.3, -100.0, -0.1])
    drop = torch.bernoulli(torch.full((3, 4), 0.75), generator=g) / 0.75
    drop[0, 1], drop[1, 1], drop[2, 1] = 0.0, 1.0 / 0.75, 1.0 / 0.75
    xd, ga, be = (t.to(DEV).requires_grad_(True) for t in (x, gamma, beta))
    y = bn_relu_dropout2d(xd, ga, be, None, None, relu=True, drop=drop.to(DEV))
    y.backward(torch.randn(3, 4, 6, 6, generator=g).to(DEV))
    y, gx = y.detach().cpu(), xd.grad.cpu()
    want = torch.relu(beta[1]) * drop[:, 1].view(3, 1, 1).expand(3, 6, 6)
    assert torch.equal(y[:, 1], want)
    assert bool(torch.isfinite(gx).all())
    assert float(y[:, 2].abs().max()) == 0.0 and float(gx[:, 2].abs().max()) == 0.0
    assert float(ga.grad[2]) == 0.0 and float(be.grad[2]) == 0.0


def test_determinism_and_partial_gradients():
    """Two calls on the same inputs are bit-identical; gx requested alone
    equals gx requested with the rest; without running pointers y is
    unchanged."""
    from dll import _native
    c = R.case((1, 64, 56, 56))
    a = _run(c, True, True)
    b = _run(c, True, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(_run(c, True, True, running=False)[0], a[0])
    x, ga, be, drop, gy = (c[k].to(DEV) for k in ("x", "gamma", "beta", "drop", "gy"))
    _, mean, invstd = _native.bn_train_forward(x, ga, be, drop, 1e-5, 0.1, None, None, True)
    gx_all, gg, gb = _native.bn_train_backward(x, gy, ga, be, drop, mean, invstd, True)
    gx_only, n1, n2 = _native.bn_train_backward(x, gy, ga, be, drop, mean, invstd, True, need_gamma=False,
                                                need_beta=False)
    assert n1 is None and n2 is None
    assert torch.equal(gx_only, gx_all) and torch.equal(gx_all, a[1])
    assert torch.equal(gg, a[2]) and torch.equal(gb, a[3])


def test_running_statistics_version_bump_and_no_grad():
    """The native call writes the running statistics through raw pointers;
    the operator bumps their version counters (PlanCache keys on them).  Under
    torch.no_grad() the statistics are still updated."""
    from dll.ops import bn_relu_dropout2d
    c = R.case((3, 5, 7, 9))
    x = c["x"].to(DEV)
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    v0 = (rm._version, rv._version)
    with torch.no_grad():
        y = bn_relu_dropout2d(x, c["gamma"].to(DEV), c["beta"].to(DEV), rm, rv)
    assert rm._version > v0[0] and rv._version > v0[1]
    assert not y.requires_grad
    fw = R.forward(c["x"], c["gamma"], c["beta"], None)
    want_rm, want_rv = R.running_update(c["rm"], c["rv"], fw, 0.1)
    _per_tensor("running_mean", rm, want_rm)
    _per_tensor("running_var", rv, want_rv)
    assert not torch.equal(rm.cpu(), c["rm"])
