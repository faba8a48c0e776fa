"""Train-mode BatchNorm + ReLU + Dropout2d
(keypoint-detection_amd/csrc/bn_train.hip) at the edges its parity shapes leave out: tensors that are contiguous but start at an odd
element offset (the 16-byte path's alignment test), H*W around the 1024-value
chunk, the optional arguments, and inputs whose mean lies thousands of standard
deviations from zero.

Reference and bars as tests/test_bn_train.py: the float64 restatement
(tests/bn_train_ref.py) forced to the native ReLU mask; 1e-5 per channel for y
and gx, 1e-5 per tensor for the rest.  Two kinds of case get derived bars for
y, gx and ggamma (tests/bn_train_edges_cases.py: far_bars, cancel_bar,
ggamma_bar): the far means, and E.TWO_VALUES.  In both, the fp32 mean's half
ulp times invstd is no longer small against xhat, so the count of ReLU mask
elements that differ from float64 (<= 1e-5 everywhere else) gives way to a
derived test: an element may differ only where the float64 pre-activation
lies within that uncertainty of zero (E.kink_band)."""
import pytest
import torch

import bn_train_edges_cases as E
import bn_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = E.REL
EPS, MOM = 1e-5, 0.1


def _per_channel(name, got, ref, bar=None):
    err = (got.double().cpu() - ref).abs().amax(dim=(0, 2, 3))
    bar = REL * ref.abs().amax(dim=(0, 2, 3)) if bar is None else bar
    print(f"{name}: worst channel at {float((err / bar.clamp_min(1e-300)).max()):.3f} of the bound")
    bad = (err > bar).nonzero().flatten().tolist()
    assert not bad, f"{name}: channels {bad[:8]} err {err[bad[:8]].tolist()} bar {bar[bad[:8]].tolist()}"


def _per_tensor(name, got, ref):
    err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{name}: {err:.3e} against {REL * scale:.3e}")
    assert err <= REL * scale, f"{name}: {err:.3e} > {REL * scale:.3e}"


def _offset(t):
    """t's values in a tensor of t's shape that is contiguous but starts one
    element (4 bytes) into its buffer: never 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _native(c, with_drop=True, relu=True, gamma=True, beta=True, momentum=MOM, x=None, gy=None, stats=None):
    """The two C entries on the case's tensors (x, gy: device tensors to use
    instead; stats: (mean, invstd) for the backward instead of the forward's).
    Returns y, save_mean, save_invstd, gx, ggamma, gbeta, running_mean, running_var."""
    from dll import _native
    xd = c["x"].to(DEV) if x is None else x
    gyd = c["gy"].to(DEV) if gy is None else gy
    ga = c["gamma"].to(DEV) if gamma else None
    be = c["beta"].to(DEV) if beta else None
    drop = c["drop"].to(DEV) if with_drop else None
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    y, mean, invstd = _native.bn_train_forward(xd, ga, be, drop, EPS, momentum, rm, rv, relu)
    m, s = (mean, invstd) if stats is None else stats
    gx, gg, gb = _native.bn_train_backward(xd, gyd, ga, be, drop, m, s, relu)
    torch.cuda.synchronize()
    return y, mean, invstd, gx, gg, gb, rm, rv


def _reference(c, with_drop=True, relu=True, gamma=True, beta=True, momentum=MOM, check_mask=True):
    """The restatement on the native ReLU mask (a forward without drop), as
    test_parity_with_the_restatement forces it."""
    from dll import _native
    ga, be = (c["gamma"] if gamma else None), (c["beta"] if beta else None)
    drop = c["drop"] if with_drop else None
    y0, _, _ = _native.bn_train_forward(c["x"].to(DEV), None if ga is None else ga.to(DEV),
                                        None if be is None else be.to(DEV), None, EPS, momentum, None, None, relu)
    mask = (y0 > 0).cpu()
    if relu:
        fw64 = R.forward(c["x"], ga, be, drop, EPS, relu)
        differs = mask.double() != fw64["mask"]
        print(f"mask: {float(differs.double().mean()):.3e} of the elements differ from float64")
        if check_mask:
            assert float(differs.double().mean()) <= 1e-5
        else:   # only inside the band around the kink that the fp32 mean and xhat leave uncertain
            pre64, band = E.kink_band(fw64, ga, be)
            assert bool((pre64.abs() <= band)[differs].all()), "a ReLU mask element differs outside the fp32 uncertainty"
    fw = R.forward(c["x"], ga, be, drop, EPS, relu, mask=mask if relu else None)
    bw = R.backward(fw, c["gy"], ga)
    rm, rv = R.running_update(c["rm"], c["rv"], fw, momentum)
    return fw, bw, rm, rv


def _check(got, fw, bw, rm, rv, bars=None):
    """bars: per-channel (y, gx, ggamma) bars in place of the 1e-5 ones."""
    y, mean, invstd, gx, gg, gb, grm, grv = got
    _per_channel("y", y, fw["y"], bars and bars[0])
    _per_channel("gx", gx, bw["gx"], bars and bars[1])
    if bars:
        gg_err = (gg.double().cpu() - bw["ggamma"]).abs()
        print(f"ggamma: worst channel at {float((gg_err / bars[2]).max()):.3f} of the bound")
        assert bool((gg_err <= bars[2]).all()), f"ggamma: worst {float((gg_err / bars[2]).max()):.3f} of the bound"
    else:
        _per_tensor("ggamma", gg, bw["ggamma"])
    _per_tensor("gbeta", gb, bw["gbeta"])
    _per_tensor("save_mean", mean, fw["mean"])
    _per_tensor("save_invstd", invstd, fw["invstd"])
    _per_tensor("running_mean", grm, rm)
    _per_tensor("running_var", grv, rv)


# ---------------------------------------------------------------- offset views
@pytest.mark.parametrize("which", ["x", "gy", "both"])
@pytest.mark.parametrize("shape", E.OFFSET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_offset_views_take_the_one_value_path(shape, which):
    """H*W % 4 == 0, so the aligned call runs on 16-byte accesses and the
    offset one on single values.  Both meet the bar; the statistics, y, gx and
    the parameter gradients are also bit-identical: both paths cut the sums
    into the same (image, chunk) runs and add them in double."""
    c = R.case(shape)
    assert shape[2] * shape[3] % 4 == 0
    aligned = _native(c)
    assert c["x"].to(DEV).data_ptr() % 16 == 0
    xo = _offset(c["x"].to(DEV)) if which in ("x", "both") else None
    gyo = _offset(c["gy"].to(DEV)) if which in ("gy", "both") else None
    # the backward of the offset case on offset copies of the first call's statistics as well
    stats = (_offset(aligned[1]), _offset(aligned[2])) if which == "both" else None
    got = _native(c, x=xo, gy=gyo, stats=stats)
    _check(got, *_reference(c))
    for name, u, v in zip(("y", "save_mean", "save_invstd", "gx", "ggamma", "gbeta", "running_mean", "running_var"),
                          got, aligned):
        assert torch.equal(u, v), f"{name}: the offset call's bits differ from the aligned call's"


# ---------------------------------------------------------------- the chunk boundary
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape", E.CHUNK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chunk_boundary(shape, relu):
    """E.TWO_VALUES has two values per channel: the three terms of gx cancel
    there, and y, gx and ggamma are held to the fp32 evaluation's own bounds
    (bn_train_edges_cases.py: far_bars, cancel_bar, ggamma_bar;
    tests/test_train_edges_cpu.py shows that the 1e-5 bar of each of the three
    is out of reach of any fp32 evaluation at that shape).  The statistics and
    gbeta keep the 1e-5 bar; the mask is checked by E.kink_band."""
    c = R.case(shape)
    if shape != E.TWO_VALUES:
        return _check(_native(c, relu=relu), *_reference(c, relu=relu))
    fw, bw, rm, rv = _reference(c, relu=relu, check_mask=False)
    g = E.masked_gy(fw, c["gy"])
    bar_y, bar_gx = E.far_bars(fw, bw, c["gamma"], g)
    _check(_native(c, relu=relu), fw, bw, rm, rv, (bar_y, bar_gx + E.cancel_bar(fw, bw, c["gamma"], g), E.ggamma_bar(fw, bw)))


# ---------------------------------------------------------------- optional arguments
@pytest.mark.parametrize("gamma,beta", [(False, False), (True, False), (False, True)], ids=["none", "gamma", "beta"])
def test_without_gamma_or_beta(gamma, beta):
    c = R.case((3, 5, 7, 9))
    got = _native(c, gamma=gamma, beta=beta)
    fw, bw, rm, rv = _reference(c, gamma=gamma, beta=beta)
    _check(got, fw, bw, rm, rv)


def test_momentum_zero_leaves_the_running_statistics():
    c = R.case((3, 5, 7, 9))
    got = _native(c, momentum=0.0)
    assert torch.equal(got[6].cpu(), c["rm"]) and torch.equal(got[7].cpu(), c["rv"])
    _check(got, *_reference(c, momentum=0.0))


def test_momentum_one_replaces_the_running_statistics():
    c = R.case((3, 5, 7, 9))
    got = _native(c, momentum=1.0)
    fw, bw, rm, rv = _reference(c, momentum=1.0)
    n = fw["n"]
    assert torch.equal(rm, fw["mean"]) and torch.allclose(rv, fw["var"] * n / (n - 1), rtol=1e-15, atol=0)
    _check(got, fw, bw, rm, rv)


# ---------------------------------------------------------------- far mean
@pytest.mark.parametrize("mean,std", E.FAR_MEANS, ids=["1024+0.5", "-4096+2"])
def test_mean_far_from_zero(mean, std):
    """|mean| / std of 2048: a float32 sum x^2 / n - mean^2 has no correct digit
    left there (tests/test_train_edges_cpu.py shows it failing this bar)."""
    c = E.far_case(mean, std)
    fw, bw, rm, rv = _reference(c, check_mask=False)
    g = E.masked_gy(fw, c["gy"])
    bar_y, bar_gx = E.far_bars(fw, bw, c["gamma"], g)
    _check(_native(c), fw, bw, rm, rv, (bar_y, bar_gx, E.ggamma_bar(fw, bw)))
