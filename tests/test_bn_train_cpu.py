"""Train-mode BatchNorm + ReLU + Dropout2d without a GPU: the float64
restatement (tests/bn_train_ref.py) against torch's float64 autograd, the
argument checks of the two C entries (made before any device work), and the
train-mode error handling of HeatmapHead and its attention submodules."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bn_train_ref as R


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("with_drop", [True, False], ids=["drop", "nodrop"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_matches_torch_fp64(shape, with_drop, relu):
    """y, gx, ggamma, gbeta within 1e-12 and the running statistics within
    1e-15 of F.batch_norm(training=True) -> relu -> mask multiply in float64
    (the two agree to 6e-13 at [2][256][56][56])."""
    c = R.case(shape)
    N, C = shape[:2]
    drop = c["drop"] if with_drop else None
    fw = R.forward(c["x"], c["gamma"], c["beta"], drop, 1e-5, relu)
    bw = R.backward(fw, c["gy"], c["gamma"])
    rm, rv = R.running_update(c["rm"], c["rv"], fw, 0.1)

    x, ga, be = (c[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    trm, trv = c["rm"].double().clone(), c["rv"].double().clone()
    y = F.batch_norm(x, trm, trv, ga, be, True, 0.1, 1e-5)
    if relu:
        y = F.relu(y)
    if with_drop:
        y = y * drop.double().view(N, C, 1, 1)
    y.backward(c["gy"].double())
    for name, got, want in (("y", fw["y"], y.detach()), ("gx", bw["gx"], x.grad), ("ggamma", bw["ggamma"], ga.grad),
                            ("gbeta", bw["gbeta"], be.grad)):
        err = float((got - want).abs().max())
        assert err <= 1e-12, f"{name}: {err:.3e}"
    for name, got, want in (("running_mean", rm, trm), ("running_var", rv, trv)):
        err = float((got - want).abs().max())
        assert err <= 1e-15, f"{name}: {err:.3e}"


def test_forced_mask_is_used():
    c = R.case((3, 5, 7, 9))
    mask = torch.zeros(3, 5, 7, 9, dtype=torch.bool)
    fw = R.forward(c["x"], c["gamma"], c["beta"], None, 1e-5, True, mask=mask)
    assert float(fw["y"].abs().max()) == 0.0
    assert float(R.backward(fw, c["gy"], c["gamma"])["gx"].abs().max()) == 0.0


# ---------------------------------------------------------------- ABI checks
_P = ctypes.c_void_p(4096)   # a non-null pointer; a failed check returns before anything reads it


def _fwd(lib, N=2, C=3, H=4, W=4, x=_P, eps=1e-5, momentum=0.1, rm=_P, rv=_P, y=ctypes.c_void_p(1 << 20)):
    return lib.kpd_bn_train_forward(x, N, C, H, W, _P, _P, None, eps, momentum, rm, rv, 1, y, _P, _P, None)


def _bwd(lib, N=2, C=3, H=4, W=4, x=_P, gy=_P):
    return lib.kpd_bn_train_backward(x, gy, N, C, H, W, _P, _P, None, _P, _P, 1, None, None, None, None)


def test_abi_validation_without_a_device():
    from dll import _native
    lib = _native.load()
    assert _fwd(lib, N=1, H=1, W=1) == -1
    assert b"more than 1 value per channel" in lib.kpd_last_error()
    assert _bwd(lib, N=1, H=1, W=1) == -1
    assert b"more than 1 value per channel" in lib.kpd_last_error()
    assert _fwd(lib, C=0) == -1 and b"C " in lib.kpd_last_error()
    assert _bwd(lib, C=0) == -1 and b"C " in lib.kpd_last_error()
    assert _fwd(lib, N=0) == -1 and _fwd(lib, H=0) == -1 and _fwd(lib, W=-1) == -1
    assert _fwd(lib, eps=0.0) == -1 and b"eps" in lib.kpd_last_error()
    assert _fwd(lib, eps=float("nan")) == -1
    assert _fwd(lib, momentum=1.5) == -1 and b"momentum" in lib.kpd_last_error()
    assert _fwd(lib, momentum=-0.1) == -1
    assert _fwd(lib, rv=None) == -1 and b"running_mean and running_var" in lib.kpd_last_error()
    assert _fwd(lib, rm=None) == -1
    assert _fwd(lib, x=None) == -1 and b"x is null" in lib.kpd_last_error()
    assert _fwd(lib, y=None) == -1 and b"y is null" in lib.kpd_last_error()
    assert _fwd(lib, y=_P) == -1 and b"alias" in lib.kpd_last_error()
    assert _bwd(lib, x=None) == -1 and b"x is null" in lib.kpd_last_error()
    assert _bwd(lib, gy=None) == -1 and b"gy is null" in lib.kpd_last_error()
    # nothing requested: no work, no device
    assert _bwd(lib) == 0


def test_python_operator_rejects_cpu_tensors():
    from dll import _native
    from dll.ops import bn_relu_dropout2d
    with pytest.raises(_native.KpdNativeError, match="HIP device"):
        bn_relu_dropout2d(torch.zeros(2, 3, 4, 4), None, None, None, None)
    with pytest.raises(ValueError, match="drop"):
        bn_relu_dropout2d(torch.zeros(2, 3, 4, 4), None, None, None, None, drop=torch.ones(3, 2))


# ------------------------------------------------- train-mode error handling
def _head():
    from dll.configs.model_config import HeatmapHeadConfig
    from dll.models.heatmap_head import HeatmapHead
    torch.manual_seed(5)
    return HeatmapHead(HeatmapHeadConfig())


def test_train_mode_head_rejects_cpu_input():
    from dll import _native
    head = _head().train()
    with pytest.raises(_native.KpdNativeError, match="HIP device"):
        head(torch.zeros(1, 64, 14, 14))


def test_train_mode_attention_runs_through_torch():
    """ChannelAttention and SpatialAttention in train mode compute through
    torch ops (with autograd) instead of the owning head's plan: on a CPU
    tensor they match the formulas in float64 to 1e-6."""
    head = _head().train()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 64, 10, 12, generator=g)
    ca, sa = head.channel_attention, head.spatial_attention
    with torch.no_grad():   # non-trivial biases
        for p in list(ca.parameters()) + list(sa.parameters()):
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
    xr = x.clone().requires_grad_(True)
    cw = ca(xr)
    sw = sa(xr)
    assert cw.shape == (3, 64, 1, 1) and sw.shape == (3, 1, 10, 12)
    (cw.sum() + sw.sum()).backward()
    assert xr.grad is not None and ca.fc[0].weight.grad is not None and sa.conv.weight.grad is not None

    x64 = x.double()
    w0, b0, w2, b2 = (t.detach().double() for t in (ca.fc[0].weight, ca.fc[0].bias, ca.fc[2].weight, ca.fc[2].bias))

    def fc(v):
        return torch.relu(v @ w0.T + b0) @ w2.T + b2

    cw64 = torch.sigmoid(fc(x64.mean(dim=(2, 3))) + fc(x64.amax(dim=(2, 3))))
    pooled = torch.stack([x64.mean(dim=1), x64.amax(dim=1)], dim=1)
    sw64 = torch.sigmoid(F.conv2d(pooled, sa.conv.weight.detach().double(), sa.conv.bias.detach().double(), padding=3))
    assert float((cw.detach().double().flatten(1) - cw64).abs().max()) <= 1e-6
    assert float((sw.detach().double() - sw64).abs().max()) <= 1e-6
