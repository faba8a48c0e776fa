"""float64 restatement of the train-mode BatchNorm2d + ReLU + Dropout2d rules
(include/kpd.h, kpd_bn_train_forward / kpd_bn_train_backward),
written from the formulas.  With n = N * H * W values per channel:

    mean = sum x / n          var = sum (x - mean)^2 / n          invstd = 1 / sqrt(var + eps)
    xhat = (x - mean) * invstd        pre = xhat * gamma + beta
    y    = (relu ? max(pre, 0) : pre) * drop[n][c]
    g    = gy * drop[n][c] * [pre > 0]        gbeta = sum g        ggamma = sum g * xhat
    gx   = gamma * invstd * (g - gbeta / n - xhat * ggamma / n)
    rm  <- (1 - m) rm + m mean        rv <- (1 - m) rv + m var n / (n - 1)

``mask`` forces the ReLU mask [pre > 0] (a [N, C, H, W] bool tensor): a
pre-activation within fp32 rounding of zero may fall on the other side of the
kink in another precision, and the comparison of gradients wants one mask.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch


def _cv(t: Optional[torch.Tensor], C: int, fill: float) -> torch.Tensor:
    v = torch.full((C,), fill, dtype=torch.float64) if t is None else t.detach().double().cpu().reshape(C)
    return v.view(1, C, 1, 1)


def forward(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
            drop: Optional[torch.Tensor], eps: float = 1e-5, relu: bool = True,
            mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    x = x.detach().double().cpu()
    N, C, H, W = x.shape
    n = N * H * W
    mean = x.sum(dim=(0, 2, 3), keepdim=True) / n
    var = ((x - mean) ** 2).sum(dim=(0, 2, 3), keepdim=True) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * invstd
    pre = xhat * _cv(gamma, C, 1.0) + _cv(beta, C, 0.0)
    if not relu:
        m = torch.ones_like(pre)
    elif mask is None:
        m = (pre > 0).double()
    else:
        m = mask.detach().cpu().double()
    d = torch.ones(N, C, 1, 1, dtype=torch.float64) if drop is None else drop.detach().double().cpu().view(N, C, 1, 1)
    return {"y": pre * m * d, "mean": mean.flatten(), "var": var.flatten(), "invstd": invstd.flatten(), "xhat": xhat,
            "mask": m, "drop": d, "n": n}


def backward(fw: Dict[str, torch.Tensor], gy: torch.Tensor, gamma: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
    n, xhat = fw["n"], fw["xhat"]
    C = xhat.shape[1]
    g = gy.detach().double().cpu() * fw["drop"] * fw["mask"]
    gbeta = g.sum(dim=(0, 2, 3), keepdim=True)
    ggamma = (g * xhat).sum(dim=(0, 2, 3), keepdim=True)
    gx = _cv(gamma, C, 1.0) * fw["invstd"].view(1, C, 1, 1) * (g - gbeta / n - xhat * ggamma / n)
    return {"gx": gx, "ggamma": ggamma.flatten(), "gbeta": gbeta.flatten()}


def running_update(rm: torch.Tensor, rv: torch.Tensor, fw: Dict[str, torch.Tensor], momentum: float = 0.1):
    n = fw["n"]
    rm, rv = rm.detach().double().cpu(), rv.detach().double().cpu()
    return (1 - momentum) * rm + momentum * fw["mean"], (1 - momentum) * rv + momentum * fw["var"] * n / (n - 1)


# ---- the cases of the parity tests: (N, C, H, W), shared by the CPU and the GPU file
SHAPES = [(3, 5, 7, 9),        # H*W = 63: one value per access
          (4, 3, 1, 1),        # one pixel per plane, n = 4
          (37, 2, 8, 8),       # uneven image slices
          (1, 64, 56, 56),     # the reference's per-ROI call
          (2, 256, 56, 56),    # the head's wide stage
          (2, 17, 20, 13),     # generic
          (3, 2048, 1, 3),     # more chunks than workgroups of a channel, dealt unevenly (scalar)
          (6, 4096, 2, 2)]     # one workgroup per channel walks six chunks (16-byte accesses)
_CASES: Dict[tuple, Dict[str, torch.Tensor]] = {}


def case(shape) -> Dict[str, torch.Tensor]:
    """Inputs of a shape, drawn once and never modified: a per-channel mean
    offset of up to several standard deviations, a Dropout2d(0.25) multiplier
    with at least one dropped plane."""
    if shape not in _CASES:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(N * 100003 + C * 1009 + H * 31 + W)
        x = torch.randn(N, C, H, W, generator=g) * 0.5 + torch.linspace(-3, 3, C).view(1, C, 1, 1)
        drop = torch.bernoulli(torch.full((N, C), 0.75), generator=g) / 0.75
        drop[0, 0] = 0.0
        _CASES[shape] = {"x": x, "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g) * 0.3,
                         "drop": drop, "gy": torch.randn(N, C, H, W, generator=g),
                         "rm": torch.randn(C, generator=g) * 0.1, "rv": torch.rand(C, generator=g) + 0.5}
    return _CASES[shape]
