"""A CPU replica of HeatmapHead's train-mode forward, built from torch ops in a
chosen dtype (float64: the reference of tests/test_head_train.py; float32:
the yardstick of what fp32 arithmetic costs on the same graph).

    cw = sigmoid(fc(mean_hw x) + fc(max_hw x))        x1 = x * cw
    sw = sigmoid(conv7x7([mean_c x1, max_c x1]))      x2 = x1 * sw
    three times: conv3x3 -> batch-statistics BN -> ReLU        (the first two: Dropout2d, rate 0 here)
    heat = sigmoid(conv1x1)

``masks`` forces the three ReLU masks (bool tensors, e.g. ``tap > 0`` of the
native forward's ``train_taps``): a pre-activation within fp32 rounding of
zero may fall on either side of the kink, and one flipped element moves a
weight gradient by about 1e-4 of its magnitude.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

BNS = ("deconv_layers.1", "deconv_layers.5", "final_layer.1")
CONVS = ("deconv_layers.0", "deconv_layers.4", "final_layer.0")


def leaves(sd: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    """The state dict as leaves of ``dtype`` on the CPU: parameters require grad,
    buffers are private copies (the BNs update them)."""
    out = {}
    for k, v in sd.items():
        t = v.detach().cpu().clone()
        if t.is_floating_point():
            t = t.to(dtype)
            if not k.endswith(("running_mean", "running_var")):
                t.requires_grad_(True)
        out[k] = t
    return out


def forward(p: Dict[str, torch.Tensor], x: torch.Tensor, masks: Optional[List[torch.Tensor]] = None,
            momentum: float = 0.1, eps: float = 1e-5):
    """(heat, cw [R,64,1,1], sw [R,1,H,W], own masks); updates the running
    statistics and num_batches_tracked in ``p`` as nn.BatchNorm2d does."""
    dtype = p["final_layer.3.weight"].dtype
    x = x.detach().cpu().to(dtype)

    def fc(v):
        h = torch.relu(F.linear(v, p["channel_attention.fc.0.weight"], p["channel_attention.fc.0.bias"]))
        return F.linear(h, p["channel_attention.fc.2.weight"], p["channel_attention.fc.2.bias"])

    cw = torch.sigmoid(fc(x.mean(dim=(2, 3))) + fc(x.amax(dim=(2, 3))))[:, :, None, None]
    x = x * cw
    pooled = torch.cat([x.mean(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)], dim=1)
    sw = torch.sigmoid(F.conv2d(pooled, p["spatial_attention.conv.weight"], p["spatial_attention.conv.bias"],
                                padding=3))
    x = x * sw
    own = []
    for i, (cv, bn) in enumerate(zip(CONVS, BNS)):
        x = F.conv2d(x, p[cv + ".weight"], p[cv + ".bias"], padding=1)
        pre = F.batch_norm(x, p[bn + ".running_mean"], p[bn + ".running_var"], p[bn + ".weight"], p[bn + ".bias"],
                           True, momentum, eps)
        p[bn + ".num_batches_tracked"] += 1
        own.append(pre.detach() > 0)
        x = pre * (own[i] if masks is None else masks[i].cpu()).to(dtype)
    heat = torch.sigmoid(F.conv2d(x, p["final_layer.3.weight"], p["final_layer.3.bias"]))
    return heat, cw, sw, own


def grads(p: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: v.grad for k, v in p.items() if v.is_floating_point() and v.requires_grad}


def sgd_step(p: Dict[str, torch.Tensor], lr: float) -> None:
    with torch.no_grad():
        for v in p.values():
            if v.is_floating_point() and v.requires_grad:
                v -= lr * v.grad
                v.grad = None
