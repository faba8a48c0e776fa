"""HeatmapHead (reference: dll/models/heatmap_head.py:20-151) and the heatmap
decoders (:265-413).

Same submodule names as the reference -- ``channel_attention.fc.{0,2}``,
``spatial_attention.conv``, ``deconv_layers.{0,1,4,5}``,
``final_layer.{0,1,3}`` -- so state dicts load unchanged.  ``forward`` runs
the native HIP path on the input's device (csrc/: the attention kernels, the
three 3x3 convs on MFMA and the fused final 1x1 + sigmoid, kpd_heatmap_head):
the module packs its own weights into a plan under the model's
``heatmap_head.`` prefix.  The decoders are device kernels
(kpd_decode_heatmaps).  There is no CPU fallback: CPU inputs raise.

In train mode (``head.train()``) the forward is composed of differentiable
pieces instead of the plan: the two attention blocks in torch ops, every 3x3
convolution through ``dll.ops.conv3x3`` and every BatchNorm2d + ReLU +
Dropout2d through ``dll.ops.bn_relu_dropout2d`` (batch statistics, running
statistics updated; both native forward and backward), the final 1x1
convolution and the sigmoid in torch ops.  ``loss.backward()`` and an
optimiser step then work on the head, and ``eval()`` afterwards serves the
updated weights and running statistics through the plan.
``train_precision`` chooses the arithmetic of the train path's three 3x3
convolutions: "split" (fp32-accurate, the default) or "mixed" (bf16-rounded
operands, fp32 accumulation: DESIGN.md §3i; ``Trainer(use_amp=True)`` sets
it).  It does not touch the eval path, the plan or ``precision``.
"""
import ctypes
import weakref
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native
from ..ops import bn_relu_dropout2d, conv3x3
from ..configs.model_config import HeatmapHeadConfig


class ChannelAttention(nn.Module):
    """sigmoid(fc(avgpool) + fc(maxpool)), returned as [B, C, 1, 1] (reference :115-136).
    Runs through the owning HeatmapHead's native plan."""

    def __init__(self, in_channels: int, reduction_ratio: int = 16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.fc = nn.Sequential(nn.Linear(in_channels, in_channels // reduction_ratio), nn.ReLU(inplace=True),
                                nn.Linear(in_channels // reduction_ratio, in_channels))
        self._owner = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:   # torch ops with autograd (the train path of HeatmapHead)
            cw = torch.sigmoid(self.fc(self.avg_pool(x).flatten(1)) + self.fc(self.max_pool(x).flatten(1)))
            return cw.view(x.size(0), -1, 1, 1)
        head = _owner(self)
        _, cw, _ = head._plan(x.device).heatmap_head(x, _native.HEAD_CHANNEL_ATT)
        return cw.view(x.size(0), -1, 1, 1)


class SpatialAttention(nn.Module):
    """sigmoid(conv7x7([mean_c, max_c])) as [B, 1, H, W] (reference :138-151)."""

    def __init__(self, kernel_size: int = 7):
        super().__init__()
        self.conv = nn.Conv2d(2, 1, kernel_size=kernel_size, padding=kernel_size // 2)
        self._owner = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:   # torch ops with autograd (the train path of HeatmapHead)
            pooled = torch.cat([x.mean(dim=1, keepdim=True), x.max(dim=1, keepdim=True)[0]], dim=1)
            # the 7x7 conv as unfold + matmul: the framework's own convolution backward is not
            # bit-reproducible from run to run on the device, a matmul's is
            k, pad = self.conv.kernel_size, self.conv.padding
            cols = F.unfold(pooled, k, padding=pad)                          # [B, 2 * k * k, H * W]
            pre = torch.matmul(self.conv.weight.view(1, -1), cols) + self.conv.bias.view(1, 1, 1)
            return torch.sigmoid(pre).view(x.size(0), 1, x.size(2), x.size(3))
        head = _owner(self)
        _, _, sw = head._plan(x.device).heatmap_head(x, _native.HEAD_SPATIAL_ATT)
        return sw.unsqueeze(1)


def _owner(m: nn.Module) -> "HeatmapHead":
    head = m._owner() if m._owner is not None else None
    if head is None:
        raise NotImplementedError(f"{type(m).__name__}.forward runs through its HeatmapHead's native plan; "
                                  "use it as a HeatmapHead submodule (or call HeatmapHead.forward)")
    return head


class HeatmapHead(nn.Module):
    precision = "split"   # "fp32" | "split" (fp32-accurate) | "mixed" (bf16 convs); the model sets its own
    train_precision = "split"   # the train path's conv3x3 precision: "split" | "mixed" (bf16 operands, §3i)

    def __init__(self, config: HeatmapHeadConfig):
        super().__init__()
        self.config = config
        if config.use_attention:
            self.channel_attention = ChannelAttention(config.in_channels)
            self.spatial_attention = SpatialAttention()
            self.channel_attention._owner = weakref.ref(self)
            self.spatial_attention._owner = weakref.ref(self)
        layers = []
        for i in range(config.num_deconv_layers):
            cin = config.in_channels if i == 0 else config.deconv_channels[i - 1]
            layers += [nn.Conv2d(cin, config.deconv_channels[i], 3, 1, 1), nn.BatchNorm2d(config.deconv_channels[i]),
                       nn.ReLU(inplace=True), nn.Dropout2d(config.dropout_rate)]
        self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Sequential(
            nn.Conv2d(config.deconv_channels[-1], config.hidden_channels, 3, padding=1),
            nn.BatchNorm2d(config.hidden_channels), nn.ReLU(inplace=True),
            nn.Conv2d(config.hidden_channels, config.num_keypoints, 1))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._plans = _native.PlanCache("heatmap_head.")
        # inspection hook of the train path (the analogue of kpd_debug_copy's "tap0".."tap3"): when this
        # is a list, a train-mode forward appends its three post-activation tensors to it, detached
        self.train_taps = None

    def _plan(self, device: torch.device) -> "_native.Plan":
        if self.training:
            raise NotImplementedError("the native plan serves the eval path only (BatchNorm running statistics, "
                                      "no dropout); a train-mode forward does not go through it")
        return self._plans.get(self, device, self.precision)

    def _conv_bn_relu(self, x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, p: float) -> torch.Tensor:
        """conv3x3 -> batch-statistics BN -> ReLU -> Dropout2d(p), as nn.BatchNorm2d
        and nn.Dropout2d behave in train mode; both operators native."""
        x = conv3x3(x, conv.weight, conv.bias, precision=self.train_precision)
        momentum = 0.0 if bn.momentum is None else bn.momentum
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
            if bn.momentum is None:   # cumulative moving average
                momentum = 1.0 / float(bn.num_batches_tracked)
        drop = None
        if p > 0:
            drop = torch.empty(x.size(0), x.size(1), device=x.device)
            drop = drop.bernoulli_(1 - p).div_(1 - p) if p < 1 else drop.zero_()
        x = bn_relu_dropout2d(x, bn.weight, bn.bias, bn.running_mean if bn.track_running_stats else None,
                              bn.running_var if bn.track_running_stats else None, momentum=momentum, eps=bn.eps,
                              relu=True, drop=drop)
        if isinstance(self.train_taps, list):
            self.train_taps.append(x.detach())
        return x

    def _forward_train(self, x: torch.Tensor):
        """The train path, whatever ``precision`` says: the native 3x3
        convolutions of dll.ops.conv3x3 in ``train_precision`` (fp32-accurate
        split products by default, bf16-rounded operands under "mixed"), the
        rest in fp32."""
        _native._require_cuda(x, "x")
        x = x.float()
        att = None
        if self.config.use_attention:
            cw = self.channel_attention(x)
            x = x * cw
            sw = self.spatial_attention(x)
            x = x * sw
            att = (cw, sw)
        mods = list(self.deconv_layers)
        for i in range(0, len(mods), 4):
            x = self._conv_bn_relu(x, mods[i], mods[i + 1], mods[i + 3].p)
        conv, bn, _, last = self.final_layer
        x = self._conv_bn_relu(x, conv, bn, 0.0)
        R, Ch, H, W = x.shape
        w = last.weight.view(last.weight.size(0), Ch)
        heat = torch.matmul(w, x.view(R, Ch, H * W)) + last.bias.view(1, -1, 1)   # the 1x1 conv
        return torch.sigmoid(heat).view(R, -1, H, W), att

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, Optional[Tuple[torch.Tensor, torch.Tensor]]]:
        """x [B, 64, 56, 56] ROI features -> (heatmaps [B, 17, 56, 56] in (0, 1),
        (channel weights [B, 64, 1, 1], spatial weights [B, 1, 56, 56]) or None
        without attention) -- reference :81-113.  In train mode: the same
        tuple from the differentiable train path (module docstring)."""
        if self.training:
            return self._forward_train(x)
        parts = _native.HEAD_ALL if self.config.use_attention else _native.HEAD_CONVS
        heat, cw, sw = self._plan(x.device).heatmap_head(x, parts)
        att = (cw.view(x.size(0), -1, 1, 1), sw.unsqueeze(1)) if self.config.use_attention else None
        return heat, att


def _ensure_batch(heatmaps: torch.Tensor) -> Tuple[torch.Tensor, bool]:
    if heatmaps.dim() == 3:
        return heatmaps.unsqueeze(0), True
    return heatmaps, False


def _remove_batch(t: torch.Tensor, was_3d: bool) -> torch.Tensor:
    return t.squeeze(0) if was_3d else t


def decode_heatmaps(heatmaps: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Argmax decode (reference :265-296): normalised (x, y) of each map's
    maximum (first index on ties, as torch.max) and the maximum as the score.
    [B,K,H,W] -> ([B,K,2], [B,K]); a [K,H,W] input drops the batch dim."""
    h, was_3d = _ensure_batch(heatmaps)
    kp, sc, _ = _native.decode_heatmaps(h, _native.DECODE_ARGMAX)
    return _remove_batch(kp, was_3d), _remove_batch(sc, was_3d)


def decode_heatmaps_subpixel(heatmaps: torch.Tensor, window_size: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mass-weighted mean over the window around each maximum (reference
    :298-370); the window's maximum as the score, zeros where the window's
    mass is not positive.  Keeps the reference's shape quirk: a [K,H,W] input
    returns [1,K,2] / [1,K] (its batch-dim removal never triggers)."""
    h = heatmaps.unsqueeze(0) if heatmaps.dim() == 3 else heatmaps
    kp, sc, _ = _native.decode_heatmaps(h, _native.DECODE_SUBPIXEL, float(window_size))
    return kp, sc


def decode_heatmaps_soft_argmax(heatmaps: torch.Tensor, temperature: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Soft-argmax (integral regression) over softmax(h / temperature)
    (reference :372-413); the raw maximum as the score."""
    h, was_3d = _ensure_batch(heatmaps)
    kp, sc, _ = _native.decode_heatmaps(h, _native.DECODE_SOFTARGMAX, float(temperature))
    return _remove_batch(kp, was_3d), _remove_batch(sc, was_3d)


def generate_target_heatmap(keypoints: torch.Tensor, heatmap_size: Tuple[int, int], sigma: float = 3.0) -> torch.Tensor:
    """Gaussian training targets (reference heatmap_head.py:163-224) on the
    device (``kpd_target_heatmaps``).  [B,P,K,2] input is flattened to B*P
    rows of which the reference fills the first B (its loop runs over B);
    [B,K,2] gives one plane set per row.  Returns [B,K,H,W] fp32.  Values
    match the reference within fp32 rounding of the normalised kernel."""
    if keypoints.dim() == 4:
        B, P, K, _ = keypoints.shape
        kp = keypoints.reshape(B * P, K, -1)[:B]
    elif keypoints.dim() == 3:
        B, K, _ = keypoints.shape
        kp = keypoints
    else:
        raise ValueError(f"Unexpected keypoints shape: {keypoints.shape}")
    _native._require_cuda(keypoints, "keypoints")
    H, W = int(heatmap_size[0]), int(heatmap_size[1])
    kp = kp[..., :2].float().contiguous()
    out = torch.empty(B, K, H, W, device=kp.device, dtype=torch.float32)
    lib = _native.load()
    with torch.cuda.device(kp.device):
        rc = lib.kpd_target_heatmaps(_native._ptr(kp), B * K, H, W, ctypes.c_double(sigma), _native._ptr(out),
                                     _native._stream(kp.device))
    _native.check(rc, "kpd_target_heatmaps")
    return out


def generate_roi_targets(keypoints: torch.Tensor, visibilities: torch.Tensor, boxes: torch.Tensor, rows=None,
                         heatmap_size: Tuple[int, int] = (56, 56), sigma: float = 2.0):
    """Per-ROI training targets of the top-down head (``kpd_roi_targets``,
    DESIGN.md §3h): keypoints [B,P,K,2] image-normalised, visibilities
    [B,P,K], boxes [B,P,4] cxcywh -> (heat [n,K,H,W], weight [n,K]) for the
    ROIs ``rows`` (indices into B*P; None = all, in order).  Each person's own
    joints are placed in that person's box by the decoders' convention (pixel
    i is i/(W-1) of the unclamped box) as a Gaussian of peak 1 at the
    sub-pixel centre; a joint that is unlabelled, outside its box, NaN, or in
    an empty box gets weight 0 and a zero plane.  On the device, without a
    host synchronisation."""
    if keypoints.dim() != 4 or keypoints.size(-1) < 2:
        raise ValueError(f"keypoints must be [B, P, K, 2], got {tuple(keypoints.shape)}")
    B, P, K = keypoints.shape[:3]
    if tuple(visibilities.shape) != (B, P, K) or tuple(boxes.shape) != (B, P, 4):
        raise ValueError(f"visibilities must be [{B}, {P}, {K}] and boxes [{B}, {P}, 4], got "
                         f"{tuple(visibilities.shape)} and {tuple(boxes.shape)}")
    _native._require_cuda(keypoints, "keypoints")
    return _native.roi_targets(keypoints[..., :2].reshape(B * P, K, 2), visibilities.reshape(B * P, K),
                               boxes.reshape(B * P, 4), rows, int(heatmap_size[0]), int(heatmap_size[1]), float(sigma))


def generate_target_heatmap_adaptive(keypoints: torch.Tensor, heatmap_size: Tuple[int, int],
                                     base_sigma: float = 3.0, adaptive: bool = True) -> torch.Tensor:
    """Reference :226-252: sigma scaled with min(H, W) / 56, floored at 0.8x."""
    sigma = base_sigma * max(0.8, min(heatmap_size) / 56.0) if adaptive else base_sigma
    return generate_target_heatmap(keypoints, heatmap_size, sigma)
