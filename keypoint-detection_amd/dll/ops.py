"""Training-side operator (the backward of K6): the
HeatmapHead's 3x3 convolution -- nn.Conv2d(C, O, 3, padding=1), reference
dll/models/heatmap_head.py:31-45,55-66 -- as an autograd Function whose
forward and backward both run native (libkpd: kpd_conv3x3_forward /
kpd_conv3x3_backward: fp32-accurate split f16 hi / lo MFMA products with fp32
accumulation for the forward and dgrad at 56 x 56 with 64 | 256 channels and
for every wgrad, exact fp32 products on the generic fallback; deterministic
sums).  With ``precision="mixed"`` the same three run on bf16-rounded
operands, one v_mfma_f32_16x16x32_bf16 product per MAC with fp32 accumulation
and no scale passes (kpd_conv3x3_*_prec): the arithmetic of
``Trainer(use_amp=True)``; tensors, parameters and gradients stay fp32.  The
reference gets these gradients from autograd in Trainer.train
(dll/training/trainer.py:263,272).

    from dll.ops import conv3x3
    y = conv3x3(x, conv.weight, conv.bias)     # == F.conv2d(x, w, b, padding=1)

and the train-mode BatchNorm2d + ReLU + Dropout2d that follows each of them
(libkpd: kpd_bn_train_forward / kpd_bn_train_backward):

    from dll.ops import bn_relu_dropout2d
    y = bn_relu_dropout2d(x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                          momentum=bn.momentum, eps=bn.eps, drop=mask)
    # == F.relu(F.batch_norm(x, rm, rv, w, b, True, momentum, eps)) * mask[:, :, None, None]

and the person detector's training loss on the pooled trunk features (libkpd:
kpd_detector_targets + kpd_detector_loss): anchor matching,
focal + smooth-L1 loss and the closed-form gradients of box_heads[0] /
cls_heads[0] in one fused pass:

    from dll.ops import detector_loss
    loss = detector_loss(plan.detector_features(image), box.weight, box.bias, cls.weight, cls.bias,
                         person_head.anchors, gt_boxes, (H, W))
    loss.backward()            # loss.cls_part / loss.box_part: the two parts, detached

and the coordinate term on the decoded keypoints (libkpd: kpd_coord_loss /
kpd_softargmax_backward): the soft-argmax decode as a
differentiable op, and SpatialCoordinateLoss of it with the gradient onto the
heatmaps in the same pass:

    from dll.ops import soft_argmax, soft_argmax_coord_loss
    coords = soft_argmax(heat, temperature=1.0)                  # == decode_heatmaps_soft_argmax(heat)[0]
    loss, coords = soft_argmax_coord_loss(heat, gt_coords, visibility)

and the ROI align between FPN level 0 and the heatmap head as a differentiable
op (libkpd: kpd_roi_align forward, kpd_roi_align_backward, DESIGN.md §3l: a
deterministic gather, no floating-point atomics), which is what lets
``Trainer(train_neck=True)`` train the FPN's level-0 path under the head:

    from dll.ops import roi_align_boxes
    x = roi_align_boxes(level0, boxes, rows, topk)   # [n, Cs, 56, 56]; gradient to level0 only
"""
from __future__ import annotations

from typing import Optional

import torch

from torch.autograd.function import once_differentiable

from . import _native


class Conv3x3Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], precision: str = "split"):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.bias_dtype = bias.dtype if bias is not None else None
        ctx.precision = precision
        # computed in fp32, returned like F.conv2d
        return _native.conv3x3_forward(x, weight, bias, precision).to(x.dtype)

    @staticmethod
    def backward(ctx, grad_y: torch.Tensor):
        x, weight = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        gx, gw, gb = _native.conv3x3_backward(x, weight, grad_y, need_x=nx, need_w=nw, need_b=ctx.has_bias and nb,
                                              precision=ctx.precision)
        if gw is not None:
            gw = gw.to(weight.dtype)
        if gx is not None:
            gx = gx.to(x.dtype)
        if gb is not None:
            gb = gb.to(ctx.bias_dtype)
        return gx, gw, gb, None


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
            precision: str = "split") -> torch.Tensor:
    """F.conv2d(x, weight, bias, padding=1) with a native forward and backward.

    precision "split" (default): fp32-accurate.  "mixed": every product of the
    forward, the dgrad and the wgrad is of its two operands each rounded to
    bf16 (nearest even) from its fp32 value, accumulated in fp32; the bias and
    the bias gradient stay fp32.  Tensors are fp32 either way."""
    _native.conv3_precision(precision)   # before any device check
    return Conv3x3Function.apply(x, weight, bias, precision)


class BnReluDropout2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, drop):
        y, mean, invstd = _native.bn_train_forward(x, weight, bias, drop, eps, momentum, running_mean, running_var,
                                                   relu)
        # the native call wrote the running statistics through raw pointers: bump their
        # version counters, which PlanCache keys on (a later eval() forward repacks)
        for t in (running_mean, running_var):
            if t is not None:
                torch.autograd.graph.increment_version(t)
        ctx.relu = bool(relu)
        ctx.dtypes = (x.dtype, None if weight is None else weight.dtype, None if bias is None else bias.dtype)
        if any(ctx.needs_input_grad[:3]):   # nothing is kept under torch.no_grad()
            ctx.save_for_backward(x, weight, bias, drop, mean, invstd)
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y: torch.Tensor):
        x, weight, bias, drop, mean, invstd = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        gx, gg, gb = _native.bn_train_backward(x, grad_y, weight, bias, drop, mean, invstd, ctx.relu, need_x=nx,
                                               need_gamma=nw and weight is not None,
                                               need_beta=nb and bias is not None)
        if gx is not None:
            gx = gx.to(ctx.dtypes[0])
        if gg is not None:
            gg = gg.to(ctx.dtypes[1]).view_as(weight)
        if gb is not None:
            gb = gb.to(ctx.dtypes[2]).view_as(bias)
        return gx, gg, gb, None, None, None, None, None, None


def bn_relu_dropout2d(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                      running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], *,
                      momentum: float = 0.1, eps: float = 1e-5, relu: bool = True,
                      drop: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Batch-statistics batch norm of x [N, C, H, W], then ReLU (``relu``), then
    the per-plane multiplier ``drop`` [N, C] (Dropout2d with rate p: 0 or
    1 / (1 - p)); native forward and backward.  running_mean / running_var
    (both or neither; [C] fp32 on x's device) are updated in place with
    ``momentum`` as F.batch_norm does, also under torch.no_grad()."""
    if drop is not None and (drop.dim() != 2 or tuple(drop.shape) != tuple(x.shape[:2])):
        raise ValueError(f"drop must be [N, C] = {list(x.shape[:2])}, got {list(drop.shape)}")
    return BnReluDropout2dFunction.apply(x, weight, bias, running_mean, running_var, float(momentum), float(eps),
                                         bool(relu), drop)


class DetectorLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, box_weight, box_bias, cls_weight, cls_bias, anchors, gt_boxes, image_size, pos_thr,
                neg_thr, tie_eps, alpha, gamma, beta, box_weight_factor):
        assign, n_pos, _ = _native.detector_targets(anchors, gt_boxes, pooled.shape[0], image_size, pos_thr, neg_thr,
                                                    tie_eps)
        params = (box_weight, box_bias, cls_weight, cls_bias)
        want = any(ctx.needs_input_grad[1:5])
        loss, grads = _native.detector_loss(pooled, *params, anchors, gt_boxes, assign, n_pos, image_size, alpha,
                                            gamma, beta, box_weight_factor, want_grad=want)
        if want:   # the gradients of loss[0], in the parameters' own shapes and dtypes
            ctx.save_for_backward(*[g.view_as(p).to(p.dtype) for g, p in zip(grads, params)])
        ctx.mark_non_differentiable(assign, n_pos)
        return loss[0], loss[1], loss[2], assign, n_pos

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_cls, g_box, _ga, _gn):
        # the class and box parts are detached extras: only the total's gradient flows
        grads = [g * g_loss if need else None for g, need in zip(ctx.saved_tensors, ctx.needs_input_grad[1:5])]
        return (None, *grads) + (None,) * 10


def detector_loss(pooled: torch.Tensor, box_weight: torch.Tensor, box_bias: torch.Tensor, cls_weight: torch.Tensor,
                  cls_bias: torch.Tensor, anchors: torch.Tensor, gt_boxes: Optional[torch.Tensor], image_size, *,
                  pos_thr: float = 0.5, neg_thr: float = 0.4, tie_eps: float = 1e-5, alpha: float = 0.25,
                  gamma: float = 2.0, beta: float = 1.0 / 9, box_weight_factor: float = 1.0) -> torch.Tensor:
    """The person detector's training loss on pooled
    [B, 3136, 128] (``Plan.detector_features``) with gradients to the four
    parameters of box_heads[0] / cls_heads[0] (their nn.Conv2d shapes
    [36,128,1,1], [36], [9,128,1,1], [9]); nothing flows to ``pooled`` (the
    trunk is frozen).  gt_boxes [B, G, 4] cxcywh normalised, G <= 64 (None or
    G = 0: every anchor negative); image_size (H, W).  Returns the 0-d loss
    (sum FL + box_weight_factor * sum SL1) / N with the detached extras
    ``cls_part``, ``box_part`` (0-d), ``assign`` [B, 28224] int32 and ``n_pos``
    [B] int32 as attributes.  Device tensors only; no host synchronisation."""
    _native._require_cuda(pooled, "pooled")
    for t, name in ((box_weight, "box_weight"), (box_bias, "box_bias"), (cls_weight, "cls_weight"),
                    (cls_bias, "cls_bias"), (anchors, "anchors")):
        _native._require_cuda(t, name)
    if gt_boxes is not None:
        _native._require_cuda(gt_boxes, "gt_boxes")
    loss, cls_part, box_part, assign, n_pos = DetectorLossFunction.apply(
        pooled, box_weight, box_bias, cls_weight, cls_bias, anchors, gt_boxes, tuple(int(v) for v in image_size),
        float(pos_thr), float(neg_thr), float(tie_eps), float(alpha), float(gamma), float(beta),
        float(box_weight_factor))
    loss.cls_part, loss.box_part = cls_part.detach(), box_part.detach()
    loss.assign, loss.n_pos = assign, n_pos
    return loss


class SoftArgmaxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heat: torch.Tensor, temperature: float):
        ctx.save_for_backward(heat)
        ctx.temperature = temperature
        return _native.decode_heatmaps(heat, _native.DECODE_SOFTARGMAX, temperature)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_coords: torch.Tensor):
        (heat,) = ctx.saved_tensors
        return _native.softargmax_backward(heat, grad_coords, ctx.temperature).to(heat.dtype), None


def soft_argmax(heat: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """The soft-argmax decode of heat [n, K, H, W] -> coords [n, K, 2]
    (normalised x, y), differentiable with respect to ``heat``: the forward is
    ``decode_heatmaps_soft_argmax``'s (kpd_decode_heatmaps, bit for bit), the
    backward kpd_softargmax_backward."""
    _native._coord_heat(heat, temperature)   # shape, device and temperature checks before any launch
    return SoftArgmaxFunction.apply(heat, float(temperature))


class SoftArgmaxCoordLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heat, gt_coords, visibility, temperature, loss_type, pixel_weight_scale, distance_threshold):
        loss, coords, grad = _native.coord_loss(heat, gt_coords, visibility, temperature, loss_type,
                                                pixel_weight_scale, distance_threshold,
                                                want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad if grad is not None else torch.empty(0, device=heat.device))
        ctx.heat_dtype = heat.dtype
        ctx.mark_non_differentiable(coords)
        return loss.to(heat.dtype), coords

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_coords):
        (grad,) = ctx.saved_tensors
        if grad.numel() == 0:
            return (None,) * 7
        return (grad * g_loss).to(ctx.heat_dtype), None, None, None, None, None, None


def soft_argmax_coord_loss(heat: torch.Tensor, gt_coords: torch.Tensor, visibility: torch.Tensor,
                           temperature: float = 1.0, loss_type: str = "smooth_l1", pixel_weight_scale: float = 100.0,
                           distance_threshold: float = 5.0):
    """``SpatialCoordinateLoss`` of the soft-argmax decode of heat [n, K, H, W]
    against gt_coords [n, K, 2] (the decode's normalised frame) over the joints
    with visibility [n, K] > 0, in one native pass (kpd_coord_loss, DESIGN.md
    §3k) -> (loss 0-d, coords [n, K, 2]).  The gradient with respect to
    ``heat`` is computed in the forward when ``heat.requires_grad``; ``coords``
    is detached (use ``soft_argmax`` for a differentiable decode).  A masked
    joint's gt may hold anything, NaN included.  Device tensors only; no host
    synchronisation."""
    return SoftArgmaxCoordLossFunction.apply(heat, gt_coords, visibility, float(temperature), str(loss_type),
                                             float(pixel_weight_scale), float(distance_threshold))


def boxes_to_rois(boxes: torch.Tensor, rows: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """The rows ``rows`` of cxcywh boxes [B, P, 4] as roi_align rois [n, 5] (image,
    x1, y1, x2, y2) on a height x width map, by the fused forward's rule
    (kpd_roi_features): corners clamped to [0, 1], then scaled, in fp32."""
    r = rows.long()
    b = boxes.reshape(-1, 4).float()[r]
    half = b[:, 2:] / 2
    scale = torch.tensor([width, height], dtype=torch.float32, device=b.device)
    lo = torch.clamp(b[:, :2] - half, 0, 1) * scale
    hi = torch.clamp(b[:, :2] + half, 0, 1) * scale
    image = torch.div(r, boxes.size(1), rounding_mode="floor").to(torch.float32)
    return torch.cat([image[:, None], lo, hi], dim=1)


class RoiAlignBoxesFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, level0, boxes, rows, topk):
        B, C, H, W = level0.shape
        rois = boxes_to_rois(boxes, rows, H, W)
        if topk is None:
            out = _native.roi_align(level0, rois, 56)
        else:
            # x[b, topk[b]] as B * Cs single-channel images, and every ROI once per channel on its own
            # image's Cs planes: one kpd_roi_align call whatever topk holds.  This is a detour off the
            # fused forward's path, paid for simplicity: the gather materialises a [B, Cs, H, W] copy
            # (201 MB at 64 x 64 x 128 x 96) and the per-ROI coordinate work is repeated Cs times; top-k +
            # this forward measure 0.68 ms of a 35.7 ms step.  A channel-indexed
            # forward kernel would avoid both.
            Cs = topk.size(1)
            sel = torch.gather(level0.detach().float(), 1, topk.long()[:, :, None, None].expand(B, Cs, H, W))
            n = rois.size(0)
            planes = (rois[:, :1] * Cs + torch.arange(Cs, device=rois.device, dtype=torch.float32)[None, :])
            per_plane = torch.cat([planes.reshape(-1, 1), rois[:, None, 1:].expand(n, Cs, 4).reshape(-1, 4)], dim=1)
            out = _native.roi_align(sel.reshape(B * Cs, 1, H, W), per_plane, 56).view(n, Cs, 56, 56)
        ctx.save_for_backward(boxes, rows, topk if topk is not None else torch.empty(0, device=level0.device))
        ctx.shape, ctx.has_topk, ctx.dtype = (C, H, W), topk is not None, level0.dtype
        return out.to(level0.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: torch.Tensor):
        boxes, rows, topk = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        g = _native.roi_align_backward(grad_out, boxes, rows, topk if ctx.has_topk else None, *ctx.shape)
        return g.to(ctx.dtype), None, None, None


def roi_align_boxes(level0: torch.Tensor, boxes: torch.Tensor, rows: torch.Tensor,
                    topk: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ROI align of FPN level 0 [B, C, H, W] over the rows ``rows`` (ascending
    indices into B*P, an integer device tensor) of cxcywh boxes [B, P, 4], as the
    fused forward does it (56 x 56 bins, aligned=False, adaptive sampling grid),
    on the channels ``topk`` [B, Cs] of each ROI's image (None: all C) ->
    [n, Cs, 56, 56], differentiable with respect to ``level0``: the forward is
    kpd_roi_align on x[b, topk[b]], the backward kpd_roi_align_backward
    (deterministic, no atomics).  boxes, rows and topk get no
    gradient.  Device tensors only; no host synchronisation."""
    _native._require_cuda(level0, "level0")
    if level0.dim() != 4:
        raise ValueError(f"level0 must be [B, C, H, W], got {tuple(level0.shape)}")
    B = level0.size(0)
    if boxes.dim() != 3 or boxes.size(0) != B or boxes.size(2) != 4:
        raise ValueError(f"boxes must be [{B}, P, 4], got {tuple(boxes.shape)}")
    if rows.dim() != 1 or rows.is_floating_point():
        raise ValueError("rows must be a 1-D integer tensor")
    if rows.numel() > B * boxes.size(1):
        raise ValueError(f"rows holds {rows.numel()} indices for {B * boxes.size(1)} boxes")
    if topk is not None and (topk.dim() != 2 or topk.size(0) != B or topk.is_floating_point()
                             or topk.size(1) > level0.size(1)):
        raise ValueError(f"topk must be an integer tensor [{B}, Cs <= {level0.size(1)}], got {tuple(topk.shape)}")
    dev = level0.device
    boxes = boxes.detach().to(dev, torch.float32).contiguous()
    rows = rows.detach().to(dev, torch.int32).contiguous()
    topk = None if topk is None else topk.detach().to(dev, torch.int32).contiguous()
    return RoiAlignBoxesFunction.apply(level0, boxes, rows, topk)
