"""Plain CPU restatement of the detector-training rules: anchor
matching, the focal + smooth-L1 loss and its closed-form gradients, in float64
(torch on the CPU only, no autograd in the closed forms).

match(..., dtype=torch.float32) is the matching in the device's arithmetic:
every operation of the IoU in fp32 in the order of csrc/nms.hip's iou_cxcywh
(= oracle.kpd_oracle.box_iou_cxcywh), thresholds rounded to fp32; float64 is
the same formulas on the same fp32 inputs in double.  Where the two agree on
every anchor (tests/test_det_train_cpu.py checks it for each GPU fixture) a
device mismatch is a bug, not a rounding effect.

chain(...) is the same loss written with differentiable torch ops in a dtype
of the caller's choosing: float64 pins the closed-form gradients to autograd,
float32 is the GPU tests' yardstick (what an fp32 torch implementation of the
same formulas loses against float64).
"""
import math

import torch
import torch.nn.functional as F

from oracle.kpd_oracle import box_iou_cxcywh

GRID = 56
A = GRID * GRID * 9


def anchor_boxes(anchors, H, W, dtype):
    """[A,4] (ax, ay, aw, ah): the anchor buffer with w, h divided by the image's W, H in ``dtype``."""
    a = anchors.to(torch.float32).to(dtype)
    return torch.stack([a[:, 0], a[:, 1], a[:, 2] / W, a[:, 3] / H], dim=1)


def present(gt):
    """[.., G] bool: a row is absent if all four values are 0, if w <= 0 or h <= 0, or if any value is NaN."""
    nan = torch.isnan(gt).any(dim=-1)
    zero = (gt == 0).all(dim=-1)
    return ~nan & ~zero & (gt[..., 2] > 0) & (gt[..., 3] > 0)


def match(anchors, gt_boxes, B, H, W, pos_thr=0.5, neg_thr=0.4, tie_eps=1e-5, dtype=torch.float64):
    """-> dict(assign [B,A] int32, n_pos [B] int32, gt_best [B,G] dtype, iou [B] list of [A,G] or None).
    gt_boxes [B,G,4] fp32 (or None: G = 0)."""
    G = 0 if gt_boxes is None else gt_boxes.shape[1]
    assign = torch.full((B, A), -1, dtype=torch.int32)
    gt_best = torch.zeros(B, G, dtype=dtype)
    ious = []
    if G == 0:
        return dict(assign=assign, n_pos=torch.zeros(B, dtype=torch.int32), gt_best=gt_best, iou=[None] * B)
    an = anchor_boxes(anchors, H, W, dtype)
    # the thresholds rounded to fp32, as the device receives them
    pt, nt, te = (torch.tensor(v, dtype=torch.float32).to(dtype) for v in (pos_thr, neg_thr, tie_eps))
    for b in range(B):
        g32 = gt_boxes[b].to(torch.float32)
        pres = present(g32)
        # NaN -> 0 (the row is absent anyway); an infinity stays one, as the device sees it (torch.nan_to_num
        # would make it the largest finite number, and the box's IoU a positive denormal instead of 0)
        gb = torch.where(torch.isnan(g32), torch.zeros_like(g32), g32).to(dtype)
        iou = box_iou_cxcywh(an, gb)                       # [A, G]
        iou = torch.where(iou > 0, iou, torch.zeros_like(iou))
        ious.append(iou)
        if not bool(pres.any()):
            continue
        masked = torch.where(pres[None, :], iou, torch.full_like(iou, -1.0))
        best, arg = masked.max(dim=1)
        # ties: the lower slot (torch.max's index is unspecified among equals)
        arg = (masked == best[:, None]).to(torch.int64).argmax(dim=1)
        a = torch.full((A,), -1, dtype=torch.int64)
        a = torch.where(best >= nt, torch.full_like(a, -2), a)
        a = torch.where(best >= pt, arg, a)
        gmax = torch.where(pres, iou.max(dim=0).values, torch.zeros(G, dtype=dtype))
        gt_best[b] = gmax
        # the band is capped at half the maximum, so a sub-pixel GT (gmax < tie_eps) keeps to its tie set
        band = torch.minimum(te, gmax / 2)
        low = (pres[None, :] & (gmax[None, :] > 0) & (iou >= gmax[None, :] - band[None, :])).any(dim=1)
        a = torch.where(low, arg, a)
        assign[b] = a.to(torch.int32)
    return dict(assign=assign, n_pos=(assign >= 0).sum(dim=1).to(torch.int32), gt_best=gt_best, iou=ious)


def threshold_margin(m, pos_thr=0.5, neg_thr=0.4, tie_eps=1e-5):
    """(thr, tie) of a float64 ``match`` result: the smallest distance of any anchor's best IoU to pos_thr /
    neg_thr, and of any IoU to its GT's gmax - min(tie_eps, gmax / 2) (at most that band: the maximum itself);
    inf without a present GT."""
    thr = tie = math.inf
    for b, iou in enumerate(m["iou"]):
        if iou is None:
            continue
        gm = m["gt_best"][b]
        on = gm > 0
        if not bool(on.any()):
            continue
        best = iou[:, on].max(dim=1).values
        thr = min(thr, float((best - pos_thr).abs().min()), float((best - neg_thr).abs().min()))
        band = torch.clamp(gm[on] / 2, max=tie_eps)
        tie = min(tie, float((iou[:, on] - (gm[on] - band)[None, :]).abs().min()))
    return thr, tie


def heads(x, box_w, box_b, cls_w, cls_b):
    """x [B,3136,128] -> (d [B,A,4], z [B,A]) in x's dtype: the 1x1 heads per cell, anchors in order (i, j, a)."""
    B = x.shape[0]
    d = F.linear(x, box_w.reshape(36, 128).to(x.dtype), box_b.to(x.dtype)).reshape(B, A, 4)
    z = F.linear(x, cls_w.reshape(9, 128).to(x.dtype), cls_b.to(x.dtype)).reshape(B, A)
    return d, z


def box_targets(anchors, gt_boxes, assign, H, W, dtype):
    """[B,A,4] encoded targets (the decode's inverse), zeros where assign < 0."""
    an = anchor_boxes(anchors, H, W, dtype)
    B = assign.shape[0]
    t = torch.zeros(B, A, 4, dtype=dtype)
    if gt_boxes is None or gt_boxes.shape[1] == 0:
        return t
    for b in range(B):
        pos = assign[b] >= 0
        g = gt_boxes[b].to(torch.float32).to(dtype)[assign[b][pos].long()]
        a = an[pos]
        t[b][pos] = torch.stack([(g[:, 0] - a[:, 0]) / a[:, 2], (g[:, 1] - a[:, 1]) / a[:, 3],
                                 torch.log(g[:, 2] / a[:, 2]), torch.log(g[:, 3] / a[:, 3])], dim=1)
    return t


def loss_and_grads(x, box_w, box_b, cls_w, cls_b, anchors, gt_boxes, assign, H, W, alpha=0.25, gamma=2.0,
                   beta=1.0 / 9, box_weight=1.0, n=None):
    """Closed forms in float64 -> dict(loss, cls, box (python floats), n (N), g_box_w [36,128], g_box_b [36],
    g_cls_w [9,128], g_cls_b [9]).  loss = (sum FL + box_weight sum SL1) / N, cls = sum FL / N, box = sum SL1 / N.
    N = max(1, n), n = the number of assign >= 0 unless given (the device reads it from n_pos)."""
    dt = torch.float64
    x = x.to(dt)
    B = x.shape[0]
    d, z = heads(x, box_w.to(dt), box_b.to(dt), cls_w.to(dt), cls_b.to(dt))
    pos, ign = assign >= 0, assign == -2
    N = max(1, int(pos.sum()) if n is None else int(n))
    p = torch.sigmoid(z)
    q = torch.sigmoid(-z)
    logp, logq = -F.softplus(-z), -F.softplus(z)
    fl1 = -alpha * q ** gamma * logp
    fl0 = -(1 - alpha) * p ** gamma * logq
    g1 = alpha * q ** gamma * (gamma * p * logp - q)
    g0 = (1 - alpha) * p ** gamma * (p - gamma * q * logq)
    fl = torch.where(pos, fl1, fl0)
    gz = torch.where(pos, g1, g0)
    fl = torch.where(ign, torch.zeros_like(fl), fl)
    gz = torch.where(ign, torch.zeros_like(gz), gz)
    t = box_targets(anchors, gt_boxes, assign, H, W, dt)
    df = d - t
    ad = df.abs()
    sl = torch.where(ad < beta, 0.5 * df * df / beta, ad - 0.5 * beta)
    gd = torch.where(ad < beta, df / beta, torch.sign(df))
    sl = sl * pos[..., None]
    gd = gd * pos[..., None]
    cls_sum, box_sum = float(fl.sum()), float(sl.sum())
    gz = (gz / N).reshape(B * GRID * GRID, 9)
    gd = (gd * (box_weight / N)).reshape(B * GRID * GRID, 36)
    xf = x.reshape(B * GRID * GRID, 128)
    return dict(loss=(cls_sum + box_weight * box_sum) / N, cls=cls_sum / N, box=box_sum / N, n=N,
                g_box_w=gd.t() @ xf, g_box_b=gd.sum(dim=0), g_cls_w=gz.t() @ xf, g_cls_b=gz.sum(dim=0))


def chain(x, box_w, box_b, cls_w, cls_b, anchors, gt_boxes, assign, H, W, alpha=0.25, gamma=2.0, beta=1.0 / 9,
          box_weight=1.0, dtype=torch.float64, n=None):
    """The same loss as differentiable torch ops in ``dtype`` -> (loss, cls part, box part), 0-d tensors; the
    parameters are used as given (leaf tensors of ``dtype`` that require grad get their gradients by autograd).
    ``n`` as in loss_and_grads."""
    x = x.to(dtype)
    d, z = heads(x, box_w, box_b, cls_w, cls_b)
    pos, ign = assign >= 0, assign == -2
    N = max(1, int(pos.sum()) if n is None else int(n))
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    fl1 = alpha * q ** gamma * F.softplus(-z)
    fl0 = (1 - alpha) * p ** gamma * F.softplus(z)
    fl = torch.where(pos, fl1, fl0)
    fl = torch.where(ign, torch.zeros_like(fl), fl)
    t = box_targets(anchors, gt_boxes, assign, H, W, dtype)
    sl = F.smooth_l1_loss(d, t, beta=beta, reduction="none") * pos[..., None]
    cls_part, box_part = fl.sum() / N, sl.sum() / N
    return cls_part + box_weight * box_part, cls_part, box_part
