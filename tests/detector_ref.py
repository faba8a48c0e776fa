"""Plain CPU references of the person-detector glue (torch on the CPU only).

candidates: FPN level 0 -> every anchor's decoded box and score, the arithmetic
and the candidate order (i, j, a) of oracle.kpd_oracle.person_detect, in the
dtype asked for (the GPU tests ask for float64).
greedy_nms: the greedy NMS of oracle.kpd_oracle.nms(stable=True) on fp32
arrays, which also reports how close any IoU it compared came to the
threshold, so a test can tell a wrong decision from a rounding one.
tests/test_detector_ref_cpu.py pins both to the oracle."""
import math

import torch
import torch.nn.functional as F

from oracle.kpd_oracle import box_iou_cxcywh

GRID = 56
NUM_CANDIDATES = GRID * GRID * 9
BBOX_CLIP = math.log(1000.0 / 16)


def candidates(feat0, sd, H, W, dtype, p="person_detector."):
    """feat0 [B,128,Hf,Wf] -> (boxes [B,28224,4] cxcywh, scores [B,28224]) in
    ``dtype``: adaptive average pool to 56 x 56, box_heads[0] / cls_heads[0],
    sigmoid, anchor decode (anchor w/h in pixels over the image's W/H)."""
    B = feat0.shape[0]
    g = F.adaptive_avg_pool2d(feat0.to(dtype), (GRID, GRID))
    box = F.conv2d(g, sd[p + "box_heads.0.weight"].to(dtype), sd[p + "box_heads.0.bias"].to(dtype))
    cls = F.conv2d(g, sd[p + "cls_heads.0.weight"].to(dtype), sd[p + "cls_heads.0.bias"].to(dtype))
    box = box.permute(0, 2, 3, 1).reshape(B, -1, 4)
    score = torch.sigmoid(cls.permute(0, 2, 3, 1).reshape(B, -1))
    anc = sd[p + "anchors"].to(dtype)
    aw = anc[:, 2] / W
    ah = anc[:, 3] / H
    cx = anc[:, 0] + box[..., 0] * aw
    cy = anc[:, 1] + box[..., 1] * ah
    w = aw * torch.exp(torch.clamp(box[..., 2], max=BBOX_CLIP))
    h = ah * torch.exp(torch.clamp(box[..., 3], max=BBOX_CLIP))
    return torch.stack([cx, cy, w, h], dim=-1), score


def greedy_nms(boxes, scores, thr, limit):
    """boxes [n,4], scores [n] fp32 -> (kept indices int64, margin).  Order: a
    stable descending sort (ties and -inf: lower index first; -0.0 == +0.0);
    keep the best remaining candidate, stop at ``limit`` kept (0 / None: no
    limit), drop every remaining candidate whose fp32 IoU with it is NOT <= thr
    (thr rounded to fp32, as the device receives it; IoU: the oracle's
    box_iou_cxcywh).  margin: the smallest |IoU64 - thr| over every comparison
    made, IoU64 the same formula on the same fp32 boxes in float64 (inf when
    nothing was compared)."""
    boxes = boxes.to(torch.float32)
    scores = scores.to(torch.float32)
    thr32 = torch.tensor(thr, dtype=torch.float32)
    thr64 = thr32.double()
    b64 = boxes.double()
    order = torch.sort(scores, descending=True, stable=True).indices
    keep = []
    margin = math.inf
    while order.numel() > 0:
        i = order[0]
        keep.append(int(i))
        if limit and len(keep) >= limit:
            break
        order = order[1:]
        if order.numel() == 0:
            break
        iou = box_iou_cxcywh(boxes[i:i + 1], boxes[order])[0]
        margin = min(margin, float((box_iou_cxcywh(b64[i:i + 1], b64[order])[0] - thr64).abs().min()))
        order = order[iou <= thr32]
    return torch.tensor(keep, dtype=torch.int64), margin
