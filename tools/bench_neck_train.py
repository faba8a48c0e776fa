#!/usr/bin/env python3
"""Cost of training the FPN's level-0 path under the heatmap head (DESIGN.md
§3l, §7), alternated in one process.

64 seeded 256 x 192 images with 2 persons each (128 ROIs, level 0 128 x 96):

(a) `kpd_roi_align_backward` (gout [128,64,56,56] -> gfeat [64,128,128,96])
    against
      * the torch chain of the same formulas: My [n,56,H] and Mx [n,56,W] built
        on the device from the boxes (fp32 coordinates and decisions, weights
        scattered with scatter_add_), My^T . G . Mx / count by batched matmul,
        then the scatter through topk (index_put_ with accumulate), and
      * a device-to-device `copy_` moving the call's byte count (gout read once
        + gfeat written once = read + write of a tensor of half that size),
        with the bytes/s the call achieves.
(b) One `Trainer.train_step` with `train_neck=True` against `train_neck=False`
    (two models from the same weights, the same batch).
(c) The split of the `train_neck=True` step, by HIP events inside one step:
    body taps, neck forward (laterals + level-0 conv + batch norm), top-k + ROI
    align forward, head forward + loss, backward (head, ROI align, neck),
    optimizer.

Every variant is timed with HIP events around `--inner` back-to-back calls on
resident tensors; after warm-ups the variants alternate `--rounds` times and
the medians are reported with min-max.  One JSON line; no pass/fail threshold.

The measurement runs in a child process under its own `timeout`:

    python tools/bench_neck_train.py [--images 64] [--rounds 7] [--inner 3] [--timeout 600]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    import torch
    from dll import _native
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.heatmap_head import generate_roi_targets
    from dll.models.synthetic import synthetic_boxes, synthetic_images, synthetic_state_dict
    from dll.ops import roi_align_boxes
    from dll.training import Trainer
    dev = torch.device("cuda", 0)
    B, P, K, C, Cs, H, W, S = a.images, 2, 17, 128, 64, 128, 96, 56

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def alternate(variants, inner):
        for _ in range(2):
            for fn in variants.values():
                timed(fn, inner)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn, inner))
        return {k: statistics.median(v) for k, v in ms.items()}, ms

    def report(med, ms, names):
        out = {}
        for k in names:
            out[k + "_ms"] = round(med[k], 4)
            out[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        return out

    cfg = TrainingConfig()
    trainers = {}
    for name, neck in (("head_only", False), ("train_neck", True)):
        m = MultiPersonKeypointModel(ModelConfig(), cfg)
        m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0))
        trainers[name] = Trainer(m, dev, [], [], cfg, train_neck=neck)
    image = synthetic_images(B, 3, 256, 192, seed=a.seed + 1, device=dev)
    boxes = synthetic_boxes(B, P, seed=a.seed + 2, device=dev)
    g = torch.Generator().manual_seed(a.seed + 3)
    uv = (torch.rand(B, P, K, 2, generator=g) * 0.9 + 0.05).to(dev)
    kp = boxes[:, :, None, :2] - boxes[:, :, None, 2:] / 2 + uv * boxes[:, :, None, 2:]
    vis = torch.randint(0, 3, (B, P, K), generator=g).float().to(dev)
    batch = {"image": image, "bboxes": [boxes], "keypoints": kp, "visibilities": vis}
    n = B * P
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    res = {"metric": "neck_train_ms", "images": B, "persons": P, "rois": n, "rounds": a.rounds, "inner": a.inner}

    # ---- (a) the ROI-align backward
    gout = torch.randn(n, Cs, S, S, generator=torch.Generator().manual_seed(a.seed + 4)).to(dev)
    topk = torch.stack([torch.randperm(C, generator=g)[:Cs] for _ in range(B)]).to(dev)
    topk32 = topk.to(torch.int32)
    bidx = torch.arange(B, device=dev).repeat_interleave(P)
    b4 = boxes.view(-1, 4)
    lo = ((b4[:, :2] - b4[:, 2:] / 2).clamp(0, 1) * torch.tensor([W, H], device=dev, dtype=torch.float32))
    hi = ((b4[:, :2] + b4[:, 2:] / 2).clamp(0, 1) * torch.tensor([W, H], device=dev, dtype=torch.float32))
    size = (hi - lo).clamp(min=1.0)
    grid = torch.ceil(size / S)
    gmax = [int(grid[:, 0].max()), int(grid[:, 1].max())]       # (a host read, outside the timed chain)
    pp = torch.arange(S, device=dev, dtype=torch.float32)

    def axis_matrix(ax, extent):
        st, bn, gr = lo[:, ax, None, None], (size[:, ax] / S)[:, None, None], grid[:, ax, None, None]
        ii = torch.arange(gmax[ax], device=dev, dtype=torch.float32)[None, None, :]
        c = st + pp[None, :, None] * bn + (ii + 0.5) * bn / gr
        ok = ((ii < gr) & ~((c < -1.0) | (c > extent))).float()
        c = c.clamp(min=0.0)
        l0 = c.floor().long()
        edge = l0 >= extent - 1
        l0 = torch.where(edge, torch.full_like(l0, extent - 1), l0)
        h0 = torch.where(edge, l0, l0 + 1)
        frac = torch.where(edge, torch.zeros_like(c), c - l0.float())
        M = torch.zeros(n, S, extent, device=dev)
        M.scatter_add_(2, l0, (1.0 - frac) * ok)
        M.scatter_add_(2, h0, frac * ok)
        return M

    def chain():
        Mx, My = axis_matrix(0, W), axis_matrix(1, H)
        My = My / (grid[:, 0] * grid[:, 1]).clamp(min=1.0)[:, None, None]
        d = torch.matmul(My.transpose(1, 2)[:, None], torch.matmul(gout, Mx[:, None]))     # [n, Cs, H, W]
        out = torch.zeros(B, C, H, W, device=dev)
        out.index_put_((bidx[:, None].expand(n, Cs), topk[bidx]), d, accumulate=True)
        return out

    def native():
        return _native.roi_align_backward(gout, boxes, rows, topk32, C, H, W)

    gn, gc = native(), chain()
    torch.cuda.synchronize()
    res["backward_max_abs_diff_to_chain"] = float((gn - gc).abs().max())
    res["backward_max_abs"] = float(gn.abs().max())
    res["backward_bit_equal_between_calls"] = bool(torch.equal(gn, native()))
    nbytes = (gout.numel() + gn.numel()) * 4
    del gc
    ca = torch.empty(nbytes // 8, device=dev)
    cb = torch.empty_like(ca)
    torch.cuda.empty_cache()
    med, ms = alternate({"native": native, "chain": chain, "copy": lambda: cb.copy_(ca)}, a.inner)
    res["backward"] = report(med, ms, ("native", "chain", "copy"))
    res["backward"].update(native_over_chain=round(med["native"] / med["chain"], 3),
                           native_over_copy=round(med["native"] / med["copy"], 3), mbytes=round(nbytes / 1e6, 1),
                           native_gbytes_per_s=round(nbytes / med["native"] / 1e6, 1),
                           copy_gbytes_per_s=round(nbytes / med["copy"] / 1e6, 1))
    del ca, cb, gn
    torch.cuda.empty_cache()

    # ---- (b) the step, with and without the neck
    first = {k: float(t.train_step(batch)["loss"]) for k, t in trainers.items()}
    inner = max(1, a.inner // 2)
    med, ms = alternate({k: (lambda t=t: t.train_step(batch)) for k, t in trainers.items()}, inner)
    res["step"] = report(med, ms, ("head_only", "train_neck"))
    res["step"].update(train_neck_over_head_only=round(med["train_neck"] / med["head_only"], 3), first_loss=first)

    # ---- (c) the split of the train_neck step
    tr = trainers["train_neck"]
    model, head, opt, crit = tr.model, tr.head, tr.optimizer, tr.model.loss_fn.heatmap_loss
    fpn = model.backbone.fpn
    gt, tw = generate_roi_targets(kp, vis, boxes, rows, (S, S), 2.0)
    names = ("body", "neck_forward", "roi_forward", "head_forward", "backward", "optimizer")
    # the level-0 conv's share of the neck, forward and backward, on its own
    from dll.ops import conv3x3
    wc = fpn.fpn_convs[0][0].weight
    xin = torch.randn(B, C, H, W, device=dev).requires_grad_(True)
    gy = torch.randn(B, C, H, W, device=dev)

    def conv_fwd():
        with torch.no_grad():
            return conv3x3(xin, wc, None)

    def conv_fwd_bwd():
        conv3x3(xin, wc, None).backward(gy)
        xin.grad, wc.grad = None, None

    def staged():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        fpn.train()
        head.train()
        opt.zero_grad(set_to_none=True)
        ev[0].record()
        with torch.no_grad():
            taps = list(model.backbone.body(image).values())
        ev[1].record()
        level0 = fpn.forward_level0(taps)
        ev[2].record()
        with torch.no_grad():
            tk = model.channel_attention.native_select(level0.detach(), 64, select=False)[1]
        x = roi_align_boxes(level0, boxes, rows, tk)
        ev[3].record()
        loss = crit(head(x)[0], gt, tw)
        ev[4].record()
        loss.backward()
        ev[5].record()
        opt.step()
        ev[6].record()
        ev[6].synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(names))]

    for _ in range(2):
        staged()
    runs = [staged() for _ in range(a.rounds)]
    split = {}
    for i, k in enumerate(names):
        v = [r[i] for r in runs]
        split[k + "_ms"] = round(statistics.median(v), 4)
        split[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    split["sum_ms"] = round(sum(split[k + "_ms"] for k in names), 4)
    res["split"] = split
    med, ms = alternate({"conv3x3_forward": conv_fwd, "conv3x3_forward_backward": conv_fwd_bwd}, inner)
    res["level0_conv"] = report(med, ms, ("conv3x3_forward", "conv3x3_forward_backward"))
    res["level0_conv"]["forward_backward_share_of_train_neck_step"] = round(
        med["conv3x3_forward_backward"] / res["step"]["train_neck_ms"], 3)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="back-to-back calls per timed interval")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=600, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # the GPU step: a fresh child under its own time limit
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()), "--worker"]
    cmd += [v for v in sys.argv[1:] if v != "--worker"]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
