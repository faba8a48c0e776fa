#!/usr/bin/env python3
"""Cost of the fused coordinate loss on the decoded keypoints and of a training
step with it, alternated in one process.

(a) `dll.ops.soft_argmax_coord_loss` forward + backward (kpd_coord_loss: one
    read of the heatmaps, one write of their gradient, 3 launches) on
    `--rois` x 17 x 56 x 56 seeded sigmoid-of-normal heatmaps against the torch
    chain of the same formulas in fp32 with autograd: softmax over the plane,
    the two expectations, smooth-L1, the distance clamp, the masked mean
    (without SpatialCoordinateLoss's host synchronisation: the chain at its
    best).
(b) The same against a device-to-device `copy_` of the tensor (one read and
    one write of its bytes: what the fused call has to move); the achieved
    bytes/s of both.
(c) One whole `Trainer.train_step` (Adam) at `--rois` ROIs (rois / 2 images
    with 2 people each) with coord_weight 0 and 1.

Every variant is timed with HIP events around `--inner` back-to-back calls on
resident tensors; after warm-ups the variants alternate `--rounds` times and
the medians are reported with min-max.  One JSON line; the tool sets no
pass/fail threshold.  The measurement runs in a child process under its own
`timeout`:

    python tools/bench_coord_loss.py [--rois 128] [--rounds 7] [--inner 5] [--timeout 600]
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
    import torch.nn.functional as F
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_boxes, synthetic_images, synthetic_state_dict
    from dll.ops import soft_argmax_coord_loss
    from dll.training import Trainer
    dev = torch.device("cuda", 0)
    R, K, H, W = a.rois, 17, 56, 56
    T, S, tau = 1.0, 100.0, 5.0

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

    res = {"metric": "coord_loss_ms", "rois": R, "shape": [R, K, H, W], "rounds": a.rounds, "inner": a.inner}

    # ---- (a), (b) the fused call, the torch chain, the copy
    g = torch.Generator(device=dev).manual_seed(a.seed)
    heat = torch.sigmoid(torch.randn(R, K, H, W, device=dev, generator=g)).requires_grad_(True)
    gt = torch.rand(R, K, 2, device=dev, generator=g)
    vis = (torch.rand(R, K, device=dev, generator=g) > 0.25).float()
    xs = torch.arange(W, device=dev, dtype=torch.float32) / (W - 1)
    ys = torch.arange(H, device=dev, dtype=torch.float32) / (H - 1)

    def fused():
        heat.grad = None
        loss, _ = soft_argmax_coord_loss(heat, gt, vis, T, "smooth_l1", S, tau)
        loss.backward()
        return loss

    def chain():
        heat.grad = None
        p = torch.softmax(heat.reshape(R, K, H * W) / T, dim=-1).reshape(R, K, H, W)
        coords = torch.stack([(p.sum(dim=2) * xs).sum(dim=-1), (p.sum(dim=3) * ys).sum(dim=-1)], dim=-1)
        mask = (vis > 0).float()
        target = torch.where(mask.unsqueeze(-1) > 0, gt, torch.zeros((), device=dev))
        per = F.smooth_l1_loss(coords, target, reduction="none").sum(dim=-1) * mask
        per = per * torch.clamp(torch.norm(coords - target, dim=-1) / tau, min=1.0, max=3.0) * S
        loss = per.sum() / (mask.sum() + 1e-8)
        loss.backward()
        return loss

    lf = fused()
    gf = heat.grad.clone()
    lc = chain()
    torch.cuda.synchronize()
    res["loss_check"] = {"fused": float(lf.detach()), "chain": float(lc.detach()),
                         "grad_max_rel_diff": float((gf - heat.grad).abs().max() / heat.grad.abs().max())}
    ca, cb = torch.empty_like(heat), torch.empty_like(heat)
    med, ms = alternate({"fused": fused, "chain": chain, "copy": lambda: cb.copy_(ca)}, a.inner)
    nbytes = heat.numel() * 4
    res["loss"] = report(med, ms, ("fused", "chain", "copy"))
    res["loss"].update(fused_over_chain=round(med["fused"] / med["chain"], 3),
                       fused_over_copy=round(med["fused"] / med["copy"], 3), tensor_mbytes=round(nbytes / 1e6, 2),
                       fused_gbytes_per_s=round(2 * nbytes / med["fused"] / 1e6, 1),
                       copy_gbytes_per_s=round(2 * nbytes / med["copy"] / 1e6, 1))
    del ca, cb, gf
    heat.grad = None
    torch.cuda.empty_cache()

    # ---- (c) the training step without and with the term
    B, P = max(1, R // 2), 2
    image = synthetic_images(B, 3, 256, 192, seed=a.seed + 1, device=dev)
    boxes = synthetic_boxes(B, P, seed=a.seed + 2, device=dev)
    uv = torch.rand(B, P, K, 2, device=dev, generator=g) * 0.9 + 0.05
    kp = boxes[:, :, None, :2] - boxes[:, :, None, 2:] / 2 + uv * boxes[:, :, None, 2:]
    batch = {"image": image, "bboxes": [boxes], "keypoints": kp,
             "visibilities": torch.randint(1, 3, (B, P, K), device=dev, generator=g).float()}
    trainers = {}
    for name, w in (("train_step_w0", 0.0), ("train_step_w1", 1.0)):
        cfg = TrainingConfig()
        model = MultiPersonKeypointModel(ModelConfig(), cfg)
        model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=0))
        trainers[name] = Trainer(model, dev, [], [], cfg, coord_weight=w)
    rows = {k: tr.train_step(batch)["rows"] for k, tr in trainers.items()}
    med, ms = alternate({k: (lambda tr=tr: tr.train_step(batch)) for k, tr in trainers.items()}, max(1, a.inner // 2))
    res["step"] = report(med, ms, tuple(trainers))
    res["step"].update(rows=rows, w1_over_w0=round(med["train_step_w1"] / med["train_step_w0"], 4))
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls per timed interval")
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
