#!/usr/bin/env python3
"""Cost of one detector training step and of its device pieces, alternated in
one process.

64 seeded 256 x 192 images with 2 labelled boxes each:

(a) `Plan.detector_features` (kpd_detector_features: the forward's trunk
    stages up to FPN level 0, then the 56 x 56 pool) against the eval forward
    of the same batch without boxes (`model(image)`: the eval detector and the
    heads behind it), of which it is a prefix plus the pool.
(b) `detector_targets` + `detector_loss` (kpd_detector_targets,
    kpd_detector_loss: matching, loss and the four gradients, two launches
    each) against the torch chain on the same assignment -- `F.linear` on the
    pooled features, the same focal / smooth-L1 formulas in torch, autograd --
    and against a device-to-device `copy_` of the pooled tensor's bytes (the
    fused pass reads them once: its floor); the achieved bytes/s of both.
(c) One whole `DetectorTrainer.train_step` (Adam) and its split: trunk
    features, matching + loss + backward, optimizer step.

Every variant is timed with HIP events around `--inner` back-to-back calls on
resident tensors; after warm-ups the variants alternate `--rounds` times and
the medians are reported with min-max.  One JSON line; the tool sets no
pass/fail threshold.  The measurement runs in a child process under its own
`timeout`:

    python tools/bench_det_train.py [--images 64] [--rounds 7] [--inner 3] [--timeout 600]
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
    from dll import _native
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_boxes, synthetic_images, synthetic_state_dict
    from dll.training import DetectorTrainer
    dev = torch.device("cuda", 0)
    B, G, H, W = a.images, 2, 256, 192

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
    model = MultiPersonKeypointModel(ModelConfig(), cfg)
    model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=0))
    trainer = DetectorTrainer(model, dev, [], [], cfg)
    image = synthetic_images(B, 3, H, W, seed=a.seed + 1, device=dev)
    boxes = synthetic_boxes(B, G, seed=a.seed + 2, device=dev)
    batch = {"image": image, "bboxes": [boxes]}
    plan = model.native_plan(dev)
    res = {"metric": "detector_train_step_ms", "images": B, "boxes_per_image": G, "rounds": a.rounds, "inner": a.inner}

    # ---- (a) the trunk's pooled features
    def features():
        return plan.detector_features(image)

    def forward():
        with torch.no_grad():
            return model({"image": image})

    med, ms = alternate({"detector_features": features, "eval_forward": forward}, a.inner)
    res["trunk"] = report(med, ms, ("detector_features", "eval_forward"))
    res["trunk"]["detector_features_over_eval_forward"] = round(med["detector_features"] / med["eval_forward"], 3)
    plan = model.native_plan(dev)
    x = features()
    torch.cuda.empty_cache()

    # ---- (b) matching + loss + gradients
    head = model.person_detector
    anchors = head.anchors
    prm = [head.box_heads[0].weight, head.box_heads[0].bias, head.cls_heads[0].weight, head.cls_heads[0].bias]
    alpha, gamma, beta = 0.25, 2.0, 1.0 / 9

    def native_targets():
        return _native.detector_targets(anchors, boxes, B, (H, W))

    assign, n_pos, _ = native_targets()

    def native_loss():
        return _native.detector_loss(x, *prm, anchors, boxes, assign, n_pos, (H, W), alpha, gamma, beta)

    def native_both():
        a_, n_, _ = _native.detector_targets(anchors, boxes, B, (H, W))
        return _native.detector_loss(x, *prm, anchors, boxes, a_, n_, (H, W), alpha, gamma, beta)

    # the torch chain on the native assignment (its targets encoded once, outside the timed region)
    an = torch.stack([anchors[:, 0], anchors[:, 1], anchors[:, 2] / W, anchors[:, 3] / H], dim=1)
    pos, ign = assign >= 0, assign == -2
    gsel = torch.gather(boxes, 1, assign.clamp(min=0).long()[..., None].expand(-1, -1, 4))
    tgt = torch.stack([(gsel[..., 0] - an[:, 0]) / an[:, 2], (gsel[..., 1] - an[:, 1]) / an[:, 3],
                       torch.log(gsel[..., 2] / an[:, 2]), torch.log(gsel[..., 3] / an[:, 3])], dim=-1)
    tgt = torch.where(pos[..., None], tgt, torch.zeros((), device=dev))
    leaves = [p.detach().clone().requires_grad_(True) for p in prm]

    def chain():
        for p in leaves:
            p.grad = None
        d = F.linear(x, leaves[0].view(36, 128), leaves[1]).view(B, -1, 4)
        z = F.linear(x, leaves[2].view(9, 128), leaves[3]).view(B, -1)
        p, q = torch.sigmoid(z), torch.sigmoid(-z)
        fl = torch.where(pos, alpha * q ** gamma * F.softplus(-z), (1 - alpha) * p ** gamma * F.softplus(z))
        fl = torch.where(ign, torch.zeros((), device=dev), fl)
        sl = F.smooth_l1_loss(d, tgt, beta=beta, reduction="none") * pos[..., None]
        loss = (fl.sum() + sl.sum()) / n_pos.sum().clamp(min=1)
        loss.backward()
        return loss

    ln, gn = native_loss()
    lc = chain()
    torch.cuda.synchronize()
    res["loss_check"] = {"native": float(ln[0]), "chain": float(lc.detach()),
                         "grad_max_rel_diff": max(float((g.view_as(p.grad) - p.grad).abs().max() / p.grad.abs().max())
                                                  for g, p in zip(gn, leaves))}
    ca, cb = torch.empty_like(x), torch.empty_like(x)
    med, ms = alternate({"targets": native_targets, "loss": native_loss, "targets_loss": native_both, "chain": chain,
                         "copy": lambda: cb.copy_(ca)}, a.inner)
    res["loss"] = report(med, ms, ("targets", "loss", "targets_loss", "chain", "copy"))
    nbytes = x.numel() * 4
    res["loss"].update(targets_loss_over_chain=round(med["targets_loss"] / med["chain"], 3),
                       loss_over_copy=round(med["loss"] / med["copy"], 3), pooled_mbytes=round(nbytes / 1e6, 2),
                       loss_gbytes_per_s=round(nbytes / med["loss"] / 1e6, 1),
                       copy_gbytes_per_s=round(2 * nbytes / med["copy"] / 1e6, 1))
    del ca, cb
    torch.cuda.empty_cache()

    # ---- (c) the step and its split
    opt, crit = trainer.optimizer, trainer.loss_fn

    def loss_step():
        opt.zero_grad(set_to_none=True)
        crit(head, x, boxes, (H, W)).backward()

    loss_step()   # gradients exist for the optimizer-only variant
    med, ms = alternate({"train_step": lambda: trainer.train_step(batch), "trunk": lambda: trainer.trunk_plan()
                         .detector_features(image), "loss_step": loss_step, "optimizer": opt.step},
                        max(1, a.inner // 2))
    res["step"] = report(med, ms, ("train_step", "trunk", "loss_step", "optimizer"))
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
