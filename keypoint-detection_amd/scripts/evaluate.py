#!/usr/bin/env python3
"""Real-data evaluation on a YOLO-pose split, end to end on the device:
decode (host) -> ITransform + target heatmaps (kpd_preprocess,
kpd_target_heatmaps) -> collate -> MultiPersonKeypointModel (kpd_forward) ->
metrics.

``--metric pck`` (the default): ADE / PCK (kpd_keypoint_metrics), the
reference's validation metrics (dll/training/trainer.py:384-429), averaged
over batches as its validate_epoch does (:305-395); the loss terms are not
computed (training is out of scope).  They compare prediction slot p with
ground-truth slot p, so they are defined only with the ground-truth boxes.

``--metric oks``: COCO keypoint AP / AP50 / AP75 / AR (kpd_oks_match per batch,
``dll.utils.OksEvaluator``), which matches predicted poses to labelled persons
and therefore also scores ``--boxes detector``, the model's own person
detector (``model({"image": x})``).  ``--metric both`` prints both sets.

``--pose-nms hard|soft|soft-linear`` (with ``--metric oks`` or ``both``) puts
OKS pose-NMS (kpd_pose_nms, ``dll.utils.suppress_poses``) between the forward
and the OKS matching: two boxes on one person no longer count as a true and a
false positive.  ADE / PCK are slot-wise and keep the unsuppressed outputs.

``--flip-test`` turns on the model's flip-test (``model.flip_test``: a second
forward over the mirrored images, the two heatmaps merged and decoded by
kpd_flip_merge), the protocol top-down pose results are usually reported with:
every metric is then computed on the merged outputs and the JSON line carries
``"flip_test": true``.  Without the option the line has no such key.

The loader's ``efficient_collate_fn`` drops images without a labelled person
from a batch, so detections on such images are not counted as false
positives (inherited behaviour).

    python scripts/evaluate.py --config configs/default_config.yaml \
        --model best_model.pth --dataset-dir data/ --split val --batch-size 32 \
        [--boxes detector --metric oks [--pose-nms hard]]
"""
from __future__ import annotations

import argparse
import json
import sys
from collections import defaultdict
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from dll.data import create_optimized_dataloader  # noqa: E402
from dll.utils import OksEvaluator, calculate_validation_metrics, suppress_poses  # noqa: E402
from predict import (add_flip_test_argument, add_pose_nms_arguments, flip_test_enabled, load_config,  # noqa: E402
                     load_model, pose_nms_options, setup_logging)


def evaluate(model, loader, pck_thresholds, boxes="gt", oks=None, pose_nms=None):
    """One pass over ``loader``.  ``pck_thresholds`` None skips ADE / PCK;
    ``oks`` (an ``OksEvaluator``) is updated per batch, on the device; with
    ``pose_nms`` (``suppress_poses`` options) it scores the poses OKS pose-NMS
    leaves, while the slot-wise ADE / PCK keep the unsuppressed outputs.
    Returns (metrics, batches) or, with ``oks``, (metrics, batches, images)."""
    sums, n, images = defaultdict(float), 0, 0
    with torch.no_grad():
        for batch in loader:
            inp = {"image": batch["image"]}
            if boxes == "gt":
                inp["bboxes"] = batch["bboxes"]
            out = model(inp)
            if pck_thresholds is not None:
                for k, v in calculate_validation_metrics(out, batch, pck_thresholds).items():
                    sums[k] += v
            if oks is not None:
                if pose_nms is not None:
                    out = suppress_poses(out, batch["orig_size"], **pose_nms)
                    oks.update(out, batch, scores=out["pose_scores"])
                else:
                    oks.update(out, batch)
                images += batch["image"].shape[0]
            n += 1
    metrics = {k: v / max(n, 1) for k, v in sums.items()}
    if oks is None:
        return metrics, n
    metrics.update(oks.summarize())
    return metrics, n, images


def main(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate keypoint PCK / ADE or COCO OKS AP on a dataset split")
    ap.add_argument("--config", required=True)
    ap.add_argument("--model", required=True, help="checkpoint path, or 'synthetic'")
    ap.add_argument("--dataset-dir", required=True)
    ap.add_argument("--split", default="val")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--precision", default="split", choices=["split", "fp32", "mixed"])
    ap.add_argument("--boxes", default="gt", choices=["gt", "detector"],
                    help="person boxes: the labels' (gt) or the model's person detector")
    ap.add_argument("--metric", default="pck", choices=["pck", "oks", "both"],
                    help="pck: slot-wise ADE / PCK; oks: COCO keypoint AP / AP50 / AP75 / AR; both")
    add_pose_nms_arguments(ap)
    add_flip_test_argument(ap)
    args = ap.parse_args(argv)
    if args.boxes == "detector" and args.metric != "oks":
        ap.error("ADE / PCK compare prediction slot p with ground-truth slot p and are not defined for detector "
                 "boxes, which have their own order and count: use --boxes detector --metric oks")
    if args.pose_nms != "off" and args.metric == "pck":
        ap.error("--pose-nms acts on the poses COCO OKS AP scores; ADE / PCK are slot-wise and ignore it: "
                 "use --metric oks or --metric both")
    setup_logging()
    cfg = load_config(args.config)
    device = torch.device(args.device)
    bcfg = cfg["model"]["backbone"]
    thresholds = cfg.get("training", {}).get("pck_thresholds", [0.002, 0.05, 0.2])
    loader = create_optimized_dataloader(args.dataset_dir, batch_size=args.batch_size, split=args.split,
                                         img_size=bcfg["input_size"], grayscale=bcfg.get("in_channels", 3) == 1,
                                         device=device)
    model = load_model(args.model, cfg, device, args.precision)
    flip = {"flip_test": True} if flip_test_enabled(args) else {}   # the key appears only with the option on
    if flip:
        model.flip_test = True
    if args.metric == "pck":
        metrics, n = evaluate(model, loader, thresholds)
        print(json.dumps({"split": args.split, "batches": n, **flip, **metrics}))
        return metrics
    metrics, n, images = evaluate(model, loader, thresholds if args.metric == "both" else None, boxes=args.boxes,
                                  oks=OksEvaluator(), pose_nms=pose_nms_options(args))
    line = {"split": args.split, "batches": n, "boxes": args.boxes, "images": images}
    if args.pose_nms != "off":
        line["pose_nms"] = args.pose_nms
    print(json.dumps({**line, **flip, **metrics}))
    return metrics


if __name__ == "__main__":
    main()
