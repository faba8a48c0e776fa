#!/usr/bin/env python3
"""Train the heatmap head on frozen trunk features (``dll.training.Trainer``,
DESIGN.md §3h) on a YOLO-pose dataset with ``train`` and ``val`` splits:
decode (host) -> augmentation + ITransform (device) -> collate ->
kpd_roi_features + kpd_roi_targets -> HeatmapHead train step -> checkpoints.

    python scripts/train.py --config configs/default_config.yaml --data_dir data/ \
        --output_dir runs/head [--model best_model.pth|synthetic] [--resume runs/head/checkpoint_epoch_5.pth] \
        [--epochs N] [--batch-size N] [--max-steps N] [--seed S] [--augment] [--precision split|fp32|mixed] [--amp] \
        [--train heatmap_head|detector] [--coord-weight W] [--coord-temperature T] \
        [--train-neck] [--neck-lr-scale S]

``--model`` gives the starting weights (a checkpoint, or ``synthetic`` for the
seeded synthetic state dict; default: the freshly initialised model);
``--resume`` continues a run from one of its checkpoints (model, optimizer,
epoch, history).  ``--max-steps`` bounds the batches of every train and
validation epoch.  ``--amp`` trains in bf16 mixed precision
(``Trainer(use_amp=True)``: bf16 operands in the head's 3x3 convolutions, fp32
master weights, no loss scaling); ``--precision`` is the plan's, for the trunk
features and validation.  One JSON line per epoch goes to stdout: epoch, train_loss,
loss (validation), avg_ADE, pck_*, learning_rate, steps, skipped_steps, seconds.
``--coord-weight W`` (W > 0) adds W x the coordinate loss of the soft-argmax
decoded keypoints to every step (``Trainer(coord_weight=W)``);
the line then also holds coord_loss and avg_ADE_soft (validation).  It is an
error with ``--train detector``.
``--train-neck`` trains the FPN's level-0 path (``backbone.fpn.lateral_convs``
and ``fpn_convs.0``, which have no pretrained weights) together with the head
(``Trainer(train_neck=True)``), at ``--neck-lr-scale`` times the
head's learning rate; the body and ``channel_attention`` stay frozen.  A
detector trained before such a run must be retrained after it (it reads level
0 too).  Both are an error with ``--train detector``.

``--train detector`` trains the person detector instead (``DetectorTrainer``,
DESIGN.md §3j: kpd_detector_features -> anchor matching + focal / smooth-L1 loss
-> step on ``person_detector.box_heads.0`` / ``cls_heads.0``), on the same
dataset's boxes; its JSON line holds epoch, train_loss, loss, cls_loss,
box_loss, recall_50, learning_rate, steps, skipped_steps, seconds, and its
checkpoints load in predict.py / evaluate.py like any other.  ``--amp`` with it
is an error: the step has no MFMA-bound part to speed up.
Every argument is checked before the device is touched.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def training_config_from_dict(d):
    """A ``TrainingConfig`` from the YAML ``training`` block (nested blocks become their dataclasses)."""
    from dll.configs.base_config import DeviceConfig
    from dll.configs.training_config import (AugmentationConfig, LossConfig, LRSchedulerConfig, OptimizerConfig,
                                             TrainingConfig)
    nested = {"optimizer": OptimizerConfig, "augmentation": AugmentationConfig, "loss": LossConfig,
              "lr_scheduler": LRSchedulerConfig, "device": DeviceConfig}
    kw = {}
    for k, v in (d or {}).items():
        kw[k] = nested[k](**v) if k in nested and isinstance(v, dict) else v
    return TrainingConfig(**kw)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Train the heatmap head on frozen trunk features")
    ap.add_argument("--config", required=True)
    ap.add_argument("--data_dir", "--data-dir", dest="data_dir", required=True)
    ap.add_argument("--output_dir", "--output-dir", dest="output_dir", required=True)
    ap.add_argument("--resume", default=None, help="checkpoint of this run to continue from")
    ap.add_argument("--model", default=None, help="starting weights: a checkpoint path, or 'synthetic'")
    ap.add_argument("--epochs", type=int, default=None, help="overrides training.num_epochs")
    ap.add_argument("--batch-size", type=int, default=None, help="overrides training.batch_size")
    ap.add_argument("--max-steps", type=int, default=None, help="batches per train / validation epoch")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--augment", action="store_true", help="augment the train split (also: augmentation.enabled)")
    ap.add_argument("--precision", default="split", choices=["split", "fp32", "mixed"])
    ap.add_argument("--amp", action="store_true", help="bf16 mixed-precision training (Trainer use_amp=True)")
    ap.add_argument("--coord-weight", type=float, default=0.0,
                    help="weight of the coordinate term on the soft-argmax decoded keypoints (0: off)")
    ap.add_argument("--coord-temperature", type=float, default=1.0,
                    help="soft-argmax temperature of that term (1.0: the eval forward's decode)")
    ap.add_argument("--train-neck", action="store_true",
                    help="also train the FPN's level-0 path under the head (Trainer train_neck=True)")
    ap.add_argument("--neck-lr-scale", type=float, default=None,
                    help="learning rate of the neck's parameters relative to the head's (default 1.0)")
    ap.add_argument("--train", default="heatmap_head", choices=["heatmap_head", "detector"],
                    help="what to train on the frozen trunk (default: the heatmap head)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.train == "detector" and args.amp:
        ap.error("--amp does not apply to --train detector: the step has no MFMA-bound part to speed up")
    if not (0.0 <= args.coord_weight < float("inf")):
        ap.error("--coord-weight must be finite and >= 0")
    if not (0.0 < args.coord_temperature < float("inf")):
        ap.error("--coord-temperature must be positive and finite")
    if args.train == "detector" and args.coord_weight > 0:
        ap.error("--coord-weight does not apply to --train detector: the detector has no keypoint output")
    if args.train == "detector" and (args.train_neck or args.neck_lr_scale is not None):
        ap.error("--train-neck / --neck-lr-scale do not apply to --train detector: the detector's trainer keeps "
                 "the whole trunk frozen")
    if args.neck_lr_scale is not None and not args.train_neck:
        ap.error("--neck-lr-scale needs --train-neck")
    if args.neck_lr_scale is not None and not (0.0 < args.neck_lr_scale < float("inf")):
        ap.error("--neck-lr-scale must be positive and finite")
    for name in ("epochs", "batch_size", "max_steps"):
        v = getattr(args, name)
        if v is not None and v < 1:
            ap.error(f"--{name.replace('_', '-')} must be at least 1")
    if not Path(args.config).is_file():
        ap.error(f"--config: no such file: {args.config}")
    for split in ("train", "val"):
        for sub in ("images", "labels"):
            if not (Path(args.data_dir) / split / sub).is_dir():
                ap.error(f"--data_dir: {Path(args.data_dir) / split / sub} not found "
                         "(expected <data_dir>/{train,val}/{images,labels})")
    if args.resume is not None and not Path(args.resume).is_file():
        ap.error(f"--resume: no such checkpoint: {args.resume}")
    if args.model is not None and args.model != "synthetic" and not Path(args.model).is_file():
        ap.error(f"--model: no such checkpoint: {args.model} (or 'synthetic')")
    if args.resume is not None and args.model is not None:
        ap.error("--resume restores the model from its checkpoint; do not combine it with --model")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    from dll.data import KeypointAugmentation, create_optimized_dataloader
    from dll.training import DetectorTrainer, Trainer
    from predict import load_config, load_model, setup_logging
    setup_logging()
    cfg = load_config(args.config)
    tcfg = training_config_from_dict(cfg.get("training"))
    if args.epochs is not None:
        tcfg.num_epochs = args.epochs
    if args.batch_size is not None:
        tcfg.batch_size = args.batch_size
    torch.manual_seed(args.seed)
    device = torch.device(args.device)
    bcfg = cfg["model"]["backbone"]
    aug = KeypointAugmentation(tcfg, seed=args.seed, device=device) if args.augment or tcfg.augmentation.enabled \
        else None
    if aug is not None:
        tcfg.augmentation.enabled = True
    common = dict(batch_size=tcfg.batch_size, num_workers=0, img_size=bcfg["input_size"],
                  grayscale=bcfg.get("in_channels", 3) == 1, device=device)
    train_dl = create_optimized_dataloader(args.data_dir, split="train", augmentation=aug, **common)
    val_dl = create_optimized_dataloader(args.data_dir, split="val", **common)
    if args.model is None:   # the seeded initialisation, built as load_model builds its model
        model = _fresh_model(cfg, device, args.precision)
    else:
        model = load_model(args.model, cfg, device, args.precision)
    if args.train == "detector":
        trainer = DetectorTrainer(model, device, train_dl, val_dl, tcfg, output_dir=args.output_dir)
    else:
        trainer = Trainer(model, device, train_dl, val_dl, tcfg, output_dir=args.output_dir, use_amp=args.amp,
                          coord_weight=args.coord_weight, coord_temperature=args.coord_temperature,
                          train_neck=args.train_neck,
                          neck_lr_scale=1.0 if args.neck_lr_scale is None else args.neck_lr_scale)
    trainer.max_steps = args.max_steps
    if args.resume is not None:
        trainer.resume(args.resume)
    _, history = trainer.train(on_epoch=lambda line: print(json.dumps(line), flush=True))
    return history


def _fresh_model(cfg, device, precision):
    from dll.configs import BackboneConfig, KeypointHeadConfig, ModelConfig, PersonDetectionConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    mc = cfg["model"]
    model_config = ModelConfig(backbone=BackboneConfig(**mc["backbone"]),
                               person_head=PersonDetectionConfig(**mc["person_head"]),
                               keypoint_head=KeypointHeadConfig(**mc["keypoint_head"]),
                               num_keypoints=mc["keypoint_head"]["num_keypoints"])
    return MultiPersonKeypointModel(model_config, TrainingConfig(), precision=precision).to(device).eval()


if __name__ == "__main__":
    main()
