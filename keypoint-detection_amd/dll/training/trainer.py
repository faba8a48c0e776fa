"""Trainer of the heatmap head on frozen trunk features.

The reference's ``dll.training.Trainer`` signature, checkpoints and history,
driving the native pieces of a top-down training step:

    rows   = the boxes that are not all zero                 (one host sync)
    x      = plan.roi_features(image, boxes, rows)            kpd_roi_features, no_grad
    gt, tw = generate_roi_targets(keypoints, vis, boxes, rows)   kpd_roi_targets
    loss   = model.loss_fn.heatmap_loss(head(x)[0], gt, tw)   head.train(): native fwd + bwd
    loss  += coord_weight * coord_loss(heat, joints in the ROI frame, tw)   coord_weight > 0: kpd_coord_loss
    loss.backward(); optimizer.step()

With ``train_neck=False`` (the default) only ``model.heatmap_head`` is trained:
the optimizer holds its parameters and
nothing else, the rest of the model stays in eval mode, and every epoch ends
with a check that no state tensor outside ``heatmap_head.`` changed.  The
trunk plan is taken from ``model.native_plan(device)`` once per epoch: its
cache key includes the head's parameters, which change every step, so asking
per step would re-pack every weight per step; ``roi_features`` never reads the
(stale) head weights of that plan.

``use_amp=True`` is bf16 mixed precision: the head's three
3x3 convolutions -- which are the step -- multiply bf16-rounded operands with
fp32 accumulation in the forward, the dgrad and the wgrad
(``head.train_precision = "mixed"``); parameters, gradients, optimizer state,
batch norm, the attention blocks, the final 1x1 and the loss stay fp32 (fp32
master weights).  bf16 has fp32's exponent range, so there is no loss scaling
and ``scaler`` is None -- the reference's f16 autocast needs its GradScaler,
this does not.  Checkpoints hold fp32 state only: a run may switch between
the two modes at any ``resume``.  Validation runs the eval head as always.

``coord_weight > 0`` adds the coordinate term on the decoded keypoints
(DESIGN.md §3k): ``SpatialCoordinateLoss`` (smooth-L1, scale 100, threshold 5:
the reference's ImprovedKeypointLoss defaults) of the soft-argmax decode of the
train-mode heatmaps at ``coord_temperature`` -- 1.0, the default, is the eval
forward's own decode, so the term supervises what ``outputs["keypoints"]``
returns -- against each person's joints in their own ROI frame, masked by the
per-joint weight of the heatmap targets, so unlabelled joints, joints outside
their box and padding boxes drop out of both terms alike.  The step's loss is
``heatmap_loss + coord_weight * coord_loss`` with a fixed weight (the
reference's DynamicLossBalancer reads every component on the host each step;
the step keeps its one synchronisation).  Validation then also reports
``coord_loss`` and ``avg_ADE_soft``, the ADE of that soft-argmax decode.  With
``coord_weight == 0`` (default) none of this runs: steps, history keys and
checkpoints are what they were.  Whether the term improves trained accuracy,
and at which weight or temperature, is unmeasured: no dataset run exists.

``train_neck=True`` trains the FPN's level-0 path with the head (DESIGN.md
§3l).  The parts of the neck between the pretrained body and the head -- the
four ``backbone.fpn.lateral_convs`` and ``backbone.fpn.fpn_convs.0`` -- have no
pretrained weights anywhere, so a head-only run fits the head to a random
projection.  The step's ``x`` then comes from ``neck_roi_features`` (frozen
native body taps -> ``fpn.forward_level0`` in train mode -> frozen top-64
indices -> ``dll.ops.roi_align_boxes``, whose backward is the deterministic
kpd_roi_align_backward) instead of the plan, and the optimizer gets a second
parameter group at ``learning_rate * neck_lr_scale`` holding exactly
``backbone.fpn.lateral_convs.{0,1,2,3}.weight``, ``fpn_convs.0.0.weight`` and
``fpn_convs.0.1.{weight,bias}``.  ``backbone.fpn`` is in train mode for the
step and back in eval mode at the epoch's end; the frozen-state check then
allows those seven tensors and the batch norm's three buffers to change and
still covers everything else: the body, ``channel_attention`` (the top-k has no
gradient), ``fpn_convs.1..3`` (not on the heatmap path), the person head.
``use_amp=True`` also runs the level-0 convolution on bf16 operands.
Validation is unchanged: the eval head on the plan's features, the plan
re-taken per epoch and so re-packed from the new FPN weights and statistics.
Checkpoints keep their format; the optimizer state has one more group, so
``resume`` into a trainer with the other ``train_neck`` setting raises.  What
follows from moving level 0: the person detector and KEYPOINT_HEAD read level
0 too, so a detector trained (``DetectorTrainer``) before a neck run must be
retrained after it.  Accuracy stays unmeasured: no dataset run exists.

Out of scope: the visibility term (the head's visibility is a threshold on the
map's maximum and has no gradient), DynamicLossBalancer, coordinate
supervision of the detector or KEYPOINT_HEAD, training the body,
``channel_attention`` (a differentiable top-k), FPN levels 1-3 or
KEYPOINT_HEAD (the person detector has its own trainer, ``DetectorTrainer``
in detector_trainer.py, DESIGN.md §3j;
joint detector + head steps are out of scope of both), ``torch.autocast`` /
``GradScaler`` integration, f16 training, AMP on a CPU device (raises),
multi-GPU training.
"""
from __future__ import annotations

import logging
import time
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch.optim import lr_scheduler

from ..configs.training_config import TrainingConfig
from ..losses.keypoint_loss import SoftArgmaxCoordinateLoss
from ..models.heatmap_head import decode_heatmaps, generate_roi_targets
from ..models.keypoint_model import neck_roi_features
from ..utils.metric import _metrics_on_device

logger = logging.getLogger(__name__)

HEAD_PREFIX = "heatmap_head."
NECK_PREFIX = "backbone.fpn."
TARGET_SIGMA = 2.0   # the reference's _convert_keypoints_to_heatmaps


def batch_boxes(batch: Dict) -> torch.Tensor:
    """The [B, P, 4] box tensor of a collated batch (``efficient_collate_fn`` wraps it in a list)."""
    bb = batch["bboxes"]
    bb = bb[0] if isinstance(bb, (list, tuple)) else bb
    if bb.dim() != 3 or bb.size(-1) != 4:
        raise ValueError(f"bboxes must be [B, P, 4], got {tuple(bb.shape)}")
    return bb


class Trainer:
    def __init__(self, model: nn.Module, device: torch.device, train_dataloader, val_dataloader,
                 config: TrainingConfig, output_dir: Optional[Union[str, Path]] = None, use_amp: bool = False,
                 coord_weight: float = 0.0, coord_temperature: float = 1.0, train_neck: bool = False,
                 neck_lr_scale: float = 1.0):
        if not (0.0 <= float(coord_weight) < float("inf")):
            raise ValueError(f"coord_weight must be finite and >= 0, got {coord_weight}")
        if not (0.0 < float(coord_temperature) < float("inf")):
            raise ValueError(f"coord_temperature must be positive and finite, got {coord_temperature}")
        if use_amp and torch.device(device).type != "cuda":
            raise NotImplementedError("AMP training runs on the native bf16 kernels of the heatmap head's train path "
                                      "(DESIGN.md §3i), which need a GPU device; construct the Trainer with "
                                      "use_amp=False")
        if not (0.0 < float(neck_lr_scale) < float("inf")):
            raise ValueError(f"neck_lr_scale must be positive and finite, got {neck_lr_scale}")
        if train_neck and torch.device(device).type != "cuda":
            raise NotImplementedError("train_neck runs the FPN's level-0 path on the native conv3x3, batch-norm and "
                                      "ROI-align backward kernels (DESIGN.md §3l), which need a GPU device; construct "
                                      "the Trainer with train_neck=False")
        if not hasattr(model, "heatmap_head"):
            raise TypeError("Trainer trains model.heatmap_head; pass a MultiPersonKeypointModel")
        if train_neck and not hasattr(getattr(model, "backbone", None), "fpn"):
            raise TypeError("train_neck trains model.backbone.fpn; pass a MultiPersonKeypointModel")
        self.device = torch.device(device)
        self.model = model.to(self.device)
        self.head = self.model.heatmap_head
        self.train_dataloader = train_dataloader
        self.val_dataloader = val_dataloader
        self.config = config
        self.output_dir = Path(output_dir) if output_dir else None
        if self.output_dir:
            self.output_dir.mkdir(parents=True, exist_ok=True)
        # bf16 operands in the head's 3x3 convolutions, fp32 everything else; no loss scaling (module docstring)
        self.use_amp = bool(use_amp)
        self.scaler = None
        self.head.train_precision = "mixed" if self.use_amp else "split"
        # the coordinate term on the decoded keypoints (module docstring); 0: never built, never launched
        self.coord_weight = float(coord_weight)
        self.coord_temperature = float(coord_temperature)
        self.coord_loss_fn = SoftArgmaxCoordinateLoss(self.coord_temperature) if self.coord_weight > 0 else None
        # the FPN's level-0 path trained with the head (module docstring); False: never touched
        self.train_neck = bool(train_neck)
        self.neck_lr_scale = float(neck_lr_scale)
        self.model.eval()
        self.optimizer = self._create_optimizer()
        sc = config.lr_scheduler
        self.scheduler = lr_scheduler.ReduceLROnPlateau(self.optimizer, mode=str(sc.mode), factor=float(sc.factor),
                                                        patience=int(sc.patience), min_lr=float(sc.min_lr),
                                                        threshold=float(sc.threshold))
        self.scheduler_metric = str(sc.metric)
        self.pck_thresholds = [float(t) for t in config.pck_thresholds]
        self.history: Dict[str, List] = {}
        self.epoch = 0               # epochs completed
        self.best_val_loss = float("inf")
        self.max_steps: Optional[int] = None   # per epoch (scripts/train.py --max-steps)
        self._plan = None

    # ------------------------------------------------------------------ setup
    def _create_optimizer(self) -> torch.optim.Optimizer:
        oc = self.config.optimizer
        params = list(self.head.parameters())
        if self.train_neck:   # a second group: exactly the parameters on the level-0 path, at their own rate
            params = [{"params": params},
                      {"params": [p for _, p in self.neck_parameters()],
                       "lr": float(oc.learning_rate) * self.neck_lr_scale}]
        name = str(oc.name).lower()
        if name == "adam":
            return torch.optim.Adam(params, lr=float(oc.learning_rate), betas=(float(oc.beta1), float(oc.beta2)),
                                    weight_decay=float(oc.weight_decay))
        if name == "sgd":
            return torch.optim.SGD(params, lr=float(oc.learning_rate), momentum=float(oc.momentum),
                                   weight_decay=float(oc.weight_decay))
        raise ValueError(f"Unsupported optimizer: {oc.name}")

    def neck_parameters(self) -> List[Tuple[str, nn.Parameter]]:
        """(state-dict name, parameter) of the parameters on the FPN's level-0 path, in a fixed order."""
        fpn = self.model.backbone.fpn
        named = dict(fpn.named_parameters())
        return [(NECK_PREFIX + k, named[k]) for k in fpn.LEVEL0_PARAMETERS]

    def _trained_names(self) -> set:
        """State tensors outside ``heatmap_head.`` that an epoch may change."""
        if not self.train_neck:
            return set()
        fpn = self.model.backbone.fpn
        return {NECK_PREFIX + k for k in fpn.LEVEL0_PARAMETERS + fpn.LEVEL0_BUFFERS}

    def _frozen_versions(self) -> Dict[str, Tuple[int, int]]:
        free = self._trained_names()
        return {k: (t.data_ptr(), t._version) for k, t in self.model.state_dict(keep_vars=True).items()
                if not k.startswith(HEAD_PREFIX) and k not in free}

    def trunk_plan(self):
        """The model's plan, taken once per epoch (module docstring)."""
        if self._plan is None:
            self._plan = self.model.native_plan(self.device)
        return self._plan

    # ------------------------------------------------------------------ one batch
    def _features_and_targets(self, batch: Dict, through_neck: bool = False):
        """(x [n,64,56,56], gt [n,K,H,W], tw [n,K], rows [n] int32, boxes [B,P,4]) or None without a
        labelled box.  The nonzero() below is the step's one host synchronisation.  ``through_neck``
        (the train step of train_neck): x from neck_roi_features, with a gradient to the FPN's level-0
        path; otherwise the plan's frozen features."""
        image = batch["image"].to(self.device)
        boxes = batch_boxes(batch).to(self.device, torch.float32).contiguous()
        rows = torch.nonzero((boxes != 0).any(dim=-1).flatten()).flatten().to(torch.int32)   # ascending
        if rows.numel() == 0:
            return None
        if through_neck:
            x = neck_roi_features(self.model, image, boxes, rows, "mixed" if self.use_amp else "split")
        else:
            with torch.no_grad():
                x = self.trunk_plan().roi_features(image, boxes, rows)
        kp = batch["keypoints"].to(self.device, torch.float32)
        vis = batch["visibilities"].to(self.device, torch.float32)
        # the head keeps its input's spatial size (config.heatmap_size is unused by it, a reference quirk)
        gt, tw = generate_roi_targets(kp, vis, boxes, rows, tuple(x.shape[2:]), TARGET_SIGMA)
        return x, gt, tw, rows, boxes

    def _roi_joints(self, batch: Dict, rows: torch.Tensor, boxes: torch.Tensor, K: int):
        """Each person's joints [n,K,2] in their own ROI's frame, (kp - (c - wh/2)) / wh: the inverse of
        validate_epoch's mapping.  An empty side gives inf / NaN, which the target weight of that ROI (0)
        masks.  Device indexing, no host synchronisation."""
        kp = batch["keypoints"].to(self.device, torch.float32).reshape(-1, K, 2)[rows.long()]
        b = boxes.view(-1, 4)[rows.long()].unsqueeze(1)
        return (kp - (b[..., :2] - b[..., 2:] / 2)) / b[..., 2:]

    def train_step(self, batch: Dict) -> Dict:
        """One optimizer step on a collated batch: {'loss': 0-d device tensor
        (detached), 'rows': n, 'skipped': bool}; with coord_weight > 0 'loss'
        is the total and 'heatmap_loss' / 'coord_loss' its two parts.  A batch
        without a labelled box is skipped (no step, loss None)."""
        if self.train_neck:
            self.model.backbone.fpn.train()
        ft = self._features_and_targets(batch, through_neck=self.train_neck)
        if ft is None:
            return {"loss": None, "rows": 0, "skipped": True}
        x, gt, tw, rows, boxes = ft
        self.head.train()
        self.optimizer.zero_grad(set_to_none=True)
        heat = self.head(x)[0]
        loss = self.model.loss_fn.heatmap_loss(heat, gt, tw)
        parts = {}
        if self.coord_loss_fn is not None:
            coord = self.coord_loss_fn(heat, self._roi_joints(batch, rows, boxes, heat.size(1)), tw)
            parts = {"heatmap_loss": loss.detach(), "coord_loss": coord.detach()}
            loss = loss + self.coord_weight * coord
        loss.backward()
        self.optimizer.step()
        return {"loss": loss.detach(), "rows": int(rows.numel()), "skipped": False, **parts}

    def train_epoch(self) -> Dict[str, float]:
        self._plan = None
        self.model.eval()
        before = self._frozen_versions()
        losses, steps, skipped = [], 0, 0
        for batch in self.train_dataloader:
            if self.max_steps is not None and steps + skipped >= self.max_steps:
                break
            out = self.train_step(batch)
            if out["skipped"]:
                skipped += 1
                continue
            steps += 1
            losses.append(out["loss"])
        self.head.eval()
        if self.train_neck:
            self.model.backbone.fpn.eval()
        changed = [k for k, v in self._frozen_versions().items() if before.get(k) != v]
        what = f"{HEAD_PREFIX} and the FPN's level-0 path" if self.train_neck else HEAD_PREFIX
        assert not changed, f"state outside {what} changed during the epoch: {changed[:5]}"
        loss = float(torch.stack(losses).double().mean()) if losses else 0.0
        return {"loss": loss, "steps": steps, "skipped_steps": skipped}

    def validate_epoch(self) -> Dict[str, float]:
        """Mean loss, ADE and PCK over the validation batches with a labelled
        box: the head in eval mode through its own plan on the same features
        and targets; the heatmaps argmax-decoded and mapped to image
        coordinates through the unclamped box, against the labelled joints.
        With coord_weight > 0 also the coordinate term (``coord_loss``; ``loss``
        stays the heatmap term) and ``avg_ADE_soft``, the ADE of the soft-argmax
        decode at coord_temperature."""
        self._plan = None
        self.model.eval()
        names = ["loss", "avg_ADE"] + [f"pck_{t}" for t in self.config.pck_thresholds]
        if self.coord_loss_fn is not None:
            names += ["coord_loss", "avg_ADE_soft"]
        sums, n = dict.fromkeys(names, 0.0), 0
        with torch.no_grad():
            for batch in self.val_dataloader:
                if self.max_steps is not None and n >= self.max_steps:
                    break
                ft = self._features_and_targets(batch)
                if ft is None:
                    continue
                x, gt, tw, rows, boxes = ft
                heat = self.head(x)[0]
                loss = self.model.loss_fn.heatmap_loss(heat, gt, tw)
                kp_roi, _ = decode_heatmaps(heat)                                   # [n, K, 2] in the ROI's frame
                b = boxes.view(-1, 4)[rows.long()].unsqueeze(1)                     # [n, 1, 4]
                pred = kp_roi * b[..., 2:] + (b[..., :2] - b[..., 2:] / 2)           # unclamped box
                K = heat.size(1)
                want = batch["keypoints"].to(self.device, torch.float32).reshape(-1, K, 2)[rows.long()]
                vis = batch["visibilities"].to(self.device, torch.float32).reshape(-1, K)[rows.long()]
                vals = _metrics_on_device(pred, want, vis, self.pck_thresholds)
                if self.coord_loss_fn is not None:
                    coord = self.coord_loss_fn(heat, self._roi_joints(batch, rows, boxes, K), tw)
                    soft = self.coord_loss_fn.last_coords * b[..., 2:] + (b[..., :2] - b[..., 2:] / 2)
                    vals = vals + [float(coord), _metrics_on_device(soft, want, vis, self.pck_thresholds)[0]]
                for name, v in zip(names, [float(loss)] + vals):
                    sums[name] += float(v)
                n += 1
        return {k: v / max(n, 1) for k, v in sums.items()}

    # ------------------------------------------------------------------ checkpoints
    def _checkpoint(self, epoch: int) -> Dict:
        return {"epoch": int(epoch), "model_state_dict": self.model.state_dict(),
                "optimizer_state_dict": self.optimizer.state_dict(),
                "history": {k: list(v) for k, v in self.history.items()}}

    def save_checkpoint(self, epoch: int, is_best: bool = False, periodic: bool = True) -> None:
        if not self.output_dir:
            return
        ckpt = self._checkpoint(epoch)
        if periodic:
            torch.save(ckpt, self.output_dir / f"checkpoint_epoch_{epoch}.pth")
        if is_best:
            torch.save(ckpt, self.output_dir / "best_model.pth")

    def resume(self, path: Union[str, Path]) -> int:
        """Restore the model, the optimizer, the epoch and the history; returns the epochs completed."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        groups = len(ckpt["optimizer_state_dict"]["param_groups"])
        if groups != len(self.optimizer.param_groups):
            was, now = groups > 1, self.train_neck
            raise ValueError(f"{path}: the checkpoint's optimizer holds {groups} parameter group(s) (written with "
                             f"train_neck={was}) and this trainer {len(self.optimizer.param_groups)} "
                             f"(train_neck={now}); resume with the train_neck setting of the run that wrote it")
        self.model.load_state_dict(ckpt["model_state_dict"])
        self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        self.history = {k: list(v) for k, v in ckpt.get("history", {}).items()}
        self.epoch = int(ckpt["epoch"])
        if self.history.get("loss"):
            self.best_val_loss = min(self.history["loss"])
        self._plan = None
        return self.epoch

    # ------------------------------------------------------------------ loop
    def _scheduler_value(self, val: Dict[str, float]) -> float:
        return float(val.get(self.scheduler_metric, val["loss"]))

    def _record(self, epoch: int, train: Dict[str, float], val: Dict[str, float], lr: float, seconds: float) -> Dict:
        line = {"epoch": int(epoch), "train_loss": float(train["loss"]), "loss": float(val["loss"]),
                "avg_ADE": float(val["avg_ADE"])}
        line.update({k: float(v) for k, v in val.items() if k.startswith("pck_")})
        line.update({k: float(val[k]) for k in ("coord_loss", "avg_ADE_soft") if k in val})
        line.update({"learning_rate": float(lr), "steps": int(train["steps"]),
                     "skipped_steps": int(train["skipped_steps"]), "seconds": float(seconds)})
        for k, v in line.items():
            self.history.setdefault(k, []).append(v)
        return line

    def train(self, on_epoch=None) -> Tuple[nn.Module, Dict]:
        """Epochs ``self.epoch + 1 .. config.num_epochs``; ``on_epoch(line)``
        receives each epoch's record (plain Python numbers).  Returns the model
        and the history."""
        for epoch in range(self.epoch + 1, int(self.config.num_epochs) + 1):
            t0 = time.perf_counter()
            train = self.train_epoch()
            val = self.validate_epoch()
            self.scheduler.step(self._scheduler_value(val))
            lr = self.optimizer.param_groups[0]["lr"]
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            line = self._record(epoch, train, val, lr, time.perf_counter() - t0)
            self.epoch = epoch
            is_best = val["loss"] < self.best_val_loss
            if is_best:
                self.best_val_loss = val["loss"]
            interval = max(1, int(self.config.checkpoint_interval))
            self.save_checkpoint(epoch, is_best=is_best, periodic=epoch % interval == 0)
            soft = "  coord loss %.6f  soft ADE %.5f" % (val["coord_loss"], val["avg_ADE_soft"]) \
                if "coord_loss" in val else ""
            logger.info("epoch %d: train loss %.6f  val loss %.6f  ADE %.5f%s  lr %.2e", epoch, train["loss"],
                        val["loss"], val["avg_ADE"], soft, lr)
            if on_epoch is not None:
                on_epoch(line)
        return self.model, self.history
