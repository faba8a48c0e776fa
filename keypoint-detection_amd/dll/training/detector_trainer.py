"""Trainer of the person detector on frozen trunk features.

``Trainer``'s constructor shape, checkpoint dict, history and ``resume``,
driving the native pieces of a detector training step:

    x    = plan.detector_features(image)                   kpd_detector_features, no_grad
    loss = DetectionLoss(person_head, x, boxes, (H, W))    kpd_detector_targets + kpd_detector_loss
    loss.backward(); optimizer.step()

Only ``person_detector.box_heads.0`` and ``person_detector.cls_heads.0`` are
trained -- 5,805 parameters, the only ones the eval detector reads: the
optimizer holds them and nothing else, the model stays in eval mode, and every
epoch ends with ``Trainer``'s check that no other state tensor changed.  The
step has no host synchronisation: the matching, the positive count N and the
loss stay on the device, and a batch without a labelled box still steps (every
anchor a negative, N = 1).  The trunk plan is taken once per epoch, as
``Trainer`` takes it: ``detector_features`` never reads the (stale) head
weights of that plan.  Validation reports the loss, its two parts and
``recall_50``: the share of labelled boxes that some box kept by the eval
detector (``model`` without ``bboxes``; its plan re-packs, the cache key
includes the parameters) overlaps at IoU >= 0.5.

The rules are build-defined (the reference has no detector training); parity
with any external detector trainer is unpinned, and accuracy is unmeasured: no
dataset run exists.

Out of scope: training the trunk or KEYPOINT_HEAD, heads 1-3 of ``box_heads`` /
``cls_heads`` (the forward never reads them), joint detector + heatmap-head
steps, hard-negative mining, IoU-based box losses, AMP (the step has no
MFMA-bound part to speed up), multi-GPU training.
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
from ..losses.detection_loss import DetectionLoss
from .trainer import batch_boxes

logger = logging.getLogger(__name__)

DETECTOR_PREFIXES = ("person_detector.box_heads.0.", "person_detector.cls_heads.0.")
MAX_GT = 64   # kpd_detector_targets' ground-truth slots per image


class DetectorTrainer:
    def __init__(self, model: nn.Module, device: torch.device, train_dataloader, val_dataloader,
                 config: TrainingConfig, output_dir: Optional[Union[str, Path]] = None, use_amp: bool = False,
                 loss_fn: Optional[DetectionLoss] = None):
        if use_amp:
            raise NotImplementedError("the detector step has no MFMA-bound part for mixed precision to speed up; "
                                      "construct the DetectorTrainer with use_amp=False")
        if not hasattr(model, "person_detector"):
            raise TypeError("DetectorTrainer trains model.person_detector; pass a MultiPersonKeypointModel")
        self.device = torch.device(device)
        self.model = model.to(self.device)
        self.head = self.model.person_detector
        self.loss_fn = loss_fn or DetectionLoss()
        self.train_dataloader = train_dataloader
        self.val_dataloader = val_dataloader
        self.config = config
        self.output_dir = Path(output_dir) if output_dir else None
        if self.output_dir:
            self.output_dir.mkdir(parents=True, exist_ok=True)
        self.use_amp = False
        self.scaler = None
        self.model.eval()
        self.optimizer = self._create_optimizer()
        sc = config.lr_scheduler
        self.scheduler = lr_scheduler.ReduceLROnPlateau(self.optimizer, mode=str(sc.mode), factor=float(sc.factor),
                                                        patience=int(sc.patience), min_lr=float(sc.min_lr),
                                                        threshold=float(sc.threshold))
        self.scheduler_metric = str(sc.metric)
        self.history: Dict[str, List] = {}
        self.epoch = 0               # epochs completed
        self.best_val_loss = float("inf")
        self.max_steps: Optional[int] = None   # per epoch (scripts/train.py --max-steps)
        self._plan = None

    # ------------------------------------------------------------------ setup
    def trained_parameters(self) -> List[nn.Parameter]:
        return list(self.head.box_heads[0].parameters()) + list(self.head.cls_heads[0].parameters())

    def _create_optimizer(self) -> torch.optim.Optimizer:
        oc = self.config.optimizer
        params = self.trained_parameters()
        name = str(oc.name).lower()
        if name == "adam":
            return torch.optim.Adam(params, lr=float(oc.learning_rate), betas=(float(oc.beta1), float(oc.beta2)),
                                    weight_decay=float(oc.weight_decay))
        if name == "sgd":
            return torch.optim.SGD(params, lr=float(oc.learning_rate), momentum=float(oc.momentum),
                                   weight_decay=float(oc.weight_decay))
        raise ValueError(f"Unsupported optimizer: {oc.name}")

    def _frozen_versions(self) -> Dict[str, Tuple[int, int]]:
        return {k: (t.data_ptr(), t._version) for k, t in self.model.state_dict(keep_vars=True).items()
                if not k.startswith(DETECTOR_PREFIXES)}

    def trunk_plan(self):
        """The model's plan, taken once per epoch (module docstring)."""
        if self._plan is None:
            self._plan = self.model.native_plan(self.device)
        return self._plan

    # ------------------------------------------------------------------ one batch
    def _features_and_boxes(self, batch: Dict):
        """(x [B,3136,128], boxes [B,G,4], (H, W)); no host synchronisation."""
        image = batch["image"].to(self.device)
        boxes = batch_boxes(batch).to(self.device, torch.float32).contiguous()
        if boxes.size(0) != image.size(0):
            raise ValueError(f"bboxes describe {boxes.size(0)} images but the batch has {image.size(0)}")
        if boxes.size(1) > MAX_GT:
            raise ValueError(f"{boxes.size(1)} box slots per image; the detector matching takes at most {MAX_GT}")
        with torch.no_grad():
            x = self.trunk_plan().detector_features(image)
        return x, boxes, tuple(image.shape[2:])

    def train_step(self, batch: Dict) -> Dict:
        """One optimizer step on a collated batch: {'loss', 'cls_loss',
        'box_loss': 0-d device tensors (detached), 'n_pos': [B] int32 device
        tensor, 'skipped': False}."""
        x, boxes, size = self._features_and_boxes(batch)
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.loss_fn(self.head, x, boxes, size)
        loss.backward()
        self.optimizer.step()
        return {"loss": loss.detach(), "cls_loss": loss.cls_part, "box_loss": loss.box_part, "n_pos": loss.n_pos,
                "skipped": False}

    def train_epoch(self) -> Dict[str, float]:
        self._plan = None
        self.model.eval()
        before = self._frozen_versions()
        losses, steps = [], 0
        for batch in self.train_dataloader:
            if self.max_steps is not None and steps >= self.max_steps:
                break
            losses.append(self.train_step(batch)["loss"])
            steps += 1
        changed = [k for k, v in self._frozen_versions().items() if before.get(k) != v]
        assert not changed, f"state outside {DETECTOR_PREFIXES} changed during the epoch: {changed[:5]}"
        loss = float(torch.stack(losses).double().mean()) if losses else 0.0
        return {"loss": loss, "steps": steps, "skipped_steps": 0}

    def validate_epoch(self) -> Dict[str, float]:
        """Mean loss and parts over the validation batches, and recall_50 over
        their labelled boxes (1.0 when there is none) against the boxes the
        eval detector keeps."""
        self._plan = None
        self.model.eval()
        sums, n = torch.zeros(3, dtype=torch.float64, device=self.device), 0
        hit = torch.zeros((), dtype=torch.int64, device=self.device)
        total = torch.zeros((), dtype=torch.int64, device=self.device)
        with torch.no_grad():
            for batch in self.val_dataloader:
                if self.max_steps is not None and n >= self.max_steps:
                    break
                x, boxes, size = self._features_and_boxes(batch)
                loss = self.loss_fn(self.head, x, boxes, size)
                sums += torch.stack([loss, loss.cls_part, loss.box_part]).double()
                det = self.model({"image": batch["image"].to(self.device)})["boxes"]    # the eval detector
                for b in range(boxes.size(0)):
                    gt = boxes[b][(boxes[b] != 0).any(dim=-1) & (boxes[b][:, 2] > 0) & (boxes[b][:, 3] > 0)]
                    kept = det[b][(det[b] != 0).any(dim=-1)]
                    total += gt.size(0)
                    if gt.size(0) and kept.size(0):
                        hit += (self.head.box_iou(gt, kept).max(dim=1).values >= 0.5).sum()
                n += 1
        self._plan = None   # (the eval forwards re-packed the model's plan; take it afresh next epoch)
        loss, cls_loss, box_loss = (float(v) / max(n, 1) for v in sums.cpu())
        total = int(total)
        return {"loss": loss, "cls_loss": cls_loss, "box_loss": box_loss,
                "recall_50": float(int(hit)) / total if total else 1.0}

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
                "cls_loss": float(val["cls_loss"]), "box_loss": float(val["box_loss"]),
                "recall_50": float(val["recall_50"]), "learning_rate": float(lr), "steps": int(train["steps"]),
                "skipped_steps": int(train["skipped_steps"]), "seconds": float(seconds)}
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
            logger.info("epoch %d: train loss %.6f  val loss %.6f (class %.6f, box %.6f)  recall@0.5 %.4f  lr %.2e",
                        epoch, train["loss"], val["loss"], val["cls_loss"], val["box_loss"], val["recall_50"], lr)
            if on_epoch is not None:
                on_epoch(line)
        return self.model, self.history
