"""dll.training.DetectorTrainer on the device: one train_step
against the float64 replica (tests/det_train_ref.py) fed with the device's own
pooled features, run-to-run bit-identity from one seed, which state an epoch
touches, a batch without a labelled box, and scripts/train.py --train detector
end to end on a five-image dataset (checkpoint, predict and evaluate on it)."""
import contextlib
import io
import json
import sys

import numpy as np
import pytest
import torch

import det_train_ref as R
from conftest import PKG
from det_train_cases import MAIN_SIZE, main_boxes
from test_trainer import _write_dataset

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CONFIG = str(PKG / "configs" / "default_config.yaml")
HEADS = ("person_detector.box_heads.0.weight", "person_detector.box_heads.0.bias",
         "person_detector.cls_heads.0.weight", "person_detector.cls_heads.0.bias")
LR = 1e-3


def make_batch(labelled=True):
    """The main fixture of test_det_train.py as a collated batch on the CPU."""
    from dll.models.synthetic import synthetic_images
    boxes = main_boxes() if labelled else torch.zeros(2, 3, 4)
    return {"image": synthetic_images(2, 3, *MAIN_SIZE, seed=1234), "bboxes": [boxes]}


def _to_dev(batch):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in batch.items()}


def _trainer(sd, optimizer, train=(), val=()):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.configs.training_config import OptimizerConfig
    from dll.models import MultiPersonKeypointModel
    from dll.training import DetectorTrainer
    cfg = TrainingConfig(optimizer=OptimizerConfig(**optimizer))
    model = MultiPersonKeypointModel(ModelConfig(), cfg)
    model.load_state_dict(sd)
    return DetectorTrainer(model, DEV, list(train), list(val), cfg)


def test_the_optimizer_holds_the_two_heads_only(model_sd):
    tr = _trainer(model_sd, dict(name="sgd", learning_rate=LR))
    params = [p for g in tr.optimizer.param_groups for p in g["params"]]
    assert sum(p.numel() for p in params) == 5805
    want = {k: v for k, v in tr.model.state_dict(keep_vars=True).items() if k in HEADS}
    assert {p.data_ptr() for p in params} == {v.data_ptr() for v in want.values()}
    from dll.training import DetectorTrainer
    with pytest.raises(NotImplementedError):
        DetectorTrainer(tr.model, DEV, [], [], tr.config, use_amp=True)


def test_train_step_matches_the_float64_replica(model_sd):
    """Plain SGD (momentum 0, weight decay 0), one step: the loss, its parts and the four updated tensors
    against the float64 replica on the device's own pooled features, under test_det_train.py's rule (4 x the
    error of the same formulas by torch in fp32 on the CPU, floor 8 fp32 ulps of max|ref|)."""
    from test_det_train import _check
    tr = _trainer(model_sd, dict(name="sgd", learning_rate=LR, momentum=0.0, weight_decay=0.0))
    batch = _to_dev(make_batch())
    x, boxes, size = tr._features_and_boxes(batch)
    assert tuple(x.shape) == (2, 3136, 128) and size == MAIN_SIZE
    out = tr.train_step(batch)
    assert not out["skipped"] and out["n_pos"].tolist() == [495, 177]
    H, W = MAIN_SIZE
    gt, anchors = main_boxes(), model_sd["person_detector.anchors"]
    prm = [model_sd[k].reshape(-1, 128) if k.endswith("weight") else model_sd[k] for k in HEADS]
    assign = R.match(anchors, gt, 2, H, W)["assign"]
    ref = R.loss_and_grads(x.cpu(), *prm, anchors, gt, assign, H, W)
    leaves = [p.clone().float().requires_grad_(True) for p in prm]
    c32 = R.chain(x.cpu(), *leaves, anchors, gt, assign, H, W, dtype=torch.float32)
    c32[0].backward()
    for name, dev, c, key in (("loss", out["loss"], c32[0], "loss"), ("cls", out["cls_loss"], c32[1], "cls"),
                              ("box", out["box_loss"], c32[2], "box")):
        _check(name, float(dev), float(c.detach()), ref[key])
    new = tr.model.state_dict()
    for k, p, leaf, g in zip(HEADS, prm, leaves, ("g_box_w", "g_box_b", "g_cls_w", "g_cls_b")):
        assert not torch.equal(new[k].cpu().reshape(p.shape), p), k
        _check(k, new[k].cpu().reshape(p.shape), (leaf - LR * leaf.grad).detach(), p.double() - LR * ref[g])


def _three_steps(sd):
    tr = _trainer(sd, dict(name="adam", learning_rate=1e-3))
    batch = _to_dev(make_batch())
    torch.manual_seed(17)
    frozen = tr._frozen_versions()
    losses = torch.stack([tr.train_step(batch)["loss"] for _ in range(3)]).cpu()
    assert tr._frozen_versions() == frozen
    return losses, {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}


def test_two_trainers_from_one_seed_are_bit_identical(model_sd):
    la, a = _three_steps(model_sd)
    lb, b = _three_steps(model_sd)
    assert torch.equal(la, lb), (la, lb)
    assert not [k for k in a if not torch.equal(a[k], b[k])]
    assert float(la[2]) < float(la[1]) < float(la[0])


def test_an_epoch_changes_the_four_head_tensors_only(model_sd):
    """train_epoch over two batches (its frozen-state assertion holds), then validate_epoch: every tensor but
    the four of box_heads.0 / cls_heads.0 is bit for bit the starting one; the validation line is complete."""
    batches = [_to_dev(make_batch()), _to_dev(make_batch())]
    tr = _trainer(model_sd, dict(name="sgd", learning_rate=LR), train=batches, val=batches[:1])
    line = tr.train_epoch()
    assert line["steps"] == 2 and line["skipped_steps"] == 0 and line["loss"] > 0
    after = {k: v.detach().cpu() for k, v in tr.model.state_dict().items()}
    changed = sorted(k for k, v in after.items() if not torch.equal(v, model_sd[k]))
    assert changed == sorted(HEADS)
    val = tr.validate_epoch()
    assert set(val) == {"loss", "cls_loss", "box_loss", "recall_50"}
    assert all(np.isfinite(v) for v in val.values()) and 0.0 <= val["recall_50"] <= 1.0
    assert abs(val["loss"] - (val["cls_loss"] + val["box_loss"])) <= 1e-5 * val["loss"]
    assert all(torch.equal(v.detach().cpu(), after[k]) for k, v in tr.model.state_dict().items())


def test_a_batch_without_a_labelled_box_still_steps(model_sd):
    """All negatives, N = 1: the class tensors move, the box tensors do not (their gradient is exactly 0)."""
    tr = _trainer(model_sd, dict(name="sgd", learning_rate=1e-6, momentum=0.0, weight_decay=0.0))
    out = tr.train_step(_to_dev(make_batch(labelled=False)))
    assert not out["skipped"] and out["n_pos"].tolist() == [0, 0]
    assert float(out["box_loss"]) == 0.0 and float(out["loss"]) == float(out["cls_loss"]) > 0
    new = {k: v.detach().cpu() for k, v in tr.model.state_dict().items()}
    changed = sorted(k for k, v in new.items() if not torch.equal(v, model_sd[k]))
    assert changed == sorted(k for k in HEADS if "cls_heads" in k)


def test_train_cli_end_to_end(tmp_path, capsys):
    """scripts/train.py --train detector on five train images, synthetic starting weights, 1 epoch of at most
    2 steps: the JSON line parses, best_model.pth loads with weights_only and differs from the start in the
    four head tensors only; predict.py (no --gt: the detector path) and evaluate.py --boxes detector run on it."""
    for d in (PKG / "scripts",):
        if str(d) not in sys.path:
            sys.path.insert(0, str(d))
    import evaluate
    import predict
    import train
    data, out = _write_dataset(tmp_path / "data"), tmp_path / "out"
    base = ["--config", CONFIG, "--data_dir", data, "--output_dir", str(out), "--batch-size", "2", "--max-steps", "2",
            "--seed", "3", "--train", "detector"]
    with pytest.raises(SystemExit):
        train.main(base + ["--model", "synthetic", "--amp"])
    capsys.readouterr()
    train.main(base + ["--model", "synthetic", "--epochs", "1"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["epoch"] == 1 and line["steps"] == 2 and line["skipped_steps"] == 0
    for k in ("train_loss", "loss", "cls_loss", "box_loss", "recall_50", "learning_rate", "seconds"):
        assert isinstance(line[k], float) and np.isfinite(line[k]), k
    assert line["train_loss"] > 0 and line["loss"] > 0
    ckpt = torch.load(out / "best_model.pth", map_location="cpu", weights_only=True)
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "history"} and ckpt["epoch"] == 1
    assert ckpt["history"]["recall_50"] == [line["recall_50"]]
    start = predict.load_model("synthetic", predict.load_config(CONFIG), DEV).state_dict()   # as --model synthetic
    changed = sorted(k for k, v in ckpt["model_state_dict"].items() if not torch.equal(v, start[k].cpu()))
    assert changed == sorted(HEADS)
    from PIL import Image
    png = tmp_path / "img.png"
    Image.fromarray(np.random.default_rng(2).integers(0, 256, (128, 96, 3), dtype=np.uint8)).save(png)
    with contextlib.redirect_stdout(io.StringIO()):
        res = predict.main(["--config", CONFIG, "--model", str(out / "best_model.pth"), "--input", str(png),
                            "--output", str(tmp_path / "pred")])
    assert res is not None
    m = evaluate.main(["--config", CONFIG, "--model", str(out / "best_model.pth"), "--dataset-dir", data,
                       "--split", "val", "--batch-size", "2", "--boxes", "detector", "--metric", "oks"])
    assert isinstance(m, dict) and m
    capsys.readouterr()
