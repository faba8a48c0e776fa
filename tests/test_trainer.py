"""dll.training.Trainer on the device: train_step against the float64 replica
of the head (tests/head_train_ref.py) fed with the device's own ROI features,
run-to-run bit-identity from one seed, and scripts/train.py end to end on a
five-image dataset (checkpoint, evaluate on it, resume)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import head_train_ref as HR
from conftest import PKG

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from data_cases import LABEL_CASES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CONFIG = str(PKG / "configs" / "default_config.yaml")
# test_train_step_matches_the_float64_replica: chosen on the CPU with the float64 replica on ROI features
# from oracle.kpd_oracle (the same batch): its loss falls from 2.125162e-01 to 1.367446e-01 over the 6 steps,
# 0.643 x the start (0.3: 0.760 x, 0.1: 0.878 x)
LR = 0.5


def make_batch():
    """One 256 x 192 image with three person slots, the middle one the
    collate's all-zero padding: a collated batch on the CPU."""
    from dll.models.synthetic import synthetic_images
    g = torch.Generator().manual_seed(5)
    boxes = torch.tensor([[[0.35, 0.45, 0.4, 0.6], [0.0, 0.0, 0.0, 0.0], [0.6, 0.55, 0.5, 0.7]]])
    uv = torch.rand(1, 3, 17, 2, generator=g) * 0.9 + 0.05
    kp = boxes[:, :, None, :2] - boxes[:, :, None, 2:] / 2 + uv * boxes[:, :, None, 2:]
    vis = torch.randint(1, 3, (1, 3, 17), generator=g).float()
    vis[0, 0, 3] = 0          # an unlabelled joint
    kp[0, 2, 5] = 0.99        # a joint outside its box
    kp[0, 1], vis[0, 1] = 0, 0
    return {"image": synthetic_images(1, 3, 256, 192, seed=41), "bboxes": [boxes], "keypoints": kp,
            "visibilities": vis}


def _to_dev(batch):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in batch.items()}


def _trainer(sd, dropout, optimizer):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.configs.model_config import HeatmapHeadConfig
    from dll.configs.training_config import OptimizerConfig
    from dll.models import MultiPersonKeypointModel
    from dll.training import Trainer
    cfg = TrainingConfig(optimizer=OptimizerConfig(**optimizer))
    model = MultiPersonKeypointModel(ModelConfig(heatmap_head=HeatmapHeadConfig(dropout_rate=dropout)), cfg)
    model.load_state_dict(sd)
    return Trainer(model, DEV, [], [], cfg)


def test_train_step_matches_the_float64_replica(model_sd):
    """Head dropout 0, plain SGD (momentum 0, weight decay 0), the same batch
    for 6 steps: the per-step loss stays within max(10 x |float32 replica -
    float64 replica|, 1e-5 x |float64|) of the float64 replica, which is fed
    the device's roi_features and targets; the replica's and the native run's
    last loss are below 0.8 x their first.

    Measured on the MI355X: float64 replica 2.125162e-01 -> 1.367945e-01,
    native 2.125162e-01 -> 1.368020e-01; native deviation per step 4.3e-9,
    7.5e-9, 1.7e-7, 1.1e-6, 3.3e-6, 7.6e-6 against bounds 2.1e-6, 2.9e-6,
    1.1e-5, 5.6e-5, 5.5e-6, 5.9e-5 (the float32 replica's own deviation swings
    between 5e-7 and 6e-6 from step 2 on; step 4 is the closest, 0.60 x)."""
    from oracle import loss_oracle as LO
    tr = _trainer(model_sd, 0.0, dict(name="sgd", learning_rate=LR, momentum=0.0, weight_decay=0.0))
    batch = _to_dev(make_batch())
    x, gt, tw, rows, _ = tr._features_and_targets(batch)
    assert rows.tolist() == [0, 2] and tuple(x.shape) == (2, 64, 56, 56)
    assert float(tw.sum()) == 2 * 17 - 2                 # the unlabelled joint and the one outside its box
    native = [tr.train_step(batch) for _ in range(6)]
    assert all(o["rows"] == 2 and not o["skipped"] for o in native)
    native = [float(v) for v in torch.stack([o["loss"] for o in native]).cpu()]
    x, gt, tw = x.cpu(), gt.cpu(), tw.cpu()
    hsd = {k[len("heatmap_head."):]: v for k, v in model_sd.items() if k.startswith("heatmap_head.")}
    runs = {}
    for dt in (torch.float64, torch.float32):
        p = HR.leaves(hsd, dt)
        runs[dt] = []
        for _ in range(6):
            loss = LO.adaptive_heatmap_loss(HR.forward(p, x)[0], gt, tw)
            runs[dt].append(float(loss.detach()))
            loss.backward()
            HR.sgd_step(p, LR)
    r64, r32 = runs[torch.float64], runs[torch.float32]
    print("float64 replica:", " ".join(f"{v:.6e}" for v in r64))
    print("native:         ", " ".join(f"{v:.6e}" for v in native))
    assert r64[5] < 0.8 * r64[0]
    for k in range(6):
        bound = max(10 * abs(r32[k] - r64[k]), 1e-5 * abs(r64[k]))
        print(f"step {k}: native dev {abs(native[k] - r64[k]):.3e}  fp32 replica dev {abs(r32[k] - r64[k]):.3e}  "
              f"bound {bound:.3e}")
        assert abs(native[k] - r64[k]) <= bound, f"step {k}: {abs(native[k] - r64[k]):.3e} > {bound:.3e}"
    assert native[5] < 0.8 * native[0]


def test_a_batch_without_boxes_is_skipped(model_sd):
    tr = _trainer(model_sd, 0.0, dict(name="sgd", learning_rate=LR))
    batch = _to_dev(make_batch())
    batch["bboxes"] = [torch.zeros_like(batch["bboxes"][0])]
    before = {k: v.clone() for k, v in tr.model.state_dict().items()}
    out = tr.train_step(batch)
    assert out == {"loss": None, "rows": 0, "skipped": True}
    assert all(torch.equal(v, before[k]) for k, v in tr.model.state_dict().items())


def _four_steps(sd):
    tr = _trainer(sd, 0.2, dict(name="adam", learning_rate=1e-3))
    batch = _to_dev(make_batch())
    torch.manual_seed(17)
    tr.model.eval()
    frozen = tr._frozen_versions()
    losses = torch.stack([tr.train_step(batch)["loss"] for _ in range(4)]).cpu()
    assert tr._frozen_versions() == frozen
    return losses, {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}


def test_two_trainers_from_one_seed_are_bit_identical(model_sd):
    """4 Adam steps with head dropout 0.2 from the same seed: the losses and
    the head's state dict are bit-identical between two trainers, nothing
    outside heatmap_head. changed, and the head's running statistics did."""
    la, a = _four_steps(model_sd)
    lb, b = _four_steps(model_sd)
    assert torch.equal(la, lb), (la, lb)
    differing = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differing, differing
    for k, v in a.items():
        if not k.startswith("heatmap_head."):
            assert torch.equal(v, model_sd[k]), k
    for k in ("heatmap_head.deconv_layers.1.running_mean", "heatmap_head.final_layer.1.running_var",
              "heatmap_head.final_layer.3.weight"):
        assert not torch.equal(a[k], model_sd[k]), k
    assert int(a["heatmap_head.deconv_layers.1.num_batches_tracked"]) == \
        int(model_sd["heatmap_head.deconv_layers.1.num_batches_tracked"]) + 4


def _write_dataset(root: Path, size=(96, 128)):
    from PIL import Image
    rng = np.random.default_rng(1)
    splits = {"train": ["two", "one", "ragged", "none_valid", "short"], "val": ["extra", "one"]}
    for split, names in splits.items():
        (root / split / "images").mkdir(parents=True)
        (root / split / "labels").mkdir(parents=True)
        for n in names:
            Image.fromarray(rng.integers(0, 256, (*size, 3), dtype=np.uint8)).save(root / split / "images" / f"{n}.png")
            (root / split / "labels" / f"{n}.txt").write_text(LABEL_CASES[n])
    return str(root)


def test_train_cli_end_to_end(tmp_path, capsys):
    """scripts/train.py on five train images (one without a valid person),
    synthetic starting weights, 1 epoch of at most 2 steps: the JSON line
    parses, best_model.pth loads with weights_only, evaluate.py runs on it,
    and a resumed run continues at epoch 2."""
    for d in (PKG / "scripts",):
        if str(d) not in sys.path:
            sys.path.insert(0, str(d))
    import evaluate
    import train
    data, out = _write_dataset(tmp_path / "data"), tmp_path / "out"
    base = ["--config", CONFIG, "--data_dir", data, "--output_dir", str(out), "--batch-size", "2", "--max-steps", "2",
            "--seed", "3"]
    capsys.readouterr()
    train.main(base + ["--model", "synthetic", "--epochs", "1"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["epoch"] == 1 and line["steps"] + line["skipped_steps"] == 2 and line["steps"] >= 1
    for k in ("train_loss", "loss", "avg_ADE", "pck_0.05", "learning_rate", "seconds"):
        assert isinstance(line[k], float) and np.isfinite(line[k]), k
    assert line["train_loss"] > 0 and line["loss"] > 0
    ckpt = torch.load(out / "best_model.pth", map_location="cpu", weights_only=True)
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "history"} and ckpt["epoch"] == 1
    assert ckpt["history"]["epoch"] == [1] and ckpt["history"]["loss"] == [line["loss"]]
    torch.save(ckpt, out / "checkpoint_epoch_1.pth")      # (checkpoint_interval 5: the periodic file is not due yet)
    m = evaluate.main(["--config", CONFIG, "--model", str(out / "best_model.pth"), "--dataset-dir", data,
                       "--split", "val", "--batch-size", "2"])
    assert "avg_ADE" in m
    capsys.readouterr()
    history = train.main(base + ["--resume", str(out / "checkpoint_epoch_1.pth"), "--epochs", "2"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [ln["epoch"] for ln in lines] == [2] and history["epoch"] == [1, 2]
