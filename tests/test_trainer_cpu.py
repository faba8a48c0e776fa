"""dll.training.Trainer and scripts/train.py without a device: what the
optimizer holds and how it maps from the config, the refusals, and the
command line's argument errors (which come before any device use)."""
import sys

import pytest
import torch

from conftest import PKG

CONFIG = str(PKG / "configs" / "default_config.yaml")


def _trainer(**opt):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.configs.training_config import OptimizerConfig
    from dll.models import MultiPersonKeypointModel
    from dll.training import Trainer
    cfg = TrainingConfig(optimizer=OptimizerConfig(**opt))
    model = MultiPersonKeypointModel(ModelConfig(), cfg)
    return Trainer(model, torch.device("cpu"), [], [], cfg), model


def test_optimizer_holds_exactly_the_head():
    tr, model = _trainer()
    held = {id(p) for g in tr.optimizer.param_groups for p in g["params"]}
    named = dict(model.named_parameters())
    head = {id(p) for k, p in named.items() if k.startswith("heatmap_head.")}
    assert held == head and 0 < len(head) < len(named)
    assert not model.training and not model.heatmap_head.training     # the whole model starts in eval mode


def test_optimizer_maps_from_the_config():
    tr, _ = _trainer(name="adam", learning_rate=3e-4, beta1=0.8, beta2=0.95, weight_decay=0.01)
    g = tr.optimizer.param_groups[0]
    assert isinstance(tr.optimizer, torch.optim.Adam)
    assert (g["lr"], g["betas"], g["weight_decay"]) == (3e-4, (0.8, 0.95), 0.01)
    tr, _ = _trainer(name="SGD", learning_rate=0.05, momentum=0.7, weight_decay=0.0)
    g = tr.optimizer.param_groups[0]
    assert isinstance(tr.optimizer, torch.optim.SGD)
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (0.05, 0.7, 0.0)
    with pytest.raises(ValueError, match="Unsupported optimizer"):
        _trainer(name="lion")


def test_scheduler_and_refusals():
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.training import Trainer
    cfg = TrainingConfig()
    cfg.lr_scheduler.metric = "avg_ADE"
    cfg.lr_scheduler.patience = 7
    model = MultiPersonKeypointModel(ModelConfig(), cfg)
    tr = Trainer(model, torch.device("cpu"), [], [], cfg)
    assert isinstance(tr.scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau) and tr.scheduler.patience == 7
    assert tr._scheduler_value({"loss": 2.0, "avg_ADE": 0.5}) == 0.5
    tr.scheduler_metric = "no_such_metric"
    assert tr._scheduler_value({"loss": 2.0, "avg_ADE": 0.5}) == 2.0     # falls back to the loss
    with pytest.raises(NotImplementedError, match="AMP"):
        Trainer(model, torch.device("cpu"), [], [], cfg, use_amp=True)
    with pytest.raises(TypeError):
        Trainer(torch.nn.Linear(2, 2), torch.device("cpu"), [], [], cfg)


def _train_module():
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    import train
    return train


def _dataset_dirs(root):
    for split in ("train", "val"):
        for sub in ("images", "labels"):
            (root / split / sub).mkdir(parents=True)
    return str(root)


def test_cli_argument_errors_come_before_the_device(tmp_path, capsys, monkeypatch):
    train = _train_module()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    data = _dataset_dirs(tmp_path / "data")
    out = str(tmp_path / "out")
    good = ["--config", CONFIG, "--data_dir", data, "--output_dir", out]
    cases = [
        (["--config", CONFIG, "--data_dir", data], "output_dir"),                       # a required one missing
        (["--config", "nowhere.yaml", "--data_dir", data, "--output_dir", out], "no such file"),
        (["--config", CONFIG, "--data_dir", str(tmp_path / "nowhere"), "--output_dir", out], "not found"),
        (good + ["--epochs", "0"], "--epochs must be at least 1"),
        (good + ["--batch-size", "0"], "--batch-size must be at least 1"),
        (good + ["--max-steps", "-3"], "--max-steps must be at least 1"),
        (good + ["--resume", str(tmp_path / "none.pth")], "no such checkpoint"),
        (good + ["--model", str(tmp_path / "none.pth")], "no such checkpoint"),
        (good + ["--precision", "fp8"], "invalid choice"),
        (good + ["--seed", "x"], "invalid int"),
    ]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
    assert not (tmp_path / "out").exists()


def test_training_config_from_yaml_block():
    train = _train_module()
    cfg = train.training_config_from_dict({"num_epochs": 3, "optimizer": {"name": "sgd", "learning_rate": 0.1},
                                           "lr_scheduler": {"patience": 2}, "pck_thresholds": [0.1]})
    assert cfg.num_epochs == 3 and cfg.optimizer.name == "sgd" and cfg.optimizer.momentum == 0.9
    assert cfg.lr_scheduler.patience == 2 and cfg.pck_thresholds == [0.1]
    assert train.training_config_from_dict(None).num_epochs == 50
