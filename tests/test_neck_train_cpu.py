"""Trainer(train_neck=True) and scripts/train.py --train-neck without a device:
the refusals, the parameter groups, what the frozen-state check lets go, and
the command line's argument errors."""
import sys

import pytest
import torch

from conftest import PKG

CONFIG = str(PKG / "configs" / "default_config.yaml")
NECK_PARAMETERS = ["backbone.fpn.lateral_convs.0.weight", "backbone.fpn.lateral_convs.1.weight",
                   "backbone.fpn.lateral_convs.2.weight", "backbone.fpn.lateral_convs.3.weight",
                   "backbone.fpn.fpn_convs.0.0.weight", "backbone.fpn.fpn_convs.0.1.weight",
                   "backbone.fpn.fpn_convs.0.1.bias"]
NECK_BUFFERS = ["backbone.fpn.fpn_convs.0.1.running_mean", "backbone.fpn.fpn_convs.0.1.running_var",
                "backbone.fpn.fpn_convs.0.1.num_batches_tracked"]


def _parts(**opt):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.configs.training_config import OptimizerConfig
    from dll.models import MultiPersonKeypointModel
    cfg = TrainingConfig(optimizer=OptimizerConfig(**opt))
    return MultiPersonKeypointModel(ModelConfig(), cfg), cfg


def test_constructor_refuses_a_cpu_device_and_bad_scales():
    from dll.training import Trainer
    model, cfg = _parts()
    with pytest.raises(NotImplementedError, match="train_neck"):
        Trainer(model, torch.device("cpu"), [], [], cfg, train_neck=True)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="neck_lr_scale"):
            Trainer(model, torch.device("cpu"), [], [], cfg, neck_lr_scale=bad)
    tr = Trainer(model, torch.device("cpu"), [], [], cfg, neck_lr_scale=0.5)     # accepted, and unused
    assert tr.train_neck is False and len(tr.optimizer.param_groups) == 1


def test_parameter_groups_hold_the_head_and_exactly_the_level0_path():
    """The groups as the constructor builds them with train_neck=True (built here
    on a CPU trainer by the same method: the constructor itself needs a device)."""
    from dll.training import Trainer
    model, cfg = _parts(name="adam", learning_rate=2e-3, weight_decay=0.01)
    tr = Trainer(model, torch.device("cpu"), [], [], cfg, neck_lr_scale=0.25)
    assert tr._trained_names() == set()
    tr.train_neck = True
    opt = tr._create_optimizer()
    named = dict(model.named_parameters())
    by_id = {id(p): k for k, p in named.items()}
    head, neck = opt.param_groups
    assert sorted(by_id[id(p)] for p in head["params"]) == sorted(k for k in named if k.startswith("heatmap_head."))
    assert [by_id[id(p)] for p in neck["params"]] == NECK_PARAMETERS
    assert [k for k, _ in tr.neck_parameters()] == NECK_PARAMETERS
    assert head["lr"] == 2e-3 and neck["lr"] == pytest.approx(2e-3 * 0.25)
    assert head["weight_decay"] == neck["weight_decay"] == 0.01
    # the frozen-state check lets exactly these and the batch norm's buffers go
    assert tr._trained_names() == set(NECK_PARAMETERS + NECK_BUFFERS)
    watched = set(tr._frozen_versions())
    sd = set(model.state_dict())
    assert watched == {k for k in sd if not k.startswith("heatmap_head.")} - set(NECK_PARAMETERS + NECK_BUFFERS)
    for k in ("backbone.fpn.fpn_convs.1.0.weight", "backbone.fpn.fpn_convs.3.1.running_mean",
              "backbone.body.features.0.0.weight", "channel_attention.fc.0.weight",
              "person_detector.box_heads.0.weight"):
        assert k in watched, k


def test_forward_level0_refuses_cpu_taps_and_a_wrong_count():
    from dll import _native
    model, _ = _parts()
    fpn = model.backbone.fpn
    taps = [torch.zeros(1, c, 8 >> i, 8 >> i) for i, c in enumerate((16, 24, 48, 576))]
    with pytest.raises(ValueError, match="Expected 4 features"):
        fpn.forward_level0(taps[:3])
    with pytest.raises(_native.KpdNativeError):
        fpn.forward_level0(taps)
    assert set(fpn.LEVEL0_PARAMETERS) <= set(dict(fpn.named_parameters()))
    assert set(fpn.LEVEL0_BUFFERS) <= set(dict(fpn.named_buffers()))


def test_cli_refuses_the_neck_flags_with_the_detector(tmp_path, capsys, monkeypatch):
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    for split in ("train", "val"):
        for sub in ("images", "labels"):
            (tmp_path / "data" / split / sub).mkdir(parents=True)
    good = ["--config", CONFIG, "--data_dir", str(tmp_path / "data"), "--output_dir", str(tmp_path / "out")]
    cases = [(good + ["--train-neck", "--train", "detector"], "do not apply to --train detector"),
             (good + ["--neck-lr-scale", "0.5", "--train", "detector"], "do not apply to --train detector"),
             (good + ["--neck-lr-scale", "0.5"], "needs --train-neck"),
             (good + ["--train-neck", "--neck-lr-scale", "0"], "positive and finite"),
             (good + ["--train-neck", "--neck-lr-scale", "x"], "invalid float")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
    args = train.parse_args(good + ["--train-neck", "--neck-lr-scale", "0.1"])
    assert args.train_neck is True and args.neck_lr_scale == 0.1
    assert train.parse_args(good).train_neck is False
