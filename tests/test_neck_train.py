"""Training the FPN's level-0 path under the heatmap head on the device
(DESIGN.md §3l): neck_roi_features is the function the eval forward computes,
its parameter gradients against a float64 CPU replica, Trainer(train_neck=True)
steps, checkpoints and resume, and scripts/train.py --train-neck."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import roi_align_grad_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CONFIG = str(PKG / "configs" / "default_config.yaml")
FPN = "backbone.fpn."
NECK_PARAMETERS = [FPN + k for k in ("lateral_convs.0.weight", "lateral_convs.1.weight", "lateral_convs.2.weight",
                                     "lateral_convs.3.weight", "fpn_convs.0.0.weight", "fpn_convs.0.1.weight",
                                     "fpn_convs.0.1.bias")]
NECK_BUFFERS = [FPN + "fpn_convs.0.1." + k for k in ("running_mean", "running_var", "num_batches_tracked")]


def _model(sd, precision="split", dropout=None):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.configs.model_config import HeatmapHeadConfig
    from dll.models import MultiPersonKeypointModel
    mc = ModelConfig() if dropout is None else ModelConfig(heatmap_head=HeatmapHeadConfig(dropout_rate=dropout))
    m = MultiPersonKeypointModel(mc, TrainingConfig(), precision=precision)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


# ------------------------------------------------------------------ eval agreement
@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_eval_mode_agrees_with_the_plan(model_sd, precision):
    """With the model in eval(), neck_roi_features is Plan.roi_features: within
    the atol 2e-5 test_gpu_parity applies to the forward's ROI buffer against
    the oracle, on identical top-k indices."""
    from dll.models.keypoint_model import neck_roi_features
    from dll.models.synthetic import synthetic_boxes, synthetic_images
    m = _model(model_sd, precision)
    img = synthetic_images(2, 3, 256, 192, seed=21, device=DEV)
    boxes = synthetic_boxes(2, 2, seed=22, device=DEV)
    rows = torch.arange(4, dtype=torch.int32, device=DEV)
    plan = m.native_plan(DEV)
    want = plan.roi_features(img, boxes, rows)
    plan_topk = torch.empty(2, 64, dtype=torch.int32, device=DEV)
    plan.forward(img, boxes, torch.empty(2, 2, 1, 17, 2, device=DEV), torch.empty(2, 2, 1, 17, 3, device=DEV),
                 torch.empty(2, 2, 17, 56, 56, device=DEV), topk=plan_topk)
    with torch.no_grad():
        got, topk, level0 = neck_roi_features(m, img, boxes, rows, return_parts=True)
    assert tuple(level0.shape) == (2, 128, 128, 96) and tuple(got.shape) == (4, 64, 56, 56)
    if not torch.equal(topk.cpu(), plan_topk.long().cpu()):       # a finding to explain from the score gap
        scores = m.channel_attention.native_select(level0, 64, select=False)[0]
        gap = scores.sort(dim=1, descending=True).values[:, 63:65]
        raise AssertionError(f"top-k differs from the plan's; scores around the cut: {gap.tolist()}")
    err = float((got - want).abs().max())
    print(f"{precision}: max |neck_roi_features - Plan.roi_features| = {err:.3e}, max |x| = {float(want.abs().max()):.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=2e-5, rtol=0)
    assert not any(p.grad is not None for p in m.parameters())


# ------------------------------------------------------------------ gradients
def _replica(sd, taps, boxes, rows, topk, mask, gup, dtype):
    """The level-0 path in torch ops on the CPU in ``dtype``, ROI align as the
    dense My . F . Mx^T / count built from ops_ref._axis -> ({name: grad}, x, the
    replica's own ReLU mask); ``mask`` (the native one) is what it applies."""
    p = {k: sd[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in NECK_PARAMETERS}
    top = None
    for i in (3, 2, 1, 0):
        lat = F.conv2d(taps[i].to(dtype), p[f"{FPN}lateral_convs.{i}.weight"])
        top = lat if top is None else lat + F.interpolate(top, size=lat.shape[2:], mode="nearest")
    x = F.conv2d(top, p[FPN + "fpn_convs.0.0.weight"], padding=1)
    pre = F.batch_norm(x, None, None, p[FPN + "fpn_convs.0.1.weight"], p[FPN + "fpn_convs.0.1.bias"], True, 0.1, 1e-5)
    level0 = pre * mask.to(dtype)
    B, C, H, W = level0.shape
    rois = G.boxes_to_rois(boxes, rows, H, W).numpy()
    outs = []
    for i, r in enumerate(rows):
        b = r // boxes.shape[1]
        My, Mx, count, _ = G.roi_matrices(rois[i], H, W)
        My, Mx = torch.from_numpy(My).to(dtype), torch.from_numpy(Mx).to(dtype)
        outs.append(torch.einsum("ph,chw,qw->cpq", My, level0[b, topk[b]], Mx) / count)
    out = torch.stack(outs)
    (out * gup.to(dtype)).sum().backward()
    return {k: v.grad for k, v in p.items()}, out.detach(), pre.detach() > 0


def _close(name, got, r64, r32):
    """tests/test_head_train.py's criterion: 4 x the error of the float32 CPU
    replica, but not below 2e-5 x max|ref|."""
    got = got.detach().double().cpu().reshape(r64.shape)
    err = float((got - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    scale = float(r64.abs().max())
    bound = max(4 * e32, 2e-5 * scale)
    print(f"{name}: native {err:.3e}  fp32 replica {e32:.3e}  scale {scale:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"


def test_parameter_gradients_match_the_float64_replica(model_sd):
    """2 x 3 x 64 x 48 images (level 0 is 32 x 24), P = 2, fpn in train(), a
    seeded upstream gradient into the ROI features: the seven parameter
    gradients of the level-0 path against the float64 replica with the native
    ReLU mask forced."""
    from dll.models.keypoint_model import neck_roi_features
    from dll.models.synthetic import synthetic_boxes, synthetic_images
    m = _model(model_sd)
    img = synthetic_images(2, 3, 64, 48, seed=51, device=DEV)
    boxes = synthetic_boxes(2, 2, seed=52, device=DEV)
    rows = torch.arange(4, dtype=torch.int32, device=DEV)
    gup = torch.randn(4, 64, 56, 56, generator=torch.Generator().manual_seed(53))
    m.backbone.fpn.train()
    x, topk, level0 = neck_roi_features(m, img, boxes, rows, return_parts=True)
    assert tuple(level0.shape) == (2, 128, 32, 24) and x.requires_grad
    x.backward(gup.to(DEV))
    m.backbone.fpn.eval()
    with torch.no_grad():
        taps = [t.cpu() for t in m.backbone.body(img).values()]
    named = dict(m.named_parameters())
    with_grad = sorted(k for k, p in named.items() if p.grad is not None)
    assert with_grad == sorted(NECK_PARAMETERS)                   # nothing else received a gradient
    mask = (level0.detach() > 0).cpu()
    ref = {dt: _replica(model_sd, taps, boxes.cpu(), list(range(4)), topk.cpu(), mask, gup, dt)
           for dt in (torch.float64, torch.float32)}
    # the native mask is the float64 one but for near-zero pre-activations (as tests/test_head_train.py
    # checks the head's): a wrong sign pattern in the native conv or batch norm does not hide behind the forcing
    flipped = float((mask != ref[torch.float64][2]).float().mean())
    print(f"ReLU mask: {flipped:.2e} of the elements differ from the float64 replica's own")
    assert flipped <= 1e-4
    assert 0.05 < float(mask.float().mean()) < 0.95
    _close("roi features", x, ref[torch.float64][1], ref[torch.float32][1])
    for k in NECK_PARAMETERS:
        _close("grad " + k, named[k].grad, ref[torch.float64][0][k], ref[torch.float32][0][k])
    bufs = dict(m.named_buffers())
    assert int(bufs[NECK_BUFFERS[2]]) == int(model_sd[NECK_BUFFERS[2]]) + 1
    assert not torch.equal(bufs[NECK_BUFFERS[0]].cpu(), model_sd[NECK_BUFFERS[0]])


# ------------------------------------------------------------------ trainer
def make_batch():
    """One 256 x 192 image, three person slots, the middle one all-zero padding (a collated batch)."""
    from dll.models.synthetic import synthetic_images
    g = torch.Generator().manual_seed(5)
    boxes = torch.tensor([[[0.35, 0.45, 0.4, 0.6], [0.0, 0.0, 0.0, 0.0], [0.6, 0.55, 0.5, 0.7]]])
    uv = torch.rand(1, 3, 17, 2, generator=g) * 0.9 + 0.05
    kp = boxes[:, :, None, :2] - boxes[:, :, None, 2:] / 2 + uv * boxes[:, :, None, 2:]
    vis = torch.randint(1, 3, (1, 3, 17), generator=g).float()
    kp[0, 1], vis[0, 1] = 0, 0
    batch = {"image": synthetic_images(1, 3, 256, 192, seed=41), "bboxes": [boxes], "keypoints": kp,
             "visibilities": vis}
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in batch.items()}


def _trainer(sd, out_dir=None, **kw):
    from dll.configs import TrainingConfig
    from dll.configs.training_config import OptimizerConfig
    from dll.training import Trainer
    cfg = TrainingConfig(optimizer=OptimizerConfig(name="adam", learning_rate=1e-3))
    return Trainer(_model(sd, dropout=0.0), DEV, [], [], cfg, output_dir=out_dir, **kw)


def _eval_heatmap(model, batch):
    model.eval()
    with torch.no_grad():
        return model({"image": batch["image"], "bboxes": batch["bboxes"]})["heatmap"].clone()


def test_two_steps_train_the_neck_and_nothing_else(model_sd, tmp_path):
    tr = _trainer(model_sd, tmp_path, train_neck=True, neck_lr_scale=0.5)
    assert [g["lr"] for g in tr.optimizer.param_groups] == [1e-3, 5e-4]
    batch = make_batch()
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    heat_before = _eval_heatmap(tr.model, batch)
    frozen = tr._frozen_versions()
    outs = [tr.train_step(batch) for _ in range(2)]
    assert all(o["rows"] == 2 and not o["skipped"] for o in outs)
    assert all(bool(torch.isfinite(o["loss"])) for o in outs)
    assert tr.model.backbone.fpn.training and not tr.model.backbone.body.training
    assert tr._frozen_versions() == frozen
    tr.model.backbone.fpn.eval()
    after = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    for k in NECK_PARAMETERS + NECK_BUFFERS:
        assert not torch.equal(after[k], before[k]), k
    assert int(after[NECK_BUFFERS[2]]) == int(before[NECK_BUFFERS[2]]) + 2
    for k, v in after.items():
        if not k.startswith("heatmap_head.") and k not in NECK_PARAMETERS + NECK_BUFFERS:
            assert torch.equal(v, before[k]), k                   # the body, channel_attention, fpn_convs.1..3, ...
    assert any(not torch.equal(after[k], before[k]) for k in after if k.startswith("heatmap_head."))
    heat_after = _eval_heatmap(tr.model, batch)
    assert float((heat_after - heat_before).abs().max()) > 1e-4
    # the checkpoint serves the same forward, and resumes
    tr.epoch = 1
    tr.save_checkpoint(1, is_best=True, periodic=False)
    ckpt = torch.load(tmp_path / "best_model.pth", map_location="cpu", weights_only=True)
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "history"}
    assert len(ckpt["optimizer_state_dict"]["param_groups"]) == 2
    fresh = _model(ckpt["model_state_dict"], dropout=0.0)
    assert torch.equal(_eval_heatmap(fresh, batch), heat_after)
    tr2 = _trainer(model_sd, None, train_neck=True, neck_lr_scale=0.5)
    assert tr2.resume(tmp_path / "best_model.pth") == 1
    for k, v in tr2.model.state_dict().items():
        assert torch.equal(v, after[k]), k
    s1, s2 = tr.optimizer.state_dict(), tr2.optimizer.state_dict()
    assert s1["param_groups"] == s2["param_groups"] and set(s1["state"]) == set(s2["state"])
    for i in s1["state"]:
        assert torch.equal(s1["state"][i]["exp_avg"].cpu(), s2["state"][i]["exp_avg"].cpu())
    assert bool(torch.isfinite(tr2.train_step(batch)["loss"]))
    with pytest.raises(ValueError, match="train_neck"):
        _trainer(model_sd, None, train_neck=False).resume(tmp_path / "best_model.pth")


def test_epoch_loop_puts_the_neck_back_in_eval_mode(model_sd):
    tr = _trainer(model_sd, None, train_neck=True)
    batch = make_batch()
    tr.train_dataloader = [batch, batch]
    tr.val_dataloader = [batch]
    stats = tr.train_epoch()
    assert stats["steps"] == 2 and np.isfinite(stats["loss"])
    assert not tr.model.backbone.fpn.training and not tr.head.training
    val = tr.validate_epoch()                                     # the plan, re-packed from the new FPN weights
    assert np.isfinite(val["loss"]) and np.isfinite(val["avg_ADE"])


def test_without_train_neck_the_backbone_stays_bit_equal(model_sd):
    tr = _trainer(model_sd, None)
    assert len(tr.optimizer.param_groups) == 1
    batch = make_batch()
    outs = [tr.train_step(batch) for _ in range(2)]
    assert all(bool(torch.isfinite(o["loss"])) for o in outs)
    assert not tr.model.backbone.fpn.training
    for k, v in tr.model.state_dict().items():
        if k.startswith("backbone."):
            assert torch.equal(v.cpu(), model_sd[k]), k


# ------------------------------------------------------------------ command line
def test_train_cli_with_the_neck(tmp_path, capsys):
    """--train-neck with --train detector is an argument error; a --max-steps 1
    run on synthetic weights writes a checkpoint whose neck moved and which
    predict.py's loader takes."""
    from PIL import Image
    from data_cases import LABEL_CASES
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    import predict
    import train
    rng = np.random.default_rng(1)
    for split, names in {"train": ["two", "one"], "val": ["one"]}.items():
        for sub in ("images", "labels"):
            (tmp_path / "data" / split / sub).mkdir(parents=True)
        for n in names:
            Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(
                tmp_path / "data" / split / "images" / f"{n}.png")
            (tmp_path / "data" / split / "labels" / f"{n}.txt").write_text(LABEL_CASES[n])
    base = ["--config", CONFIG, "--data_dir", str(tmp_path / "data"), "--output_dir", str(tmp_path / "out"),
            "--batch-size", "2", "--max-steps", "1", "--seed", "3", "--model", "synthetic", "--epochs", "1"]
    with pytest.raises(SystemExit) as e:
        train.main(base + ["--train-neck", "--train", "detector"])
    assert e.value.code == 2 and "--train detector" in capsys.readouterr().err
    train.main(base + ["--train-neck", "--neck-lr-scale", "0.5"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and lines[0]["steps"] == 1 and np.isfinite(lines[0]["train_loss"])
    ckpt = torch.load(tmp_path / "out" / "best_model.pth", map_location="cpu", weights_only=True)
    assert len(ckpt["optimizer_state_dict"]["param_groups"]) == 2
    model = predict.load_model(str(tmp_path / "out" / "best_model.pth"), predict.load_config(CONFIG), DEV)
    synthetic = predict.load_model("synthetic", predict.load_config(CONFIG), DEV).state_dict()
    sd = model.state_dict()
    assert not torch.equal(sd[NECK_PARAMETERS[4]], synthetic[NECK_PARAMETERS[4]])
    assert torch.equal(sd[FPN + "fpn_convs.1.0.weight"], synthetic[FPN + "fpn_convs.1.0.weight"])
    assert torch.equal(sd["backbone.body.features.0.0.weight"], synthetic["backbone.body.features.0.0.weight"])
