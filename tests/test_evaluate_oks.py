"""scripts/evaluate.py with --boxes / --metric, and OksEvaluator end to end on a
small YOLO-pose split written from tests/golden/data_cases.LABEL_CASES (the
size test_data.py::test_gpu_dataset_and_loader_end_to_end uses: 64 x 64 gray
input, synthetic seed-0 weights).

AP / AR are compared with tests/oks_ref.py on host copies of the same tensors
within 1e-12 (tests/test_oks.py states why); the labels fed back as predictions
give exactly 1.0."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oks_ref as R
from conftest import PKG

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from data_cases import LABEL_CASES  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
OKS_KEYS = {"oks_AP", "oks_AP50", "oks_AP75", "oks_AR"}
PCK_KEYS = {"avg_ADE", "pck_0.002", "pck_0.05", "pck_0.2"}


def _evaluate_module():
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    import evaluate
    return evaluate


def _write_dataset(root: Path, names, size=(96, 128)):
    from PIL import Image
    rng = np.random.default_rng(1)
    (root / "val" / "images").mkdir(parents=True)
    (root / "val" / "labels").mkdir(parents=True)
    for n in names:
        Image.fromarray(rng.integers(0, 256, (*size, 3), dtype=np.uint8)).save(root / "val" / "images" / f"{n}.png")
        (root / "val" / "labels" / f"{n}.txt").write_text(LABEL_CASES[n])


# ------------------------------------------------------------------ CPU: the flags are parsed before any device use
@pytest.mark.parametrize("metric", ["pck", "both", None])
def test_cli_rejects_slotwise_metrics_with_detector_boxes(metric, capsys):
    evaluate = _evaluate_module()
    argv = ["--config", "nowhere.yaml", "--model", "synthetic", "--dataset-dir", "nowhere", "--boxes", "detector"]
    with pytest.raises(SystemExit) as e:
        evaluate.main(argv + (["--metric", metric] if metric else []))
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "not defined for detector" in err and "--metric oks" in err


def test_cli_rejects_unknown_choices(capsys):
    evaluate = _evaluate_module()
    base = ["--config", "nowhere.yaml", "--model", "synthetic", "--dataset-dir", "nowhere"]
    for extra in (["--boxes", "oracle"], ["--metric", "map"]):
        with pytest.raises(SystemExit):
            evaluate.main(base + extra)
    capsys.readouterr()


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def split64(tmp_path_factory):
    """The 64 x 64 gray split, its loader and the model; the forward outputs per batch, computed once."""
    from dll.configs import BackboneConfig, ModelConfig, TrainingConfig
    from dll.data import create_optimized_dataloader
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_state_dict
    root = tmp_path_factory.mktemp("oks_split")
    _write_dataset(root, ["two", "one", "ragged", "invisible"])
    dl = create_optimized_dataloader(str(root), batch_size=3, num_workers=0, split="val", img_size=64, grayscale=True,
                                     device=DEV)
    m = MultiPersonKeypointModel(ModelConfig(backbone=BackboneConfig(in_channels=1, input_size=64)), TrainingConfig())
    m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0))
    m = m.to(DEV).eval()
    batches = list(dl)
    with torch.no_grad():
        outs = [m({"image": b["image"], "bboxes": b["bboxes"]}) for b in batches]
    return m, dl, batches, outs


@gpu
def test_gpu_gt_boxes_match_restatement(split64):
    from dll.utils import OksEvaluator
    evaluate = _evaluate_module()
    m, dl, batches, outs = split64
    assert [b["image"].shape[0] for b in batches] == [3, 1] and all(b["orig_size"][0] == (128, 96) for b in batches)
    ev = OksEvaluator()
    want_batches = []
    for out, batch in zip(outs, batches):
        ev.update(out, batch)
        host = {k: v.cpu().numpy() for k, v in ev.inputs(out, batch).items()}
        assert host["pred_kpts"].shape[1] == host["gt_kpts"].shape[1] and (host["scale"] == (128, 96)).all()
        want_batches.append(R.evaluate_batch(**host))
        a, gap = R.margins(want_batches[-1]["oks"])
        assert a >= 1e-9 and gap >= 1e-9, (a, gap)
    got, want = ev.summarize(), R.average_precision(want_batches)
    print(got, want)
    assert set(got) == OKS_KEYS
    for k in OKS_KEYS:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
        assert 0.0 <= got[k] <= 1.0                       # six labelled persons: defined
    # the script's loop is the same computation
    metrics, n, images = evaluate.evaluate(m, dl, None, boxes="gt", oks=OksEvaluator())
    assert (n, images) == (2, 4) and set(metrics) == OKS_KEYS
    assert all(abs(metrics[k] - got[k]) <= 1e-12 for k in OKS_KEYS), (metrics, got)
    metrics, n, images = evaluate.evaluate(m, dl, [0.05], boxes="gt", oks=OksEvaluator())
    assert set(metrics) == OKS_KEYS | {"avg_ADE", "pck_0.05"}
    assert all(abs(metrics[k] - got[k]) <= 1e-12 for k in OKS_KEYS), (metrics, got)


@gpu
def test_gpu_labels_as_predictions_score_one(split64):
    from dll.utils import OksEvaluator
    _, _, batches, _ = split64
    ev = OksEvaluator()
    for batch in batches:
        G = batch["keypoints"].shape[1]
        present = (torch.arange(G, device=DEV)[None] < batch["num_persons"].to(DEV)[:, None]).float()
        ev.update({"keypoints": batch["keypoints"][:, :, None].contiguous()}, batch, scores=present)
    assert ev.summarize() == {"oks_AP": 1.0, "oks_AP50": 1.0, "oks_AP75": 1.0, "oks_AR": 1.0}


def _cli(tmp_path, capsys, *extra):
    evaluate = _evaluate_module()
    _write_dataset(tmp_path, ["two", "one", "ragged"], size=(120, 90))
    m = evaluate.main(["--config", str(PKG / "configs" / "default_config.yaml"), "--model", "synthetic",
                       "--dataset-dir", str(tmp_path), "--split", "val", "--batch-size", "2", *extra])
    return m, json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@gpu
def test_gpu_cli_metric_oks(tmp_path, capsys):
    m, line = _cli(tmp_path, capsys, "--metric", "oks")
    assert set(m) == OKS_KEYS and set(line) == OKS_KEYS | {"split", "batches", "boxes", "images"}
    assert line["boxes"] == "gt" and line["images"] == 3 and line["batches"] == 2
    assert all(0.0 <= line[k] <= 1.0 for k in OKS_KEYS)


@gpu
def test_gpu_cli_metric_both(tmp_path, capsys):
    m, line = _cli(tmp_path, capsys, "--metric", "both")
    assert set(m) == OKS_KEYS | PCK_KEYS and set(line) == OKS_KEYS | PCK_KEYS | {"split", "batches", "boxes", "images"}


@gpu
def test_gpu_cli_detector_boxes(tmp_path, capsys):
    m, line = _cli(tmp_path, capsys, "--boxes", "detector", "--metric", "oks")
    assert set(m) == OKS_KEYS and line["boxes"] == "detector" and line["images"] == 3
    assert all(0.0 <= line[k] <= 1.0 or line[k] == -1.0 for k in OKS_KEYS)
