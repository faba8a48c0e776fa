"""--flip-test in scripts/evaluate.py and scripts/predict.py:
parsed before any device use; on, evaluate.py's JSON line carries
"flip_test": true and its metrics are those of evaluate() with
model.flip_test = True, and predict.py writes overlays and label files from
the merged outputs; off (or absent), both scripts print and write exactly what
they do without the option.  The split is the small YOLO-pose one of
tests/test_pose_nms_cli.py (tests/golden/data_cases.LABEL_CASES)."""
import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import PKG

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from data_cases import LABEL_CASES  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
OKS_KEYS = {"oks_AP", "oks_AP50", "oks_AP75", "oks_AR"}
NAMES = ("two", "one", "ragged")
CONFIG = str(PKG / "configs" / "default_config.yaml")


def _script(name):
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    return __import__(name)


# ------------------------------------------------------------------ CPU: the flag is parsed before any device use
def test_flip_test_option_parses():
    import argparse
    predict = _script("predict")
    ap = argparse.ArgumentParser()
    predict.add_flip_test_argument(ap)
    assert not predict.flip_test_enabled(ap.parse_args([]))
    assert predict.flip_test_enabled(ap.parse_args(["--flip-test"]))
    assert predict.flip_test_enabled(ap.parse_args(["--flip-test", "on"]))
    assert not predict.flip_test_enabled(ap.parse_args(["--flip-test", "off"]))


def test_both_scripts_accept_flip_test_before_touching_anything():
    """A valid command line gets as far as reading the (missing) config file: the option is known to both parsers."""
    evaluate, predict = _script("evaluate"), _script("predict")
    with pytest.raises(FileNotFoundError):
        evaluate.main(["--config", "nowhere.yaml", "--model", "synthetic", "--dataset-dir", "nowhere", "--flip-test"])
    with pytest.raises(FileNotFoundError):
        predict.main(["--config", "nowhere.yaml", "--model", "synthetic", "--input", "nowhere", "--output", "nowhere",
                      "--flip-test"])


@pytest.mark.parametrize("bad", [["--flip-test", "maybe"], ["--flip-test=yes"], ["--fliptest"], ["--flip_test"]])
def test_both_scripts_reject_an_unknown_value_or_spelling(bad, capsys):
    evaluate, predict = _script("evaluate"), _script("predict")
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--config", "nowhere.yaml", "--model", "synthetic", "--dataset-dir", "nowhere"] + bad)
    assert e.value.code == 2 and "flip" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        predict.main(["--config", "nowhere.yaml", "--model", "synthetic", "--input", "nowhere", "--output", "nowhere"] + bad)
    assert e.value.code == 2 and "flip" in capsys.readouterr().err


# ------------------------------------------------------------------ GPU: evaluate.py
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("flip_eval")
    rng = np.random.default_rng(1)
    (root / "val" / "images").mkdir(parents=True)
    (root / "val" / "labels").mkdir(parents=True)
    for n in NAMES:
        Image.fromarray(rng.integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(root / "val" / "images" / f"{n}.png")
        (root / "val" / "labels" / f"{n}.txt").write_text(LABEL_CASES[n])
    return root


def _evaluate_cli(root, capsys, *extra):
    evaluate = _script("evaluate")
    m = evaluate.main(["--config", CONFIG, "--model", "synthetic", "--dataset-dir", str(root), "--split", "val",
                       "--batch-size", "2", "--metric", "both", *extra])
    return m, capsys.readouterr().out.strip().splitlines()[-1]


@gpu
def test_gpu_evaluate_cli_flip_test(dataset, capsys):
    evaluate, predict = _script("evaluate"), _script("predict")
    plain_m, plain = _evaluate_cli(dataset, capsys)
    _, off = _evaluate_cli(dataset, capsys, "--flip-test", "off")
    assert "flip_test" not in plain and off == plain
    m, text = _evaluate_cli(dataset, capsys, "--flip-test")
    line = json.loads(text)
    assert '"flip_test": true' in text and line["flip_test"] is True
    assert set(line) == set(json.loads(plain)) | {"flip_test"} and OKS_KEYS <= set(m) and set(m) == set(plain_m)
    assert line["images"] == 3 and line["batches"] == 2
    # the same numbers as evaluate() on a model with the attribute set
    from dll.data import create_optimized_dataloader
    from dll.utils import OksEvaluator
    cfg = predict.load_config(CONFIG)
    bcfg = cfg["model"]["backbone"]
    loader = create_optimized_dataloader(str(dataset), batch_size=2, split="val", img_size=bcfg["input_size"],
                                         grayscale=bcfg.get("in_channels", 3) == 1, device=DEV)
    model = predict.load_model("synthetic", cfg, DEV, "split")
    model.flip_test = True
    thresholds = cfg.get("training", {}).get("pck_thresholds", [0.002, 0.05, 0.2])
    want, n, images = evaluate.evaluate(model, loader, thresholds, oks=OksEvaluator())
    assert (n, images) == (2, 3) and want == m and all(line[k] == v for k, v in want.items())
    # and not the plain forward's: the slot-wise distance moves with the merged keypoints
    moved = [k for k in m if k not in OKS_KEYS and m[k] != plain_m[k]]
    print("plain", plain_m, "flip", m)
    assert moved, (m, plain_m)


# ------------------------------------------------------------------ GPU: predict.py
LABELS = {"a": [[0.5, 0.5, 0.4, 0.8], [0.3, 0.4, 0.2, 0.3]]}
SHAPES = {"a": (200, 150), "c": (170, 130)}                       # "c": the person detector


def _predict_cli(args):
    predict = _script("predict")
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = predict.main(["--config", CONFIG, "--model", "synthetic", "--size", "256x192"] + args)
    return res["results"], out.getvalue()


def _files(folder):
    return {p.name: p.read_bytes() for p in sorted(folder.iterdir())}


@gpu
def test_gpu_predict_cli_flip_test(tmp_path):
    from PIL import Image
    from dll.utils import format_pose_labels
    predict = _script("predict")
    d = tmp_path
    for i, (stem, (h, w)) in enumerate(SHAPES.items()):
        Image.fromarray(np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f"{stem}.png")
    for stem, rows in LABELS.items():
        (d / f"{stem}.txt").write_text("".join("0 " + " ".join(str(v) for v in r) + "\n" for r in rows))
    common = ["--input", str(d), "--gt", str(d)]
    _, text_plain = _predict_cli(common + ["--output", str(d / "plain")])
    _, text_off = _predict_cli(common + ["--output", str(d / "off"), "--flip-test", "off"])
    results, text_on = _predict_cli(common + ["--output", str(d / "on"), "--flip-test"])
    plain, off, on = _files(d / "plain"), _files(d / "off"), _files(d / "on")
    assert sorted(plain) == ["a_keypoints.png", "a_keypoints.txt", "c_keypoints.png", "c_keypoints.txt"]
    assert off == plain and text_off == text_plain                  # byte for byte
    assert sorted(on) == sorted(plain)
    assert on["a_keypoints.txt"] != plain["a_keypoints.txt"] and on["a_keypoints.png"] != plain["a_keypoints.png"]
    assert on["a_keypoints.txt"].count(b"\n") == 2
    # the label file holds the merged outputs of an independent flip-test forward
    cfg = predict.load_config(CONFIG)
    model = predict.load_model("synthetic", cfg, DEV, "split")
    model.flip_test = True
    transform = predict.make_transform(cfg["model"]["backbone"].get("in_channels", 3), (256, 192), DEV)
    image = Image.open(d / "a.png").convert("RGB")
    with torch.no_grad():
        out = model({"image": transform.batch([image]).to(DEV), "bboxes": torch.tensor([LABELS["a"]], device=DEV)})
    assert "keypoint_peaks" in out
    assert on["a_keypoints.txt"].decode() == format_pose_labels(out)
    got = dict(results)[d / "a.png"]
    assert torch.equal(got["keypoints"], out["keypoints"]) and torch.equal(got["heatmap"], out["heatmap"])
    # the detector image went through the merge as well
    det = dict(results)[d / "c.png"]
    assert "keypoint_peaks" in det and torch.equal(det["keypoint_peaks"], det["heatmap"].amax((-2, -1)))
