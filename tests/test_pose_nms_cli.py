"""--pose-nms in scripts/evaluate.py and scripts/predict.py, and what OKS
pose-NMS does to COCO keypoint AP: every labelled pose of a small YOLO-pose
split (tests/golden/data_cases.LABEL_CASES) fed back as a prediction together
with an exact lower-scoring copy.  Unsuppressed, each copy is a false positive
that ranks between true positives; after suppress_poses(mode="hard") the four
numbers are 1 (within 1e-12, tests/test_oks.py states why).  With --pose-nms
off both scripts print and write exactly what they do without the option."""
import contextlib
import io
import json
import logging
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oks_ref
from conftest import PKG

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from data_cases import LABEL_CASES  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
OKS_KEYS = {"oks_AP", "oks_AP50", "oks_AP75", "oks_AR"}
f32 = np.float32
NAMES = ("two", "one", "ragged")
SIZE = (128, 96)                                       # (W, H) of every image of the split


def _script(name):
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    return __import__(name)


# ------------------------------------------------------------------ CPU: the flags are parsed before any device use
def test_both_scripts_reject_an_unknown_pose_nms_choice(capsys):
    evaluate, predict = _script("evaluate"), _script("predict")
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--config", "nowhere.yaml", "--model", "synthetic", "--dataset-dir", "nowhere", "--metric", "oks",
                       "--pose-nms", "maybe"])
    assert e.value.code == 2 and "--pose-nms" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        predict.main(["--config", "nowhere.yaml", "--model", "synthetic", "--input", "nowhere", "--output", "nowhere",
                      "--pose-nms", "maybe"])
    assert e.value.code == 2 and "--pose-nms" in capsys.readouterr().err


def test_evaluate_rejects_pose_nms_with_the_slotwise_metric(capsys):
    evaluate = _script("evaluate")
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--config", "nowhere.yaml", "--model", "synthetic", "--dataset-dir", "nowhere", "--pose-nms", "hard"])
    assert e.value.code == 2 and "--metric oks" in capsys.readouterr().err


def test_option_helpers():
    import argparse
    predict = _script("predict")
    ap = argparse.ArgumentParser()
    predict.add_pose_nms_arguments(ap)
    assert predict.pose_nms_options(ap.parse_args([])) is None
    assert predict.pose_nms_options(ap.parse_args(["--pose-nms", "off", "--pose-nms-threshold", "0.5"])) is None
    got = predict.pose_nms_options(ap.parse_args(["--pose-nms", "soft-linear", "--pose-nms-vis", "0.3"]))
    assert got == {"mode": "soft_linear", "threshold": 0.9, "vis_threshold": 0.3}


# ------------------------------------------------------------------ duplicated labels as predictions
def _duplicated_labels():
    """The labels of NAMES as arrays (G = 2 slots, K = 17; short rows zero padded) and as predictions: slots
    0..G-1 the labelled poses at score 0.9 - 0.1 g, slots G..2G-1 exact copies at 0.85 - 0.1 g."""
    B, G, K = len(NAMES), 2, 17
    kp, vis, boxes = np.zeros((B, G, K, 2), f32), np.zeros((B, G, K), f32), np.zeros((B, G, 4), f32)
    n = np.zeros(B, np.int32)
    for b, name in enumerate(NAMES):
        rows = [[float(v) for v in line.split()] for line in LABEL_CASES[name].splitlines() if line.strip()]
        n[b] = len(rows)
        for g, row in enumerate(rows):
            boxes[b, g] = row[1:5]
            trip = np.array(row[5:], f32).reshape(-1, 3)[:K]
            kp[b, g, :len(trip)], vis[b, g, :len(trip)] = trip[:, :2], trip[:, 2]
    scale = np.tile(np.array(SIZE, f32), (B, 1))
    area = boxes[..., 2] * boxes[..., 3] * scale[:, 0:1] * scale[:, 1:2]
    present = np.arange(G)[None] < n[:, None]
    scores = np.concatenate([np.where(present, 0.9 - 0.1 * np.arange(G), 0), np.where(present, 0.85 - 0.1 * np.arange(G), 0)],
                            1).astype(f32)
    gt = dict(gt_kpts=kp, gt_vis=vis, gt_boxes=boxes, gt_area=area.astype(f32), n_gt=n, scale=scale)
    return gt, np.concatenate([kp, kp], 1), scores, np.concatenate([boxes, boxes], 1)


def test_duplicates_cost_precision_without_suppression():
    gt, pred, scores, _ = _duplicated_labels()
    assert list(gt["n_gt"]) == [2, 1, 2] and (gt["gt_vis"].sum(-1)[gt["gt_boxes"].any(-1)] > 0).all()
    got = oks_ref.average_precision([oks_ref.evaluate_batch(pred, scores, **gt)])
    assert got["oks_AP"] < 0.9 and got["oks_AR"] == 1.0, got
    clean = oks_ref.average_precision([oks_ref.evaluate_batch(pred[:, :2], scores[:, :2], **gt)])
    assert clean == {k: 1.0 for k in OKS_KEYS}


@gpu
def test_gpu_hard_suppression_restores_ap_one():
    from dll.utils import OksEvaluator, suppress_poses
    gt, pred, scores, boxes = _duplicated_labels()
    dev = lambda a: torch.from_numpy(a).to(DEV)     # noqa: E731
    batch = {"keypoints": dev(gt["gt_kpts"]), "visibilities": dev(gt["gt_vis"]), "bboxes": dev(gt["gt_boxes"]),
             "num_persons": dev(gt["n_gt"]).long(), "orig_size": [SIZE] * len(NAMES)}
    out = {"keypoints": dev(pred)[:, :, None].contiguous(), "boxes": dev(boxes), "box_scores": dev(scores)}
    ev = OksEvaluator()
    ev.update(out, batch, scores=out["box_scores"])
    raw = ev.summarize()
    want = oks_ref.average_precision([oks_ref.evaluate_batch(pred, scores, **gt)])
    assert all(abs(raw[k] - want[k]) <= 1e-12 for k in OKS_KEYS) and raw["oks_AP"] < 0.9
    kept = suppress_poses(out, batch["orig_size"], mode="hard", rescore=False, return_oks=True)
    assert kept["pose_n_keep"].tolist() == [2, 1, 2]
    assert kept["pose_keep"].tolist() == [[0, 1, -1, -1], [0, -1, -1, -1], [0, 1, -1, -1]]
    assert torch.equal(kept["pose_scores"][:, :2], out["box_scores"][:, :2]) and (kept["pose_scores"][:, 2:] == 0).all()
    assert kept["pose_oks"][0, 0, 2] == 1.0 and kept["pose_oks"][0, 1, 3] == 1.0 and kept["pose_oks"][0, 0, 1] < 0.5
    ev.reset()
    ev.update(kept, batch, scores=kept["pose_scores"])
    got = ev.summarize()
    print(raw, got)
    assert set(got) == OKS_KEYS and all(abs(got[k] - 1.0) <= 1e-12 for k in OKS_KEYS), got


# ------------------------------------------------------------------ GPU: evaluate.py
def _write_dataset(root: Path, size=(120, 90)):
    from PIL import Image
    rng = np.random.default_rng(1)
    (root / "val" / "images").mkdir(parents=True)
    (root / "val" / "labels").mkdir(parents=True)
    for n in NAMES:
        Image.fromarray(rng.integers(0, 256, (*size, 3), dtype=np.uint8)).save(root / "val" / "images" / f"{n}.png")
        (root / "val" / "labels" / f"{n}.txt").write_text(LABEL_CASES[n])


def _evaluate_cli(root, capsys, *extra):
    evaluate = _script("evaluate")
    m = evaluate.main(["--config", str(PKG / "configs" / "default_config.yaml"), "--model", "synthetic",
                       "--dataset-dir", str(root), "--split", "val", "--batch-size", "2", "--boxes", "detector",
                       "--metric", "oks", *extra])
    return m, capsys.readouterr().out.strip().splitlines()[-1]


@gpu
def test_gpu_evaluate_cli_pose_nms_hard(tmp_path, capsys):
    _write_dataset(tmp_path)
    m, text = _evaluate_cli(tmp_path, capsys, "--pose-nms", "hard")
    line = json.loads(text)
    assert '"pose_nms": "hard"' in text and line["pose_nms"] == "hard"
    assert set(m) == OKS_KEYS and set(line) == OKS_KEYS | {"split", "batches", "boxes", "images", "pose_nms"}
    assert line["boxes"] == "detector" and line["images"] == 3 and line["batches"] == 2
    assert all(0.0 <= line[k] <= 1.0 or line[k] == -1.0 for k in OKS_KEYS)


@gpu
def test_gpu_evaluate_cli_pose_nms_off_prints_the_same_line(tmp_path, capsys):
    _write_dataset(tmp_path)
    _, plain = _evaluate_cli(tmp_path, capsys)
    _, off = _evaluate_cli(tmp_path, capsys, "--pose-nms", "off", "--pose-nms-threshold", "0.5")
    assert off == plain and "pose_nms" not in plain


# ------------------------------------------------------------------ GPU: predict.py
LABELS = {"a": [[0.5, 0.5, 0.4, 0.8], [0.5, 0.5, 0.4, 0.8], [0.3, 0.4, 0.2, 0.3]]}     # the first box twice
SHAPES = {"a": (200, 150), "c": (170, 130)}                                           # "c": the person detector


def _predict_cli(args):
    predict = _script("predict")
    records = []

    class _Keep(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())

    root, handler = logging.getLogger(), _Keep()
    level = root.level
    root.addHandler(handler)
    root.setLevel(logging.INFO)
    try:
        with contextlib.redirect_stdout(io.StringIO()) as out:
            res = predict.main(["--config", str(PKG / "configs" / "default_config.yaml"), "--model", "synthetic",
                                "--size", "256x192"] + args)
    finally:
        root.removeHandler(handler)
        root.setLevel(level)
    return res["results"], records, out.getvalue()


@pytest.fixture(scope="module")
def predict_inputs(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("pose_nms_predict")
    for i, (stem, (h, w)) in enumerate(SHAPES.items()):
        Image.fromarray(np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f"{stem}.png")
    for stem, rows in LABELS.items():
        (d / f"{stem}.txt").write_text("".join("0 " + " ".join(str(v) for v in r) + "\n" for r in rows))
    _, log, text = _predict_cli(["--input", str(d), "--gt", str(d), "--output", str(d / "plain")])
    return d, log, text


def _files(folder):
    return {p.name: p.read_bytes() for p in sorted(folder.iterdir())}


@gpu
def test_gpu_predict_cli_pose_nms_off_writes_identical_files(predict_inputs):
    d, log, text = predict_inputs
    _, log_off, text_off = _predict_cli(["--input", str(d), "--gt", str(d), "--output", str(d / "off"), "--pose-nms", "off"])
    plain, off = _files(d / "plain"), _files(d / "off")
    assert sorted(plain) == ["a_keypoints.png", "a_keypoints.txt", "c_keypoints.png", "c_keypoints.txt"]
    assert plain == off and text == text_off
    assert [m.replace("/off/", "/plain/") for m in log_off] == log
    assert plain["a_keypoints.txt"].count(b"\n") == 3


@gpu
def test_gpu_predict_cli_pose_nms_hard_drops_the_doubled_person(predict_inputs):
    d, log, _ = predict_inputs
    results, log_hard, _ = _predict_cli(["--input", str(d), "--gt", str(d), "--output", str(d / "hard"),
                                         "--pose-nms", "hard"])
    plain, hard = _files(d / "plain"), _files(d / "hard")
    assert sorted(hard) == sorted(plain)
    lines, lines_plain = hard["a_keypoints.txt"].splitlines(), plain["a_keypoints.txt"].splitlines()
    assert len(lines_plain) == 3 and lines_plain[0] == lines_plain[1]              # the doubled person, twice
    assert 1 <= len(lines) <= 2 and lines[0] == lines_plain[0] and lines.count(lines[0]) == 1
    out = dict(results)[d / "a.png"]
    keep = out["pose_keep"][0].tolist()
    assert 0 in keep and 1 not in keep and out["box_scores"][0].tolist()[:2] == [1.0, 0.0]
    assert out["pose_n_keep"].shape == (1,) and out["keypoints"].shape[:2] == (1, 3)
    # the detector image: as many label lines as the log says persons were kept
    kept = [m for m in log_hard if m.startswith("detector kept")]
    assert len(kept) == 1
    n = int(kept[0].split()[2])
    det = dict(results)[d / "c.png"]
    assert n == int((det["box_scores"][0] > 0).sum()) == int(det["pose_n_keep"][0])
    assert hard["c_keypoints.txt"].count(b"\n") == n <= plain["c_keypoints.txt"].count(b"\n")
    # a single file takes the same path
    single, _, _ = _predict_cli(["--input", str(d / "a.png"), "--gt", str(d / "a.txt"), "--output", str(d / "one"),
                                 "--pose-nms", "hard"])
    one = _files(d / "one")
    assert sorted(one) == ["a_keypoints.png", "a_keypoints.txt"]
    assert one["a_keypoints.txt"].count(b"\n") == len(lines) and torch.equal(single[0][1]["pose_keep"], out["pose_keep"])
