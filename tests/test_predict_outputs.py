"""scripts/predict.py writes what it logs: per image the device-drawn overlay
``<stem>_keypoints<suffix>`` at the image's own resolution and the label file
``<stem>_keypoints.txt``, for a directory (one labelled image, one on the
detector path) and for a single file."""
import contextlib
import io
import logging
import sys

import numpy as np
import pytest
import torch

import draw_ref as R
from conftest import PKG

gpu = pytest.mark.gpu
H, W = 256, 192                                   # the size tests/test_predict_directory.py runs at
LABELS = {"a": [[0.5, 0.5, 0.4, 0.8], [0.3, 0.4, 0.2, 0.3]]}      # "c" has no label file: person detector
SHAPES = {"a": (200, 150), "c": (170, 130)}
SEEDS = {"a": 0, "c": 2}


def _predict():
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    import predict
    return predict


def _image(stem):
    h, w = SHAPES[stem]
    rng = np.random.default_rng(SEEDS[stem])
    yy, xx = np.mgrid[0:h, 0:w]
    shape = ((xx > w * 0.4) * 90 + (((yy - h / 2) ** 2 + (xx - w / 2) ** 2) < (min(h, w) / 3) ** 2) * 60)
    return ((rng.integers(0, 80, (h, w, 3)) + shape[..., None]) % 256).astype(np.uint8)


def _main(predict, args):
    records = []

    class _Keep(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())

    root, handler = logging.getLogger(), _Keep()
    level = root.level
    root.addHandler(handler)
    root.setLevel(logging.INFO)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            res = predict.main(["--config", str(PKG / "configs" / "default_config.yaml"), "--model", "synthetic",
                                "--size", f"{H}x{W}"] + args)
    finally:
        root.removeHandler(handler)
        root.setLevel(level)
    return res["results"], records


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from PIL import Image
    predict = _predict()
    d = tmp_path_factory.mktemp("predict_out")
    for stem in SHAPES:
        Image.fromarray(_image(stem)).save(d / f"{stem}.png")
    for stem, rows in LABELS.items():
        (d / f"{stem}.txt").write_text("".join("0 " + " ".join(str(v) for v in r) + "\n" for r in rows))
    results, log = _main(predict, ["--input", str(d), "--gt", str(d), "--output", str(d / "out")])
    single, slog = _main(predict, ["--input", str(d / "a.png"), "--gt", str(d / "a.txt"), "--output", str(d / "one")])
    return {"dir": d, "results": results, "log": log, "single": single, "single_log": slog}


def _expected(stem, out):
    """draw_ref on one image's returned outputs, with the wrapper's box rule restated: detector slots with
    score 0 get zero boxes (the labelled image's boxes hold no all-zero row to compact)."""
    from dll.utils import DrawStyle
    kp = out["keypoints"].cpu().numpy()[:, :, 0]
    vis = out["visibilities"].cpu().numpy()[:, :, 0]
    boxes = out["boxes"][0].cpu().numpy()[None].astype(np.float32)
    if "box_scores" in out:
        boxes = boxes * (out["box_scores"].cpu().numpy()[..., None] > 0)
    want = R.draw_ref([_image(stem)], kp, vis, boxes, None, R.style_of(DrawStyle()), R.BOXES | R.LIMBS | R.JOINTS)[0]
    return want, kp, vis, boxes


def _parse(path):
    from dll.data.dataloader import OptimizedKeypointsDataset
    ds = object.__new__(OptimizedKeypointsDataset)
    ds.num_keypoints = 17
    return ds._parse_label_file_vectorized(path)


def _check_files(out_dir, stem, out):
    from PIL import Image
    png, txt = out_dir / f"{stem}_keypoints.png", out_dir / f"{stem}_keypoints.txt"
    assert png.exists() and txt.exists()
    got = np.asarray(Image.open(png))
    assert got.shape == (*SHAPES[stem], 3)
    want, kp, vis, boxes = _expected(stem, out)
    assert np.array_equal(got, want) and (want != _image(stem)).any()
    drawn = [p for p in range(boxes.shape[1]) if boxes[0, p].any()]
    assert drawn
    ann = _parse(txt)
    assert ann.keypoints.shape == (1, len(drawn), 17, 2)
    assert np.abs(ann.keypoints[0].numpy() - kp[0, drawn]).max() <= 1e-6
    assert np.abs(ann.bboxes[0].numpy() - boxes[0, drawn]).max() <= 1e-6
    assert np.array_equal(ann.visibilities[0].numpy(), vis[0, drawn].argmax(-1))


@gpu
def test_directory_writes_overlay_and_labels(run):
    assert [p.name for p, _ in run["results"]] == ["a.png", "c.png"]
    for path, out in run["results"]:
        _check_files(run["dir"] / "out", path.stem, out)
    assert sorted(p.name for p in (run["dir"] / "out").iterdir()) == [
        "a_keypoints.png", "a_keypoints.txt", "c_keypoints.png", "c_keypoints.txt"]
    for stem in SHAPES:
        assert f"Saved visualization to {run['dir'] / 'out' / (stem + '_keypoints.png')}" in run["log"]


@gpu
def test_single_file_writes_both_files(run):
    (path, out), = run["single"]
    _check_files(run["dir"] / "one", "a", out)
    assert f"Saved visualization to {run['dir'] / 'one' / 'a_keypoints.png'}" in run["single_log"]
    # the single-image overlay is the directory's
    assert (run["dir"] / "one" / "a_keypoints.txt").read_text().count("\n") == 2


@gpu
def test_visualize_keypoints_multi_person(run, tmp_path):
    """The reference's import target on returned outputs: the array it returns is the file it saves."""
    from PIL import Image
    from dll.data.dataloader import visualize_keypoints_multi_person
    out = run["results"][0][1]
    want, kp, vis, boxes = _expected("a", out)
    got = visualize_keypoints_multi_person(Image.fromarray(_image("a")), kp[0], vis[0], boxes[0],
                                           save_path=tmp_path / "v.png")
    assert np.array_equal(got, want) and np.array_equal(np.asarray(Image.open(tmp_path / "v.png")), want)
