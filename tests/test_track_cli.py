"""scripts/predict.py --track on the GPU: a directory of three copies of one
image as a frame sequence.  The input is constant, so the One-Euro filter
returns the forward's keypoints bit for bit (tests/test_track.py states why)
and every file but tracks.txt equals the run without the option; the chunked
pipeline carries the tracker's state from chunk to chunk and does not show it
a file that failed to decode.  The flag parsing is tested without a GPU in
tests/test_track_cpu.py."""
import contextlib
import io
import logging
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOXES = [[0.5, 0.5, 0.4, 0.8], [0.3, 0.4, 0.2, 0.3]]
FRAMES = ("f0", "f1", "f2")
K = 17


def _script(name):
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    return __import__(name)


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
    return res, records, out.getvalue()


def _write_frames(d, names):
    from PIL import Image
    pixels = np.random.default_rng(5).integers(0, 256, (150, 200, 3), dtype=np.uint8)
    for stem in names:
        Image.fromarray(pixels).save(d / f"{stem}.png")
        (d / f"{stem}.txt").write_text("".join("0 " + " ".join(str(v) for v in r) + "\n" for r in BOXES))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("track_predict")
    _write_frames(d, FRAMES)
    common = ["--input", str(d), "--gt", str(d)]
    plain = _predict_cli(common + ["--output", str(d / "plain")])
    tracked = _predict_cli(common + ["--output", str(d / "track"), "--track"])
    return d, plain, tracked


def _files(folder):
    return {p.name: p.read_bytes() for p in sorted(folder.iterdir())}


def _parse(text):
    """tracks.txt -> [(frame, id, score, box [4], keypoint tokens)]; every float must be written as %.6f."""
    rows = []
    for line in text.splitlines():
        tok = line.split()
        assert len(tok) == 7 + 3 * K, line
        floats = tok[2:7] + [t for i, t in enumerate(tok[7:]) if i % 3 != 2]
        assert all(t == f"{float(t):.6f}" for t in floats), line
        assert all(int(t) in (0, 1, 2) for t in tok[9::3])
        rows.append((int(tok[0]), int(tok[1]), float(tok[2]), tok[3:7], tok[7:]))
    return rows


@gpu
def test_gpu_without_the_option_nothing_changes(runs):
    d, (_, log, text), _ = runs
    plain = _files(d / "plain")
    assert sorted(plain) == sorted(f"{s}_keypoints{e}" for s in FRAMES for e in (".png", ".txt"))
    _, log_off, text_off = _predict_cli(["--input", str(d), "--gt", str(d), "--output", str(d / "off"), "--track", "off",
                                         "--track-threshold", "0.9", "--track-no-smooth"])
    assert _files(d / "off") == plain and text_off == text
    assert [m.replace("/off/", "/plain/") for m in log_off] == log


@gpu
def test_gpu_track_writes_tracks_and_the_same_label_files(runs):
    d, (plain_res, _, text), (res, log, text_tracked) = runs
    plain, tracked = _files(d / "plain"), _files(d / "track")
    assert sorted(tracked) == sorted(list(plain) + ["tracks.txt"])
    for name, data in plain.items():                       # constant input: the smoothed poses are the forward's
        assert tracked[name] == data, name
    assert text_tracked == text and any(m.startswith("tracking on") for m in log)
    rows = _parse(tracked["tracks.txt"].decode())
    assert [r[0] for r in rows] == [0, 0, 1, 1, 2, 2] and [r[1] for r in rows] == [0, 1] * 3
    assert all(0.0 < r[2] <= 1.0 for r in rows)
    for stem, pair in zip(FRAMES, (rows[0:2], rows[2:4], rows[4:6])):
        labels = [line.split() for line in plain[f"{stem}_keypoints.txt"].decode().splitlines()]
        assert len(labels) == 2
        for row, label in zip(pair, labels):               # the label line after its class, token for token
            assert row[3] + row[4] == label[1:]
    for (path, out), (_, out_plain) in zip(res["results"], plain_res["results"]):
        assert out["track_ids"].tolist() == [[0, 1]] and out["track_ids"].dtype == torch.int32
        assert out["keypoints"].shape == out_plain["keypoints"].shape == (1, 2, 1, K, 2)
        assert torch.equal(out["keypoints"], out_plain["keypoints"]) and torch.equal(out["keypoints_raw"], out["keypoints"])
        assert "track_ids" not in out_plain
    assert [int(out["track_hits"][0, 0]) for _, out in res["results"]] == [1, 2, 3]


@gpu
def test_gpu_state_carries_over_chunks_and_skips_undecodable_files(runs, tmp_path):
    from dll.utils import PoseTracker
    predict = _script("predict")
    _, _, (res, _, _) = runs
    model = res["model"]
    _write_frames(tmp_path, ("f0", "f1", "f3"))
    (tmp_path / "f2.png").write_bytes(b"not an image")         # frame 2 of the sorted list: logged and skipped
    cfg = predict.load_config(PKG / "configs" / "default_config.yaml")
    transform = predict.make_transform(cfg["model"]["backbone"].get("in_channels", 3), (256, 192), DEV)
    tracker = PoseTracker(K, device=DEV, max_age=0)            # a frame the tracker saw without the persons would kill them
    with contextlib.redirect_stdout(io.StringIO()):
        results = predict.predict_directory_nms(model, tmp_path, transform, DEV, tmp_path / "out", gt_dir=tmp_path,
                                                batch_size=2, track=tracker)
    assert [p.name for p, _ in results] == ["f0.png", "f1.png", "f3.png"]
    assert [out["track_ids"].tolist() for _, out in results] == [[[0, 1]]] * 3      # chunks (f0, f1) and (f2, f3)
    assert [out["track_hits"].tolist() for _, out in results] == [[[1, 1]], [[2, 2]], [[3, 3]]]
    rows = _parse((tmp_path / "out" / "tracks.txt").read_text())
    assert [r[0] for r in rows] == [0, 0, 1, 1, 3, 3] and [r[1] for r in rows] == [0, 1] * 3
    with pytest.raises(ValueError):
        predict.predict_directory_nms(model, tmp_path, transform, DEV, None, reference_zeros=True, track=tracker)


@gpu
def test_gpu_track_with_the_person_detector_and_pose_nms(runs, tmp_path):
    """No label files: the detector's boxes, pose-NMS in front of the tracker.  As many tracks.txt lines per frame as
    label lines, the same ids in every frame (the frames are identical), a suppressed or empty slot has id -1."""
    d, _, _ = runs
    from PIL import Image
    for stem in FRAMES:
        Image.open(d / f"{stem}.png").save(tmp_path / f"{stem}.png")
    res, _, _ = _predict_cli(["--input", str(tmp_path), "--output", str(tmp_path / "out"), "--track", "--pose-nms", "hard"])
    files = _files(tmp_path / "out")
    rows = _parse(files["tracks.txt"].decode())
    per_frame = [[r for r in rows if r[0] == f] for f in range(3)]
    counts = [files[f"{s}_keypoints.txt"].count(b"\n") for s in FRAMES]
    assert [len(p) for p in per_frame] == counts and counts[0] == counts[1] == counts[2]
    assert [r[1] for r in per_frame[0]] == [r[1] for r in per_frame[1]] == [r[1] for r in per_frame[2]]
    assert sorted(r[1] for r in per_frame[0]) == list(range(counts[0]))
    for _, out in res["results"]:
        present = out["track_scores"][0] > 0
        assert ((out["track_ids"][0] >= 0) == present).all() and int(present.sum()) == counts[0]
        assert torch.equal(out["keypoints"], out["keypoints_raw"])
