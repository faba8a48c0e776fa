"""scripts/predict.py predict_directory: a directory as one batched device
pipeline (host decode -> ITransform.batch -> one forward per mode), against
the oracle's forward, the single-image path and the reference's printout."""
import contextlib
import inspect
import io
import logging
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import kpd_oracle as O
from oracle import preprocess_oracle as PO

H, W = 256, 192
# label lines per image stem: 2 persons, 1 person; "c" has no label file (person detector)
LABELS = {"a": [[0.5, 0.5, 0.4, 0.8], [0.3, 0.4, 0.2, 0.3]], "b": [[0.45, 0.55, 0.5, 0.7]]}
SHAPES = {"a": (200, 150), "b": (240, 180), "c": (170, 130)}
# Visibility class = sigmoid(max of the sigmoid heatmap) against 0.3 / 0.7, i.e. the heatmap maximum against
# logit(0.7) = 0.8473 (0.3 is out of reach).  Seeds 0, 1, 2 below: the oracle's 51 maxima (3 persons x 17) stay at
# least 0.054 away from it -- computed on the CPU beforehand and asserted below with a bound of 0.01 -- against the
# split mode's 5e-5 heatmap tolerance.
SEEDS = {"a": 0, "b": 1, "c": 2}
VIS_MARGIN = 1e-2


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


def _oracle_given(sd):
    """O.forward on the oracle-preprocessed labelled images and their zero-padded boxes."""
    x = torch.from_numpy(np.stack([PO.itransform_gray(_image(s), (H, W), 2.0, (8, 8)) for s in ("a", "b")]))
    boxes = torch.zeros(2, 2, 4)
    boxes[0] = torch.tensor(LABELS["a"])
    boxes[1, :1] = torch.tensor(LABELS["b"])
    return O.forward(sd, {"image": x, "bboxes": boxes})


def test_predict_directory_signature():
    predict = _predict()
    params = list(inspect.signature(predict.predict_directory).parameters.values())
    assert [p.name for p in params[:5]] == ["model", "input_dir", "transform", "device", "output_dir"]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and p.default is inspect.Parameter.empty
               for p in params[:5])
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[5:])
    assert {p.name: p.default for p in params[5:]} == {"gt_dir": None, "reference_zeros": False, "batch_size": 64}


def test_itransform_batch_exists_without_device():
    from dll.data import ITransform
    assert callable(ITransform(img_size=(H, W), clip_limit=2.0, tile_size=(8, 8), device="cpu").batch)


def test_oracle_visibilities_clear_of_thresholds(model_sd_gray):
    """No device: the margin the comment at SEEDS quotes."""
    ref = _oracle_given(model_sd_gray)
    mx = ref["heatmap"].amax(dim=(-1, -2))                          # [2 images, 2 persons, 17]
    valid = torch.tensor([[True, True], [True, False]])             # b's second slot is the zero padding
    margin = (mx[valid] - float(np.log(0.7 / 0.3))).abs().min()
    assert margin > VIS_MARGIN, float(margin)


gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One `predict.py --input <dir> --gt <dir>` run: three PNGs of different
    sizes (labels with 2 and 1 persons, one without a label) and a truncated PNG."""
    from PIL import Image
    predict = _predict()
    d = tmp_path_factory.mktemp("predict_dir")
    for stem in SHAPES:
        Image.fromarray(_image(stem)).save(d / f"{stem}.png")
    for stem, rows in LABELS.items():
        (d / f"{stem}.txt").write_text("".join("0 " + " ".join(str(v) for v in r) + "\n" for r in rows))
    data = (d / "a.png").read_bytes()
    (d / "broken.png").write_bytes(data[:len(data) // 2])
    records = []

    class _Keep(logging.Handler):
        def emit(self, record):
            records.append((record.levelno, record.getMessage()))

    root, handler, out = logging.getLogger(), _Keep(), io.StringIO()
    level = root.level
    root.addHandler(handler)
    root.setLevel(logging.INFO)
    try:
        with contextlib.redirect_stdout(out):
            res = predict.main(["--config", str(PKG / "configs" / "default_config.yaml"), "--model", "synthetic",
                                "--input", str(d), "--gt", str(d), "--output", str(d / "out"),
                                "--size", f"{H}x{W}"])
    finally:
        root.removeHandler(handler)
        root.setLevel(level)
    return {"dir": d, "model": res["model"], "results": res["results"], "stdout": out.getvalue(), "log": records,
            "predict": predict}


@gpu
def test_directory_results_in_order_and_shapes(run):
    assert [p.name for p, _ in run["results"]] == ["a.png", "b.png", "c.png"]
    a, b, c = (o for _, o in run["results"])
    assert a["keypoints"].shape == (1, 2, 1, 17, 2) and a["visibilities"].shape == (1, 2, 1, 17, 3)
    assert b["keypoints"].shape == (1, 1, 1, 17, 2) and b["heatmap"].shape == (1, 1, 17, 56, 56)
    assert c["keypoints"].shape == (1, 5, 1, 17, 2) and c["box_scores"].shape == (1, 5)
    assert len(a["boxes"]) == 1 and a["boxes"][0].shape == (2, 4) and b["boxes"][0].shape == (1, 4)
    msgs = [m for _, m in run["log"]]
    assert "a.png: boxes from given boxes" in msgs and "b.png: boxes from given boxes" in msgs
    assert "c.png: boxes from person detector" in msgs
    # the truncated file is logged as an error and skipped; the batch goes on
    assert any(lv == logging.ERROR and "broken.png" in m for lv, m in run["log"])
    assert run["stdout"].count("Predicted Keypoints:") == 3


@gpu
def test_directory_given_boxes_vs_oracle(run):
    sd = {k: v.cpu() for k, v in run["model"].state_dict().items()}
    ref = _oracle_given(sd)
    for i, persons in ((0, 2), (1, 1)):
        out = run["results"][i][1]
        np.testing.assert_allclose(out["keypoints"].cpu().numpy(), ref["keypoints"][i:i + 1, :persons].numpy(),
                                   atol=1e-5)
        assert torch.equal(out["visibilities"].cpu(), ref["visibilities"][i:i + 1, :persons])


@gpu
def test_directory_detector_image_vs_oracle(run):
    """The unlabelled image as test_predict_cli_detector checks it: the boxes
    equal the oracle's detector on the same FPN level 0 (read back from a
    repeat of that one-image detector forward)."""
    from PIL import Image
    from test_gpu_parity import _check_detections
    predict, model = run["predict"], run["model"]
    out = run["results"][2][1]
    transform = predict.make_transform(1, (H, W), DEV)
    x = transform.batch([Image.open(run["dir"] / "c.png").convert("RGB")])
    with torch.no_grad():
        again = model({"image": x})
    assert torch.equal(again["boxes"][0], out["boxes"][0]) and torch.equal(again["box_scores"], out["box_scores"])
    feat = model.native_plan(DEV).debug_buffer("feat0").view(1, H // 2, W // 2, 128).permute(0, 3, 1, 2).cpu()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    ref_boxes, ref_scores = O.person_detect(feat, sd, H, W, 0.3, 0.3, 5)
    _check_detections(torch.stack([b.cpu() for b in out["boxes"]]), out["box_scores"].cpu(), ref_boxes, ref_scores,
                      "predict_directory detector")


@gpu
def test_directory_printout_per_image(run):
    """Every image's block is the reference's: shape line, 17 names, and the
    nose line of its own person 0."""
    predict = run["predict"]
    blocks = run["stdout"].split("\nPredicted Keypoints:\n")[1:]
    assert len(blocks) == 3
    for block, (_, out), shape in zip(blocks, run["results"], ("(2, 17, 2)", "(17, 2)", "(5, 17, 2)")):
        lines = block.splitlines()
        assert lines[0] == "-" * 40 and lines[1] == f"Keypoints shape: {shape}"
        k0 = out["keypoints"][0, 0, 0].cpu()
        assert lines[2] == f" 1. {'nose':<15} ({float(k0[0, 0]):.3f}, {float(k0[0, 1]):.3f})"
        assert [ln[4:].split()[0] for ln in lines[2:19]] == predict.KEYPOINT_NAMES


@gpu
def test_directory_matches_single_image_calls(run, capsys):
    """Each per-image result against predict_single_image on that file alone
    (keypoints atol 1e-5, visibilities equal); prints whether they were bit-equal."""
    predict, model, d = run["predict"], run["model"], run["dir"]
    transform = predict.make_transform(1, (H, W), DEV)
    bit_equal = {}
    for path, out in run["results"]:
        gt = d / f"{path.stem}.txt"
        single = predict.predict_single_image(model, path, transform, DEV, gt if gt.exists() else None,
                                              return_outputs=True)[1]
        assert single["keypoints"].shape == out["keypoints"].shape
        np.testing.assert_allclose(out["keypoints"].cpu().numpy(), single["keypoints"].cpu().numpy(), atol=1e-5)
        assert torch.equal(out["visibilities"], single["visibilities"])
        bit_equal[path.name] = bool(torch.equal(out["keypoints"], single["keypoints"])
                                    and torch.equal(out["heatmap"], single["heatmap"]))
    capsys.readouterr()
    print(f"predict_directory vs predict_single_image bit-equal: {bit_equal}")
