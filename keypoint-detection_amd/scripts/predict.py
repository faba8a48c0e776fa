#!/usr/bin/env python3
"""Keypoint prediction CLI -- same flags and printout as the reference
(scripts/predict.py:162-223, print format :118-129), with working imports.

    python scripts/predict.py --config configs/default_config.yaml \
        --model best_model.pth --input img.jpg --gt img.txt --output out/

Differences (documented in DESIGN.md):
  * ITransform runs on the device (dll.data.ITransform): its OpenCV stages
    (CLAHE, Canny edge blend, blur) are restated in HIP, since OpenCV is absent
    in this image; Resize/ToTensor/Normalize are bit-exact to Pillow;
  * ``--model synthetic`` builds the seeded synthetic weights (no trained
    checkpoint exists: the reference's outputs/best_model.pth is a missing blob);
  * ``--size HxW`` allows the non-square 256x192 input of BASELINE config C1;
  * ``--precision`` picks the numeric mode; the default is ``split``, the
    fp32-accurate headline path (f16 hi/lo x3 MFMA products), like the model's;
  * without ``--gt`` the reference passes ``bboxes=None`` (:99), which makes its
    model return all-zero keypoints (keypoint_model.py:111-113,123-135).  Here
    the person detector supplies the boxes instead (the
    build-defined glue of PERSON_HEAD + NMS, keypoint_model.py:114-119,
    person_head.py:96-139); ``--reference-zeros`` keeps the reference's zeros;
  * a directory ``--input`` runs through ``predict_directory`` (:133-160) as one
    batched device pipeline: host decode, one ``ITransform.batch`` and one
    forward per mode for every chunk of images, the reference's printout per
    image;
  * the reference logs "Saved visualization to ..." and writes nothing (its
    drawing import does not resolve).  Here every image leaves two files in
    ``--output``: ``<stem>_keypoints<suffix>``, the overlay (boxes, skeleton,
    joints) drawn on the device at the image's own resolution
    (``dll.utils.draw_poses``, one call per forward), and
    ``<stem>_keypoints.txt``, the prediction as YOLO-pose label lines;
  * ``--pose-nms hard|soft|soft-linear`` puts OKS pose-NMS
    (``dll.utils.suppress_poses``, kpd_pose_nms) between the forward and the
    outputs: of two boxes on one person only the higher-scoring pose is drawn,
    written and counted.  ``off`` (the default) changes nothing;
  * ``--flip-test`` turns on the model's flip-test (a second forward over the
    mirrored image, the two heatmaps merged and decoded by kpd_flip_merge):
    overlays, label files and the printout come from the merged outputs.
    Without the option nothing changes;
  * ``--track`` (directory input only) treats the sorted files as consecutive
    frames of one sequence: after the forwards (and pose-NMS) of every chunk
    the poses go through ``dll.utils.PoseTracker`` (kpd_track_poses: greedy
    OKS association with the live tracks, a One-Euro filter per joint along
    each track; the state carries from chunk to chunk).  Overlays and label
    files come from the smoothed poses, and ``<output>/tracks.txt`` lists every
    present pose as ``frame id score cx cy w h`` + K groups ``x y v``.  The
    tracker's defaults are unmeasured (no checkpoint, no sequence data).
    Without the option nothing changes.
Runs on the HIP device (the accelerated path has no CPU fallback).
"""
from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from dll.configs import (BackboneConfig, KeypointHeadConfig, ModelConfig,  # noqa: E402
                         PersonDetectionConfig, TrainingConfig)
from dll.data import ITransform  # noqa: E402
from dll.models import MultiPersonKeypointModel  # noqa: E402
from dll.utils import PoseTracker, draw_poses, format_pose_labels, suppress_poses  # noqa: E402
from dll.utils.draw import joint_classes, keypoints_tensor, person_boxes, visibilities_tensor  # noqa: E402
from dll.utils.oks import keypoint_peaks, pose_scores  # noqa: E402

KEYPOINT_NAMES = ["nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder",
                  "left_elbow", "right_elbow", "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee",
                  "right_knee", "left_ankle", "right_ankle"]


def load_config(path):
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


def setup_logging():
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")


def load_model(model_path, config_dict, device, precision="split"):
    """Reference load_model (:30-62): configs from the YAML, filtered
    strict=False state-dict load (weights_only -- nothing executable is
    unpickled)."""
    mc = config_dict["model"]
    model_config = ModelConfig(backbone=BackboneConfig(**mc["backbone"]),
                               person_head=PersonDetectionConfig(**mc["person_head"]),
                               keypoint_head=KeypointHeadConfig(**mc["keypoint_head"]),
                               num_keypoints=mc["keypoint_head"]["num_keypoints"])
    model = MultiPersonKeypointModel(model_config, TrainingConfig(), precision=precision)
    if str(model_path) == "synthetic":
        from dll.models.synthetic import synthetic_state_dict
        model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=0))
    else:
        ckpt = torch.load(model_path, map_location="cpu", weights_only=True)
        sd = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
        own = model.state_dict()
        model.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)
    return model.to(device).eval()


POSE_NMS_CHOICES = ("off", "hard", "soft", "soft-linear")


def add_pose_nms_arguments(ap):
    """--pose-nms / --pose-nms-threshold / --pose-nms-vis, shared with evaluate.py."""
    ap.add_argument("--pose-nms", default="off", choices=POSE_NMS_CHOICES,
                    help="OKS pose-NMS between pose scoring and the output (dll.utils.suppress_poses): hard "
                         "suppression, or soft score decay (Gaussian / linear)")
    ap.add_argument("--pose-nms-threshold", type=float, default=0.9, help="OKS threshold of --pose-nms")
    ap.add_argument("--pose-nms-vis", type=float, default=0.2,
                    help="keypoints whose heatmap peak is not above this in both poses do not count in the pose OKS")


def add_flip_test_argument(ap):
    """--flip-test [on|off], shared with evaluate.py: the bare option means on, the default is off."""
    ap.add_argument("--flip-test", nargs="?", const="on", default="off", choices=("on", "off"),
                    help="also run every image's left-right mirror and decode the average of the two heatmaps "
                         "(MultiPersonKeypointModel.flip_test, kpd_flip_merge); costs a second forward")


def flip_test_enabled(args) -> bool:
    return args.flip_test == "on"


def add_track_arguments(ap):
    """--track [on|off] and its options: the bare option means on, the default is off."""
    ap.add_argument("--track", nargs="?", const="on", default="off", choices=("on", "off"),
                    help="directory input only: treat the sorted files as consecutive frames and track the poses "
                         "across them (dll.utils.PoseTracker, kpd_track_poses); writes <output>/tracks.txt")
    ap.add_argument("--track-threshold", type=float, default=0.3,
                    help="OKS a pose needs with a track to continue it (unmeasured default)")
    ap.add_argument("--track-max-age", type=int, default=10,
                    help="frames a track survives without a match (unmeasured default)")
    ap.add_argument("--track-fps", type=float, default=30.0, help="frame rate the One-Euro filter assumes")
    ap.add_argument("--track-no-smooth", action="store_true",
                    help="associate only: leave the keypoints as the forward decoded them")


def track_options(args):
    """``PoseTracker`` options of the parsed flags, None with --track off."""
    if args.track == "off":
        return None
    return {"threshold": args.track_threshold, "max_age": args.track_max_age, "fps": args.track_fps,
            "smooth": not args.track_no_smooth}


def pose_nms_options(args):
    """``suppress_poses`` options of the parsed flags, None with --pose-nms off."""
    if args.pose_nms == "off":
        return None
    return {"mode": args.pose_nms.replace("-", "_"), "threshold": args.pose_nms_threshold,
            "vis_threshold": args.pose_nms_vis}


def _suppress(outputs, images, pose_nms):
    """``outputs`` after OKS pose-NMS at the decoded ``images``' own (W, H);
    unchanged without options, and when no forward ran: the all-zero [B, 1, K, 2]
    keypoints of a call without any box (``bboxes=None``, an empty label file)
    hold no pose to suppress."""
    if pose_nms is None or outputs["keypoints"].dim() != 5:
        return outputs
    return suppress_poses(outputs, [im.size for im in images], **pose_nms)


def make_transform(in_channels: int, size, device):
    """The reference's ITransform(img_size, clip_limit=2.0, tile_size=(8, 8))
    (predict.py:179-183) on the device (dll.data.ITransform, kpd_preprocess):
    the grayscale pipeline (CLAHE + edge blend) for a 1-channel backbone, the
    RGB pipeline for a 3-channel one."""
    return ITransform(img_size=size, clip_limit=2.0, tile_size=(8, 8), grayscale=(in_channels == 1), device=device)


def read_gt_boxes(gt_path, device):
    """YOLO label lines 'cls cx cy w h ...' -> [P,4] (reference :78-93)."""
    boxes = []
    with open(gt_path) as f:
        for line in f:
            d = line.strip().split()
            if len(d) >= 5:
                boxes.append([float(d[1]), float(d[2]), float(d[3]), float(d[4])])
    return torch.tensor(boxes, device=device)


def output_path_for(output_dir, image_path):
    """``<output_dir>/<stem>_keypoints<suffix>`` (reference :146, :195, :210)."""
    image_path = Path(image_path)
    return Path(output_dir) / f"{image_path.stem}_keypoints{image_path.suffix}"


def save_prediction(drawn, outputs, output_path):
    """Write one image's two files: the overlay ``drawn`` (uint8 [H, W, 3]
    device tensor at the image's own resolution -- the one host copy) to
    ``output_path`` and the prediction as YOLO-pose label text
    (``dll.utils.format_pose_labels``) beside it as ``<stem>_keypoints.txt``."""
    from PIL import Image
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(drawn.cpu().numpy()).save(output_path)
    output_path.with_suffix(".txt").write_text(format_pose_labels(outputs))


def predict_single_image(model, image_path, transform, device, gt_path=None, output_path=None,
                         reference_zeros=False, return_outputs=False, pose_nms=None):
    """Reference predict_single_image (:64-131).  Without a GT file the
    detector branch runs (``model({'image': x})``: no 'bboxes' key), unless
    ``reference_zeros`` asks for the reference's ``bboxes=None`` call.  With
    ``pose_nms`` (``suppress_poses`` options) the outputs go through OKS
    pose-NMS before anything is drawn, saved or logged.  With ``output_path``
    the overlay (drawn on the device, ``dll.utils.draw_poses``) and the label
    file are written (``save_prediction``)."""
    from PIL import Image
    image = Image.open(image_path).convert("RGB")
    x = transform(image).unsqueeze(0).to(device)
    bboxes = read_gt_boxes(gt_path, device) if gt_path and Path(gt_path).exists() else None
    if bboxes is not None:
        batch, mode = {"image": x, "bboxes": bboxes.unsqueeze(0)}, "given boxes"
    elif reference_zeros:
        batch, mode = {"image": x, "bboxes": None}, "reference zeros (bboxes=None)"
    else:
        batch, mode = {"image": x}, "person detector"
    logging.info(f"{Path(image_path).name}: boxes from {mode}")
    with torch.no_grad():
        outputs = _suppress(model(batch), [image], pose_nms)
    if output_path is not None:
        save_prediction(draw_poses([image], outputs)[0], outputs, output_path)
    if bboxes is None and not reference_zeros:
        n = int((outputs["box_scores"][0] > 0).sum())
        logging.info(f"detector kept {n} person(s); person 0 box (cx, cy, w, h) = "
                     f"{[round(float(v), 4) for v in outputs['boxes'][0][0]]}")
    keypoints = outputs["keypoints"].squeeze().cpu().numpy()
    print("\nPredicted Keypoints:")
    print("-" * 40)
    print(f"Keypoints shape: {keypoints.shape}")
    if len(keypoints.shape) == 3:
        keypoints = keypoints[0]
    for i, name in enumerate(KEYPOINT_NAMES):
        if i < len(keypoints):
            x_, y_ = keypoints[i]
            print(f"{i + 1:2d}. {name:<15} ({x_:.3f}, {y_:.3f})")
    return (keypoints, outputs) if return_outputs else keypoints


IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png")


def _print_keypoints(outputs):
    """The reference's printout (:104-129) of one image's outputs."""
    keypoints = outputs["keypoints"].squeeze().cpu().numpy()
    print("\nPredicted Keypoints:")
    print("-" * 40)
    print(f"Keypoints shape: {keypoints.shape}")
    if len(keypoints.shape) == 3:
        keypoints = keypoints[0]
    for i, name in enumerate(KEYPOINT_NAMES):
        if i < len(keypoints):
            x_, y_ = keypoints[i]
            print(f"{i + 1:2d}. {name:<15} ({x_:.3f}, {y_:.3f})")


def _slice_outputs(outputs, i, persons=None):
    """Image ``i`` of a batch's outputs, cut to its own person count: the
    shapes of a single-image call."""
    out = {}
    for k, v in outputs.items():
        if isinstance(v, torch.Tensor):
            v = v[i:i + 1]
            out[k] = v[:, :persons] if persons is not None and v.dim() >= 2 else v
        else:   # the per-image box list
            out[k] = [v[i] if persons is None else v[i][:persons]]
    return out


def _frames_in_order(groups, n, device):
    """The outputs of a chunk's forwards (``groups``: (image indices, batched
    outputs) per forward) as one outputs dict of ``n`` frames in frame order,
    zero padded to the chunk's largest person count: what ``PoseTracker.track``
    and ``draw_poses`` read ('keypoints', 'visibilities', 'boxes' in slot
    order, 'box_scores' = the base pose score, 0 for an absent or suppressed
    slot, and 'keypoint_peaks' in place of the heatmaps, which are not copied)."""
    shaped = []
    for indices, out in groups:
        kp = keypoints_tensor(out, len(indices))
        P, K = kp.shape[1], kp.shape[2]
        shaped.append((torch.tensor(indices, device=device), P, kp, visibilities_tensor(out, len(indices), P, K, device),
                       person_boxes(out, len(indices), P, device), pose_scores(out, rescore=False),
                       keypoint_peaks(out)))
    P, K = max(g[1] for g in shaped), shaped[0][2].shape[2]
    frames = {"keypoints": torch.zeros(n, P, 1, K, 2, device=device), "visibilities": torch.zeros(n, P, K, 3, device=device),
              "boxes": torch.zeros(n, P, 4, device=device), "box_scores": torch.zeros(n, P, device=device),
              "keypoint_peaks": torch.zeros(n, P, K, device=device)}
    for idx, p, kp, vis, boxes, base, peaks in shaped:
        frames["keypoints"][idx, :p, 0] = kp
        frames["visibilities"][idx, :p] = vis
        frames["boxes"][idx, :p] = boxes
        frames["box_scores"][idx, :p] = base
        frames["keypoint_peaks"][idx, :p] = peaks
    return frames


def format_track_lines(frame, outputs):
    """One frame's lines of ``tracks.txt``: per present pose (track score > 0)
    ``frame id score cx cy w h`` followed by K groups ``x y v`` -- floats as
    %.6f, id -1 for a pose without a table entry, v the visibility class."""
    kp = keypoints_tensor(outputs, 1).cpu()
    P, K = kp.shape[1], kp.shape[2]
    cls = joint_classes(visibilities_tensor(outputs, 1, P, K, "cpu")).clamp(min=0)
    boxes = person_boxes(outputs, 1, P, "cpu")
    ids, scores = outputs["track_ids"].cpu()[0], outputs["track_scores"].cpu()[0]
    lines = []
    for p in range(P):
        if not float(scores[p]) > 0:
            continue
        vals = [str(int(frame)), str(int(ids[p])), f"{float(scores[p]):.6f}"] + [f"{float(v):.6f}" for v in boxes[0, p]]
        for k in range(K):
            vals += [f"{float(kp[0, p, k, 0]):.6f}", f"{float(kp[0, p, k, 1]):.6f}", str(int(cls[0, p, k]))]
        lines.append(" ".join(vals) + "\n")
    return "".join(lines)


def predict_directory(model, input_dir, transform, device, output_dir, *, gt_dir=None, reference_zeros=False,
                      batch_size=64):
    """``predict_directory_nms`` without OKS pose-NMS: the reference's
    predict_directory (:133-160) and its arguments."""
    return predict_directory_nms(model, input_dir, transform, device, output_dir, gt_dir=gt_dir,
                                 reference_zeros=reference_zeros, batch_size=batch_size)


def predict_directory_nms(model, input_dir, transform, device, output_dir, *, gt_dir=None, reference_zeros=False,
                          batch_size=64, pose_nms=None, track=None):
    """Reference predict_directory (:133-160) as a batched device pipeline:
    the images with the reference's extensions, in sorted order, are decoded
    on the host; every chunk of at most ``batch_size`` is preprocessed by one
    ``transform.batch`` call and takes one forward per mode.  Images whose
    label file ``gt_dir/<stem>.txt`` exists form the given-boxes batch, their
    boxes zero padded to the chunk's largest person count (the forward skips
    all-zero boxes); the others form the person-detector batch, or the
    ``bboxes=None`` batch with ``reference_zeros``.  Each image logs its mode
    and prints the block of ``predict_single_image``.  A file that fails to
    decode is logged and skipped, as in the reference's try/except.  With
    ``pose_nms`` (``suppress_poses`` options) every forward's outputs go
    through OKS pose-NMS at its images' own sizes first.  With an
    ``output_dir`` every forward's batched outputs are drawn onto its images by
    one ``draw_poses`` call and each image's overlay and label file are written
    (``save_prediction``).  With ``track`` (a ``PoseTracker`` of one sequence)
    the files are consecutive frames: after its forwards and pose-NMS every
    chunk's outputs are put back in frame order, padded to the chunk's largest
    person count, and go through one ``track.track`` call (the state carries
    from chunk to chunk; a file that failed to decode is not seen); drawing
    and the label files use the tracked (smoothed) poses, the per-image
    outputs carry ``track_ids``, and ``<output_dir>/tracks.txt`` lists every
    present pose (``format_track_lines``; frame = the position in the sorted
    file list).  Returns ``[(path, outputs_i)]`` with the shapes of a
    single-image call."""
    from PIL import Image
    input_dir = Path(input_dir)
    if output_dir is not None:
        Path(output_dir).mkdir(parents=True, exist_ok=True)
    files = sorted(f for f in input_dir.glob("*") if f.suffix.lower() in IMAGE_EXTENSIONS)
    logging.info(f"Found {len(files)} images in {input_dir}")
    if track is not None and reference_zeros:
        raise ValueError("tracking needs poses: reference_zeros runs no forward")
    results, track_lines = [], []
    for c0 in range(0, len(files), max(int(batch_size), 1)):
        decoded = []   # (path, image, boxes or None)
        for frame, path in enumerate(files[c0:c0 + max(int(batch_size), 1)], c0):
            try:
                image = Image.open(path).convert("RGB")
                gt = Path(gt_dir) / f"{path.stem}.txt" if gt_dir else None
                boxes = read_gt_boxes(gt, device) if gt is not None and gt.exists() else None
                if boxes is not None and (boxes.dim() != 2 or boxes.size(0) == 0):
                    boxes = None   # an empty label file: no caller boxes
            except Exception as e:
                logging.error(f"Error processing {path.name}: {e}")
                continue
            decoded.append((path, image, boxes, frame))
        if not decoded:
            continue
        x = transform.batch([d[1] for d in decoded]).to(device)
        given = [i for i, d in enumerate(decoded) if d[2] is not None]
        other = [i for i, d in enumerate(decoded) if d[2] is None]
        per_image, drawn, groups = {}, {}, []

        def draw(indices, out):   # one draw call per forward, on its batched outputs, at the original resolutions
            if track is not None:
                groups.append((indices, out))   # drawn after the tracker, from the smoothed poses
            elif output_dir is not None:
                drawn.update(zip(indices, draw_poses([decoded[i][1] for i in indices], out)))

        with torch.no_grad():
            if given:
                persons = [decoded[i][2].size(0) for i in given]
                bt = torch.zeros(len(given), max(persons), 4, device=device)
                for j, i in enumerate(given):
                    bt[j, :persons[j]] = decoded[i][2]
                out = model({"image": x[given] if other else x, "bboxes": bt})
                out = _suppress(out, [decoded[i][1] for i in given], pose_nms)
                draw(given, out)
                for j, i in enumerate(given):
                    per_image[i] = ("given boxes", _slice_outputs(out, j, persons[j]))
            if other:
                xo = x[other] if given else x
                if reference_zeros:
                    out, mode = model({"image": xo, "bboxes": None}), "reference zeros (bboxes=None)"
                else:
                    out, mode = model({"image": xo}), "person detector"
                out = _suppress(out, [decoded[i][1] for i in other], pose_nms)
                draw(other, out)
                for j, i in enumerate(other):
                    per_image[i] = (mode, _slice_outputs(out, j))
            if track is not None:
                tracked = track.track(_frames_in_order(groups, len(decoded), device), [d[1].size for d in decoded])
                if output_dir is not None:
                    drawn.update(enumerate(draw_poses([d[1] for d in decoded], tracked)))
                for i, (mode, outputs) in per_image.items():
                    p = outputs["keypoints"].shape[1]
                    for k in ("track_ids", "track_hits", "track_scores", "keypoints", "keypoints_raw"):
                        if k in tracked:
                            outputs[k] = tracked[k][i:i + 1, :p]
        for i, (path, _, _, frame) in enumerate(decoded):
            mode, outputs = per_image[i]
            logging.info(f"{path.name}: boxes from {mode}")
            if mode == "person detector":
                kept = int((outputs["box_scores"][0] > 0).sum())
                logging.info(f"detector kept {kept} person(s); person 0 box (cx, cy, w, h) = "
                             f"{[round(float(v), 4) for v in outputs['boxes'][0][0]]}")
            _print_keypoints(outputs)
            if output_dir is not None:
                output_path = output_path_for(output_dir, path)
                save_prediction(drawn[i], outputs, output_path)
                logging.info(f"Saved visualization to {output_path}")
            if track is not None and output_dir is not None:
                track_lines.append(format_track_lines(frame, outputs))
            results.append((path, outputs))
    if track is not None and output_dir is not None:
        (Path(output_dir) / "tracks.txt").write_text("".join(track_lines))
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(description="Predict keypoints in images")
    ap.add_argument("--config", required=True)
    ap.add_argument("--model", required=True, help="checkpoint path, or 'synthetic'")
    ap.add_argument("--input", required=True)
    ap.add_argument("--gt")
    ap.add_argument("--output", required=True)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--precision", default="split", choices=["split", "fp32", "mixed"],
                    help="split (default): fp32-accurate f16x3 MFMA; fp32: fp32 MFMA; mixed: bf16 heatmap convs")
    ap.add_argument("--reference-zeros", action="store_true",
                    help="without --gt, call the model with bboxes=None like the reference (all-zero keypoints) "
                         "instead of running the person detector")
    ap.add_argument("--size", default=None, help="HxW input size (default: input_size square)")
    add_pose_nms_arguments(ap)
    add_flip_test_argument(ap)
    add_track_arguments(ap)
    args = ap.parse_args(argv)
    if track_options(args) is not None and Path(args.input).is_file():
        ap.error("--track needs a directory --input: the sorted files are the frames of the sequence")
    if track_options(args) is not None and args.reference_zeros:
        ap.error("--track needs poses: --reference-zeros runs no forward")
    setup_logging()
    cfg = load_config(args.config)
    device = torch.device(args.device)
    bcfg = cfg["model"]["backbone"]
    size = tuple(int(v) for v in args.size.split("x")) if args.size else (bcfg["input_size"], bcfg["input_size"])
    transform = make_transform(bcfg.get("in_channels", 3), size, device)
    logging.info(f"Loading model from {args.model}")
    model = load_model(args.model, cfg, device, args.precision)
    if flip_test_enabled(args):
        model.flip_test = True
        logging.info("flip-test on: every forward also runs the mirrored image and decodes the merged heatmaps")
    inp = Path(args.input)
    gt = Path(args.gt) if args.gt else None
    Path(args.output).mkdir(parents=True, exist_ok=True)
    logging.info(f"precision {args.precision}")
    results = []
    if inp.is_file():
        output_path = output_path_for(args.output, inp)
        results.append((inp, predict_single_image(model, inp, transform, device, gt if gt and gt.is_file() else None,
                                                  output_path=output_path, reference_zeros=args.reference_zeros,
                                                  return_outputs=True, pose_nms=pose_nms_options(args))[1]))
        logging.info(f"Saved visualization to {output_path}")
    else:
        tracker = None
        if track_options(args) is not None:
            tracker = PoseTracker(cfg["model"]["keypoint_head"]["num_keypoints"], device=device, **track_options(args))
            logging.info("tracking on: the sorted files are consecutive frames of one sequence")
        results = predict_directory_nms(model, inp, transform, device, args.output, gt_dir=gt,
                                        reference_zeros=args.reference_zeros, pose_nms=pose_nms_options(args),
                                        track=tracker)
    logging.info("Prediction completed successfully!")
    return {"model": model, "results": results}


if __name__ == "__main__":
    main()
