#!/usr/bin/env python3
"""Cost of COCO keypoint matching behind the forward: `OksEvaluator.update`
on the device (kpd_oks_match, one launch for the whole batch) against the
numpy restatement `tests/oks_ref.py` evaluating the same batch on the host,
in one process.

Workload: 64 seeded images with 5 predicted poses and 5 labelled persons
each (17 keypoints, seeded boxes, prediction = label + noise of 0.02 .. 0.2
sqrt(area), scores from 8 x 8 heatmaps), the ten COCO thresholds.  The device
path is timed with a host clock around `update` and a synchronise, on
resident tensors (the forward's outputs and the collated batch are already
there); the host path gets host copies of the kernel's inputs, made outside
the clock.  After warm-ups the two alternate `--rounds` times; medians are
reported.  One JSON line: both times per 64 images, their ratio, and the C2
forward time recorded in BENCH_r06.json for scale.  No pass/fail threshold.

The measurement runs in a child process under its own `timeout`:

    python tools/bench_oks.py [--n 64] [--rounds 9] [--timeout 300]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
C2_FORWARD_IMAGES_PER_S = 39800.0   # BENCH_r06.json, C2 (64 x 256x192, split precision)


def workload(n, persons, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    K = 17
    sizes = [(int(w), int(h)) for w, h in rng.integers(320, 1281, (n, 2))]
    c = rng.uniform(0.3, 0.7, (n, persons, 2))
    wh = rng.uniform(0.2, 0.5, (n, persons, 2))
    boxes = np.concatenate([c, wh], -1).astype(np.float32)
    gt = (c[:, :, None] + rng.uniform(-0.5, 0.5, (n, persons, K, 2)) * wh[:, :, None]).astype(np.float32)
    vis = rng.integers(0, 3, (n, persons, K)).astype(np.float32)
    vis[..., 0] = 2
    level = rng.choice([0.02, 0.05, 0.1, 0.2], (n, persons, K))
    side = np.sqrt(wh[..., 0] * wh[..., 1])[..., None, None]     # sqrt(area) in normalised units
    ang = rng.uniform(0, 2 * np.pi, (n, persons, K))
    pred = gt + level[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1) * side
    pred = pred[:, rng.permutation(persons)].astype(np.float32)  # detector order, not label order
    heat = rng.uniform(0, 1, (n, persons, K, 8, 8)).astype(np.float32)
    det_boxes = rng.uniform(0.2, 0.6, (n, persons, 4)).astype(np.float32)
    box_scores = rng.uniform(0.3, 1.0, (n, persons)).astype(np.float32)
    return sizes, boxes, gt, vis, pred, heat, det_boxes, box_scores


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch
    import oks_ref
    from dll.utils import OksEvaluator
    dev = torch.device("cuda", 0)
    sizes, boxes, gt, vis, pred, heat, det_boxes, box_scores = workload(a.n, a.persons, a.seed)
    t = lambda x: torch.from_numpy(x).to(dev)     # noqa: E731
    out = {"keypoints": t(pred[:, :, None]), "heatmap": t(heat), "boxes": [t(b) for b in det_boxes],
           "box_scores": t(box_scores)}
    batch = {"keypoints": t(gt), "visibilities": t(vis), "bboxes": [t(boxes)],
             "num_persons": torch.full((a.n,), a.persons, device=dev), "orig_size": sizes}
    ev = OksEvaluator()
    host_in = {k: v.cpu().numpy() for k, v in ev.inputs(out, batch).items()}

    def device():
        ev.reset()
        t0 = time.perf_counter()
        ev.update(out, batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host():
        t0 = time.perf_counter()
        res = oks_ref.evaluate_batch(**host_in)
        return (time.perf_counter() - t0) * 1e3, res

    for _ in range(3):
        device()
        host()
    ms_d, ms_h = [], []
    for _ in range(a.rounds):
        ms_d.append(device())
        ms_h.append(host()[0])
    t0 = time.perf_counter()
    ap = ev.summarize()
    ms_sum = (time.perf_counter() - t0) * 1e3
    want = oks_ref.average_precision([host()[1]])
    d, h = statistics.median(ms_d), statistics.median(ms_h)
    print(json.dumps({"metric": "oks_match_ms_per_batch", "n": a.n, "dets": a.persons, "gts": a.persons, "keypoints": 17,
                      "thresholds": 10, "rounds": a.rounds, "device_update_ms": round(d, 3),
                      "host_numpy_ms": round(h, 3), "host_over_device": round(h / d, 1),
                      "device_ms_min_max": [round(min(ms_d), 3), round(max(ms_d), 3)],
                      "host_ms_min_max": [round(min(ms_h), 3), round(max(ms_h), 3)],
                      "device_us_per_image": round(d / a.n * 1e3, 2), "summarize_ms": round(ms_sum, 3),
                      "oks_AP": round(ap["oks_AP"], 6), "oks_AP_host": round(want["oks_AP"], 6),
                      "c2_forward_ms_recorded": round(a.n / C2_FORWARD_IMAGES_PER_S * 1e3, 3)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--persons", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # the GPU step: a fresh child under its own time limit
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()), "--worker"]
    cmd += [v for v in sys.argv[1:] if v != "--worker"]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
