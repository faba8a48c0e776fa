#!/usr/bin/env python3
"""Cost of the pose overlay behind the forward: `draw_poses` on the device
(kpd_draw_poses, one call for the whole batch) against PIL `ImageDraw`
drawing the same boxes, lines and ellipses on the host, in one process.

Workload: 64 seeded uint8 images of 480 x 640 x 3, 2 persons each (seeded
boxes, 17 keypoints inside them, 17 x 56 x 56 heatmaps), all four layers
(heat underlay, boxes, limbs, joints).  The device path is timed with a host
clock around the call and a synchronise, drawing in place into resident
images (the forward's outputs are already there); the host path draws boxes,
limbs and joints into PIL images (the heat underlay has no ImageDraw
counterpart and is left out there, which favours the host).  After warm-ups
the two alternate `--rounds` times; medians are reported.  One JSON line:
both times per 64 images, their ratio, and the C2 forward time recorded in
BENCH_r06.json for scale.  No pass/fail threshold.

The measurement runs in a child process under its own `timeout`:

    python tools/bench_draw.py [--n 64] [--rounds 9] [--timeout 300]
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


def workload(n, h, w, persons, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    c = rng.uniform(0.3, 0.7, (n, persons, 2))
    wh = rng.uniform(0.25, 0.55, (n, persons, 2))
    boxes = np.concatenate([c, wh], -1).astype(np.float32)
    kp = (c[:, :, None] + (rng.uniform(-0.5, 0.5, (n, persons, 17, 2)) * wh[:, :, None])).astype(np.float32)
    vis = np.eye(3, dtype=np.float32)[rng.integers(1, 3, (n, persons, 17))]
    heat = rng.uniform(0, 1, (n, persons, 17, 56, 56)).astype(np.float32) ** 4
    return imgs, kp, vis, boxes, heat


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    import torch
    from PIL import Image, ImageDraw
    from dll.utils import DrawStyle, draw_poses
    dev = torch.device("cuda", 0)
    imgs, kp, vis, boxes, heat = workload(a.n, a.height, a.width, a.persons, a.seed)
    st = DrawStyle()
    out = {"keypoints": torch.from_numpy(kp[:, :, None]).to(dev), "visibilities": torch.from_numpy(vis[:, :, None]).to(dev),
           "heatmap": torch.from_numpy(heat).to(dev), "boxes": [torch.from_numpy(b).to(dev) for b in boxes]}
    dimgs = [torch.from_numpy(i).to(dev) for i in imgs]
    pil = [Image.fromarray(i) for i in imgs]
    layers = ("heat", "boxes", "limbs", "joints")

    def device():
        t0 = time.perf_counter()
        draw_poses(dimgs, out, style=st, layers=layers, inplace=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    r, lw, bw = st.joint_radius / 16, max(round(st.limb_half_width / 8), 1), max(round(st.box_half_width / 8), 1)
    cls = vis.argmax(-1)
    lcol = st.resolved_limb_colors()

    def host():
        t0 = time.perf_counter()
        for i, im in enumerate(pil):
            d = ImageDraw.Draw(im)
            for p in range(a.persons):
                cx, cy, bw_, bh_ = boxes[i, p]
                d.rectangle([(cx - bw_ / 2) * a.width, (cy - bh_ / 2) * a.height, (cx + bw_ / 2) * a.width,
                             (cy + bh_ / 2) * a.height], outline=st.box_color, width=bw)
                xy = kp[i, p] * (a.width, a.height)
                for (ja, jb), col in zip(st.limbs, lcol):
                    d.line([tuple(xy[ja]), tuple(xy[jb])], fill=col, width=lw)
                for k in range(17):
                    x, y = xy[k]
                    d.ellipse([x - r, y - r, x + r, y + r], fill=st.joint_colors[cls[i, p, k]])
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):
        device()
        host()
    ms_d, ms_h = [], []
    for _ in range(a.rounds):
        ms_d.append(device())
        ms_h.append(host())
    d, h = statistics.median(ms_d), statistics.median(ms_h)
    print(json.dumps({"metric": "draw_ms_per_batch", "n": a.n, "image": [a.height, a.width, 3], "persons": a.persons,
                      "layers_device": list(layers), "layers_host": ["boxes", "limbs", "joints"], "rounds": a.rounds,
                      "device_ms": round(d, 3), "host_pil_ms": round(h, 3), "host_over_device": round(h / d, 1),
                      "device_ms_min_max": [round(min(ms_d), 3), round(max(ms_d), 3)],
                      "host_ms_min_max": [round(min(ms_h), 3), round(max(ms_h), 3)],
                      "device_us_per_image": round(d / a.n * 1e3, 2), "host_us_per_image": round(h / a.n * 1e3, 1),
                      "c2_forward_ms_recorded": round(a.n / C2_FORWARD_IMAGES_PER_S * 1e3, 3)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--persons", type=int, default=2)
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
