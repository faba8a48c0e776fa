#!/usr/bin/env python3
"""Rate of the preprocessing stage in front of the forward, and the overhead
of calling it per image: n single `preprocess` calls (kpd_preprocess, the
batched pipeline at n = 1: one allocation and one set of launches per image)
against one `preprocess_batch` (kpd_preprocess_batch) over the same images, in
one process.  Both run the same kernels, so the ratio is what batching saves
in launches, allocations and serialised Canny floods.

Workload: 64 seeded uint8 images of 480 x 640 x 3 (blobs, bars and steps over
mild noise -- photo-like edge density, not white noise), the grayscale
pipeline of scripts/predict.py (gray -> CLAHE 2.0 / 8x8 -> edge blend) to
256 x 192.  After warm-ups of both paths and a bit-equality check of their
outputs (a check of the n = 1 wrapper), the two are timed alternately (HIP events around the whole set of
calls, `--rounds` times each; the median is reported).  One JSON line:
images/s of both paths, their ratio, and the C2 forward rate recorded in
BENCH_r06.json for scale.

The measurement runs in a child process under its own `timeout`, so a hang
ends the step instead of the caller's session:

    python tools/bench_preprocess.py [--n 64] [--rounds 7] [--timeout 300]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
C2_FORWARD_IMAGES_PER_S = 39800.0   # BENCH_r06.json, C2 (64 x 256x192, split precision)


def images(n, h, w, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        a = np.full((h, w, 3), 0.0) + rng.uniform(30, 90, 3)
        a += (xx[..., None] * rng.uniform(-0.08, 0.08) + yy[..., None] * rng.uniform(-0.08, 0.08))
        for _ in range(6):      # soft blobs
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(30, 140)
            a += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))[..., None] * rng.uniform(-60, 90, 3)
        for _ in range(5):      # hard-edged boxes
            y0, x0 = int(rng.uniform(0, h - 40)), int(rng.uniform(0, w - 40))
            a[y0:y0 + int(rng.uniform(20, 200)), x0:x0 + int(rng.uniform(20, 260))] += rng.uniform(-70, 70, 3)
        a += rng.normal(0, 3.0, (h, w, 3))
        out.append(a.clip(0, 255).astype(np.uint8))
    return out


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    import torch
    from dll.data.transforms import FLAG_CLAHE, FLAG_EDGES, FLAG_GRAY, preprocess, preprocess_batch
    dev = torch.device("cuda", 0)
    imgs = [torch.from_numpy(x).to(dev) for x in images(a.n, a.height, a.width, a.seed)]
    size, flags = (a.out_h, a.out_w), FLAG_GRAY | FLAG_CLAHE | FLAG_EDGES
    out_s = torch.empty(a.n, 1, *size, device=dev)
    out_b = torch.empty(a.n, 1, *size, device=dev)

    def single():
        for i, t in enumerate(imgs):
            preprocess(t, size, (0.5,), (0.5,), flags, 2.0, (8, 8), out=out_s[i])

    def batch():
        preprocess_batch(imgs, size, (0.5,), (0.5,), flags, 2.0, (8, 8), out=out_b)

    for _ in range(2):
        single()
        batch()
    torch.cuda.synchronize()
    identical = bool(torch.equal(out_s, out_b))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms_s, ms_b = [], []
    for _ in range(a.rounds):
        ms_s.append(timed(single))
        ms_b.append(timed(batch))
    s, b = statistics.median(ms_s), statistics.median(ms_b)
    print(json.dumps({"metric": "preprocess_images_per_s", "n": a.n, "image": [a.height, a.width, 3],
                      "out": list(size), "pipeline": "gray+clahe+edges", "rounds": a.rounds,
                      "single_images_per_s": round(a.n / s * 1e3, 1), "batch_images_per_s": round(a.n / b * 1e3, 1),
                      "batch_over_single": round(s / b, 2), "single_ms": round(s, 3), "batch_ms": round(b, 3),
                      "single_ms_min_max": [round(min(ms_s), 3), round(max(ms_s), 3)],
                      "batch_ms_min_max": [round(min(ms_b), 3), round(max(ms_b), 3)],
                      "outputs_identical": identical,
                      "c2_forward_images_per_s_recorded": C2_FORWARD_IMAGES_PER_S}))
    return 0 if identical else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out-h", type=int, default=256)
    ap.add_argument("--out-w", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
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
