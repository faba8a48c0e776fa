#!/usr/bin/env python3
"""Cost of the training augmentation in front of the transform: one
`augment_batch` call (kpd_augment_batch: every image warped and its labels
moved in one launch per 16 images) against two yardsticks in one process --

  (a) the equivalent chain of torch operators: uint8 -> float,
      `F.affine_grid` + `F.grid_sample` (bilinear, zero padding) per size
      group, gain / offset, round and clamp back to uint8, and the label rule
      (joint swap, map, frame test, box hull and clip) as float64 tensor maths;
  (b) a device-to-device `copy_` of the source's byte count, which reads and
      writes what the augmentation must at least read and write: the
      bandwidth yardstick.

Workload: 64 seeded 480x640x3 images with 2 persons each (17 keypoints), every
image mirrored, rotated and scaled.  Each variant is timed with HIP events
around `--inner` back-to-back calls on resident tensors; after warm-ups the
three alternate `--rounds` times and the medians are reported.  The chain's
results are checked against the fused call's once: the images agree to a few
grey levels (the chain samples in fp32, the kernel on a 1/32-pixel grid), the
labels to 1e-6.

One JSON line: the three times, the host's share of the fused call (wall time
of the enqueue alone), the two ratios, the achieved bytes/s of the fused call (source plus destination bytes, from the shapes) and the C2 forward
time recorded in BENCH_r06.json for scale.  The tool sets no pass/fail
threshold.

The measurement runs in a child process under its own `timeout`:

    python tools/bench_augment.py [--n 64] [--rounds 9] [--inner 10] [--timeout 300]
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


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    import numpy as np
    import torch
    import torch.nn.functional as F
    from dll.data import AugmentParams, augment_batch
    from dll.utils import flip_index
    dev = torch.device("cuda", 0)
    n, H, W, C, P, K = a.n, 480, 640, 3, 2, 17
    g = torch.Generator(device="cpu").manual_seed(a.seed)
    src = torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8).to(dev)
    images = list(src.unbind(0))
    kp = (torch.rand(n, P, K, 2, generator=g) * 0.6 + 0.2).to(dev)
    vis = torch.randint(1, 3, (n, P, K), generator=g).float().to(dev)
    boxes = torch.cat([torch.rand(n, P, 2, generator=g) * 0.2 + 0.4, torch.rand(n, P, 2, generator=g) * 0.3 + 0.2],
                      -1).to(dev)
    u = torch.rand(n, 4, generator=g, dtype=torch.float64).numpy()
    par = AugmentParams(np.ones(n, bool), (2 * u[:, 0] - 1) * 30.0, 0.8 + 0.4 * u[:, 1],
                        np.rint(256 * (1 + (2 * u[:, 2] - 1) * 0.2)), np.rint(256 * 255 * (2 * u[:, 3] - 1) * 0.2))
    pairs = flip_index(K)

    # the chain's constants, resident like the fused call's inputs are
    _, N = par.matrices(W, H)
    N64 = torch.tensor(N.reshape(n, 2, 3), device=dev)
    inv = np.linalg.inv(np.concatenate([N.reshape(n, 2, 3), np.tile([[[0.0, 0.0, 1.0]]], (n, 1, 1))], 1))[:, :2]
    L, t = inv[:, :, :2], inv[:, :, 2]
    theta = torch.tensor(np.concatenate([L, (L.sum(2) + 2 * t - 1)[:, :, None]], 2), dtype=torch.float32, device=dev)
    gain = torch.tensor(par.gain / 256.0, dtype=torch.float32, device=dev).view(n, 1, 1, 1)
    offset = torch.tensor(par.offset / 256.0, dtype=torch.float32, device=dev).view(n, 1, 1, 1)
    idx = torch.tensor(pairs, device=dev)

    def fused():
        return augment_batch(images, kp, vis, boxes, params=par, pairs=pairs)

    def chain():
        x = src.permute(0, 3, 1, 2).float()
        grid = F.affine_grid(theta, (n, C, H, W), align_corners=False)
        y = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        out = (y * gain + offset).round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        k64, v = kp.index_select(2, idx).double(), vis.index_select(2, idx)      # every image is mirrored
        m = torch.einsum("nij,npkj->npki", N64[:, :, :2], k64) + N64[:, None, None, :, 2]
        m32 = m.float()
        keep = (v == 0) | ((k64[..., 0] == 0) & (k64[..., 1] == 0))
        inside = ((m32 >= 0) & (m32 < 1)).all(-1)
        kp2 = torch.where(keep[..., None], k64.float(), m32 * inside[..., None])
        vis2 = torch.where(keep, v, v * inside)
        b = boxes.double()
        half = 0.5 * b[..., 2:]
        lo, hi = b[..., :2] - half, b[..., :2] + half
        cx = torch.stack([lo[..., 0], hi[..., 0], lo[..., 0], hi[..., 0]], -1)
        cy = torch.stack([lo[..., 1], lo[..., 1], hi[..., 1], hi[..., 1]], -1)
        px = N64[:, None, None, 0, 0] * cx + N64[:, None, None, 0, 1] * cy + N64[:, None, None, 0, 2]
        py = N64[:, None, None, 1, 0] * cx + N64[:, None, None, 1, 1] * cy + N64[:, None, None, 1, 2]
        x0, x1 = px.amin(-1).clamp(0, 1), px.amax(-1).clamp(0, 1)
        y0, y1 = py.amin(-1).clamp(0, 1), py.amax(-1).clamp(0, 1)
        live = ((x1 - x0 > 0) & (y1 - y0 > 0) & (b != 0).any(-1))[..., None]
        box2 = (torch.stack([0.5 * (x0 + x1), 0.5 * (y0 + y1), x1 - x0, y1 - y0], -1) * live).float()
        return out, kp2, vis2, box2

    nbytes = src.numel()
    ca, cb = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def copy():
        return cb.copy_(ca)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            res = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner, res

    f, c = fused(), chain()
    torch.cuda.synchronize()
    d = (torch.stack(f[0]).int() - c[0].int()).abs()
    img_max, img_mean = int(d.max()), float(d.float().mean())
    lab_diff = max(float((f[1] - c[1]).abs().max()), float((f[3] - c[3]).abs().max()))
    assert img_mean <= 2.0, img_mean     # noise images: neighbouring taps differ by ~85 levels, the grid is 1/32 px
    assert lab_diff <= 1e-6 and torch.equal(f[2], c[2]), lab_diff

    variants = {"fused": fused, "chain": chain, "copy": copy}
    for _ in range(3):
        for fn in variants.values():
            timed(fn)
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn)[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    # the host's share of the fused call: matrices, argument tables and the enqueue, no device wait inside
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.inner):
        fused()
    host_ms = (time.perf_counter() - t0) * 1e3 / a.inner
    torch.cuda.synchronize()
    res = {"metric": "augment_ms_per_batch", "n": n, "image": [H, W, C], "persons": P, "keypoints": K,
           "rounds": a.rounds, "inner": a.inner,
           "fused_ms": round(med["fused"], 4), "chain_ms": round(med["chain"], 4), "copy_ms": round(med["copy"], 4),
           "fused_host_enqueue_ms": round(host_ms, 4),
           "fused_over_chain": round(med["fused"] / med["chain"], 3),
           "fused_over_copy": round(med["fused"] / med["copy"], 3),
           "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
           "chain_ms_min_max": [round(min(ms["chain"]), 4), round(max(ms["chain"]), 4)],
           "copy_ms_min_max": [round(min(ms["copy"]), 4), round(max(ms["copy"]), 4)],
           "fused_gbytes_per_s": round(2 * nbytes / (med["fused"] * 1e-3) / 1e9, 1),
           "copy_gbytes_per_s": round(2 * nbytes / (med["copy"] * 1e-3) / 1e9, 1),
           "image_max_abs_diff": img_max, "image_mean_abs_diff": round(img_mean, 4), "labels_max_abs_diff": lab_diff,
           "c2_forward_ms_recorded": round(n / C2_FORWARD_IMAGES_PER_S * 1e3, 3)}
    if a.profile:   # where the host's share goes
        import cProfile
        import pstats
        pr = cProfile.Profile()
        pr.enable()
        for _ in range(50):
            fused()
        pr.disable()
        torch.cuda.synchronize()
        pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(14)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed interval")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring child may take")
    ap.add_argument("--profile", action="store_true", help="also print a cProfile of 50 fused calls to stderr")
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
