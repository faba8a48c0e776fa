#!/usr/bin/env python3
"""Cost of the flip-test merge behind the two forwards: one `flip_merge` call
(kpd_flip_merge: both heatmaps read once, the merged map written once, decoded
in the same launch) against the equivalent chain of torch operators -- flip,
index_select, add, mul, kpd_decode_heatmaps(KPD_DECODE_MODEL), the box
transform, amax for the peaks and the padding fix-up -- in one process.

Workloads: seeded signed heatmaps of 64 images x 1 person and 64 x 5 persons
(17 keypoints, 56 x 56), every box live.  Each variant is timed with HIP events
around `--inner` back-to-back calls on resident tensors; after warm-ups the two
alternate `--rounds` times and the medians are reported.  The chain's results
are checked against the fused call's once (merged map bit-equal, keypoints
within 1e-5).

The second part is the end-to-end cost on the synthetic model at 64 x 256x192
and at 1 x 256x192 with 1 box, split precision: the plain forward,
`flip_test=True` (one forward over the concatenated straight and mirrored
batch, then the merge) and the alternative of two separate forwards plus the
merge, alternating in the same way; the two flip-test forms are checked to
give bit-identical outputs.

One JSON line: the times, their ratios, the achieved bytes/s of the fused call
and the C2 forward time recorded in BENCH_r06.json for scale.  The acceptance
gate of the kernel is `fused_over_chain <= 1` in this same run; the tool itself
sets no pass/fail threshold.

The measurement runs in a child process under its own `timeout`:

    python tools/bench_flip_merge.py [--n 64] [--rounds 9] [--inner 10] [--timeout 300]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
C2_FORWARD_IMAGES_PER_S = 39800.0   # BENCH_r06.json, C2 (64 x 256x192, split precision)


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    import torch
    from dll import _native
    from dll.utils import flip_index, flip_merge, mirror_boxes, mirror_images
    dev = torch.device("cuda", 0)
    K, H, W = 17, 56, 56
    idx = torch.tensor(flip_index(K), device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            res = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner, res

    def alternate(variants):
        for _ in range(3):
            for fn in variants.values():
                timed(fn)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn)[0])
        return {k: statistics.median(v) for k, v in ms.items()}, ms

    def merge_workload(n, P, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        level = torch.rand(n, P, K, 1, 1, generator=g) * 8 - 6
        ha = (level + 0.5 * torch.randn(n, P, K, H, W, generator=g)).to(dev)
        hb = (level[:, :, flip_index(K)] + 0.5 * torch.randn(n, P, K, H, W, generator=g)).to(dev)
        boxes = torch.cat([torch.rand(n, P, 2, generator=g) * 0.4 + 0.3, torch.rand(n, P, 2, generator=g) * 0.4 + 0.2],
                          -1).to(dev)

        def fused():
            return flip_merge(ha, hb, boxes)

        def chain():
            m = (ha + hb.index_select(2, idx).flip(-1)) * 0.5
            kp, _, vis = _native.decode_heatmaps(m.view(n * P, K, H, W), _native.DECODE_MODEL)
            wh = boxes[..., None, 2:]
            kp = (kp.view(n, P, K, 2) * wh + (boxes[..., None, :2] - wh / 2)).clamp_(0, 1)
            peaks = m.amax((-2, -1))
            live = (boxes != 0).any(-1)                      # every box is live here: slot order = caller order
            lk = live[..., None, None].to(kp.dtype)
            vis = vis.view(n, P, K, 3) * lk
            vis[:, 0, :, 0] += (~live.any(1))[:, None].to(vis.dtype)   # the dummy person
            return {"heatmap": m * lk[..., None], "keypoints": (kp * lk)[:, :, None], "visibilities": vis[:, :, None],
                    "keypoint_peaks": peaks * lk[..., 0]}

        f, c = fused(), chain()
        torch.cuda.synchronize()
        assert torch.equal(f["heatmap"], c["heatmap"]) and torch.equal(f["keypoint_peaks"], c["keypoint_peaks"])
        assert torch.equal(f["visibilities"], c["visibilities"])
        diff = float((f["keypoints"] - c["keypoints"]).abs().max())
        assert diff <= 1e-5, diff
        med, ms = alternate({"fused": fused, "chain": chain})
        nbytes = 3 * ha.numel() * 4 + boxes.numel() * 4 + n * P * K * 6 * 4
        return {"fused_ms": round(med["fused"], 4), "chain_ms": round(med["chain"], 4),
                "fused_over_chain": round(med["fused"] / med["chain"], 3),
                "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
                "chain_ms_min_max": [round(min(ms["chain"]), 4), round(max(ms["chain"]), 4)],
                "fused_gbytes_per_s": round(nbytes / (med["fused"] * 1e-3) / 1e9, 1),
                "keypoints_max_abs_diff": diff}

    def end_to_end(n):
        from dll.configs import ModelConfig, TrainingConfig
        from dll.models import MultiPersonKeypointModel
        from dll.models.synthetic import synthetic_boxes, synthetic_images, synthetic_state_dict
        m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig())
        m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0))
        m = m.to(dev).eval()
        x, boxes = synthetic_images(n, 3, 256, 192, seed=1).to(dev), synthetic_boxes(n, 1, seed=2).to(dev)

        def plain():
            m.flip_test = False
            return m({"image": x, "bboxes": boxes})

        def flip():
            m.flip_test = True
            return m({"image": x, "bboxes": boxes})

        def two_forwards():
            m.flip_test = False
            a_, b_ = m({"image": x, "bboxes": boxes}), m({"image": mirror_images(x), "bboxes": mirror_boxes(boxes)})
            return flip_merge(a_["heatmap"], b_["heatmap"], boxes, inplace=True)

        with torch.no_grad():
            f, c = flip(), two_forwards()
            torch.cuda.synchronize()
            same = all(torch.equal(f[k], c[k]) for k in ("heatmap", "keypoints", "visibilities", "keypoint_peaks"))
            med, _ = alternate({"plain": plain, "flip": flip, "two_forwards": two_forwards})
        m.flip_test = False
        return {"n": n, "plain_forward_ms": round(med["plain"], 3), "flip_test_forward_ms": round(med["flip"], 3),
                "flip_over_plain": round(med["flip"] / med["plain"], 3),
                "two_forwards_ms": round(med["two_forwards"], 3),
                "two_forwards_over_plain": round(med["two_forwards"] / med["plain"], 3),
                "flip_test_equals_two_forwards": same}

    res = {"metric": "flip_merge_ms_per_batch", "keypoints": K, "heatmap": [H, W], "rounds": a.rounds, "inner": a.inner,
           "p1": {"n": a.n, "persons": 1, **merge_workload(a.n, 1, a.seed)},
           "p5": {"n": a.n, "persons": 5, **merge_workload(a.n, 5, a.seed + 1)},
           "end_to_end": end_to_end(a.n), "end_to_end_1": end_to_end(1),
           "c2_forward_ms_recorded": round(a.n / C2_FORWARD_IMAGES_PER_S * 1e3, 3)}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed interval")
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
