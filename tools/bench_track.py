#!/usr/bin/env python3
"""Cost of OKS pose tracking behind the forward: one `PoseTracker.update` on
the device (kpd_track_poses, one launch for all frames and sequences of the
call) against the numpy restatement `tests/track_ref.py` on the host,
including the device-to-host copies of the kernel's inputs that a host tracker
needs, in one process.

Workloads: one sequence of 64 seeded frames with 5 pose slots (17 keypoints;
six persons wander over the slots, each absent from a frame with probability
0.1, so the sequence holds matches, births and re-identifications after
gaps), and 8 such sequences in one call.  The device path is timed with a host clock around
`update` and a synchronise, from a zeroed state (the reset is outside the
clock), on resident tensors (a forward's outputs are already there); the host
path is timed over the copies and `track_ref.track_sequences`.  After warm-ups
the two alternate `--rounds` times; medians are reported.  One JSON line: both
times for each workload, their ratios, microseconds per frame, whether the ids
agree, and the C2 forward time recorded in BENCH_r06.json for scale.  No
pass/fail threshold: the kernel is latency-bound by construction (a sequential
dependency over frames on one CU per sequence); what it buys is the host round
trip it removes.

The measurement runs in a child process under its own `timeout`:

    python tools/bench_track.py [--frames 64] [--rounds 5] [--timeout 600]
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


def workload(sequences, frames, slots, seed):
    """[S, B, D, ...] arrays of `sequences` seeded sequences (tests/track_cases.build)."""
    import numpy as np
    import track_cases
    seqs = []
    for s in range(sequences):
        rng = np.random.default_rng(seed + s)
        layout = []
        for _ in range(frames):
            shown = [p if rng.uniform() >= 0.1 else -1 for p in rng.permutation(6)[:slots]]
            layout.append(shown)
        seqs.append(track_cases.build(seed=seed + 100 + s, layout=layout))
    return {k: np.stack([q[k] for q in seqs]) for k in seqs[0]}


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import torch
    import track_ref
    from dll.utils import PoseTracker
    dev = torch.device("cuda", 0)

    def measure(sequences, seed):
        arrays = workload(sequences, a.frames, a.slots, seed)
        t = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
        tracker = PoseTracker(17, sequences, device=dev)

        def device():
            tracker.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tracker.update(**t)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res

        def host():
            t0 = time.perf_counter()
            on_host = {k: v.cpu().numpy() for k, v in t.items()}
            res = track_ref.track_sequences(**on_host)
            return (time.perf_counter() - t0) * 1e3, res

        for _ in range(2):
            device()
            host()
        ms_d, ms_h = [], []
        for _ in range(a.rounds):
            ms_d.append(device()[0])
            ms_h.append(host()[0])
        got, want = device()[1], host()[1]
        same = bool(np.array_equal(got["track_id"].cpu().numpy(), want["track_id"]))
        return statistics.median(ms_d), statistics.median(ms_h), ms_d, ms_h, same, want["events"]

    d, h, ms_d, ms_h, same, events = measure(1, a.seed)
    d8, h8, ms_d8, _, same8, _ = measure(8, a.seed + 1000)
    print(json.dumps({"metric": "track_ms_per_call", "frames": a.frames, "slots": a.slots, "keypoints": 17,
                      "rounds": a.rounds, "device_update_ms": round(d, 3), "host_numpy_ms": round(h, 3),
                      "host_over_device": round(h / d, 1), "device_ms_min_max": [round(min(ms_d), 3), round(max(ms_d), 3)],
                      "host_ms_min_max": [round(min(ms_h), 3), round(max(ms_h), 3)],
                      "device_us_per_frame": round(d / a.frames * 1e3, 2), "ids_equal": same, "events": events,
                      "s8_device_update_ms": round(d8, 3), "s8_host_numpy_ms": round(h8, 3),
                      "s8_host_over_device": round(h8 / d8, 1),
                      "s8_device_ms_min_max": [round(min(ms_d8), 3), round(max(ms_d8), 3)],
                      "s8_device_us_per_frame": round(d8 / (8 * a.frames) * 1e3, 2), "s8_ids_equal": same8,
                      "c2_forward_ms_recorded": round(64 / C2_FORWARD_IMAGES_PER_S * 1e3, 3)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--slots", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=600, help="seconds the measuring child may take")
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
