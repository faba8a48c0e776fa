#!/usr/bin/env python3
"""Golden vectors for the stand-alone operators at their shape and value
edges, produced by the REFERENCE's own code in this container (imported as
make_data_golden.py imports it):

* `generate_target_heatmap` / `generate_target_heatmap_adaptive`
  (dll/models/heatmap_head.py:163-252) on ops_edges_cases.target_cases();
* `decode_heatmaps`, `decode_heatmaps_subpixel`, `decode_heatmaps_soft_argmax`
  (:265-413) on ops_edges_cases.decode_jobs();
* `Trainer._calculate_validation_metrics` (dll/training/trainer.py:384-429) on
  ops_edges_cases.metric_cases().

Only outputs are stored; the inputs are regenerated from seeds.

    python -B tests/golden/make_ops_edges_golden.py   -> tests/golden/ops_edges.npz
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import numpy as np  # noqa: E402

from make_data_golden import import_reference  # noqa: E402
from ops_edges_cases import ARGMAX, MODEL, SOFTARGMAX, SUBPIXEL, decode_jobs, metric_cases, target_cases  # noqa: E402

OUT = ROOT / "tests" / "golden" / "ops_edges.npz"


def main():
    gen, Trainer, _ = import_reference()
    import dll.models.heatmap_head as hh
    data = {}
    for name, kp, size, sigma, adaptive in target_cases():
        fn = hh.generate_target_heatmap_adaptive if adaptive else gen
        data[f"hm_{name}"] = fn(kp.clone(), size, sigma).numpy()
    for key, heat, mode, param in decode_jobs():
        if mode == MODEL:
            continue
        if mode == ARGMAX:
            k, s = hh.decode_heatmaps(heat.clone())
        elif mode == SUBPIXEL:
            k, s = hh.decode_heatmaps_subpixel(heat.clone(), window_size=int(param))
        else:
            assert mode == SOFTARGMAX
            k, s = hh.decode_heatmaps_soft_argmax(heat.clone(), temperature=param)
        data[f"dec_{key}_kpts"], data[f"dec_{key}_scores"] = k.numpy(), s.numpy()
    for name, pred, gt, vis, thresholds in metric_cases():
        stub = types.SimpleNamespace(config=types.SimpleNamespace(pck_thresholds=thresholds))
        stub._get_default_metrics = types.MethodType(Trainer._get_default_metrics, stub)
        m = Trainer._calculate_validation_metrics(stub, {"keypoints": pred}, {"keypoints": gt, "visibilities": vis})
        data[f"met_{name}"] = np.array([m["avg_ADE"]] + [m[f"pck_{t}"] for t in thresholds], np.float64)
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, len(data), "arrays", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
