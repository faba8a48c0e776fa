#!/usr/bin/env python3
"""Cost of the train-mode pieces of the heatmap head, alternated in one process.

(a) The operator.  `dll.ops.bn_relu_dropout2d` (kpd_bn_train_forward /
    kpd_bn_train_backward: batch-statistics BatchNorm + ReLU + Dropout2d
    multiplier), forward + backward at [64][256][56][56] and [64][64][56][56],
    against two yardsticks:
      * the torch chain `F.batch_norm(training=True)` -> `relu` -> multiply by
        the same [N, C] mask, with autograd;
      * device-to-device `copy_`s of the same byte count: the fused operator
        moves 3 tensor passes forward (x twice, y) and 5 backward (x and gy
        twice, gx), i.e. four tensor-sized `copy_`s (one read + one write each).
    Reported: the three times, the two ratios, the achieved bytes/s (8 tensor
    passes over the fused time; the copies' own rate next to it) and the wall
    time of the enqueue alone, the host's share of a call.
(b) The head.  One `HeatmapHead` train step at 64 ROIs of 56 x 56 -- forward,
    `AdaptiveHeatmapLoss`, backward -- against the same head assembled from
    `nn.Conv2d` / `nn.BatchNorm2d` / `nn.Dropout2d` (the attention blocks are
    torch ops on both sides) with the same weights on the same device.

Every variant is timed with HIP events around `--inner` back-to-back calls on
resident tensors; after warm-ups the variants alternate `--rounds` times and
the medians are reported.  The chain's results are checked against the fused
operator's once.  One JSON line; the tool sets no pass/fail threshold.

`--amp` measures instead one comparison: the head step with
`train_precision` "split" against "mixed" (bf16 operands in the three 3x3
convolutions) -- two heads with the same weights on the same
inputs, alternated: medians with min-max, the ratio, and the max abs
difference of the first step's loss between the two.

The measurement runs in a child process under its own `timeout`:

    python tools/bench_head_train.py [--rois 64] [--rounds 7] [--inner 4] [--timeout 600] [--amp]
"""
import argparse
import copy
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def worker(a):
    sys.path.insert(0, str(ROOT / "keypoint-detection_amd"))
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from dll.configs.model_config import HeatmapHeadConfig
    from dll.losses import AdaptiveHeatmapLoss
    from dll.models.heatmap_head import HeatmapHead, generate_target_heatmap
    from dll.models.synthetic import synthetic_state_dict
    from dll.ops import bn_relu_dropout2d
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(a.seed)

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def alternate(variants, inner):
        for _ in range(2):
            for fn in variants.values():
                timed(fn, inner)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn, inner))
        return {k: statistics.median(v) for k, v in ms.items()}, ms

    if a.amp:
        heads = {}
        for prec in ("split", "mixed"):
            h = HeatmapHead(HeatmapHeadConfig())
            h.load_state_dict(synthetic_state_dict(h.state_dict(), seed=7))
            h.train_precision = prec
            heads[prec] = h.to(dev).train()
        R = a.rois
        xh = torch.rand(R, 64, 56, 56, generator=g).to(dev)
        gt = generate_target_heatmap((torch.rand(R, 17, 2, generator=g) * 0.8 + 0.1).to(dev), (56, 56), sigma=3.0)
        crit = AdaptiveHeatmapLoss()
        first = {}

        def step(prec):
            heads[prec].zero_grad(set_to_none=True)
            loss = crit(heads[prec](xh)[0], gt)
            loss.backward()
            return loss.detach()

        for prec in heads:   # the same dropout masks in both first steps
            torch.manual_seed(a.seed)
            first[prec] = float(step(prec))
        med, ms = alternate({p: (lambda p=p: step(p)) for p in heads}, max(1, a.inner // 2))
        spread = max(max(ms[p]) - min(ms[p]) for p in heads)
        print(json.dumps({
            "metric": "head_train_amp_ms", "rois": R, "rounds": a.rounds, "inner": max(1, a.inner // 2),
            "split_ms": round(med["split"], 3), "mixed_ms": round(med["mixed"], 3),
            "split_ms_min_max": [round(min(ms["split"]), 3), round(max(ms["split"]), 3)],
            "mixed_ms_min_max": [round(min(ms["mixed"]), 3), round(max(ms["mixed"]), 3)],
            "split_ms_all": [round(v, 3) for v in ms["split"]], "mixed_ms_all": [round(v, 3) for v in ms["mixed"]],
            "mixed_over_split": round(med["mixed"] / med["split"], 3),
            "gain_ms": round(med["split"] - med["mixed"], 3), "larger_spread_ms": round(spread, 3),
            "first_loss": {k: v for k, v in first.items()},
            "first_loss_max_abs_diff": abs(first["split"] - first["mixed"])}))
        return 0

    res = {"metric": "head_train_ms", "rois": a.rois, "rounds": a.rounds, "inner": a.inner, "operator": []}

    # ---- (a) the operator
    for C in (256, 64):
        N, H, W = a.rois, 56, 56
        x = torch.randn(N, C, H, W, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(N, C, H, W, generator=g).to(dev)
        ga = (torch.rand(C, generator=g) + 0.5).to(dev).requires_grad_(True)
        be = (torch.randn(C, generator=g) * 0.3).to(dev).requires_grad_(True)
        drop = (torch.bernoulli(torch.full((N, C), 0.9), generator=g) / 0.9).to(dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        def fused():
            y = bn_relu_dropout2d(x, ga, be, rm, rv, momentum=0.1, eps=1e-5, relu=True, drop=drop)
            return y, torch.autograd.grad(y, (x, ga, be), gy)

        def chain():
            y = F.relu(F.batch_norm(x, rm, rv, ga, be, True, 0.1, 1e-5)) * drop.view(N, C, 1, 1)
            return y, torch.autograd.grad(y, (x, ga, be), gy)

        ca, cb = torch.empty_like(gy), torch.empty_like(gy)

        def copies():
            for _ in range(4):
                cb.copy_(ca)

        yf, gf = fused()
        yc, gc = chain()
        torch.cuda.synchronize()
        diffs = [float((u - v).abs().max() / v.abs().max()) for u, v in zip((yf,) + gf, (yc,) + gc)]
        # sanity only: ReLU elements flipped between two fp32 batch norms move ggamma / gbeta
        assert max(diffs) <= 1e-2, diffs
        del yf, gf, yc, gc
        med, ms = alternate({"fused": fused, "chain": chain, "copy": copies}, a.inner)
        host = {}   # wall time of the enqueue alone (no device wait inside): the host's share of a call
        for k, fn in (("fused", fused), ("chain", chain)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            host[k] = (time.perf_counter() - t0) * 1e3 / a.inner
        torch.cuda.synchronize()
        tensor_bytes = N * C * H * W * 4
        res["operator"].append({
            "shape": [N, C, H, W], "fused_ms": round(med["fused"], 4), "chain_ms": round(med["chain"], 4),
            "copy_ms": round(med["copy"], 4), "fused_over_chain": round(med["fused"] / med["chain"], 3),
            "fused_over_copy": round(med["fused"] / med["copy"], 3),
            "fused_host_enqueue_ms": round(host["fused"], 4), "chain_host_enqueue_ms": round(host["chain"], 4),
            "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
            "chain_ms_min_max": [round(min(ms["chain"]), 4), round(max(ms["chain"]), 4)],
            "copy_ms_min_max": [round(min(ms["copy"]), 4), round(max(ms["copy"]), 4)],
            "fused_gbytes_per_s": round(8 * tensor_bytes / (med["fused"] * 1e-3) / 1e9, 1),
            "copy_gbytes_per_s": round(8 * tensor_bytes / (med["copy"] * 1e-3) / 1e9, 1),
            "max_rel_diff_to_chain": max(diffs)})
        del x, gy, ca, cb
        torch.cuda.empty_cache()

    # ---- (b) the head
    head = HeatmapHead(HeatmapHeadConfig())
    head.load_state_dict(synthetic_state_dict(head.state_dict(), seed=7))
    head = head.to(dev).train()

    class TorchHead(nn.Module):
        def __init__(self, h):
            super().__init__()
            self.fc = copy.deepcopy(h.channel_attention.fc)
            self.sconv = copy.deepcopy(h.spatial_attention.conv)
            self.deconv_layers = copy.deepcopy(h.deconv_layers)
            self.final_layer = copy.deepcopy(h.final_layer)

        def forward(self, x):
            cw = torch.sigmoid(self.fc(x.mean(dim=(2, 3))) + self.fc(x.amax(dim=(2, 3))))
            x = x * cw[:, :, None, None]
            x = x * torch.sigmoid(self.sconv(torch.cat([x.mean(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)], 1)))
            return torch.sigmoid(self.final_layer(self.deconv_layers(x)))

    ref = TorchHead(head).to(dev).train()
    R = a.rois
    xh = torch.rand(R, 64, 56, 56, generator=g).to(dev)
    gt = generate_target_heatmap((torch.rand(R, 17, 2, generator=g) * 0.8 + 0.1).to(dev), (56, 56), sigma=3.0)
    crit = AdaptiveHeatmapLoss()

    def native_step():
        head.zero_grad(set_to_none=True)
        crit(head(xh)[0], gt).backward()

    def torch_step():
        ref.zero_grad(set_to_none=True)
        crit(ref(xh), gt).backward()

    med, ms = alternate({"native": native_step, "torch": torch_step}, max(1, a.inner // 2))
    res["head_step"] = {
        "rois": R, "native_ms": round(med["native"], 3), "torch_modules_ms": round(med["torch"], 3),
        "native_over_torch": round(med["native"] / med["torch"], 3),
        "native_ms_min_max": [round(min(ms["native"]), 3), round(max(ms["native"]), 3)],
        "torch_ms_min_max": [round(min(ms["torch"]), 3), round(max(ms["torch"]), 3)]}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4, help="back-to-back calls per timed interval")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=600, help="seconds the measuring child may take")
    ap.add_argument("--amp", action="store_true", help="head step, train_precision split against mixed")
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
