"""Plain references for the stand-alone operator kernels (csrc/ops_kernels.hip,
csrc/data_kernels.hip, topk_kernel of csrc/head_kernels.hip).  No device code:
numpy / torch on the CPU.  Every decision (which index is the maximum, which
sample is skipped, which pixels a target covers, which keypoint counts) is
taken the way the reference implementation takes it, in its number format;
every sum is taken in fp64.  tests/test_ops_ref_cpu.py ties each function to
the fixtures made by the reference's own code.
"""
from __future__ import annotations

import math

import numpy as np
import torch

ARGMAX, SUBPIXEL, SOFTARGMAX, MODEL = 0, 1, 2, 3
F32 = np.float32


# ----------------------------------------------------------------- decoders
def _argmax_first(flat: np.ndarray) -> int:
    """torch.max's index: a NaN counts as the maximum, the first index wins."""
    nan = np.isnan(flat)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(flat))          # first occurrence of the maximum


def visibility_ref(mx: np.ndarray) -> np.ndarray:
    """keypoint_model.py:262-280: sigmoid in fp32, compared as a double with
    0.3 and 0.7 (a NaN confidence fails both tests: class 2)."""
    conf = torch.sigmoid(torch.from_numpy(np.asarray(mx, F32))).double().numpy()
    cls = np.where(conf < 0.3, 0, np.where(conf < 0.7, 1, 2))
    return np.eye(3, dtype=F32)[cls]


def decode_ref(heat: torch.Tensor, mode: int, param: float = 0.0) -> dict:
    """heat [B,K,H,W] fp32 -> dict of
         kpts [B,K,2] fp64 (argmax: the fp32 values, exactly), scores [B,K] fp32,
         vis [B,K,3] (MODEL), and for SUBPIXEL what sizes a tolerance:
         n_window [B,K] and cond [B,K,2] = sum|v*x| / |sum v| (x, y)."""
    h32 = heat.detach().cpu().float().numpy()
    B, K, H, W = h32.shape
    kpts = np.zeros((B, K, 2), np.float64)
    scores = np.zeros((B, K), F32)
    n_window = np.zeros((B, K), np.int64)
    cond = np.zeros((B, K, 2), np.float64)
    for b in range(B):
        for k in range(K):
            p = h32[b, k]
            mi = _argmax_first(p.reshape(-1))
            xc, yc = mi % W, mi // W
            mx = p[yc, xc]
            if mode == ARGMAX:
                kpts[b, k] = (F32(xc) / F32(W - 1), F32(yc) / F32(H - 1))
                scores[b, k] = mx
            elif mode == SUBPIXEL:
                pad = int(param) // 2                          # Python floor: negative window -> empty
                x0, x1 = max(0, xc - pad), min(W, xc + pad + 1)
                y0, y1 = max(0, yc - pad), min(H, yc + pad + 1)
                if x1 <= x0 or y1 <= y0:
                    continue
                win = p[y0:y1, x0:x1].astype(np.float64)
                n_window[b, k] = win.size
                mass = win.sum()
                if not mass > 0:                               # zero, negative or NaN mass: zeros
                    continue
                ys, xs = np.meshgrid(np.arange(y0, y1, dtype=np.float64), np.arange(x0, x1, dtype=np.float64),
                                     indexing="ij")
                kpts[b, k] = ((xs * win).sum() / mass / (W - 1), (ys * win).sum() / mass / (H - 1))
                cond[b, k] = (np.abs(xs * win).sum() / abs(mass), np.abs(ys * win).sum() / abs(mass))
                scores[b, k] = p[y0:y1, x0:x1].max()           # mass > 0: no NaN in the window
            else:
                z = torch.from_numpy(p.reshape(-1)).double()
                if mode == SOFTARGMAX:
                    z = z / float(F32(param))                  # tensor / Python scalar: the scalar becomes fp32
                sm = torch.softmax(z, dim=0).numpy().reshape(H, W)
                ex = (sm * np.arange(W, dtype=np.float64)[None, :]).sum()
                ey = (sm * np.arange(H, dtype=np.float64)[:, None]).sum()
                kpts[b, k] = (ex / (W - 1), ey / (H - 1))
                scores[b, k] = mx
    out = {"kpts": kpts, "scores": scores, "n_window": n_window, "cond": cond}
    if mode == MODEL:
        out["vis"] = visibility_ref(scores)
    return out


def subpixel_bound(ref: dict, H: int, W: int) -> np.ndarray:
    """(n_window + 3) * 2^-23 * sum|v x| / |sum v| / (W - 1), per plane and axis:
    n products and sums, the mass, the quotient and the normalisation in fp32."""
    n = ref["n_window"][..., None].astype(np.float64)
    return (n + 3) * 2.0 ** -23 * ref["cond"] / np.array([W - 1, H - 1], np.float64)


def soft_argmax_fp32(heat: torch.Tensor, temperature=None) -> np.ndarray:
    """The reference's own soft-argmax formula in torch fp32 on the CPU
    (heatmap_head.py:388-408 / keypoint_model.py:284-313), restated: the
    yardstick for what an fp32 evaluation can reach."""
    h = heat.detach().cpu().float()
    B, K, H, W = h.shape
    z = h if temperature is None else h / temperature
    sm = torch.softmax(z.reshape(B, K, -1), dim=2).reshape(B, K, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    ey = (sm * ys).sum(dim=(2, 3)) / (H - 1)
    ex = (sm * xs).sum(dim=(2, 3)) / (W - 1)
    return torch.stack([ex, ey], dim=-1).numpy()


# ---------------------------------------------------------------- ROI align
def _axis(start: F32, bin_: F32, n_out: int, grid: int, size: int):
    """One axis of torchvision's roi_align forward: sample coordinates in fp32
    in its expression order, its decisions on them, fp64 weights.
    -> (M [n_out, size] fp64 interpolation matrix, distance to a skip boundary)."""
    M = np.zeros((n_out, size), np.float64)
    dist = math.inf
    for p in range(n_out):
        for i in range(grid):
            c = F32(F32(start + F32(F32(p) * bin_)) + F32(F32(F32(F32(i) + F32(0.5)) * bin_) / F32(grid)))
            dist = min(dist, abs(float(c) + 1.0), abs(float(c) - size))
            if c < F32(-1.0) or c > F32(size):
                continue
            if c <= 0:
                c = F32(0)
            lo = int(c)
            if lo >= size - 1:
                hi = lo = size - 1
                c = F32(lo)
            else:
                hi = lo + 1
            l = float(c) - lo
            M[p, lo] += 1.0 - l
            M[p, hi] += l
    return M, dist


def roi_align_ref(feat: torch.Tensor, rois: torch.Tensor, out_hw, spatial_scale: float = 1.0,
                  sampling_ratio: int = -1, aligned: bool = False):
    """torchvision.ops.roi_align forward restated.  feat [B,C,H,W], rois [R,5]
    -> (out [R,C,oh,ow] fp64, info) with info["skip_dist"] the smallest distance
    of any sample coordinate from a skip boundary (-1, H, W) and info["grid"]
    the (gh, gw) of every ROI.  The skip test is separable (a sample is dropped
    when either coordinate is outside), so the bin average is My . feat . Mx^T.
    A batch index that names no image gives zeros (the project's contract;
    torchvision reads out of bounds)."""
    f = feat.detach().cpu().double().numpy()
    r32 = rois.detach().cpu().float().numpy()
    B, C, H, W = f.shape
    oh, ow = (out_hw, out_hw) if isinstance(out_hw, int) else tuple(out_hw)
    out = np.zeros((len(r32), C, oh, ow), np.float64)
    info = {"skip_dist": math.inf, "grid": []}
    scale, off = F32(spatial_scale), F32(0.5 if aligned else 0.0)
    for r, ro in enumerate(r32):
        x1, y1, x2, y2 = (F32(F32(v * scale) - off) for v in ro[1:])
        rw, rh = F32(x2 - x1), F32(y2 - y1)
        if not aligned:
            rw, rh = max(rw, F32(1.0)), max(rh, F32(1.0))
        bh, bw = F32(rh / F32(oh)), F32(rw / F32(ow))
        gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(F32(rh / F32(oh))))
        gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(F32(rw / F32(ow))))
        info["grid"].append((gh, gw))
        bf = float(ro[0])
        if not (-1.0 < bf < B):
            continue
        count = max(gh * gw, 1)
        My, dy = _axis(y1, bh, oh, gh, H)
        Mx, dx = _axis(x1, bw, ow, gw, W)
        if gh > 0 and gw > 0:
            info["skip_dist"] = min(info["skip_dist"], dy, dx)
        out[r] = np.einsum("ph,chw,qw->cpq", My, f[int(bf)], Mx) / count
    return out, info


def roi_align_bound(info: dict, feat: torch.Tensor) -> np.ndarray:
    """(4 gh gw + 2) * 2^-23 * max|feat| per ROI (the issue's rounding budget)."""
    m = float(feat.abs().max()) if feat.numel() else 0.0
    return np.array([(4 * max(gh, 0) * max(gw, 0) + 2) * 2.0 ** -23 * m for gh, gw in info["grid"]])


# -------------------------------------------------- channel attention, top-k
def channel_select_ref(x: torch.Tensor, sd: dict, k: int = 64, prefix: str = "channel_attention."):
    """ChannelAttention + select_top_k_channels in fp64.  -> (scores [B,C] fp64,
    topk [B,k] int64, min_gap [B]: the smallest difference between two
    neighbouring distinct finite scores in the ranking).  Order: a NaN before
    every number (torch.topk), then score descending, index ascending among
    equals."""
    xd = x.detach().cpu().double()
    w0, b0 = sd[prefix + "fc.0.weight"].double(), sd[prefix + "fc.0.bias"].double()
    w2, b2 = sd[prefix + "fc.2.weight"].double(), sd[prefix + "fc.2.bias"].double()

    def fc(v):
        return torch.relu(v @ w0.T + b0) @ w2.T + b2
    scores = torch.sigmoid(fc(xd.mean(dim=(2, 3))) + fc(xd.amax(dim=(2, 3)))).numpy()
    topk, gaps = [], []
    for s in scores:
        order = sorted(range(len(s)), key=lambda c: (0, 0.0, c) if math.isnan(s[c]) else (1, -s[c], c))
        topk.append(order[:k])
        fin = np.array([s[c] for c in order if not math.isnan(s[c])])
        d = -np.diff(fin)
        gaps.append(float(d[d > 0].min()) if (d > 0).any() else math.inf)
    return scores, np.array(topk, np.int64), np.array(gaps)


def conv1x1_ref(x: torch.Tensor, w: torch.Tensor, b=None):
    """-> (out [B,Cout,H,W] fp64, mag [B,Cout,H,W] = sum_ci |w x| (+ |b|)) for the error bound."""
    xd, wd = x.detach().cpu().double(), w.detach().cpu().double().reshape(w.shape[0], -1)
    out = torch.einsum("oc,bchw->bohw", wd, xd)
    mag = torch.einsum("oc,bchw->bohw", wd.abs(), xd.abs())
    if b is not None:
        bd = b.detach().cpu().double().view(1, -1, 1, 1)
        out, mag = out + bd, mag + bd.abs()
    return out.numpy(), mag.numpy()


# ------------------------------------------------------------------ targets
# The reference's own fp32 table (tests/golden/ops_edges.npz) against the fp64
# table below, largest relative difference over the ops_edges target cases:
# measured 3.12e-7 (test_ops_ref_cpu.py asserts it stays below this ceiling).
TABLE_REL_ERR = 3.13e-7


def gaussian_table(sigma: float, table_dtype=np.float32) -> np.ndarray:
    """get_gaussian_kernel(6*int(sigma)+1, sigma).  fp32 (default): torch's
    steps, the denominator 2*sigma**2 rounded to fp32 once from the double.
    fp64: the same table from the same fp32 denominator, exp / sum / division
    in double -- the yardstick for the fp32 table's own error."""
    ks = 6 * int(sigma) + 1
    den = F32(2 * sigma ** 2)
    co = np.arange(ks, dtype=F32) - F32((ks - 1) / 2)
    sq = (co[:, None] ** 2 + co[None, :] ** 2).astype(F32)
    if table_dtype == np.float32:
        g = np.exp((-sq / den).astype(F32)).astype(F32)
        return (g / g.sum(dtype=F32)).astype(F32)
    g = np.exp(-sq.astype(np.float64) / np.float64(den))
    return g / g.sum()


def target_heatmap_ref(kp: torch.Tensor, size, sigma: float, table_dtype=np.float64) -> np.ndarray:
    """generate_target_heatmap (heatmap_head.py:163-224) restated; sigma is a
    Python double.  kp [B,K,2] or [B,P,K,2] (flattened to B*P rows of which the
    first B are filled, as the reference's loop does) -> [B,K,H,W].  The
    pixel coordinates and the inside test are fp32.  A NaN keypoint leaves its
    plane zero: the project's contract (the reference raises on int(NaN))."""
    kp = kp.detach().cpu().float()
    if kp.dim() == 4:
        B, P, K, _ = kp.shape
        kp = kp.reshape(B * P, K, -1)[:B]
    B, K = kp.shape[:2]
    H, W = int(size[0]), int(size[1])
    g = gaussian_table(sigma, table_dtype)
    ks = g.shape[0]
    r = ks // 2
    out = np.zeros((B, K, H, W), g.dtype)
    px = (kp[..., 0].numpy() * F32(W)).astype(F32)
    py = (kp[..., 1].numpy() * F32(H)).astype(F32)
    for b in range(B):
        for k in range(K):
            x0, y0 = px[b, k], py[b, k]
            if not (x0 >= 0 and y0 >= 0 and x0 < W and y0 < H):
                continue
            fx, fy = int(x0), int(y0)
            xa, xb = max(fx - r, 0), min(fx + r + 1, W)
            ya, yb = max(fy - r, 0), min(fy + r + 1, H)
            out[b, k, ya:yb, xa:xb] = g[ya - fy + r:yb - fy + r, xa - fx + r:xb - fx + r]
    return out


def adaptive_sigma(size, base_sigma: float = 3.0) -> float:
    """generate_target_heatmap_adaptive (heatmap_head.py:243-248)."""
    return base_sigma * max(0.8, min(size) / 56.0)


# ------------------------------------------------------------------ metrics
def keypoint_metrics_ref(pred: torch.Tensor, gt: torch.Tensor, vis: torch.Tensor, thresholds):
    """Trainer._calculate_validation_metrics (trainer.py:406-422) on matching
    shapes [...,2] / [...]: fp32 distance, fp64 means.  -> (ADE, [PCK_t], counts
    [#visible, #correct_t ...]); dist <= t compares with the fp32 threshold (a
    Python scalar against an fp32 tensor); PCK divides by all keypoints."""
    d = (pred.detach().cpu().float() - gt.detach().cpu().float()).numpy().reshape(-1, 2)
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32)).astype(F32)
    m = vis.detach().cpu().float().numpy().reshape(-1) > 0
    n, nv = len(dist), int(m.sum())
    if nv == 0:
        return 0.0, [0.0] * len(thresholds), [0] * (1 + len(thresholds))
    counts = [int(((dist <= F32(t)) & m).sum()) for t in thresholds]
    return float(dist[m].astype(np.float64).mean()), [c / n for c in counts], [nv] + counts
