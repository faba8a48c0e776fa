"""Numpy restatement of kpd_flip_merge (include/kpd.h) and of
dll.utils.flip.mirror_boxes.  The merged map and its peaks are formed in
float32 exactly as the kernel forms them (one add, an exact halving, a
maximum), so they compare bit for bit; the decode runs in float64 on that
float32 map, so the kernel's fp32 soft-argmax is compared against the exact
value of the same softmax."""
import numpy as np

f32 = np.float32
TINY = np.finfo(np.float32).tiny


def flip_index(K=17):
    idx = list(range(K))
    for a in range(1, K - 1, 2):
        idx[a], idx[a + 1] = a + 1, a
    return idx


def mirror_boxes(boxes):
    b = np.asarray(boxes, f32)
    out = b.copy()
    zero = (b == 0).all(-1)
    cx = (f32(1) - b[..., 0]).astype(f32)
    degenerate = (cx == 0) & (b[..., 1:] == 0).all(-1) & ~zero
    cx[degenerate] = TINY
    cx[zero] = 0
    out[..., 0] = cx
    return out


def mirror_swap(heat, pairs):
    """[..., K, H, W]: planes permuted by ``pairs`` and mirrored left-right."""
    return np.ascontiguousarray(np.asarray(heat)[..., list(pairs), :, ::-1])


def compaction(boxes):
    """Per image the caller rows of its non-zero boxes, in order (slot s = s-th of them)."""
    b = np.asarray(boxes, f32)
    return [[p for p in range(b.shape[1]) if not (b[i, p] == 0).all()] for i in range(b.shape[0])]


def flip_merge(heat_a, heat_b, boxes, pairs):
    a, b, boxes = np.asarray(heat_a, f32), np.asarray(heat_b, f32), np.asarray(boxes, f32)
    n, P, K, H, W = a.shape
    heat = np.zeros((n, P, K, H, W), f32)
    kp = np.zeros((n, P, K, 2), np.float64)
    vis = np.zeros((n, P, K, 3), f32)
    peaks = np.zeros((n, P, K), f32)
    conf = np.full((n, P, K), np.nan)
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    for i, rows in enumerate(compaction(boxes)):
        if not rows:
            vis[i, 0, :, 0] = 1          # the dummy person
        for s, p in enumerate(rows):
            cx, cy, w, h = (np.float64(v) for v in boxes[i, p])
            m = (f32(0.5) * (a[i, s] + mirror_swap(b[i, s], pairs)).astype(f32)).astype(f32)
            heat[i, s] = m
            peaks[i, s] = m.max((-2, -1))
            for k in range(K):
                d = m[k].astype(np.float64)
                e = np.exp(d - d.max())
                e /= e.sum()
                kx = (e.sum(0) * xs).sum() / (W - 1) if W > 1 else 0.0
                ky = (e.sum(1) * ys).sum() / (H - 1) if H > 1 else 0.0
                kp[i, s, k] = (min(max(kx * w + (cx - w / 2), 0.0), 1.0), min(max(ky * h + (cy - h / 2), 0.0), 1.0))
                c = 1.0 / (1.0 + np.exp(-np.float64(peaks[i, s, k])))
                conf[i, s, k] = c
                vis[i, s, k, 0 if c < 0.3 else (1 if c < 0.7 else 2)] = 1
    return {"heatmap": heat, "keypoints": kp, "visibilities": vis, "keypoint_peaks": peaks, "confidence": conf}


def margin(ref):
    """Smallest distance of a live plane's sigmoid(peak) from the class borders 0.3 / 0.7."""
    c = ref["confidence"][~np.isnan(ref["confidence"])]
    return float(np.minimum(np.abs(c - 0.3), np.abs(c - 0.7)).min()) if c.size else np.inf
