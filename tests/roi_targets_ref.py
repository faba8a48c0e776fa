"""Numpy restatement of kpd_roi_targets (include/kpd.h).

Decisions (the box origin, u, v, the `on` test, px, py) are taken in float32
in the operation order the header states; the plane values are computed in
float64 from those float32 px, py (``dtype=np.float32`` computes them in
float32 in the kernel's order instead, which is what the tests measure the
float32 rule's own deviation with)."""
import numpy as np


def roi_targets_ref(kpts, vis, boxes, rows, H, W, sigma, dtype=np.float64):
    """kpts [R,K,2], vis [R,K], boxes [R,4] -> (heat [n,K,H,W] of ``dtype``, weight [n,K] float32)."""
    f = np.float32
    kpts, vis, boxes = np.asarray(kpts, f), np.asarray(vis, f), np.asarray(boxes, f)
    R, K = vis.shape
    rows = np.arange(R) if rows is None else np.asarray(rows, np.int64)
    k, v, b = kpts[rows], vis[rows], boxes[rows]
    with np.errstate(all="ignore"):
        cx, cy, w, h = (b[:, i:i + 1] for i in range(4))
        bx, by = cx - w / f(2), cy - h / f(2)
        u, vv = (k[..., 0] - bx) / w, (k[..., 1] - by) / h
        on = (w > 0) & (h > 0) & (v > 0) & (u >= 0) & (u <= 1) & (vv >= 0) & (vv <= 1)   # NaN compares false
        px, py = u * f(W - 1), vv * f(H - 1)
        assert px.dtype == f and u.dtype == f
        if dtype == np.float32:
            den = f(2) * f(sigma) * f(sigma)
        else:
            den = 2.0 * float(sigma) * float(sigma)
        dx = np.arange(W, dtype=dtype)[None, None, None, :] - px.astype(dtype)[..., None, None]
        dy = np.arange(H, dtype=dtype)[None, None, :, None] - py.astype(dtype)[..., None, None]
        heat = np.exp(-(dx * dx + dy * dy) / dtype(den)).astype(dtype)
    heat = np.where(on[..., None, None], heat, dtype(0))
    return heat, on.astype(f)


def decode_to_image(heat, boxes_rows):
    """Argmax of each plane read as i/(W-1), mapped through the unclamped box: [n,K,2] image-normalised."""
    n, K, H, W = heat.shape
    idx = heat.reshape(n, K, -1).argmax(-1)
    x, y = (idx % W) / (W - 1), (idx // W) / (H - 1)
    b = np.asarray(boxes_rows, np.float64)
    cx, cy, w, h = (b[:, i:i + 1] for i in range(4))
    return np.stack([x * w + (cx - w / 2), y * h + (cy - h / 2)], -1)


def cases(R, K, seed):
    """Seeded boxes and joints inside them, with every `off` case and both
    border cases planted (needs R >= 3, K >= 5): returns kpts, vis, boxes and
    {name: (r, k)}."""
    rng = np.random.default_rng(seed)
    f = np.float32
    boxes = np.stack([rng.uniform(0.3, 0.7, R), rng.uniform(0.3, 0.7, R), rng.uniform(0.1, 0.5, R),
                      rng.uniform(0.1, 0.5, R)], 1).astype(f)
    uv = rng.uniform(0.02, 0.98, (R, K, 2))
    kpts = (boxes[:, None, :2] - boxes[:, None, 2:] / 2 + uv * boxes[:, None, 2:]).astype(f)
    vis = rng.integers(1, 3, (R, K)).astype(f)
    # dyadic box 0: origin (0.25, 0.25), size 0.5 -> u exactly 0 and exactly 1
    boxes[0] = (0.5, 0.5, 0.5, 0.5)
    kpts[0] = (0.25 + 0.5 * rng.integers(1, 8, (K, 2)) / 8).astype(f)
    where = {"u0": (0, 0), "u1": (0, 1), "vis0": (0, 2), "outside": (0, 3), "nan": (0, 4)}
    kpts[0, 0] = (0.25, 0.5)
    kpts[0, 1] = (0.75, 0.75)
    vis[0, 2] = 0
    kpts[0, 3] = (0.8, 0.5)
    kpts[0, 4] = (np.nan, 0.5)
    boxes[1, 2] = 0          # w == 0: the whole row is off
    boxes[2] = 0             # the collate padding: an all-zero box
    where["w0"], where["zero_box"] = (1, 0), (2, 0)
    return kpts, vis, boxes, where
