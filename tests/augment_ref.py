"""Numpy restatement of the augmentation rules (DESIGN.md §3f,
kpd_augment_batch).  A helper for tests/test_augment.py, not a test module.

Every output pixel of the whole image is evaluated from the written rule in
int64 -- no tiles, no stepping along a row, no clamped indices -- so nothing
here shares the kernel's structure.  It takes the same q / N / flags the kernel
takes, so bit-equality does not hinge on host trigonometry; ``matrices`` is a
restatement of the host's construction of them for the property tests.
"""
import numpy as np

i64, f64, f32 = np.int64, np.float64, np.float32


def matrices(W, H, mirror=False, angle_deg=0.0, scale=1.0):
    """(q int32 [6], N float64 [6]) of one W x H image: A = s R(t) diag(+-1, 1),
    p' = c + A (p - c) with c = ((W-1)/2, (H-1)/2); q = floor([A^-1 | c - A^-1 c] * 65536 + 0.5);
    N the forward map under px = x W - 0.5, x' = (px' + 0.5) / W."""
    t = np.deg2rad(f64(angle_deg))
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]], f64)
    A = f64(scale) * R @ np.diag([-1.0 if mirror else 1.0, 1.0])
    Ai = np.linalg.inv(A)
    c = np.array([(W - 1) / 2, (H - 1) / 2], f64)
    q = np.floor(np.concatenate([Ai, (c - Ai @ c)[:, None]], 1) * 65536.0 + 0.5).astype(np.int32)
    S, Si = np.diag([f64(W), f64(H)]), np.diag([1.0 / W, 1.0 / H])
    # px = S x - 0.5;  px' = c + A (S x - 0.5 - c);  x' = Si (px' + 0.5)
    M = Si @ A @ S
    b = Si @ (c + 0.5 - A @ (c + 0.5))
    return q.reshape(6), np.concatenate([M, b[:, None]], 1).reshape(6)


def warp(img, q, fill=(0, 0, 0), gain=256, offset=0):
    """The image rule on one uint8 [H, W] or [H, W, C] image."""
    flat = img.ndim == 2
    src = (img[:, :, None] if flat else img).astype(i64)
    H, W, C = src.shape
    q = np.asarray(q).astype(i64).reshape(6)
    y, x = np.mgrid[0:H, 0:W].astype(i64)
    sx = q[0] * x + q[1] * y + q[2]
    sy = q[3] * x + q[4] * y + q[5]
    sx5, sy5 = (sx + 1024) >> 11, (sy + 1024) >> 11
    ix, fx = sx5 >> 5, sx5 & 31
    iy, fy = sy5 >> 5, sy5 & 31
    padded = np.empty((H + 2, W + 2, C), i64)   # the source inside a one-pixel frame of fill
    padded[:] = np.asarray(fill, i64)[:C]
    padded[1:-1, 1:-1] = src

    def t(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return padded[np.where(inside, yy + 1, 0), np.where(inside, xx + 1, 0)]

    fx, fy = fx[:, :, None], fy[:, :, None]
    acc = ((32 - fx) * (32 - fy) * t(iy, ix) + fx * (32 - fy) * t(iy, ix + 1)
           + (32 - fx) * fy * t(iy + 1, ix) + fx * fy * t(iy + 1, ix + 1))
    v = (acc + 512) >> 10
    out = np.clip((v * i64(gain) + i64(offset) + 128) >> 8, 0, 255).astype(np.uint8)
    return out[:, :, 0] if flat else out


def _map(N, x, y):
    return (N[0] * x + N[1] * y) + N[2], (N[3] * x + N[4] * y) + N[5]


def labels(kpts, vis, boxes, N, mirror, pairs):
    """The label rule on one image: kpts [P, K, 2], vis [P, K], boxes [P, 4] (fp32) -> the same, fp32."""
    N = np.asarray(N, f64).reshape(6)
    P, K = vis.shape
    okp, ovis, obox = np.zeros((P, K, 2), f32), np.zeros((P, K), f32), np.zeros((P, 4), f32)
    for p in range(P):
        for k in range(K):
            s = pairs[k] if mirror else k
            x, y, v = kpts[p, s, 0], kpts[p, s, 1], vis[p, s]
            if v == 0 or (x == 0 and y == 0):
                okp[p, k], ovis[p, k] = (x, y), v
                continue
            X, Y = _map(N, f64(x), f64(y))
            X, Y = f32(X), f32(Y)
            if 0 <= X < 1 and 0 <= Y < 1:
                okp[p, k], ovis[p, k] = (X, Y), v
        cx, cy, w, h = (f64(t) for t in boxes[p])
        if cx == 0 and cy == 0 and w == 0 and h == 0:
            continue
        x0, x1, y0, y1 = cx - 0.5 * w, cx + 0.5 * w, cy - 0.5 * h, cy + 0.5 * h
        pts = [_map(N, a, b) for a, b in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
        lx, hx = (min(max(f(p_[0] for p_ in pts), 0.0), 1.0) for f in (min, max))
        ly, hy = (min(max(f(p_[1] for p_ in pts), 0.0), 1.0) for f in (min, max))
        if hx - lx > 0 and hy - ly > 0:
            obox[p] = (0.5 * (lx + hx), 0.5 * (ly + hy), hx - lx, hy - ly)
    return okp, ovis, obox


def label_margin(kpts, vis, boxes, N, mirror, pairs):
    """The smallest distance of a transformed live joint coordinate, or of a mapped box edge before
    clipping, from the borders 0 and 1 -- the tests' condition on their seeds."""
    N = np.asarray(N, f64).reshape(6)
    m = np.inf
    for p in range(vis.shape[0]):
        for k in range(vis.shape[1]):
            x, y, v = kpts[p, k, 0], kpts[p, k, 1], vis[p, k]
            if v == 0 or (x == 0 and y == 0):
                continue
            for c in _map(N, f64(x), f64(y)):
                m = min(m, abs(c), abs(c - 1))
        cx, cy, w, h = (f64(t) for t in boxes[p])
        if cx == 0 and cy == 0 and w == 0 and h == 0:
            continue
        x0, x1, y0, y1 = cx - 0.5 * w, cx + 0.5 * w, cy - 0.5 * h, cy + 0.5 * h
        pts = [_map(N, a, b) for a, b in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
        for ax in (0, 1):
            for e in (min(p_[ax] for p_ in pts), max(p_[ax] for p_ in pts)):
                m = min(m, abs(e), abs(e - 1))
    return m
