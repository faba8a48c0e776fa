"""Shapes, draws and exact one-hot expectations shared by
tests/test_conv3_shapes.py (device) and tests/test_train_edges_cpu.py (the
expectations against torch in float64).  Needs no GPU.

Shapes are (N, C, H, W, O).  With W2 = W + 2 the wgrad kernels walk zero-padded
planes of (H + 2) * W2 positions, padded up to a multiple of the 32-position
K-step; they pick 128- or 256-wide tiles by C > 128 and O > 128."""
import torch
import torch.nn.functional as F

SHAPES = [
    # tile thresholds and grids of more than one tile
    (2, 127, 6, 6, 129),     # C one 128 tile with one padded row; O just over: 256 tile, 127 padded rows
    (2, 129, 5, 7, 128),     # the transpose of that choice; padded plane 63
    (2, 128, 6, 6, 128),     # both exactly at the threshold: 128 tiles, no padded row
    (1, 257, 4, 4, 257),     # 256 tiles, two along each axis, 255 padded rows in the second
    (2, 130, 3, 2, 300),     # 256 x 256 tiles, two along O only
    # degenerate maps: padded plane 3 wide and / or 3 high, the guard at its smallest
    (3, 1, 1, 1, 1),
    (2, 3, 1, 9, 2),
    (2, 3, 9, 1, 2),
    (2, 8, 2, 2, 8),
    # W + 2 mod 4 = 0, 1, 2, 3 at H = 3 (the bf16 wgrad's funnel shift by off mod 4)
    (2, 6, 3, 2, 10),
    (2, 6, 3, 3, 10),
    (2, 6, 3, 4, 10),
    (2, 6, 3, 5, 10),
    # the K-step tail: padded plane 64 (no zero tail), 63 (tail of one), 128
    (1, 4, 6, 6, 4),
    (1, 4, 5, 7, 4),
    (1, 4, 6, 14, 4),
    # the generic GEMM's 64 x 64 tiles and K-steps of 16: H*W 64 | 65, M 64 | 65, 9 C = 144
    (1, 16, 8, 8, 64),
    (1, 7, 5, 13, 65),
    (2, 16, 8, 8, 65),
    # 56 x 56 and its near misses that fail the fast forward / dgrad shape test
    (1, 32, 56, 56, 64),
    (1, 128, 56, 56, 64),
    (1, 64, 56, 55, 64),
    (1, 64, 55, 56, 64),
]
PLACEMENT_SHAPES = [(2, 5, 3, 4, 6), (1, 130, 2, 3, 129), (1, 64, 56, 56, 64)]
MULTI_TILE = (1, 257, 4, 4, 257)
PRECISIONS = ["split", "mixed"]


def shape_id(s):
    return "x".join(map(str, s))


def padded_plane(shape):
    """(H + 2) * (W + 2): the positions of one zero-padded plane."""
    return (shape[2] + 2) * (shape[3] + 2)


_DATA = {}


def draw(shape):
    """x, w, b, gy of a shape as the conv tests draw them, once, never modified."""
    if shape not in _DATA:
        N, C, H, W, O = shape
        g = torch.Generator().manual_seed(N * 1000 + C + O)
        _DATA[shape] = (torch.randn(N, C, H, W, generator=g), torch.randn(O, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5,
                        torch.randn(O, generator=g) * 0.1, torch.randn(N, O, H, W, generator=g))
    return _DATA[shape]


def ref_split(x, w, b, gy):
    """(y, gx, gw, gb) of torch's conv2d with autograd in float64 on the CPU."""
    x64, w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x64, w64, b64, padding=1)
    y.backward(gy.double().cpu())
    return y.detach(), x64.grad, w64.grad, b64.grad


# ---------------------------------------------------------------- one-hot placements
def placements(H, W):
    """Every corner, the middle of every border, and the interior pixel nearest
    the centre (duplicates of a small map dropped), as (y, x)."""
    ys, xs = sorted({0, H // 2, H - 1}), sorted({0, W // 2, W - 1})
    return [(y, x) for y in ys for x in xs]


def neighbours(H, W, y, x):
    """The in-map positions within one pixel of (y, x), (y, x) itself included,
    and one position further away when the map has one."""
    near = [(y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 <= y + dy < H and 0 <= x + dx < W]
    far = [(yy, xx) for yy in (0, H - 1) for xx in (0, W - 1) if abs(yy - y) > 1 or abs(xx - x) > 1]
    return near + far[:1]


def dyadic_weights(shape, seed=5):
    """w [O][C][3][3] and b [O]: integers in [-8, 8] over 8, none zero in w --
    exact in f16, in bf16 and in every sum of two of them."""
    _, C, _, _, O = shape
    g = torch.Generator().manual_seed(seed + C * 7 + O)
    w = torch.randint(1, 9, (O, C, 3, 3), generator=g).float() * (torch.randint(0, 2, (O, C, 3, 3), generator=g) * 2 - 1)
    b = torch.randint(-8, 9, (O,), generator=g).float()
    return w / 8, b / 8


def onehot(dims, idx, device=None):
    t = torch.zeros(*dims, device=device)
    t[idx] = 1.0
    return t


def expect_wgrad(shape, xi, gi):
    """gw for x = one 1.0 at xi = (n, c, y, x) and gy = one 1.0 at gi = (n', o, y', x'):
    one 1.0 at the tap (y - y' + 1, x - x' + 1) when n == n' and the tap lies in the kernel."""
    _, C, _, _, O = shape
    gw = torch.zeros(O, C, 3, 3)
    ky, kx = xi[2] - gi[2] + 1, xi[3] - gi[3] + 1
    if xi[0] == gi[0] and 0 <= ky < 3 and 0 <= kx < 3:
        gw[gi[1], xi[1], ky, kx] = 1.0
    return gw


def expect_forward(shape, xi, w, b):
    """y for x = one 1.0 at xi: the bias, plus w[:, c, ky, kx] at the output pixel
    (y - ky + 1, x - kx + 1) of image n for every tap whose pixel lies in the map."""
    N, _, H, W, O = shape
    n, c, y, x = xi
    out = b.view(1, O, 1, 1).expand(N, O, H, W).clone()
    for ky in range(3):
        for kx in range(3):
            py, px = y - ky + 1, x - kx + 1
            if 0 <= py < H and 0 <= px < W:
                out[n, :, py, px] += w[:, c, ky, kx]
    return out


def expect_dgrad(shape, gi, w):
    """gx for gy = one 1.0 at gi = (n, o, y, x): w[o, :, ky, kx] at the input pixel
    (y + ky - 1, x + kx - 1) of image n."""
    N, C, H, W, _ = shape
    n, o, y, x = gi
    out = torch.zeros(N, C, H, W)
    for ky in range(3):
        for kx in range(3):
            py, px = y + ky - 1, x + kx - 1
            if 0 <= py < H and 0 <= px < W:
                out[n, :, py, px] += w[o, :, ky, kx]
    return out
