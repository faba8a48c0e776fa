"""kpd_draw_poses (csrc/draw.hip): pose overlays drawn on the device.

CPU part: the ABI, the argument checks (made-up device addresses: they return
before any device work), the numpy restatement tests/draw_ref.py against
values known without it, the label text against the project's own label
parser.  GPU part: the kernel against draw_ref, bit for bit."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import draw_ref as R
from conftest import ROOT

gpu = pytest.mark.gpu
c_int, c_void_p, u8 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint8


# ------------------------------------------------------------------ ABI
def test_symbol_declared_bound_exported():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    assert re.search(r"\bint\s+kpd_draw_poses\s*\(", hdr)
    assert "kpd_draw_poses" in _native.EXPORTS
    lib = _native.load()
    assert hasattr(lib, "kpd_draw_poses") and lib.kpd_draw_poses.restype is c_int
    assert len(lib.kpd_draw_poses.argtypes) == 26


def test_header_constants_match_native():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+KPD_DRAW_(\w+)\s+(\d+)", hdr)}
    mine = {k[5:]: v for k, v in vars(_native).items() if k.startswith("DRAW_")}
    assert defs == mine and {"CHUNK", "TILE_W", "TILE_H", "BOXES", "LIMBS", "JOINTS", "HEAT"} <= set(defs)
    assert (R.BOXES, R.LIMBS, R.JOINTS, R.HEAT) == (defs["BOXES"], defs["LIMBS"], defs["JOINTS"], defs["HEAT"])


# ------------------------------------------------------------------ argument checks
def _args(**over):
    a = dict(images=(c_void_p * 2)(0x10000, 0x20000), heights=(c_int * 2)(16, 16), widths=(c_int * 2)(16, 16),
             pitches=(c_int * 2)(48, 48), n=2, kp=c_void_p(0x30000), vis=c_void_p(0x40000), boxes=c_void_p(0x50000),
             heat=None, P=1, K=17, hh=0, hw=0, limbs=(c_int * 4)(0, 1, 1, 2), L=2, lcol=(u8 * 6)(), jcol=(u8 * 9)(),
             bcol=(u8 * 3)(), r=32, h=16, hb=16, alpha=256, heat_alpha=128, min_class=0, flags=7, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over, word", [
    (dict(n=0), "n must be positive"),
    (dict(n=-3), "n must be positive"),
    (dict(images=None), "null array"),
    (dict(heights=None), "null array"),
    (dict(pitches=None), "null array"),
    (dict(kp=None), "null array"),
    (dict(vis=None), "null array"),
    (dict(jcol=None), "null array"),
    (dict(limbs=None), "null array"),
    (dict(pitches=(c_int * 2)(48, 47)), "image 1"),
    (dict(widths=(c_int * 2)(16, 16385), pitches=(c_int * 2)(48, 3 * 16385)), "image 1"),
    (dict(images=(c_void_p * 2)(0x10000, None)), "image 1"),
    (dict(K=33), "K"),
    (dict(L=65), "L"),
    (dict(limbs=(c_int * 4)(0, 1, 1, 17)), "limb 1"),
    (dict(limbs=(c_int * 4)(-1, 1, 1, 2)), "limb 0"),
    (dict(alpha=257), "alpha"),
    (dict(alpha=-1), "alpha"),
    (dict(heat_alpha=300), "alpha"),
    (dict(r=513), "[0, 512]"),
    (dict(h=513), "[0, 512]"),
    (dict(hb=600), "[0, 512]"),
    (dict(min_class=3), "min_class"),
    (dict(flags=16), "flag"),
    (dict(boxes=None), "need boxes"),
    (dict(flags=15), "heatmap"),
])
def test_argument_checks(over, word):
    from dll import _native
    lib = _native.load()
    assert lib.kpd_draw_poses(*_args(**over)) == -1          # KPD_EINVAL
    msg = lib.kpd_last_error().decode()
    assert msg.startswith("kpd_draw_poses") and word in msg, msg


# ------------------------------------------------------------------ the restatement against known values
def _onehot(cls):
    return np.eye(3, dtype=np.float32)[np.asarray(cls)]


def _single(H, W, kp, cls, st, flags, boxes=None, base=0):
    """One person on a constant image; kp [K,2] normalised, cls [K]."""
    img = np.full((H, W, 3), base, np.uint8)
    kp = np.asarray(kp, np.float32)[None]
    return R.draw_one(img, kp, _onehot(cls)[None], boxes, None, st, flags)


def test_ref_hand_mask_joint():
    st = R.Style(joint_radius=32, alpha=256, joint_colors=((1, 2, 3), (4, 5, 6), (200, 100, 50)))
    out = _single(16, 16, [[0.5, 0.5]], [2], st, R.JOINTS)
    want = np.zeros((16, 16), bool)
    want[6:10, 6:10] = True
    for y, x in ((6, 6), (6, 9), (9, 6), (9, 9)):     # offset (+-1.5, +-1.5) px: 4.5 > 4
        want[y, x] = False
    assert want.sum() == 12
    assert np.array_equal((out != 0).any(-1), want)
    assert (out[want] == (200, 100, 50)).all()        # alpha 256 is the colour itself


def test_ref_hand_mask_limb():
    st = R.Style(limbs=((0, 1),), limb_colors=((9, 8, 7),), limb_half_width=16)
    out = _single(16, 16, [[4 / 16, 8 / 16], [12 / 16, 8 / 16]], [2, 2], st, R.LIMBS)
    want = np.zeros((16, 16), bool)
    want[7:9, 4:12] = True
    assert want.sum() == 16
    assert np.array_equal((out != 0).any(-1), want) and (out[want] == (9, 8, 7)).all()


def test_ref_alpha_zero_changes_nothing():
    st = R.Style(limbs=((0, 1),), limb_colors=((9, 8, 7),), alpha=0)
    out = _single(16, 16, [[0.2, 0.3], [0.8, 0.6]], [2, 2], st, R.LIMBS | R.JOINTS, base=77)
    assert (out == 77).all()


@pytest.mark.parametrize("cx, cy, r16", [(0.5, 0.5, 16), (0.47, 0.53, 23), (0.31, 0.62, 57), (0.503, 0.297, 160),
                                         (0.66, 0.41, 99), (0.5, 0.5, 512)])
def test_ref_disc_area_bounds(cx, cy, r16):
    """Every pixel square lies within sqrt(2)/2 of its centre, so a disc of radius r >= 1 px covers
    pi (r - sqrt2/2)^2 <= N <= pi (r + sqrt2/2)^2 pixels."""
    st = R.Style(joint_radius=r16)
    out = _single(96, 96, [[cx, cy]], [2], st, R.JOINTS)
    n, r, s = int((out != 0).any(-1).sum()), r16 / 16, math.sqrt(2) / 2
    assert math.pi * (r - s) ** 2 <= n <= math.pi * (r + s) ** 2, (n, r)


@pytest.mark.parametrize("a, b, h16", [((0.2, 0.2), (0.8, 0.7), 24), ((0.15, 0.8), (0.85, 0.3), 40),
                                       ((0.5, 0.1), (0.52, 0.9), 16), ((0.9, 0.5), (0.1, 0.45), 100),
                                       ((0.3, 0.3), (0.7, 0.7), 33)])
def test_ref_limb_area_bounds(a, b, h16):
    st = R.Style(limbs=((0, 1),), limb_colors=((255, 255, 255),), limb_half_width=h16)
    S = 128
    out = _single(S, S, [a, b], [2, 2], st, R.LIMBS)
    n, h, s2 = int((out != 0).any(-1).sum()), h16 / 16, math.sqrt(2)
    ax, ay, bx, by = (R.quantise(v, S) / 16 for v in (*a, *b))
    ell = math.hypot(bx - ax, by - ay)
    assert (ell - s2) * (2 * h - s2) <= n <= (ell + s2) * (2 * h + s2), (n, ell, h)


def test_ref_limb_isqrt_form_is_the_squared_test():
    """|p x d| <= isqrt(h^2 d.d) is (p x d)^2 <= h^2 d.d, in exact Python integers."""
    rng = np.random.default_rng(5)
    for _ in range(2000):
        dx, dy = (int(v) for v in rng.integers(-(1 << 21), 1 << 21, 2))
        h = int(rng.integers(0, 513))
        bound = h * h * (dx * dx + dy * dy)
        T = math.isqrt(bound)
        for cross in (max(T - 1, 0), T, T + 1, int(rng.integers(0, 1 << 43))):      # |p x d| at the boundary and anywhere
            assert (cross <= T) == (cross * cross <= bound)


def test_ref_blend_order():
    """A limb (drawn first) under a joint (drawn second) at alpha 128: the rule order, not the reverse."""
    la, jb = 200, 40
    st = R.Style(limbs=((0, 1),), limb_colors=((la, la, la),), joint_colors=((jb, jb, jb),) * 3, alpha=128,
                 joint_radius=48, limb_half_width=32)
    out = _single(16, 16, [[0.25, 0.5], [0.75, 0.5]], [2, 2], st, R.LIMBS | R.JOINTS, base=10)
    bl = lambda v, c: (v * 128 + c * 128 + 128) >> 8     # noqa: E731
    assert out[8, 4, 0] == bl(bl(10, la), jb) != bl(bl(10, jb), la)      # limb and joint 0 overlap at (4, 8)
    assert out[8, 8, 0] == bl(10, la)                                     # limb alone


def test_ref_zero_box_person_and_min_class():
    st = R.Style(joint_radius=32, min_class=1)
    kp = np.array([[[0.25, 0.25]], [[0.75, 0.75]], [[0.25, 0.75]]], np.float32)
    vis = _onehot([[2], [2], [0]])
    boxes = np.array([[0.5, 0.5, 0.5, 0.5], [0, 0, 0, 0], [0.5, 0.5, 0.9, 0.9]], np.float32)
    out = R.draw_one(np.zeros((32, 32, 3), np.uint8), kp, vis, boxes, None, st, R.JOINTS)
    lit = (out != 0).any(-1)
    assert lit[8, 8] and not lit[24, 24] and not lit[24, 8]     # drawn; zero box; class 0 < min_class
    vis0 = np.zeros_like(vis)                                    # all-zero rows: no class, never drawn
    assert not R.draw_one(np.zeros((32, 32, 3), np.uint8), kp, vis0, None, None, R.Style(), R.JOINTS).any()


# ------------------------------------------------------------------ label text
def _parse_labels(path):
    from dll.data.dataloader import OptimizedKeypointsDataset
    ds = object.__new__(OptimizedKeypointsDataset)
    ds.num_keypoints = 17
    return ds._parse_label_file_vectorized(path)


def test_label_file_roundtrip(tmp_path):
    from dll.utils import format_pose_labels
    g = torch.Generator().manual_seed(3)
    kp = torch.rand(1, 3, 1, 17, 2, generator=g)
    cls = torch.randint(0, 3, (1, 3, 1, 17), generator=g)
    vis = torch.nn.functional.one_hot(cls, 3).float()
    b0, b2 = [0.5, 0.4, 0.3, 0.6], [0.123456789, 0.7, 0.2, 0.25]
    # caller boxes with an all-zero row between: the forward compacts persons, so slots 0, 1 belong to b0, b2
    given = {"keypoints": kp, "visibilities": vis, "boxes": [torch.tensor([b0, [0.0] * 4, b2])]}
    path = tmp_path / "given_keypoints.txt"
    path.write_text(format_pose_labels(given))
    ann = _parse_labels(path)
    assert ann.keypoints.shape == (1, 2, 17, 2)
    assert torch.allclose(ann.bboxes[0], torch.tensor([b0, b2]), atol=1e-6, rtol=0)
    assert torch.allclose(ann.keypoints[0], kp[0, :2, 0], atol=1e-6, rtol=0)
    assert torch.equal(ann.visibilities[0], cls[0, :2, 0].float()) and torch.equal(ann.classes, torch.zeros(2).long())
    assert all(re.fullmatch(r"0( \d\.\d{6}){4}( \d\.\d{6} \d\.\d{6} [012]){17}", ln) for ln in
               path.read_text().splitlines())
    # detector outputs: slots with score 0 are absent, the others keep their slot
    det = {"keypoints": kp, "visibilities": vis, "boxes": [torch.tensor([b0, b2, b2])],
           "box_scores": torch.tensor([[0.9, 0.0, 0.4]])}
    path = tmp_path / "det_keypoints.txt"
    path.write_text(format_pose_labels(det))
    ann = _parse_labels(path)
    assert torch.allclose(ann.keypoints[0], kp[0, [0, 2], 0], atol=1e-6, rtol=0)
    assert torch.allclose(ann.bboxes[0], torch.tensor([b0, b2]), atol=1e-6, rtol=0)
    # nothing drawn: an empty file
    assert format_pose_labels({"keypoints": kp, "visibilities": vis, "boxes": [torch.zeros(3, 4)]}) == ""


def test_reference_import_line_resolves():
    from dll.data.dataloader import visualize_keypoints_multi_person
    from dll.utils import COCO_SKELETON, DrawStyle, draw_poses
    assert callable(visualize_keypoints_multi_person) and callable(draw_poses)
    assert len(COCO_SKELETON) == 19 and all(0 <= v < 17 for ab in COCO_SKELETON for v in ab)
    assert len(DrawStyle().resolved_limb_colors()) == 19


# ------------------------------------------------------------------ GPU
DEV = torch.device("cuda:0")
CHAIN = tuple((k, k + 1) for k in range(16)) + ((0, 5), (3, 11), (16, 2))     # 19 limbs over 17 joints


def _style(rng, limbs=CHAIN, **kw):
    d = dict(limbs=limbs, limb_colors=tuple(tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in limbs),
             joint_colors=((90, 90, 90), (250, 160, 10), (255, 30, 60)), box_color=(20, 240, 70), joint_radius=40,
             limb_half_width=20, box_half_width=12, alpha=200, heat_alpha=180, min_class=0)
    d.update(kw)
    return R.Style(**d)


def _case(rng, sizes, P, K=17, hh=8, hw=5, spread=(-0.1, 1.1)):
    n = len(sizes)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    kp = rng.uniform(*spread, (n, P, K, 2)).astype(np.float32)
    vis = _onehot(rng.integers(0, 3, (n, P, K)))
    c = rng.uniform(0.2, 0.8, (n, P, 2))
    boxes = np.concatenate([c, rng.uniform(0.1, 0.9, (n, P, 2))], -1).astype(np.float32)
    heat = rng.uniform(-0.1, 1.05, (n, P, K, hh, hw)).astype(np.float32)
    return imgs, kp, vis, boxes, heat


def _native_draw(dev_imgs, kp, vis, boxes, heat, st, flags):
    """kpd_draw_poses through ctypes on uint8 [H,W,3] device tensors (dense rows), in place."""
    from dll import _native
    lib = _native.load()
    n = len(dev_imgs)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)     # noqa: E731
    kp_d, vis_d, box_d, heat_d = t(kp), t(vis), t(boxes), t(heat)
    P, K = kp.shape[1:3]
    hh, hw = heat.shape[-2:] if heat is not None else (0, 0)
    L = len(st.limbs)
    ints = c_int * n
    with torch.cuda.device(DEV):
        rc = lib.kpd_draw_poses(
            (c_void_p * n)(*[d.data_ptr() for d in dev_imgs]), ints(*[d.shape[0] for d in dev_imgs]),
            ints(*[d.shape[1] for d in dev_imgs]), ints(*[d.stride(0) for d in dev_imgs]), n, _native._ptr(kp_d),
            _native._ptr(vis_d), _native._ptr(box_d), _native._ptr(heat_d), P, K, hh, hw,
            (c_int * max(2 * L, 1))(*[v for ab in st.limbs for v in ab]), L,
            (u8 * max(3 * L, 1))(*[v for c in st.limb_colors for v in c]), (u8 * 9)(*[v for c in st.joint_colors for v in c]),
            (u8 * 3)(*st.box_color), st.joint_radius, st.limb_half_width, st.box_half_width, st.alpha, st.heat_alpha,
            st.min_class, flags, _native._stream(DEV))
    _native.check(rc, "kpd_draw_poses")
    torch.cuda.synchronize()


def _gpu(imgs, kp, vis, boxes, heat, st, flags):
    dev = [torch.from_numpy(i.copy()).to(DEV) for i in imgs]
    _native_draw(dev, kp, vis, boxes, heat, st, flags)
    return [d.cpu().numpy() for d in dev]


def _check(imgs, kp, vis, boxes, heat, st, flags):
    got = _gpu(imgs, kp, vis, boxes, heat, st, flags)
    want = R.draw_ref(imgs, kp, vis, boxes, heat, st, flags)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (i, int((g != w).any(-1).sum()))
    assert any((w != i).any() for w, i in zip(want, imgs))      # something was drawn
    return got


@gpu
def test_gpu_hand_mask():
    st = R.Style(joint_radius=32, alpha=256, joint_colors=((1, 2, 3), (4, 5, 6), (200, 100, 50)))
    kp, vis = np.full((1, 1, 1, 2), 0.5, np.float32), _onehot([[[2]]])
    got = _check([np.zeros((16, 16, 3), np.uint8)], kp, vis, None, None, st, R.JOINTS)[0]
    assert int((got != 0).any(-1).sum()) == 12 and (got[7, 7] == (200, 100, 50)).all() and not got[6, 6].any()


@gpu
@pytest.mark.parametrize("x0", [11, 12])     # rows at 1 mod 4 (byte stores only) and at 0 mod 4 (dword stores)
def test_gpu_pitched_view_in_place(x0):
    """A 53 x 37 column slice of a wider tensor, three persons with an all-zero box between, all layers:
    the view equals the restatement, the parent's other bytes are untouched."""
    rng = np.random.default_rng(11)
    imgs, kp, vis, boxes, heat = _case(rng, [(53, 37)], 3)
    boxes[0, 1] = 0
    parent = torch.from_numpy(rng.integers(0, 256, (53, 64, 3), dtype=np.uint8)).to(DEV)
    before = parent.cpu().numpy().copy()
    view = parent[:, x0:x0 + 37]
    view.copy_(torch.from_numpy(imgs[0]).to(DEV))
    assert view.stride(0) == 192 and view.data_ptr() % 4 == (3 * x0) % 4
    st = _style(rng)
    _native_draw([view], kp, vis, boxes, heat, st, R.ALL)
    after = parent.cpu().numpy()
    want = R.draw_ref(imgs, kp, vis, boxes, heat, st, R.ALL)[0]
    assert np.array_equal(after[:, x0:x0 + 37], want) and (want != imgs[0]).any()
    assert np.array_equal(after[:, :x0], before[:, :x0]) and np.array_equal(after[:, x0 + 37:], before[:, x0 + 37:])


@gpu
def test_gpu_tile_seams():
    from dll import _native
    tw, th = _native.DRAW_TILE_W, _native.DRAW_TILE_H
    rng = np.random.default_rng(12)
    H, W = 3 * th + 7, 3 * tw + 21
    imgs, kp, vis, boxes, heat = _case(rng, [(H, W)], 3)
    kp[0, 0, :2] = [[0.01, 0.02], [0.99, 0.97]]        # limb (0, 1): corner to corner, across every seam
    kp[0, 0, 2:4] = [[0.98, 0.03], [0.02, 0.99]]
    boxes[0, 0] = [0.5, 0.5, 0.96, 0.9]                 # outline and heat over every tile
    _check(imgs, kp, vis, boxes, heat, _style(rng, joint_radius=200, limb_half_width=60), R.ALL)


@gpu
def test_gpu_crowded_tile_keeps_order():
    """40 persons x (19 limbs + 17 joints) inside one 8 x 8 pixel region at alpha 128: over a thousand
    records on one tile, consumed in blocks of 256 -- any reordering changes the blend."""
    rng = np.random.default_rng(13)
    H, W = 40, 72
    imgs, kp, vis, _, _ = _case(rng, [(H, W)], 40)
    kp[..., 0] = rng.uniform(20 / W, 28 / W, kp.shape[:-1])
    kp[..., 1] = rng.uniform(10 / H, 18 / H, kp.shape[:-1])
    st = _style(rng, alpha=128, joint_radius=24, limb_half_width=12,
                joint_colors=((255, 0, 0), (0, 255, 0), (0, 0, 255)))
    got = _check(imgs, kp, vis, None, None, st, R.LIMBS | R.JOINTS)[0]
    # order matters here: the same primitives blended person-reversed differ
    rev = R.draw_ref(imgs, kp[:, ::-1], vis[:, ::-1], None, None, st, R.LIMBS | R.JOINTS)[0]
    assert (rev != got).any()


@gpu
@pytest.mark.parametrize("r16", [40, 0])
def test_gpu_degenerate_inputs(r16):
    rng = np.random.default_rng(14)
    limbs = ((0, 1), (1, 2), (2, 3))
    imgs, kp, vis, boxes, heat = _case(rng, [(32, 48)], 7, K=4)
    vis[:] = _onehot(2)
    kp[0, 0, :2] = [[-50.0, -30.0], [60.0, 40.0]]      # endpoints far outside (clamped to +-2^20 subpixels)
    kp[0, 0, 2] = [3e38, 0.5]                            # the product overflows fp32: clamped, not removed
    kp[0, 1, 1] = kp[0, 1, 0]                            # a zero-length limb
    kp[0, 2, 1] = [np.nan, 0.4]                          # removes joint 1 and limbs (0, 1), (1, 2)
    kp[0, 2, 3] = [0.3, np.inf]
    boxes[0, 3] = [0.9, 0.5, 0.6, 0.7]                   # half outside the image
    boxes[0, 4] = [0.5, 0.5, 1e-6, 0.4]                  # quantises to zero width: no outline, no heat
    boxes[0, 5] = [0.5, np.nan, 0.2, 0.2]                # non-finite: no outline, no heat, person drawn
    vis[0, 6, 1] = _onehot(0)                            # class 0 under min_class 1
    st = _style(rng, limbs=limbs, min_class=1, joint_radius=r16)
    _check(imgs, kp, vis, boxes, heat, st, R.ALL)


@gpu
def test_gpu_chunk_plus_one_images():
    from dll import _native
    rng = np.random.default_rng(15)
    n = _native.DRAW_CHUNK + 1
    sizes = [(int(rng.integers(24, 41)), int(rng.integers(20, 51))) for _ in range(n)]
    sizes[0], sizes[-1] = (24, 20), (40, 50)
    imgs, kp, vis, boxes, heat = _case(rng, sizes, 2)
    st = _style(rng)
    got = _check(imgs, kp, vis, boxes, heat, st, R.ALL)
    for i in range(n):
        one = _gpu(imgs[i:i + 1], kp[i:i + 1], vis[i:i + 1], boxes[i:i + 1], heat[i:i + 1], st, R.ALL)[0]
        assert np.array_equal(one, got[i]), i


@gpu
@pytest.mark.parametrize("hh, hw, flags", [(56, 56, R.HEAT), (56, 56, R.ALL), (8, 5, R.HEAT)])
def test_gpu_heat(hh, hw, flags):
    rng = np.random.default_rng(16)
    imgs, kp, vis, boxes, heat = _case(rng, [(70, 90), (33, 41)], 2, hh=hh, hw=hw)
    heat[0, 0, 3, 2, 1], heat[0, 0, :, 1, 1], heat[1, 1, 0, 0, 0] = np.nan, np.nan, np.inf
    _check(imgs, kp, vis, boxes, heat, _style(rng), flags)


@gpu
def test_gpu_wrapper_compacts_boxes_and_takes_any_image():
    """draw_poses: all-zero caller boxes leave the person slots as in the forward, detector slots with score
    0 get zero boxes; PIL / gray / host inputs are copied, inplace=True draws into the caller's tensor."""
    from PIL import Image
    from dll.utils import DrawStyle, draw_poses
    rng = np.random.default_rng(17)
    imgs, kp, vis, boxes, heat = _case(rng, [(40, 56), (31, 45)], 3)
    boxes[0, 1] = 0
    compact = boxes.copy()
    compact[0] = [boxes[0, 0], boxes[0, 2], [0, 0, 0, 0]]
    ds = DrawStyle()
    st = R.style_of(ds)
    out = {"keypoints": torch.from_numpy(kp[:, :, None]).to(DEV), "visibilities": torch.from_numpy(vis[:, :, None]).to(DEV),
           "heatmap": torch.from_numpy(heat).to(DEV), "boxes": [torch.from_numpy(b).to(DEV) for b in boxes]}
    layers = ("heat", "boxes", "limbs", "joints")
    got = draw_poses([Image.fromarray(imgs[0]), torch.from_numpy(imgs[1])], out, style=ds, layers=layers)
    want = R.draw_ref(imgs, kp, vis, compact, heat, st, R.ALL)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    # detector outputs keep their slots; a zero score removes the person
    scores = np.array([[0.9, 0.0, 0.5], [0.7, 0.6, 0.0]], np.float32)
    masked = boxes * (scores[..., None] > 0)
    det = dict(out, boxes=[torch.from_numpy(b).to(DEV) for b in boxes], box_scores=torch.from_numpy(scores).to(DEV))
    dev_imgs = [torch.from_numpy(i.copy()).to(DEV) for i in imgs]
    back = draw_poses(dev_imgs, det, style=ds, inplace=True)
    want = R.draw_ref(imgs, kp, vis, masked, None, st, R.BOXES | R.LIMBS | R.JOINTS)
    assert all(b is d for b, d in zip(back, dev_imgs))
    assert all(np.array_equal(d.cpu().numpy(), w) for d, w in zip(dev_imgs, want))
    # a gray image is replicated to RGB; the caller's tensor is left alone without inplace
    gray = torch.from_numpy(imgs[0][..., 0].copy()).to(DEV)
    g3 = draw_poses([gray], {k: (v[:1] if isinstance(v, torch.Tensor) else v[:1]) for k, v in out.items()}, style=ds)[0]
    want = R.draw_ref([np.repeat(imgs[0][..., :1], 3, -1)], kp[:1], vis[:1], compact[:1], None, st,
                      R.BOXES | R.LIMBS | R.JOINTS)[0]
    assert np.array_equal(g3.cpu().numpy(), want) and np.array_equal(gray.cpu().numpy(), imgs[0][..., 0])
