"""kpd_preprocess_batch / preprocess_batch / ITransform.batch: n images in one
native call, image i bit for bit what the single-image call and the numpy
oracle (oracle/preprocess_oracle.py) give for it alone.

CPU part: the symbol is declared, bound and exported, and every argument
check answers KPD_EINVAL before any device work (the pointers handed in are
not device memory).  GPU part: one mixed batch through both pipelines and the
n = 1, single-plane and chunk-boundary cases, all np.array_equal."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import preprocess_oracle as O

FLAG_GRAY, FLAG_CLAHE, FLAG_BLUR, FLAG_EDGES = 1, 2, 4, 8


# ------------------------------------------------------------------ CPU: ABI and argument checks
def test_batch_symbol_declared_bound_exported():
    from dll import _native
    assert "kpd_preprocess_batch" in _native.EXPORTS
    hdr = (ROOT / "include" / "kpd.h").read_text()
    assert "int kpd_preprocess_batch(" in hdr and f"#define KPD_PRE_BATCH_CHUNK {_native.PRE_BATCH_CHUNK}" in hdr
    lib = _native.load()
    assert lib.kpd_preprocess_batch.argtypes is not None and lib.kpd_preprocess_batch.restype is ctypes.c_int


def _call(n=2, hs=(40, 30), ws=(50, 20), pitches=None, C=3, flags=FLAG_GRAY | FLAG_CLAHE | FLAG_EDGES, tiles=(8, 8),
          null=None):
    """kpd_preprocess_batch on made-up addresses: only the argument checks may run."""
    from dll import _native
    lib = _native.load()
    k = max(len(hs), 1)
    pitches = pitches if pitches is not None else [w * C for w in ws]
    args = {"srcs": (ctypes.c_void_p * k)(*[0x10000 * (i + 1) for i in range(len(hs))]),
            "hs": (ctypes.c_int * k)(*hs), "ws": (ctypes.c_int * k)(*ws), "ps": (ctypes.c_int * k)(*pitches)}
    if null:
        args[null] = None
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    rc = lib.kpd_preprocess_batch(args["srcs"], args["hs"], args["ws"], args["ps"], n, C, flags, ctypes.c_float(2.0),
                                  tiles[0], tiles[1], 32, 32, mean, std, ctypes.c_void_p(0x900000), None)
    return rc, lib.kpd_last_error().decode()


def test_batch_argument_checks_before_device_work():
    rc, msg = _call(n=0)
    assert rc == -1 and "n must be positive" in msg
    for null in ("srcs", "hs", "ws", "ps"):
        rc, msg = _call(null=null)
        assert rc == -1 and "null" in msg, null
    rc, msg = _call(C=2, flags=0)
    assert rc == -1 and "kpd_preprocess_batch" in msg
    rc, msg = _call(C=3, flags=FLAG_CLAHE | FLAG_EDGES)            # EDGES on 3 channels without GRAY
    assert rc == -1 and "EDGES" in msg
    rc, msg = _call(pitches=[150, 59])                             # image 1: 20 px * 3 channels = 60 > 59
    assert rc == -1 and "image 1" in msg and "pitch" in msg
    rc, msg = _call(hs=(40, 30), ws=(50, 7))                       # an 8 x 8 tile grid on a 7-pixel-wide image 1
    assert rc == -1 and "image 1" in msg and "CLAHE" in msg
    rc, msg = _call(hs=(40, 32 * 40), ws=(50, 20), flags=FLAG_GRAY)   # the downscale limit is per image
    assert rc == -1 and "image 1" in msg and "downscale" in msg


def test_batch_python_api_importable():
    from dll.data import ITransform
    from dll.data.transforms import preprocess_batch
    t = ITransform(img_size=(64, 48), clip_limit=2.0, tile_size=(8, 8), grayscale=True, device="cpu")
    assert callable(t.batch) and callable(preprocess_batch)
    with pytest.raises(TypeError):
        preprocess_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], (8, 8), [0.5], [0.5], FLAG_GRAY)   # a CPU tensor
    with pytest.raises(ValueError):
        preprocess_batch([], (8, 8), [0.5], [0.5])


# ------------------------------------------------------------------ images (structured edge content, not noise)
def _edge_image(rng, h, w):
    """The structure of test_preprocess._edge_image: a vertical step, a disc and stripes over low noise."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = rng.integers(0, 50, (h, w, 3))
    shape = ((xx > w * 0.45) * 120 + (((yy - h / 2) ** 2 + (xx - w / 3) ** 2) < (min(h, w) / 4) ** 2) * 70
             + ((yy // 9) % 2) * (xx > w * 0.7) * 40)
    return ((base + shape[..., None]) % 256).astype(np.uint8)


def _seam_image(rng, h, w):
    """Bars every 16 pixels in both directions: edges on and across every seam
    of the fused post-Canny kernel's 32 x 16 tiles."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = 40 + ((xx % 16) < 3) * 110 + ((yy % 16) < 2) * 80 + rng.integers(0, 6, (h, w))
    return np.repeat(a[..., None], 3, 2).clip(0, 255).astype(np.uint8)


def _snake_image(h=64, w=80):
    """A comb-shaped boundary of weak contrast (Canny candidates, gradient
    between the thresholds) whose only seeds sit at its left end, where the
    step is made strong: the hysteresis needs >= 60 flood levels to reach the
    far end (checked in test_fixture_images_have_the_intended_edges)."""
    rng = np.random.default_rng(21)
    a = np.full((h, w), 90, np.int64)
    a[:10, :] += 55
    for x0 in range(6, w - 6, 16):
        a[10:h - 8, x0:x0 + 8] += 55
    a[10:18, :5] -= 70
    a += rng.integers(0, 3, (h, w))
    return np.repeat(a[..., None], 3, 2).clip(0, 255).astype(np.uint8)


def _border_image(h=56, w=72):
    """Bright lines along row 0 and along the last column, and two bars that
    run into all four borders.  (The ridge of a border line lands two pixels
    inside: with the replicated-border Sobel the gradient on row 0 is
    one-sided and loses the non-maximum suppression, so its dilation is what
    reaches the border; the bars put Canny pixels on the four borders
    themselves.)"""
    rng = np.random.default_rng(22)
    a = np.full((h, w), 40, np.int64)
    a[:, w // 3:w // 3 + 4] = 230
    a[h // 2:h // 2 + 4, :] = 230
    a[0, :] = 230
    a[:, w - 1] = 230
    a += rng.integers(0, 4, (h, w))
    return np.repeat(a[..., None], 3, 2).clip(0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _mixed():
    """The mixed batch (name, uint8 HWC image).  Order matters: the snake sits
    next to the flat image, which has no seeds at all."""
    rng = np.random.default_rng(13)
    return (("ragged 97x83", _edge_image(rng, 97, 83)),
            ("seams 120x160", _seam_image(rng, 120, 160)),
            ("snake 64x80", _snake_image()),
            ("flat 40x50", np.full((40, 50, 3), 90, np.uint8)),
            ("upscaled 33x47", _edge_image(rng, 33, 47)),
            ("border 56x72", _border_image()))


@functools.lru_cache(maxsize=None)
def _gray_u8(i, clip):
    """Oracle: image i after gray -> CLAHE -> edge blend, before the resize (computed once, shared)."""
    a = O.edge_blend_u8(O.clahe_u8(O.rgb_to_gray_cv(_mixed()[i][1]), clip, 8, 8))
    a.setflags(write=False)
    return a


def _canny_maps(img, clip):
    d = O.median5_u8(O.gaussian_blur_u8(O.clahe_u8(O.rgb_to_gray_cv(img), clip, 8, 8), 5, 1.5))
    return O.canny_u8(d, 100, 200), O.canny_u8(d, 200, 200)      # final edges; the seeds alone (low = high)


def test_fixture_images_have_the_intended_edges():
    """No device: the oracle's Canny on the fixture images shows what each is in the batch for."""
    imgs = dict(_mixed())
    for clip in (1.5, 2.0):
        edges, seeds = _canny_maps(imgs["snake 64x80"], clip)
        sy, sx = np.nonzero(seeds)
        ey, ex = np.nonzero(edges)
        assert 0 < len(sy) and sx.max() <= 8, "the seeds sit at the left end only"
        far = np.min(np.maximum(np.abs(ey[:, None] - sy[None]), np.abs(ex[:, None] - sx[None])), axis=1).max()
        assert far >= 60 and len(ey) > 400, (far, len(ey))        # an 8-connected flood moves one pixel per level
        edges, _ = _canny_maps(imgs["border 56x72"], clip)
        assert edges[0].any() and edges[:, -1].any() and edges[-1].any() and edges[:, 0].any()
        assert (edges[2] > 0).sum() > 30 and (edges[:, -3] > 0).sum() > 20     # the ridges of the border lines
        edges, seeds = _canny_maps(imgs["flat 40x50"], clip)
        assert not edges.any() and not seeds.any()
        edges, _ = _canny_maps(imgs["seams 120x160"], clip)
        assert edges[:, 30:34].any() and edges[14:18].any()        # across a vertical and a horizontal tile seam


# ------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAY_FLAGS = FLAG_GRAY | FLAG_CLAHE | FLAG_EDGES


def _device_images(pitched=0):
    """The mixed batch on the device; image `pitched` as a column slice of a
    wider tensor (rows dense, pitch > W * C): preprocess_batch documents that
    such a view is read in place."""
    out = []
    for i, (_, img) in enumerate(_mixed()):
        if i == pitched:
            h, w, _ = img.shape
            wide = torch.full((h, w + 13, 3), 201, dtype=torch.uint8, device=DEV)
            wide[:, 5:5 + w] = torch.from_numpy(img).to(DEV)
            view = wide[:, 5:5 + w]
            assert not view.is_contiguous() and view.stride(0) == (w + 13) * 3
            out.append(view)
        else:
            out.append(torch.from_numpy(img).to(DEV))
    return out


@gpu
@pytest.mark.parametrize("size", [(96, 96), (64, 48)])
def test_gpu_mixed_batch_gray(size):
    from dll.data.transforms import preprocess, preprocess_batch
    clip = 1.5
    imgs = _device_images(pitched=0)
    got = preprocess_batch(imgs, size, (0.5,), (0.5,), GRAY_FLAGS, clip, (8, 8))
    assert got.shape == (len(imgs), 1, *size) and got.is_contiguous()
    got = got.cpu().numpy()
    for i, (name, _) in enumerate(_mixed()):
        want = O.to_tensor_normalize(O.pil_resize_bilinear(_gray_u8(i, clip), *size), [0.5], [0.5])
        assert np.array_equal(got[i], want), f"{name}: batch vs oracle"
        single = preprocess(imgs[i], size, (0.5,), (0.5,), GRAY_FLAGS, clip, (8, 8)).cpu().numpy()
        assert np.array_equal(got[i], single), f"{name}: batch vs single-image call"
    # the flat image has no edges (its maximum stays 0, no neighbour's maximum leaks in): 0.7 * its CLAHE level
    level = int(O.clahe_u8(np.full((40, 50), 90, np.uint8), clip, 8, 8)[0, 0])
    flat = O.to_tensor_normalize(O.add_weighted_u8(np.array([[level]], np.uint8), 0.7, np.zeros((1, 1), np.uint8), 0.3),
                                 [0.5], [0.5])[0, 0, 0]
    assert (got[3] == flat).all()


@gpu
def test_gpu_mixed_batch_rgb():
    from dll.data.transforms import IMAGENET_MEAN, IMAGENET_STD, preprocess, preprocess_batch
    imgs = _device_images(pitched=4)
    flags = FLAG_CLAHE | FLAG_BLUR
    got = preprocess_batch(imgs, (64, 64), IMAGENET_MEAN, IMAGENET_STD, flags, 2.0, (8, 8)).cpu().numpy()
    assert got.shape == (len(imgs), 3, 64, 64)
    for i, (name, img) in enumerate(_mixed()):
        assert np.array_equal(got[i], O.itransform_rgb(img, 64, 2.0, (8, 8))), f"{name}: batch vs oracle"
        single = preprocess(imgs[i], (64, 64), IMAGENET_MEAN, IMAGENET_STD, flags, 2.0, (8, 8)).cpu().numpy()
        assert np.array_equal(got[i], single), f"{name}: batch vs single-image call"


@gpu
def test_gpu_itransform_batch_equals_call():
    """ITransform.batch on PIL images, arrays and tensors: [i] equals __call__ on x_i and the oracle."""
    from PIL import Image
    from dll.data import ITransform
    names = [n for n, _ in _mixed()]
    raw = [img for _, img in _mixed()]
    mixed_types = [Image.fromarray(raw[0]), raw[1], torch.from_numpy(raw[2]), Image.fromarray(raw[3]), raw[4],
                   _device_images(pitched=5)[5]]
    t = ITransform(img_size=(64, 48), clip_limit=2.0, tile_size=(8, 8), grayscale=True, device=DEV)
    got = t.batch(mixed_types)
    assert got.shape == (6, 1, 64, 48)
    for i, x in enumerate(mixed_types):
        assert torch.equal(got[i], t(x)), names[i]
        want = O.to_tensor_normalize(O.pil_resize_bilinear(_gray_u8(i, 2.0), 64, 48), [0.5], [0.5])
        assert np.array_equal(got[i].cpu().numpy(), want), names[i]
    t = ITransform(img_size=64, clip_limit=2.0, tile_size=(8, 8), grayscale=False, device=DEV)
    got = t.batch(mixed_types[:2])
    for i in range(2):
        assert torch.equal(got[i], t(mixed_types[i])), names[i]


@gpu
def test_gpu_single_plane_edges_only_and_n1():
    """[H, W] input with EDGES alone (no gray conversion, no CLAHE), one of
    them a pitched view; and a batch of one image."""
    from dll.data.transforms import preprocess, preprocess_batch
    planes = [np.ascontiguousarray(img[..., 1]) for _, img in _mixed()[:3]]
    dev = [torch.from_numpy(p).to(DEV) for p in planes]
    wide = torch.zeros(planes[1].shape[0], planes[1].shape[1] + 7, dtype=torch.uint8, device=DEV)
    wide[:, 3:3 + planes[1].shape[1]] = dev[1]
    dev[1] = wide[:, 3:3 + planes[1].shape[1]]
    got = preprocess_batch(dev, (48, 40), (0.0,), (1.0,), FLAG_EDGES).cpu().numpy()
    for i, p in enumerate(planes):
        want = O.to_tensor_normalize(O.pil_resize_bilinear(O.edge_blend_u8(p), 48, 40), [0.0], [1.0])
        assert np.array_equal(got[i], want), i
        assert np.array_equal(got[i], preprocess(dev[i], (48, 40), (0.0,), (1.0,), FLAG_EDGES).cpu().numpy()), i
    name, img = _mixed()[0]
    one = preprocess_batch([torch.from_numpy(img).to(DEV)], (96, 96), (0.5,), (0.5,), GRAY_FLAGS, 1.5, (8, 8))
    assert one.shape == (1, 1, 96, 96)
    want = O.to_tensor_normalize(O.pil_resize_bilinear(_gray_u8(0, 1.5), 96, 96), [0.5], [0.5])
    assert np.array_equal(one[0].cpu().numpy(), want)


@gpu
def test_gpu_one_more_than_a_chunk():
    """n = KPD_PRE_BATCH_CHUNK + 1 images of 24x20 .. 40x50: the second
    descriptor table holds one image; offsets and counters carry across chunks."""
    from dll import _native
    from dll.data.transforms import preprocess, preprocess_batch
    n = _native.PRE_BATCH_CHUNK + 1
    rng = np.random.default_rng(29)
    imgs = [_edge_image(rng, 24 + (i * 5) % 17, 20 + (i * 7) % 31) for i in range(n)]
    assert max(a.shape[0] for a in imgs) == 40 and max(a.shape[1] for a in imgs) == 50
    dev = [torch.from_numpy(a).to(DEV) for a in imgs]
    got = preprocess_batch(dev, (32, 32), (0.5,), (0.5,), GRAY_FLAGS, 1.5, (8, 8)).cpu().numpy()
    assert got.shape == (n, 1, 32, 32)
    for i, a in enumerate(imgs):
        assert np.array_equal(got[i], O.itransform_gray(a, 32, 1.5, (8, 8))), f"image {i} vs oracle"
        single = preprocess(dev[i], (32, 32), (0.5,), (0.5,), GRAY_FLAGS, 1.5, (8, 8)).cpu().numpy()
        assert np.array_equal(got[i], single), f"image {i} vs single-image call"
