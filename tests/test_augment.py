"""kpd_augment_batch (csrc/augment.hip) and dll.data.augmentation against the
numpy restatement tests/augment_ref.py.

Images are integer arithmetic: compared bit for bit.  Label coordinates and
boxes are the same float64 expressions on both sides, differing at most by
contraction; the fp32 store of a value below 1 can then differ by one ulp, at
most 6e-8, and the tolerance is twice that: 1.2e-7.  Visibility, zeroed rows
and zeroed joints are compared exactly; the seeded cases are checked (here, on
the CPU) to keep every transformed joint and every box edge 1e-4 clear of the
borders of [0, 1).
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import ROOT

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
TOL = 1.2e-7
COCO = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
CHUNK = 16   # KPD_AUG_CHUNK (asserted against the header and the binding below)


# ------------------------------------------------------------------ cases
def _labels(rng, n, P, K):
    kp = rng.uniform(0.3, 0.7, (n, P, K, 2)).astype(f32)
    vis = rng.integers(1, 3, (n, P, K)).astype(f32)
    box = np.concatenate([rng.uniform(0.4, 0.6, (n, P, 2)), rng.uniform(0.1, 0.3, (n, P, 2))], -1).astype(f32)
    return kp, vis, box


def _params(n, mirror=0, angle=0.0, scale=1.0, gain=256, offset=0):
    from dll.data import AugmentParams
    b = lambda v, t: np.broadcast_to(np.asarray(v, t), (n,)).copy()   # noqa: E731
    return AugmentParams(b(mirror, bool), b(angle, float), b(scale, float), b(gain, np.int32), b(offset, np.int32))


@functools.lru_cache(maxsize=None)
def _case(name):
    """images (list of uint8 arrays), params, fill, pairs, labels (kp, vis, box) or None"""
    rng = np.random.default_rng({"tiny": 1, "unit": 2, "mixed": 3, "tiles": 4, "chunk": 5, "long": 6, "klimit": 7,
                                 "longer": 8}[name])
    img = lambda h, w, c: rng.integers(0, 256, (h, w, c) if c > 1 else (h, w), dtype=np.uint8)   # noqa: E731
    fill, pairs, lab = 0, None, None
    if name == "tiny":      # less than one wave; odd width
        imgs, par = [img(5, 7, 1)], _params(1, mirror=1)
        lab, pairs = _labels(rng, 1, 1, 3), [0, 2, 1]
    elif name == "unit":    # every tap but the centre is fill
        imgs, par, fill = [img(1, 1, 3)], _params(1, angle=30.0, scale=0.8), (9, 90, 200)
        lab = _labels(rng, 1, 2, 17)
    elif name == "mixed":
        wide = img(33, 80, 3)
        imgs = [wide[:, 5:70], img(17, 130, 3), img(64, 64, 3)]   # image 0: a column slice, pitch 240 > 195
        par = _params(3, mirror=[1, 0, 0], angle=[10.0, 0.0, -25.0], scale=[1.3, 1.0, 0.85], gain=[256, 256, 200],
                      offset=[0, 0, 1500])
        fill = (30, 60, 90)
        kp, vis, box = _labels(rng, 3, 3, 17)
        kp[0, 0], vis[0, 0], box[0, 0] = 0, 0, 0                  # a zero-box padding person
        kp[0, 1, 3:9], vis[0, 1, 3:9] = 0, 0                      # a person with (0, 0, 0) joints
        kp[0, 1, 12] = 0                                          # ... and one at the origin with v set
        box[0, 2] = [0.98, 0.03, 0.02, 0.04]                      # mapped past the left edge: clipping empties it
        kp[0, 2, :4] = [[0.02, 0.02], [0.97, 0.5], [0.5, 0.99], [0.01, 0.98]]   # ... and joints that leave the frame
        lab = (kp, vis, box)
    elif name == "tiles":   # one past the 64 x 16 tile's edge in both directions
        imgs, par, fill = [img(65, 129, 3)], _params(1, angle=-15.0, scale=1.2, gain=300, offset=-2000), (114,) * 3
        lab = _labels(rng, 1, 2, 17)
    elif name == "chunk":   # crosses a descriptor-table boundary
        n = CHUNK + 1
        imgs, par = [img(8, 8, 1) for _ in range(n)], _params(n, mirror=[i % 2 for i in range(n)])
        lab, pairs = _labels(rng, n, 1, 2), [1, 0]
    elif name == "long":    # q00 * x reaches 2^31 - 2^17: the largest sums that still fit 32 bits
        imgs, par = [img(2, 16384, 1)], _params(1, scale=0.5)
    elif name == "longer":  # sx reaches 2.7e9 > 2^31: fails with 32-bit coordinate sums
        imgs, par = [img(2, 16384, 1)], _params(1, scale=0.25)
    elif name == "klimit":  # K at its limit, every joint swapped
        imgs, par = [img(8, 8, 1)], _params(1, mirror=1)
        lab, pairs = _labels(rng, 1, 1, 32), list(range(31, -1, -1))
    hs, ws = [i.shape[0] for i in imgs], [i.shape[1] for i in imgs]
    q, N = par.matrices(ws, hs)
    f3 = (fill,) * 3 if np.isscalar(fill) else fill
    ref_imgs = [R.warp(im, q[i], f3, par.gain[i], par.offset[i]) for i, im in enumerate(imgs)]
    ref_lab, margin = None, np.inf
    if lab is not None:
        pr = COCO if pairs is None else pairs
        per = [R.labels(lab[0][i], lab[1][i], lab[2][i], N[i], par.mirror[i], pr) for i in range(len(imgs))]
        ref_lab = tuple(np.stack([p[j] for p in per]) for j in range(3))
        margin = min(R.label_margin(lab[0][i], lab[1][i], lab[2][i], N[i], par.mirror[i], pr)
                     for i in range(len(imgs)))
    for a in (*imgs, *ref_imgs, *(lab or ()), *(ref_lab or ())):
        a.setflags(write=False)
    return imgs, par, fill, pairs, lab, ref_imgs, ref_lab, margin, (q, N)


CASES = ["tiny", "unit", "mixed", "tiles", "chunk", "long", "longer", "klimit"]


# ------------------------------------------------------------------ CPU
def test_symbol_is_declared_bound_and_exported():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    assert re.search(r"\bint kpd_augment_batch\s*\(", hdr)
    assert "kpd_augment_batch" in _native.EXPORTS
    lib = _native.load()
    assert lib.kpd_augment_batch.restype is ctypes.c_int and len(lib.kpd_augment_batch.argtypes) == 23
    assert (_native.AUG_CHUNK, _native.AUG_TILE_W, _native.AUG_TILE_H, _native.AUG_MAX_SIDE, _native.AUG_MAX_K) == \
        (CHUNK, 64, 16, 16384, 32)
    for line in ("#define KPD_AUG_CHUNK 16", "#define KPD_AUG_TILE_W 64", "#define KPD_AUG_TILE_H 16",
                 "#define KPD_AUG_MAX_SIDE 16384", "#define KPD_AUG_MAX_K 32"):
        assert line in hdr, line


def _raw_call(lib, n=1, C=1, H=8, W=8, pitch=None, q=None, gain=256, offset=0, pairs=(0, 2, 1), P=1, K=3,
              labels=True, src=0x10000, dst=0x20000, stream=None):
    """One raw call whose device pointers are never dereferenced: the checks under test fail first."""
    ints = ctypes.c_int * max(n, 1)
    vp = ctypes.c_void_p * max(n, 1)
    q = (65536, 0, 0, 0, 65536, 0) if q is None else q
    lab = [ctypes.c_void_p(0x30000 + 0x1000 * i) if labels else None for i in range(6)]
    return lib.kpd_augment_batch(
        vp(*[src] * max(n, 1)), ints(*[H] * max(n, 1)), ints(*[W] * max(n, 1)),
        ints(*[W * C if pitch is None else pitch] * max(n, 1)), vp(*[dst] * max(n, 1)), n, C,
        (ctypes.c_int32 * (6 * max(n, 1)))(*list(q) * max(n, 1)),
        (ctypes.c_double * (6 * max(n, 1)))(*[1, 0, 0, 0, 1, 0] * max(n, 1)), ints(*[0] * max(n, 1)),
        (ctypes.c_int32 * max(n, 1))(*[gain] * max(n, 1)), (ctypes.c_int32 * max(n, 1))(*[offset] * max(n, 1)),
        (ctypes.c_uint8 * 3)(0, 0, 0), None if pairs is None else (ctypes.c_int32 * 33)(*pairs),
        lab[0], lab[1], lab[2], P, K, lab[3], lab[4], lab[5], stream)


def test_scalar_argument_checks_need_no_device():
    """The checks run before any device work and name the offending argument."""
    from dll import _native
    lib = _native.load()
    big = 1 << 19
    for kw, word in ((dict(C=2), b"channels"), (dict(H=0), b"image 0: sides"), (dict(W=16385), b"image 0: sides"),
                     (dict(K=0), b"K"), (dict(K=33, pairs=tuple(range(33))), b"K"), (dict(P=0), b"P"),
                     (dict(pairs=(1, 2, 0)), b"pairs"), (dict(pairs=(0, 3, 1)), b"pairs"), (dict(pairs=None), b"pairs"),
                     (dict(q=(big, 0, 0, 0, 65536, 0)), b"image 0: q"), (dict(q=(65536, 0, 0, -big, 65536, 0)), b"image 0: q"),
                     (dict(n=-1), b"n"), (dict(gain=65536), b"image 0: gain"), (dict(offset=1 << 24), b"image 0: offset"),
                     (dict(pitch=7), b"image 0: pitch"), (dict(src=0), b"image 0: null source"),
                     (dict(dst=0x10000 + 8), b"image 0: destination overlaps")):
        assert _raw_call(lib, **kw) == -1, kw
        msg = lib.kpd_last_error()
        assert msg.startswith(b"kpd_augment_batch: " + word), (kw, msg)
    assert _raw_call(lib, n=0) == 0
    assert _raw_call(lib, n=0, labels=False, P=0, K=0, pairs=None) == 0
    # P, K and pairs are ignored without labels: the call gets as far as the per-image checks
    assert _raw_call(lib, labels=False, P=0, K=0, pairs=None, H=0) == -1
    assert lib.kpd_last_error().startswith(b"kpd_augment_batch: image 0: sides")
    # the largest translation and coefficients are accepted as far as the checks go
    assert _raw_call(lib, q=(big - 1, 1 - big, 2 ** 31 - 1, 0, 65536, -2 ** 31), gain=65535, offset=1 - (1 << 24),
                     src=0) == -1
    assert lib.kpd_last_error().startswith(b"kpd_augment_batch: image 0: null source")


@pytest.mark.parametrize("shape", [(5, 7, 1), (33, 65, 3)])
def test_ref_identity_is_a_copy_and_a_mirror_is_a_flip(shape):
    H, W, C = shape
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (H, W, C) if C > 1 else (H, W), dtype=np.uint8)
    q, N = R.matrices(W, H)
    assert q.tolist() == [65536, 0, 0, 0, 65536, 0] and N.tolist() == [1, 0, 0, 0, 1, 0]
    assert np.array_equal(R.warp(img, q, (7, 7, 7)), img)
    qm, Nm = R.matrices(W, H, mirror=True)
    assert np.array_equal(R.warp(img, qm, (7, 7, 7)), img[:, ::-1])
    assert Nm.tolist() == [-1, 0, 1, 0, 1, 0]     # x' = 1 - x
    # the package builds the same matrices
    par = _params(2, mirror=[0, 1])
    pq, pN = par.matrices(W, H)
    assert np.array_equal(pq, np.stack([q, qm])) and np.array_equal(pN, np.stack([N, Nm]))
    assert pq.dtype == np.int32 and pN.dtype == np.float64


@pytest.mark.parametrize("mirror,angle,scale", [(0, 15.0, 1.2), (1, -30.0, 0.8), (1, 7.0, 1.0)])
def test_ref_labels_follow_pixels(mirror, angle, scale):
    """A Gaussian dot at a keypoint: the warped image's intensity centroid lies within 0.1 px of N applied to the
    keypoint.  A half-pixel centre-convention error would show as at least 0.4 px."""
    H, W = 96, 128
    kx, ky = 0.5625, 0.40625    # the dot stays inside the frame under all three maps
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    px, py = kx * W - 0.5, ky * H - 0.5
    img = np.rint(255 * np.exp(-((x - px) ** 2 + (y - py) ** 2) / (2 * 3.0 ** 2))).astype(np.uint8)
    q, N = R.matrices(W, H, bool(mirror), angle, scale)
    pq, pN = _params(1, mirror=mirror, angle=angle, scale=scale).matrices(W, H)
    assert np.abs(pq[0].astype(np.int64) - q).max() <= 1 and np.abs(pN[0] - N).max() <= 1e-12
    out = R.warp(img, pq[0]).astype(np.float64)
    assert out.sum() > 1000
    cx, cy = (out * x).sum() / out.sum(), (out * y).sum() / out.sum()
    kp, vis, _ = R.labels(np.array([[[kx, ky]]], f32), np.ones((1, 1), f32), np.zeros((1, 4), f32), pN[0], mirror, [0])
    assert vis[0, 0] == 1
    ex, ey = kp[0, 0, 0] * W - 0.5, kp[0, 0, 1] * H - 0.5
    err = float(np.hypot(cx - ex, cy - ey))
    print("centroid error px", err)
    assert err <= 0.1, err


def test_ref_label_rules():
    """Padding stays padding, a joint that leaves the frame is zeroed, a mirror swaps left and right, a box is
    re-hulled and clipped, and a box clipped empty becomes a zero row while its joints keep their own rule."""
    _, Nm = R.matrices(64, 48, mirror=True)
    kp = np.array([[[0.25, 0.5], [0.125, 0.25], [0, 0]], [[0, 0], [0, 0], [0, 0]]], f32)
    vis = np.array([[2, 1, 2], [0, 0, 0]], f32)
    box = np.array([[0.25, 0.5, 0.25, 0.5], [0, 0, 0, 0]], f32)
    okp, ovis, obox = R.labels(kp, vis, box, Nm, True, [0, 2, 1])
    assert okp[0].tolist() == [[0.75, 0.5], [0, 0], [0.875, 0.25]] and ovis[0].tolist() == [2, 2, 1]
    assert not okp[1].any() and not ovis[1].any() and not obox[1].any()
    assert obox[0].tolist() == [0.75, 0.5, 0.25, 0.5]
    _, Nz = R.matrices(64, 48, scale=2.0)
    kp = np.array([[[0.5, 0.5], [0.875, 0.5], [0.5, 0.125]]], f32)
    okp, ovis, obox = R.labels(kp, np.ones((1, 3), f32), np.array([[0.9375, 0.5, 0.0625, 0.25]], f32), Nz, False, [0, 1, 2])
    assert okp[0].tolist() == [[0.5, 0.5], [0, 0], [0, 0]] and ovis[0].tolist() == [1, 0, 0]
    assert not obox.any()                           # x in [1.3125, 1.4375]: clipped to nothing; joint 0 lives on
    okp, ovis, obox = R.labels(kp, np.ones((1, 3), f32), np.array([[0.75, 0.5, 0.25, 0.25]], f32), Nz, False, [0, 1, 2])
    assert obox[0].tolist() == [0.875, 0.5, 0.25, 0.5]   # x in [0.75, 1.25] -> [0.75, 1]; y in [0.25, 0.75]


def test_seeded_cases_keep_their_margins_and_their_scenarios():
    """A condition on the seeds, not on the kernel."""
    for name in CASES:
        m = _case(name)[7]
        print(name, "margin", m)
        assert m >= 1e-4, (name, m)
    imgs, par, fill, pairs, lab, ref_imgs, ref_lab, _, (q, N) = _case("mixed")
    assert imgs[0].strides[0] == 240 and imgs[0].shape == (33, 65, 3)
    assert np.array_equal(ref_imgs[1], imgs[1])                        # the identity image: a bit-exact copy
    kp, vis, box = ref_lab
    assert not kp[0, 0].any() and not vis[0, 0].any() and not box[0, 0].any()
    # image 0 is mirrored: output joint k comes from source joint COCO[k]
    assert not kp[0, 1, 11].any() and vis[0, 1, 11] == lab[1][0, 1, 12] != 0     # (0, 0) with v set passes through
    assert lab[2][0, 2].any() and not box[0, 2].any()                  # a box that clipping empties ...
    gone = [0, 1, 2, 4]                                                # ... sources 0..3 leave the frame ...
    rest = [k for k in range(17) if k not in gone]
    assert (vis[0, 2, gone] == 0).all() and not kp[0, 2, gone].any()
    assert (vis[0, 2, rest] != 0).all() and kp[0, 2, rest].all()       # ... and the person's other joints live on
    assert box[1].any() and np.array_equal(kp[1], lab[0][1]) and np.array_equal(box[1, 0, :2], lab[2][1, 0, :2])
    unit = _case("unit")
    centre = unit[0][0][0, 0].astype(int)
    got = unit[5][0][0, 0].astype(int)
    assert np.array_equal(got, centre)     # the 1 x 1 image maps its centre to itself, whatever the angle
    lq = _case("longer")[8][0][0].astype(np.int64)
    assert lq[0] * 16383 + lq[2] >= 2 ** 31 > _case("long")[8][0][0, 0].astype(np.int64) * 16383 >= 2 ** 31 - 2 ** 17


def test_sample_is_seeded_gated_and_ranged():
    from dll.configs import AugmentationConfig, TrainingConfig
    from dll.data import AugmentParams, KeypointAugmentation

    def aug(seed=5, **kw):
        cfg = TrainingConfig()
        cfg.augmentation = AugmentationConfig(enabled=True, **kw)
        return KeypointAugmentation(cfg, seed=seed, device="cpu")

    on = {"enabled": True, "brightness": 0.2, "contrast": 0.3}
    a, b = aug(prob=1.0, color=on).sample(64), aug(prob=1.0, color=on).sample(64)
    for f in ("mirror", "angle_deg", "scale", "gain", "offset"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert not np.array_equal(a.angle_deg, aug(seed=6, prob=1.0).sample(64).angle_deg)
    assert a.mirror.all() and (np.abs(a.angle_deg) <= 30).all() and a.angle_deg.std() > 5
    assert ((a.scale >= 0.8) & (a.scale <= 1.2)).all() and a.scale.std() > 0.05
    assert ((a.gain >= round(256 * 0.7)) & (a.gain <= round(256 * 1.3))).all() and a.gain.std() > 5
    assert (np.abs(a.offset) <= round(256 * 255 * 0.2)).all() and a.offset.std() > 1000
    # the documented column use
    u = torch.rand(64, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).numpy()
    assert np.array_equal(a.angle_deg, (2 * u[:, 2] - 1) * 30.0) and np.array_equal(a.scale, 0.8 + u[:, 4] * (1.2 - 0.8))
    assert np.array_equal(a.gain, np.rint(256 * (1 + (2 * u[:, 7] - 1) * 0.3)))
    assert np.array_equal(a.offset, np.rint(256 * 255 * (2 * u[:, 6] - 1) * 0.2))
    half = aug(prob=0.5).sample(64)
    assert np.array_equal(half.mirror, u[:, 0] < 0.5) and np.array_equal(half.angle_deg != 0, u[:, 1] < 0.5)
    assert np.array_equal(half.scale != 1, u[:, 3] < 0.5)
    z, ident = aug(prob=0.0, color=on).sample(16), AugmentParams.identity(16)
    for f in ("mirror", "angle_deg", "scale", "gain", "offset"):
        assert np.array_equal(getattr(z, f), getattr(ident, f)), f
    assert ident.gain.tolist() == [256] * 16 and ident.matrices(7, 5)[0][3].tolist() == [65536, 0, 0, 0, 65536, 0]
    off = aug(prob=1.0, flip={"enabled": False, "horizontal": True}, rotate={"enabled": False, "max_angle": 30.0},
              scale={"enabled": False, "range": [0.8, 1.2]}).sample(16)      # colour is disabled by default
    for f in ("mirror", "angle_deg", "scale", "gain", "offset"):
        assert np.array_equal(getattr(off, f), getattr(ident, f)), f
    assert not aug(prob=1.0, flip={"enabled": True, "horizontal": False}).sample(8).mirror.any()


def test_config_takes_the_reference_yaml_block():
    import yaml

    from dll.configs import AugmentationConfig, TrainingConfig
    block = yaml.safe_load("""
        enabled: false
        prob: 0.5
        flip: {enabled: true, horizontal: true}
        rotate: {enabled: true, max_angle: 15.0}
        scale: {enabled: true, range: [0.8, 1.2]}
    """)
    cfg = AugmentationConfig(**block)
    cfg.validate()
    assert cfg.rotate["max_angle"] == 15.0 and cfg.color["enabled"] is False and cfg.fill == 0
    d = AugmentationConfig()
    assert d.enabled is False and d.flip == {"enabled": True, "horizontal": True}
    assert d.rotate == {"enabled": True, "max_angle": 30.0} and d.scale == {"enabled": True, "range": [0.8, 1.2]}
    assert TrainingConfig().augmentation == d
    shipped = yaml.safe_load((ROOT / "keypoint-detection_amd" / "configs" / "default_config.yaml").read_text())
    AugmentationConfig(**shipped["training"]["augmentation"]).validate()
    for bad in (dict(prob=1.5), dict(rotate={"enabled": True, "max_angle": -1.0}),
                dict(scale={"enabled": True, "range": [0.0, 1.0]}), dict(scale={"enabled": True, "range": [1.2, 0.8]})):
        with pytest.raises(AssertionError):
            AugmentationConfig(**bad).validate()


def test_disabled_augmentation_returns_its_inputs_and_cpu_tensors_raise():
    from dll import _native
    from dll.data import AugmentParams, KeypointAugmentation, augment_batch
    a = KeypointAugmentation(device="cpu")     # the default config: enabled == False
    img, kp, vis, bx = object(), torch.zeros(1, 1, 17, 2), torch.zeros(1, 1, 17), [torch.zeros(1, 4)]
    out = a(img, kp, vis, bx)
    assert out[0] is img and out[1] is kp and out[2] is vis and out[3] is bx
    with pytest.raises(_native.KpdNativeError):
        augment_batch([torch.zeros(4, 4, dtype=torch.uint8)], params=AugmentParams.identity(1))
    with pytest.raises(TypeError):
        augment_batch([torch.zeros(4, 4)], params=AugmentParams.identity(1))
    with pytest.raises(ValueError):
        augment_batch([], params=AugmentParams.identity(1))
    assert augment_batch([], params=AugmentParams.identity(0)) == []


# ------------------------------------------------------------------ GPU
def _gpu(imgs, par, fill, pairs, lab):
    from dll.data import augment_batch
    ts = []
    for im in imgs:
        base = im if im.base is None or im.flags["C_CONTIGUOUS"] else im.base     # keep a slice a slice
        t = torch.from_numpy(np.array(base)).to(DEV)
        ts.append(t if base is im else t[:, 5:70])
    labels = () if lab is None else tuple(torch.from_numpy(np.array(a)).to(DEV) for a in lab)
    out = augment_batch(ts, *labels, params=par, pairs=pairs, fill=fill)
    torch.cuda.synchronize()
    return out


def _compare_labels(got, ref):
    kp, vis, box = (t.cpu().numpy() for t in got)
    rkp, rvis, rbox = ref
    assert kp.dtype == f32 and kp.shape == rkp.shape and vis.shape == rvis.shape and box.shape == rbox.shape
    assert np.array_equal(vis, rvis)
    assert np.array_equal(kp == 0, rkp == 0) and np.array_equal(box == 0, rbox == 0)
    ek = np.abs(kp.astype(np.float64) - rkp).max()
    eb = np.abs(box.astype(np.float64) - rbox).max()
    print("keypoints max|d|", ek, "boxes max|d|", eb)
    assert ek <= TOL and eb <= TOL, (ek, eb)


@gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_matches_the_restatement(name):
    imgs, par, fill, pairs, lab, ref_imgs, ref_lab, margin, _ = _case(name)
    assert margin >= 1e-4
    out = _gpu(imgs, par, fill, pairs, lab)
    outs = out if lab is None else out[0]
    assert len(outs) == len(imgs)
    for i, (o, r) in enumerate(zip(outs, ref_imgs)):
        assert o.dtype == torch.uint8 and tuple(o.shape) == r.shape, i
        assert np.array_equal(o.cpu().numpy(), r), (name, i)
    if lab is not None:
        _compare_labels(out[1:], ref_lab)
    if name == "mixed":
        assert np.array_equal(outs[1].cpu().numpy(), imgs[1])     # identity: a bit-exact copy
        base = outs[0].untyped_storage().data_ptr()
        assert all(o.untyped_storage().data_ptr() == base for o in outs)   # views of one allocation


@gpu
def test_gpu_an_image_does_not_depend_on_its_batch():
    imgs, par, fill, pairs, lab, *_ = _case("mixed")
    both = _gpu(imgs, par, fill, pairs, lab)
    one = _params(1, mirror=par.mirror[1], angle=par.angle_deg[1], scale=par.scale[1], gain=par.gain[1],
                  offset=par.offset[1])
    alone = _gpu(imgs[1:2], one, fill, pairs, tuple(a[1:2] for a in lab))
    assert torch.equal(both[0][1], alone[0][0])
    for b, a in zip(both[1:], alone[1:]):
        assert torch.equal(b[1:2], a)


@gpu
def test_gpu_image_only_call_and_an_empty_batch():
    from dll import _native
    from dll.data import AugmentParams, augment_batch
    imgs, par, fill, _, _, ref_imgs, *_ = _case("tiles")
    outs = _gpu(imgs, par, fill, None, None)
    assert isinstance(outs, list) and np.array_equal(outs[0].cpu().numpy(), ref_imgs[0])
    assert augment_batch([], params=AugmentParams.identity(0)) == []
    assert _raw_call(_native.load(), n=0, stream=_native._stream(DEV)) == 0


@gpu
def test_gpu_overlap_checks():
    from dll import _native
    lib = _native.load()
    a, b = torch.zeros(8, 8, dtype=torch.uint8, device=DEV), torch.zeros(8, 8, dtype=torch.uint8, device=DEV)
    c, d = torch.zeros(8, 8, dtype=torch.uint8, device=DEV), torch.zeros(8, 8, dtype=torch.uint8, device=DEV)
    kp, vis, bx = torch.zeros(2, 1, 3, 2, device=DEV), torch.zeros(2, 1, 3, device=DEV), torch.zeros(2, 1, 4, device=DEV)
    kpo, viso, bxo = torch.zeros_like(kp), torch.ones_like(vis), torch.zeros_like(bx)
    p = _native._ptr

    def call(srcs, dsts, kp_out=kpo, vis_out=viso):
        n = len(srcs)
        ints, vp = ctypes.c_int * n, ctypes.c_void_p * n
        with torch.cuda.device(DEV):
            return lib.kpd_augment_batch(
                vp(*[t.data_ptr() for t in srcs]), ints(*[8] * n), ints(*[8] * n), ints(*[8] * n),
                vp(*[t.data_ptr() for t in dsts]), n, 1, (ctypes.c_int32 * (6 * n))(*[65536, 0, 0, 0, 65536, 0] * n),
                (ctypes.c_double * (6 * n))(*[1, 0, 0, 0, 1, 0] * n), ints(*[0] * n),
                (ctypes.c_int32 * n)(*[256] * n), (ctypes.c_int32 * n)(*[0] * n), (ctypes.c_uint8 * 3)(0, 0, 0),
                (ctypes.c_int32 * 3)(0, 2, 1), p(kp), p(vis), p(bx), 1, 3, p(kp_out), p(vis_out), p(bxo),
                _native._stream(DEV))

    for args, word in ((([a, b], [a, d]), b"image 0: destination overlaps"),        # a destination equal to its source
                       (([a, b], [c, a]), b"image 1: destination overlaps"),        # ... to another image's source
                       (([a, b], [c, d], kp), b"keypoints_out overlaps keypoints"),  # a label output equal to its input
                       (([a, b], [c, d], kpo, kp), b"visibilities_out overlaps keypoints")):
        assert call(*args) == -1, word
        msg = lib.kpd_last_error()
        assert msg.startswith(b"kpd_augment_batch: " + word), msg
    assert call([a, a], [c, d]) == 0        # one source read twice is fine
    torch.cuda.synchronize()
    assert viso.sum() == 0                  # the valid call ran


def _write_dataset(root, split, rng):
    from PIL import Image
    (root / split / "images").mkdir(parents=True)
    (root / split / "labels").mkdir(parents=True)
    imgs = {}
    for name, persons in (("a", 2), ("b", 1)):
        img = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
        Image.fromarray(img).save(root / split / "images" / f"{name}.png")
        rows = []
        for _ in range(persons):
            # coordinates on a 1/256 grid: exact in the label text and in fp32
            kp = rng.integers(64, 192, (17, 2)) / 256.0
            v = rng.integers(1, 3, 17)
            box = [0.5, 0.5, 0.25, 0.5]
            rows.append(" ".join(["0"] + [repr(float(t)) for t in box] +
                                 [f"{float(x)!r} {float(y)!r} {int(c)}" for (x, y), c in zip(kp, v)]))
        (root / split / "labels" / f"{name}.txt").write_text("\n".join(rows) + "\n")
        imgs[name] = img
    return imgs


@gpu
def test_gpu_dataset_wiring(tmp_path):
    from dll.configs import AugmentationConfig, TrainingConfig
    from dll.data import KeypointAugmentation, OptimizedKeypointsDataset, create_optimized_dataloader
    from dll.models.heatmap_head import generate_target_heatmap
    rng = np.random.default_rng(21)
    raw = _write_dataset(tmp_path, "train", rng)
    _write_dataset(tmp_path, "val", np.random.default_rng(21))

    def aug(enabled=True):
        cfg = TrainingConfig()
        cfg.augmentation = AugmentationConfig(enabled=enabled, prob=1.0, rotate={"enabled": False, "max_angle": 30.0},
                                              scale={"enabled": False, "range": [0.8, 1.2]})
        return KeypointAugmentation(cfg, seed=3, device=DEV)

    kw = dict(img_size=64, grayscale=False, device=DEV, enable_caching=False)
    plain = OptimizedKeypointsDataset(str(tmp_path), split="train", **kw)
    ds = OptimizedKeypointsDataset(str(tmp_path), split="train", augmentation=aug(), **kw)     # does not raise
    for i, name in enumerate(("a", "b")):
        s, s0 = ds[i], plain[i]
        want = ds.transform(torch.from_numpy(np.ascontiguousarray(raw[name][:, ::-1])))
        assert torch.equal(s["image"], want) and not torch.equal(s["image"], s0["image"])
        kp0 = s0["keypoints"].to(DEV)
        assert s["keypoints"].is_cuda and s["keypoints"].shape == kp0.shape
        mirrored = torch.stack([1.0 - kp0[..., COCO, 0], kp0[..., COCO, 1]], -1)
        assert float((s["keypoints"] - mirrored).abs().max()) <= TOL
        assert torch.equal(s["visibilities"].cpu(), s0["visibilities"][..., COCO])
        b0 = s0["bboxes"].to(DEV)
        assert float((s["bboxes"] - torch.stack([1 - b0[:, 0], b0[:, 1], b0[:, 2], b0[:, 3]], -1)).abs().max()) <= TOL
        heat = generate_target_heatmap(s["keypoints"], ds.heatmap_size, sigma=3.0)
        assert torch.equal(s["heatmaps"], heat.unsqueeze(0) if heat.dim() == 3 else heat)
        assert not torch.equal(s["heatmaps"], s0["heatmaps"])
    val, val0 = (OptimizedKeypointsDataset(str(tmp_path), split="val", augmentation=a, **kw) for a in (aug(), None))
    off = OptimizedKeypointsDataset(str(tmp_path), split="train", augmentation=aug(enabled=False), **kw)
    for i in range(2):
        for x, y in ((val[i], val0[i]), (off[i], plain[i])):
            for key in ("image", "heatmaps", "keypoints", "visibilities", "bboxes"):
                assert torch.equal(x[key].cpu(), y[key].cpu()), key
    dl = create_optimized_dataloader(str(tmp_path), batch_size=2, num_workers=0, split="train", img_size=64,
                                     grayscale=False, device=DEV, augmentation=aug())
    assert dl.dataset.augmentation is not None
    batch = next(iter(dl))
    assert batch["image"].shape == (2, 3, 64, 64) and batch["keypoints"].is_cuda
