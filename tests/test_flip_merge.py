"""kpd_flip_merge (csrc/flip_merge.hip) and dll.utils.flip against the numpy
restatement tests/flip_ref.py.

The merged map and the peaks are one fp32 add, an exact halving and a maximum:
compared bit for bit.  The visibility classes are compared exactly; the seeded
cases are checked (here, on the CPU) to keep every sigmoid(peak) 1e-4 clear of
the class borders 0.3 / 0.7, far more than the fp32 sigmoid's rounding.  The
keypoints are an fp32 soft-argmax compared with the float64 one of the same
fp32 map within 1e-6, the tolerance tests/test_gpu_api.py pins the model decode
to its golden with; the box transform scales by w, h <= 1, so it does not grow.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import flip_ref as R
from conftest import ROOT

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32

# name -> (n, P, K, H, W), pairs, seed.  Seeds are chosen so that the margin condition below holds.
CASES = {
    "main": ((2, 3, 17, 56, 56), None, 11),     # a zero box between two live ones; an image with no valid box
    "tiny": ((1, 1, 3, 5, 7), [0, 2, 1], 12),   # less than one wave; odd width: the centre column maps to itself
    "unit": ((1, 2, 1, 1, 1), [0], 13),         # H = W = 1: coordinate 0
    "wide": ((1, 1, 32, 8, 64), list(range(31, -1, -1)), 14),   # K at its limit, every plane swapped
    "odd": ((3, 1, 2, 65, 63), [1, 0], 15),     # 4095 values: not a multiple of 64, H != W; image 1 is a dummy
}


def _boxes(name, n, P, rng):
    b = np.stack([rng.uniform(0.3, 0.7, (n, P)), rng.uniform(0.3, 0.7, (n, P)), rng.uniform(0.2, 0.6, (n, P)),
                  rng.uniform(0.2, 0.6, (n, P))], -1).astype(f32)
    if name == "main":
        b[0, 1] = 0                      # skipped: slot 1 of image 0 is caller row 2
        b[0, 2] = [0.0, 1.0, 0.5, 0.4]   # centred on the image's corner: about half the joints clamp on each axis
        b[1] = 0                         # no valid box: the dummy person
    if name == "odd":
        b[1] = 0
    return b


@functools.lru_cache(maxsize=None)
def _case(name):
    (n, P, K, H, W), pairs, seed = CASES[name]
    rng = np.random.default_rng(seed)
    pairs = R.flip_index(K) if pairs is None else pairs
    # signed maps: a plane's level is drawn over [-6, 2], so its peak lands in every visibility class
    level = rng.uniform(-6.0, 2.0, (n, P, K, 1, 1))
    a = (level + rng.normal(0, 0.5, (n, P, K, H, W))).astype(f32)
    b = (R.mirror_swap(level, pairs)[..., ::-1] + rng.normal(0, 0.5, (n, P, K, H, W))).astype(f32)
    for t in (a, b):   # one sharp off-centre bump per plane, so the soft-argmax is not the plane's centre
        t[..., H // 3, (2 * W) // 3] += f32(3.0)
    boxes = _boxes(name, n, P, rng)
    ref = R.flip_merge(a, b, boxes, pairs)
    for v in (a, b, boxes, *ref.values()):
        v.setflags(write=False)
    return a, b, boxes, pairs, ref


# ------------------------------------------------------------------ CPU
def test_symbol_is_declared_bound_and_exported():
    from dll import _native
    hdr = (ROOT / "include" / "kpd.h").read_text()
    assert re.search(r"\bint kpd_flip_merge\s*\(", hdr)
    assert "kpd_flip_merge" in _native.EXPORTS and callable(_native.flip_merge)
    lib = _native.load()
    assert lib.kpd_flip_merge.restype is ctypes.c_int and len(lib.kpd_flip_merge.argtypes) == 14
    assert (_native.FLIP_MAX_K, _native.FLIP_MAX_SIDE) == (32, 1024)
    assert "#define KPD_FLIP_MAX_K 32" in hdr and "#define KPD_FLIP_MAX_SIDE 1024" in hdr


def test_scalar_argument_checks_need_no_device():
    """The checks run before any device work: with null arrays they still name the argument."""
    from dll import _native
    lib = _native.load()
    ident = (ctypes.c_int32 * 33)(*range(33))

    def call(pairs=ident, n=1, P=1, K=17, H=56, W=56):
        return lib.kpd_flip_merge(None, None, None, pairs, n, P, K, H, W, None, None, None, None, None)

    for kw, word in ((dict(K=33), b"K"), (dict(K=0), b"K"), (dict(H=0), b"H"), (dict(W=1025), b"W"), (dict(P=0), b"P"),
                     (dict(n=-1), b"n"), (dict(pairs=None), b"pairs"),
                     (dict(pairs=(ctypes.c_int32 * 3)(1, 2, 0), K=3), b"pairs"),
                     (dict(pairs=(ctypes.c_int32 * 3)(0, 3, 1), K=3), b"pairs"), (dict(), b"heat_a")):
        assert call(**kw) == -1, kw
        msg = lib.kpd_last_error()
        assert msg.startswith(b"kpd_flip_merge: " + word), (kw, msg)
    assert call(n=0) == 0


def test_flip_index_is_an_involution():
    from dll.utils import COCO_FLIP_PAIRS, flip_index
    idx = flip_index()
    assert idx == R.flip_index(17) == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
    assert all(idx[idx[k]] == k for k in range(17)) and idx[0] == 0
    assert len(COCO_FLIP_PAIRS) == 8 and all(idx[a] == b and idx[b] == a for a, b in COCO_FLIP_PAIRS)
    assert flip_index(3, ((1, 2),)) == [0, 2, 1] and flip_index(4, ()) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        flip_index(5)                      # the COCO pairs do not fit 5 keypoints
    with pytest.raises(ValueError):
        flip_index(4, ((0, 1), (1, 2)))    # overlapping pairs: no involution


def test_mirror_boxes_rules():
    from dll.utils import mirror_boxes, mirror_images
    tiny = float(np.finfo(f32).tiny)
    b = torch.tensor([[[0.25, 0.5, 0.125, 0.75], [0, 0, 0, 0], [1.0, 0, 0, 0], [0.0, 0.5, 0.25, 0.25],
                       [1.0, 0.5, 0.0, 0.0]]])
    m = mirror_boxes(b)
    assert m.shape == b.shape and m.dtype == torch.float32
    assert m[0, 0].tolist() == [0.75, 0.5, 0.125, 0.75]
    assert m[0, 1].tolist() == [0, 0, 0, 0]                     # padding stays padding
    assert m[0, 2].tolist() == [tiny, 0, 0, 0]                  # a live row stays live
    assert m[0, 3].tolist() == [1.0, 0.5, 0.25, 0.25] and m[0, 4].tolist() == [0.0, 0.5, 0.0, 0.0]
    assert torch.equal((m == 0).all(-1), (b == 0).all(-1))      # both passes compact identically
    assert np.array_equal(m.numpy(), R.mirror_boxes(b.numpy()))
    g = torch.Generator().manual_seed(3)
    dyadic = torch.randint(1, 64, (4, 3, 4), generator=g).float() / 64
    dyadic[1, 2] = 0
    assert torch.equal(mirror_boxes(mirror_boxes(dyadic)), dyadic)
    assert np.array_equal(R.mirror_boxes(R.mirror_boxes(dyadic.numpy())), dyadic.numpy())
    x = torch.arange(24.0).reshape(1, 2, 3, 4)
    assert torch.equal(mirror_images(x)[0, 1, 2], torch.tensor([23.0, 22.0, 21.0, 20.0]))
    with pytest.raises(ValueError):
        mirror_boxes(torch.zeros(2, 3))


def test_ref_merging_a_map_with_its_own_mirror_swap_returns_it():
    a, _, boxes, pairs, _ = _case("main")
    got = R.flip_merge(a, R.mirror_swap(a, pairs), boxes, pairs)
    live = np.zeros(a.shape[:2], bool)
    for i, rows in enumerate(R.compaction(boxes)):
        live[i, :len(rows)] = True
    assert live.sum() == 2 and np.array_equal(got["heatmap"][live], a[live])
    assert np.array_equal(got["keypoint_peaks"][live], a[live].max((-2, -1)))


def test_ref_mirrored_single_pixel_peaks_stay_one_peak():
    K, H, W, c, y = 3, 5, 8, 6, 2
    pairs = [0, 2, 1]
    a, b = np.zeros((1, 1, K, H, W), f32), np.zeros((1, 1, K, H, W), f32)
    for k in range(K):
        a[0, 0, k, y, c] = 8 + k
        b[0, 0, pairs[k], y, W - 1 - c] = 8 + k
    got = R.flip_merge(a, b, np.array([[[0.5, 0.5, 1, 1]]], f32), pairs)
    assert np.array_equal(got["heatmap"], a)
    assert (np.count_nonzero(got["heatmap"][0, 0], axis=(-2, -1)) == 1).all()
    assert np.allclose(got["keypoints"][0, 0, :, 0], c / (W - 1), atol=2e-2) and (got["visibilities"][0, 0, :, 2] == 1).all()


def test_ref_padding_and_dummy_slots():
    a, b, boxes, pairs, ref = _case("main")
    assert R.compaction(boxes) == [[0, 2], []]
    for key in ("heatmap", "keypoints", "keypoint_peaks"):
        assert not ref[key][0, 2].any() and not ref[key][1].any() and ref[key][0, :2].any(), key
    v = ref["visibilities"]
    assert not v[0, 2].any() and not v[1, 1:].any()
    assert (v[1, 0, :, 0] == 1).all() and not v[1, 0, :, 1:].any()       # the dummy person: class 0
    assert (v[0, :2].sum(-1) == 1).all()
    # slot 1 of image 0 is decoded with caller row 2's box, which clamps
    kp = ref["keypoints"][0, 1]
    assert (kp[:, 0] <= 0.25).all() and kp.min() == 0.0 and kp.max() == 1.0
    assert ((kp[:, 0] > 0) & (kp[:, 0] < 0.25)).any() and ((kp[:, 1] > 0.8) & (kp[:, 1] < 1)).any()
    odd = _case("odd")
    assert R.compaction(odd[2]) == [[0], [], [0]] and (odd[4]["visibilities"][1, 0, :, 0] == 1).all()


def test_seeded_cases_keep_their_margins():
    """A condition on the seeds, not on the kernel: no sigmoid(peak) within 1e-4 of a class border, and all three
    visibility classes occur across the cases (the maps are signed, so class 0 does)."""
    seen = np.zeros(3, int)
    for name in CASES:
        ref = _case(name)[4]
        m = R.margin(ref)
        print(name, "margin", m)
        assert m >= 1e-4, (name, m)
        live = ~np.isnan(ref["confidence"])
        seen += ref["visibilities"][live].sum(0).astype(int)
    print("classes", seen)
    assert (seen > 0).all(), seen


# ------------------------------------------------------------------ GPU
def _gpu(a, b, boxes, pairs, **kw):
    from dll.utils import flip_merge
    out = flip_merge(torch.tensor(a).to(DEV), torch.tensor(b).to(DEV), torch.tensor(boxes).to(DEV),
                     pairs, **kw)
    torch.cuda.synchronize()
    return out


def _compare(out, ref):
    n, P, K = ref["keypoint_peaks"].shape
    assert out["keypoints"].shape == (n, P, 1, K, 2) and out["visibilities"].shape == (n, P, 1, K, 3)
    assert np.array_equal(out["heatmap"].cpu().numpy().view(np.uint32), ref["heatmap"].view(np.uint32))
    assert np.array_equal(out["keypoint_peaks"].cpu().numpy().view(np.uint32), ref["keypoint_peaks"].view(np.uint32))
    assert np.array_equal(out["visibilities"].cpu().numpy()[:, :, 0], ref["visibilities"])
    err = np.abs(out["keypoints"].cpu().numpy()[:, :, 0].astype(np.float64) - ref["keypoints"]).max()
    print("keypoints max|d|", err)
    assert err <= 1e-6, err


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_matches_the_restatement(name):
    a, b, boxes, pairs, ref = _case(name)
    _compare(_gpu(a, b, boxes, pairs), ref)


@gpu
@pytest.mark.parametrize("name", ["main", "tiny"])
def test_gpu_in_place_gives_the_same_results(name):
    a, b, boxes, pairs, ref = _case(name)
    from dll.utils import flip_merge
    ta = torch.tensor(a).to(DEV)
    out = flip_merge(ta, torch.tensor(b).to(DEV), torch.tensor(boxes).to(DEV), pairs, inplace=True)
    torch.cuda.synchronize()
    assert out["heatmap"] is ta
    _compare(out, ref)


@gpu
def test_gpu_default_pairs_are_the_coco_ones_and_cpu_tensors_raise():
    from dll import _native
    from dll.utils import flip_merge
    a, b, boxes, pairs, ref = _case("main")
    _compare(_gpu(a, b, boxes, None), ref)
    with pytest.raises(_native.KpdNativeError):
        flip_merge(torch.tensor(a), torch.tensor(b).to(DEV), torch.tensor(boxes).to(DEV))
    with pytest.raises(_native.KpdNativeError):
        flip_merge(torch.tensor(a).to(DEV), torch.tensor(b).to(DEV), torch.tensor(boxes))
    with pytest.raises(ValueError):
        flip_merge(torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)[:1], torch.tensor(boxes).to(DEV))


@gpu
def test_gpu_an_image_does_not_depend_on_its_batch():
    a, b, boxes, pairs, _ = _case("main")
    both = _gpu(a, b, boxes, pairs)
    alone = _gpu(a[:1], b[:1], boxes[:1], pairs)
    for key in ("heatmap", "keypoints", "visibilities", "keypoint_peaks"):
        assert torch.equal(both[key][:1], alone[key]), key


@gpu
def test_gpu_argument_checks_name_the_argument():
    from dll import _native
    lib = _native.load()
    n, P, K, H, W = 1, 1, 3, 5, 7
    a, b = torch.zeros(n, P, K, H, W, device=DEV), torch.zeros(n, P, K, H, W, device=DEV)
    boxes = torch.tensor([[[0.5, 0.5, 0.5, 0.5]]], device=DEV)
    kp, vis, pk = torch.zeros(n, P, K, 2, device=DEV), torch.zeros(n, P, K, 3, device=DEV), torch.zeros(n, P, K, device=DEV)
    ok = (ctypes.c_int32 * 33)(0, 2, 1, *range(3, 33))
    p = _native._ptr

    def call(pairs=ok, heat_out=None, n=n, K=K, H=H):
        with torch.cuda.device(DEV):
            return lib.kpd_flip_merge(p(a), p(b), p(boxes), pairs, n, P, K, H, W, heat_out, p(kp), p(vis), p(pk),
                                      _native._stream(DEV))

    for kw, word in ((dict(pairs=(ctypes.c_int32 * 3)(1, 2, 0)), b"pairs"), (dict(heat_out=p(b)), b"heat_out"),
                     (dict(heat_out=ctypes.c_void_p(b.data_ptr() + 4)), b"heat_out"), (dict(K=33), b"K"),
                     (dict(H=0), b"H")):
        assert call(**kw) == -1, kw
        msg = lib.kpd_last_error()
        assert msg.startswith(b"kpd_flip_merge: " + word), (kw, msg)
    assert call(n=0) == 0
    assert call() == 0 and call(heat_out=p(a)) == 0
    torch.cuda.synchronize()
    assert vis.sum() == K      # the valid calls ran: one class per plane
    with pytest.raises(ValueError, match="pairs"):
        _native.flip_merge(a, b, boxes, [1, 2, 0], None, kp, vis, pk)
