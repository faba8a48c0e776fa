"""kpd_roi_targets without a device: the properties of the numpy restatement
(tests/roi_targets_ref.py), the decode round trip through the decoders'
coordinate convention, and the argument checks of the two new C entry points."""
import ctypes

import numpy as np
import pytest

import roi_targets_ref as RR


@pytest.mark.parametrize("H,W,sigma", [(56, 56, 2.0), (14, 10, 1.0)])
def test_restatement_properties(H, W, sigma):
    kpts, vis, boxes, where = RR.cases(6, 17, seed=3)
    heat, weight = RR.roi_targets_ref(kpts, vis, boxes, None, H, W, sigma)
    assert heat.shape == (6, 17, H, W) and weight.shape == (6, 17) and heat.dtype == np.float64
    on = weight > 0
    assert on.sum() > 40 and set(np.unique(weight)) == {0.0, 1.0}
    # a labelled joint inside its box: the centre is at most half a pixel from the grid in each axis
    peak = heat.reshape(6, 17, -1).max(-1)
    assert np.all(peak[on] >= np.exp(-0.25 / sigma ** 2)) and np.all(peak[on] <= 1.0)
    assert np.all(heat[~on] == 0)
    for name in ("vis0", "outside", "nan", "w0", "zero_box"):
        r, k = where[name]
        assert weight[r, k] == 0 and not heat[r, k].any(), name
    assert not weight[1].any() and not weight[2].any()     # w == 0 and the all-zero box: whole rows
    # u exactly 0 and exactly 1 on dyadic inputs are on, with the peak in the border column
    r, k = where["u0"]
    assert weight[r, k] == 1 and heat[r, k].argmax() % W == 0 and heat[r, k].max() >= np.exp(-0.125 / sigma ** 2)
    r, k = where["u1"]
    assert weight[r, k] == 1 and heat[r, k].argmax() % W == W - 1 and heat[r, k].argmax() // W == H - 1
    assert heat[r, k].max() == 1.0


def test_rows_gather_and_empty():
    kpts, vis, boxes, _ = RR.cases(6, 17, seed=3)
    full, wfull = RR.roi_targets_ref(kpts, vis, boxes, None, 14, 10, 1.0)
    part, wpart = RR.roi_targets_ref(kpts, vis, boxes, [4, 0, 3], 14, 10, 1.0)
    assert np.array_equal(part, full[[4, 0, 3]]) and np.array_equal(wpart, wfull[[4, 0, 3]])
    none, wnone = RR.roi_targets_ref(kpts, vis, boxes, [], 14, 10, 1.0)
    assert none.shape == (0, 17, 14, 10) and wnone.shape == (0, 17)


def test_decode_round_trip():
    """The argmax of each `on` plane, read as i/(W-1) and mapped through the
    box, recovers the labelled joint within 0.5 heatmap pixels per axis
    (seeded boxes and joints at 56 x 56: 0.492 measured)."""
    kpts, vis, boxes, _ = RR.cases(24, 17, seed=11)
    heat, weight = RR.roi_targets_ref(kpts, vis, boxes, None, 56, 56, 2.0)
    on = weight > 0
    got = RR.decode_to_image(heat, boxes)
    with np.errstate(all="ignore"):
        err = np.abs(got - kpts.astype(np.float64)) / boxes[:, None, 2:].astype(np.float64) * 55
    worst = float(err[on].max())
    print(f"decode round trip: {worst:.3f} heatmap pixels over {int(on.sum())} joints")
    assert on.sum() > 300 and worst <= 0.5


def test_float32_rule_is_close_to_float64():
    kpts, vis, boxes, _ = RR.cases(6, 17, seed=3)
    h64, _ = RR.roi_targets_ref(kpts, vis, boxes, None, 56, 56, 2.0)
    h32, _ = RR.roi_targets_ref(kpts, vis, boxes, None, 56, 56, 2.0, dtype=np.float32)
    assert h32.dtype == np.float32 and float(np.abs(h32 - h64).max()) < 1e-6


def _lib():
    from dll import _native
    return _native.load()


def test_roi_targets_argument_checks():
    lib = _lib()
    one = ctypes.c_void_p(64)   # non-null, never dereferenced: the checks come before any device work

    def call(kp=one, vis=one, boxes=one, rows=None, n=1, R=1, K=17, H=56, W=56, sigma=2.0, heat=one, weight=one):
        return lib.kpd_roi_targets(kp, vis, boxes, rows, n, R, K, H, W, sigma, heat, weight, None)

    assert call(n=0) == 0
    assert call(n=0, kp=None, heat=None) == 0
    for bad in (dict(kp=None), dict(vis=None), dict(boxes=None), dict(heat=None), dict(weight=None), dict(n=-1),
                dict(H=1), dict(W=1), dict(K=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("inf")),
                dict(sigma=float("nan")), dict(n=2, R=1)):
        assert call(**bad) == -1, bad
        assert b"kpd_roi_targets" in lib.kpd_last_error(), bad


def test_roi_features_argument_checks():
    lib = _lib()
    one = ctypes.c_void_p(64)
    rc = lib.kpd_roi_features(None, one, 1, 3, 64, 64, one, 1, None, 1, one, None)
    assert rc == -1 and b"null plan" in lib.kpd_last_error()
    h = ctypes.c_void_p()
    assert lib.kpd_plan_create(0, 3, ctypes.byref(h)) == 0

    def call(image=one, B=1, C=3, H=64, W=64, boxes=one, P=1, rows=None, n=1, out=one):
        return lib.kpd_roi_features(h, image, B, C, H, W, boxes, P, rows, n, out, None)

    # the argument checks come first (no finalized plan is needed to see them) ...
    for bad, word in ((dict(image=None), b"image"), (dict(B=0), b"image"), (dict(H=16), b"image"),
                      (dict(C=1), b"channels"), (dict(boxes=None), b"boxes"), (dict(P=0), b"boxes"),
                      (dict(n=-1), b"rows"), (dict(n=2), b"rows"), (dict(out=None), b"output")):
        assert call(**bad) == -1, bad
        assert word in lib.kpd_last_error(), (bad, lib.kpd_last_error())
    # ... then the plan's state
    assert call() == -3 and b"finalized" in lib.kpd_last_error()
    lib.kpd_plan_destroy(h)
