"""roi_align_nchw_kernel (csrc/ops_kernels.hip) through _native.roi_align on
everything extract_roi_features never passes: aligned, fixed sampling ratios,
spatial scales, non-square outputs, multi-image batches, the sample-skip
branch and the batch-index check, against tests/ops_ref.roi_align_ref (tied
to the oracle's scalar loop and the golden ROI slice by test_ops_ref_cpu.py).

Which branch each box reaches (feature map 20 x 16, in feature pixels):
  inside            plain bilinear samples
  touch_*           samples on the clamp at 0 and the `>= H-1` edge case
  cross_*           part of the samples beyond -1 / H / W: skipped
  outside_*         every sample skipped: exact zeros
  zero, inverted    aligned=False clamps the size to 1; aligned=True with
                    sampling_ratio=-1 gives grid <= 0: zeros; with a fixed
                    ratio torchvision samples a degenerate / mirrored box
  huge              a box several times the map, grid up to 77 per bin
  random            seeded boxes, kept only when the reference's own distance
                    from a skip boundary exceeds 1e-3 (none is dropped: checked
                    on the CPU below)

Bar: (4 gh gw + 2) * 2^-23 * max|feat| per ROI; boxes on the pixel grid at
dyadic coordinates on integer-valued features must be exact.  The skip test
is the operator's only discontinuity, so every non-dyadic case is checked to
stay 1e-3 away from it.
"""
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ops_ref as R  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")

H, W = 20, 16
OUT_SIZES = [(1, 1), (7, 5), (3, 14), (56, 56)]
COMBOS = list(itertools.product((False, True), (-1, 1, 2, 3), (1.0, 0.5, 0.25), OUT_SIZES))

EDGE_BOXES = {                       # x1, y1, x2, y2 in feature pixels
    "inside": (1.3, 2.2, 9.7, 17.9),
    "touch_tl": (0.0, 0.0, 4.3, 5.1),
    "touch_br": (11.7, 14.9, 16.0, 20.0),
    "full": (0.0, 0.0, 16.0, 20.0),
    "cross_left": (-3.37, 5.21, 5.13, 12.37),
    "cross_right": (10.23, 5.21, 19.61, 12.37),
    "cross_top": (4.11, -2.83, 9.37, 6.19),
    "cross_bottom": (4.11, 15.27, 9.37, 23.71),
    "outside_tl": (-30.3, -30.7, -20.1, -22.9),
    "outside_br": (40.3, 50.7, 48.1, 60.9),
    "zero": (5.3, 6.7, 5.3, 6.7),
    "inverted": (9.3, 12.7, 4.1, 3.3),
    "huge": (-20.3, -25.7, 40.9, 51.3),
}
N_RANDOM = 6


def rois_for(scale: float, seed: int = 11) -> torch.Tensor:
    """[R,5]: the edge boxes and N_RANDOM seeded boxes, in input coordinates
    (feature pixels / scale); batch indices out of order, one image repeated."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(N_RANDOM, 2, generator=g) * torch.tensor([W, H]) * 1.2 - torch.tensor([W, H]) * 0.1
    wh = torch.rand(N_RANDOM, 2, generator=g) * torch.tensor([W, H]) * 0.8 + 0.2
    boxes = torch.cat([torch.tensor(list(EDGE_BOXES.values())), torch.cat([c - wh / 2, c + wh / 2], dim=1)])
    bidx = torch.tensor([2, 0, 1, 1, 0, 2, 2, 1, 0, 0, 1, 2, 1, 2, 0, 1, 1, 0, 2])[: len(boxes)]
    return torch.cat([bidx[:, None].float(), boxes / scale], dim=1)


def features(C: int, h: int = H, w: int = W, B: int = 3, seed: int = 5) -> torch.Tensor:
    return torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(seed))


SHAPES = [(1, 5, 7), (130, 5, 7), (1, 20, 16), (130, 20, 16), (3, 5, 7)]


def shape_combos(C):
    return [(False, -1, 1.0, (7, 5)), (True, 2, 0.5, (3, 14)), (True, -1, 0.25, (1, 1)),
            (False, 3, 1.0, (56, 56) if C < 130 else (7, 5))]


def shape_rois(scale, h, w):
    rois = rois_for(scale)
    rois[:, 1:] *= torch.tensor([w / W, h / H, w / W, h / H])            # the same boxes on the smaller map
    return rois


def test_cases_stay_clear_of_the_skip_boundary():
    """No case is dropped: every combination keeps all boxes more than 1e-3
    from a skip boundary by the reference's own coordinates (CPU)."""
    feat = features(1)
    worst = np.inf
    for aligned, sr, scale, out in COMBOS:
        _, info = R.roi_align_ref(feat, rois_for(scale), out, scale, sr, aligned)
        worst = min(worst, info["skip_dist"])
        assert info["skip_dist"] > 1e-3, (aligned, sr, scale, out, info["skip_dist"])
    for C, h, w in SHAPES:
        for aligned, sr, scale, out in shape_combos(C):
            _, info = R.roi_align_ref(features(1, h, w), shape_rois(scale, h, w), out, scale, sr, aligned)
            worst = min(worst, info["skip_dist"])
            assert info["skip_dist"] > 1e-3, (C, h, w, aligned, sr, scale, out, info["skip_dist"])
    assert len(rois_for(1.0)) == len(EDGE_BOXES) + N_RANDOM
    assert (len(rois_for(1.0)) * 3 * 7 * 5) % 256 != 0           # a partial last workgroup
    print("smallest distance from a skip boundary:", worst)


def _check(feat, rois, out, scale, sr, aligned, tag):
    from dll import _native
    want, info = R.roi_align_ref(feat, rois, out, scale, sr, aligned)
    got = _native.roi_align(feat.to(DEV), rois.to(DEV), out, scale, sr, aligned).cpu().numpy()
    assert got.shape == want.shape, tag
    bound = R.roi_align_bound(info, feat)[:, None, None, None]
    err = np.abs(got - want)
    assert (err <= bound).all(), (tag, float((err - bound).max()), int(np.argmax((err - bound).max(axis=(1, 2, 3)))))
    return got, want


@gpu
@pytest.mark.parametrize("aligned", [False, True])
def test_cross_of_modes_ratios_scales_and_output_sizes(aligned):
    feat = features(3)
    names = list(EDGE_BOXES)
    for al, sr, scale, out in COMBOS:
        if al != aligned:
            continue
        got, want = _check(feat, rois_for(scale), out, scale, sr, al, (al, sr, scale, out))
        for n in ("outside_tl", "outside_br"):
            assert (got[names.index(n)] == 0).all(), (n, al, sr, scale, out)
        if al and sr == -1:                                      # grid <= 0: no sample, zeros
            for n in ("zero", "inverted"):
                assert (got[names.index(n)] == 0).all() and (want[names.index(n)] == 0).all(), (n, scale, out)
        if not al:                                               # size clamped to 1: a real window
            assert np.abs(want[names.index("zero")]).max() > 0


@gpu
@pytest.mark.parametrize("C,h,w", SHAPES)
def test_feature_shapes(C, h, w):
    feat = features(C, h, w)
    for aligned, sr, scale, out in shape_combos(C):
        _check(feat, shape_rois(scale, h, w), out, scale, sr, aligned, (C, h, w, aligned, sr, scale, out))


@gpu
def test_dyadic_boxes_on_integer_features_are_exact():
    """Boxes whose bins and sample offsets are dyadic: every weight is exact in
    fp32 and the sums are small integers over powers of two."""
    feat = torch.randint(-8, 9, (3, 3, H, W), generator=torch.Generator().manual_seed(6)).float()
    from dll import _native
    cases = [((1, 1), (0.5, 1.25, 8.5, 9.25)), ((7, 5), (1.0, 2.0, 11.0, 16.0)), ((3, 14), (1.0, 1.0, 15.0, 7.0)),
             ((56, 56), (1.0, 2.0, 15.0, 9.0)), ((7, 5), (-4.0, -6.0, 6.0, 8.0)), ((3, 14), (9.0, 17.0, 23.0, 23.0))]
    for (out, box), aligned, sr, scale in itertools.product(cases, (False, True), (-1, 1, 2), (1.0, 0.5, 0.25)):
        rois = torch.tensor([[b, *[v / scale for v in box]] for b in (1, 0, 2, 1)])
        want, _ = R.roi_align_ref(feat, rois, out, scale, sr, aligned)
        got = _native.roi_align(feat.to(DEV), rois.to(DEV), out, scale, sr, aligned).cpu().numpy()
        assert np.array_equal(got.astype(np.float64), want), (out, box, aligned, sr, scale)


@gpu
def test_no_rois_returns_empty():
    from dll import _native
    out = _native.roi_align(features(3).to(DEV), torch.zeros(0, 5, device=DEV), (7, 5), 0.5, 2, True)
    assert out.shape == (0, 3, 7, 5)


@gpu
@pytest.mark.parametrize("aligned", [False, True])
def test_batch_index_outside_the_batch_gives_zeros(aligned):
    """The kernel checks ro[0] against B.  Views of a larger allocation, so
    code without the check reads memory the test owns: big[:2] with index 2
    and 3, big[2:] with index -1 and -2, big[1:4] with index 3; NaN too."""
    from dll import _native
    big = features(3, B=5, seed=9).to(DEV) + 3.0
    box = [2.0, 3.0, 11.0, 15.0]
    nan = float("nan")
    for view, idx in ((big[:2], [2.0, 0.0, 3.0, 1.0]), (big[2:], [-1.0, 0.0, nan, -2.0, 2.0]),
                      (big[1:4], [3.0, 2.0, -1.0, 0.0])):
        B = view.shape[0]
        rois = torch.tensor([[i, *box] for i in idx])
        got = _native.roi_align(view, rois.to(DEV), (7, 5), 1.0, 2, aligned).cpu().numpy()
        want, info = R.roi_align_ref(view.cpu(), rois, (7, 5), 1.0, 2, aligned)
        assert (np.abs(got - want) <= R.roi_align_bound(info, view.cpu())[:, None, None, None]).all(), idx
        for r, i in enumerate(idx):
            if 0 <= i < B:
                assert np.abs(got[r]).min() > 0, (idx, r)            # a real image: features 3 +- randn
            else:
                assert (got[r] == 0).all() and (want[r] == 0).all(), (idx, r)
