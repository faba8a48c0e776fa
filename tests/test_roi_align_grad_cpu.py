"""tests/roi_align_grad_ref.py against tests/ops_ref.py:roi_align_ref, without a
device: the backward reference is the exact adjoint of the forward reference
the ROI-align kernels are pinned with, and the binding is registered."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ops_ref as R  # noqa: E402
import roi_align_grad_ref as G  # noqa: E402

MAPS = [(13, 9), (8, 12)]


def _setup(H, W, C, Cs, seed=3):
    boxes = G.edge_boxes()
    gen = torch.Generator().manual_seed(seed)
    feat = torch.randn(2, C, H, W, generator=gen, dtype=torch.float64)
    topk = None if Cs == C else G.shuffled_topk(2, Cs, C, seed + 1)
    return boxes, feat, topk, gen


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,Cs", [(5, 5), (12, 7)])
@pytest.mark.parametrize("rows", list(G.ROW_SETS))
def test_reference_is_the_adjoint_of_the_forward_reference(H, W, C, Cs, rows):
    """<roi_align_ref(F), G> == <F, grad_ref(G)> in fp64 to 1e-12 relative."""
    boxes, feat, topk, gen = _setup(H, W, C, Cs)
    rs = G.ROW_SETS[rows]
    gout = torch.randn(len(rs), Cs, 56, 56, generator=gen, dtype=torch.float64)
    gathered = feat if topk is None else torch.stack([feat[b, topk[b].long()] for b in range(2)])
    out, _ = R.roi_align_ref(gathered, G.boxes_to_rois(boxes, rs, H, W), 56)
    gfeat, S, N = G.roi_align_grad_ref(gout, boxes, rs, topk, C, H, W)
    lhs, rhs = float((out * gout.numpy()).sum()), float((feat.numpy() * gfeat).sum())
    scale = float((np.abs(feat.numpy()) * S).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)
    assert (N[S > 0] > 0).all() and (np.abs(gfeat) <= S * (1 + 1e-12)).all()


@pytest.mark.parametrize("H,W", MAPS + [(128, 96)])
def test_one_hot_gradient_gives_the_outer_product_of_two_rows(H, W):
    boxes = G.edge_boxes()
    rs = G.ROW_SETS["with_padding"]
    rois = G.boxes_to_rois(boxes, rs, H, W).numpy()
    for i, (p, q) in enumerate([(0, 0), (55, 55), (17, 40), (3, 54), (55, 1), (28, 28)]):
        gout = torch.zeros(len(rs), 2, 56, 56, dtype=torch.float64)
        gout[i, 1, p, q] = 1.0
        gfeat, _, N = G.roi_align_grad_ref(gout, boxes, rs, None, 2, H, W)
        My, Mx, count, _ = G.roi_matrices(rois[i], H, W)
        b = rs[i] // 3
        assert np.array_equal(gfeat[b, 1], np.outer(My[p], Mx[q]) / count)
        assert (gfeat[1 - b] == 0).all() and (gfeat[b, 0] == 0).all()
        assert N[b, 1].max() > 0


def test_whole_image_grid_at_the_training_map():
    """The 128 x 96 case of the device test covers sampling grids above 1: 3 x 2."""
    rois = G.boxes_to_rois(torch.tensor([[[0.5, 0.5, 1.0, 1.0]]]), [0], 128, 96).numpy()
    assert G.roi_matrices(rois[0], 128, 96)[3] == (3, 2)


def test_thin_box_puts_every_bin_on_a_few_pixels():
    """A size-1 ROI: each bin touches 2 x 2 pixels, and all 56 x 56 of them lie
    in a patch of at most 3 x 3 (2 x 2 when the corner is on the pixel grid,
    as the padding box's is): the longest sums of the device test."""
    for H, W in MAPS:
        for row, patch in ((1, 3), (5, 2)):
            rois = G.boxes_to_rois(G.edge_boxes(), [row], H, W).numpy()
            My, Mx, count, grid = G.roi_matrices(rois[0], H, W)
            assert grid == (1, 1) and count == 1
            assert 2 <= (My != 0).any(axis=0).sum() <= patch and 2 <= (Mx != 0).any(axis=0).sum() <= patch
            gout = torch.ones(1, 1, 56, 56, dtype=torch.float64)
            _, _, N = G.roi_align_grad_ref(gout, G.edge_boxes(), [row], None, 1, H, W)
            assert N.sum() == 4 * 56 * 56 and (N > 0).sum() <= patch * patch
            assert N.max() >= 4 * 56 * 56 // (patch * patch)


@pytest.mark.parametrize("H,W", MAPS)
def test_unselected_channels_and_images_without_rows_are_exactly_zero(H, W):
    boxes, _, topk, gen = _setup(H, W, 12, 7)
    for name, rs in G.ROW_SETS.items():
        gout = torch.randn(len(rs), 7, 56, 56, generator=gen, dtype=torch.float64)
        gfeat, S, N = G.roi_align_grad_ref(gout, boxes, rs, topk, 12, H, W)
        for b in range(2):
            off = sorted(set(range(12)) - set(int(c) for c in topk[b]))
            assert (gfeat[b, off] == 0).all() and (N[b, off] == 0).all(), name
            if not any(r // 3 == b for r in rs):
                assert (gfeat[b] == 0).all() and (S[b] == 0).all(), name
    empty, _, _ = G.roi_align_grad_ref(torch.zeros(0, 7, 56, 56), boxes, [], topk, 12, H, W)
    assert (empty == 0).all()


def test_padding_box_is_the_size_one_roi_at_the_origin():
    rois = G.boxes_to_rois(G.edge_boxes(), [5], 13, 9).numpy()
    assert rois[0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    My, Mx, count, grid = G.roi_matrices(rois[0], 13, 9)
    assert grid == (1, 1) and (My[:, 2:] == 0).all() and (Mx[:, 2:] == 0).all() and My[:, :2].sum() == pytest.approx(56)


def test_binding_is_registered_and_validates_before_the_device():
    """kpd_roi_align_backward is exported and bound; bad arguments come back as
    KPD_EINVAL with a message, before any device work (no device here)."""
    from dll import _native
    lib = _native.load()
    assert "kpd_roi_align_backward" in _native.EXPORTS and hasattr(lib, "kpd_roi_align_backward")
    one = 1   # any non-null address: validation fails before it is read
    assert lib.kpd_roi_align_backward(one, one, one, 1, 2, 3, None, 6, 5, 8, 12, one, None) == -1      # Cs > C
    assert b"kpd_roi_align_backward" in lib.kpd_last_error()
    assert lib.kpd_roi_align_backward(None, one, one, 1, 2, 3, None, 5, 5, 8, 12, one, None) == -1     # null gout
    assert lib.kpd_roi_align_backward(one, one, one, 7, 2, 3, None, 5, 5, 8, 12, one, None) == -1      # n > B * P
    assert lib.kpd_roi_align_backward(one, one, one, 1, 2, 3, None, 4, 5, 8, 12, one, None) == -1      # Cs != C, no topk
    assert lib.kpd_roi_align_backward(one, one, one, 1, 2, 3, None, 5, 5, 8, 4096, one, None) == -1    # too wide
    assert b"LDS" in lib.kpd_last_error()


@pytest.mark.parametrize("H,W", [(13, 9), (64, 48), (128, 96), (40, 500), (551, 8)])
def test_compact_tables_stay_inside_the_kernels_capacity(H, W):
    """The kernel stores an axis matrix as footprint x longest band floats and
    sizes that table 3 * size + 512 (csrc/roi_align_grad.hip derives the bound;
    a longer band would be clamped, dropping terms).  On the reference's own
    matrices, extents swept over the whole range at shifting offsets, and the
    edge boxes: the table never needs more, and the sweep reaches 56-bin bands."""
    boxes = [G.sweep_boxes(H, W, 97)]
    if H * W < 128 * 96:
        boxes.append(G.edge_boxes().reshape(1, 6, 4))
    worst_x = worst_y = 0
    for bx in boxes:
        rois = G.boxes_to_rois(bx, range(bx.shape[1]), H, W).numpy()
        for roi in rois:
            My, Mx, _, _ = G.roi_matrices(roi, H, W)
            worst_x, worst_y = max(worst_x, G.compact_table_size(Mx)), max(worst_y, G.compact_table_size(My))
    print(f"{H}x{W}: largest table x {worst_x} of {3 * W + 512}, y {worst_y} of {3 * H + 512}")
    assert worst_x <= min(56 * W, 3 * W + 512) and worst_y <= min(56 * H, 3 * H + 512)
    assert worst_x >= 2 * 56 and worst_y >= 2 * 56            # the size-1 end of the sweep: full bands
