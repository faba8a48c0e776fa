"""kpd_roi_align_backward (csrc/roi_align_grad.hip) through
_native.roi_align_backward and dll.ops.roi_align_boxes against
tests/roi_align_grad_ref.py, at the smallest shapes at which the kernel can go
wrong: a 13 x 9 map (odd sizes, W % 4 != 0: scalar stores) and an 8 x 12 map
(the 16-byte path), each with C = Cs = 5 without topk (a partial channel chunk)
and with C = 128, Cs = 64 and a shuffled distinct topk per image; the boxes of
roi_align_grad_ref.edge_boxes (whole image, thinner than a pixel, over both
corners, an overlap, the all-zero padding box left out and included, an image
without a row); and the whole image at a 128 x 96 map (sampling grid 3 x 2,
four row bands per channel chunk).

Bar: |got - want| <= (N + 2) 2^-23 S per element (derived in the reference's
docstring); zeros exactly where nothing lands; equal bits between calls and
between batches."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ops_ref as R  # noqa: E402
import roi_align_grad_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

MAPS = [(13, 9), (8, 12)]
CHANNELS = [(5, 5), (128, 64)]
_cache = {}


def case(H, W, C, Cs, rows_name):
    """(boxes, rows, topk, gout, (want, S, N)) -- the reference computed once per case."""
    key = (H, W, C, Cs, rows_name)
    if key not in _cache:
        boxes = G.edge_boxes()
        rows = G.ROW_SETS[rows_name]
        topk = None if Cs == C else G.shuffled_topk(2, Cs, C, 7)
        gen = torch.Generator().manual_seed(H * 1000 + W)
        gout = torch.randn(6, Cs, 56, 56, generator=gen)[rows]   # one gradient per box, whatever the row set
        _cache[key] = (boxes, rows, topk, gout, G.roi_align_grad_ref(gout, boxes, rows, topk, C, H, W))
    return _cache[key]


def run(boxes, rows, topk, gout, C, H, W, prefill=True):
    """The raw call into a NaN-filled gfeat (the contract: written completely, no memset needed)."""
    from dll import _native
    lib = _native.load()
    B, P = boxes.shape[:2]
    n = len(rows)
    g = gout.to(DEV).contiguous()
    bx = boxes.to(DEV).contiguous()
    rw = torch.tensor(rows, dtype=torch.int32, device=DEV)
    tk = None if topk is None else topk.to(DEV).contiguous()
    out = torch.full((B, C, H, W), float("nan"), device=DEV) if prefill else torch.empty(B, C, H, W, device=DEV)
    rc = lib.kpd_roi_align_backward(_native._ptr(g) if n else None, _native._ptr(bx) if n else None,
                                    _native._ptr(rw) if n else None, n, B, P, _native._ptr(tk), gout.shape[1], C, H, W,
                                    _native._ptr(out), _native._stream(DEV))
    _native.check(rc, "kpd_roi_align_backward")
    return out


def check_against_reference(got, ref, tag):
    want, S, N = ref
    got = got.cpu().double().numpy()
    assert not np.isnan(got).any(), tag
    err, bound = np.abs(got - want), G.roi_align_grad_bound(S, N)
    print(tag, "max err / bound:", float((err / np.maximum(bound, 1e-300)).max()), "max N:", int(N.max()))
    assert (err <= bound).all(), (tag, float((err - bound).max()))
    assert (got[N == 0] == 0.0).all(), tag          # untouched pixels, unselected channels, images without a row


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,Cs", CHANNELS)
@pytest.mark.parametrize("rows_name", list(G.ROW_SETS))
def test_matches_reference(H, W, C, Cs, rows_name):
    boxes, rows, topk, gout, ref = case(H, W, C, Cs, rows_name)
    got = run(boxes, rows, topk, gout, C, H, W)
    check_against_reference(got, ref, (H, W, C, Cs, rows_name))
    if topk is not None:
        for b in range(2):
            off = sorted(set(range(C)) - set(int(c) for c in topk[b]))
            assert (got[b, off] == 0).all()
    again = run(boxes, rows, topk, gout, C, H, W)
    assert torch.equal(got, again)                  # two calls, equal bits


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,Cs", CHANNELS)
def test_an_image_does_not_depend_on_its_batch(H, W, C, Cs):
    """Image 1's gradient is bit-equal whether image 0 has rows or not; the padding
    box adds its own size-1 ROI at the origin and changes nothing else."""
    boxes, rows, topk, gout, _ = case(H, W, C, Cs, "labelled")
    full = run(boxes, rows, topk, gout, C, H, W)
    _, rows1, _, gout1, _ = case(H, W, C, Cs, "image0_empty")
    alone = run(boxes, rows1, topk, gout1, C, H, W)
    assert torch.equal(full[1], alone[1]) and (alone[0] == 0).all()
    _, rows0, _, gout0, _ = case(H, W, C, Cs, "image1_empty")
    first = run(boxes, rows0, topk, gout0, C, H, W)
    assert torch.equal(full[0], first[0]) and (first[1] == 0).all()
    _, rowsp, _, goutp, _ = case(H, W, C, Cs, "with_padding")
    padded = run(boxes, rowsp, topk, goutp, C, H, W)
    assert torch.equal(padded[0], full[0])
    assert torch.equal(padded[1, :, 2:], full[1, :, 2:]) and torch.equal(padded[1, :, :, 2:], full[1, :, :, 2:])
    assert not torch.equal(padded[1], full[1])


def test_row_order_sum_of_overlapping_rois():
    """Two ROIs that land on the same pixels (the single-row calls show that they
    do) are summed into them inside the bound of the joint sum."""
    H, W, C = 8, 12, 5
    boxes, rows, topk, gout, ref = case(H, W, C, C, "image0_empty")       # the corner box and the box inside it
    both = run(boxes, rows, topk, gout, C, H, W)
    one = [run(boxes, [r], topk, gout[i:i + 1], C, H, W) for i, r in enumerate(rows)]
    assert (one[0][1] != 0).logical_and(one[1][1] != 0).any()             # they do overlap
    check_against_reference(both, ref, "overlap")


def test_whole_image_at_the_training_map():
    """128 x 96, C = 4, the whole image: grid 3 x 2 and four row bands."""
    H, W, C = 128, 96, 4
    boxes = torch.tensor([[[0.5, 0.5, 1.0, 1.0]]])
    gout = torch.randn(1, C, 56, 56, generator=torch.Generator().manual_seed(5))
    ref = G.roi_align_grad_ref(gout, boxes, [0], None, C, H, W)
    got = run(boxes, [0], None, gout, C, H, W)
    check_against_reference(got, ref, "128x96")
    assert (ref[2] > 0).all()                                             # every pixel is touched
    assert torch.equal(got, run(boxes, [0], None, gout, C, H, W))


@pytest.mark.parametrize("H,W,count", [(64, 48, 48), (56, 56, 29), (40, 500, 13), (300, 8, 23)])
def test_extent_sweep_on_maps_whose_row_band_the_lds_budget_sets(H, W, count):
    """ROI extents swept over [1, W] and [1, H] at shifting offsets, all on one
    image: every band length and footprint the compact LDS tables can meet (a
    band longer than the table's capacity would be clamped and lose terms: the
    bound catches that).  64 x 48 and 56 x 56 are level 0 of 128 x 96 and 112 x
    112 images, one band each; at 40 x 500 the column tables leave the row
    band 5 rows (8 bands, grid up to 9); 300 x 8 is tall and narrow."""
    C = 3
    boxes = G.sweep_boxes(H, W, count)
    rows = list(range(count))
    gout = torch.randn(count, C, 56, 56, generator=torch.Generator().manual_seed(H + W))
    ref = G.roi_align_grad_ref(gout, boxes, rows, None, C, H, W)
    got = run(boxes, rows, None, gout, C, H, W)
    check_against_reference(got, ref, ("sweep", H, W))
    assert torch.equal(got, run(boxes, rows, None, gout, C, H, W))


def test_no_rows_gives_zeros():
    boxes = G.edge_boxes()
    for (H, W), (C, Cs) in zip(MAPS, CHANNELS):
        topk = None if Cs == C else G.shuffled_topk(2, Cs, C, 7)
        got = run(boxes, [], topk, torch.zeros(0, Cs, 56, 56), C, H, W)
        assert (got == 0).all() and not torch.isnan(got).any()


def test_invalid_arguments_raise_before_any_launch():
    from dll import _native
    boxes = G.edge_boxes().to(DEV)
    g = torch.zeros(2, 5, 56, 56, device=DEV)
    rows = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = torch.full((2, 5, 8, 12), 7.0, device=DEV)
    lib = _native.load()
    st = _native._stream(DEV)
    p = _native._ptr
    long_rows = torch.arange(7, dtype=torch.int32, device=DEV)
    for args in ((p(g), p(boxes), p(rows), 2, 2, 3, None, 6, 5, 8, 12, p(out), st),          # Cs > C
                 (None, p(boxes), p(rows), 2, 2, 3, None, 5, 5, 8, 12, p(out), st),          # null gout
                 (p(g), p(boxes), p(long_rows), 7, 2, 3, None, 5, 5, 8, 12, p(out), st)):    # rows longer than B * P
        assert lib.kpd_roi_align_backward(*args) == -1
        with pytest.raises(ValueError):
            _native.check(-1, "kpd_roi_align_backward")
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                                # nothing was launched
    with pytest.raises(ValueError):
        _native.roi_align_backward(g, boxes, long_rows, None, 5, 8, 12)
    with pytest.raises(ValueError):
        _native.roi_align_backward(g, boxes, rows, torch.zeros(2, 4, dtype=torch.int32, device=DEV), 5, 8, 12)


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,Cs", CHANNELS)
def test_roi_align_boxes_forward_and_backward(H, W, C, Cs):
    """dll.ops.roi_align_boxes: the forward agrees with _native.roi_align on the
    gathered channels within roi_align_bound, the backward delivers the raw
    call's tensor, and boxes / rows / topk get no gradient."""
    from dll import _native
    from dll.ops import roi_align_boxes
    boxes, rows, topk, gout, _ = case(H, W, C, Cs, "with_padding")
    feat = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(9))
    level0 = feat.to(DEV).requires_grad_(True)
    bx = boxes.to(DEV)
    rw = torch.tensor(rows, dtype=torch.int32, device=DEV)
    tk = None if topk is None else topk.to(DEV)
    out = roi_align_boxes(level0, bx, rw, tk)
    assert out.shape == (len(rows), Cs, 56, 56)
    gathered = feat if topk is None else torch.stack([feat[b, topk[b].long()] for b in range(2)])
    rois = G.boxes_to_rois(boxes, rows, H, W)
    direct = _native.roi_align(gathered.to(DEV), rois.to(DEV), 56)
    want, info = R.roi_align_ref(gathered, rois, 56)
    bound = R.roi_align_bound(info, gathered)[:, None, None, None]
    assert (np.abs(out.detach().cpu().numpy() - direct.cpu().numpy()) <= bound).all()
    assert (np.abs(out.detach().cpu().double().numpy() - want) <= bound).all()
    out.backward(gout.to(DEV))
    assert torch.equal(level0.grad, run(boxes, rows, topk, gout, C, H, W))
    assert torch.equal(level0.grad, _native.roi_align_backward(gout.to(DEV), bx, rw, tk, C, H, W))
    assert not bx.requires_grad and bx.grad is None
