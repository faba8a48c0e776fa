"""FPN level 0 with shared lateral terms (fpn0x_kernel class pairs): the second
member of a position-class pair starts from the first member's lateral-1
accumulators, so a pair must stay on one workgroup, in order, whatever the
batch size and the number of epochs the persistent grid takes.

Shape: 200 x 152 images -> level 0 of 100 x 76, a 25 x 19 lateral-1 grid: two
row blocks per image, the second one partial (475 = 256 + 219 pixels).  B = 28
is 56 row blocks = 448 slots: more than one epoch on a 256-CU device; B = 1, 2
and 3 take the small-launch schedule (10 slots per row block, one epoch).
Tolerances are those of test_gpu_parity.test_odd_size_vs_oracle (split
precision: feat0 rtol / atol 1e-5, keypoints 1e-5, heatmaps 5e-5)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import kpd_oracle as O

H, W, B = 200, 152, 28
HF, WF = H // 2, W // 2


def _dev():
    return torch.device("cuda:0")


def _model(sd, full_level0):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig(), precision="split")
    m.load_state_dict(sd)
    m.full_level0 = full_level0
    return m.to(_dev()).eval()


def _feat(m, n):
    f = m.native_plan(_dev()).debug_buffer("feat0").view(n, HF, WF, 128)
    return f.permute(0, 3, 1, 2).cpu().clone()


@pytest.fixture(scope="module")
def case(model_sd):
    """Inputs, the oracle's forward (once) and the full-map GPU forward of the batch."""
    from dll.models.synthetic import synthetic_boxes, synthetic_images
    img = synthetic_images(B, 3, H, W, seed=77)
    boxes = synthetic_boxes(B, 1, seed=78)
    ref = O.forward(model_sd, {"image": img, "bboxes": boxes}, return_debug=True)
    m = _model(model_sd, True)
    with torch.no_grad():
        m({"image": img.to(_dev()), "bboxes": boxes.to(_dev())})
    torch.cuda.synchronize()
    feat = _feat(m, B)
    scores = m.native_plan(_dev()).debug_buffer("scores").view(B, 128).cpu().clone()
    return {"img": img, "boxes": boxes, "ref": ref, "model": m, "feat": feat, "scores": scores}


def _assert_feat(got, want, what):
    """rtol / atol 1e-5, reported per position class (y % 4, x % 4)."""
    err = (got - want).abs() / (1e-5 + 1e-5 * want.abs())
    worst = {(a, b): float(err[:, :, a::4, b::4].max()) for a in range(4) for b in range(4)}
    print(what, "max error / tolerance per class:", {k: round(v, 3) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: classes over tolerance (error / tolerance): {bad}"


@pytest.mark.gpu
def test_full_map_parity_across_epochs(case):
    _assert_feat(case["feat"], case["ref"]["_feat0"], f"B={B}")


@pytest.mark.gpu
def test_full_map_parity_one_epoch(case, model_sd):
    m = case["model"]
    with torch.no_grad():
        m({"image": case["img"][:2].to(_dev()), "bboxes": case["boxes"][:2].to(_dev())})
    torch.cuda.synchronize()
    _assert_feat(_feat(m, 2), case["ref"]["_feat0"][:2], "B=2")


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, B // 2, B - 1])
def test_batch_and_epoch_independence(case, i):
    """Image i of the batch (first, middle, last row blocks) equals the image
    alone and in a batch of 3 (at position i % 3), bit for bit."""
    m, img, boxes = case["model"], case["img"], case["boxes"]
    with torch.no_grad():
        m({"image": img[i:i + 1].to(_dev()), "bboxes": boxes[i:i + 1].to(_dev())})
    torch.cuda.synchronize()
    assert torch.equal(_feat(m, 1)[0], case["feat"][i]), "alone"
    pos = i % 3
    idx = [(i + 5) % B, (i + 9) % B]
    idx.insert(pos, i)
    with torch.no_grad():
        m({"image": img[idx].to(_dev()), "bboxes": boxes[idx].to(_dev())})
    torch.cuda.synchronize()
    assert torch.equal(_feat(m, 3)[pos], case["feat"][i]), "batch of 3"


@pytest.mark.gpu
def test_topk_and_statistics(case, model_sd):
    """The channel statistics stay per class: scores (atol 1e-6 as in
    test_forward_main_vs_golden) and top-64 index sets of every image."""
    want = O.channel_scores(case["ref"]["_feat0"], model_sd)
    np.testing.assert_allclose(case["scores"].numpy(), want.numpy(), atol=1e-6)
    topk = case["scores"].topk(64, dim=1).indices
    for n in range(B):
        assert set(topk[n].tolist()) == set(case["ref"]["_topk"][n].tolist()), f"image {n}"


@pytest.mark.gpu
def test_footprint_stores_vs_oracle(case, model_sd):
    """One box per image, level 0 stored only inside the ROI-align footprints."""
    m = _model(model_sd, False)
    with torch.no_grad():
        out = m({"image": case["img"].to(_dev()), "bboxes": case["boxes"].to(_dev())})
    ref = case["ref"]
    np.testing.assert_allclose(out["keypoints"].cpu().numpy(), ref["keypoints"].numpy(), atol=1e-5)
    np.testing.assert_allclose(out["heatmap"].cpu().numpy(), ref["heatmap"].numpy(), atol=5e-5)


def test_class_table_pairs():
    """Host side of the packing: pair members share a weight block, corners and
    first members have their own, 26 distinct group blocks in all."""
    from dll import _native
    lib = _native.load()
    ng = (ctypes.c_int * 16)()
    g = (ctypes.c_int * 64)()
    woff = (ctypes.c_int * 16)()
    blocks = ctypes.c_int()
    assert lib.kpd_fpn0x_class_table(ng, g, woff, ctypes.byref(blocks)) == 0
    ng, g, woff = list(ng), [list(g)[c * 4:c * 4 + 4] for c in range(16)], list(woff)
    cls = lambda a, b: a * 4 + b
    pairs = [(cls(1, b), cls(2, b)) for b in range(4)] + [(cls(0, 1), cls(0, 2)), (cls(3, 1), cls(3, 2))]
    for first, second in pairs:
        assert woff[first] == woff[second] and ng[first] == ng[second] and g[first] == g[second], (first, second)
    seconds = {s for _, s in pairs}
    own = [c for c in range(16) if c not in seconds]
    assert len(own) == 10 and len({woff[c] for c in own}) == 10
    for c in (cls(0, 0), cls(0, 3), cls(3, 0), cls(3, 3)):
        assert ng[c] == 4 and sum(woff[c] == w for w in woff) == 1
    assert [ng[c] for c in range(16)] == [4, 2, 2, 4, 2, 1, 1, 2, 2, 1, 1, 2, 4, 2, 2, 4]
    assert blocks.value == sum(ng[c] for c in own) == 26
    # blocks are packed back to back: [128][ng][128] hi + lo f16 elements each
    order = sorted(own, key=lambda c: woff[c])
    assert woff[order[0]] == 0
    for c, nxt in zip(order, order[1:]):
        assert woff[nxt] - woff[c] == 128 * ng[c] * 128 * 2
