"""Plan.roi_features (kpd_roi_features): the trunk's ROI features exactly as
the fused forward serves them to HeatmapHead -- bit-equal to the forward's own
"roi" debug buffer, independent of which rows or images share the call, and
without effect on later eager or graph-replayed forwards."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(sd, precision):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig(), precision=precision)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _forward_roi(m, img, boxes):
    """The "roi" debug buffer of a model forward, as [R, 64, 56, 56]."""
    with torch.no_grad():
        m({"image": img, "bboxes": boxes})
    R = boxes.size(0) * boxes.size(1)
    return m.native_plan(DEV).debug_buffer("roi").view(R, 56, 56, 64).permute(0, 3, 1, 2).contiguous()


def _inputs():
    from dll.models.synthetic import synthetic_boxes, synthetic_images
    img = synthetic_images(2, 3, 256, 192, seed=31, device=DEV)
    boxes = synthetic_boxes(2, 2, seed=32, device=DEV).clone()
    boxes[1, 0] = 0          # one all-zero (padding) box
    return img, boxes


@pytest.mark.parametrize("precision", ["split", "fp32"])
def test_bit_equal_to_the_forward(model_sd, precision):
    m = _model(model_sd, precision)
    img, boxes = _inputs()
    want = _forward_roi(m, img, boxes)
    plan = m.native_plan(DEV)
    rows = [0, 1, 3]
    got = plan.roi_features(img, boxes, rows)
    assert tuple(got.shape) == (3, 64, 56, 56) and got.dtype == torch.float32
    assert torch.equal(got, want[rows])
    assert float(got.abs().max()) > 0
    # rows=None is the explicit full list (the padding box's row included, as the forward computes it)
    full = plan.roi_features(img, boxes)
    assert torch.equal(full, plan.roi_features(img, boxes, [0, 1, 2, 3]))
    assert torch.equal(full, want)
    # a device int32 tensor is read in place
    assert torch.equal(plan.roi_features(img, boxes, torch.tensor(rows, dtype=torch.int32, device=DEV)), got)
    assert tuple(plan.roi_features(img, boxes, []).shape) == (0, 64, 56, 56)


@pytest.mark.parametrize("precision", ["split", "fp32"])
def test_large_map_lateral_fallback(model_sd, precision):
    """480 x 384: the per-level lateral path of test_gpu_parity's case of the same name."""
    from dll.models.synthetic import synthetic_images
    m = _model(model_sd, precision)
    img = synthetic_images(1, 3, 480, 384, seed=9, device=DEV)
    boxes = torch.tensor([[[0.45, 0.55, 0.4, 0.7]]], device=DEV)
    want = _forward_roi(m, img, boxes)
    assert torch.equal(m.native_plan(DEV).roi_features(img, boxes, [0]), want)


def test_rows_do_not_depend_on_their_company(model_sd):
    m = _model(model_sd, "split")
    img, boxes = _inputs()
    plan = m.native_plan(DEV)
    full = plan.roi_features(img, boxes)
    for rows in ([3], [0, 3], [1, 3]):
        assert torch.equal(plan.roi_features(img, boxes, rows), full[rows]), rows
    # image 1 alone: its ROIs are rows 2, 3 of the pair
    alone = plan.roi_features(img[1:].contiguous(), boxes[1:].contiguous())
    assert torch.equal(alone, full[2:])
    with pytest.raises(ValueError):
        plan.roi_features(img, boxes[:1])


def test_forwards_are_unaffected(model_sd):
    """Five forwards on fixed tensors with graph replay on (eager, capture,
    replays), roi_features at another batch size in between, the forward
    again: every output bit-equal to the first forward's."""
    from dll.models.synthetic import synthetic_boxes, synthetic_images
    m = _model(model_sd, "split")
    img, boxes = _inputs()
    with torch.no_grad():
        ref = m({"image": img, "bboxes": boxes})
    plan = m.native_plan(DEV)
    kpts = torch.empty(2, 2, 1, 17, 2, device=DEV)
    vis = torch.empty(2, 2, 1, 17, 3, device=DEV)
    heat = torch.empty(2, 2, 17, 56, 56, device=DEV)

    def forward_and_check(tag):
        kpts.fill_(-1.0)
        heat.fill_(-1.0)
        plan.forward(img, boxes, kpts, vis, heat)
        torch.cuda.synchronize()
        assert torch.equal(kpts, ref["keypoints"]) and torch.equal(heat, ref["heatmap"]), tag
        assert torch.equal(vis, ref["visibilities"]), tag

    plan.set_graphs(True)
    try:
        for it in range(5):
            forward_and_check(("before", it))
        for B in (1, 3):      # a smaller batch (fits the carve) and a larger one (re-carves)
            img_b = synthetic_images(B, 3, 256, 192, seed=33, device=DEV)
            boxes_b = synthetic_boxes(B, 2, seed=34, device=DEV)
            x = plan.roi_features(img_b, boxes_b)
            assert tuple(x.shape) == (2 * B, 64, 56, 56) and bool(torch.isfinite(x).all())
            for it in range(3):
                forward_and_check(("after", B, it))
    finally:
        plan.set_graphs(False)
