"""MultiPersonKeypointModel(flip_test=True) on the device.

In split and fp32 precision an image's result does not depend on the batch it
ran in, so a flip-test forward is bit-identical to two plain forwards plus
dll.utils.flip_merge; and because the fp32 addition of the merge commutes, the
merged heatmap of the mirrored input is bit for bit the mirror-swap of the
merged heatmap of the original -- an equivariance a plain forward does not have
(stride-2 convolutions and aligned=False ROI-align are not mirror-symmetric),
which the last assertion of the equivariance test pins as well.

Box coordinates are multiples of 1/64, so mirroring them (1 - cx) is exact and
mirroring twice returns the input.  Keypoints of the mirrored run are compared
with 1 - x within 2e-6: both sides are fp32 soft-argmax results of bit-mirrored
maps whose sums run in a different lane order (each within 1e-6 of the exact
value, tests/test_flip_merge.py).
"""
import pytest
import torch

import flip_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W = 96, 64                # a size tests/test_distributed.py's forwards run
BOXES = [[[32 / 64, 32 / 64, 24 / 64, 48 / 64], [20 / 64, 28 / 64, 16 / 64, 24 / 64]],
         [[40 / 64, 30 / 64, 32 / 64, 40 / 64], [0.0, 0.0, 0.0, 0.0]]]     # image 1: one zero-padded box
MERGED = ("heatmap", "keypoints", "visibilities")


def _model(sd, precision, **kw):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig(), precision=precision, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module", params=["split", "fp32"])
def setup(request, model_sd):
    """The models and the forwards every test below reads (none modifies them)."""
    from dll.models.synthetic import synthetic_images
    from dll.utils import mirror_boxes, mirror_images
    plain, flip = _model(model_sd, request.param), _model(model_sd, request.param, flip_test=True)
    x = synthetic_images(2, 3, H, W, seed=41).to(DEV)
    boxes = torch.tensor(BOXES, device=DEV)
    mx, mb = mirror_images(x).contiguous(), mirror_boxes(boxes)
    assert torch.equal(mirror_boxes(mb), boxes) and torch.equal(mirror_images(mx), x)
    with torch.no_grad():
        outs = {"plain": plain({"image": x, "bboxes": boxes}), "plain_mirrored": plain({"image": mx, "bboxes": mb}),
                "flip": flip({"image": x, "bboxes": boxes}), "flip_mirrored": flip({"image": mx, "bboxes": mb})}
    torch.cuda.synchronize()
    return dict(plain=plain, flip=flip, x=x, boxes=boxes, mx=mx, mb=mb, outs=outs)


def test_flip_test_off_changes_nothing(setup, model_sd):
    m = setup["plain"]
    assert m.flip_test is False
    off = _model(model_sd, m.precision, flip_test=False)
    with torch.no_grad():
        got = off({"image": setup["x"], "bboxes": setup["boxes"]})
    want = setup["outs"]["plain"]
    assert set(got) == set(want) == {"heatmap", "keypoints", "visibilities", "boxes"}
    for k in MERGED:
        assert torch.equal(got[k], want[k]), k
    # the attribute is settable, like full_level0
    off.flip_test = True
    with torch.no_grad():
        on = off({"image": setup["x"], "bboxes": setup["boxes"]})
    for k in MERGED + ("keypoint_peaks",):
        assert torch.equal(on[k], setup["outs"]["flip"][k]), k


def test_flip_test_equals_two_forwards_and_the_merge(setup):
    from dll.utils import flip_merge
    outs = setup["outs"]
    want = flip_merge(outs["plain"]["heatmap"], outs["plain_mirrored"]["heatmap"], setup["boxes"])
    got = outs["flip"]
    assert set(got) == {"heatmap", "keypoints", "visibilities", "keypoint_peaks", "boxes"}
    for k in MERGED + ("keypoint_peaks",):
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert got["keypoints"].shape == (2, 2, 1, 17, 2) and got["visibilities"].shape == (2, 2, 1, 17, 3)
    assert not torch.equal(got["heatmap"], outs["plain"]["heatmap"])         # the mirrored pass does contribute
    # the padding slot of image 1 as the forward writes it
    for k in MERGED:
        assert not got[k][1, 1].any() and not outs["plain"][k][1, 1].any(), k
    assert not got["keypoint_peaks"][1, 1].any() and (got["keypoint_peaks"][1, 0] > 0).all()
    assert got["boxes"] is not None and torch.equal(torch.stack(list(got["boxes"])), setup["boxes"])


def test_flip_test_is_mirror_equivariant(setup):
    a, b = setup["outs"]["flip"], setup["outs"]["flip_mirrored"]
    idx = R.flip_index(17)
    assert torch.equal(b["heatmap"], a["heatmap"][:, :, idx].flip(-1))
    assert torch.equal(b["keypoint_peaks"], a["keypoint_peaks"][:, :, idx])
    assert torch.equal(b["visibilities"], a["visibilities"][:, :, :, idx])
    ka, kb = a["keypoints"][:, :, 0, idx].double(), b["keypoints"][:, :, 0].double()
    live = torch.tensor([[True, True], [True, False]], device=DEV)
    inside = (ka[..., 0] > 0) & (ka[..., 0] < 1)
    assert inside[live].all()                                       # no clamp hides the mirror
    ex = ((1.0 - ka[..., 0]) - kb[..., 0]).abs()[live].max().item()
    ey = (ka[..., 1] - kb[..., 1]).abs()[live].max().item()
    print("mirror keypoints max|d| x", ex, "y", ey)
    assert ex <= 2e-6 and ey <= 2e-6
    assert not kb[1, 1].any()
    # a plain forward is not equivariant: this is what the merge adds
    p, pm = setup["outs"]["plain"], setup["outs"]["plain_mirrored"]
    assert not torch.equal(pm["heatmap"], p["heatmap"][:, :, idx].flip(-1))


def test_flip_test_detector_branch(setup):
    from dll.utils import flip_merge, mirror_boxes
    plain, flip, x, mx = setup["plain"], setup["flip"], setup["x"], setup["mx"]
    with torch.no_grad():
        p = plain({"image": x})
        f = flip({"image": x})
        bt = torch.stack(list(p["boxes"])).contiguous()
        second = plain({"image": mx, "bboxes": mirror_boxes(bt)})
    assert bt.shape == (2, plain.max_persons, 4) and (bt != 0).any()
    assert torch.equal(torch.stack(list(f["boxes"])), bt) and torch.equal(f["box_scores"], p["box_scores"])
    want = flip_merge(p["heatmap"], second["heatmap"], bt)
    for k in MERGED + ("keypoint_peaks",):
        assert torch.equal(f[k], want[k]), k


def test_keypoint_peaks_come_from_the_merge(setup):
    from dll.utils import keypoint_peaks
    out = setup["outs"]["flip"]
    got = keypoint_peaks(out)
    assert got is out["keypoint_peaks"] or torch.equal(got, out["keypoint_peaks"])
    assert torch.equal(got, out["heatmap"].amax((-2, -1)))
    plain = setup["outs"]["plain"]
    assert "keypoint_peaks" not in plain and torch.equal(keypoint_peaks(plain), plain["heatmap"].amax((-2, -1)))


def test_flip_test_loss_is_computed_on_the_merged_outputs(setup, model_sd):
    """A batch with targets (the trainer's validation call): the eval outputs are the merged ones and the loss is
    the loss of those, not of the straight pass."""
    precision = setup["plain"].precision
    m, ref = _model(model_sd, precision, flip_test=True), _model(model_sd, precision)     # fresh loss-balancer states
    g = torch.Generator().manual_seed(43)
    tg = {"keypoints": torch.rand(2, 2, 17, 2, generator=g).to(DEV),
          "visibilities": torch.randint(0, 3, (2, 2, 17), generator=g).to(DEV),
          "heatmaps": torch.rand(2, 2, 17, 56, 56, generator=g).to(DEV)}
    with torch.no_grad():
        out = m({"image": setup["x"], "bboxes": setup["boxes"], **tg})
        merged, straight = setup["outs"]["flip"], setup["outs"]["plain"]
        for k in MERGED + ("keypoint_peaks",):
            assert torch.equal(out[k], merged[k]), k
        exp = ref._compute_loss_and_metrics({k: merged[k] for k in MERGED}, {"image": setup["x"], **tg})
        other = _model(model_sd, precision)._compute_loss_and_metrics({k: straight[k] for k in MERGED},
                                                                      {"image": setup["x"], **tg})
    assert float(out["loss"]) == float(exp["loss"]) and float(out["loss"]) != float(other["loss"])
    for k in ("heatmap_loss", "coordinate_loss", "visibility_loss", "total_loss"):
        assert out[k] == exp[k], k


def test_flip_test_keeps_the_dual_head_outputs_and_the_empty_batch(setup, model_sd):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_state_dict
    precision = setup["plain"].precision
    m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig(), precision=precision, dual_head=True)
    m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0))
    m = m.to(DEV).eval()
    batch = {"image": setup["x"], "bboxes": setup["boxes"]}
    from dll.utils import flip_merge
    with torch.no_grad():
        off = m(batch)
        mirrored = m({"image": setup["mx"], "bboxes": setup["mb"]})
        m.flip_test = True
        on = m(batch)
        empty = m({"image": setup["x"], "bboxes": None})
    assert torch.equal(on["kh_keypoints"], off["kh_keypoints"]) and torch.equal(on["kh_visibilities"], off["kh_visibilities"])
    assert "keypoint_peaks" in on and not torch.equal(on["heatmap"], off["heatmap"])
    want = flip_merge(off["heatmap"], mirrored["heatmap"], setup["boxes"])
    for k in MERGED + ("keypoint_peaks",):      # both passes run with the dual-head flag: the flags select kernels
        assert torch.equal(on[k], want[k]), k
    # the all-empty batch returns early, unchanged
    assert set(empty) == {"keypoints", "visibilities", "heatmap", "boxes"} and not empty["heatmap"].any()
