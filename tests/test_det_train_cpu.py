"""The detector-training restatement (tests/det_train_ref.py) on
the CPU: the matching rules on hand-made cases, its closed-form gradients
against torch autograd in float64, and -- for every fixture the GPU tests use --
that the fp32 matching (the device's arithmetic) and the float64 matching agree
on every anchor, so a device mismatch there is a bug, not a rounding effect."""
import pytest
import torch

import det_train_ref as R
from det_train_cases import CASES, MAIN_SIZE, main_boxes

H, W = MAIN_SIZE
DTYPES = (torch.float64, torch.float32)


@pytest.fixture(scope="module")
def anchors():
    from dll.configs import PersonDetectionConfig
    from dll.models import PERSON_HEAD
    return PERSON_HEAD(PersonDetectionConfig()).anchors.clone()


def _abox(anchors, n):
    """Anchor n as a normalised cxcywh box (float64 -> fp32)."""
    return R.anchor_boxes(anchors, H, W, torch.float64)[n].to(torch.float32)


def _match1(anchors, rows, dtype):
    gt = torch.stack([torch.as_tensor(r, dtype=torch.float32) for r in rows])[None]
    return R.match(anchors, gt, 1, H, W, dtype=dtype)


N0 = (20 * 56 + 30) * 9 + 4      # cell (20, 30), the 64 x 64 anchor


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_gt_equal_to_an_anchor_takes_it(anchors, dtype):
    m = _match1(anchors, [_abox(anchors, N0)], dtype)
    a = m["assign"][0]
    assert int(a[N0]) == 0 and abs(float(m["gt_best"][0, 0]) - 1.0) < 1e-6
    assert int(m["n_pos"][0]) == int((a >= 0).sum()) >= 1
    # the same shape one cell away overlaps by (1 - s) / (1 + s), s = (192 / 56) / 64: ~0.90, positive too
    assert int(a[N0 + 9]) == 0 and int(a[N0 - 9]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_ignore_band(anchors, dtype):
    """A person-sized box: anchors whose best IoU lies in [0.4, 0.5) are ignored (-2) unless they tie the
    GT's maximum; below 0.4 they are negative."""
    m = _match1(anchors, [[0.5, 0.5, 0.3, 0.45]], dtype)
    a, iou = m["assign"][0], m["iou"][0][:, 0]
    gmax = float(m["gt_best"][0, 0])
    assert gmax >= 0.5
    band = (iou >= 0.4) & (iou < 0.5)
    assert int(band.sum()) > 0 and bool((a[band] == -2).all())
    assert bool((a[iou >= 0.5] == 0).all()) and bool((a[iou < 0.4] == -1).all())
    assert int((a == -2).sum()) == int(band.sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_small_box_gets_its_low_quality_set(anchors, dtype):
    """gmax < 0.4: the anchors within tie_eps of the maximum become positives, every other anchor stays negative."""
    m = _match1(anchors, [[0.41, 0.37, 0.03, 0.04]], dtype)
    a, iou = m["assign"][0], m["iou"][0][:, 0]
    gmax = float(m["gt_best"][0, 0])
    assert 0 < gmax < 0.4
    tie = iou >= gmax - 1e-5
    assert int(tie.sum()) >= 1 and bool((a[tie] == 0).all()) and bool((a[~tie] == -1).all())
    assert int(m["n_pos"][0]) == int(tie.sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_gts_claiming_one_anchor(anchors, dtype):
    box = _abox(anchors, N0)
    shrunk = box.clone()
    shrunk[2:] *= 0.9                                   # IoU 0.81 with the anchor
    assert int(_match1(anchors, [shrunk, box], dtype)["assign"][0, N0]) == 1      # the higher IoU wins
    assert int(_match1(anchors, [box, shrunk], dtype)["assign"][0, N0]) == 0
    assert int(_match1(anchors, [box, box], dtype)["assign"][0, N0]) == 0         # a tie: the lower slot


@pytest.mark.parametrize("dtype", DTYPES)
def test_absent_rows(anchors, dtype):
    """A zero row between valid rows keeps the slots of its neighbours; w = 0 and NaN rows are absent; G = 0
    and an image of absent rows only are all negative."""
    p, q = [0.4, 0.45, 0.3, 0.5], [0.62, 0.55, 0.25, 0.6]
    both = _match1(anchors, [p, q], dtype)["assign"][0]
    for absent in ([0, 0, 0, 0], [0.5, 0.5, 0.0, 0.4], [0.5, 0.5, 0.3, -0.1], [0.5, float("nan"), 0.3, 0.4]):
        m = _match1(anchors, [p, absent, q], dtype)
        a = m["assign"][0]
        assert not bool((a == 1).any()) and float(m["gt_best"][0, 1]) == 0.0
        assert torch.equal(torch.where(a == 2, torch.ones_like(a), a), both)
        only = _match1(anchors, [absent], dtype)
        assert bool((only["assign"] == -1).all()) and int(only["n_pos"][0]) == 0
    m = R.match(anchors, None, 2, H, W, dtype=dtype)
    assert tuple(m["assign"].shape) == (2, R.A) and bool((m["assign"] == -1).all()) and m["n_pos"].tolist() == [0, 0]
    m = R.match(anchors, torch.zeros(2, 0, 4), 2, H, W, dtype=dtype)
    assert bool((m["assign"] == -1).all())


def test_closed_form_gradients_equal_autograd():
    """loss_and_grads' closed forms against autograd of chain() in float64, with positives, ignored anchors
    and both smooth-L1 branches in play, and non-default hyper-parameters."""
    from dll.configs import PersonDetectionConfig
    from dll.models import PERSON_HEAD
    anchors = PERSON_HEAD(PersonDetectionConfig()).anchors
    g = torch.Generator().manual_seed(3)
    gt = main_boxes()
    assign = R.match(anchors, gt, 2, H, W)["assign"]
    assert int((assign >= 0).sum()) > 100 and int((assign == -2).sum()) > 100
    x = torch.randn(2, 3136, 128, generator=g)
    prm = [torch.randn(s, generator=g, dtype=torch.float64) * 0.1 for s in ((36, 128), (36,), (9, 128), (9,))]
    for kw in (dict(), dict(alpha=0.4, gamma=1.5, beta=0.5, box_weight=2.0)):
        leaves = [p.clone().requires_grad_(True) for p in prm]
        loss, cls_part, box_part = R.chain(x, *leaves, anchors, gt, assign, H, W, **kw)
        loss.backward()
        ref = R.loss_and_grads(x, *prm, anchors, gt, assign, H, W, **kw)
        assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        assert abs(ref["cls"] - float(cls_part.detach())) <= 1e-12 * abs(float(cls_part.detach()))
        assert abs(ref["box"] - float(box_part.detach())) <= 1e-12 * abs(float(box_part.detach()))
        d = torch.nn.functional.linear(x.double(), prm[0], prm[1])
        for name, leaf in zip(("g_box_w", "g_box_b", "g_cls_w", "g_cls_b"), leaves):
            err = float((ref[name] - leaf.grad).abs().max()) / float(leaf.grad.abs().max())
            assert err <= 1e-12, (name, err)
        assert float(d.abs().max()) > 1.0     # deltas beyond beta: the linear branch is exercised


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_and_float64_matchings_agree_on_every_gpu_fixture(anchors, name):
    B, (h, w), gt = CASES[name]
    m64 = R.match(anchors, gt, B, h, w, dtype=torch.float64)
    m32 = R.match(anchors, gt, B, h, w, dtype=torch.float32)
    differ = int((m64["assign"] != m32["assign"]).sum())
    print(f"{name}: positives {m64['n_pos'].tolist()} ignored {(m64['assign'] == -2).sum(dim=1).tolist()} "
          f"margins (thresholds, ties) {R.threshold_margin(m64)} differing anchors {differ}")
    assert differ == 0
    assert torch.equal(m64["n_pos"], m32["n_pos"])


def test_the_main_fixture(anchors):
    """The figures the GPU tests' main fixture was chosen by."""
    m = R.match(anchors, main_boxes(), 2, H, W)
    assert m["n_pos"].tolist() == [495, 177]
    assert (m["assign"] == -2).sum(dim=1).tolist() == [824, 618]
    thr, tie = R.threshold_margin(m)
    assert 3e-5 < thr < 4e-5 and tie > 1e-6


def test_init_detection_bias_and_loss_hyper_parameters():
    """cls_heads[0].bias = -log((1 - prior) / prior), the other heads and forward untouched; DetectionLoss
    rejects hyper-parameters the C entry would."""
    import math
    from dll.configs import PersonDetectionConfig
    from dll.losses import DetectionLoss
    from dll.models import PERSON_HEAD
    ph = PERSON_HEAD(PersonDetectionConfig())
    before = {k: v.clone() for k, v in ph.state_dict().items()}
    ph.init_detection_bias(0.01)
    after = ph.state_dict()
    assert [k for k in after if not torch.equal(after[k], before[k])] == ["cls_heads.0.bias"]
    assert torch.allclose(after["cls_heads.0.bias"], torch.full((9,), -math.log(99.0)))
    assert abs(float(torch.sigmoid(after["cls_heads.0.bias"][0])) - 0.01) < 1e-7
    for bad in (0.0, 1.0):
        with pytest.raises(ValueError):
            ph.init_detection_bias(bad)
    for kw in (dict(pos_thr=0.3, neg_thr=0.4), dict(beta=0.0), dict(alpha=1.5), dict(gamma=-1.0), dict(box_weight=-1.0)):
        with pytest.raises(ValueError):
            DetectionLoss(**kw)
    assert "beta=0.111111" in repr(DetectionLoss())


def test_train_cli_rejects_amp_with_the_detector(capsys):
    import sys
    from conftest import PKG
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    import train
    with pytest.raises(SystemExit) as e:
        train.parse_args(["--config", "c.yaml", "--data_dir", "d", "--output_dir", "o", "--train", "detector", "--amp"])
    assert e.value.code == 2 and "--train detector" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(["--config", "c.yaml", "--data_dir", "d", "--output_dir", "o", "--train", "trunk"])
