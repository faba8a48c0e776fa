"""tests/detector_ref.py against the project's oracle (itself pinned to the
reference goldens): the references the GPU detector and NMS tests compare
with must restate oracle.kpd_oracle.person_detect / nms(stable=True) exactly."""
import torch

from detector_ref import NUM_CANDIDATES, candidates, greedy_nms
from oracle import kpd_oracle as O


def _dual_sd():
    from dll.configs import KeypointHeadConfig, ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_state_dict
    m = MultiPersonKeypointModel(ModelConfig(keypoint_head=KeypointHeadConfig(height=56, width=56)),
                                 TrainingConfig(), dual_head=True)
    return synthetic_state_dict(m.state_dict(), seed=0)


def test_candidates_and_nms_restate_person_detect():
    """64 x 64 images (level 0 of 32 x 32: upsampling bins): fp32 candidates
    thresholded and passed through greedy_nms equal O.person_detect bit for
    bit; the float64 candidates agree with the fp32 ones to fp32 rounding."""
    from dll.models.synthetic import synthetic_images
    sd = _dual_sd()
    H = W = 64
    feat = O.backbone_level0(synthetic_images(2, 3, H, W, seed=900 + H + W), sd)
    boxes, scores = candidates(feat, sd, H, W, torch.float32)
    assert boxes.shape == (2, NUM_CANDIDATES, 4) and scores.shape == (2, NUM_CANDIDATES)
    b64, s64 = candidates(feat.double(), sd, H, W, torch.float64)
    assert b64.dtype == torch.float64
    assert float(((boxes - b64).abs() / (1e-5 + 1e-5 * b64.abs())).max()) < 1.0
    assert float(((scores - s64).abs() / (1e-5 + 1e-5 * s64.abs())).max()) < 1.0
    for conf, iou, P in ((0.3, 0.3, 5), (0.0, 0.5, 64), (1.0, 0.3, 5)):
        ref_b, ref_s = O.person_detect(feat, sd, H, W, conf, iou, P)
        for b in range(2):
            idx = torch.nonzero(scores[b] > conf).flatten()
            keep, margin = greedy_nms(boxes[b, idx], scores[b, idx], iou, P)
            if len(idx):
                assert torch.equal(keep, O.nms(boxes[b, idx], scores[b, idx], iou, P, stable=True)), (conf, iou, P, b)
            exp_b, exp_s = torch.zeros(P, 4), torch.zeros(P)
            exp_b[:len(keep)] = boxes[b, idx[keep]]
            exp_s[:len(keep)] = scores[b, idx[keep]]
            assert torch.equal(exp_s, ref_s[b]), (conf, iou, P, b)
            if not torch.equal(exp_b, ref_b[b]):
                # O.person_detect sorts with torch's unstable sort: among exactly
                # tied scores it may keep the same boxes in another order
                assert P == 64 and (exp_s[1:] == exp_s[:-1]).any(), (conf, iou, P, b)
                assert sorted(exp_b.tolist()) == sorted(ref_b[b].tolist()), (conf, iou, P, b)
            assert (margin > 0) if len(idx) > 1 else (margin == float("inf"))
    assert float(ref_s.abs().max()) == 0.0   # conf = 1.0: nothing detected


def test_greedy_nms_vs_oracle_stable():
    """Random boxes with tied scores, -inf scores and both zeros: the same
    kept indices as O.nms(stable=True), with and without a limit; the margin
    is the distance of the closest compared IoU (float64) to the threshold."""
    g = torch.Generator().manual_seed(11)
    n = 700
    boxes = torch.rand(n, 4, generator=g) * torch.tensor([1.0, 1.0, 0.2, 0.2]) + torch.tensor([0.0, 0.0, 0.02, 0.02])
    scores = torch.randint(0, 40, (n,), generator=g).float() / 40          # many exact ties
    scores[100:140] = -float("inf")
    scores[200:220] = -0.0
    scores[220:240] = 0.0
    for thr, mo in ((0.3, 0), (0.3, 7), (0.5, 50), (0.0, 0)):
        keep, margin = greedy_nms(boxes, scores, thr, mo)
        assert torch.equal(keep, O.nms(boxes, scores, thr, mo if mo > 0 else None, stable=True)), (thr, mo)
        assert 0.0 <= margin < 1.0
    # two boxes, one comparison: the margin is that pair's |IoU - thr|
    two = torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.6, 0.5, 0.2, 0.2]])
    keep, margin = greedy_nms(two, torch.tensor([0.9, 0.8]), 0.3, 0)
    iou = float(O.box_iou_cxcywh(two[:1].double(), two[1:].double()))
    assert keep.tolist() == [0] and abs(iou - 1 / 3) < 1e-6
    assert abs(margin - abs(iou - float(torch.tensor(0.3, dtype=torch.float32)))) < 1e-12
    # signed zeros rank as equal: lower index first
    z = torch.tensor([[0.1, 0.1, 0.05, 0.05], [0.5, 0.5, 0.05, 0.05], [0.9, 0.9, 0.05, 0.05]])
    assert greedy_nms(z, torch.tensor([-0.0, 0.0, -0.0]), 0.3, 2)[0].tolist() == [0, 1]
    keep, margin = greedy_nms(z[:1], torch.tensor([0.5]), 0.3, 0)
    assert keep.tolist() == [0] and margin == float("inf")
