"""Detector training on the device: kpd_detector_targets,
kpd_detector_loss and kpd_detector_features against the float64 restatement
tests/det_train_ref.py.  Each check is paired with the bug it catches.

  matching   assign and n_pos equal the restatement exactly on every fixture of
             det_train_cases (B 1 / 2 / 3 / 5, G 0 / 1 / 3 / 64, two image
             sizes -- the anchor normalisation depends on W and H; absent rows
             of every kind), and each image of a batch matches as it does alone
             (a per-batch maximum or count leaking between images).
             test_det_train_cpu.py shows fp32 and float64 agree on all of them.
  loss       the loss triple and the four gradients against float64, the error
             per tensor normalised by max|ref|.  Yardstick: the same formulas by
             torch in fp32 on the CPU (det_train_ref.chain + autograd) on the
             same inputs against the same reference, computed here.  The device
             may use 4 x the yardstick (its summation order over B * 3136 cells
             differs), with a floor of 8 fp32 ulps of max|ref|.  B = 5 is 280
             row blocks on a grid capped at 256 workgroups: workgroups 0..23 own
             two blocks (the register accumulation across blocks).
  features   kpd_detector_features against float64 adaptive_avg_pool2d of the
             "feat0" debug copy of a forward, at the level-0 bar 1e-5 + 1e-5
             |ref| (FEAT_TOL of test_detector_paths.py), at level-0 sizes 17 x
             17, 56 x 56, 100 x 76 and 128 x 96; the float64 heads and decode
             on these features reproduce the forward's "pd_boxes" at that bar
             (a cell order or a pooling bin that differs from the eval path's).
  SGD        five plain-SGD steps (lr 1e-3) on the main fixture through
             dll.ops.detector_loss against a float64 replica run here: loss and
             parameters after every step under the same 4 x rule, the loss
             falling at every step.

Measured on the MI355X (relative to max|ref|; device / fp32 torch chain; also
in DESIGN.md §3j):
  main fixture (B = 2, positives [495, 177], float64 loss 67.860074):
    loss 5.0e-8 / 6.2e-8, class part 1.0e-8 / 1.0e-8, box part 4.7e-8 / 4.7e-8,
    g_box_w 4.8e-8 / 9.2e-8, g_box_b 2.4e-8 / 1.1e-7, g_cls_w 4.1e-8 / 1.9e-7,
    g_cls_b 2.2e-8 / 5.5e-8
  B = 5, G = 3: loss 1.0e-8 / 1.0e-8, gradients 3.0e-8 .. 5.9e-8 / 8.1e-8 .. 2.0e-7
  B = 1, G = 64: loss 7.2e-9 / 7.2e-9, gradients 1.4e-8 .. 3.9e-8 / 5.7e-8 .. 2.0e-7
  the bar was the 8-ulp floor (4.8e-7 .. 9.5e-7) in every case
  five SGD steps: float64 and device 67.86 60.50 53.70 47.50 41.85 36.68;
    parameters after the fifth step 4.8e-8 .. 1.7e-7 / the same to three digits
  pooled features: at most 0.012 of the level-0 bar; candidates from them 0.20
"""
import numpy as np
import pytest
import torch

import det_train_ref as R
from det_train_cases import CASES, MAIN_SIZE, main_boxes
from detector_ref import NUM_CANDIDATES, candidates

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FEAT_TOL = 1e-5
GRADS = ("g_box_w", "g_box_b", "g_cls_w", "g_cls_b")
_CACHE = {}


def _model():
    if "model" not in _CACHE:
        from dll.configs import ModelConfig, TrainingConfig
        from dll.models import MultiPersonKeypointModel
        from dll.models.synthetic import synthetic_state_dict
        m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig(), streams=1)
        sd = synthetic_state_dict(m.state_dict(), seed=0)
        m.load_state_dict(sd)
        _CACHE["model"] = (m.to(DEV).eval(), sd)
    return _CACHE["model"]


def _params(sd):
    p = "person_detector."
    return [sd[p + "box_heads.0.weight"].reshape(36, 128), sd[p + "box_heads.0.bias"],
            sd[p + "cls_heads.0.weight"].reshape(9, 128), sd[p + "cls_heads.0.bias"]]


def _pooled(B, size, seed=1234):
    """The device's own pooled features of B seeded images (device tensor), once per (B, size)."""
    key = ("pooled", B, size, seed)
    if key not in _CACHE:
        from dll.models.synthetic import synthetic_images
        m, _ = _model()
        with torch.no_grad():
            _CACHE[key] = m.native_plan(DEV).detector_features(synthetic_images(B, 3, *size, seed=seed).to(DEV))
    return _CACHE[key]


def _ref_match(name):
    key = ("match", name)
    if key not in _CACHE:
        _, sd = _model()
        B, (H, W), gt = CASES[name]
        _CACHE[key] = R.match(sd["person_detector.anchors"], gt, B, H, W)
    return _CACHE[key]


def _dev_targets(gt, B, size, **kw):
    from dll import _native
    m, _ = _model()
    return _native.detector_targets(m.person_detector.anchors, None if gt is None else gt.to(DEV), B, size, **kw)


def _check(name, dev, chain32, ref):
    """The 4 x-of-the-fp32-chain rule on one tensor (or scalar); prints both errors."""
    dev, chain32, ref = (torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in (dev, chain32, ref))
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert float(dev.abs().max()) == 0.0, name
        return 0.0, 0.0
    e_dev = float((dev - ref).abs().max()) / scale
    e_32 = float((chain32 - ref).abs().max()) / scale
    floor = 8 * float(np.spacing(np.float32(scale))) / scale
    print(f"  {name}: device {e_dev:.2e}  fp32 chain {e_32:.2e}  bar {max(4 * e_32, floor):.2e}  (max|ref| {scale:.3e})")
    assert e_dev <= max(4 * e_32, floor), f"{name}: device {e_dev:.3e} > max(4 x {e_32:.3e}, {floor:.3e})"
    return e_dev, e_32


@pytest.mark.parametrize("name", sorted(CASES))
def test_matching_equals_the_restatement(name):
    B, size, gt = CASES[name]
    ref = _ref_match(name)
    assign, n_pos, best = _dev_targets(gt, B, size, want_best=True)
    assert torch.equal(n_pos.cpu(), ref["n_pos"]), (n_pos.cpu().tolist(), ref["n_pos"].tolist())
    differ = int((assign.cpu() != ref["assign"]).sum())
    assert differ == 0, f"{differ} anchors differ"
    if gt is not None:
        assert float((best.cpu().double() - ref["gt_best"]).abs().max()) <= 1e-6
    if B > 1:   # each image alone
        for b in range(B):
            a1, n1, _ = _dev_targets(None if gt is None else gt[b:b + 1], 1, size)
            assert torch.equal(a1[0], assign[b]) and int(n1[0]) == int(n_pos[b]), b


def test_matching_thresholds_are_arguments():
    """Non-default thresholds reach the kernel: pos 0.6 / neg 0.3 / tie 1e-3 against the restatement (fp32 and
    float64 agree on it: checked here, before the device is asked)."""
    _, sd = _model()
    gt, (H, W) = main_boxes(), MAIN_SIZE
    kw = dict(pos_thr=0.6, neg_thr=0.3, tie_eps=1e-3)
    ref = R.match(sd["person_detector.anchors"], gt, 2, H, W, **kw)
    assert torch.equal(ref["assign"], R.match(sd["person_detector.anchors"], gt, 2, H, W, dtype=torch.float32,
                                              **kw)["assign"])
    assign, n_pos, _ = _dev_targets(gt, 2, MAIN_SIZE, **kw)
    assert torch.equal(assign.cpu(), ref["assign"]) and torch.equal(n_pos.cpu(), ref["n_pos"])
    assert not torch.equal(ref["assign"], _ref_match("main")["assign"])


def _loss_case(name, **hyper):
    from dll import _native
    m, sd = _model()
    B, size, gt = CASES[name]
    H, W = size
    x = _pooled(B, size)
    ref_m = _ref_match(name)
    assign, n_pos, _ = _dev_targets(gt, B, size)
    assert torch.equal(assign.cpu(), ref_m["assign"])
    prm = _params(sd)
    kw = dict(alpha=hyper.get("alpha", 0.25), gamma=hyper.get("gamma", 2.0), beta=hyper.get("beta", 1.0 / 9))
    bw = hyper.get("box_weight", 1.0)
    loss, grads = _native.detector_loss(x, *[p.to(DEV) for p in prm], m.person_detector.anchors,
                                        None if gt is None else gt.to(DEV), assign, n_pos, size,
                                        box_weight_factor=bw, **kw)
    xc = x.cpu()
    ref = R.loss_and_grads(xc, *prm, sd["person_detector.anchors"], gt, ref_m["assign"], H, W, box_weight=bw, **kw)
    leaves = [p.clone().float().requires_grad_(True) for p in prm]
    c32 = R.chain(xc, *leaves, sd["person_detector.anchors"], gt, ref_m["assign"], H, W, box_weight=bw,
                  dtype=torch.float32, **kw)
    c32[0].backward()
    return loss.cpu(), [g.cpu() for g in grads], ref, [float(v.detach()) for v in c32], [l.grad for l in leaves]


@pytest.mark.parametrize("name,hyper", [("main", {}), ("b5_g3", {}), ("b1_g64", {}),
                                        ("main", dict(alpha=0.4, gamma=1.5, beta=0.5, box_weight=2.0))],
                         ids=["main", "b5_g3", "b1_g64", "main_hyper"])
def test_loss_and_gradients_against_float64(name, hyper):
    loss, grads, ref, c32, g32 = _loss_case(name, **hyper)
    print(f"{name} {hyper}: float64 loss {ref['loss']:.6f} (class {ref['cls']:.6f}, box {ref['box']:.6f}), N {ref['n']}")
    for k, key in enumerate(("loss", "cls", "box")):
        _check(key, float(loss[k]), c32[k], ref[key])
    for key, g, gc in zip(GRADS, grads, g32):
        assert tuple(g.shape) == tuple(ref[key].shape)
        _check(key, g, gc, ref[key])


def test_loss_only_and_repeat_calls_are_bit_identical():
    from dll import _native
    m, sd = _model()
    B, size, gt = CASES["b5_g3"]
    x, prm = _pooled(B, size), [p.to(DEV) for p in _params(sd)]
    assign, n_pos, _ = _dev_targets(gt, B, size)
    args = (x, *prm, m.person_detector.anchors, gt.to(DEV), assign, n_pos, size)
    l1, g1 = _native.detector_loss(*args)
    l2, g2 = _native.detector_loss(*args)
    l0, g0 = _native.detector_loss(*args, want_grad=False)
    assert g0 is None and torch.equal(l0, l1) and torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    a2, n2, _ = _dev_targets(gt, B, size)
    assert torch.equal(a2, assign) and torch.equal(n2, n_pos)


def test_a_batch_without_labels_is_all_negative():
    """G = 0 (NULL boxes): N = 1, so the loss is the plain sum of the negatives' focal terms; the box part and
    the box gradients are exactly 0."""
    loss, grads, ref, c32, g32 = _loss_case("b3_g0")
    assert ref["n"] == 1 and ref["box"] == 0.0
    assert float(loss[2]) == 0.0 and float(loss[0]) == float(loss[1])
    assert float(grads[0].abs().max()) == 0.0 and float(grads[1].abs().max()) == 0.0
    _check("loss", float(loss[0]), c32[0], ref["loss"])
    _check("g_cls_w", grads[2], g32[2], ref["g_cls_w"])
    _check("g_cls_b", grads[3], g32[3], ref["g_cls_b"])


@pytest.mark.parametrize("H,W,B", [(34, 34, 2), (112, 112, 2), (200, 152, 2), (256, 192, 1)],
                         ids=["17x17", "56x56", "100x76", "128x96"])
def test_detector_features(H, W, B):
    from dll.models.synthetic import synthetic_images
    m, sd = _model()
    img = synthetic_images(B, 3, H, W, seed=900 + H + W).to(DEV)
    with torch.no_grad():
        m(img)                                               # the eval detector: level 0 at every pixel
    plan = m.native_plan(DEV)
    Hf, Wf = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    feat0 = plan.debug_buffer("feat0").view(B, Hf, Wf, 128).permute(0, 3, 1, 2).cpu()
    pd_boxes = plan.debug_buffer("pd_boxes").view(B, NUM_CANDIDATES, 4).cpu()
    x = plan.detector_features(img)
    assert tuple(x.shape) == (B, 3136, 128)
    x = x.cpu()
    ref = torch.nn.functional.adaptive_avg_pool2d(feat0.double(), (56, 56)).permute(0, 2, 3, 1).reshape(B, 3136, 128)
    err = (x.double() - ref).abs()
    worst = float((err / (FEAT_TOL + FEAT_TOL * ref.abs())).max())
    print(f"pooled features: worst error / bar {worst:.3f}")
    assert worst <= 1.0
    # the float64 heads and decode on these features give the forward's own candidates
    boxes, _ = candidates(x.reshape(B, 56, 56, 128).permute(0, 3, 1, 2), sd, H, W, torch.float64)
    worst = float(((pd_boxes.double() - boxes).abs() / (FEAT_TOL + FEAT_TOL * boxes.abs())).max())
    print(f"candidates from the features: worst error / bar {worst:.3f}")
    assert worst <= 1.0
    # images are independent, and a repeat is bit-identical
    assert torch.equal(plan.detector_features(img[:1]).cpu()[0], x[0])
    assert torch.equal(plan.detector_features(img).cpu(), x)


def test_five_sgd_steps_follow_the_float64_replica():
    """Plain SGD, lr 1e-3, on the main fixture through dll.ops.detector_loss.  The float64 replica's losses
    (start of each step, then after the last) 67.86, 60.50, 53.70, 47.50, 41.85, 36.68."""
    from dll.ops import detector_loss
    m, sd = _model()
    H, W = MAIN_SIZE
    gt, lr = main_boxes(), 1e-3
    x = _pooled(2, MAIN_SIZE)
    xc, anchors = x.cpu(), sd["person_detector.anchors"]
    assign = _ref_match("main")["assign"]
    shapes = [(36, 128, 1, 1), (36,), (9, 128, 1, 1), (9,)]
    dev = [p.clone().reshape(s).to(DEV).requires_grad_(True) for p, s in zip(_params(sd), shapes)]
    p64 = [p.clone().double() for p in _params(sd)]
    p32 = [p.clone().float().requires_grad_(True) for p in _params(sd)]
    losses = {"dev": [], "f64": [], "f32": []}
    for step in range(6):
        loss = detector_loss(x, *dev, m.person_detector.anchors, gt.to(DEV), (H, W))
        assert torch.equal(loss.assign.cpu(), assign)
        ref = R.loss_and_grads(xc, *p64, anchors, gt, assign, H, W)
        c32 = R.chain(xc, *p32, anchors, gt, assign, H, W, dtype=torch.float32)
        losses["dev"].append(float(loss.detach()))
        losses["f64"].append(ref["loss"])
        losses["f32"].append(float(c32[0].detach()))
        print(f"step {step}:")
        _check("loss", losses["dev"][-1], losses["f32"][-1], ref["loss"])
        _check("cls part", float(loss.cls_part), float(c32[1].detach()), ref["cls"])
        _check("box part", float(loss.box_part), float(c32[2].detach()), ref["box"])
        for key, a, b, c in zip(GRADS, dev, p32, p64):
            _check("param of " + key, a.detach().cpu().reshape(c.shape), b.detach(), c)
        if step == 5:
            break
        loss.backward()
        c32[0].backward()
        with torch.no_grad():
            for a, b, c, key in zip(dev, p32, p64, GRADS):
                a -= lr * a.grad
                b -= lr * b.grad
                c -= lr * ref[key]
                a.grad = b.grad = None
    print("float64:", " ".join(f"{v:.2f}" for v in losses["f64"]))
    print("device: ", " ".join(f"{v:.2f}" for v in losses["dev"]))
    assert [round(v, 2) for v in losses["f64"]] == [67.86, 60.50, 53.70, 47.50, 41.85, 36.68]
    assert all(b < a for a, b in zip(losses["dev"], losses["dev"][1:]))
    assert all(b < a for a, b in zip(losses["f64"], losses["f64"][1:]))


def test_arguments_are_checked_before_the_device():
    from dll import _native, ops
    m, sd = _model()
    anchors = m.person_detector.anchors
    with pytest.raises(ValueError, match="G must be"):   # (the binding caps G first: ask the C entry directly)
        _native.check(_native.load().kpd_detector_targets(_native._ptr(anchors), None, 1, 65, 256, 192, 0.5, 0.4, 1e-5,
                                                          None, None, None, None), "kpd_detector_targets")
    with pytest.raises(ValueError, match="at most 64"):
        _native.detector_targets(anchors, torch.zeros(1, 65, 4, device=DEV), 1, MAIN_SIZE)
    with pytest.raises(ValueError, match="neg_thr"):
        _native.detector_targets(anchors, torch.zeros(1, 1, 4, device=DEV), 1, MAIN_SIZE, pos_thr=0.5, neg_thr=0.6)
    x = _pooled(2, MAIN_SIZE)
    assign, n_pos, _ = _dev_targets(main_boxes(), 2, MAIN_SIZE)
    prm = [p.to(DEV) for p in _params(sd)]
    with pytest.raises(ValueError, match="beta"):
        _native.detector_loss(x, *prm, anchors, main_boxes().to(DEV), assign, n_pos, MAIN_SIZE, beta=0.0)
    with pytest.raises(_native.KpdNativeError, match="device tensor"):
        ops.detector_loss(x.cpu(), *prm, anchors, None, MAIN_SIZE)
