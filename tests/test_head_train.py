"""HeatmapHead in train mode on the device: forward and backward against a
float64 CPU replica (tests/head_train_ref.py), train -> eval hand-over to the
native plan, Dropout2d, and a short training run."""
import pytest
import torch

import head_train_ref as HR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 0.05   # test_short_training_run


def _head(dropout=0.0, seed=7):
    from dll.configs.model_config import HeatmapHeadConfig
    from dll.models.heatmap_head import HeatmapHead
    from dll.models.synthetic import synthetic_state_dict
    head = HeatmapHead(HeatmapHeadConfig(dropout_rate=dropout))
    sd = synthetic_state_dict(head.state_dict(), seed=seed)
    head.load_state_dict(sd)
    return head.to(DEV), sd


def _close(name, got, r64, r32):
    """4 x the error of the float32 CPU replica (different fp32 summation
    orders on the two sides), but not below 2e-5 * max|ref|."""
    got, r64 = got.detach().double().cpu().reshape(r64.shape), r64.detach()
    err = float((got - r64).abs().max())
    e32 = float((r32.detach().double() - r64).abs().max())
    scale = float(r64.abs().max())
    bound = max(4 * e32, 2e-5 * scale)
    print(f"{name}: native {err:.3e}  fp32 replica {e32:.3e}  scale {scale:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("shape", [(3, 64, 14, 14), (2, 64, 56, 56)], ids=["generic14", "split56"])
def test_train_forward_backward_parity(shape):
    """Heatmaps, attention weights, every parameter gradient, the running
    statistics and num_batches_tracked of a train-mode forward + backward
    (dropout 0, loss = mean squared error to a random target) against the
    float64 replica with the native ReLU masks (head.train_taps) forced.

    Measured on the MI355X (native error / float32 CPU replica's error /
    bound).  generic14: heatmaps 3.6e-6 / 1.3e-6 / 2.0e-5, attention weights
    7e-8 / 1e-7 / 1.6e-5, every gradient within its bound, the closest
    deconv_layers.0.bias (zero in exact arithmetic: 2.2e-9 / 3.4e-9 / 1.3e-8).
    split56: heatmaps 3.5e-6 / 1.8e-6 / 2.0e-5, every gradient within its
    bound, the closest channel_attention.fc.0.bias 2.9e-9 / 6.5e-10 / 1.3e-8;
    grad spatial_attention.conv.bias, which sums conv 1's dgrad over 401k
    elements, 1.8e-10 / 2.4e-10 / 1.29e-8.  (With weights of one sign in every
    output channel the split 3x3 path's one-signed accumulation error added
    up in that sum to 2.54e-8; dll.ops.conv3x3 alternates the sign over the
    output channels since)"""
    head, sd = _head()
    g = torch.Generator().manual_seed(shape[0] * 100 + shape[2])
    x = torch.rand(*shape, generator=g)
    target = torch.rand(shape[0], 17, shape[2], shape[3], generator=g)
    head.train()
    head.train_taps = []
    heat, (cw, sw) = head(x.to(DEV))
    ((heat - target.to(DEV)) ** 2).mean().backward()
    taps = head.train_taps
    assert len(taps) == 3 and not any(t.requires_grad for t in taps)
    masks = [(t > 0).cpu() for t in taps]

    ref = {}
    for dt in (torch.float64, torch.float32):
        p = HR.leaves(sd, dt)
        h, c, s, own = HR.forward(p, x, masks)
        ((h - target.to(dt)) ** 2).mean().backward()
        ref[dt] = (p, h, c, s, own)
    p64, h64, c64, s64, own64 = ref[torch.float64]
    p32, h32, c32, s32, _ = ref[torch.float32]
    for m, m64 in zip(masks, own64):   # the native masks are the float64 ones but for near-zero pre-activations
        assert float((m != m64).float().mean()) <= 1e-4
    _close("heatmaps", heat, h64, h32)
    _close("channel weights", cw, c64, c32)
    _close("spatial weights", sw, s64, s32)
    g64, g32 = HR.grads(p64), HR.grads(p32)
    named = dict(head.named_parameters())
    assert set(named) == set(g64)
    for k in sorted(g64):
        assert named[k].grad is not None, k
        _close("grad " + k, named[k].grad, g64[k], g32[k])
    bufs = dict(head.named_buffers())
    for bn in HR.BNS:
        for leaf in ("running_mean", "running_var"):
            got, want = bufs[f"{bn}.{leaf}"].double().cpu(), p64[f"{bn}.{leaf}"]
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), f"{bn}.{leaf}"
        assert int(bufs[bn + ".num_batches_tracked"]) == int(p64[bn + ".num_batches_tracked"]) == 1


def test_train_then_eval_serves_the_updated_head():
    """After one train forward + backward + SGD step, eval() differs from the
    eval output before the step (the plan was rebuilt from the new weights and
    running statistics) and equals the CPU oracle on the head's state dict."""
    from oracle import kpd_oracle as O
    head, _ = _head()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 64, 56, 56, generator=g)
    xd = x.to(DEV)
    head.eval()
    with torch.no_grad():
        before = head(xd)[0].clone()
    head.train()
    opt = torch.optim.SGD(head.parameters(), lr=0.1)
    heat, _ = head(xd)
    ((heat - 0.25) ** 2).mean().backward()
    opt.step()
    head.eval()
    with torch.no_grad():
        after, (cw, sw) = head(xd)
    torch.cuda.synchronize()
    assert float((after - before).abs().max()) > 1e-3
    sd = {"heatmap_head." + k: v.detach().cpu() for k, v in head.state_dict().items()}
    want = O.heatmap_head(x, sd)
    assert torch.allclose(after.cpu(), want, atol=5e-5, rtol=0), float((after.cpu() - want).abs().max())


def _dropout_run(seed):
    head, _ = _head(dropout=0.5)
    head.train()
    head.train_taps = []
    g = torch.Generator().manual_seed(8)
    x = torch.rand(4, 64, 14, 14, generator=g).to(DEV)
    torch.manual_seed(seed)
    heat, _ = head(x)
    ((heat - 0.25) ** 2).mean().backward()
    return heat.detach(), {k: p.grad for k, p in head.named_parameters()}, head.train_taps, x


def test_dropout_planes_and_seed():
    """dropout_rate 0.5: every (roi, channel) plane of the first two taps is
    all zero or untouched (tap 0: bit-equal to twice the dropout-free tap), the
    zeroed share of the 4 x 256 planes lies in [0.35, 0.65], and the same
    torch.manual_seed gives bit-identical outputs and gradients."""
    heat, grads, taps, x = _dropout_run(3)
    free, _ = _head(dropout=0.0)
    free.train()
    free.train_taps = []
    with torch.no_grad():
        free(x)
    full0 = free.train_taps[0] * 2.0
    assert float((full0.flatten(2).abs().amax(dim=2) == 0).float().mean()) < 0.01   # no plane is zero by itself
    for i in (0, 1):
        zero = taps[i].flatten(2).abs().amax(dim=2) == 0
        share = float(zero.float().mean())
        print(f"tap {i}: {share:.3f} of the planes zeroed")
        assert 0.35 <= share <= 0.65
        if i == 0:
            kept = ~zero
            assert torch.equal(taps[0][kept], full0[kept])
    heat2, grads2, _, _ = _dropout_run(3)
    assert torch.equal(heat, heat2)
    differing = [k for k in grads if not torch.equal(grads[k], grads2[k])]
    assert not differing, differing
    heat3, _, _, _ = _dropout_run(4)
    assert not torch.equal(heat, heat3)


def test_short_training_run():
    """4 ROIs at 14 x 14, targets from generate_target_heatmap (sigma 1),
    AdaptiveHeatmapLoss, plain SGD, 10 steps, dropout 0.  The learning rate
    0.05 was chosen with the float64 CPU replica: its loss falls from
    2.108353e-01 (step 0) to 1.164119e-01 (step 10), below 0.8 x the start
    (measured native: 2.108353e-01 to 1.164120e-01).  The
    native per-step losses stay within 10 x the deviation of the float32 CPU
    replica from the float64 one (not below 1e-5 relative), and the native
    loss falls below 0.8 x its start."""
    from dll.losses import AdaptiveHeatmapLoss
    from dll.models.heatmap_head import generate_target_heatmap
    from oracle import loss_oracle as LO
    head, sd = _head()
    g = torch.Generator().manual_seed(21)
    x = torch.rand(4, 64, 14, 14, generator=g)
    kp = torch.rand(4, 17, 2, generator=g) * 0.8 + 0.1
    gt_dev = generate_target_heatmap(kp.to(DEV), (14, 14), sigma=1.0)
    gt = gt_dev.cpu()

    head.train()
    crit = AdaptiveHeatmapLoss()
    opt = torch.optim.SGD(head.parameters(), lr=LR)
    xd = x.to(DEV)
    native = []
    for _ in range(11):
        opt.zero_grad(set_to_none=True)
        loss = crit(head(xd)[0], gt_dev)
        loss.backward()
        opt.step()
        native.append(loss.detach())
    native = [float(v) for v in torch.stack(native).cpu()]

    runs = {}
    for dt in (torch.float64, torch.float32):
        p = HR.leaves(sd, dt)
        runs[dt] = []
        for _ in range(11):
            heat = HR.forward(p, x)[0]
            loss = LO.adaptive_heatmap_loss(heat, gt)
            runs[dt].append(float(loss.detach()))
            loss.backward()
            HR.sgd_step(p, LR)
    r64, r32 = runs[torch.float64], runs[torch.float32]
    print("float64 replica:", " ".join(f"{v:.6e}" for v in r64))
    print("native:         ", " ".join(f"{v:.6e}" for v in native))
    assert r64[10] < 0.8 * r64[0]
    for k in range(11):
        bound = max(10 * abs(r32[k] - r64[k]), 1e-5 * abs(r64[k]))
        print(f"step {k}: native dev {abs(native[k] - r64[k]):.3e}  fp32 replica dev {abs(r32[k] - r64[k]):.3e}")
        assert abs(native[k] - r64[k]) <= bound, f"step {k}: {abs(native[k] - r64[k]):.3e} > {bound:.3e}"
    assert native[10] < 0.8 * native[0]
