"""The CPU side of the head-training edge tests (test_conv3_shapes.py,
test_loss_select_edges.py, test_bn_train_edges.py): every helper those files
lean on is tied to torch here, and every "the reference alone satisfies the
precondition" statement of theirs is checked without a device."""
import pytest
import torch

import bn_train_edges_cases as E
import bn_train_ref as R
import conv3_shapes_cases as K
import loss_select_cases as S


# ---------------------------------------------------------------- conv3: the shapes reach what they name
def test_conv_shapes_reach_the_named_edges():
    planes = {s: K.padded_plane(s) for s in K.SHAPES}
    assert planes[(1, 4, 6, 6, 4)] == 64 and planes[(1, 4, 5, 7, 4)] == 63 and planes[(1, 4, 6, 14, 4)] == 128
    assert sorted((s[3] + 2) % 4 for s in K.SHAPES if s[:3] == (2, 6, 3)) == [0, 1, 2, 3]
    chans = {s[1] for s in K.SHAPES} | {s[4] for s in K.SHAPES}
    assert {127, 128, 129, 257} <= chans
    assert any(-(-s[1] // 256) > 1 and -(-s[4] // 256) > 1 for s in K.SHAPES)     # tiles along both axes
    assert len(set(K.SHAPES)) == len(K.SHAPES)


@pytest.mark.parametrize("shape", K.PLACEMENT_SHAPES[:2], ids=K.shape_id)
def test_placement_expectations_are_torchs_float64(shape):
    """expect_wgrad / expect_forward / expect_dgrad against conv2d with autograd
    in float64, at every pixel placement the device tests use, on channels of
    its own choice (the 56 x 56 shape runs the same code on more pixels)."""
    N, C, H, W, O = shape
    w, b = K.dyadic_weights(shape)
    assert bool((w != 0).all()) and torch.equal(w * 8, (w * 8).round()) and float(w.abs().max()) <= 1.0
    assert torch.equal(w.to(torch.bfloat16).float(), w) and torch.equal(w.half().float(), w)
    seen = 0
    for k, (y, x) in enumerate(K.placements(H, W)):
        n, c, o = k % N, (k * 3) % C, (k * 5) % O
        xi = (n, c, y, x)
        x1 = K.onehot((N, C, H, W), xi)
        yr, _, _, _ = K.ref_split(x1, w, b, torch.zeros(N, O, H, W))
        assert torch.equal(K.expect_forward(shape, xi, w, b).double(), yr)
        g1 = K.onehot((N, O, H, W), (n, o, y, x))
        _, gxr, _, _ = K.ref_split(torch.zeros(N, C, H, W), w, b, g1)
        assert torch.equal(K.expect_dgrad(shape, (n, o, y, x), w).double(), gxr)
        for (yy, xx) in K.neighbours(H, W, y, x):
            gi = (n, o, yy, xx)
            _, _, gwr, gbr = K.ref_split(x1, w, b, K.onehot((N, O, H, W), gi))
            assert torch.equal(K.expect_wgrad(shape, xi, gi).double(), gwr)
            assert torch.equal(K.onehot((O,), o).double(), gbr)
            seen += int(gwr.sum().item())
    assert seen >= 4 * len(K.placements(H, W))          # most neighbours are taps; the far one is not


def test_placements_cover_corners_borders_and_interior():
    assert K.placements(56, 56) == [(y, x) for y in (0, 28, 55) for x in (0, 28, 55)]
    assert K.placements(2, 3) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    assert (0, 3) in K.neighbours(3, 4, 2, 0) or (0, 3) in K.neighbours(3, 4, 1, 1)   # a far position exists
    assert len(K.neighbours(56, 56, 28, 28)) == 10 and len(K.neighbours(56, 56, 0, 0)) == 5


# ---------------------------------------------------------------- loss: the select's inputs
@pytest.mark.parametrize("name", list(S.CASES))
def test_select_case_is_not_hidden_by_the_clamp(name):
    thr = S.check_band(name)
    from oracle import loss_oracle
    assert float(thr) == float(loss_oracle.adaptive_threshold(S.build(name).view(1, 1, 1, -1)))


@pytest.mark.parametrize("lo,hi,copies", [(0.17, 0.19, 0), (0.2, 0.2, 0), (0.2, 0.21, 1), (S._FF_LOW, 0.25, 3)])
@pytest.mark.parametrize("n", [1000, 4097, 12])
def test_planted_rank_is_what_torch_interpolates_from(n, lo, hi, copies):
    x, rank, lo_t, hi_t = S.planted(n, lo, hi, seed=n, copies_below=copies)
    v = torch.sort(x).values
    assert v[rank] == lo_t and v[rank + 1] == hi_t
    assert int((x == lo_t).sum()) == copies + 1 + int(float(lo_t) == float(hi_t))
    below, w = S.rank_of(n)
    assert below == rank and 0.0 < w < 1.0              # fractional rank: the successor is needed
    assert float(torch.quantile(x, S.Q)) == float(torch.lerp(lo_t, hi_t, torch.tensor(w)))


def test_key_bytes_of_the_planted_values():
    assert S.key(S._FF_LOW) & 0xFF == 0xFF and S.key(S.from_bits(S.bits(S._FF_LOW) + 1)) & 0xFF == 0
    assert (S.key(S._FF_SECOND) >> 8) & 0xFF == 0xFF and S.key(S._FF_SECOND) & 0xFF != 0xFF
    a, b = S.key(S._TOP_BYTE_LO), S.key(S._TOP_BYTE_HI)
    assert b == a + 1 and (a >> 24) != (b >> 24)
    # the key is order-preserving over both signs, zeros and denormals
    vals = [-3.0, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 0.1, 0.5]
    keys = [S.key(S.from_bits(S.bits(v))) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    x = S.build("zeros_denormals")
    odd = (x == 0) | ((x.abs() > 0) & (x.abs() < 2.0 ** -126))
    assert int(odd.sum()) == 800 and bool((x.view(torch.int32) == -2 ** 31).any())   # -0.0 is there
    c = S.build("consecutive_bits").view(torch.int32)
    assert int(c.max() - c.min()) == 999 and len(set(((c >> 8) & 0xFF).tolist())) > 1
    rank, _ = S.rank_of(1000)
    assert torch.sort(S.build("ff_low_byte")).values[rank].item() == S._FF_LOW
    assert torch.sort(S.build("ff_second_byte")).values[rank].item() == S._FF_SECOND


@pytest.mark.parametrize("alpha", [1.0, 0.5, 3.0])
def test_oracle_is_finite_for_the_powf_exponents(alpha):
    pred, gt = S.loss_inputs()
    assert float((pred - gt).abs().min()) >= 1e-2
    loss, grad = S.oracle_loss_and_grad(pred, gt, None, alpha)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0


def test_oracle_is_not_finite_at_zero_error_below_one():
    """Why the alpha < 1 case keeps pred away from gt: the reference's own gradient is NaN there."""
    _, gt = S.loss_inputs()
    _, grad = S.oracle_loss_and_grad(gt.clone(), gt, None, 0.5)
    assert not bool(torch.isfinite(grad).all())


# ---------------------------------------------------------------- BN: the far mean tells the algorithms apart
def _misses(err, bar):
    return bool((err > bar).any())


@pytest.mark.parametrize("mean,std", E.FAR_MEANS, ids=["1024+0.5", "-4096+2"])
def test_one_pass_float32_variance_fails_the_far_mean_bar(mean, std):
    c = E.far_case(mean, std)
    fw = R.forward(c["x"], c["gamma"], c["beta"], c["drop"], 1e-5, True)
    bw = R.backward(fw, c["gy"], c["gamma"])
    assert float((fw["mean"].abs() * fw["invstd"]).min()) > 1000          # |mean| / std in the thousands
    bar_y, _ = E.far_bars(fw, bw, c["gamma"], E.masked_gy(fw, c["gy"]))
    m1, s1 = E.one_pass_fp32_stats(c["x"])
    y1 = E.forward_with_stats(c["x"], c["gamma"], c["beta"], m1, s1, fw["mask"]) * fw["drop"]
    assert _misses((s1.double() - fw["invstd"]).abs().max(), 1e-5 * fw["invstd"].abs().max())
    assert _misses((y1 - fw["y"]).abs().amax(dim=(0, 2, 3)), bar_y)
    # the kernel's formulation -- double sums, mean and invstd stored as fp32, xhat in fp32 -- meets it
    m2, s2 = fw["mean"].float(), fw["invstd"].float()
    xhat = (c["x"] - m2.view(1, -1, 1, 1)) * s2.view(1, -1, 1, 1)
    y2 = torch.addcmul(c["beta"].view(1, -1, 1, 1), xhat, c["gamma"].view(1, -1, 1, 1)).double() * fw["mask"] * fw["drop"]
    assert not _misses((y2 - fw["y"]).abs().amax(dim=(0, 2, 3)), bar_y)
    # ggamma: the ideal fp32 evaluation misses the plain per-tensor 1e-5 (by 10.7 x and 5.2 x)
    # and meets ggamma_bar, the 1e-5 plus the mean's half ulp carried by gbeta
    _, _, gg, mask = E.ideal_fp32(c)
    fwm = R.forward(c["x"], c["gamma"], c["beta"], c["drop"], 1e-5, True, mask=mask)
    bwm = R.backward(fwm, c["gy"], c["gamma"])
    err_gg, plain_gg = (gg - bwm["ggamma"]).abs(), E.REL * bwm["ggamma"].abs().max()
    print(f"ideal fp32 ggamma: {float(err_gg.max() / plain_gg):.2f} x the plain bar, "
          f"{float((err_gg / E.ggamma_bar(fwm, bwm)).max()):.2f} of ggamma_bar")
    assert _misses(err_gg, plain_gg) and float(err_gg.max() / plain_gg) > 3
    assert not _misses(err_gg, E.ggamma_bar(fwm, bwm))
    pre64, band = E.kink_band(fw, c["gamma"], c["beta"])
    assert bool((pre64.abs() <= band)[mask.double() != fw["mask"]].all())


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
def test_two_values_per_channel_cannot_meet_a_bar_relative_to_gx(relu):
    """(1, 4097, 1, 2): with n = 2 the three terms of gx cancel to eps / (var + eps)
    of themselves.  The ideal fp32 evaluation on exact statistics misses 1e-5
    max|gx_c| (by three orders of magnitude) and 1e-5 max|y_c| in some channels,
    so no kernel with fp32 statistics meets them; it meets far_bars + cancel_bar,
    which is what the device is held to at this shape."""
    c = R.case(E.TWO_VALUES)
    y, gx, gg, mask = E.ideal_fp32(c, relu)
    fw = R.forward(c["x"], c["gamma"], c["beta"], c["drop"], 1e-5, relu, mask=mask if relu else None)
    bw = R.backward(fw, c["gy"], c["gamma"])
    g = E.masked_gy(fw, c["gy"])
    err_y, err_gx = ((a - b).abs().amax(dim=(0, 2, 3)) for a, b in ((y, fw["y"]), (gx, bw["gx"])))
    plain_y, plain_gx = (E.REL * t.abs().amax(dim=(0, 2, 3)) for t in (fw["y"], bw["gx"]))
    print(f"ideal fp32 over the plain bar: y {int((err_y > plain_y).sum())} channels (worst {float((err_y / plain_y.clamp_min(1e-300)).max()):.1f} x), "
          f"gx {int((err_gx > plain_gx).sum())} channels (worst {float((err_gx / plain_gx.clamp_min(1e-300)).max()):.1f} x)")
    assert _misses(err_y, plain_y) and _misses(err_gx, plain_gx)
    assert float((err_gx / plain_gx.clamp_min(1e-300)).max()) > 100
    bar_y, bar_gx = E.far_bars(fw, bw, c["gamma"], g)
    assert not _misses(err_y, bar_y)
    assert not _misses(err_gx, bar_gx + E.cancel_bar(fw, bw, c["gamma"], g))
    err_gg, plain_gg = (gg - bw["ggamma"]).abs(), E.REL * bw["ggamma"].abs().max()
    print(f"ideal fp32 ggamma: {float(err_gg.max() / plain_gg):.2f} x the plain bar, "
          f"{float((err_gg / E.ggamma_bar(fw, bw)).max()):.2f} of ggamma_bar")
    assert _misses(err_gg, plain_gg)                    # measured 1.16 x (relu), 1.08 x over
    assert not _misses(err_gg, E.ggamma_bar(fw, bw))
    # the mask of the ideal evaluation differs from float64 only inside kink_band
    fw64 = R.forward(c["x"], c["gamma"], c["beta"], c["drop"], 1e-5, relu)
    pre64, band = E.kink_band(fw64, c["gamma"], c["beta"])
    assert bool((pre64.abs() <= band)[mask.double() != fw64["mask"]].all())


def test_other_chunk_shapes_meet_the_plain_bar_in_the_ideal_evaluation():
    for shape in E.CHUNK_SHAPES[:5] + E.CHUNK_SHAPES[6:] + E.OFFSET_SHAPES:
        cc = R.case(shape)
        y, gx, _, mask = E.ideal_fp32(cc)
        f = R.forward(cc["x"], cc["gamma"], cc["beta"], cc["drop"], 1e-5, True, mask=mask)
        b = R.backward(f, cc["gy"], cc["gamma"])
        for got, ref in ((y, f["y"]), (gx, b["gx"])):
            assert not _misses((got - ref).abs().amax(dim=(0, 2, 3)), E.REL * ref.abs().amax(dim=(0, 2, 3))), shape


def test_chunk_shapes_sit_on_the_chunk():
    hw = [s[2] * s[3] for s in E.CHUNK_SHAPES]
    assert hw[:5] == [1023, 1025, 1028, 1024, 1028] and hw[2] % 4 == 0 and hw[0] % 4 and hw[1] % 4
    assert E.CHUNK_SHAPES[5] == E.TWO_VALUES and 4096 // E.CHUNK_SHAPES[5][1] == 0 and E.CHUNK_SHAPES[5][0] * hw[5] == 2
    assert all(s[2] * s[3] % 4 == 0 for s in E.OFFSET_SHAPES)
    N, C, H, W = E.CHUNK_SHAPES[6]                       # S = 3 chunks over G = 2 workgroups
    assert N * -(-H * W // 1024) == 3 and min(3, 4096 // C) == 2
