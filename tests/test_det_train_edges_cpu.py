"""Every precondition tests/test_det_train_edges.py leans on, on
the CPU: the capped low-quality band against the uncapped one, fp32 = float64
matching on every anchor of every edge case (so a device mismatch is a bug, not
rounding), that each case reaches what it is named for, and that the loss cases
saturate, split the smooth-L1 branches and plant their values as described."""
import math

import pytest
import torch

import det_train_edge_cases as E
import det_train_ref as R

A = R.A


def _both(name):
    m64, m32 = E.ref_match(name), E.ref_match(name, torch.float32)
    c = E.TIE_ZERO if name == "tie_zero" else E.MATCHING[name]
    differ = int((m64["assign"] != m32["assign"]).sum())
    print(f"{name}: positives {m64['n_pos'].tolist()} ignored {(m64['assign'] == -2).sum(dim=1).tolist()} "
          f"margins (thresholds, ties) {R.threshold_margin(m64, **c['kw'])} differing anchors {differ}")
    return m64, m32, c, differ


def test_every_older_fixture_stays_on_the_uncapped_rule():
    """min(tie_eps, gmax / 2) is tie_eps wherever gmax >= 2 tie_eps: every fixture of det_train_cases has
    gmax >= 0.0647 (0.065 to three places) on each present GT and is matched with tie_eps at most 1e-3, so its
    expectations stay bit for bit."""
    from det_train_cases import CASES, MAIN_SIZE, main_boxes
    lo = math.inf
    for name, (B, (h, w), gt) in CASES.items():
        if gt is None:
            continue
        m = R.match(E.anchors(), gt, B, h, w)
        lo = min(lo, float(m["gt_best"][R.present(gt)].min()))
    print(f"smallest gmax of a present GT over the older fixtures: {lo:.4f}")
    assert round(lo, 3) == 0.065                      # 0.0647: thirty times the 2e-3 the rule needs
    assert lo >= 2 * 1e-3
    m = R.match(E.anchors(), main_boxes(), 2, *MAIN_SIZE)
    assert m["n_pos"].tolist() == [495, 177] and (m["assign"] == -2).sum(dim=1).tolist() == [824, 618]


def test_a_sub_pixel_box_claims_its_tie_set_not_the_image():
    """A person in slot 0 and a dot of side 1e-3 ... 1e-5 in slot 1.  Uncapped (gmax - tie_eps), the dot's band
    reaches IoU 0 once gmax < tie_eps and every anchor turns positive; capped at gmax / 2 the positives do not
    depend on the side: the person's, plus the smallest-area anchors that contain the dot."""
    counts, dots = [], []
    for s in E.TINY_SIDES:
        m64, m32, c, differ = _both(f"tiny_{s:g}")
        assert differ == 0
        counts.append(int(m64["n_pos"][0]))
        dots.append(m64["assign"][0] == 1)
        gmax = m64["gt_best"][0]
        uncapped = ((gmax[None, :] > 0) & (m64["iou"][0] >= gmax[None, :] - 1e-5)).any(dim=1)
        print(f"  side {s:g}: gmax {float(gmax[1]):.3e}, the dot's anchors {int(dots[-1].sum())}, "
              f"uncapped low-quality set {int(uncapped.sum())}")
        if float(gmax[1]) < 1e-5:
            assert int(uncapped.sum()) == A           # the defect this rule replaces
        assert not bool((m64["assign"][E.present_iou_zero(m64, c["gt"])] >= 0).any())
    assert len(set(counts)) == 1 and all(torch.equal(d, dots[0]) for d in dots), counts
    alone = R.match(E.anchors(), E.tiny_boxes(1e-3)[:, :1], 1, *E.MAIN)
    assert int(dots[0].sum()) > 100 and counts[0] > int(alone["n_pos"][0])
    assert float(E.ref_match("tiny_0.0003")["gt_best"][0, 1]) < 1e-5 < float(E.ref_match("tiny_0.001")["gt_best"][0, 1])


def _reach_thr_equal(m, c):
    best = torch.stack([i.max(dim=1).values for i in m["iou"]])
    assert int(((best >= 0.4) & (best < 0.5)).sum()) > 100 and not bool((m["assign"] == -2).any())


def _reach_neg_zero(m, c):
    a = m["assign"]
    assert bool(((a[0] >= 0) | (a[0] == -2)).all()) and int((a[0] == -2).sum()) > 20000 and bool((a[1] == -1).all())
    assert int((m["iou"][0].max(dim=1).values == 0).sum()) > 1000      # best = 0 = neg_thr: still ignored


def _reach_tie_wide(m, c):
    assert int(m["n_pos"][0]) > int(E.ref_match("thr_default")["n_pos"][0])


def _reach_pos_09(m, c):
    a = m["assign"][0]
    assert int(a[E.N0]) == 0 and int(a[E.N0 + 9]) == -2 and int(m["n_pos"][0]) < int((a == -2).sum())
    assert float(m["iou"][0][:, 1].max()) < 0.9 and int((a == 1).sum()) >= 1      # Q lives on its tie set


def _reach_slot63(m, c):
    a = m["assign"][0]
    assert int(m["n_pos"][0]) > 20 and bool(((a == 63) | (a < 0)).all())


def _reach_dup(m, c):
    a = m["assign"][0]
    assert int(m["n_pos"][0]) > 20 and bool((a[a >= 0] == 0).all()) and float(m["gt_best"][0, 63]) >= 0.5
    only = E.ref_match("slot63_only")["assign"][0]
    assert torch.equal(a, torch.where(only == 63, torch.zeros_like(only), only))


def _reach_slots_62_63(m, c):
    a = m["assign"][0]
    assert int((a == 62).sum()) > 20 and int((a == 63).sum()) > 20 and not bool(((a >= 0) & (a < 62)).any())
    assert float(m["gt_best"][0, :62].abs().max()) == 0.0


def _reach_nonfinite(m, c):
    two = R.match(E.anchors(), E.image(2, {0: E.P, 1: E.Q})[None], 1, *E.MAIN)["assign"][0]
    a = m["assign"][0]
    assert float(m["gt_best"][0, 1:4].abs().max()) == 0.0 and float(m["gt_best"][1].abs().max()) == 0.0
    assert not bool(((a >= 1) & (a <= 3)).any()) and int((a == 4).sum()) > 20
    assert torch.equal(torch.where(a == 4, torch.ones_like(a), a), two)
    assert bool((m["assign"][1] == -1).all()) and int(m["n_pos"][1]) == 0
    assert bool(R.present(c["gt"])[0].all()) and R.present(c["gt"])[1].tolist() == [True, True, False, True, False]


def _reach_corners(m, c):
    a = m["assign"]
    assert int((a[0, A - 64:] >= 0).sum()) >= 8 and int((a[2, :64] >= 0).sum()) >= 8
    assert int(m["n_pos"][1]) == 0 and bool((a[1] == -1).all()) and bool((a[2][a[2] >= 0] == 1).all())


def _reach_sizes(m, c):
    assert all(int(n) >= 3 for n in m["n_pos"])


def _reach_default(m, c):
    a = m["assign"]
    assert all(int((a[b] >= 0).sum()) > 50 and int((a[b] == -2).sum()) > 100 for b in range(2))


REACH = {"thr_equal": _reach_thr_equal, "neg_zero": _reach_neg_zero, "tie_wide": _reach_tie_wide,
         "pos_09": _reach_pos_09, "slot63_only": _reach_slot63, "dup_0_63": _reach_dup,
         "slots_62_63": _reach_slots_62_63, "nonfinite": _reach_nonfinite, "corners": _reach_corners,
         "size_64x512": _reach_sizes, "size_512x64": _reach_sizes, "size_34x34": _reach_sizes,
         "thr_default": _reach_default}


@pytest.mark.parametrize("name", sorted(REACH))
def test_matching_case_preconditions(name):
    m64, m32, c, differ = _both(name)
    assert differ == 0 and torch.equal(m64["n_pos"], m32["n_pos"])
    assert torch.equal(m64["n_pos"], (m64["assign"] >= 0).sum(dim=1).int())
    assert not bool((m64["assign"][E.present_iou_zero(m64, c["gt"])] >= 0).any())
    REACH[name](m64, c)


def test_every_matching_case_has_its_precondition():
    assert set(REACH) | {f"tiny_{s:g}" for s in E.TINY_SIDES} == set(E.MATCHING)


def test_tie_eps_zero_sandwich_holds_for_the_restatement():
    """tie_eps = 0 keeps only exact maxima, which fp32 implementations may break differently: the device is held
    to best >= pos_thr from below and to the tie_eps = 1e-5 matching from above; both restatements obey it."""
    upper = E.ref_match("thr_default")["assign"] >= 0
    for dtype in (torch.float64, torch.float32):
        m = E.ref_match("tie_zero", dtype)
        pos = m["assign"] >= 0
        lower = torch.stack([i.max(dim=1).values >= 0.5 for i in m["iou"]])
        assert bool((pos | ~lower).all()) and bool((upper | ~pos).all())
        for b in range(2):
            for g in torch.nonzero(m["gt_best"][b] > 0).flatten().tolist():
                assert bool(pos[b][m["iou"][b][:, g] >= m["gt_best"][b, g] - 1e-6].any())
    assert int(upper.sum()) > int((E.ref_match("tie_zero")["assign"] >= 0).sum())     # the band matters here


# ---------------------------------------------------------------- loss
def test_the_grid_arithmetic_the_cases_are_named_for():
    def owned(B):
        nb = 56 * B
        nwg = min(nb, 256)
        return nwg, [len(range(w, nb, nwg)) for w in range(nwg)]
    nwg, own = owned(4)
    assert nwg == 224 and set(own) == {1} and nwg % 64 == 32
    nwg, own = owned(10)
    assert nwg == 256 and own[:48] == [3] * 48 and own[48:] == [2] * 208
    assert 264 % 256 == 8 and 524 % 256 == 12 and 524 // 256 == 2
    for B in (4, 10):
        c = E.grid_case(B)
        assert all(int(n) > 20 for n in c["n_pos"]) and int((c["assign"] == -2).sum()) > 100


def _ref_and_chain(c, dtype, n=None):
    kw = dict(c["hyper"])
    n = int(c["n_pos"].sum()) if n is None else n
    ref = R.loss_and_grads(c["x"], *c["prm"], E.anchors(), c["gt"], c["assign"], *c["size"], n=n, **kw)
    leaves = [p.clone().to(dtype).requires_grad_(True) for p in c["prm"]]
    out = R.chain(c["x"], *leaves, E.anchors(), c["gt"], c["assign"], *c["size"], dtype=dtype, n=n, **kw)
    out[0].backward()
    return ref, [float(v.detach()) for v in out], [l.grad for l in leaves]


def test_n_argument_scales_closed_forms_and_chain_alike():
    for n_pos in ((0, 0, 0), (1000, 0, 7)):
        c = E.n_pos_case(n_pos)
        assert int((c["assign"] >= 0).sum()) > 100 and c["n_pos"].tolist() == list(n_pos)
        ref, c64, g64 = _ref_and_chain(c, torch.float64)
        assert ref["n"] == max(1, sum(n_pos))
        own = R.loss_and_grads(c["x"], *c["prm"], E.anchors(), c["gt"], c["assign"], *c["size"])
        assert abs(ref["loss"] * ref["n"] - own["loss"] * own["n"]) <= 1e-12 * abs(own["loss"] * own["n"])
        assert abs(ref["loss"] - c64[0]) <= 1e-12 * abs(c64[0])
        for key, g in zip(E.GRADS, g64):
            assert float((ref[key] - g).abs().max()) <= 1e-12 * float(g.abs().max()), key


@pytest.mark.parametrize("cell", sorted(E.PLANT_CELLS))
def test_planted_value_lands_in_one_column(cell):
    base = E.planted_base()
    r0 = R.loss_and_grads(base["x"], *base["prm"], E.anchors(), base["gt"], base["assign"], *base["size"])
    b, i, j = E.PLANT_CELLS[cell]
    n = (i * 56 + j) * 9
    assert base["assign"][b, n:n + 9].tolist() == list(E.PLANT_LABELS)
    assert float(r0["g_box_w"].abs().max()) == 0.0 and float(r0["g_cls_w"].abs().max()) == 0.0
    ch = E.PLANT_CHANNELS[1]
    c1, cx = E.planted_case(cell, ch, 1.0), E.planted_case(cell, ch)
    assert int((cx["x"] != 0).sum()) == 1 and float(cx["x"][b, i * 56 + j, ch]) == E.PLANT_X
    r1 = R.loss_and_grads(c1["x"], *c1["prm"], E.anchors(), c1["gt"], c1["assign"], *c1["size"])
    rx = R.loss_and_grads(cx["x"], *cx["prm"], E.anchors(), cx["gt"], cx["assign"], *cx["size"])
    for key in ("g_box_w", "g_cls_w"):
        other = torch.ones(128, dtype=torch.bool)
        other[ch] = False
        assert float(rx[key][:, other].abs().max()) == 0.0
        assert torch.equal(rx[key][:, ch], r1[key][:, ch] * E.PLANT_X)      # (x is dyadic: the scaling is exact)
    # the column is that cell's 45 gradients: 6 positives x 4 deltas, and the 8 anchors that are not ignored
    assert int((rx["g_box_w"][:, ch] != 0).sum()) == 24 and int((rx["g_cls_w"][:, ch] != 0).sum()) == 8
    assert torch.equal(rx["g_box_b"], r0["g_box_b"]) and torch.equal(rx["g_cls_b"], r0["g_cls_b"])
    assert rx["loss"] == r0["loss"]


def test_saturation_cases_saturate():
    a = E.default_assign()
    groups = {"positives": a >= 0, "negatives": a == -1, "ignored": a == -2}
    z3, z10 = E.logits(E.saturation_case(3.0)), E.logits(E.saturation_case(10.0))
    print(f"max|z|: x3 {float(z3.abs().max()):.1f}, x10 {float(z10.abs().max()):.1f}")
    assert float(z3.abs().max()) > 88
    for name, mask in groups.items():
        hi, lo = int((z10[mask] > 104).sum()), int((z10[mask] < -104).sum())
        print(f"  x10 {name}: {hi} above 104, {lo} below -104 of {int(mask.sum())}")
        assert hi >= 5 and lo >= 5


def test_smooth_l1_cases_sit_on_their_branches():
    for kind, lo, hi in (("quadratic", 0.99, 1.0), ("linear", 0.0, 0.01), ("both", 0.2, 0.8)):
        c = E.smooth_l1_case(kind)
        r = E.box_residuals(c)
        share = float((r < c["hyper"]["beta"]).double().mean())
        print(f"{kind}: beta {c['hyper']['beta']:g}, {r.shape[0]} positives, quadratic share {share:.4f}")
        assert lo <= share <= hi


def test_label_cases():
    c = E.label_case("all_ignored")
    r = R.loss_and_grads(c["x"], *c["prm"], E.anchors(), c["gt"], c["assign"], *c["size"])
    assert r["loss"] == 0.0 and all(float(r[k].abs().max()) == 0.0 for k in E.GRADS) and c["n_pos"].tolist() == [0, 0]
    c = E.label_case("image_all_positive")
    assert int(c["n_pos"][0]) == A and 50 < int(c["n_pos"][1]) < A
    for kind, values, canon in (("too_large", {3, 1000, E.INT32_MAX}, -2), ("too_small", {-3, E.INT32_MIN}, -1)):
        odd, plain = E.label_case(kind)
        changed = odd["assign"] != plain["assign"]
        assert set(odd["assign"][changed].tolist()) == values and bool((plain["assign"][changed] == canon).all())
        assert int(changed.sum()) > 1000 and torch.equal(odd["n_pos"], plain["n_pos"])
        base = E.default_assign()
        assert int(((base >= 0) & changed).sum()) > 10      # positives among the replaced labels too
    c = E.extreme_target_case()
    t = R.box_targets(E.anchors(), c["gt"], c["assign"], *c["size"], torch.float64)
    print(f"extreme targets: log targets {float(t[..., 2:].min()):.2f} .. {float(t[..., 2:].max()):.2f}")
    assert float(t[..., 2:].min()) < -11 and float(t[..., 2:].max()) > 5 and bool(torch.isfinite(t).all())
    assert all(int((c["assign"] == g).sum()) > 100 for g in (0, 1, 2))
