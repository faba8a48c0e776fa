"""The split-precision scale arithmetic when weight and input magnitudes move
(DESIGN.md §5e).

precision="split" derives power-of-two scales from weights (w_exp, bc / bs,
the lateral-chain bound) and activations (per-image maxima, per-ROI hsc
bounds).  A bound that is too small turns an f16 hi into inf; one that is too
loose, or a clamp, pushes lo into f16 subnormals.  Every other parity test
draws one set of weights (seed 0) and only ever scales images up.

* Function-preserving variants (tests/scale_variants.py): the seed-0
  references stay valid bit for bit (tests/test_scale_variants.py) while
  every exponent inside the split kernels moves by k.  Bars as in
  test_dispatch_paths; the outputs are also bit-identical to the seed-0 GPU
  outputs (the scales are exact powers of two), except past the +-100 clamp.
* Function-changing weights and input magnitudes: the oracle with the same
  state dict / image, float64 for level 0 and the scores.  A "full" case first
  hard-asserts on that reference that the smallest adjacent score gap over
  ranks 1..65 is >= 4e-6, twice what two scores inside the 1e-6 bar can
  close, so the top-64 *order* (which channel feeds which conv weight) is
  decided by the reference, not by rounding.  A "level-0 only" case (taps,
  level 0, scores, top-64 set) needs that of the rank 64 / 65 gap only.

All forwards: precision="split" (two fp32 controls), full_level0, the dispatch
cases' inputs (synthetic_images(seed = 1000 + 7 H + W), two boxes per image).
"""
import pytest
import torch

import scale_variants as V
import test_dispatch_paths as D
from oracle import kpd_oracle as O

pytestmark = pytest.mark.gpu
DEV = D.DEV

SMALL, LARGE = "128x96", "512x384"
LATERAL_TOKENS = {SMALL: ["lateral_chain:split:small+reuse", "level0:fpn0x:tpc1"],
                  LARGE: ["lateral:per_level", "lat0:split_rows", "lat1:split_rows", "level0:fpn0x:tpc12"]}
MIN_GAP = 4e-6


def _sd64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _reference(sd, img, boxes):
    """The oracle for one state dict and batch: float64 taps, level 0, scores; O.forward outputs."""
    sd64 = _sd64(sd)
    taps = O.mbv3_small_taps(img.double(), sd64)
    feat0 = O.fpn_level(O.fpn_laterals(taps, sd64)[0], sd64, 0)
    scores = O.channel_scores(feat0, sd64)
    return {"taps": taps, "feat0": feat0, "scores": scores, "topk": scores.topk(64, dim=1).indices,
            "out": O.forward(sd, {"image": img, "bboxes": boxes})}


def _gaps(scores):
    """Per image: the smallest adjacent gap of the sorted scores over ranks 1..65, and the rank 64 / 65 gap."""
    v = scores.sort(dim=1, descending=True).values
    d = v[:, :64] - v[:, 1:65]
    return d.min(dim=1).values.tolist(), d[:, 63].tolist()


def _forward(model, img, boxes):
    """One forward with the path log on: tokens, debug buffers (NCHW, on the host) and outputs."""
    from dll._native import _level_sizes
    B, _, H, W = img.shape
    plan = model.native_plan(DEV)
    plan.path_log(True)
    with torch.no_grad():
        out = model({"image": img.to(DEV), "bboxes": boxes.to(DEV)})
    torch.cuda.synchronize()
    sizes = _level_sizes(H, W)
    r = {"tokens": plan.paths(), "taps": []}
    for i, (c, lv) in enumerate(zip(D.TAP_CH, D.TAP_LEVEL)):
        h, w = sizes[lv]
        r["taps"].append(plan.debug_buffer(f"tap{i}").view(B, h, w, -1)[..., :c].permute(0, 3, 1, 2).cpu().contiguous())
    h0, w0 = sizes[0]
    r["feat0"] = plan.debug_buffer("feat0").view(B, h0, w0, 128).permute(0, 3, 1, 2).cpu().contiguous()
    r["scores"] = plan.debug_buffer("scores").view(B, 128).cpu().clone()
    r["out"] = {k: out[k].cpu().clone() for k in ("keypoints", "visibilities", "heatmap")}
    plan.path_log(False)
    return r


def _run(sd, img, boxes, precision="split"):
    m = D._model(sd, precision)
    try:
        return _forward(m, img, boxes)
    finally:
        del m


def _check(label, got, ref, gain=0, full=True, tokens=("hm:hmconv:split",)):
    """The bars of test_dispatch_paths; level 0 is compared after the variant's
    exact gain 2^gain is taken out, so the bar means what it means at seed 0."""
    missing = [t for t in tokens if not any(D._matches(t, x) for x in got["tokens"])]
    assert not missing, f"{label}: not logged {missing}; paths {got['tokens']}"
    feat0 = torch.ldexp(got["feat0"], torch.tensor(-gain))
    rep = {f"tap{i}": D._ratio(got["taps"][i], ref["taps"][i], D.TAP_TOL) for i in range(4)}
    rep["feat0"] = D._ratio(feat0, ref["feat0"], D.FEAT_TOL)
    rep["scores"] = float((got["scores"].double() - ref["scores"]).abs().max()) / 1e-6
    if full:
        out, want = got["out"], ref["out"]
        rep["keypoints"] = float((out["keypoints"] - want["keypoints"]).abs().max()) / 1e-5
        rep["heatmap"] = float((out["heatmap"] - want["heatmap"]).abs().max()) / 5e-5
    print(f"\n{label} max error / tolerance:", {k: round(v, 3) for k, v in rep.items()})
    for k in ("taps", "feat0", "scores"):
        t = got[k] if k != "taps" else torch.cat([x.flatten() for x in got[k]])
        assert torch.isfinite(t).all(), f"{label}: non-finite {k}"
    bad = {k: v for k, v in rep.items() if not v <= 1.0}
    assert not bad, f"{label}: over tolerance (error / tolerance) {bad}"
    topk = got["scores"].topk(64, dim=1).indices
    for n in range(topk.shape[0]):
        assert set(topk[n].tolist()) == set(ref["topk"][n].tolist()), f"{label}: top-64 set of image {n}"
    if full:
        assert torch.equal(got["out"]["visibilities"], ref["out"]["visibilities"]), f"{label}: visibilities"
    return rep


def _bit_diff(got, base, gain=0):
    """The quantities of a variant's forward that are not bit-identical to the seed-0 forward's."""
    diff = [f"tap{i}" for i in range(4) if not torch.equal(got["taps"][i], base["taps"][i])]
    if not torch.equal(torch.ldexp(got["feat0"], torch.tensor(-gain)), base["feat0"]):
        diff.append("feat0")
    if not torch.equal(got["scores"], base["scores"]):
        diff.append("scores")
    return diff + [k for k in ("keypoints", "visibilities", "heatmap") if not torch.equal(got["out"][k], base["out"][k])]


PRESERVING = [(SMALL, n) for n in V.VARIANTS] + [(LARGE, n) for n in V.LARGE_VARIANTS]


@pytest.mark.parametrize("cid,name", PRESERVING, ids=[f"{c}-{n}" for c, n in PRESERVING])
def test_function_preserving_variant(model_sd, cid, name):
    """Seed-0 references; every scale exponent of the split kernels moved by the variant's k."""
    ref, base = D._ref(cid, model_sd), D._run(cid, "split", model_sd)
    got = _run(V.variant(model_sd, name), ref["img"], ref["boxes"])
    _check(f"{cid} {name}", got, ref, V.gain_of(name), tokens=["hm:hmconv:split"] + LATERAL_TOKENS[cid])
    diff = _bit_diff(got, base, V.gain_of(name))
    assert not diff, f"{cid} {name}: not bit-identical to the seed-0 forward: {diff}"


@pytest.mark.parametrize("name", ["fpn+40", "gain+24"])
def test_fp32_control(model_sd, name):
    """precision="fp32" has no scales: a failure here means the test is wrong, not a split kernel."""
    ref = D._ref(SMALL, model_sd)
    got = _run(V.variant(model_sd, name), ref["img"], ref["boxes"], "fp32")
    _check(f"{SMALL} {name} fp32", got, ref, V.gain_of(name), tokens=["hm:conv:k3", "hm:final:separate"])
    assert "hm:hmconv:split" not in got["tokens"]


@pytest.mark.parametrize("name", list(V.CLAMP_VARIANTS))
def test_clamp_reach(model_sd, name):
    """fpn k = +90: level-0 conv weights of ~2^-92 put the weight exponent
    14 - e at 104 / 105, clamped to 100 (pack_fpn0x).  k = -90 and -96: the
    bound on |lateral 1| of ~2^-85 / 2^-91 puts split_exp_of at 98 (not yet
    clamped: bit-identical to seed 0) and at 104, clamped to 100.  A clamp
    lowers the common product exponent P, so both operands keep 4-5 fewer bits
    below their hi: the bars hold, bit-identity with seed 0
    cannot and is printed, not asserted."""
    ref, base = D._ref(SMALL, model_sd), D._run(SMALL, "split", model_sd)
    got = _run(V.variant(model_sd, name), ref["img"], ref["boxes"])
    _check(f"{SMALL} {name}", got, ref, tokens=["hm:hmconv:split"] + LATERAL_TOKENS[SMALL])
    print(f"{SMALL} {name} not bit-identical to seed 0:", _bit_diff(got, base))


def _changed_weights(model_sd, case):
    from dll.configs import ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_state_dict
    if case.startswith("seed"):
        m = MultiPersonKeypointModel(ModelConfig(), TrainingConfig())
        return synthetic_state_dict(m.state_dict(), seed=int(case[4:]))
    sd = {k: v.clone() for k, v in model_sd.items()}
    key = f"backbone.fpn.lateral_convs.{case[3:]}.weight"
    sd[key] = sd[key] * 2.0 ** -8
    return sd


def _vs_own_oracle(label, sd, img, boxes, full):
    ref = _reference(sd, img, boxes)
    gmin, g64 = _gaps(ref["scores"])
    print(f"\n{label} score gaps over ranks 1..65 (fp64): min {['%.2e' % g for g in gmin]}, "
          f"64/65 {['%.2e' % g for g in g64]}")
    assert min(gmin if full else g64) >= MIN_GAP, f"{label}: the reference's own score gaps do not decide the top-64"
    got = _run(sd, img, boxes)
    _check(label, got, ref, full=full, tokens=["hm:hmconv:split"] + LATERAL_TOKENS[SMALL])
    return got, ref


# seed 3: 6.9e-7 between two ranks below 64 on image 1 -- the order inside the
# top 64 is not decided at the 1e-6 bar, the set (rank 64 / 65: 9.5e-4) is
@pytest.mark.parametrize("case,full", [("seed1", True), ("seed2", True), ("lat1", True), ("lat3", True),
                                       ("seed3", False)])
def test_function_changing_weights(model_sd, case, full):
    """Other weight draws, and one lateral 256 x quieter than its neighbours
    (lat1: lateral 1's own term; lat3: the coarsest term of the chain's bound)."""
    ref0 = D._ref(SMALL, model_sd)
    _vs_own_oracle(f"{SMALL} {case}", _changed_weights(model_sd, case), ref0["img"], ref0["boxes"], full)


def _magnitude_images(img):
    return {"zero": torch.zeros_like(img[:1]), "const": torch.full_like(img[:1], 0.7),
            "x2^-4": img * 2.0 ** -4, "x2^-8": img * 2.0 ** -8}


@pytest.mark.parametrize("case,full", [("zero", True), ("const", True), ("x2^-4", True), ("x2^-8", False)])
def test_input_magnitude(model_sd, case, full):
    """Black, constant and low-contrast images, seed-0 weights (the per-image
    maxima behind fpn0x_exps and the lateral bound go to their floor: an
    all-zero image's stem output is the folded BN bias alone)."""
    ref0 = D._ref(SMALL, model_sd)
    img = _magnitude_images(ref0["img"])[case]
    _vs_own_oracle(f"{SMALL} {case}", model_sd, img, ref0["boxes"][:img.shape[0]], full)


def test_mixed_magnitude_batch(model_sd):
    """B = 5: [image 0, zeros, constant 0.7, image 0 x 2^-4, image 1 x 4].  Every
    image against the oracle, and every image's keypoints and heatmap
    bit-identical to the same image run alone: the scales are per image."""
    ref0 = D._ref(SMALL, model_sd)
    img, boxes = ref0["img"], ref0["boxes"]
    mags = _magnitude_images(img)
    batch = torch.cat([img[:1], mags["zero"], mags["const"], mags["x2^-4"][:1], img[1:2] * 4])
    bxs = boxes[[0, 0, 0, 0, 1]]
    got, _ = _vs_own_oracle(f"{SMALL} B=5 mixed magnitudes", model_sd, batch, bxs, True)
    m = D._model(model_sd, "split")
    for n in range(5):
        alone = _forward(m, batch[n:n + 1], bxs[n:n + 1])
        for k in ("keypoints", "heatmap", "visibilities"):
            assert torch.equal(alone["out"][k][0], got["out"][k][n]), f"image {n}: {k} alone vs in the batch"
        assert torch.equal(alone["feat0"][0], got["feat0"][n]), f"image {n}: level 0 alone vs in the batch"
