"""Every shape-dispatched path of the forward against a float64 reference.

The forward's stages pick between specialised kernels by image size and batch.  Each
case below is the smallest shape that reaches one group of those kernels; the
dispatch path log (kpd_plan_path_log) proves which kernels ran, so a later
change to a gate cannot move a case onto another kernel unnoticed.

Reference: the oracle's backbone in float64 (state dict and image cast to
double; the oracle is dtype-agnostic) for the taps, FPN level 0, the channel
scores and the top-64 sets; O.forward (fp32) for keypoints, visibilities and
heatmaps.  The fp32 oracle is within 0.04 (taps) / 0.20 (FPN levels) of an
rtol = atol = 1e-5 band of the fp64 one, so the bars measure the kernels.

Bars (error <= atol + rtol * |ref|):
  feat0         rtol = atol = 1e-5           test_gpu_parity.test_odd_size_vs_oracle
  scores        atol 1e-6
  keypoints     1e-5 (mixed 1e-3)            test_gpu_parity's module docstring
  heatmaps      5e-5 (mixed 3e-2)            same
  visibilities  identical (mixed: <= 2 % of keypoints flip)
  taps          rtol = atol = TAP_TOL = 2e-6 the tighter of 1e-4 (test_gpu_api's bar) and 4x
                                             the worst error measured over all cases, 0.047
                                             of a 1e-5 band (384 x 288), rounded up to one
                                             digit; 4x because the summation order differs
                                             per path and batch (DESIGN.md "Dispatch paths")
"""
import re

import pytest
import torch

from oracle import kpd_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

TAP_TOL = 2e-6
FEAT_TOL = 1e-5
TAP_CH = (16, 24, 48, 576)
TAP_LEVEL = (0, 3, 8, 11)

# id -> (H, W, B, precisions, tokens that must be logged, tokens that must not);
# "precision>token" holds in that precision only
CASES = {
    # seproj at 48 pixels on features.4-8 (no se_excite: C < 288), the 12-pixel
    # blocks fused without seproj, the small + reuse lateral chain, fpn0x tpc 1;
    # output maps under 12 columns: the two-column exdw kernels of every block
    "128x96": (128, 96, 2, ("split",),
               ["f1:dwsum+se16_proj", "f4:exdw+seproj:po48", "f5:exdw+seproj:po48", "f6:exdw+seproj:po48",
                "f7:exdw+seproj:po48", "f8:exdw+seproj:po48", "f4:seproj:m3:t1:w8",
                "f4:exdw:rt:k5s2:cs16:xt2", "f5:exdw:rt:k5s1:cs16:xt2", "f8:exdw:rt:k5s1:cs16:xt2",
                "f9:exdw:hs:k5s2:cs32:xt2", "f10:exdw:rt:k5s1:cs32:xt2", "f11:exdw:rt:k5s1:cs32:xt2",
                "f9:exdw+se_kernel+project", "f10:exdw+se_kernel+project", "f11:exdw+se_kernel+project",
                "lateral:chain", "lateral_chain:split:small+reuse", "level0:fpn0x:tpc1"],
               ["f4:se_excite", "f8:se_excite", "lat0:lateral_stream"]),
    # level 0 (125 x 95) is not 4x lateral 1 (32 x 24): lateral_stream with
    # non-integer nearest indexing, the fp32 level-0 conv, separate channel
    # statistics -- in split and mixed precision too; seproj po192 as at 256 x 192:
    # 16 x 12 outputs on the four-column hardswish exdw kernels, features.10 / 11
    # (4 x 3, with fc1 partials) on the two-column BL kernel
    "250x190": (250, 190, 2, ("fp32", "split", "mixed"),
                ["lat0:lateral_stream", "level0:conv", "fpn0:conv:k3", "topk:channel_stats",
                 "f4:exdw+seproj:po192", "f8:exdw+seproj:po192", "f4:seproj:m3:t3:w8",
                 "f4:exdw:hs:k5s2:cs16:xt4", "f5:exdw:hs:k5s1:cs16:xt4", "f8:exdw:hs:k5s1:cs16:xt4",
                 "f10:exdw:bl:xt2", "f11:exdw:bl:xt2",
                 "f9:exdw+seproj:po48", "f9:se_excite", "f9:seproj:m3:t2:w8", "lateral:chain",
                 "lateral_chain:fp32:small"],
                ["level0:fpn0x:tpc*", "level0:conv+stats", "lat0:split_rows"]),
    # features.4 reads 784 pixels, one 16-pixel tile over kFuseMaxPix: the generic
    # expand conv + dwconv + se_kernel + project; lateral 3 of 49 pixels: chain not small
    "224x224": (224, 224, 2, ("split",),
                ["f4:generic+se_kernel", "f5:exdw+se_kernel+project", "lateral:chain",
                 "lateral_chain:split:big", "level0:fpn0x:tpc4"],
                ["f4:exdw+seproj:po192", "f4:exdw+se_kernel+project", "lateral_chain:split:small+reuse"]),
    # features.1 output width 64: dwsum + se16_proj at its limit; in fp32 the
    # level-0 conv with the channel statistics in its epilogue (4096 pixels = 32 M-tiles)
    "64x256": (64, 256, 2, ("fp32", "split"),
               ["f1:dwsum+se16_proj", "split>level0:fpn0x:tpc1", "fp32>level0:conv+stats", "fp32>lat0:lateral_stream"],
               ["f1:generic+se_kernel", "topk:channel_stats"]),
    # width 65: features.1 on the generic chain; level 0 (32 x 130) not 4x lateral 1 (8 x 33)
    "64x260": (64, 260, 2, ("split",),
               ["f1:generic+se_kernel", "lat0:lateral_stream", "level0:conv"],
               ["f1:dwsum+se16_proj", "level0:fpn0x:tpc*"]),
    # the 384 x 288 geometry: 432- and 108-pixel SE maps, fused without seproj
    "384x288": (384, 288, 2, ("split",),
                ["f5:exdw+se_kernel+project", "f8:exdw+se_kernel+project", "f9:exdw+se_kernel+project",
                 "f11:exdw+se_kernel+project", "f4:generic+se_kernel", "lateral:chain", "level0:fpn0x:tpc7"],
                ["f5:exdw+seproj:po192", "f9:exdw+seproj:po48"]),
    # features.5-8 fused at exactly kFuseMaxPix = 768 pixels, seproj po192 +
    # se_excite (+ exdw_bl) on the 576-wide blocks, features.1 generic, lateral 3
    # of 192 pixels: per-level lateral convs + split_rows, fpn0x tpc 12;
    # features.9 writes 12 columns: its four-column (runtime-activation) exdw kernel
    "512x384": (512, 384, 1, ("split",),
                ["f1:generic+se_kernel", "f4:generic+se_kernel", "f5:exdw+se_kernel+project",
                 "f8:exdw+se_kernel+project", "f9:exdw+seproj:po192", "f10:exdw+seproj:po192",
                 "f11:exdw+seproj:po192", "f9:se_excite", "f10:se_excite", "f11:se_excite",
                 "f9:exdw:rt:k5s2:cs32:xt4", "f10:exdw:bl:xt4", "f11:exdw:bl:xt4", "lateral:per_level",
                 "lat0:split_rows", "lat1:split_rows", "level0:fpn0x:tpc12"],
                ["lateral:chain", "f1:dwsum+se16_proj"]),
    # lateral 3 of 2 x 2, SE maps of 4 pixels, every level odd, level 0 (17 x 17) not 4x lateral 1 (5 x 5)
    "34x34": (34, 34, 3, ("fp32", "split"),
              ["f9:exdw+se_kernel+project", "f11:exdw+se_kernel+project", "lateral:chain", "lat0:lateral_stream",
               "level0:conv", "topk:channel_stats"],
              ["level0:fpn0x:tpc*"]),
    # Found with the path log itself -- the shapes the other
    # features.2 / features.3 kernels and lateral-chain variants need:
    # features.1 148 columns wide: too many pixels for fir23's register tiles,
    # just inside fir's 64 KB of LDS (147 and 148 are the only such widths):
    # features.2 on fir, features.3 on exdw without SE; lateral 3 of 57 pixels
    # with lateral 1 of 666: the big + reuse chain; features.10 / 11 (3 x 19, not a
    # seproj size) on the four-column exdw kernel without fc1 partials
    "72x592": (72, 592, 1, ("split",),
               ["f2:fir:th*", "f3:exdw+project", "f3:exdw:rt:k3s1:cs16:xt4", "f10:exdw:rt:k5s1:cs32:xt4",
                "f11:exdw:rt:k5s1:cs32:xt4", "lateral_chain:split:big+reuse"], ["f2:fir23:t*", "f2:generic"]),
    # features.1 176 columns wide: features.2 and features.3 (880 pixels) on the
    # generic three launches; level 0 (37 x 352) not 4x lateral 1 (10 x 88) with
    # a 66-pixel lateral 3: the fp32 big chain
    "74x704": (74, 704, 1, ("split",),
               ["f2:generic", "f3:generic", "lateral_chain:fp32:big", "lat0:lateral_stream"],
               ["f2:fir23:t*", "f2:fir:th*", "f3:exdw+project"]),
    # features.5-9 read 841 pixels: every SE block up to features.9 unfused,
    # features.7's expand (40 -> 120) on pw_small; lateral 3 of 225 pixels
    "456x456": (456, 456, 1, ("split",),
                ["f5:generic+se_kernel", "f7:generic+se_kernel", "f7:conv:pw_small", "f8:generic+se_kernel",
                 "f9:generic+se_kernel", "f10:exdw+se_kernel+project", "lateral:per_level", "level0:fpn0x:tpc13"],
                ["f5:exdw+se_kernel+project"]),
}
PARAMS = [(cid, prec) for cid, c in CASES.items() for prec in c[3]]


def _matches(pattern, token):
    """A listed token matches a logged one; "*" stands for an integer."""
    return re.fullmatch(re.escape(pattern).replace(r"\*", r"\d+"), token) is not None


def _model(sd, precision, dual_head=False):
    from dll.configs import KeypointHeadConfig, ModelConfig, TrainingConfig
    from dll.models import MultiPersonKeypointModel
    from dll.models.synthetic import synthetic_state_dict
    cfg = ModelConfig(keypoint_head=KeypointHeadConfig(height=56, width=56)) if dual_head else ModelConfig()
    m = MultiPersonKeypointModel(cfg, TrainingConfig(), precision=precision, dual_head=dual_head)
    m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0) if dual_head else sd)
    m.full_level0 = True
    return m.to(DEV).eval()


def _inputs(cid):
    """synthetic_images and two boxes per image; box 1 touches the left border
    (x1 = 0), on odd images the bottom border too (y2 = 1)."""
    from dll.models.synthetic import synthetic_boxes, synthetic_images
    H, W, B = CASES[cid][:3]
    seed = 1000 + H * 7 + W
    img = synthetic_images(B, 3, H, W, seed=seed)
    boxes = synthetic_boxes(B, 2, seed=seed + 1)
    boxes[:, 1, 0] = boxes[:, 1, 2] / 2
    boxes[1::2, 1, 1] = 1 - boxes[1::2, 1, 3] / 2
    return img, boxes


_REF, _RUN = {}, {}


def _ref(cid, sd):
    """The case's references, computed once and shared by its precisions."""
    if cid not in _REF:
        img, boxes = _inputs(cid)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        taps = O.mbv3_small_taps(img.double(), sd64)
        feat0 = O.fpn_level(O.fpn_laterals(taps, sd64)[0], sd64, 0)
        scores = O.channel_scores(feat0, sd64)
        _REF[cid] = {"img": img, "boxes": boxes, "taps": taps, "feat0": feat0, "scores": scores,
                     "topk": scores.topk(64, dim=1).indices, "out": O.forward(sd, {"image": img, "bboxes": boxes})}
    return _REF[cid]


def _run(cid, precision, sd):
    """One forward with the path log on; tokens, debug buffers (NCHW, on the host) and outputs."""
    key = (cid, precision)
    if key not in _RUN:
        from dll._native import _level_sizes
        img, boxes = _inputs(cid)
        H, W, B = CASES[cid][:3]
        m = _model(sd, precision)
        plan = m.native_plan(DEV)
        plan.path_log(True)
        with torch.no_grad():
            out = m({"image": img.to(DEV), "bboxes": boxes.to(DEV)})
        torch.cuda.synchronize()
        sizes = _level_sizes(H, W)
        r = {"tokens": plan.paths(), "raw": {}, "taps": []}
        for i, (c, lv) in enumerate(zip(TAP_CH, TAP_LEVEL)):
            h, w = sizes[lv]
            t = plan.debug_buffer(f"tap{i}").view(B, h, w, -1).cpu()
            r["raw"][i] = t
            r["taps"].append(t[..., :c].permute(0, 3, 1, 2).contiguous())
        h0, w0 = sizes[0]
        r["feat0"] = plan.debug_buffer("feat0").view(B, h0, w0, 128).permute(0, 3, 1, 2).cpu().contiguous()
        r["scores"] = plan.debug_buffer("scores").view(B, 128).cpu().clone()
        r["out"] = {k: out[k].cpu() for k in ("keypoints", "visibilities", "heatmap")}
        plan.path_log(False)
        del m, plan
        _RUN[key] = r
    return _RUN[key]


def _ratio(got, want, tol):
    """max of error / (atol + rtol * |ref|) with rtol = atol = tol, against a float64 reference."""
    return float(((got.double() - want).abs() / (tol + tol * want.abs())).max())


@pytest.mark.parametrize("cid,precision", PARAMS, ids=[f"{c}-{p}" for c, p in PARAMS])
def test_case_vs_fp64(model_sd, cid, precision):
    ref, got = _ref(cid, model_sd), _run(cid, precision, model_sd)
    B = CASES[cid][2]
    tokens = got["tokens"]
    print(f"\n{cid} {precision} paths: {' '.join(tokens)}")
    mine = lambda ts: [t.split(">")[-1] for t in ts if ">" not in t or t.startswith(precision + ">")]
    missing = [t for t in mine(CASES[cid][4]) if not any(_matches(t, x) for x in tokens)]
    unexpected = [t for t in mine(CASES[cid][5]) if any(_matches(t, x) for x in tokens)]
    assert not missing and not unexpected, f"{cid}: not logged {missing}, logged against the case's purpose {unexpected}"
    if precision == "split":
        assert "hm:hmconv:split" in tokens
    elif precision == "mixed":
        assert "hm:hmconv:bf16" in tokens
    else:
        assert "hm:conv:k3" in tokens and "hm:final:separate" in tokens

    # error / tolerance per tap and for FPN level 0
    rep = {f"tap{i}": _ratio(got["taps"][i], ref["taps"][i], TAP_TOL) for i in range(4)}
    rep["feat0"] = _ratio(got["feat0"], ref["feat0"], FEAT_TOL)
    print(f"{cid} {precision} max error / tolerance:", {k: round(v, 3) for k, v in rep.items()},
          "| worst tap error in units of a 1e-5 band:",
          round(max(_ratio(got["taps"][i], ref["taps"][i], 1e-5) for i in range(4)), 3))
    for i, t in got["raw"].items():   # channel padding of the NHWC buffers
        assert t.shape[-1] == (TAP_CH[i] + 15) // 16 * 16
    assert torch.count_nonzero(got["raw"][1][..., 24:]) == 0, "tap1 padding channels 24..31 must be zero"
    bad = {k: v for k, v in rep.items() if not v <= 1.0}
    assert not bad, f"{cid} {precision}: over tolerance (error / tolerance) {bad}; paths {tokens}"

    serr = float((got["scores"].double() - ref["scores"]).abs().max())
    print(f"{cid} {precision} scores max|d| {serr:.2e}")
    assert serr <= 1e-6
    topk = got["scores"].topk(64, dim=1).indices
    for n in range(B):
        assert set(topk[n].tolist()) == set(ref["topk"][n].tolist()), f"top-64 set of image {n}"

    out, want = got["out"], ref["out"]
    kerr = float((out["keypoints"] - want["keypoints"]).abs().max())
    herr = float((out["heatmap"] - want["heatmap"]).abs().max())
    flips = float((out["visibilities"] != want["visibilities"]).any(-1).float().mean())
    print(f"{cid} {precision} keypoints max|d| {kerr:.2e} heatmap max|d| {herr:.2e} visibility flips {flips:.4f}")
    if precision == "mixed":
        assert kerr <= 1e-3 and herr <= 3e-2 and flips <= 0.02
    else:
        assert kerr <= 1e-5 and herr <= 5e-5
        assert torch.equal(out["visibilities"], want["visibilities"])


@pytest.fixture(scope="module")
def seen(model_sd):
    """The tokens of every case's forward, of one dual-head + detect forward
    (256 x 192, B = 2), of detect forwards too wide for the fused detector
    (256 x 576, B = 1 and 21), of one fp32 dual-head forward on caller boxes,
    of KEYPOINT_HEAD called on its own (split), and of four large batches
    (forward only, inputs drawn on the device): launch_conv halves its M tile
    while 128-row tiles give fewer than 512 workgroups, and pw_small takes
    1x1 convs up to 4 Mi outputs, so those variants depend on the batch."""
    from dll.configs import KeypointHeadConfig
    from dll.models import KEYPOINT_HEAD
    from dll.models.synthetic import synthetic_boxes, synthetic_images, synthetic_state_dict
    tokens = {}
    for cid, precision in PARAMS:
        tokens[f"{cid}-{precision}"] = _run(cid, precision, model_sd)["tokens"]
    for name, (H, W, B, dual) in {"detect+dual 256x192": (256, 192, 2, True),
                                  "detect 256x576": (256, 576, 1, False)}.items():
        m = _model(model_sd, "split", dual_head=dual)
        plan = m.native_plan(DEV)
        plan.path_log(True)
        with torch.no_grad():
            m(synthetic_images(B, 3, H, W, seed=31).to(DEV))   # no boxes: the detector branch
        torch.cuda.synchronize()
        tokens[name] = plan.paths()
        if not dual:   # 21 images: 65856 rows of pooled 56 x 56 maps, 515 tiles of 128 rows
            with torch.no_grad():
                m(torch.randn(21, 3, H, W, device=DEV))
            torch.cuda.synchronize()
            tokens[name + " B=21"] = plan.paths()
        del m, plan
    m = _model(model_sd, "split")
    plan = m.native_plan(DEV)
    plan.path_log(True)
    box = synthetic_boxes(1, 1, seed=35).to(DEV)
    # 512 x 384: lateral 1 (3072 pixels) leaves pw_small at 11 images and takes 128-row tiles at 22, where
    # features.1's project (12288 pixels) has them too; 256 x 192: the last conv (48 pixels) at 152 / 273 images
    for H, W, B in ((512, 384, 11), (512, 384, 22), (256, 192, 152), (256, 192, 273)):
        with torch.no_grad():
            m({"image": torch.randn(B, 3, H, W, device=DEV), "bboxes": box})
        torch.cuda.synchronize()
        tokens[f"{H}x{W} B={B}"] = plan.paths()
    del m, plan
    m = _model(model_sd, "fp32", dual_head=True)
    plan = m.native_plan(DEV)
    plan.path_log(True)
    with torch.no_grad():
        m({"image": synthetic_images(2, 3, 256, 192, seed=32).to(DEV), "bboxes": synthetic_boxes(2, 2, seed=33).to(DEV)})
    torch.cuda.synchronize()
    tokens["dual fp32 256x192"] = plan.paths()
    del m, plan
    kh = KEYPOINT_HEAD(KeypointHeadConfig(height=56, width=56))
    kh.load_state_dict(synthetic_state_dict(kh.state_dict(), seed=3))
    kh.precision = "split"
    kh = kh.to(DEV).eval()
    plan = kh._plans.get(kh, DEV, "split")
    plan.path_log(True)
    kh(torch.randn(1, 128, 56, 56, generator=torch.Generator().manual_seed(34)).to(DEV))
    torch.cuda.synchronize()
    tokens["KEYPOINT_HEAD alone"] = plan.paths()
    return tokens


# Tokens no forward above reaches: one line and one reason each.
ALLOWED_UNSEEN = {
    "kh:conv:k1:bm128": "dual-head flag in fp32 precision with more than 20 ROIs (512 tiles of 128 rows)",
    "f*:conv:k1:bm128+splitk": "a pass of exactly max_pass_images images: 65409+ rows on a map of at most 256 "
                               "pixels, which only 334 images of 224 x 224 (65464 rows, the cap) give",
}


def test_every_path_is_covered(seen):
    from dll import _native
    listed = _native.all_paths()
    assert len(listed) == len(set(listed))
    union = sorted({t for ts in seen.values() for t in ts})
    for name, ts in seen.items():
        print(f"{name}: {' '.join(ts)}")
    unknown = [t for t in union if not any(_matches(p, t) for p in listed)]
    assert not unknown, f"logged but not in the library's table: {unknown}"
    uncovered = [p for p in listed if p not in ALLOWED_UNSEEN and not any(_matches(p, t) for t in union)]
    assert not uncovered, f"no case reaches {uncovered} (and the allow-list does not name them)"
    stale = [p for p in ALLOWED_UNSEEN if p not in listed or any(_matches(p, t) for t in union)]
    assert not stale, f"allow-listed but reached, or not a token of the library: {stale}"


def test_path_log_is_off_by_default_and_cleared(model_sd):
    img, boxes = _inputs("128x96")
    m = _model(model_sd, "split")
    plan = m.native_plan(DEV)
    with torch.no_grad():
        m({"image": img.to(DEV), "bboxes": boxes.to(DEV)})
    assert plan.paths() == []
    plan.path_log(True)
    with torch.no_grad():
        m({"image": img.to(DEV), "bboxes": boxes.to(DEV)})
        first = plan.paths()
        m({"image": img.to(DEV), "bboxes": boxes.to(DEV)})
    assert first and plan.paths() == first and len(first) == len(set(first))
    # hipGraph replay: the eager call and the captured one log, a replay takes no decision
    B, P = boxes.shape[:2]
    img_d, boxes_d = img.to(DEV), boxes.to(DEV)
    kpts, vis = torch.empty(B, P, 1, 17, 2, device=DEV), torch.empty(B, P, 1, 17, 3, device=DEV)
    heat = torch.empty(B, P, 17, 56, 56, device=DEV)
    plan.set_graphs(True)
    try:
        logged = []
        for _ in range(3):                                  # eager, capture + launch, replay
            plan.forward(img_d, boxes_d, kpts, vis, heat)
            torch.cuda.synchronize()
            logged.append(plan.paths())
    finally:
        plan.set_graphs(False)
    assert logged == [first, first, []]
    plan.path_log(False)
    assert plan.paths() == []


def test_shape_sequence_on_one_plan(model_sd):
    """One model runs 128 x 96 (B = 2), 250 x 190 (B = 2), its plan's backbone()
    at 128 x 96, 128 x 96 again, then image 1 of the first batch alone: the
    workspace is re-carved and re-zeroed between shapes, the split-scale slots
    (sc_dirty) cross a forward that never clears them (250 x 190 is not on the
    fpn0x path) and a backbone() that sets them and runs no top-k to zero them.
    Every 128 x 96 output is bit-identical to the first run and to a fresh
    model's."""
    keys = ("keypoints", "visibilities", "heatmap")
    img_a, box_a = _inputs("128x96")
    img_b, box_b = _inputs("250x190")

    def fwd(m, img, boxes):
        with torch.no_grad():
            out = m({"image": img.to(DEV), "bboxes": boxes.to(DEV)})
        torch.cuda.synchronize()
        n = img.shape[0]
        res = {k: out[k].cpu().clone() for k in keys}
        res["feat0"] = m.native_plan(DEV).debug_buffer("feat0").view(n, -1).cpu().clone()
        return res

    fresh = fwd(_model(model_sd, "split"), img_a, box_a)
    m = _model(model_sd, "split")
    first = fwd(m, img_a, box_a)
    fwd(m, img_b, box_b)
    m.native_plan(DEV).backbone(img_a.to(DEV))   # fpn0x with every lateral kept, no top-k: the slots stay dirty
    torch.cuda.synchronize()
    again =fwd(m, img_a, box_a)
    alone = fwd(m, img_a[1:2], box_a[1:2])
    for k in keys + ("feat0",):
        assert torch.equal(first[k], fresh[k]), f"{k}: first run vs a fresh model"
        assert torch.equal(again[k], first[k]), f"{k}: after another shape"
        assert torch.equal(alone[k][0], first[k][1]), f"{k}: image 1 alone"
