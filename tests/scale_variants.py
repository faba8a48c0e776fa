"""Power-of-two weight rescalings that leave the model's function unchanged
(DESIGN.md §5e).  Three junctions of the model are positively homogeneous, so
a factor s = 2^k moves across each of them without changing any fp32 result:
every product is scaled by an exact power of two.  The oracle's outputs stay
bit-identical to the unscaled weights' while every operand exponent, w_exp,
bc / bs and hi / lo split of the split kernels moves by k.

A plain helper module (no fixtures, no tests): tests/test_scale_variants.py
proves the variants on the CPU, tests/test_scale_robustness.py runs them on
the GPU.  Each function returns a cloned state dict.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch

SD = Dict[str, torch.Tensor]

# conv -> BN -> ReLU -> conv junctions of the HeatmapHead: (BN, the next conv's weight)
HM_JUNCTIONS = (
    ("heatmap_head.deconv_layers.1", "heatmap_head.deconv_layers.4.weight"),
    ("heatmap_head.deconv_layers.5", "heatmap_head.final_layer.0.weight"),
    ("heatmap_head.final_layer.1", "heatmap_head.final_layer.3.weight"),
)
# everything that reads FPN level 0 on the caller-boxes path, first linear map of each reader
LEVEL0_READERS = (
    "channel_attention.fc.0.weight",
    "heatmap_head.channel_attention.fc.0.weight",
    "heatmap_head.spatial_attention.conv.weight",
    "heatmap_head.deconv_layers.0.weight",
)


def _clone(sd: SD) -> SD:
    return {k: v.detach().clone() for k, v in sd.items()}


def _scale(sd: SD, key: str, k: int) -> None:
    sd[key] = torch.ldexp(sd[key], torch.tensor(k))


def rescale_fpn(sd: SD, k: int) -> SD:
    """Laterals x 2^k, the level-0 3x3 conv x 2^-k (the laterals have no bias,
    the level-0 conv has none before its BN): level 0 is unchanged, lateral 1
    and the composite fpn0x weights move by +-k."""
    out = _clone(sd)
    for i in range(4):
        _scale(out, f"backbone.fpn.lateral_convs.{i}.weight", k)
    _scale(out, "backbone.fpn.fpn_convs.0.0.weight", -k)
    return out


def rescale_hm(sd: SD, ks: Sequence[int]) -> SD:
    """Per HeatmapHead junction j: the BN's weight and bias x 2^ks[j], the next
    conv's weight x 2^-ks[j].  h1, h2, h3 move by ks[0..2]; the heatmap does not."""
    out = _clone(sd)
    for (bn, nxt), k in zip(HM_JUNCTIONS, ks):
        _scale(out, bn + ".weight", k)
        _scale(out, bn + ".bias", k)
        _scale(out, nxt, -k)
    return out


def gain_level0(sd: SD, k: int) -> SD:
    """FPN level 0 x 2^k (its BN's weight and bias), every reader's first linear
    map x 2^-k.  Holds with caller boxes only: the detector and KEYPOINT_HEAD
    read level 0 too and are not rescaled."""
    out = _clone(sd)
    _scale(out, "backbone.fpn.fpn_convs.0.1.weight", k)
    _scale(out, "backbone.fpn.fpn_convs.0.1.bias", k)
    for key in LEVEL0_READERS:
        _scale(out, key, -k)
    return out


def apply(sd: SD, fpn: int = 0, hm: Sequence[int] = (0, 0, 0), gain: int = 0) -> SD:
    """The three rescalings composed."""
    return gain_level0(rescale_hm(rescale_fpn(sd, fpn), hm), gain)


# name -> (fpn k, heatmap-head triple, gain k): every variant the GPU tests run
HM_TRIPLES = ((10, -10, 6), (-12, 12, -8), (16, 16, 16), (-16, -16, -16))
VARIANTS = {}
for _k in (-40, -12, 12, 40):
    VARIANTS[f"fpn{_k:+d}"] = (_k, (0, 0, 0), 0)
for _t in HM_TRIPLES:
    VARIANTS["hm" + ",".join(f"{v:+d}" for v in _t)] = (0, _t, 0)
for _k in (-24, -6, 6, 24):
    VARIANTS[f"gain{_k:+d}"] = (0, (0, 0, 0), _k)
VARIANTS["combined"] = (20, (16, 16, 16), -12)
# the clamps at +-100: at k = +90 the level-0 weight exponent
# 14 - e is 104 / 105; at k = -90 the lateral-1 bound's exponent is 98 (no clamp
# yet), at k = -96 it is 104
CLAMP_VARIANTS = {"fpn-96": (-96, (0, 0, 0), 0), "fpn-90": (-90, (0, 0, 0), 0), "fpn+90": (90, (0, 0, 0), 0)}
# the variants run at 512 x 384 as well (per-level laterals + split_rows: max-based scales)
LARGE_VARIANTS = ("fpn-40", "fpn+40", "gain-24", "gain+24")


def variant(sd: SD, name: str) -> SD:
    fpn, hm, gain = {**VARIANTS, **CLAMP_VARIANTS}[name]
    return apply(sd, fpn, hm, gain)


def gain_of(name: str) -> int:
    """The exponent by which the variant scales FPN level 0."""
    return {**VARIANTS, **CLAMP_VARIANTS}[name][2]
