"""The function-preserving weight rescalings of tests/scale_variants.py, on the
CPU: for every variant the GPU tests run (tests/test_scale_robustness.py) the
fp32 oracle returns heatmaps, keypoints and the top-64 channels bit-identical
to the seed-0 weights', at the GPU tests' 128 x 96 inputs.  If one of these
fails the variant is wrong, not a kernel."""
import pytest
import torch

import scale_variants as V
from oracle import kpd_oracle as O

NAMES = list(V.VARIANTS) + list(V.CLAMP_VARIANTS)


def _batch():
    from dll.models.synthetic import synthetic_boxes, synthetic_images
    H, W, B = 128, 96, 2
    seed = 1000 + H * 7 + W
    return {"image": synthetic_images(B, 3, H, W, seed=seed), "bboxes": synthetic_boxes(B, 2, seed=seed + 1)}


@pytest.fixture(scope="module")
def seed0(model_sd):
    return O.forward(model_sd, _batch(), return_debug=True)


@pytest.mark.parametrize("name", NAMES)
def test_variant_is_bit_identical_in_the_oracle(model_sd, seed0, name):
    sd = V.variant(model_sd, name)
    changed = [k for k in sd if not torch.equal(sd[k], model_sd[k])]
    assert changed, "the variant changes no weight"
    for k in changed:   # an exact power of two per tensor, nothing flushed or overflowed
        ratio = sd[k].double() / model_sd[k].double()
        ratio = ratio[model_sd[k] != 0]
        assert torch.isfinite(ratio).all() and (ratio == ratio.flatten()[0]).all(), k
        assert float(ratio.flatten()[0].log2()) == round(float(ratio.flatten()[0].log2())), k
    out = O.forward(sd, _batch(), return_debug=True)
    for key in ("heatmap", "keypoints", "visibilities", "_topk"):
        assert torch.equal(out[key], seed0[key]), f"{name}: {key} differs from seed 0"
    # level 0 itself moves by the gain exponent only, exactly
    assert torch.equal(out["_feat0"], torch.ldexp(seed0["_feat0"], torch.tensor(V.gain_of(name)))), f"{name}: level 0"


def test_variants_leave_the_input_dict_alone(model_sd):
    before = {k: v.clone() for k, v in model_sd.items()}
    V.apply(model_sd, 12, (3, -3, 5), -7)
    assert all(torch.equal(before[k], model_sd[k]) for k in before)
