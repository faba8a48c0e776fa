"""conv1x1_nchw_kernel (csrc/ops_kernels.hip) through _native.conv1x1 and
PERSON_HEAD.forward, against tests/ops_ref.conv1x1_ref (an fp64 einsum plus
the bias).

HW of 1, 255, 256, 257 (one partial workgroup, exactly one, one and a thread),
Cin of 1, 3, 128 and Cout of 1, 5, 64 (grid.y), B = 2; bias=None; B = 0; the
3-D input path of person_head.py.

Bar: a Cin-term fp32 fma chain plus the bias add against fp64 is within
(Cin + 1) * 2^-24 * sum|w x| (+ |b|), computed per output from the reference;
asserted with a factor of 2.
"""
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ops_ref as R  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _check(x, w, b, tag):
    from dll import _native
    got = _native.conv1x1(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV)).cpu().numpy()
    want, mag = R.conv1x1_ref(x, w, b)
    assert got.shape == want.shape, tag
    bound = 2 * (x.shape[1] + 1) * 2.0 ** -24 * mag
    err = np.abs(got - want)
    assert (err <= bound).all(), (tag, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))


@gpu
@pytest.mark.parametrize("hw", [(1, 1), (5, 51), (16, 16), (1, 257)])
def test_channel_counts_at_workgroup_edges(hw):
    g = torch.Generator().manual_seed(13)
    for cin, cout in itertools.product((1, 3, 128), (1, 5, 64)):
        x = torch.randn(2, cin, *hw, generator=g)
        w = torch.randn(cout, cin, 1, 1, generator=g)
        b = torch.randn(cout, generator=g)
        _check(x, w, b, (hw, cin, cout))
    _check(x, w, None, (hw, "no bias"))
    _check(x * 1e4, w * 1e-3, b * 1e3, (hw, "scaled"))             # the bound scales with the operands


@gpu
def test_empty_batch_and_argument_errors():
    from dll import _native
    w = torch.randn(5, 3, 1, 1)
    out = _native.conv1x1(torch.empty(0, 3, 4, 6, device=DEV), w.to(DEV), None)
    assert out.shape == (0, 5, 4, 6)
    with pytest.raises(ValueError):
        _native.conv1x1(torch.randn(1, 4, 2, 2, device=DEV), w.to(DEV), None)


@gpu
def test_person_head_forward_batched_and_unbatched():
    """PERSON_HEAD.forward keeps the last level's box head: [B,128,h,w] and the
    unbatched [128,h,w] path, at a size that is no multiple of the workgroup."""
    from dll.configs.model_config import PersonDetectionConfig
    from dll.models import PERSON_HEAD
    torch.manual_seed(3)
    head = PERSON_HEAD(PersonDetectionConfig()).eval()
    assert head.box_heads[0].in_channels == 128
    g = torch.Generator().manual_seed(14)
    feats = [torch.randn(2, 128, h, w, generator=g) for h, w in ((9, 7), (5, 3), (3, 2), (1, 1))]
    for n_levels in (4, 2):
        conv = head.box_heads[n_levels - 1]
        want, mag = R.conv1x1_ref(feats[n_levels - 1], conv.weight, conv.bias)
        head_dev = head.to(DEV)
        with torch.no_grad():
            got = head_dev([f.to(DEV) for f in feats[:n_levels]]).cpu().numpy()
            got3 = head_dev([f[0].to(DEV) for f in feats[:n_levels]]).cpu().numpy()
        bound = 2 * 129 * 2.0 ** -24 * mag
        assert got.shape == want.shape and (np.abs(got - want) <= bound).all(), n_levels
        assert got3.shape == want.shape[1:] and np.array_equal(got3, got[0]), n_levels
