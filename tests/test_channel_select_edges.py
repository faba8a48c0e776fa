"""nchw_channel_stats_kernel, topk_kernel and gather_planes_kernel through
ChannelAttention.native_select and select_top_k_channels, against
tests/ops_ref.channel_select_ref (fp64; tied to the golden ca_scores / ca_topk
by test_ops_ref_cpu.py).

* H x W of 1x1, 1x7, 5x51 (255), 16x16 (256) and 3x86 (258): the stats kernel's
  256-thread stride with idle threads, exactly full, and a second round;
  B = 1 and B = 3; inputs of either sign (the max branch starts from -inf, an
  all-negative plane must not come out as 0).
* Equal scores: two channels with the same fc.2 row and bias score the same
  to the bit, the lower index comes first.
* Non-finite input (select=False only: no gather runs, nothing is indexed by
  the result): +inf, -inf and NaN planes.  The order is total -- a NaN ranks
  before every number, index ascending among equals -- so the indices are
  distinct and inside [0, 128) whatever the scores are (include/kpd.h).

Bars: scores 1e-6 (the project's bar for this operator); top-k indices and
gathered planes bit for bit.  Every finite case keeps neighbouring scores
more than 2e-6 apart (checked on the CPU), so the fp32 ranking is the fp64
ranking.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ops_ref as R  # noqa: E402

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = "channel_attention."
SIZES = [(1, 1), (1, 7), (5, 51), (16, 16), (3, 86)]
NAN, INF = float("nan"), float("inf")


def finite_cases():
    """(tag, x [B,128,H,W]): randn (either sign), all negative, all positive, per size and B."""
    g = torch.Generator().manual_seed(26)          # a seed whose 2540 neighbouring scores all lie > 2e-6 apart
    out = []
    for (h, w), B in [(s, b) for s in SIZES for b in (1, 3)]:
        x = torch.randn(B, 128, h, w, generator=g)
        x[0, 5] = -x[0, 5].abs() - 0.5                              # an all-negative plane: its max is negative
        if B == 3:
            x[1] = -x[1].abs() - 0.1                                # an all-negative image
            x[2] = x[2].abs()
        out.append((f"{h}x{w}_B{B}", x))
    return out


def nonfinite_cases():
    g = torch.Generator().manual_seed(24)
    base = lambda: torch.randn(3, 128, 5, 7, generator=g)            # noqa: E731
    a = base(); a[0, 9] = INF; a[1, 9] = -INF; a[2, 9, 2, 3] = NAN   # whole planes of +-inf, one NaN element
    b = base(); b[0, 4, 0, 0] = INF; b[0, 77, 1, 1] = -INF; b[1, :, 0, 0] = INF; b[2] = NAN
    c = base(); c[0, 3, 1, 1] = INF; c[0, 3, 2, 2] = -INF            # inf and -inf in one plane: mean NaN, max inf
    c[1, 100] = -INF
    return [("planes", a), ("mixed", b), ("inf_minus_inf", c)]


def tied_sd(model_sd):
    sd = {k: v.clone() for k, v in model_sd.items() if k.startswith(P)}
    for dst, src in ((7, 90), (91, 90), (30, 2)):                   # a triple and a pair of identical channels
        sd[P + "fc.2.weight"][dst] = sd[P + "fc.2.weight"][src]
        sd[P + "fc.2.bias"][dst] = sd[P + "fc.2.bias"][src]
    return sd


def test_finite_cases_have_no_near_ties(model_sd):
    for tag, x in finite_cases():
        _, _, gap = R.channel_select_ref(x, model_sd)
        assert (gap > 2e-6).all(), (tag, gap)
        _, _, gap = R.channel_select_ref(x, tied_sd(model_sd))      # distinct scores stay apart; equal ones are equal
        assert (gap > 2e-6).all(), (tag, gap)


def _module(sd):
    from dll.models.keypoint_model import ChannelAttention
    m = ChannelAttention(128)
    m.load_state_dict({k[len(P):]: v for k, v in sd.items() if k.startswith(P)})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def ca(model_sd):
    return _module(model_sd)


@gpu
@pytest.mark.parametrize("idx", range(len(SIZES) * 2))
def test_scores_topk_and_gather(ca, model_sd, idx):
    from dll.models import select_top_k_channels
    tag, x = finite_cases()[idx]
    want_s, want_t, _ = R.channel_select_ref(x, model_sd)
    xd = x.to(DEV)
    scores, topk, sel = ca.native_select(xd, 64, select=True)
    np.testing.assert_allclose(scores.cpu().numpy(), want_s, atol=1e-6, rtol=0, err_msg=tag)
    assert np.array_equal(topk.cpu().numpy(), want_t), tag
    b = torch.arange(x.shape[0])[:, None]
    assert torch.equal(sel.cpu(), x[b, torch.from_numpy(want_t)]), tag          # bit for bit
    assert torch.equal(select_top_k_channels(xd, ca, k=64), sel), tag
    assert torch.equal(ca(xd), scores), tag


@gpu
def test_equal_scores_go_to_the_lower_index(model_sd):
    sd = tied_sd(model_sd)
    m = _module(sd)
    for tag, x in finite_cases()[4:8]:
        want_s, want_t, _ = R.channel_select_ref(x, sd)
        scores, topk, _ = m.native_select(x.to(DEV), 64, select=False)
        s = scores.cpu().numpy()
        assert (s[:, 7] == s[:, 90]).all() and (s[:, 91] == s[:, 90]).all() and (s[:, 30] == s[:, 2]).all(), tag
        np.testing.assert_allclose(s, want_s, atol=1e-6, rtol=0, err_msg=tag)
        assert np.array_equal(topk.cpu().numpy(), want_t), tag
    assert any(7 in t and 90 in t for t in want_t.tolist())                      # the tie is inside the top 64 somewhere


@gpu
def test_non_finite_scores_keep_topk_a_set_of_distinct_channels(ca, model_sd):
    """select=False: no gather runs, so nothing is read through the indices."""
    for tag, x in nonfinite_cases():
        want_s, want_t, _ = R.channel_select_ref(x, model_sd)
        scores, topk, sel = ca.native_select(x.to(DEV), 64, select=False)
        assert sel is None
        t, s = topk.cpu().numpy(), scores.cpu().numpy()
        assert ((t >= 0) & (t < 128)).all(), (tag, t)
        assert all(len(set(row.tolist())) == 64 for row in t), (tag, t)
        assert np.array_equal(np.isnan(s), np.isnan(want_s)), tag
        np.testing.assert_allclose(s, want_s, atol=1e-6, rtol=0, equal_nan=True, err_msg=tag)
        for b in range(len(t)):
            # where a whole image's scores are NaN or saturated the order is by index alone: exact
            if np.isnan(want_s[b]).all() or len(np.unique(want_s[b][~np.isnan(want_s[b])])) <= 2:
                assert np.array_equal(t[b], want_t[b]), (tag, b)
            n_nan = int(np.isnan(want_s[b]).sum())
            assert np.array_equal(t[b][: min(n_nan, 64)], want_t[b][: min(n_nan, 64)]), (tag, b)   # NaN first
    assert np.isnan(R.channel_select_ref(nonfinite_cases()[0][1], model_sd)[0][2]).all()   # one NaN: all of image 2
