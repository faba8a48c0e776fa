"""Device NMS (_native.nms -> kpd_nms) against detector_ref.greedy_nms on the
same fp32 arrays, at the sizes where the kernels change:

  n = 1, 2, 1023, 1024, 1025     one candidate per thread / a second register slot;
                                 total > kNmsPrefix (radix select of the prefix)
  n = 2047, 2048, 2049           the capacity of the prefix list
  n = 32767, 32768, 32769        nms_reg_kernel's last sizes and the first of the
                                 generic nms_kernel (global alive flags, two sweeps
                                 per kept box), which no smaller n reaches
  n = 50,000                     nms_kernel well inside its range

Scores are distinct (a permutation), centres uniform, box sides 0.02 to 0.2;
the max_output = 0 run at 32,769 uses sides 0.3 to 0.6 so that few boxes
survive.  Every case asserts that no IoU the reference compared lies within
1e-6 of the threshold (about 30 fp32 ulps at 0.3): the kept indices must then
be identical.  The seeds (the best of six per case, chosen on the CPU: the
arrays are the device's inputs) give margins of 1.1e-4 or more for
max_output = 0 up to n = 2,049 and for max_output = 5 (32,768: 9.9e-5);
3.9e-6 to 5.0e-6 for max_output = 300; 6.2e-6 for the large boxes; 1.1e-4
(n = 3,000) and 2.2e-6 (n = 40,000) for the -inf cases.

-inf scores: kpd_nms runs unfiltered, so a candidate scored -inf is alive, ranks
last by index and is kept when nothing suppresses it, as the reference keeps
it -- in nms_reg_kernel (n = 3,000) and nms_kernel (n = 40,000) alike.

Signed zeros: -0.0 and +0.0 are equal scores, so the lower index ranks first
for every n ("ties: lower index first").  Before key_of gave both zeros one
radix key the n = 3,000 case failed on an MI355X as read from the code: the
prefix held only the +0.0 candidates and the kernel kept [1500 .. 1504]; the
n = 1,000 case (no radix select) kept [0 .. 4] then as now.  n = 40,000 runs
the same construction on nms_kernel.

nms_kernel's filter (-inf starts dead) and gather (out_boxes) branches are
reachable only from a detector with more than 32,768 anchors, which this model
(56 x 56 x 9 = 28,224) cannot have; kpd_nms passes filter = 0 and no gather,
so they stay untested rather than getting an entry point of their own.
"""
import pytest
import torch

from detector_ref import greedy_nms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

IOU_MARGIN = 1e-6
THR = 0.3

# (n, max_output) -> seed;  "big": box sides 0.3 to 0.6
SIZE_CASES = {
    (1, 0): 1, (1, 5): 1, (2, 0): 1, (2, 5): 1,
    (1023, 0): 4, (1023, 5): 6, (1024, 0): 1, (1024, 5): 1, (1025, 0): 6, (1025, 5): 3,
    (2047, 0): 3, (2047, 5): 4, (2048, 0): 3, (2048, 5): 6, (2049, 0): 6, (2049, 5): 4,
    (32767, 5): 6, (32767, 300): 4, (32768, 5): 1, (32768, 300): 1,
    (32769, 5): 1, (32769, 300): 6, (50000, 5): 1, (50000, 300): 6,
}
BIG_CASE = (32769, 0, 5)
INF_CASES = {(3000, 0): 4, (3000, 60): 4, (40000, 0): 5, (40000, 100): 5}


def _random_case(n, seed, lo=0.02, hi=0.2):
    g = torch.Generator().manual_seed(seed)
    boxes = torch.rand(n, 4, generator=g) * torch.tensor([1.0, 1.0, hi - lo, hi - lo])
    boxes += torch.tensor([0.0, 0.0, lo, lo])
    scores = (torch.randperm(n, generator=g).float() + 1) / n          # distinct
    return boxes, scores


def _inf_case(n, seed):
    """The lower-scored half scores -inf; the scored boxes stay in the left
    half of the plane, so unsuppressed -inf boxes remain on the right."""
    boxes, scores = _random_case(n, seed, 0.15, 0.4)
    low = scores <= 0.5
    scores[low] = -float("inf")
    boxes[~low, 0] *= 0.45
    return boxes, scores


def _disjoint_zeros(n):
    """n disjoint boxes on a 60-column grid; the first half scores -0.0, the second +0.0."""
    i = torch.arange(n)
    boxes = torch.stack([((i % 60) + 0.5) / 60, ((i // 60) + 0.5) / 50, torch.full((n,), 0.01), torch.full((n,), 0.01)],
                        dim=1)
    scores = torch.zeros(n)
    scores[: n // 2] = -0.0
    return boxes, scores


def _check(boxes, scores, mo, what):
    from dll import _native
    got = _native.nms(boxes.to(DEV), scores.to(DEV), THR, mo).cpu()
    ref, margin = greedy_nms(boxes, scores, THR, mo)
    print(f"{what}: kept {len(ref)}, IoU margin {margin:.1e}")
    assert margin >= IOU_MARGIN, f"{what}: an IoU within {margin:.1e} of the threshold: choose another seed"
    assert torch.equal(got, ref), what
    return ref


@pytest.mark.parametrize("n,mo", list(SIZE_CASES))
def test_nms_size(n, mo):
    boxes, scores = _random_case(n, SIZE_CASES[(n, mo)])
    keep = _check(boxes, scores, mo, f"n={n} max_output={mo}")
    assert 1 <= len(keep) <= (min(n, mo) if mo else n)


def test_nms_generic_kernel_runs_dry():
    """max_output = 0 on nms_kernel: it keeps until nothing is alive."""
    n, mo, seed = BIG_CASE
    boxes, scores = _random_case(n, seed, 0.3, 0.6)
    keep = _check(boxes, scores, mo, f"n={n} max_output=0, large boxes")
    assert 1 < len(keep) < 500


@pytest.mark.parametrize("n,mo", list(INF_CASES))
def test_nms_minus_inf_scores(n, mo):
    boxes, scores = _inf_case(n, INF_CASES[(n, mo)])
    keep = _check(boxes, scores, mo, f"-inf half, n={n} max_output={mo}")
    inf_kept = scores[keep] == -float("inf")
    assert inf_kept.any() and not inf_kept.all(), "the case must keep scored and -inf candidates"
    first = int(inf_kept.nonzero()[0])
    assert inf_kept[first:].all()                       # -inf ranks last ...
    assert bool((keep[first + 1:] > keep[first:-1]).all())   # ... in index order


@pytest.mark.parametrize("n", [1000, 3000, 40000])
def test_nms_signed_zeros(n):
    boxes, scores = _disjoint_zeros(n)
    assert torch.signbit(scores[: n // 2]).all() and not torch.signbit(scores[n // 2:]).any()
    keep = _check(boxes, scores, 5, f"signed zeros, n={n}")
    assert keep.tolist() == [0, 1, 2, 3, 4]
