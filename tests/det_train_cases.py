"""The fixtures shared by tests/test_det_train_cpu.py (fp32 and float64 matchings
agree on every anchor of each) and tests/test_det_train.py (the device equals
them): seeded GT boxes per (B, G, image size).  CPU tensors only."""
from dll.models.synthetic import synthetic_boxes

MAIN_SIZE = (256, 192)


def main_boxes():
    """The main fixture's labels: synthetic_boxes(2, 3, seed=1235) with row [1, 1] zeroed."""
    gt = synthetic_boxes(2, 3, seed=1235)
    gt[1, 1] = 0
    return gt


def _mixed(B, G, seed):
    """Person-sized boxes with every fourth one shrunk to a fifth (its best IoU stays below the
    thresholds: a low-quality set) and, for G >= 8, absent rows of each kind."""
    gt = synthetic_boxes(B, G, seed=seed)
    gt[:, 3::4, 2:] *= 0.2
    if G >= 8:
        gt[:, 5] = 0
        gt[:, 6, 2] = 0
        gt[:, 7, 1] = float("nan")
        gt[0, G // 2:] = 0        # an image with half its slots padding
    return gt


def _zero_middle(B, seed):
    gt = synthetic_boxes(B, 3, seed=seed)
    gt[:, 1] = 0
    return gt


# name -> (B, (H, W), gt [B,G,4] or None).  B = 5: 280 row blocks, above the loss kernel's 256 workgroups,
# so workgroups 0..23 own two blocks.
CASES = {
    "main": (2, MAIN_SIZE, main_boxes()),
    "b1_g1_small": (1, (200, 152), synthetic_boxes(1, 1, seed=21)),
    "b3_g0": (3, MAIN_SIZE, None),
    "b3_zero_middle_small": (3, (200, 152), _zero_middle(3, 22)),
    "b1_g64": (1, MAIN_SIZE, _mixed(1, 64, 23)),
    "b5_g64_small": (5, (200, 152), _mixed(5, 64, 24)),
    "b5_g3": (5, MAIN_SIZE, _zero_middle(5, 25)),
}
