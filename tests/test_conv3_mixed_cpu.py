"""precision="mixed" of dll.ops.conv3x3 without a device: the
refusals that come before the device, the --amp switch of scripts/train.py,
and the CPU restatement (tests/conv3_mixed_ref.py) pinned against the
unrounded float64 convolution by the elementwise cap

    |mixed - exact| <= (2^-8 + 2^-18) * (|w| (*) |x|)

(a bf16 rounding moves a value by at most 2^-9 of itself, so a product of two
rounded operands by at most (1 + 2^-9)^2 - 1 of itself; the right side is the
same convolution of the absolute values), and the same for gx and gw with
their operand pairs.  Both sides are float64, so the accumulation adds ~1e-16
relative: 1e-12 of the cap's largest entry is allowed for it."""
import sys

import pytest
import torch

from conftest import PKG
from conv3_mixed_ref import CAP, bf16, exact_all, mixed_all

CONFIG = str(PKG / "configs" / "default_config.yaml")


def test_unknown_precision_raises_before_the_device():
    from dll.ops import conv3x3
    x, w, b = torch.zeros(1, 5, 9, 11), torch.zeros(7, 5, 3, 3), torch.zeros(7)
    with pytest.raises(ValueError, match="precision"):
        conv3x3(x, w, b, precision="bogus")
    with pytest.raises(ValueError, match="precision"):
        conv3x3(x, w, precision=None)


def test_head_train_precision_default():
    from dll.models.heatmap_head import HeatmapHead
    assert HeatmapHead.train_precision == "split"


def _train_module():
    if str(PKG / "scripts") not in sys.path:
        sys.path.insert(0, str(PKG / "scripts"))
    import train
    return train


def test_cli_amp_parses_and_argument_errors_come_before_the_device(tmp_path, capsys, monkeypatch):
    train = _train_module()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    for split in ("train", "val"):
        for sub in ("images", "labels"):
            (tmp_path / "data" / split / sub).mkdir(parents=True)
    good = ["--config", CONFIG, "--data_dir", str(tmp_path / "data"), "--output_dir", str(tmp_path / "out")]
    assert train.parse_args(good).amp is False
    assert train.parse_args(good + ["--amp"]).amp is True
    for argv, word in ((good + ["--amp", "--epochs", "0"], "--epochs must be at least 1"),
                       (good + ["--amp", "yes"], "unrecognized arguments"),
                       (good[:-2] + ["--amp"], "output_dir")):
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
    assert not (tmp_path / "out").exists()


def test_bf16_helper_rounds_from_the_fp32_value():
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 3.0, -2.0 ** -100], dtype=torch.float64)
    # ties to even at 1 + 2^-8; the 2^-30 is gone in fp32 first (the device never sees it)
    assert bf16(t).tolist() == [1.0, 1.0, 3.0, -2.0 ** -100]
    assert bf16(t).dtype == torch.float64


@pytest.mark.parametrize("shape", [(1, 5, 9, 11, 7), (2, 64, 14, 14, 32)])
def test_restatement_within_the_cap_of_plain_float64(shape):
    N, C, H, W, O = shape
    g = torch.Generator().manual_seed(N * 1000 + C + O)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(O, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(O, generator=g) * 0.1
    gy = torch.randn(N, O, H, W, generator=g)
    got = mixed_all(x, w, b, gy, torch.float64)
    exact, caps = exact_all(x, w, b, gy)
    for name, u, v, cap in zip(("y", "gx", "gw"), got, exact, caps):
        excess = ((u - v).abs() - CAP * cap).max().item()
        print(f"{name}: max|mixed - exact| {(u - v).abs().max().item():.3e}, max cap {CAP * cap.max().item():.3e}")
        assert (u - v).abs().max() > 0, f"{name}: the restatement did not round"
        assert excess <= 1e-12 * cap.max().item(), f"{name}: {excess:.3e} over the cap"
    assert torch.equal(got[3], gy.double().sum(dim=(0, 2, 3)))     # gb: unrounded gy
