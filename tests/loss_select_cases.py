"""Inputs that put the adaptive heatmap loss's threshold select
(keypoint-detection_amd/csrc/loss_kernels.hip: a 4-pass radix select over an order-preserving key,
then a successor search) on its edges, shared by tests/test_loss_select_edges.py
(device) and tests/test_train_edges_cpu.py (the preconditions, on torch alone).
Needs no GPU.

The threshold is clamp(quantile(gt, 0.9), 0.05, 0.3).  The clamp hides a wrong
select whenever the quantile falls outside (0.05, 0.3), so every case but the
ones marked ``clamped`` keeps the unclamped quantile strictly inside the band:
``check_band`` asserts it."""
import struct

import torch

Q, LO, HI = 0.9, 0.05, 0.3


def bits(v: float) -> int:
    return struct.unpack("<I", struct.pack("<f", v))[0]


def from_bits(b: int) -> float:
    return struct.unpack("<f", struct.pack("<I", b & 0xFFFFFFFF))[0]


def key(v: float) -> int:
    """The kernel's order-preserving unsigned image of a float."""
    u = bits(v)
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def rank_of(n: int):
    """floor(0.9f * (n - 1)) and the lerp weight, in fp32 as torch.quantile computes them."""
    r = torch.tensor(Q, dtype=torch.float32) * (n - 1)
    below = int(r.floor().item())
    return below, float((r - below).item())


def planted(n, lo, hi, seed, copies_below=0):
    """n fp32 values, shuffled by a seeded permutation, whose sorted order has
    ``lo`` at rank floor(0.9f (n - 1)) and ``hi`` at the next rank; the ranks
    below hold distinct values in (0.051, lo) -- the ``copies_below`` ranks just
    under the selected one hold copies of ``lo`` instead -- and the ranks above
    hold distinct values in (hi, 0.299).  Returns (x, rank, lo, hi) with lo and
    hi as fp32 tensors."""
    rank, _ = rank_of(n)
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    assert 0.051 < float(lo_t) <= float(hi_t) < 0.299 and rank + 1 < n and copies_below <= rank
    nb, na = rank - copies_below, n - rank - 2
    below = torch.linspace(0.051, float(lo_t), nb + 2, dtype=torch.float64)[1:-1].float()
    above = torch.linspace(float(hi_t), 0.299, na + 2, dtype=torch.float64)[1:-1].float()
    assert bool((below < lo_t).all()) and bool((above > hi_t).all())
    v = torch.cat([below, lo_t.repeat(copies_below + 1), hi_t.view(1), above])
    assert v.numel() == n
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return v[perm].contiguous(), rank, lo_t, hi_t


def _uniform(n, a, b, seed):
    return a + (b - a) * torch.rand(n, generator=torch.Generator().manual_seed(seed))


def _zeros_and_denormals(n=2000, seed=21):
    """80 % low tail, half of it -0.0, +0.0 and denormals of both signs (the
    rest negative and small positive normals); 20 % inside the band."""
    g = torch.Generator().manual_seed(seed)
    n_low = n * 8 // 10
    n_odd = n_low // 2
    den = torch.tensor([from_bits(b) for b in (1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00000100, 0x80010000)])
    odd = torch.cat([torch.tensor([-0.0, 0.0]), den])[torch.randint(0, 8, (n_odd,), generator=g)]
    low = -0.5 + 0.54 * torch.rand(n_low - n_odd, generator=g)
    top = 0.06 + 0.23 * torch.rand(n - n_low, generator=g)
    v = torch.cat([odd, low, top])
    return v[torch.randperm(n, generator=g)].contiguous()


def _levels(n, seed):
    """n draws from 64 distinct levels inside the band: heavy ties."""
    lv = (0.06 + 0.0035 * torch.arange(64, dtype=torch.float64)).float()
    return lv[torch.randint(0, 64, (n,), generator=torch.Generator().manual_seed(seed))].contiguous()


def _consecutive(n=1000, seed=23):
    """n consecutive bit patterns from the bits of 0.1f: they differ in the low
    key byte alone and cross second-byte boundaries."""
    b0 = bits(0.1)
    v = (torch.arange(n, dtype=torch.int64) + b0).to(torch.int32).view(torch.float32)
    return v[torch.randperm(n, generator=torch.Generator().manual_seed(seed))].contiguous()


_FF_LOW = from_bits(bits(0.17) | 0xFF)                           # key byte 0 = 0xFF; the next float carries into byte 1
_FF_SECOND = from_bits((bits(0.17) & ~0xFFFF) | 0xFF00 | 0x37)   # key byte 1 = 0xFF
_TOP_BYTE_LO, _TOP_BYTE_HI = from_bits(0x3DFFFFFF), from_bits(0x3E000000)   # neighbours that differ in the highest key byte

# name -> (builder, clamped side or None)
CASES = {
    "negatives_1000": (lambda: _uniform(1000, -1.0, 0.25, 31), None),
    "negatives_4097": (lambda: _uniform(4097, -1.0, 0.25, 32), None),
    "zeros_denormals": (_zeros_and_denormals, None),
    "ff_low_byte": (lambda: planted(1000, _FF_LOW, from_bits(bits(_FF_LOW) + 1), 41)[0], None),
    "ff_second_byte": (lambda: planted(1000, _FF_SECOND, from_bits(bits(_FF_SECOND) + 0x200), 42)[0], None),
    "top_byte_neighbours": (lambda: planted(1000, _TOP_BYTE_LO, _TOP_BYTE_HI, 43)[0], None),
    "consecutive_bits": (_consecutive, None),
    "followed_by_copy": (lambda: planted(1000, 0.2, 0.2, 44)[0], None),
    "copy_below_then_larger": (lambda: planted(1000, 0.2, 0.21, 45, copies_below=1)[0], None),
    "n1": (lambda: torch.tensor([0.2]), None),
    "n2": (lambda: torch.tensor([0.2, 0.1]), None),
    "n3": (lambda: torch.tensor([0.25, 0.1, 0.2]), None),
    "all_equal_in_band": (lambda: torch.full((777,), 0.17), None),
    "all_equal_high": (lambda: torch.full((777,), 0.5), "high"),
    "all_equal_negative": (lambda: torch.full((777,), -3.0), "low"),
    "grid_minus_1": (lambda: _levels(1024 * 256 - 1, 51), None),
    "grid_exact": (lambda: _levels(1024 * 256, 52), None),
    "grid_plus_1": (lambda: _levels(1024 * 256 + 1, 53), None),
}
_BUILT = {}


def build(name):
    """The case's values (1-D fp32), built once and never modified."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name][0]()
    return _BUILT[name]


def check_band(name):
    """The precondition, on the CPU: torch's unclamped quantile strictly inside
    (0.05, 0.3), or on the stated side of it for a clamped case.  Returns the
    threshold torch computes: clamp(quantile(x, 0.9), 0.05, 0.3) in fp32."""
    x, side = build(name), CASES[name][1]
    assert x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    q = float(torch.quantile(x, Q))
    if side is None:
        assert LO < q < HI, f"{name}: quantile {q} is not inside the band, the clamp would hide the select"
    elif side == "high":
        assert q > HI, f"{name}: quantile {q} should be clamped from above"
    else:
        assert q < LO, f"{name}: quantile {q} should be clamped from below"
    return torch.clamp(torch.quantile(x, Q), LO, HI)


# ---------------------------------------------------------------- loss and gradient inputs
LOSS_SHAPE = (2, 3, 9, 7)


def loss_inputs(min_gap=0.02, seed=61):
    """pred, gt of LOSS_SHAPE with |pred - gt| in [min_gap, 0.5]: for a focal
    exponent below 1 the gradient of (1 - exp(-mse))^alpha is not finite at
    mse == 0, in the reference as on the device."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(*LOSS_SHAPE, generator=g) * 0.6
    gap = min_gap + (0.5 - min_gap) * torch.rand(*LOSS_SHAPE, generator=g)
    sign = torch.randint(0, 2, LOSS_SHAPE, generator=g).float() * 2 - 1
    return (gt + sign * gap).contiguous(), gt.contiguous()


def oracle_loss_and_grad(pred, gt, tw, alpha):
    """(loss, d loss / d pred) of oracle/loss_oracle.py with autograd."""
    from oracle import loss_oracle
    p = pred.clone().requires_grad_(True)
    loss = loss_oracle.adaptive_heatmap_loss(p, gt, tw, 50.0, 1.0, True, alpha)
    loss.backward()
    return loss.detach(), p.grad
