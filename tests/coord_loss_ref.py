"""A torch restatement of the coordinate loss on the decoded keypoints
(DESIGN.md §3k), differentiable, in the dtype and on the device of ``heat``
(float64 on the CPU: the reference of tests/test_coord_loss.py and
tests/test_trainer_coord.py; float32: the yardstick of what fp32 arithmetic
costs on the same formulas):

    p      = softmax(h / T) over each plane
    coords = (sum p x / (W - 1), sum p y / (H - 1))
    loss   = SpatialCoordinateLoss(loss_type, pixel_weight_scale, distance_threshold)(coords, gt, vis)

with the gt of masked joints (vis <= 0) replaced by 0 beforehand, so that an
arbitrary or NaN label there reaches nothing (the project's
SpatialCoordinateLoss masks by multiplying).
"""
from __future__ import annotations

from functools import lru_cache

import torch

KINK_MARGIN = 1e-3


def soft_argmax(heat: torch.Tensor, temperature: float) -> torch.Tensor:
    """heat [n,K,H,W] -> coords [n,K,2]."""
    n, K, H, W = heat.shape
    p = torch.softmax(heat.reshape(n, K, H * W) / temperature, dim=-1).reshape(n, K, H, W)
    xs = torch.arange(W, dtype=heat.dtype, device=heat.device) / (W - 1)
    ys = torch.arange(H, dtype=heat.dtype, device=heat.device) / (H - 1)
    return torch.stack([(p.sum(dim=2) * xs).sum(dim=-1), (p.sum(dim=3) * ys).sum(dim=-1)], dim=-1)


def coord_loss(heat: torch.Tensor, gt: torch.Tensor, vis: torch.Tensor, temperature: float = 1.0,
               loss_type: str = "smooth_l1", pixel_weight_scale: float = 100.0, distance_threshold: float = 5.0):
    """(loss 0-d, coords [n,K,2]); gt and vis are cast to heat's dtype."""
    from dll.losses import SpatialCoordinateLoss
    coords = soft_argmax(heat, temperature)
    vis = vis.to(heat.dtype)
    g = torch.where((vis > 0).unsqueeze(-1), gt.to(heat.dtype), torch.zeros((), dtype=heat.dtype, device=heat.device))
    return SpatialCoordinateLoss(loss_type, pixel_weight_scale, distance_threshold)(coords, g, vis), coords


def loss_and_grad(heat: torch.Tensor, gt, vis, dtype=torch.float64, device="cpu", **kw):
    """(loss, coords, d loss / d heat) of ``coord_loss`` on a fresh leaf of ``dtype`` on ``device``, detached.
    Without a visible joint SpatialCoordinateLoss returns a constant 0: the gradient is then zero."""
    h = heat.detach().to(device, dtype).requires_grad_(True)
    loss, coords = coord_loss(h, gt.to(device), vis.to(device), **kw)
    loss.backward()
    grad = h.grad if h.grad is not None else torch.zeros_like(h)
    return loss.detach(), coords.detach(), grad.detach()


def softargmax_vjp(heat: torch.Tensor, grad_coords: torch.Tensor, temperature: float, dtype=torch.float64,
                   device="cpu"):
    """(coords, d <coords, grad_coords> / d heat) through autograd, detached."""
    h = heat.detach().to(device, dtype).requires_grad_(True)
    coords = soft_argmax(h, temperature)
    (coords * grad_coords.to(device, dtype)).sum().backward()
    return coords.detach(), h.grad.detach()


def kink_distance(coords: torch.Tensor, gt: torch.Tensor, vis: torch.Tensor, distance_threshold: float):
    """The smallest distance of a visible joint from a kink of the loss -- ||z| - 1| of either coordinate
    difference, |d / tau - 1|, |d / tau - 3| -- and d / tau of the visible joints, in float64."""
    seen = vis > 0
    z = (coords.double() - gt.double())[seen]
    q = z.norm(dim=-1) / distance_threshold
    if z.numel() == 0:
        return float("inf"), q
    dist = torch.cat([(z.abs() - 1).abs().flatten(), (q - 1).abs(), (q - 3).abs()])
    return float(dist.min()), q


@lru_cache(maxsize=None)
def make_case(shape, temperature: float, distance_threshold: float, first_seed: int = 0):
    """Seeded inputs of one case, float32 on the CPU: (heat = sigmoid(normal), gt uniform in [-0.1, 1.1]^2 with
    one joint at x = 1.8 (the linear branch of rho), vis in {0, 1, 2} with about a quarter masked and that joint
    visible, seed).  The seed is the first from ``first_seed`` on at which no visible joint lies within
    KINK_MARGIN of a kink, judged on the float64 decode."""
    n, K, H, W = shape
    for seed in range(first_seed, first_seed + 64):
        g = torch.Generator().manual_seed(seed)
        heat = torch.sigmoid(torch.randn(n, K, H, W, generator=g))
        gt = torch.rand(n, K, 2, generator=g) * 1.2 - 0.1
        vis = torch.randint(0, 4, (n, K), generator=g).clamp_(max=2).float()
        j = min(1, K - 1)
        gt[0, j, 0], vis[0, j] = 1.8, 1.0
        with torch.no_grad():
            coords = soft_argmax(heat.double(), temperature)
        if kink_distance(coords, gt, vis, distance_threshold)[0] > KINK_MARGIN:
            return heat, gt, vis, seed
    raise AssertionError(f"no kink-free seed for {shape}, T={temperature}, tau={distance_threshold}")
