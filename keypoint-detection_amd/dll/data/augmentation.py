"""Training augmentation on the device -- what the reference's
``AugmentationConfig`` (flip, rotate.max_angle, scale.range, prob) promises and
its ``KeypointAugmentation.__call__`` leaves as a stub ("Implement flip logic
here", dll/data/augmentation.py:29-33).

``kpd_augment_batch`` (csrc/augment.hip) warps a batch of uint8 images by a
per-image affine map -- mirror, rotation and zoom about the image centre --
with optional brightness / contrast, and moves the labels with the pixels in
the same launch: keypoints are mapped (left / right joints swapped on a
mirror), joints that leave the frame lose their visibility, boxes are re-hulled
and clipped.  The rules are written out in DESIGN.md §3f and include/kpd.h;
``tests/augment_ref.py`` restates them in numpy (images bit-equal).

The host only builds the per-image matrices, in float64 (``AugmentParams.
matrices``).  For an image of W x H with centre c = ((W-1)/2, (H-1)/2):

    A  = s * [[cos t, -sin t], [sin t, cos t]] * diag(-1 if mirror else 1, 1)
    p' = c + A (p - c)                                   forward, pixel indices
    q  = floor([A^-1 | c - A^-1 c] * 65536 + 0.5)        inverse, Q16 (the kernel's gather)
    N  = the forward map for normalised coordinates, px = x * W - 0.5, x' = (px' + 0.5) / W

There is no CPU fallback: a CPU tensor raises.  Parity with OpenCV's
``warpAffine`` (whose 1/32-pixel grid the image rule follows) is unpinned --
OpenCV is absent here -- and the effect on accuracy is unmeasured: no dataset
run of ``dll.training.Trainer`` has been made.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _native

SAMPLE_COLUMNS = 8   # uniform draws per image; their roles are fixed (KeypointAugmentation.sample)


@dataclass
class AugmentParams:
    """Per-image augmentation parameters (host numpy arrays of n entries):
    ``mirror`` bool, ``angle_deg`` and ``scale`` float64, ``gain`` and
    ``offset`` int32 in Q8 (identity 256 and 0)."""
    mirror: np.ndarray
    angle_deg: np.ndarray
    scale: np.ndarray
    gain: np.ndarray
    offset: np.ndarray

    def __post_init__(self):
        self.mirror = np.atleast_1d(np.asarray(self.mirror)).astype(bool)
        self.angle_deg = np.atleast_1d(np.asarray(self.angle_deg, dtype=np.float64))
        self.scale = np.atleast_1d(np.asarray(self.scale, dtype=np.float64))
        self.gain = np.atleast_1d(np.asarray(self.gain)).astype(np.int32)
        self.offset = np.atleast_1d(np.asarray(self.offset)).astype(np.int32)
        n = len(self.mirror)
        if any(a.ndim != 1 or len(a) != n for a in (self.angle_deg, self.scale, self.gain, self.offset)):
            raise ValueError("AugmentParams: every field needs one entry per image")
        if not (self.scale > 0).all():
            raise ValueError("AugmentParams: scale must be positive")

    def __len__(self) -> int:
        return len(self.mirror)

    @classmethod
    def identity(cls, n: int) -> "AugmentParams":
        return cls(np.zeros(n, bool), np.zeros(n), np.ones(n), np.full(n, 256, np.int32), np.zeros(n, np.int32))

    def matrices(self, W, H) -> Tuple[np.ndarray, np.ndarray]:
        """(q int32 [n, 6], N float64 [n, 6]) for images of ``W`` x ``H`` (scalars or
        one value per image), built in float64 on the host: the rows of the
        module docstring, (m00 m01 m02 m10 m11 m12) per image."""
        n = len(self)
        W = np.broadcast_to(np.asarray(W, dtype=np.float64), (n,))
        H = np.broadcast_to(np.asarray(H, dtype=np.float64), (n,))
        t = np.deg2rad(self.angle_deg)
        c, s = np.cos(t), np.sin(t)
        mx = np.where(self.mirror, -1.0, 1.0)
        a00, a01, a10, a11 = self.scale * c * mx, -self.scale * s, self.scale * s * mx, self.scale * c
        i00, i01, i10, i11 = mx * c / self.scale, mx * s / self.scale, -s / self.scale, c / self.scale   # A^-1
        cx, cy = (W - 1) / 2, (H - 1) / 2
        inv = np.stack([i00, i01, cx - (i00 * cx + i01 * cy), i10, i11, cy - (i10 * cx + i11 * cy)], axis=1)
        q = np.floor(inv * 65536.0 + 0.5)
        if (np.abs(q) >= 2.0 ** 31).any():
            raise ValueError("AugmentParams.matrices: the Q16 inverse map does not fit 32 bits")
        N = np.stack([a00, a01 * H / W, (W / 2 - a00 * W / 2 - a01 * H / 2) / W,
                      a10 * W / H, a11, (H / 2 - a10 * W / 2 - a11 * H / 2) / H], axis=1)
        return q.astype(np.int32), np.ascontiguousarray(N, dtype=np.float64)


def _fill3(fill) -> Tuple[int, int, int]:
    f = [int(fill)] * 3 if np.isscalar(fill) else [int(v) for v in fill]
    if len(f) == 1:
        f = f * 3
    if len(f) != 3 or any(not 0 <= v <= 255 for v in f):
        raise ValueError("fill must be one value or three, each in [0, 255]")
    return tuple(f)


def augment_batch(images: Sequence[torch.Tensor], keypoints: Optional[torch.Tensor] = None,
                  visibilities: Optional[torch.Tensor] = None, boxes: Optional[torch.Tensor] = None, *,
                  params: AugmentParams, pairs: Optional[Sequence[int]] = None, fill=0):
    """Warp ``images`` -- uint8 CUDA tensors [H,W] or [H,W,C] on one GPU, any
    sizes, one channel count (1 or 3) -- by ``params`` in one native call
    (kpd_augment_batch) and move the labels with them: ``keypoints`` [n,P,K,2]
    normalised, ``visibilities`` [n,P,K], ``boxes`` [n,P,4] cxcywh, all three or
    none.  ``pairs`` is the joint map of a mirror (default
    ``dll.utils.flip.flip_index(K)``), ``fill`` the colour outside the source.

    Returns the new images (views of one allocation, shaped like the inputs),
    or ``(images, keypoints, visibilities, boxes)`` when labels were given: new
    fp32 device tensors of the input shapes.  An image whose pixels are dense
    within each row is read in place at its row pitch; any other layout is made
    contiguous first.  A person's joints follow the joint rule whatever became
    of its box.  The call does not synchronise."""
    images = list(images)
    n = len(images)
    if len(params) != n:
        raise ValueError(f"augment_batch: {len(params)} parameter sets for {n} images")
    labels = (keypoints, visibilities, boxes)
    have = [t is not None for t in labels]
    if any(have) and not all(have):
        raise ValueError("augment_batch: keypoints, visibilities and boxes go together")
    if n == 0:
        if not all(have):
            return []
        return ([],) + tuple(torch.as_tensor(t).clone() for t in labels)
    imgs, flat = [], []
    for image in images:
        if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
            raise TypeError("augment_batch expects uint8 CUDA tensors [H,W] or [H,W,C]")
        _native._require_cuda(image, "image")
        if image.dim() not in (2, 3):
            raise TypeError("augment_batch expects uint8 CUDA tensors [H,W] or [H,W,C]")
        img = image if image.dim() == 3 else image[:, :, None]
        h, w, c = img.shape
        if h > 0 and w > 0 and not (img.stride(2) == 1 and img.stride(1) == c and (h == 1 or img.stride(0) >= w * c)):
            img = img.contiguous()
        imgs.append(img)
        flat.append(image.dim() == 2)
    dev, C = imgs[0].device, imgs[0].shape[2]
    if any(i.device != dev for i in imgs) or any(i.shape[2] != C for i in imgs):
        raise ValueError("augment_batch: the images must share one device and one channel count")
    hs, ws = [i.shape[0] for i in imgs], [i.shape[1] for i in imgs]
    ps = [i.stride(0) if i.shape[0] > 1 else i.shape[1] * C for i in imgs]
    P = K = 0
    kp = vis = bx = kp_out = vis_out = bx_out = None
    pr = None
    if all(have):
        kp, vis, bx = (_native._dev_f32(torch.as_tensor(t), name) for t, name in
                       zip(labels, ("keypoints", "visibilities", "boxes")))
        if kp.dim() != 4 or kp.shape[0] != n or kp.shape[3] != 2:
            raise ValueError(f"keypoints must be [{n}, P, K, 2], got {list(kp.shape)}")
        P, K = kp.shape[1], kp.shape[2]
        if tuple(vis.shape) != (n, P, K) or tuple(bx.shape) != (n, P, 4):
            raise ValueError(f"visibilities must be [{n}, {P}, {K}] and boxes [{n}, {P}, 4], got "
                             f"{list(vis.shape)} and {list(bx.shape)}")
        if any(t.device != dev for t in (kp, vis, bx)):
            raise ValueError(f"augment_batch: the labels must be on {dev}")
        if pairs is None:
            from ..utils.flip import flip_index
            pairs = flip_index(K)
        pr = [int(v) for v in pairs]
        if len(pr) != K:
            raise ValueError(f"{len(pr)} flip pairs for {K} keypoints")
        kp_out, vis_out, bx_out = torch.empty_like(kp), torch.empty_like(vis), torch.empty_like(bx)
    q, N = params.matrices(ws, hs)
    # one allocation; every image starts on a 16-byte boundary, so its rows can leave as whole dwords
    offs, total = [], 0
    for h, w in zip(hs, ws):
        offs.append(total)
        total += (h * w * C + 15) // 16 * 16
    buf = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    if len(set(zip(hs, ws))) == 1:   # one size: the views in three tensor operations, not 2 n
        outs = list(buf.view(n, total // n)[:, :hs[0] * ws[0] * C].view(n, hs[0], ws[0], C).unbind(0))
    else:
        outs = [buf[o:o + h * w * C].view(h, w, C) for o, h, w in zip(offs, hs, ws)]
    base = buf.data_ptr()
    ints = ctypes.c_int * n
    ptr = _native._ptr
    q, N = np.ascontiguousarray(q, np.int32), np.ascontiguousarray(N, np.float64)   # read in place by the call
    mirror = params.mirror.astype(np.intc)
    gain, offset = np.ascontiguousarray(params.gain, np.int32), np.ascontiguousarray(params.offset, np.int32)
    i32p, ip = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)
    with torch.cuda.device(dev):
        rc = _native.load().kpd_augment_batch(
            (ctypes.c_void_p * n)(*[i.data_ptr() for i in imgs]), ints(*hs), ints(*ws), ints(*ps),
            (ctypes.c_void_p * n)(*[base + o for o in offs]), n, C,
            q.ctypes.data_as(i32p), N.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mirror.ctypes.data_as(ip),
            gain.ctypes.data_as(i32p), offset.ctypes.data_as(i32p),
            (ctypes.c_uint8 * 3)(*_fill3(fill)), None if pr is None else (ctypes.c_int32 * max(K, 1))(*pr),
            ptr(kp), ptr(vis), ptr(bx), P, K, ptr(kp_out), ptr(vis_out), ptr(bx_out), _native._stream(dev))
    _native.check(rc, "kpd_augment_batch")
    outs = [o[:, :, 0] if f else o for o, f in zip(outs, flat)]
    if not all(have):
        return outs
    return outs, kp_out, vis_out, bx_out


class KeypointAugmentation:
    """The reference's ``KeypointAugmentation`` (same constructor argument and
    call), implemented: ``config`` is a ``TrainingConfig`` (default: a new one)
    whose ``augmentation`` block is kept as ``.config``; ``seed`` seeds the CPU
    generator the parameters are drawn from."""

    def __init__(self, config=None, seed: Optional[int] = None, device: Union[str, torch.device] = "cuda"):
        if config is None:
            from ..configs.training_config import TrainingConfig
            config = TrainingConfig()
        self.config = config.augmentation
        self.config.validate()
        self.device = torch.device(device)
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))

    def sample(self, n: int) -> AugmentParams:
        """Parameters of n images from ``u = torch.rand(n, 8, float64)`` of the
        seeded CPU generator.  Each enabled transform is applied on its own
        with probability ``prob``; the columns' roles are fixed:

            0        mirror gate          mirror on
            1, 2     rotate gate, angle   (2u - 1) * max_angle
            3, 4     scale gate, scale    lo + u * (hi - lo)
            5, 6, 7  colour gate, brightness, contrast
                     gain = round(256 * (1 + (2 u7 - 1) * contrast)),
                     offset = round(256 * 255 * (2 u6 - 1) * brightness)

        A gate passes when u < prob; a transform that is disabled or not
        selected takes its identity value."""
        cfg = self.config
        u = torch.rand(int(n), SAMPLE_COLUMNS, dtype=torch.float64, generator=self.generator).numpy()
        gate = u < float(cfg.prob)
        flip_on = bool(cfg.flip.get("enabled", False)) and bool(cfg.flip.get("horizontal", False))
        rot_on, scale_on = bool(cfg.rotate.get("enabled", False)), bool(cfg.scale.get("enabled", False))
        color_on = bool(cfg.color.get("enabled", False))
        lo, hi = (float(v) for v in cfg.scale.get("range", (1.0, 1.0)))
        mirror = gate[:, 0] & flip_on
        angle = np.where(gate[:, 1] & rot_on, (2 * u[:, 2] - 1) * float(cfg.rotate.get("max_angle", 0.0)), 0.0)
        scale = np.where(gate[:, 3] & scale_on, lo + u[:, 4] * (hi - lo), 1.0)
        col = gate[:, 5] & color_on
        gain = np.where(col, np.rint(256 * (1 + (2 * u[:, 7] - 1) * float(cfg.color.get("contrast", 0.0)))), 256)
        offset = np.where(col, np.rint(256 * 255 * (2 * u[:, 6] - 1) * float(cfg.color.get("brightness", 0.0))), 0)
        return AugmentParams(mirror, angle, scale, np.clip(gain, 0, 65535), np.clip(offset, -(2 ** 24 - 1), 2 ** 24 - 1))

    def _image(self, image) -> torch.Tensor:
        if isinstance(image, torch.Tensor):
            t = image
        else:   # PIL image or array-like, as ITransform takes them
            a = np.asarray(image.convert("RGB") if hasattr(image, "convert") and getattr(image, "mode", "RGB")
                           not in ("RGB", "L") else image)
            t = torch.from_numpy(np.array(a, dtype=np.uint8, copy=True))
        if t.dtype != torch.uint8:
            raise TypeError("KeypointAugmentation expects 8-bit images")
        return t.to(self.device, non_blocking=True)

    def __call__(self, image, keypoints, visibilities, bboxes):
        """The reference's call: ``image`` a PIL image, array or uint8 tensor,
        ``keypoints`` [1,P,K,2], ``visibilities`` [1,P,K], ``bboxes`` a list
        holding one [P,4] tensor (or that tensor).  Returns the augmented uint8
        device tensor and the labels in the same structures, on the device.
        With ``enabled == False`` the inputs come back untouched, as in the
        reference."""
        if not self.config.enabled:
            return image, keypoints, visibilities, bboxes
        img = self._image(image)
        as_list = isinstance(bboxes, (list, tuple))
        if as_list and len(bboxes) != 1:
            raise ValueError("KeypointAugmentation: bboxes must hold one [P, 4] tensor")
        bx = torch.as_tensor(bboxes[0] if as_list else bboxes)
        kp, vis = torch.as_tensor(keypoints), torch.as_tensor(visibilities)
        if kp.dim() != 4 or kp.shape[0] != 1:
            raise ValueError(f"KeypointAugmentation: keypoints must be [1, P, K, 2], got {list(kp.shape)}")
        P = kp.shape[1]
        if bx.numel() != P * 4:
            raise ValueError(f"KeypointAugmentation: {P} persons but boxes {list(bx.shape)}")
        fill = self.config.fill
        outs, kp2, vis2, bx2 = augment_batch([img], kp.to(self.device), vis.to(self.device).reshape(1, P, -1),
                                             bx.to(self.device).reshape(1, P, 4), params=self.sample(1), fill=fill)
        bx2 = bx2.reshape(bx.shape)
        return outs[0], kp2, vis2.reshape(vis.shape), ([bx2] if as_list else bx2)
