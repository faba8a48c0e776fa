"""ctypes binding of libkpd.so (include/kpd.h).

The product path has no CPU fallback: if the library is missing or fails to
load, every entry point raises ``KpdNativeError`` loudly.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import List, Optional

import torch

_LIB_PATH = Path(__file__).resolve().parent / "_lib" / "libkpd.so"
_lib: Optional[ctypes.CDLL] = None

KPD_PRECISION_FP32 = 0
KPD_PRECISION_MIXED = 1
KPD_PRECISION_SPLIT = 2
# "fp32": every conv on fp32-input MFMA; "split": fp32-accurate -- FPN level 0
# and the heatmap-head convs as three f16 MFMA products of hi/lo operand
# splits (fp32 tolerances); "mixed": split FPN level 0 + bf16 heatmap convs
PRECISIONS = {"fp32": KPD_PRECISION_FP32, "split": KPD_PRECISION_SPLIT, "mixed": KPD_PRECISION_MIXED,
              "bf16": KPD_PRECISION_MIXED}

# every symbol include/kpd.h declares (checked by tests/test_abi.py)
EXPORTS = ("kpd_last_error", "kpd_version", "kpd_plan_create", "kpd_plan_set_tensor",
           "kpd_plan_finalize", "kpd_plan_destroy", "kpd_forward", "kpd_debug_copy", "kpd_nms",
           "kpd_plan_timing", "kpd_plan_timing_stage", "kpd_plan_timing_query", "kpd_plan_set_detector",
           "kpd_bench_conv16", "kpd_build_flags", "kpd_fpn0x_class_table",
           "kpd_plan_set_streams", "kpd_preprocess", "kpd_target_heatmaps", "kpd_keypoint_metrics",
           "kpd_heatmap_head", "kpd_keypoint_head", "kpd_backbone", "kpd_channel_attention", "kpd_decode_heatmaps",
           "kpd_roi_align", "kpd_conv1x1", "kpd_adaptive_heatmap_loss", "kpd_conv3x3_forward",
           "kpd_conv3x3_backward", "kpd_conv3x3_forward_prec", "kpd_conv3x3_backward_prec", "kpd_plan_set_graphs", "kpd_backbone_body", "kpd_backbone_fpn",
           "kpd_plan_path_log", "kpd_plan_path_query", "kpd_preprocess_batch", "kpd_draw_poses",
           "kpd_oks_match", "kpd_pose_nms", "kpd_flip_merge", "kpd_augment_batch", "kpd_bn_train_forward",
           "kpd_bn_train_backward", "kpd_roi_targets", "kpd_roi_features", "kpd_detector_features",
           "kpd_detector_targets", "kpd_detector_loss", "kpd_coord_loss", "kpd_softargmax_backward",
           "kpd_roi_align_backward", "kpd_track_state_bytes", "kpd_track_poses")
PRE_BATCH_CHUNK = 32   # KPD_PRE_BATCH_CHUNK: images per descriptor table (launches grow per chunk, not per image)
# kpd_draw_poses (include/kpd.h): layer flags, images per descriptor table, one workgroup's tile, limits
DRAW_BOXES, DRAW_LIMBS, DRAW_JOINTS, DRAW_HEAT = 1, 2, 4, 8
DRAW_CHUNK = 32        # KPD_DRAW_CHUNK
DRAW_TILE_W = 64       # KPD_DRAW_TILE_W
DRAW_TILE_H = 16       # KPD_DRAW_TILE_H
DRAW_MAX_SIDE = 16384  # KPD_DRAW_MAX_SIDE
DRAW_MAX_WIDTH = 512   # KPD_DRAW_MAX_WIDTH: 32 px in 1/16-pixel units
DRAW_MAX_HEAT = 1024   # KPD_DRAW_MAX_HEAT
# kpd_oks_match (include/kpd.h): limits of one call
OKS_MAX_K = 32         # KPD_OKS_MAX_K: keypoints per pose
OKS_MAX_T = 16         # KPD_OKS_MAX_T: OKS thresholds, one wave each
OKS_MAX_D = 64         # KPD_OKS_MAX_D: detection slots per image
OKS_MAX_G = 64         # KPD_OKS_MAX_G: ground-truth slots per image
# kpd_pose_nms (include/kpd.h): limits of one call and the suppression modes
POSE_NMS_MAX_D = 64    # KPD_POSE_NMS_MAX_D: pose slots per image, one lane each
POSE_NMS_MAX_K = 32    # KPD_POSE_NMS_MAX_K: keypoints per pose
POSE_NMS_HARD, POSE_NMS_SOFT, POSE_NMS_SOFT_LINEAR = 0, 1, 2
# kpd_track_poses (include/kpd.h): limits of one call
TRACK_MAX_T = 64       # KPD_TRACK_MAX_T: tracks per sequence, one lane each
TRACK_MAX_D = 64       # KPD_TRACK_MAX_D: pose slots per frame
TRACK_MAX_K = 32       # KPD_TRACK_MAX_K: keypoints per pose
# kpd_flip_merge (include/kpd.h): limits of one call
FLIP_MAX_K = 32        # KPD_FLIP_MAX_K: keypoints per pose
FLIP_MAX_SIDE = 1024   # KPD_FLIP_MAX_SIDE: heatmap height / width
# kpd_augment_batch (include/kpd.h): images per descriptor table, one workgroup's tile, limits
AUG_CHUNK = 16         # KPD_AUG_CHUNK
AUG_TILE_W = 64        # KPD_AUG_TILE_W
AUG_TILE_H = 16        # KPD_AUG_TILE_H
AUG_MAX_SIDE = 16384   # KPD_AUG_MAX_SIDE
AUG_MAX_K = 32         # KPD_AUG_MAX_K: keypoints per pose
FLAG_DETECT = 1
FLAG_DUAL_HEAD = 2
FLAG_FULL_LEVEL0 = 4   # store all of FPN level 0 (debug copy "feat0"); default: only the ROI-align footprints
FPN_IN_CHANNELS = (16, 24, 48, 576)   # LightweightFPN's lateral input widths (backbone.py)
HEAD_CHANNEL_ATT, HEAD_SPATIAL_ATT, HEAD_CONVS, HEAD_ALL = 1, 2, 4, 7
BN_RELU = 1            # KPD_BN_RELU
DET_ANCHORS = 28224    # KPD_DET_ANCHORS: 56 x 56 cells x 9 anchors, candidate order (i, j, a)
DET_MAX_GT = 64        # KPD_DET_MAX_GT: ground-truth slots per image
DECODE_ARGMAX, DECODE_SUBPIXEL, DECODE_SOFTARGMAX, DECODE_MODEL = 0, 1, 2, 3
COORD_LOSS_TYPES = {"smooth_l1": 0, "mse": 1, "huber": 2}   # KPD_COORD_SMOOTH_L1 / _MSE / _HUBER
STAGES = ("body", "fpn_lateral", "fpn0", "topk", "person_detect", "roi_align", "hm_attention", "hm_conv1",
          "hm_conv2", "hm_conv3", "hm_final_decode", "keypoint_head")


class KpdNativeError(RuntimeError):
    pass


def lib_path() -> Path:
    """libkpd.so next to this package; KPD_LIB overrides the path, and
    KPD_DIAG_LIB=1 selects the diagnostic build (make diag: libkpd_diag.so,
    which reads the KPD_* A/B / ablation switches -- measurement tools only)."""
    if "KPD_LIB" in os.environ:
        return Path(os.environ["KPD_LIB"])
    if os.environ.get("KPD_DIAG_LIB") == "1":
        return _LIB_PATH.with_name("libkpd_diag.so")
    return _LIB_PATH


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not p.exists():
        raise KpdNativeError(f"libkpd.so not found at {p}; build it with "
                             f"`make -C keypoint-detection_amd/csrc` (or __graft_entry__.build())")
    lib = ctypes.CDLL(str(p))
    c_int, c_void_p, c_char_p = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p
    lib.kpd_last_error.restype = c_char_p
    lib.kpd_version.restype = c_char_p
    lib.kpd_plan_create.argtypes = [c_int, c_int, ctypes.POINTER(c_void_p)]
    lib.kpd_plan_set_tensor.argtypes = [c_void_p, c_char_p, c_void_p, ctypes.POINTER(ctypes.c_int64), c_int]
    lib.kpd_plan_finalize.argtypes = [c_void_p, c_int]
    lib.kpd_plan_destroy.argtypes = [c_void_p]
    lib.kpd_plan_destroy.restype = None
    lib.kpd_forward.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.kpd_plan_set_detector.argtypes = [c_void_p, ctypes.c_float, ctypes.c_float]
    lib.kpd_debug_copy.argtypes = [c_void_p, c_char_p, c_void_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_size_t), c_void_p]
    lib.kpd_plan_timing.argtypes = [c_void_p, c_int]
    lib.kpd_plan_timing_stage.argtypes = [c_void_p, c_char_p]
    lib.kpd_plan_timing_query.argtypes = [c_void_p, c_char_p, ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(c_int)]
    lib.kpd_plan_path_log.argtypes = [c_void_p, c_int]
    lib.kpd_plan_path_query.argtypes = [c_void_p, c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    lib.kpd_target_heatmaps.argtypes = [c_void_p, c_int, c_int, c_int, ctypes.c_double, c_void_p, c_void_p]
    lib.kpd_keypoint_metrics.argtypes = [c_void_p, c_void_p, c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_float),
                                         c_int, c_void_p, c_void_p]
    lib.kpd_preprocess_batch.argtypes = [ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                         ctypes.POINTER(c_int), c_int, c_int, c_int, ctypes.c_float, c_int, c_int,
                                         c_int, c_int, ctypes.POINTER(ctypes.c_float),
                                         ctypes.POINTER(ctypes.c_float), c_void_p, c_void_p]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.kpd_draw_poses.argtypes = [ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                   ctypes.POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, u8p, u8p, u8p,
                                   c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.kpd_oks_match.argtypes = [c_void_p] * 8 + [ctypes.POINTER(ctypes.c_float)] * 2 + [c_int] * 6 + \
        [c_void_p] * 8
    lib.kpd_pose_nms.argtypes = [c_void_p] * 5 + [ctypes.POINTER(ctypes.c_float)] + [c_int] * 4 + \
        [ctypes.c_float] * 3 + [c_int] + [c_void_p] * 6
    lib.kpd_flip_merge.argtypes = [c_void_p] * 3 + [ctypes.POINTER(ctypes.c_int32)] + [c_int] * 5 + [c_void_p] * 5
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.kpd_augment_batch.argtypes = [ctypes.POINTER(c_void_p)] + [ctypes.POINTER(c_int)] * 3 + \
        [ctypes.POINTER(c_void_p), c_int, c_int, i32p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int),
         i32p, i32p, u8p, i32p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.kpd_fpn0x_class_table.argtypes = [ctypes.POINTER(c_int)] * 4
    lib.kpd_nms.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_void_p, c_void_p, c_void_p]
    c_float = ctypes.c_float
    lib.kpd_heatmap_head.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p]
    lib.kpd_keypoint_head.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.kpd_backbone.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]
    lib.kpd_backbone_body.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]
    lib.kpd_backbone_fpn.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                     ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.kpd_channel_attention.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                          c_void_p, c_void_p]
    lib.kpd_decode_heatmaps.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                        c_void_p]
    lib.kpd_roi_align.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_int,
                                  c_int, c_void_p, c_void_p]
    lib.kpd_conv1x1.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.kpd_adaptive_heatmap_loss.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                              c_float, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.kpd_conv3x3_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                        c_void_p]
    lib.kpd_conv3x3_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p]
    lib.kpd_conv3x3_forward_prec.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                             c_int, c_void_p]
    lib.kpd_conv3x3_backward_prec.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                              c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    lib.kpd_bn_train_forward.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                                         c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.kpd_bn_train_backward.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.kpd_roi_targets.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                    c_void_p, c_void_p, c_void_p]
    lib.kpd_roi_features.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                     c_void_p, c_void_p]
    lib.kpd_detector_features.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.kpd_detector_targets.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_float,
                                         c_void_p, c_void_p, c_void_p, c_void_p]
    lib.kpd_detector_loss.argtypes = [c_void_p] * 9 + [c_int] * 4 + [c_float] * 4 + [c_void_p] * 6
    lib.kpd_coord_loss.argtypes = [c_void_p] * 3 + [c_int] * 3 + [c_float, c_int, c_float, c_float] + [c_void_p] * 4
    lib.kpd_softargmax_backward.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]
    lib.kpd_roi_align_backward.argtypes = [c_void_p] * 3 + [c_int] * 3 + [c_void_p] + [c_int] * 4 + [c_void_p] * 2
    lib.kpd_track_state_bytes.argtypes = [c_int]
    lib.kpd_track_poses.argtypes = [c_void_p] * 5 + [ctypes.POINTER(c_float)] + [c_int] * 4 + [c_float] * 2 + \
        [c_int] * 2 + [c_float] * 4 + [c_void_p] * 7
    for name in EXPORTS:
        if name not in ("kpd_last_error", "kpd_version", "kpd_plan_destroy"):
            getattr(lib, name).restype = c_int
    lib.kpd_track_state_bytes.restype = ctypes.c_size_t
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().kpd_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise KpdNativeError(f"{what} failed ({rc}): {msg}")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise KpdNativeError(f"{name} must be a HIP device tensor (got {t.device}); the native path "
                             f"has no CPU fallback")


class Plan:
    """Owns one ``kpd_plan`` (packed weights + workspace) on one device."""

    def __init__(self, device: torch.device, in_channels: int):
        self.lib = load()
        self.device = device
        h = ctypes.c_void_p()
        check(self.lib.kpd_plan_create(device.index or 0, in_channels, ctypes.byref(h)), "kpd_plan_create")
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.kpd_plan_destroy(h)
            self.h = None

    def set_tensor(self, name: str, t: torch.Tensor) -> None:
        t = t.detach().to("cpu", torch.float32).contiguous()
        shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
        check(self.lib.kpd_plan_set_tensor(self.h, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()),
              f"kpd_plan_set_tensor({name})")

    def finalize(self, precision: int) -> None:
        check(self.lib.kpd_plan_finalize(self.h, precision), "kpd_plan_finalize")

    def set_detector(self, conf_threshold: float, nms_iou_threshold: float) -> None:
        check(self.lib.kpd_plan_set_detector(self.h, float(conf_threshold), float(nms_iou_threshold)),
              "kpd_plan_set_detector")

    def set_streams(self, n: int) -> None:
        """Sub-batch streams for large batches (kpd_plan_set_streams)."""
        check(self.lib.kpd_plan_set_streams(self.h, int(n)), "kpd_plan_set_streams")

    def set_graphs(self, enable: bool, abandon_next_capture: bool = False) -> None:
        """Replay repeated forwards as hipGraphs (kpd_plan_set_graphs);
        abandon_next_capture (tests) makes the next capture fail over to an
        eager forward."""
        mode = (2 if abandon_next_capture else 1) if enable else 0
        check(self.lib.kpd_plan_set_graphs(self.h, mode), "kpd_plan_set_graphs")

    def forward(self, image: torch.Tensor, boxes: Optional[torch.Tensor], kpts, vis, heat, flags: int = 0,
                kh_kpts=None, kh_vis=None, box_scores=None, topk=None) -> None:
        """boxes [nb,P,4] (input; an output filled by the detector with FLAG_DETECT)."""
        _require_cuda(image, "image")
        B, C, H, W = image.shape
        nb, P = (0, 0) if boxes is None else (boxes.shape[0], boxes.shape[1])
        with torch.cuda.device(self.device):
            check(self.lib.kpd_forward(self.h, _ptr(image), B, C, H, W, _ptr(boxes), nb, P, int(flags), _ptr(kpts),
                                       _ptr(vis), _ptr(heat), _ptr(kh_kpts), _ptr(kh_vis), _ptr(box_scores),
                                       _ptr(topk), _stream(self.device)), "kpd_forward")

    def timing(self, enable: bool, stage: Optional[str] = None) -> None:
        """Record per-stage HIP events on the launch streams (only ``stage`` if given)."""
        check(self.lib.kpd_plan_timing_stage(self.h, stage.encode() if stage else None), "kpd_plan_timing_stage")
        check(self.lib.kpd_plan_timing(self.h, 1 if enable else 0), "kpd_plan_timing")

    def timing_query(self, stage: str):
        """(total_ms, launches) recorded for ``stage`` since timing(True)."""
        ms, n = ctypes.c_double(), ctypes.c_int()
        check(self.lib.kpd_plan_timing_query(self.h, stage.encode(), ctypes.byref(ms), ctypes.byref(n)),
              "kpd_plan_timing_query")
        return ms.value, n.value

    def path_log(self, enable: bool) -> None:
        """Record which kernel each dispatch point of the following eager forwards takes (kpd_plan_path_log)."""
        check(self.lib.kpd_plan_path_log(self.h, 1 if enable else 0), "kpd_plan_path_log")

    def paths(self) -> List[str]:
        """The last forward's dispatch tokens in order of first use, e.g. ``f4:exdw+seproj:po192``."""
        return _path_query(self.lib, self.h)

    # ---- stand-alone operators (the reference's submodule forwards) ----
    def heatmap_head(self, x: torch.Tensor, parts: int = HEAD_ALL):
        """HeatmapHead stages on x [R,64,56,56] -> (heat [R,17,56,56] or None,
        channel weights [R,64], spatial weights [R,56,56])."""
        x = _dev_f32(x, "x")
        R, C, H, W = x.shape
        if C != 64:
            raise ValueError(f"HeatmapHead expects 64 input channels, got {C}")
        heat = torch.empty(R, 17, H, W, device=x.device) if parts & HEAD_CONVS else None
        cw = torch.empty(R, 64, device=x.device)
        sw = torch.empty(R, H, W, device=x.device)
        with torch.cuda.device(self.device):
            check(self.lib.kpd_heatmap_head(self.h, _ptr(x), R, H, W, int(parts), _ptr(heat), _ptr(cw), _ptr(sw),
                                            _stream(self.device)), "kpd_heatmap_head")
        return heat, cw, sw

    def keypoint_head(self, x: torch.Tensor):
        x = _dev_f32(x, "x")
        R, C, H, W = x.shape
        if C != 128:
            raise ValueError(f"KEYPOINT_HEAD path expects 128 input channels, got {C}")
        kp = torch.empty(R, 17, 2, device=x.device)
        vis = torch.empty(R, 17, 3, device=x.device)
        with torch.cuda.device(self.device):
            check(self.lib.kpd_keypoint_head(self.h, _ptr(x), R, H, W, _ptr(kp), _ptr(vis), _stream(self.device)),
                  "kpd_keypoint_head")
        return kp, vis

    def backbone(self, image: torch.Tensor):
        image = _dev_f32(image, "image")
        B, C, H, W = image.shape
        sizes = _level_sizes(H, W)
        outs = [torch.empty(B, 128, *sizes[i], device=image.device) for i in (0, 3, 8, 11)]
        with torch.cuda.device(self.device):
            check(self.lib.kpd_backbone(self.h, _ptr(image), B, C, H, W, *[_ptr(o) for o in outs],
                                        _stream(self.device)), "kpd_backbone")
        return outs

    def body_taps(self, image: torch.Tensor):
        """MobileNetV3Wrapper.body(x): the four taps feat0..feat3 [B,c,h,w]
        (c = 16, 24, 48, 576 at strides 2, 8, 16, 32) -- kpd_backbone_body."""
        image = _dev_f32(image, "image")
        B, C, H, W = image.shape
        sizes = _level_sizes(H, W)
        outs = [torch.empty(B, c, *sizes[i], device=image.device) for c, i in zip((16, 24, 48, 576), (0, 3, 8, 11))]
        with torch.cuda.device(self.device):
            check(self.lib.kpd_backbone_body(self.h, _ptr(image), B, C, H, W, *[_ptr(o) for o in outs],
                                             _stream(self.device)), "kpd_backbone_body")
        return outs

    def fpn(self, feats):
        """LightweightFPN.forward on four caller taps [B,c_i,h_i,w_i] -> four
        [B,128,h_i,w_i] levels (kpd_backbone_fpn)."""
        feats = [_dev_f32(f, f"features[{i}]") for i, f in enumerate(feats)]
        if len(feats) != len(FPN_IN_CHANNELS):
            raise ValueError(f"Expected {len(FPN_IN_CHANNELS)} features, got {len(feats)}")
        B = feats[0].shape[0]
        if any(f.dim() != 4 or f.shape[0] != B for f in feats):
            raise ValueError("FPN features must be [B, C, H, W] with one batch size")
        # the reference's lateral nn.Conv2d rejects a tap of the wrong width; the
        # native conv would read the tensor with its own channel count
        for i, (f, c) in enumerate(zip(feats, FPN_IN_CHANNELS)):
            if f.shape[1] != c:
                raise RuntimeError(f"Given groups=1, weight of size [128, {c}, 1, 1], expected input"
                                   f"{list(f.shape)} to have {c} channels, but got {f.shape[1]} channels instead "
                                   f"(FPN features[{i}])")
        sizes = (ctypes.c_int * 8)(*[v for f in feats for v in f.shape[2:]])
        outs = [torch.empty(B, 128, *f.shape[2:], device=f.device) for f in feats]
        with torch.cuda.device(self.device):
            check(self.lib.kpd_backbone_fpn(self.h, *[_ptr(f) for f in feats], B, sizes, *[_ptr(o) for o in outs],
                                            _stream(self.device)), "kpd_backbone_fpn")
        return outs

    def channel_attention(self, x: torch.Tensor, k: int = 64, select: bool = False):
        """ChannelAttention scores [B,128]; top-k indices [B,k] (int64) and, with
        select, the gathered channels [B,k,H,W]."""
        x = _dev_f32(x, "x")
        B, C, H, W = x.shape
        scores = torch.empty(B, C, device=x.device)
        topk = torch.empty(B, k, device=x.device, dtype=torch.int32)
        sel = torch.empty(B, k, H, W, device=x.device) if select else None
        with torch.cuda.device(self.device):
            check(self.lib.kpd_channel_attention(self.h, _ptr(x), B, C, H, W, _ptr(scores), _ptr(topk), int(k),
                                                 _ptr(sel), _stream(self.device)), "kpd_channel_attention")
        return scores, topk.long(), sel

    def roi_features(self, image: torch.Tensor, boxes: torch.Tensor, rows=None) -> torch.Tensor:
        """The trunk's ROI features as the fused forward serves them to
        HeatmapHead (kpd_roi_features): image [B,C,H,W], boxes [B,P,4] cxcywh
        -> [n,64,56,56], the rows ``rows`` (ascending indices into B*P: an
        int32 device tensor, read in place, or a sequence; None = all) of the
        forward's own ROI buffer, bit for bit.  No head runs and no host
        synchronisation happens; indices outside [0, B*P) are the caller's
        contract (their output rows stay unwritten)."""
        image = _dev_f32(image, "image")
        boxes = _dev_f32(boxes, "boxes")
        if image.dim() != 4:
            raise ValueError(f"image must be [B, C, H, W], got {tuple(image.shape)}")
        B, C, H, W = image.shape
        if boxes.dim() != 3 or boxes.size(0) != B or boxes.size(2) != 4:
            raise ValueError(f"boxes must be [{B}, P, 4], got {tuple(boxes.shape)}")
        P = boxes.size(1)
        rows = _row_list(rows, image.device)
        n = B * P if rows is None else rows.numel()
        out = torch.empty(n, 64, 56, 56, device=image.device)
        if n == 0:   # (an empty tensor has no pointer to tell an empty row list from none)
            return out
        with torch.cuda.device(self.device):
            check(self.lib.kpd_roi_features(self.h, _ptr(image), B, C, H, W, _ptr(boxes), P, _ptr(rows), n, _ptr(out),
                                            _stream(self.device)), "kpd_roi_features")
        return out

    def detector_features(self, image: torch.Tensor) -> torch.Tensor:
        """The person detector's input (kpd_detector_features): image [B,C,H,W]
        -> [B,3136,128], FPN level 0 adaptive-average-pooled to the 56 x 56
        anchor grid (cell i * 56 + j, channel), as the eval detector pools it.
        No head runs and no host synchronisation happens."""
        image = _dev_f32(image, "image")
        if image.dim() != 4:
            raise ValueError(f"image must be [B, C, H, W], got {tuple(image.shape)}")
        B, C, H, W = image.shape
        out = torch.empty(B, 3136, 128, device=image.device)
        if B == 0:
            return out
        with torch.cuda.device(self.device):
            check(self.lib.kpd_detector_features(self.h, _ptr(image), B, C, H, W, _ptr(out), _stream(self.device)),
                  "kpd_detector_features")
        return out

    def debug_buffer(self, name: str) -> torch.Tensor:
        n = ctypes.c_size_t()
        check(self.lib.kpd_debug_copy(self.h, name.encode(), None, 0, ctypes.byref(n), None), "kpd_debug_copy")
        out = torch.empty(n.value // 4, dtype=torch.float32, device=self.device)
        check(self.lib.kpd_debug_copy(self.h, name.encode(), _ptr(out), n.value, None, _stream(self.device)),
              "kpd_debug_copy")
        return out


def _path_query(lib, handle) -> List[str]:
    n = ctypes.c_size_t()
    check(lib.kpd_plan_path_query(handle, None, 0, ctypes.byref(n)), "kpd_plan_path_query")
    buf = ctypes.create_string_buffer(n.value)
    check(lib.kpd_plan_path_query(handle, buf, n.value, None), "kpd_plan_path_query")
    return [t for t in buf.value.decode().split("\n") if t]


def all_paths() -> List[str]:
    """Every dispatch token the loaded library can emit ("*" = an index or a run-time value)."""
    return _path_query(load(), None)


def _level_sizes(H: int, W: int):
    """(h, w) of the stem output and of features.1..11 (torchvision conv arithmetic)."""
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    sizes = [(h, w)]
    for k, s_ in ((3, 2), (3, 2), (3, 1), (5, 2), (5, 1), (5, 1), (5, 1), (5, 1), (5, 2), (5, 1), (5, 1)):
        pd = (k - 1) // 2
        h, w = (h + 2 * pd - k) // s_ + 1, (w + 2 * pd - k) // s_ + 1
        sizes.append((h, w))
    return sizes


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    _require_cuda(t, name)
    return t.float().contiguous()


def _row_list(rows, device: torch.device) -> Optional[torch.Tensor]:
    """A row selection as a contiguous 1-D int32 tensor on ``device`` (None stays None)."""
    if rows is None:
        return None
    if not isinstance(rows, torch.Tensor):
        rows = torch.tensor([int(r) for r in rows], dtype=torch.int32)
    if rows.dim() != 1 or rows.is_floating_point():
        raise ValueError("rows must be a 1-D integer tensor or a sequence of ints")
    return rows.to(device, torch.int32).contiguous()


def roi_targets(keypoints: torch.Tensor, visibilities: torch.Tensor, boxes: torch.Tensor, rows, H: int, W: int,
                sigma: float):
    """kpd_roi_targets on keypoints [R,K,2], visibilities [R,K], boxes [R,4]
    (fp32 device tensors): (heat [n,K,H,W], weight [n,K]) for the ROIs ``rows``
    (None = all R, in order).  No host synchronisation."""
    keypoints = _dev_f32(keypoints, "keypoints")
    visibilities = _dev_f32(visibilities, "visibilities").to(keypoints.device)
    boxes = _dev_f32(boxes, "boxes").to(keypoints.device)
    if keypoints.dim() != 3 or keypoints.size(2) != 2:
        raise ValueError(f"keypoints must be [R, K, 2], got {tuple(keypoints.shape)}")
    R, K = keypoints.shape[:2]
    if tuple(visibilities.shape) != (R, K) or tuple(boxes.shape) != (R, 4):
        raise ValueError(f"visibilities must be [{R}, {K}] and boxes [{R}, 4], got {tuple(visibilities.shape)} "
                         f"and {tuple(boxes.shape)}")
    rows = _row_list(rows, keypoints.device)
    n = R if rows is None else rows.numel()
    heat = torch.empty(n, K, int(H), int(W), device=keypoints.device)
    weight = torch.empty(n, K, device=keypoints.device)
    with torch.cuda.device(keypoints.device):
        check(load().kpd_roi_targets(_ptr(keypoints), _ptr(visibilities), _ptr(boxes), _ptr(rows), n, R, K, int(H),
                                     int(W), float(sigma), _ptr(heat), _ptr(weight), _stream(keypoints.device)),
              "kpd_roi_targets")
    return heat, weight


def _det_inputs(anchors: torch.Tensor, gt_boxes: Optional[torch.Tensor], B: int, image_size):
    """(anchors [28224,4], gt [B,G,4] or None, G, H, W) for the detector-training entries."""
    anchors = _dev_f32(anchors, "anchors")
    if tuple(anchors.shape) != (DET_ANCHORS, 4):
        raise ValueError(f"anchors must be [{DET_ANCHORS}, 4], got {tuple(anchors.shape)}")
    H, W = (int(v) for v in image_size)
    if gt_boxes is None:
        return anchors, None, 0, H, W
    gt = _dev_f32(gt_boxes, "gt_boxes").to(anchors.device)
    if gt.dim() != 3 or gt.size(0) != B or gt.size(2) != 4:
        raise ValueError(f"gt_boxes must be [{B}, G, 4], got {tuple(gt.shape)}")
    G = gt.size(1)
    if G > DET_MAX_GT:
        raise ValueError(f"gt_boxes holds {G} slots per image; the matching takes at most {DET_MAX_GT}")
    return anchors, (gt if G > 0 else None), G, H, W


def detector_targets(anchors: torch.Tensor, gt_boxes: Optional[torch.Tensor], batch: int, image_size,
                     pos_thr: float = 0.5, neg_thr: float = 0.4, tie_eps: float = 1e-5, want_best: bool = False):
    """kpd_detector_targets: anchors [28224,4] (the PERSON_HEAD buffer), gt_boxes
    [B,G,4] cxcywh normalised (None or G = 0: no labels), image_size (H, W) ->
    (assign [B,28224] int32: GT slot, -1 negative, -2 ignored; n_pos [B] int32;
    gt_best [B,G] or None).  No host synchronisation."""
    anchors, gt, G, H, W = _det_inputs(anchors, gt_boxes, int(batch), image_size)
    B = int(batch)
    dev = anchors.device
    assign = torch.empty(B, DET_ANCHORS, dtype=torch.int32, device=dev)
    n_pos = torch.empty(B, dtype=torch.int32, device=dev)
    best = torch.empty(B, G, device=dev) if want_best else None
    with torch.cuda.device(dev):
        check(load().kpd_detector_targets(_ptr(anchors), _ptr(gt), B, G, H, W, float(pos_thr), float(neg_thr),
                                          float(tie_eps), _ptr(assign), _ptr(n_pos),
                                          _ptr(best) if G > 0 else None, _stream(dev)), "kpd_detector_targets")
    return assign, n_pos, best


def detector_loss(pooled: torch.Tensor, box_weight: torch.Tensor, box_bias: torch.Tensor, cls_weight: torch.Tensor,
                  cls_bias: torch.Tensor, anchors: torch.Tensor, gt_boxes: Optional[torch.Tensor],
                  assign: torch.Tensor, n_pos: torch.Tensor, image_size, alpha: float = 0.25, gamma: float = 2.0,
                  beta: float = 1.0 / 9, box_weight_factor: float = 1.0, want_grad: bool = True):
    """kpd_detector_loss: pooled [B,3136,128], the four parameters of
    box_heads[0] / cls_heads[0] (nn.Conv2d shapes or flat), assign / n_pos from
    detector_targets -> (loss [3] = total, class part, box part; (g_box_w
    [36,128], g_box_b [36], g_cls_w [9,128], g_cls_b [9]) or None without
    want_grad).  No host synchronisation."""
    pooled = _dev_f32(pooled, "pooled")
    if pooled.dim() != 3 or tuple(pooled.shape[1:]) != (3136, 128):
        raise ValueError(f"pooled must be [B, 3136, 128], got {tuple(pooled.shape)}")
    B, dev = pooled.size(0), pooled.device
    anchors, gt, G, H, W = _det_inputs(anchors.to(dev), gt_boxes, B, image_size)
    prm = []
    for t, n, name in ((box_weight, 36 * 128, "box_weight"), (box_bias, 36, "box_bias"),
                       (cls_weight, 9 * 128, "cls_weight"), (cls_bias, 9, "cls_bias")):
        t = _dev_f32(t.detach(), name).to(dev)
        if t.numel() != n:
            raise ValueError(f"{name} must hold {n} values, got {tuple(t.shape)}")
        prm.append(t)
    for t, shape, name in ((assign, (B, DET_ANCHORS), "assign"), (n_pos, (B,), "n_pos")):
        _require_cuda(t, name)
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous int32 tensor {list(shape)} on {dev}")
    loss = torch.empty(3, device=dev)
    grads = None
    if want_grad:
        grads = (torch.empty(36, 128, device=dev), torch.empty(36, device=dev), torch.empty(9, 128, device=dev),
                 torch.empty(9, device=dev))
    gp = [_ptr(g) for g in grads] if want_grad else [None] * 4
    with torch.cuda.device(dev):
        check(load().kpd_detector_loss(_ptr(pooled), *[_ptr(t) for t in prm], _ptr(anchors), _ptr(gt), _ptr(assign),
                                       _ptr(n_pos), B, G, H, W, float(alpha), float(gamma), float(beta),
                                       float(box_weight_factor), _ptr(loss), *gp, _stream(dev)), "kpd_detector_loss")
    return loss, grads


def decode_heatmaps(heat: torch.Tensor, mode: int, param: float = 0.0):
    """Heatmap decoders on the device: heat [B,K,H,W] -> keypoints [B,K,2],
    scores [B,K], vis [B,K,3] (mode DECODE_MODEL; else None)."""
    heat = _dev_f32(heat, "heatmaps")
    if heat.dim() != 4:
        raise ValueError(f"expected [B,K,H,W] heatmaps, got {tuple(heat.shape)}")
    B, K, H, W = heat.shape
    kp = torch.empty(B, K, 2, device=heat.device)
    sc = torch.empty(B, K, device=heat.device)
    vis = torch.empty(B, K, 3, device=heat.device) if mode == DECODE_MODEL else None
    lib = load()
    with torch.cuda.device(heat.device):
        check(lib.kpd_decode_heatmaps(_ptr(heat), B * K, H, W, int(mode), float(param), _ptr(kp), _ptr(sc), _ptr(vis),
                                      _stream(heat.device)), "kpd_decode_heatmaps")
    return kp, sc, vis


def flip_merge(heat_a: torch.Tensor, heat_b: torch.Tensor, boxes: torch.Tensor, pairs, heat_out, keypoints,
               visibilities, peaks) -> None:
    """``kpd_flip_merge`` (include/kpd.h) on contiguous fp32 device tensors:
    heat_a, heat_b [n,P,K,H,W], boxes [n,P,4], ``pairs`` K ints (host);
    writes keypoints (n*P*K*2 values), visibilities (n*P*K*3) and the nullable
    heat_out [n,P,K,H,W] (may be heat_a itself) and peaks (n*P*K).  The call
    does not synchronise."""
    named = (("heat_a", heat_a), ("heat_b", heat_b), ("boxes", boxes), ("heat_out", heat_out),
             ("keypoints", keypoints), ("visibilities", visibilities), ("keypoint_peaks", peaks))
    if not isinstance(heat_a, torch.Tensor):
        raise TypeError("heat_a must be a tensor")
    if heat_a.dim() != 5:
        raise ValueError(f"heat_a must be [n, P, K, H, W], got {list(heat_a.shape)}")
    n, P, K, H, W = heat_a.shape
    numel = {"heat_a": n * P * K * H * W, "heat_b": n * P * K * H * W, "boxes": n * P * 4,
             "heat_out": n * P * K * H * W, "keypoints": n * P * K * 2, "visibilities": n * P * K * 3,
             "keypoint_peaks": n * P * K}
    for name, t in named:
        if t is None and name in ("heat_out", "keypoint_peaks"):
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        _require_cuda(t, name)
        if t.device != heat_a.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor on {heat_a.device}")
        if t.numel() != numel[name]:
            raise ValueError(f"{name} has {t.numel()} values, heat_a {list(heat_a.shape)} needs {numel[name]}")
    if tuple(heat_b.shape) != tuple(heat_a.shape):
        raise ValueError(f"heat_b {list(heat_b.shape)} does not match heat_a {list(heat_a.shape)}")
    pr = [int(v) for v in pairs]
    if len(pr) != K:
        raise ValueError(f"{len(pr)} flip pairs for {K} keypoints")
    with torch.cuda.device(heat_a.device):
        rc = load().kpd_flip_merge(_ptr(heat_a), _ptr(heat_b), _ptr(boxes), (ctypes.c_int32 * max(K, 1))(*pr),
                                   n, P, K, H, W, _ptr(heat_out), _ptr(keypoints), _ptr(visibilities), _ptr(peaks),
                                   _stream(heat_a.device))
    check(rc, "kpd_flip_merge")


def roi_align(features: torch.Tensor, rois: torch.Tensor, output_size, spatial_scale: float = 1.0,
              sampling_ratio: int = -1, aligned: bool = False) -> torch.Tensor:
    """torchvision.ops.roi_align with a [R,5] (batch index, x1, y1, x2, y2) box tensor."""
    features = _dev_f32(features, "features")
    rois = rois.to(features.device, torch.float32).contiguous()
    if rois.dim() != 2 or rois.size(1) != 5:
        raise ValueError("rois must be [R, 5]")
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    B, C, H, W = features.shape
    out = torch.empty(rois.size(0), C, oh, ow, device=features.device)
    lib = load()
    with torch.cuda.device(features.device):
        check(lib.kpd_roi_align(_ptr(features), B, C, H, W, _ptr(rois), rois.size(0), oh, ow, float(spatial_scale),
                                int(sampling_ratio), int(bool(aligned)), _ptr(out), _stream(features.device)),
              "kpd_roi_align")
    return out


def conv1x1(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """nn.Conv2d(k=1) forward on NCHW device tensors."""
    x = _dev_f32(x, "x")
    B, C, H, W = x.shape
    w = weight.detach().to(x.device, torch.float32).reshape(weight.shape[0], -1).contiguous()
    if w.shape[1] != C:
        raise ValueError(f"weight expects {w.shape[1]} input channels, got {C}")
    b = None if bias is None else bias.detach().to(x.device, torch.float32).contiguous()
    out = torch.empty(B, w.shape[0], H, W, device=x.device)
    lib = load()
    with torch.cuda.device(x.device):
        check(lib.kpd_conv1x1(_ptr(x), B, C, H * W, _ptr(w), _ptr(b), w.shape[0], _ptr(out), _stream(x.device)),
              "kpd_conv1x1")
    return out


# dll.ops.conv3x3's precisions (kpd_conv3x3_*_prec): the fp32-accurate split products, or bf16-rounded operands
CONV3_PRECISIONS = {"split": KPD_PRECISION_SPLIT, "mixed": KPD_PRECISION_MIXED}


def conv3_precision(precision: str) -> int:
    try:
        return CONV3_PRECISIONS[precision]
    except (KeyError, TypeError):
        raise ValueError(f"conv3x3 precision must be one of {sorted(CONV3_PRECISIONS)}, got {precision!r}") from None


def conv3x3_forward(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                    precision: str = "split") -> torch.Tensor:
    """nn.Conv2d(k=3, padding=1) forward on NCHW device tensors (kpd_conv3x3_forward_prec)."""
    prec = conv3_precision(precision)
    x = _dev_f32(x, "x")
    N, C, H, W = x.shape
    w = weight.detach().to(x.device, torch.float32).contiguous()
    if w.dim() != 4 or w.shape[1] != C or w.shape[2:] != (3, 3):
        raise ValueError(f"weight must be [O][{C}][3][3], got {tuple(w.shape)}")
    b = None if bias is None else bias.detach().to(x.device, torch.float32).contiguous()
    y = torch.empty(N, w.shape[0], H, W, device=x.device)
    lib = load()
    with torch.cuda.device(x.device):
        check(lib.kpd_conv3x3_forward_prec(_ptr(x), _ptr(w), _ptr(b), N, C, H, W, w.shape[0], _ptr(y), prec,
                                           _stream(x.device)), "kpd_conv3x3_forward_prec")
    return y


def conv3x3_backward(x: torch.Tensor, weight: torch.Tensor, grad_y: torch.Tensor, need_x: bool = True,
                     need_w: bool = True, need_b: bool = True, precision: str = "split"):
    """Gradients of nn.Conv2d(k=3, padding=1) (kpd_conv3x3_backward_prec): (gx, gw, gb),
    None where not requested."""
    prec = conv3_precision(precision)
    x = _dev_f32(x, "x")
    N, C, H, W = x.shape
    w = weight.detach().to(x.device, torch.float32).contiguous()
    if w.dim() != 4 or w.shape[1] != C or w.shape[2:] != (3, 3):
        raise ValueError(f"weight must be [O][{C}][3][3], got {tuple(w.shape)}")
    O = w.shape[0]
    gy =_dev_f32(grad_y, "grad_y")
    if tuple(gy.shape) != (N, O, H, W):
        raise ValueError(f"grad_y must be [{N}][{O}][{H}][{W}], got {tuple(gy.shape)}")
    gx = torch.empty_like(x) if need_x else None
    gw = torch.empty_like(w) if need_w else None
    gb = torch.empty(O, device=x.device) if need_b else None
    lib = load()
    with torch.cuda.device(x.device):
        check(lib.kpd_conv3x3_backward_prec(_ptr(x), _ptr(w), _ptr(gy), N, C, H, W, O, _ptr(gx), _ptr(gw), _ptr(gb),
                                            prec, _stream(x.device)), "kpd_conv3x3_backward_prec")
    return gx, gw, gb


def _bn_vec(t: Optional[torch.Tensor], n: int, name: str, device: torch.device) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.detach().to(device, torch.float32).contiguous()
    if t.numel() != n:
        raise ValueError(f"{name} must hold {n} values, got {tuple(t.shape)}")
    return t


def bn_train_forward(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                     drop: Optional[torch.Tensor], eps: float, momentum: float,
                     running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], relu: bool = True):
    """Batch-statistics BatchNorm2d + ReLU + per-(image, channel) multiplier on
    NCHW device tensors (kpd_bn_train_forward): (y, save_mean, save_invstd).
    running_mean / running_var ([C] fp32, contiguous, on x's device) are
    updated in place through their pointers; the caller bumps their versions."""
    x = _dev_f32(x, "x")
    if x.dim() != 4:
        raise ValueError(f"x must be [N, C, H, W], got {tuple(x.shape)}")
    N, C, H, W = x.shape
    g, b = _bn_vec(gamma, C, "weight", x.device), _bn_vec(beta, C, "bias", x.device)
    d = _bn_vec(drop, N * C, "drop", x.device)
    for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None and (t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous()
                              or t.numel() != C):
            raise ValueError(f"{name} must be a contiguous float32 tensor of {C} values on {x.device}")
    y = torch.empty_like(x)
    mean = torch.empty(C, device=x.device)
    invstd = torch.empty(C, device=x.device)
    with torch.cuda.device(x.device):
        check(load().kpd_bn_train_forward(_ptr(x), N, C, H, W, _ptr(g), _ptr(b), _ptr(d), float(eps), float(momentum),
                                          _ptr(running_mean), _ptr(running_var), BN_RELU if relu else 0, _ptr(y),
                                          _ptr(mean), _ptr(invstd), _stream(x.device)), "kpd_bn_train_forward")
    return y, mean, invstd


def bn_train_backward(x: torch.Tensor, grad_y: torch.Tensor, gamma: Optional[torch.Tensor],
                      beta: Optional[torch.Tensor], drop: Optional[torch.Tensor], save_mean: torch.Tensor,
                      save_invstd: torch.Tensor, relu: bool = True, need_x: bool = True, need_gamma: bool = True,
                      need_beta: bool = True):
    """Gradients of bn_train_forward (kpd_bn_train_backward): (gx, ggamma,
    gbeta), None where not requested."""
    x = _dev_f32(x, "x")
    N, C, H, W = x.shape
    gy = _dev_f32(grad_y, "grad_y")
    if tuple(gy.shape) != (N, C, H, W):
        raise ValueError(f"grad_y must be [{N}][{C}][{H}][{W}], got {tuple(gy.shape)}")
    g, b = _bn_vec(gamma, C, "weight", x.device), _bn_vec(beta, C, "bias", x.device)
    d = _bn_vec(drop, N * C, "drop", x.device)
    mean, invstd = _bn_vec(save_mean, C, "save_mean", x.device), _bn_vec(save_invstd, C, "save_invstd", x.device)
    gx = torch.empty_like(x) if need_x else None
    gg = torch.empty(C, device=x.device) if need_gamma else None
    gb = torch.empty(C, device=x.device) if need_beta else None
    with torch.cuda.device(x.device):
        check(load().kpd_bn_train_backward(_ptr(x), _ptr(gy), N, C, H, W, _ptr(g), _ptr(b), _ptr(d), _ptr(mean),
                                           _ptr(invstd), BN_RELU if relu else 0, _ptr(gx), _ptr(gg), _ptr(gb),
                                           _stream(x.device)), "kpd_bn_train_backward")
    return gx, gg, gb


class PlanCache:
    """A submodule's own plan (its weights registered under the model's
    state-dict prefix), rebuilt when a parameter changes -- what the model
    does for its whole-forward plan (keypoint_model.py)."""

    def __init__(self, prefix: str, in_channels: int = 3):
        self.prefix, self.in_channels = prefix, in_channels
        self.plan, self.key = None, None

    def get(self, module: torch.nn.Module, device: torch.device, precision: str) -> "Plan":
        sd = module.state_dict(keep_vars=True)
        key = (device, precision, tuple((t.data_ptr(), t._version) for t in sd.values()))
        if self.plan is None or self.key != key:
            plan = Plan(device, self.in_channels)
            for name, t in sd.items():
                if t.is_floating_point():
                    plan.set_tensor(self.prefix + name, t)
            plan.finalize(PRECISIONS[precision])
            self.plan, self.key = plan, key
        return self.plan


def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float, max_output: int = 0) -> torch.Tensor:
    """Device NMS with PERSON_HEAD.non_max_suppression semantics; returns int64 keep indices."""
    lib = load()
    _require_cuda(boxes, "boxes")
    boxes = boxes.float().contiguous()
    scores = scores.float().contiguous()
    n = boxes.shape[0]
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=boxes.device)
    nk = torch.zeros(1, dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        check(lib.kpd_nms(_ptr(boxes), _ptr(scores), n, float(iou_threshold), int(max_output or 0), _ptr(keep),
                          _ptr(nk), _stream(boxes.device)), "kpd_nms")
    return keep[: int(nk.item())].long()


def adaptive_heatmap_loss(pred: torch.Tensor, gt: torch.Tensor, target_weight: Optional[torch.Tensor],
                          keypoint_weight: float, background_weight: float, adaptive: bool, focal_alpha: float,
                          want_grad: bool):
    """kpd_adaptive_heatmap_loss on [B,K,H,W] fp32 device tensors -> (loss 0-d tensor, grad or None,
    threshold 0-d tensor)."""
    for t, n in ((pred, "pred"), (gt, "gt")):
        _require_cuda(t, n)
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError("AdaptiveHeatmapLoss: pred and gt must be [B, K, H, W] of the same shape")
    B, K, H, W = pred.shape
    p = pred.detach().float().contiguous()
    g = gt.detach().float().contiguous()
    tw = None
    if target_weight is not None:
        _require_cuda(target_weight, "target_weight")
        tw = target_weight.detach().float().reshape(B, K).contiguous()
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    thr = torch.empty((), dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(p) if want_grad else None
    with torch.cuda.device(pred.device):
        check(load().kpd_adaptive_heatmap_loss(_ptr(p), _ptr(g), _ptr(tw), B, K, H, W, float(keypoint_weight),
                                               float(background_weight), int(bool(adaptive)), float(focal_alpha),
                                               _ptr(loss), _ptr(grad), _ptr(thr), _stream(pred.device)),
              "kpd_adaptive_heatmap_loss")
    return loss, grad, thr


def _coord_heat(heat: torch.Tensor, temperature: float):
    """heat [n,K,H,W] as a contiguous fp32 device tensor; the checks shared by the two entries below
    (made here so that they also hold for an empty tensor, which launches nothing)."""
    heat = _dev_f32(heat.detach(), "heatmaps")
    if heat.dim() != 4:
        raise ValueError(f"expected [n, K, H, W] heatmaps, got {tuple(heat.shape)}")
    if heat.size(2) < 2 or heat.size(3) < 2:
        raise ValueError(f"the soft-argmax needs H, W >= 2, got {tuple(heat.shape[2:])}")
    t = float(temperature)
    if not (t > 0.0 and t < float("inf")):
        raise ValueError(f"temperature must be positive and finite, got {temperature}")
    return heat, t


def coord_loss(heat: torch.Tensor, gt_coords: torch.Tensor, visibility: torch.Tensor, temperature: float,
               loss_type: str, pixel_weight_scale: float, distance_threshold: float, want_grad: bool):
    """kpd_coord_loss on heat [n,K,H,W], gt_coords [n,K,2], visibility [n,K]
    (device tensors) -> (loss 0-d, coords [n,K,2], grad [n,K,H,W] or None).
    No host synchronisation."""
    heat, t = _coord_heat(heat, temperature)
    if loss_type not in COORD_LOSS_TYPES:
        raise ValueError(f"Unsupported loss type: {loss_type}")
    n, K, H, W = heat.shape
    dev = heat.device
    gt = _dev_f32(gt_coords.detach(), "gt_coords").to(dev)
    vis = _dev_f32(visibility.detach(), "visibility").to(dev)
    if tuple(gt.shape) != (n, K, 2) or tuple(vis.shape) != (n, K):
        raise ValueError(f"gt_coords must be [{n}, {K}, 2] and visibility [{n}, {K}], got {tuple(gt.shape)} and "
                         f"{tuple(vis.shape)}")
    coords = torch.empty(n, K, 2, device=dev)
    loss = torch.empty((), device=dev)
    grad = torch.empty_like(heat) if want_grad else None
    with torch.cuda.device(dev):
        check(load().kpd_coord_loss(_ptr(heat), _ptr(gt), _ptr(vis), n * K, H, W, t, COORD_LOSS_TYPES[loss_type],
                                    float(pixel_weight_scale), float(distance_threshold), _ptr(coords), _ptr(loss),
                                    _ptr(grad), _stream(dev)), "kpd_coord_loss")
    return loss, coords, grad


def softargmax_backward(heat: torch.Tensor, grad_coords: torch.Tensor, temperature: float) -> torch.Tensor:
    """kpd_softargmax_backward: heat [n,K,H,W], grad_coords [n,K,2] -> d / d heat [n,K,H,W]."""
    heat, t = _coord_heat(heat, temperature)
    n, K, H, W = heat.shape
    g = _dev_f32(grad_coords.detach(), "grad_coords").to(heat.device)
    if tuple(g.shape) != (n, K, 2):
        raise ValueError(f"grad_coords must be [{n}, {K}, 2], got {tuple(g.shape)}")
    out = torch.empty_like(heat)
    with torch.cuda.device(heat.device):
        check(load().kpd_softargmax_backward(_ptr(heat), _ptr(g), n * K, H, W, t, _ptr(out), _stream(heat.device)),
              "kpd_softargmax_backward")
    return out


def roi_align_backward(grad_out: torch.Tensor, boxes: torch.Tensor, rows, topk: Optional[torch.Tensor],
                       channels: int, height: int, width: int) -> torch.Tensor:
    """kpd_roi_align_backward: grad_out [n,Cs,56,56] = dL / d(ROI features) of the
    rows ``rows`` (ascending indices into B*P; None = all) of boxes [B,P,4]
    (cxcywh, normalised), topk [B,Cs] (the level-0 channels the features were
    gathered from; None: Cs == channels, in order) -> dL / d(level 0)
    [B,channels,height,width], written completely by the call (zeros where
    nothing lands).  Deterministic; no host synchronisation."""
    g = _dev_f32(grad_out.detach(), "grad_out")
    dev = g.device
    boxes = _dev_f32(boxes.detach(), "boxes").to(dev)
    if boxes.dim() != 3 or boxes.size(2) != 4:
        raise ValueError(f"boxes must be [B, P, 4], got {tuple(boxes.shape)}")
    B, P = boxes.shape[:2]
    rows = _row_list(rows, dev)
    n = B * P if rows is None else rows.numel()
    if rows is None:
        rows = torch.arange(n, dtype=torch.int32, device=dev)
    if g.dim() != 4 or g.size(0) != n or tuple(g.shape[2:]) != (56, 56):
        raise ValueError(f"grad_out must be [{n}, Cs, 56, 56], got {tuple(g.shape)}")
    Cs, C, H, W = g.size(1), int(channels), int(height), int(width)
    if topk is not None:
        _require_cuda(topk, "topk")
        if topk.is_floating_point() or tuple(topk.shape) != (B, Cs):
            raise ValueError(f"topk must be an integer tensor [{B}, {Cs}], got {tuple(topk.shape)}")
        topk = topk.to(dev, torch.int32).contiguous()
    out = torch.empty(B, C, H, W, device=dev)
    with torch.cuda.device(dev):
        check(load().kpd_roi_align_backward(_ptr(g) if n else None, _ptr(boxes) if n else None,
                                            _ptr(rows) if n else None, n, B, P, _ptr(topk), Cs, C, H, W,
                                            _ptr(out) if out.numel() else None, _stream(dev)),
              "kpd_roi_align_backward")
    return out
