/* kpd.h -- C ABI of the MI355X-native keypoint-detection hot path (libkpd.so).
 *
 * Drop-in boundary for the reference's `MultiPersonKeypointModel.forward`
 * (eval, caller-given person boxes).  Plain pointers and sizes only; device
 * pointers are HIP device memory on the plan's device, streams are
 * hipStream_t passed as void*.  The library owns the plan (packed weights,
 * workspace); the caller owns every input/output buffer.
 *
 * Reference interfaces replaced (paths under the reference repo):
 *   kpd_plan_create/set_tensor/finalize
 *       <- MultiPersonKeypointModel.__init__ + load_state_dict
 *          dll/models/keypoint_model.py:49-71, scripts/predict.py:30-62
 *          (tensor names are the reference's state-dict keys; BN folding and
 *           NHWC/MFMA repacking happen inside finalize)
 *   kpd_forward
 *       <- MultiPersonKeypointModel.forward(batch) with batch['bboxes']
 *          dll/models/keypoint_model.py:73-210 (eval / no_grad branch):
 *          backbone.py:258-264, keypoint_model.py:653-661, :212-228,
 *          heatmap_head.py:81-113, keypoint_model.py:250-313, :230-248
 *   kpd_nms
 *       <- PERSON_HEAD.non_max_suppression  dll/models/person_head.py:96-139
 *
 * Every function returns 0 on success or a negative KPD_E* code; the message
 * of the last failure on the calling thread is available from kpd_last_error().
 */
#ifndef KPD_H_
#define KPD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KPD_OK 0
#define KPD_EINVAL (-1)     /* bad argument / shape (reference raises ValueError) */
#define KPD_EHIP (-2)       /* HIP runtime error */
#define KPD_ESTATE (-3)     /* plan not finalized / missing weights */

#define KPD_PRECISION_FP32 0   /* every conv on fp32-input MFMA (exact fp32 products) */
#define KPD_PRECISION_MIXED 1  /* heatmap-head convs on bf16 MFMA, fp32 accumulate; backbone fp32 */
#define KPD_PRECISION_SPLIT 2  /* fp32-accurate: FPN level 0 and the heatmap-head convs as three
                                  f16 MFMA products of hi/lo operand splits, fp32 accumulate */

typedef struct kpd_plan kpd_plan;

const char* kpd_last_error(void);
const char* kpd_version(void);

/* Create an empty plan bound to HIP device `device`.  in_channels: 1 or 3
 * (BackboneConfig.in_channels, reference backbone.py:251-252). */
int kpd_plan_create(int device, int in_channels, kpd_plan** out);

/* Register one reference state-dict tensor (fp32, host memory, contiguous,
 * shape as in the reference).  Unknown names are ignored (the reference's
 * predict.py filters unknown keys the same way, predict.py:47-57). */
int kpd_plan_set_tensor(kpd_plan* plan, const char* name, const float* host_data,
                        const int64_t* shape, int ndim);

/* Fold BN, repack weights (NHWC / MFMA layouts) and upload them.
 * Fails with KPD_ESTATE listing any missing tensor. */
int kpd_plan_finalize(kpd_plan* plan, int precision);

void kpd_plan_destroy(kpd_plan* plan);

/* HeatmapHead stages (kpd_heatmap_head) */
#define KPD_HEAD_CHANNEL_ATT 1
#define KPD_HEAD_SPATIAL_ATT 2
#define KPD_HEAD_CONVS 4
#define KPD_HEAD_ALL 7

#define KPD_FLAG_DETECT 1     /* no caller boxes: person detector + NMS WRITE boxes [B][P][4] */
#define KPD_FLAG_DUAL_HEAD 2  /* also run KEYPOINT_HEAD on 128-ch ROI features */
/* Write every pixel of FPN level 0.  By default, with caller boxes, the
 * level-0 conv stores only the pixels the ROI aligns of the image's boxes
 * read (the channel statistics of the top-k still see every pixel), and
 * kpd_debug_copy has no "feat0"; this flag stores the whole map (inspection,
 * tests).  Outputs are identical either way. */
#define KPD_FLAG_FULL_LEVEL0 4

/* Full eval forward.
 *   image:  [B][C][H][W] fp32 (NCHW, as the reference receives it), device
 *   boxes:  [nbox_images][P][4] fp32 cxcywh normalised to [0,1], device;
 *           nbox_images <= B (the reference iterates over the box list).
 *           With KPD_FLAG_DETECT it is an OUTPUT (nbox_images == B, P = max
 *           persons kept per image, zero padded) -- build-defined glue for
 *           the reference's person-detector branch.
 *   keypoints:    [nbox_images][P][1][17][2]  fp32 out
 *   visibilities: [nbox_images][P][1][17][3]  fp32 out (one-hot 3-class)
 *   heatmap:      [nbox_images][P][17][56][56] fp32 out, may be NULL
 *   kh_keypoints / kh_visibilities: [nbox_images][P][1][17][2|3] sigmoid
 *                 outputs of KEYPOINT_HEAD (KPD_FLAG_DUAL_HEAD), else NULL
 *   box_scores:   [B][P] detector scores (KPD_FLAG_DETECT), may be NULL
 *   topk_out:     [B][64] int32 channel indices, may be NULL (debug)
 * All-zero boxes are skipped and the remaining persons compacted, images
 * without a valid box get the reference's dummy person, P is kept as the
 * padded person count -- exactly keypoint_model.py:138-206. */
int kpd_forward(kpd_plan* plan, const float* image, int B, int C, int H, int W,
                float* boxes, int nbox_images, int P, int flags,
                float* keypoints, float* visibilities, float* heatmap,
                float* kh_keypoints, float* kh_visibilities, float* box_scores,
                int32_t* topk_out, void* stream);

/* Detector thresholds (PersonDetectionConfig.conf_threshold /
 * nms_iou_threshold, model_config.py:27-28); defaults 0.3 / 0.3. */
int kpd_plan_set_detector(kpd_plan* plan, float conf_threshold, float nms_iou_threshold);

/* Copy an internal buffer recorded by the last kpd_forward into `dst`
 * (device memory, `bytes` long).  Names: "feat0" ([B][Hf][Wf][128] NHWC f32),
 * "scores" ([B][128] f32), "roi" ([R][56][56][64] f32), "tap0".."tap3";
 * with KPD_FLAG_DETECT the NMS's inputs "pd_boxes" ([B][28224][4] cxcywh f32)
 * and "pd_scores" ([B][28224] f32, -inf where score <= conf_threshold).
 * Writes the buffer size to *size_out when dst == NULL. */
int kpd_debug_copy(kpd_plan* plan, const char* name, void* dst, size_t bytes, size_t* size_out,
                   void* stream);

/* Per-stage device timing with HIP events recorded on the launch stream.
 * kpd_plan_timing(plan, 1) clears previous records and enables recording for
 * subsequent kpd_forward calls; kpd_plan_timing_query returns the summed
 * milliseconds and the number of recorded launches of one stage
 * ("body", "fpn_lateral", "fpn0", "topk", "roi_align", "hm_attention",
 * "hm_conv1", "hm_conv2", "hm_conv3", "hm_final_decode"). */
int kpd_plan_timing(kpd_plan* plan, int enable);
/* Restrict the recording to one stage (NULL or "" = every stage): a single
 * kernel timed inside a throughput run without the other stages' event
 * bubbles. */
int kpd_plan_timing_stage(kpd_plan* plan, const char* stage);
int kpd_plan_timing_query(kpd_plan* plan, const char* stage, double* total_ms, int* count);

/* Dispatch path log (diagnostics; host side only, results unchanged).  The
 * forward picks between specialised kernels by image size and batch;
 * kpd_plan_path_log(plan, 1) makes every later eager forward (kpd_forward,
 * kpd_backbone, kpd_backbone_body, and the stand-alone kpd_heatmap_head /
 * kpd_keypoint_head) record which branch each dispatch point took.
 * kpd_plan_path_query copies the last such call's distinct tokens, one per
 * line in order of first use, e.g.
 *   f1:dwsum+se16_proj  f2:fir23:t8  f4:exdw+seproj:po192  lateral:chain
 *   level0:fpn0x:tpc3  hm:hmconv:split
 * (f<i> = features.<i>, lat<i> = FPN lateral i) into buf as a C string and
 * writes the size it needs, terminator included, to *need (both nullable).
 * A replayed hipGraph takes no decision and leaves the list empty.  With
 * plan == NULL the list is every token this build can emit, "*" standing
 * for a block / lateral index or a value chosen at run time.  Off (the
 * default) a dispatch point costs one branch. */
int kpd_plan_path_log(kpd_plan* plan, int enable);
int kpd_plan_path_query(kpd_plan* plan, char* buf, size_t bytes, size_t* need);

/* Greedy NMS on one set of n cxcywh boxes (device), reference semantics
 * (IoU > thr suppressed, score-descending order, ties -> lower index).
 * keep: [n] int32 out (first *n_keep valid), n_keep: [1] int32 out (device).
 * max_output <= 0 means unlimited. */
int kpd_nms(const float* boxes, const float* scores, int n, float iou_threshold, int max_output,
            int32_t* keep, int32_t* n_keep, void* stream);

/* Preprocessing: the reference's ITransform
 * (dll/data/transforms.py:9-113) on the device.  src: uint8 HWC image
 * (C = 1 or 3, row pitch in bytes, device memory); dst: fp32 [C'][out_h][out_w]
 * (device), C' = 1 with KPD_PRE_GRAY.  Stages in order: RGB->gray (cv2
 * fixed point), CLAHE per plane (clip_limit, tiles_x x tiles_y), the gray
 * pipeline's edge blend (to_grayscale_clahe :55-73: blur, median, Canny,
 * morphology, addWeighted; single plane only), Gaussian 3x3 sigma 0.5 (RGB
 * pipeline, :105), PIL-exact bilinear resize, ToTensor + Normalize(mean, std)
 * (host arrays of C' floats).  Replaces ITransform.__call__
 * (transforms.py:110-113).  This is kpd_preprocess_batch (below) with n = 1:
 * the same code, so the same checks (a failure's message begins
 * "kpd_preprocess:"), one stream-ordered scratch allocation, a pitched image
 * read in place, no synchronisation. */
#define KPD_PRE_GRAY 1
#define KPD_PRE_CLAHE 2
#define KPD_PRE_BLUR 4
#define KPD_PRE_EDGES 8
int kpd_preprocess(const uint8_t* src, int height, int width, int channels, int pitch, int flags, float clip_limit,
                   int tiles_x, int tiles_y, int out_h, int out_w, const float* mean, const float* std, float* dst,
                   void* stream);

/* kpd_preprocess over n images in one call (directory inference: decode on
 * the host, one batched preprocess, one forward).  srcs / heights / widths /
 * pitches: host arrays of n entries -- device pointers to uint8 HWC images
 * that share the channel count `channels`, each with its own size and row
 * pitch in bytes (any pitch >= width * channels: a strided view needs no
 * dense copy).  flags, CLAHE parameters, output size, mean and std are shared.
 * dst: fp32 [n][C'][out_h][out_w], contiguous (device) -- the forward's input.
 * kpd_preprocess runs this code with n = 1, and an image's result does not
 * depend on the images it is batched with: every stage is integer or
 * contraction-free arithmetic within one image.
 *
 * Every stage takes the image index in its grid and reads the image's
 * geometry from a descriptor table that travels by value in the kernel
 * arguments, one table per chunk of KPD_PRE_BATCH_CHUNK images: a call issues
 * one memset (edge pipeline), at most 13 launches per chunk and one
 * hysteresis launch per four chunks, however many images a chunk holds.  The
 * Canny hysteresis floods up to 4 * KPD_PRE_BATCH_CHUNK images concurrently,
 * one workgroup each; the chain behind it (dilate, erode, dilate, erode,
 * Gaussian 3x3, maximum) is one LDS-tiled kernel.
 *
 * Arguments are checked before any device work: non-null pointers, n > 0,
 * channels 1 or 3, positive sizes, GRAY only on 3 channels, EDGES only on a
 * single-plane pipeline, and per image pitch >= width * channels, a CLAHE
 * tile grid within the image and a downscale factor of at most 31; a failure
 * is KPD_EINVAL and its message names the first offending image
 * ("image <i>: ...").  Scratch is one stream-ordered
 * allocation per call (hipMallocAsync, freed on the stream), carved by prefix
 * sums over the images with 64-bit offsets.  The call does not synchronise
 * and reads none of the host arrays after it returns. */
#define KPD_PRE_BATCH_CHUNK 32
int kpd_preprocess_batch(const uint8_t* const* srcs, const int* heights, const int* widths, const int* pitches,
                         int n, int channels, int flags, float clip_limit, int tiles_x, int tiles_y, int out_h,
                         int out_w, const float* mean, const float* std, float* dst, void* stream);

/* Pose overlays on the device: person boxes, skeleton limbs,
 * joints and an optional heatmap underlay drawn in place onto n uint8 HWC RGB
 * images, straight from a forward's output tensors.  What the CLI's
 * "Saved visualization to ..." promises (reference scripts/predict.py:86-131,
 * which imports a drawing function its package never defines).
 *   images / heights / widths / pitches: host arrays of n entries -- device
 *       pointers to 3-channel images, each with its own size (sides <=
 *       KPD_DRAW_MAX_SIDE) and row pitch in bytes, pitch >= 3 * width; no byte
 *       outside [row, row + 3 * width) of any row is written, so a column
 *       slice of a wider tensor is drawn in place.
 *   keypoints    [n][P][K][2] fp32 normalised image coordinates (device): the
 *                memory of the forward's [n][P][1][K][2];
 *   visibilities [n][P][K][3] fp32 one-hot (device);
 *   boxes        [n][P][4] fp32 cxcywh normalised (device), or NULL;
 *   heatmap      [n][P][K][hh][hw] fp32 (device), or NULL; hh, hw <= KPD_DRAW_MAX_HEAT.
 *   limbs [L][2] joint indices, limb_colors [L][3], joint_colors [3][3] (one
 *   RGB colour per visibility class), box_color [3]: host tables.
 *   joint_radius, limb_half_width, box_half_width: 1/16-pixel units, each in
 *   [0, KPD_DRAW_MAX_WIDTH]; alpha, heat_alpha in [0, 256]; min_class in
 *   {0, 1, 2}: joints of a lower visibility class are not drawn.
 *   flags: KPD_DRAW_* layers.  KPD_DRAW_BOXES and KPD_DRAW_HEAT need boxes,
 *   KPD_DRAW_HEAT needs heatmap.  K in [1, 32], L in [0, 64], P >= 1.
 * The drawing rules are integer arithmetic on a 16-subpixel grid and are
 * written out in DESIGN.md §3b; tests/draw_ref.py restates them in numpy and
 * the result is bit-equal.  Image i's result does not depend on the images it
 * is drawn with.
 *
 * A setup kernel writes one 64-byte record per (image, person, primitive);
 * one 256-thread workgroup per KPD_DRAW_TILE_W x KPD_DRAW_TILE_H tile culls
 * the image's records against the tile in blocks of 256, in record order, and
 * blends the survivors into pixels held in registers; a tile nothing touches
 * is neither loaded nor stored.  Images are addressed through a descriptor
 * table passed by value, one table (two launches) per chunk of KPD_DRAW_CHUNK
 * images; the heat layer adds one launch per call.
 *
 * Arguments are checked before any device work; a failure is KPD_EINVAL and
 * per-image failures read "image <i>: ...".  Scratch is one stream-ordered
 * allocation per call.  The call does not synchronise and reads no host
 * array after it returns (the tables travel in the kernel arguments). */
#define KPD_DRAW_BOXES 1
#define KPD_DRAW_LIMBS 2
#define KPD_DRAW_JOINTS 4
#define KPD_DRAW_HEAT 8
#define KPD_DRAW_CHUNK 32      /* images per descriptor table */
#define KPD_DRAW_TILE_W 64     /* pixels of one workgroup's tile */
#define KPD_DRAW_TILE_H 16
#define KPD_DRAW_MAX_SIDE 16384
#define KPD_DRAW_MAX_WIDTH 512 /* 32 px in 1/16-pixel units */
#define KPD_DRAW_MAX_HEAT 1024
int kpd_draw_poses(uint8_t* const* images, const int* heights, const int* widths, const int* pitches, int n,
                   const float* keypoints, const float* visibilities, const float* boxes, const float* heatmap,
                   int P, int K, int hh, int hw, const int* limbs, int L, const uint8_t* limb_colors,
                   const uint8_t* joint_colors, const uint8_t* box_color, int joint_radius, int limb_half_width,
                   int box_half_width, int alpha, int heat_alpha, int min_class, int flags, void* stream);

/* Training / evaluation targets: generate_target_heatmap
 * (dll/models/heatmap_head.py:163-224).  kpts: [planes][2] normalised (x, y)
 * (device), out: [planes][H][W] fp32 (device); the (6*int(sigma)+1)^2
 * normalised Gaussian is centred at (floor(x*W), floor(y*H)) and cropped;
 * keypoints outside [0,1) leave their plane zero.  sigma is the reference's
 * Python double: the kernel size takes int() of it unrounded and 2*sigma^2 is
 * rounded to fp32 once.  Synchronises the stream (the kernel table is staged
 * from host memory). */
int kpd_target_heatmaps(const float* kpts, int planes, int H, int W, double sigma, float* out, void* stream);

/* Per-ROI training targets of the top-down HeatmapHead: the
 * person's own joints placed in the frame the head predicts in, by the
 * convention of the decoders and convert_to_original_coords (map pixel i
 * stands for i / (W - 1) of the unclamped box).  kpts [R][K][2]
 * image-normalised (x, y), vis [R][K], boxes [R][4] (cx, cy, w, h), all device
 * fp32; rows [n] int32 (device) selects and orders the ROIs, NULL = 0..n-1.
 * For output row j, r = rows[j], joint k, in fp32 without contraction:
 *   bx = cx - w/2, by = cy - h/2;  u = (x - bx) / w, v = (y - by) / h
 *   on = w > 0 && h > 0 && vis > 0 && 0 <= u <= 1 && 0 <= v <= 1
 *        (a NaN anywhere makes it false)
 *   weight[j][k] = on ? 1 : 0;  px = u * (W - 1), py = v * (H - 1)
 *   heat[j][k][y][x] = on ? expf(-((x - px)^2 + (y - py)^2) / (2 sigma^2)) : 0
 * i.e. the Gaussian of the reference's _convert_keypoints_to_heatmaps (sigma
 * 2 there): peak 1 at a sub-pixel centre, no cut-off.  heat [n][K][H][W],
 * weight [n][K] (the loss's target_weight).  KPD_EINVAL before any device
 * work: a null pointer with n > 0, n < 0, H or W < 2, K <= 0, sigma not
 * positive and finite, n > R without a row list.  Every rows[j] must lie in
 * [0, R): that is the caller's contract, the values are on the device and are
 * not checked.  n = 0 returns KPD_OK without a launch.  One launch; no
 * synchronisation, no allocation, no host table. */
int kpd_roi_targets(const float* kpts, const float* vis, const float* boxes, const int32_t* rows, int n, int R, int K,
                    int H, int W, float sigma, float* heat, float* weight, void* stream);

/* Validation metrics: Trainer._calculate_validation_metrics
 * (dll/training/trainer.py:384-429).  pred, gt: [n][2], vis: [n] (device);
 * thresholds: host array (<= 16).  out (device) = [ADE, PCK_t...]: ADE = mean
 * ||pred-gt|| over vis > 0, PCK_t = #(dist <= t and vis > 0) / n; all zero
 * when nothing is visible. */
int kpd_keypoint_metrics(const float* pred, const float* gt, const float* vis, long n, const float* thresholds,
                         int n_thresholds, float* out, void* stream);

/* COCO keypoint matching on the device: object keypoint
 * similarity (OKS) of every detection / ground-truth pair of B images and
 * COCOeval's greedy matching at T OKS thresholds (computeOks / evaluateImg for
 * keypoints at area range "all"; crowd annotations are not modelled).  The
 * per-batch half of keypoint AP: the dataset-level accumulation over the
 * outputs is a handful of tensor ops (dll/utils/oks.py).
 *   pred_kpts   [B][D][K][2] fp32 (device): the memory of a forward's
 *               [B][D][1][K][2];
 *   pred_scores [B][D] fp32 (device): a slot whose score is not > 0 (a NaN
 *               too) is absent;
 *   gt_kpts [B][G][K][2], gt_vis [B][G][K] (> 0 = labelled), gt_boxes
 *   [B][G][4] cxcywh in the keypoints' units, gt_area [B][G] in scaled units
 *   squared, n_gt [B] int32 (the valid ground truths of image b are slots
 *   0 .. n_gt[b]-1, clamped to [0, G]), scale [B][2] = (sx, sy), multiplied
 *   onto every x / y before differencing: all device;
 *   sigmas [K], thresholds [T]: host arrays (they travel in the kernel
 *   arguments, the call reads neither after it returns).
 * Rules.  var_k = (2 sigma_k)^2; k1 = the gt's labelled keypoints.  With
 * k1 > 0, dx = sx xd - sx xg over the labelled k; with k1 == 0 the gt is
 * ignored and every k measures the distance to the gt box doubled about its
 * centre (x0 = (cx - w/2) sx - w sx, x1 = (cx - w/2) sx + 2 w sx, dx =
 * max(0, x0 - sx xd) + max(0, sx xd - x1)).  e_k = (dx^2 + dy^2) / var_k /
 * (area + 2^-52) / 2 and OKS = mean of exp(-e_k) over the counted k, all in
 * double from the fp32 inputs.  Detections are ranked by score descending,
 * ties to the lower slot, the first M = min(max_dets, D) present ones kept;
 * ground truths are ordered counted ones first, each group in slot order.  Per
 * threshold t and detection in rank order: best = min(t, 1 - 1e-10); walking
 * the gts, one already matched at t is skipped, the walk stops at an ignored
 * gt once a counted one is held, a gt with OKS < best is skipped, any other
 * becomes the match and its OKS the new best (an equal OKS replaces).
 * Outputs (device):
 *   oks        [B][D][G] double, caller's slot order, 0 for an absent
 *              detection or a slot past n_gt; may be NULL;
 *   det_score  [B][M] scores in rank order, 0 past n_det;
 *   det_slot   [B][M] int32 caller slot at each rank, -1 past n_det;
 *   det_match  [B][T][M] int32 matched gt slot (caller order) or -1;
 *   det_ignore [B][T][M] uint8: the matched gt is an ignored one;
 *   gt_match   [B][T][G] int32 matched detection slot or -1;
 *   counts     [B][2] int32: n_det (ranked, <= M), n_gt_counted.
 * Inputs of present detections and valid ground truths are expected finite.
 * One launch, one workgroup per image: the OKS matrix in LDS, one wave per
 * threshold.  Arguments are checked before any device work (KPD_EINVAL, the
 * message names the argument); B = 0 returns KPD_OK without a launch; D = 0
 * or G = 0 is valid, and an array of zero elements may then be NULL.  The
 * call does not synchronise.  tests/oks_ref.py restates the rules in numpy. */
#define KPD_OKS_MAX_K 32
#define KPD_OKS_MAX_T 16
#define KPD_OKS_MAX_D 64
#define KPD_OKS_MAX_G 64
int kpd_oks_match(const float* pred_kpts, const float* pred_scores, const float* gt_kpts, const float* gt_vis,
                  const float* gt_boxes, const float* gt_area, const int32_t* n_gt, const float* scale,
                  const float* sigmas, const float* thresholds, int B, int D, int G, int K, int T, int max_dets,
                  double* oks, float* det_score, int32_t* det_slot, int32_t* det_match, uint8_t* det_ignore,
                  int32_t* gt_match, int32_t* counts, void* stream);

/* OKS pose-NMS on the device: the step of a top-down pose
 * pipeline between scoring and evaluation or drawing.  A pose whose object
 * keypoint similarity with a higher-scoring pose of the same image is too high
 * is suppressed (hard) or has its score decayed (soft).
 *   kpts   [B][D][K][2] fp32 (device): the memory of a forward's
 *          [B][D][1][K][2];
 *   scores [B][D] fp32 (device): a slot whose score is not > 0 (a NaN too) is
 *          absent;
 *   area   [B][D] in scaled units squared, kconf [B][D][K] per-keypoint
 *          confidence or NULL, scale [B][2] = (sx, sy), multiplied onto every
 *          x / y before differencing: all device;
 *   sigmas [K]: a host array (it travels in the kernel arguments, the call
 *          does not read it after it returns).
 * Rules, all in double from the fp32 inputs.  Pair OKS of present poses
 * i != j: den = (area_i + area_j) / 2 + 2^-52; keypoint k counts when kconf is
 * NULL or kconf_i[k] > vis_threshold and kconf_j[k] > vis_threshold; dx =
 * sx x_i - sx x_j, dy likewise; e_k = (dx^2 + dy^2) / (2 sigma_k)^2 / den / 2;
 * OKS = mean of exp(-e_k) over the counted k, 0 when none counts.  Pairs i < j
 * are computed and mirrored (the matrix is bit-symmetric); a pair with an
 * absent pose and the diagonal are 0.  Present poses are ranked by score
 * descending, ties to the lower slot.  threshold, vis_threshold and min_score
 * enter as the fp32 values passed.
 *   KPD_POSE_NMS_HARD: walking the ranks, the walk ends at the first pose whose
 *   score is not > min_score or once max_keep poses are kept; a pose whose OKS
 *   with an already kept pose is > threshold is suppressed (suppressed_by =
 *   the earliest-kept such pose); any other is kept with its input score.
 *   KPD_POSE_NMS_SOFT (Gaussian) / KPD_POSE_NMS_SOFT_LINEAR: current scores
 *   start as the input scores.  Repeat: take the remaining pose with the
 *   highest current score (ties to the lower slot); stop if that score is not
 *   > min_score or max_keep poses have been picked; keep it with its current
 *   score; multiply every remaining pose's current score by exp(-o^2 /
 *   threshold) (Gaussian), or by 1 - o if o >= threshold else 1 (linear), o
 *   its OKS with the pick.
 * Outputs (device):
 *   oks           [B][D][D] double, may be NULL;
 *   keep          [B][D] int32 caller slots in keep order, -1 past n_keep;
 *   n_keep        [B] int32;
 *   scores_out    [B][D] fp32 in caller slot order: the kept pose's score cast
 *                 to fp32, 0 for a suppressed, unpicked or absent slot;
 *   suppressed_by [B][D] int32 slot of the suppressing pose or -1 (always -1
 *                 in the soft modes).
 * Inputs of present poses are expected finite.  One launch, one workgroup per
 * image (an image's result does not depend on the others of the call): the OKS
 * matrix in LDS, the suppression on one wave.  Arguments are checked before
 * any device work (KPD_EINVAL, the message names the argument): D in [0,
 * KPD_POSE_NMS_MAX_D], K in [1, KPD_POSE_NMS_MAX_K], threshold in (0, 1],
 * max_keep >= 1; B = 0 returns KPD_OK without a launch; D = 0 is valid, and an
 * array of zero elements may then be NULL.  The call does not synchronise.
 * tests/pose_nms_ref.py restates the rules in numpy. */
#define KPD_POSE_NMS_MAX_D 64
#define KPD_POSE_NMS_MAX_K 32
#define KPD_POSE_NMS_HARD 0
#define KPD_POSE_NMS_SOFT 1
#define KPD_POSE_NMS_SOFT_LINEAR 2
int kpd_pose_nms(const float* kpts, const float* scores, const float* area, const float* kconf, const float* scale,
                 const float* sigmas, int B, int D, int K, int mode, float threshold, float vis_threshold,
                 float min_score, int max_keep, double* oks, int32_t* keep, int32_t* n_keep, float* scores_out,
                 int32_t* suppressed_by, void* stream);

/* Flip-test merge: the heatmaps of a forward over the images
 * and of one over their left-right mirrors, averaged and decoded in one launch.
 *   heat_a, heat_b  [n][P][K][H][W] fp32 (device): kpd_forward's heatmap of the
 *                   straight and of the mirrored pass, in the forward's
 *                   compacted person-slot order;
 *   boxes           [n][P][4] fp32 cxcywh (device): the STRAIGHT pass's boxes in
 *                   caller order, zero rows included.  The compaction is derived
 *                   here by the forward's rule: a box whose four values are all
 *                   == 0 is skipped, slot s of an image is its s-th other box;
 *   pairs           [K] (host; read before the call returns): the joint whose
 *                   mirrored plane merges into joint k -- an involution
 *                   (0 <= pairs[k] < K, pairs[pairs[k]] == k).
 * Live slot (s < the image's non-zero boxes), j = pairs[k]:
 *   m[k][y][x] = 0.5f * (a[k][y][x] + b[j][y][W-1-x])   (one fp32 add, an exact
 *   halving); peak = max m; the keypoint is the forward's decode of m with the
 *   slot's box: soft-argmax E[x] / (W-1), E[y] / (H-1) under softmax(m) (0 for
 *   W == 1 / H == 1), x = clamp(kx * w + (cx - w / 2), 0, 1), y alike; the
 *   visibility is one-hot of sigmoid(peak) (fp32, compared as a double) < 0.3 /
 *   < 0.7 / else.
 * Padding slot: zero keypoints, visibilities, peak and heat_out plane; the dummy
 * person (slot 0 of an image without a non-zero box) has visibility class 0 set
 * -- the values kpd_forward writes.
 * Outputs (device): heat_out [n][P][K][H][W] (may be NULL; may equal heat_a:
 * merged in place; any other overlap with heat_a or heat_b is KPD_EINVAL),
 * keypoints [n][P][K][2] (the memory of the forward's [n][P][1][K][2]),
 * visibilities [n][P][K][3], peaks [n][P][K] (may be NULL).
 * One launch, one wave per (slot, keypoint) plane, each input plane read once;
 * an image's result does not depend on the others of the call.  Arguments are
 * checked before any device work (KPD_EINVAL, the message names the argument):
 * K in [1, KPD_FLIP_MAX_K], H, W in [1, KPD_FLIP_MAX_SIDE], P >= 1; n = 0
 * returns KPD_OK without a launch.  No synchronisation, no allocation.
 * tests/flip_ref.py restates the rules in numpy. */
#define KPD_FLIP_MAX_K 32
#define KPD_FLIP_MAX_SIDE 1024
int kpd_flip_merge(const float* heat_a, const float* heat_b, const float* boxes, const int32_t* pairs, int n, int P,
                   int K, int H, int W, float* heat_out, float* keypoints, float* visibilities, float* peaks,
                   void* stream);

/* Training augmentation: n uint8 HWC images warped by a
 * per-image affine map (mirror, rotation, zoom) with optional gain / offset,
 * and the labels moved with the pixels.  What the reference's
 * AugmentationConfig (flip, rotate.max_angle, scale.range, prob) promises and
 * its KeypointAugmentation.__call__ leaves as a stub.
 *   srcs / heights / widths / pitches: host arrays of n entries -- device
 *       pointers to source images of `channels` (1 or 3) channels, each with
 *       its own size (sides in [1, KPD_AUG_MAX_SIDE]) and row pitch in bytes
 *       (any pitch >= width * channels);
 *   dsts: host array of n device pointers; destination i is dense
 *       [height_i][width_i][channels].  No destination may overlap any source
 *       (the warp is a gather).
 *   Per image (host arrays): q [n][6] int32, the INVERSE map in Q16 in
 *       pixel-index coordinates, rows (q00 q01 q02), (q10 q11 q12), with
 *       |q00|, |q01|, |q10|, |q11| < 2^19; N [n][6] double, the FORWARD map in
 *       normalised coordinates; mirror [n] (non-zero: left / right joints
 *       swap); gain [n] in [0, 65535] and offset [n], |offset| < 2^24, in Q8
 *       (identity 256 and 0).
 *   Per call (host): fill [3] uint8, the colour of a tap outside the source;
 *       pairs [K], the joint a mirror exchanges joint k with -- an involution,
 *       as for kpd_flip_merge.
 *   Labels (device, fp32): keypoints [n][P][K][2] normalised (x, y),
 *       visibilities [n][P][K], boxes [n][P][4] cxcywh, and one output buffer
 *       of the same shape for each.  All three inputs may be NULL for an
 *       image-only call; P, K, pairs and the outputs are then ignored.  No
 *       label output may overlap a label input (the mirror swaps joints).
 * Image rule, for output pixel (x, y) and channel ch; exact integer
 * arithmetic, arithmetic shifts, t(yy, xx) = src[yy][xx][ch] inside the source
 * and fill[ch] outside:
 *   sx  = q00 * x + q01 * y + q02            (64-bit; sy with row 1)
 *   sx5 = (sx + 1024) >> 11                  (1/32-pixel units)
 *   ix  = sx5 >> 5,  fx = sx5 & 31           (iy, fy alike)
 *   acc = (32-fx)*(32-fy)*t(iy,ix) + fx*(32-fy)*t(iy,ix+1) + (32-fx)*fy*t(iy+1,ix) + fx*fy*t(iy+1,ix+1)
 *   v   = (acc + 512) >> 10
 *   out = clamp((v * gain + offset + 128) >> 8, 0, 255)
 * Label rule, float64 with every operation rounded on its own, results stored
 * as fp32.  Output joint k is computed from input joint s = pairs[k] with the
 * mirror flag, s = k without, coordinates and visibility both.  A source joint
 * with v == 0 or x == 0 and y == 0 (padding, an unlabelled COCO joint) is
 * copied unchanged.  Any other maps to x' = (N00 * x + N01 * y) + N02, y'
 * alike; when the fp32 (x', y') is not in [0, 1) x [0, 1) the joint left the
 * frame: v' = 0, (x', y') = (0, 0); else v' = v.  An all-zero box stays
 * all-zero; any other has its corners cx -+ 0.5 * w, cy -+ 0.5 * h mapped
 * through N, the axis-aligned hull taken and each side clipped to [0, 1]; the
 * row is (0.5 * (x0 + x1), 0.5 * (y0 + y1), x1 - x0, y1 - y0), or all-zero when
 * the clipped width or height is <= 0 (the person left the frame; the forward
 * skips zero boxes).  A person's joints follow the joint rule whatever became
 * of its box.
 *
 * One launch per chunk of KPD_AUG_CHUNK images: one 256-thread workgroup per
 * KPD_AUG_TILE_W x KPD_AUG_TILE_H output tile, four consecutive pixels per
 * thread, over a flattened tile list of the chunk's images; the label work
 * rides in the same launch as extra workgroups behind the tiles.  Images and
 * parameters are addressed through a descriptor table passed by value.  Image
 * i's result does not depend on the other images of the call.
 *
 * Arguments are checked before any device work; a failure is KPD_EINVAL with
 * the argument named and per-image failures read "image <i>: ...": n >= 0,
 * channels in {1, 3}, the limits above, K in [1, KPD_AUG_MAX_K], P >= 1 (with
 * labels), pairs an involution, non-null arrays, the two overlap rules.  n = 0
 * returns KPD_OK without a launch.  No synchronisation, no allocation; no host
 * array is read after the call returns.  tests/augment_ref.py restates the
 * rules in numpy: images bit-equal, labels equal but for the fp32 store.
 * Parity with OpenCV's warpAffine (whose 1/32-pixel grid this follows) is
 * unpinned. */
#define KPD_AUG_CHUNK 16       /* images per descriptor table */
#define KPD_AUG_TILE_W 64      /* pixels of one workgroup's tile */
#define KPD_AUG_TILE_H 16
#define KPD_AUG_MAX_SIDE 16384
#define KPD_AUG_MAX_K 32
int kpd_augment_batch(const uint8_t* const* srcs, const int* heights, const int* widths, const int* pitches,
                      uint8_t* const* dsts, int n, int channels, const int32_t* q, const double* N,
                      const int* mirror, const int32_t* gain, const int32_t* offset, const uint8_t* fill,
                      const int32_t* pairs, const float* keypoints, const float* visibilities, const float* boxes,
                      int P, int K, float* keypoints_out, float* visibilities_out, float* boxes_out, void* stream);

/* Training loss: AdaptiveHeatmapLoss.forward
 * (dll/losses/keypoint_loss.py:202-280).  pred, gt: [B][K][H][W] fp32,
 * target_weight: [B][K] or NULL (all device).  Threshold = clamp(torch.quantile(
 * gt, 0.9), 0.05, 0.3) when adaptive_threshold (radix select on the device,
 * torch's fp32 rank / lerp), else 0.1.  loss_out (device, 1 float) = mean of
 * the weighted focal MSE; grad_pred (device [B][K][H][W] or NULL) = d loss /
 * d pred; threshold_out (device, 1 float, or NULL) = the threshold used.
 * Deterministic (fixed-order double reductions).  A NaN in gt is outside the
 * contract: torch.quantile returns NaN for it, the radix select orders it as
 * a number beyond the infinities and returns a finite threshold. */
int kpd_adaptive_heatmap_loss(const float* pred, const float* gt, const float* target_weight, int B, int K, int H,
                              int W, float keypoint_weight, float background_weight, int adaptive_threshold,
                              float focal_alpha, float* loss_out, float* grad_pred, float* threshold_out,
                              void* stream);

/* Training loss on the decoded keypoints: SpatialCoordinateLoss
 * (dll/losses/keypoint_loss.py:117-199) of the soft-argmax decode of every
 * plane, and its gradient with respect to the plane, in one pass.
 * heat [planes][H][W] fp32; gt [planes][2] in the decode's normalised frame;
 * vis [planes], a joint counts iff vis > 0 (all device).  Per plane
 * p = softmax((h - max h) / temperature), e = (sum p x / (W-1), sum p y / (H-1)):
 *   l = rho(e_x - g_x) + rho(e_y - g_y), d = |e - g|, f = clamp(d / distance_threshold, 1, 3)
 *   loss[0] = sum over vis > 0 of pixel_weight_scale f l / (N_vis + 1e-8)
 * rho: 0.5 z^2 for |z| < 1 else |z| - 0.5 (KPD_COORD_SMOOTH_L1, beta 1, and
 * KPD_COORD_HUBER, delta 1); z^2 (KPD_COORD_MSE).  coords [planes][2] = e of
 * every plane; grad (device [planes][H][W] or NULL) = d loss / d heat as torch
 * autograd gives it (df/de = 0 outside the open band 1 < d/tau < 3).  A plane
 * with vis <= 0 adds nothing and its gradient plane is zero by selection: its
 * gt may be NaN.  H, W >= 2; temperature, distance_threshold > 0 and finite;
 * planes = 0 writes loss 0.  Deterministic (integer count, fixed-order double
 * sum); no floating-point atomics; no host synchronisation. */
#define KPD_COORD_SMOOTH_L1 0
#define KPD_COORD_MSE 1
#define KPD_COORD_HUBER 2
int kpd_coord_loss(const float* heat, const float* gt, const float* vis, int planes, int H, int W, float temperature,
                   int loss_type, float pixel_weight_scale, float distance_threshold, float* coords, float* loss,
                   float* grad, void* stream);

/* The backward of the KPD_DECODE_SOFTARGMAX decode: grad_heat [planes][H][W]
 * = sum over c of grad_coords[plane][c] d e_c / d heat, the same plane pass
 * with the given seed. */
int kpd_softargmax_backward(const float* heat, const float* grad_coords, int planes, int H, int W, float temperature,
                            float* grad_heat, void* stream);

/* The backward of the forward's ROI align onto FPN level 0:
 * what trains the FPN neck under the heatmap head.  gout [n][Cs][56][56] =
 * dL / d(ROI features) of the rows `rows` (n ascending indices into B*P, int32,
 * device) of boxes [B][P][4] (cxcywh, normalised: the forward's); topk
 * [B][Cs] int32 (device) = the distinct level-0 channels of image b that the
 * Cs feature channels were gathered from, or NULL for Cs == C in order.
 * A box becomes a ROI exactly as kpd_roi_features makes it: corners clamped to
 * [0, 1] and scaled by W, H, extent at least 1, aligned=False, sampling grid
 * ceil(extent / 56), the sample coordinates in fp32 in torchvision's
 * expression order without contraction and the skip / clamp decisions taken
 * on them.  gfeat [B][C][H][W] (NCHW) = dL / d(level 0) is written completely
 * and every element exactly once: a ROI's channel s lands in channel
 * topk[b][s], the ROIs of an image are summed in ascending row order, and
 * pixels no ROI touches, channels topk[b] does not name and images without a
 * row are zeros -- no memset before the call.  No floating-point atomics: two
 * calls give the same bits, and an image's gradient depends on its own rows
 * only, not on what shares the call.  n = 0 is legal (all zeros).  Arguments
 * are checked before any device work (KPD_EINVAL: n > B*P, Cs > C, Cs != C
 * without topk, a null gout / boxes / rows with n > 0, a null gfeat, a map too
 * wide for the workgroup's LDS tables: W up to about 550, any H); rows outside
 * [0, B*P), or not ascending, and repeated topk entries are the caller's
 * contract (such rows are ignored or summed in an unspecified order; nothing
 * is read or written out of bounds).  No scratch, no host synchronisation. */
int kpd_roi_align_backward(const float* gout, const float* boxes, const int32_t* rows, int n, int B, int P,
                           const int32_t* topk, int Cs, int C, int H, int W, float* gfeat, void* stream);

/* Concurrency: a forward pass over B >= 32 images runs as min(n, B/16)
 * contiguous sub-batches on as many streams (forked from / joined back into
 * the caller's stream), so the latency-bound small launches of one sub-batch
 * overlap the other's.  n in [1, 4]; default 1 (n = 2 measured +4% images/s at
 * C2, but every kernel then shares the GPU with the other sub-batch, so
 * per-kernel timings no longer describe the kernel).  Results do not depend
 * on n: every split-precision scale is per image / per ROI. */
int kpd_plan_set_streams(kpd_plan* plan, int n);

/* Not part of the reference interface: replay whole forwards as hipGraphs.
 * With enable != 0, a kpd_forward call whose signature (shapes, flags, every
 * buffer address, the stream) repeats runs eagerly once, is captured the
 * second time and from then on is one hipGraphLaunch on the caller's stream
 * (the ~60 launches of a forward, not its kernels, set the latency of a
 * small batch).  A workspace re-carve or re-finalize invalidates the graphs;
 * stage timing forces eager forwards.  Results are identical either way.
 * Default: off (KPD_GRAPH=1 in the environment: on).  Measured at 64 and 1
 * images back to back, replay is no faster than the eager launches (the GPU
 * is the bound there); one synchronous 1-image forward (C1) took 0.62 ms
 * replayed against 0.67 ms eager.
 * The signature includes every buffer address: replay needs caller-owned
 * buffers reused from call to call (a caller that allocates new outputs per
 * call gets a new signature, i.e. an eager run, whenever an address changes).
 * enable = 2: on, and the next capture is abandoned as if it had failed (the
 * call then runs eagerly with the plan's workspace state restored) -- a test
 * hook for that recovery path. */
int kpd_plan_set_graphs(kpd_plan* plan, int enable);

/* Diagnostics (not part of the reference interface): times the LDS-DMA 3x3
 * conv (conv_glds.hip) on synthetic operands, N x H x W pixels, cin -> cout;
 * split != 0 selects the fp32-accurate FPN level-0 form (cin = cout = 128).
 * dbg: 0 full kernel, 1 without the K-loop loads, 2 without the MFMAs,
 * 4 with an L2-resident A working set.  *ms = mean time per launch.  The
 * ablations (dbg != 0) exist only in a diagnostic build (kpd_build_flags). */
int kpd_bench_conv16(int split, int N, int H, int W, int cin, int cout, int dbg, int iters, float* ms);

/* Build flags of this library: bit 0 (KPD_BUILD_DIAG) = diagnostic build
 * (make DIAG=1), which reads the KPD_* A/B and ablation switches and the
 * KPD_STAMPS phase stamps from the environment.  The default build reads
 * none of them (only KPD_GRAPH, the kpd_plan_set_graphs default). */
#define KPD_BUILD_DIAG 1
int kpd_build_flags(void);

/* Diagnostics (host only, no device needed): the packed position-class table
 * of the split FPN level 0.  Class c = (y % 4) * 4 + x % 4: cls_ng[16] its
 * lateral-1 pixel groups, cls_g[16 * 4] their ids (oy + 1) * 3 + (ox + 1),
 * cls_woff[16] the f16-element offset of its weight block -- classes with the
 * same lateral term share one block.  *blocks = the distinct group blocks. */
int kpd_fpn0x_class_table(int* cls_ng, int* cls_g, int* cls_woff, int* blocks);

/* ---- Stand-alone operators: the reference's submodule forwards and helper
 * functions, for callers that use them outside MultiPersonKeypointModel.forward.
 * Tensors are NCHW fp32 device memory, exactly as the reference modules take
 * and return them.  Plan-based entries need a plan holding that submodule's
 * weights under the model's state-dict names (a partial plan is fine: a
 * finalize packs the components it finds -- backbone.body, backbone.fpn,
 * channel_attention, heatmap_head, person_detector, keypoint_head). */

/* HeatmapHead.forward (heatmap_head.py:81-113): x [R][64][56][56] ->
 * heat [R][17][56][56] (sigmoid maps); attention weights ch_w [R][64] and
 * sp_w [R][56][56] (nullable).  parts = KPD_HEAD_* selects the stages: a
 * disabled attention uses weights 1 (use_attention=False), parts without
 * KPD_HEAD_CONVS computes only the attention weights (the attention modules'
 * own forwards, :129-151). */
int kpd_heatmap_head(kpd_plan* plan, const float* x, int R, int H, int W, int parts, float* heat, float* ch_w,
                     float* sp_w, void* stream);

/* KEYPOINT_HEAD.forward (keypoint_head.py:50-62): x [R][128][56][56] ->
 * keypoints [R][17][2], visibility [R][17][3] (sigmoid outputs). */
int kpd_keypoint_head(kpd_plan* plan, const float* x, int R, int H, int W, float* keypoints, float* visibility,
                      void* stream);

/* MobileNetV3Wrapper.forward (backbone.py:258-264 + LightweightFPN :29-39):
 * image [B][C][H][W] -> the four FPN levels out_i [B][128][h_i][w_i] at the
 * strides of features.0 / .3 / .8 / .12 (2, 8, 16, 32). */
int kpd_backbone(kpd_plan* plan, const float* image, int B, int C, int H, int W, float* out0, float* out1,
                 float* out2, float* out3, void* stream);

/* MobileNetV3Wrapper.body(x) (backbone.py:250-254: create_feature_extractor
 * over mobilenet_v3_small, return_nodes features.0 / .3 / .8 / .12):
 * image [B][C][H][W] -> feat0 [B][16][h0][w0], feat1 [B][24][h3][w3],
 * feat2 [B][48][h8][w8], feat3 [B][576][h11][w11] (strides 2, 8, 16, 32). */
int kpd_backbone_body(kpd_plan* plan, const float* image, int B, int C, int H, int W, float* feat0, float* feat1,
                      float* feat2, float* feat3, void* stream);

/* LightweightFPN.forward (backbone.py:29-39) on caller taps feat_i
 * [B][c_i][h_i][w_i], c = 16, 24, 48, 576; sizes = {h0, w0, h1, w1, h2, w2,
 * h3, w3} (host array).  Lateral i+1 is nearest-resized to (h_i, w_i) and added to lateral
 * i (F.interpolate 'nearest' indexing); out_i [B][128][h_i][w_i] = fpn_convs[i]
 * (3x3 + BN + ReLU) of lateral i, exact fp32 products. */
int kpd_backbone_fpn(kpd_plan* plan, const float* feat0, const float* feat1, const float* feat2, const float* feat3,
                     int B, const int* sizes, float* out0, float* out1, float* out2, float* out3, void* stream);

/* The trunk's ROI features, exactly as the fused forward serves them to
 * HeatmapHead: the stages of a kpd_forward pass with flags 0
 * up to and including the ROI align -- body, laterals, level 0 (on the ROI
 * footprints where the forward takes that path), top-k, slot map, ROI align --
 * and no head.  image [B][C][H][W], boxes [B][P][4] (cx, cy, w, h; P > 0), as
 * kpd_forward takes them; rows [n] int32 (device), ascending indices into B*P,
 * selects ROIs, NULL = all B*P (then n must equal B*P).  out [n][64][56][56]
 * NCHW = the selected rows of the pass's ROI buffer (debug buffer "roi",
 * [B*P][56][56][64]), bit for bit.  A row index outside [0, B*P) is skipped
 * (its output row is left unwritten).  Batches above the pass limit run as
 * consecutive passes on the caller's stream in workspace slot 0; no sub-batch
 * streams, never captured into a graph, no synchronisation.  It shares the
 * plan's workspace with kpd_forward and leaves it as a forward of the same
 * shapes would (debug buffers are dropped); needs the backbone, fpn and
 * channel_attention weights, not the heads'.  Arguments are validated as
 * kpd_forward's are. */
int kpd_roi_features(kpd_plan* plan, const float* image, int B, int C, int H, int W, const float* boxes, int P,
                     const int32_t* rows, int n, float* out, void* stream);

/* ChannelAttention.forward (keypoint_model.py:33-44) on x [B][128][H][W] ->
 * scores [B][128] (sigmoid); select_top_k_channels (:653-661): topk [B][k]
 * int32 (descending score, ties to the lower index) and selected
 * [B][k][H][W] = x[b, topk[b]] (both nullable).  k = 64.
 * Non-finite input follows torch: the order is total, a NaN score ranks
 * before every number (index ascending among NaNs), so topk[b] always holds
 * k distinct indices in [0, 128).  The ReLU of the FC keeps a NaN, so a NaN
 * anywhere in image b (its channel mean is NaN, and every hidden unit reads
 * every channel) makes all 128 scores of b NaN and topk[b] = 0 .. k-1; an
 * infinity gives the scores IEEE arithmetic gives (inf - inf = NaN). */
int kpd_channel_attention(kpd_plan* plan, const float* x, int B, int C, int H, int W, float* scores, int32_t* topk,
                          int k, float* selected, void* stream);

/* Heatmap decoders over `planes` maps of H x W (device):
 *   KPD_DECODE_ARGMAX     decode_heatmaps (heatmap_head.py:265-296)
 *   KPD_DECODE_SUBPIXEL   decode_heatmaps_subpixel (:298-370), param = window size
 *   KPD_DECODE_SOFTARGMAX decode_heatmaps_soft_argmax (:372-413), param = temperature
 *   KPD_DECODE_MODEL      MultiPersonKeypointModel.decode_heatmap (keypoint_model.py:250-313):
 *                         soft-argmax + 3-class visibility vis [planes][3]
 * keypoints [planes][2] normalised, scores [planes] (the maximum; nullable).
 * Edges, as torch has them: the maximum is torch.max's (first index on ties,
 * a NaN counts as the maximum, the first NaN wins; an all -inf plane gives
 * index 0); a sub-pixel window whose mass is not positive (zero, negative,
 * NaN) or that is empty (negative window size: pad = floor(w / 2) < 0) gives
 * zeros; soft-argmax divides by any non-zero temperature (0 is rejected with
 * KPD_EHIP before a launch), and a NaN in the plane or an all -inf plane
 * gives NaN coordinates, as softmax does; a NaN maximum is visibility class 2
 * (it fails both comparisons).  H, W >= 2. */
#define KPD_DECODE_ARGMAX 0
#define KPD_DECODE_SUBPIXEL 1
#define KPD_DECODE_SOFTARGMAX 2
#define KPD_DECODE_MODEL 3
int kpd_decode_heatmaps(const float* heat, int planes, int H, int W, int mode, float param, float* keypoints,
                        float* scores, float* vis, void* stream);

/* torchvision.ops.roi_align as extract_roi_features calls it
 * (keypoint_model.py:212-228): features [B][C][H][W], rois [R][5] =
 * (batch index, x1, y1, x2, y2) -> out [R][C][out_h][out_w].  The batch
 * index is truncated towards zero as torchvision does; a ROI whose index does
 * not name one of the B images (or is NaN) reads nothing and gives zeros. */
int kpd_roi_align(const float* features, int B, int C, int H, int W, const float* rois, int R, int out_h, int out_w,
                  float spatial_scale, int sampling_ratio, int aligned, float* out, void* stream);

/* 1x1 convolution with bias on NCHW (PERSON_HEAD.forward's box head,
 * person_head.py:141-166): out [B][Cout][HW] = w [Cout][Cin] . x [B][Cin][HW] + b. */
int kpd_conv1x1(const float* x, int B, int Cin, int HW, const float* w, const float* b, int Cout, float* out,
                void* stream);

/* Training side (the backward of the heatmap head's 3x3
 * convolutions: nn.Conv2d(C, O, 3, padding=1), heatmap_head.py:31-45,55-66,
 * whose gradients the reference takes from autograd in Trainer.train,
 * trainer.py:263,272).  NCHW fp32 device tensors; fp32-accurate arithmetic
 * (the heatmap convs' split f16 hi / lo products with fp32 accumulation at
 * 56 x 56 with 64 | 256 channels, and for every wgrad; exact fp32 products
 * otherwise), deterministic fixed-order sums.  Scratch comes from the
 * stream-ordered allocator; no host synchronisation.
 *   kpd_conv3x3_forward:  y [N][O][H][W] = conv(x [N][C][H][W], w [O][C][3][3]) + b (b nullable)
 *   kpd_conv3x3_backward: for gy = dL/dy [N][O][H][W]: gx = dL/dx, gw = dL/dw
 *                         [O][C][3][3], gb = dL/db [O] (each nullable). */
int kpd_conv3x3_forward(const float* x, const float* w, const float* b, int N, int C, int H, int W, int O, float* y,
                        void* stream);
int kpd_conv3x3_backward(const float* x, const float* w, const float* gy, int N, int C, int H, int W, int O,
                         float* gx, float* gw, float* gb, void* stream);
/* The same two calls with the arithmetic chosen by `precision`:
 *   KPD_PRECISION_SPLIT: the calls above, bit for bit.
 *   KPD_PRECISION_MIXED: bf16 mixed precision for training.
 *     Every product of the forward, the dgrad and the wgrad is the product of
 *     its two operands each rounded to bf16 (nearest even) from its fp32
 *     value, accumulated in fp32: one v_mfma_f32_16x16x32_bf16 per MAC group
 *     instead of three f16 products, and no scale passes.  The bias is added
 *     in fp32; gb is the sum of the unrounded gy (the split path's kernels and
 *     bits).  Tensors stay NCHW fp32; fixed-order sums, deterministic.
 * Any other value: KPD_EINVAL. */
int kpd_conv3x3_forward_prec(const float* x, const float* w, const float* b, int N, int C, int H, int W, int O,
                             float* y, int precision, void* stream);
int kpd_conv3x3_backward_prec(const float* x, const float* w, const float* gy, int N, int C, int H, int W, int O,
                              float* gx, float* gw, float* gb, int precision, void* stream);

/* Training side: nn.BatchNorm2d in train mode (batch statistics) fused with
 * the ReLU and the Dropout2d that follow it in the heatmap head's
 * deconv_layers and final_layer (heatmap_head.py:31-45,55-66), forward and
 * backward.  NCHW fp32 device tensors, the layout the conv3x3
 * entries above take and return.  gamma, beta: [C] or NULL (1 / 0); drop:
 * [N][C] multiplier per (image, channel) plane or NULL (1) -- Dropout2d with
 * rate p is a multiplier of 0 or 1 / (1 - p), drawn by the caller.  With
 * n = N * H * W values per channel:
 *
 * Statistics: mean_c = sum x / n, var_c = sum (x - mean_c)^2 / n (biased),
 * invstd_c = 1 / sqrt(var_c + eps): sums and these three in double;
 * save_mean [C] and save_invstd [C] are their fp32 roundings.  The summation
 * order depends on (N, C, H, W) alone (no atomics, no partition that depends
 * on the device's state): two calls on the same inputs are bit-identical, in
 * every output of both entries.
 * Running statistics (running_mean, running_var: [C] in/out, both or neither
 * NULL): rm <- (1 - momentum) rm + momentum mean_c, rv <- (1 - momentum) rv +
 * momentum var_c n / (n - 1) (the unbiased variance, as F.batch_norm), in
 * double, stored as fp32.
 * Forward, per element in fp32: xhat = (x - save_mean_c) * save_invstd_c,
 * pre = fmaf(xhat, gamma_c, beta_c), y = (flags & KPD_BN_RELU ? max(pre, 0) :
 * pre) * drop[n][c].
 * Backward, for gy = dL/dy: g = gy * drop[n][c] * [pre > 0] (the last factor
 * with KPD_BN_RELU only; xhat and pre recomputed from x by the forward's own
 * code, so the mask is bitwise the forward's); gbeta_c = sum g and ggamma_c =
 * sum g * xhat in double in a fixed order, stored as fp32; gx = gamma_c
 * invstd_c (g - gbeta_c / n - xhat ggamma_c / n), the three per-channel
 * coefficients gamma_c invstd_c, gbeta_c / n, ggamma_c / n prepared in double
 * (the two means carried as fp32 hi + lo pairs, so that sum gx over a channel
 * keeps no common rounding shift) and the element arithmetic in fp32.  gx,
 * ggamma, gbeta are each nullable
 * (gx alone may be requested); flags, gamma, beta, drop and the save buffers
 * are the forward's.
 *
 * Two passes each way -- statistics then apply (x read twice, y written),
 * reduce then apply (x and gy read twice, gx written) -- with 16-byte accesses
 * when H * W % 4 == 0 and the tensors are 16-byte aligned, one value per
 * access otherwise.  Scratch (per-workgroup double partials) comes from the
 * stream-ordered allocator; no host synchronisation.
 *
 * Arguments are checked before any device work; a failure is KPD_EINVAL with
 * the argument named: N, C, H, W >= 1; n > 1 ("expected more than 1 value per
 * channel", torch's ValueError); eps > 0; momentum in [0, 1]; x, y, gy and the
 * save buffers non-null; the running pointers both given or both NULL; y does
 * not overlap x (the backward reads x again); gx overlaps neither x nor gy. */
#define KPD_BN_RELU 1
int kpd_bn_train_forward(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta,
                         const float* drop, float eps, float momentum, float* running_mean, float* running_var,
                         int flags, float* y, float* save_mean, float* save_invstd, void* stream);
int kpd_bn_train_backward(const float* x, const float* gy, int N, int C, int H, int W, const float* gamma,
                          const float* beta, const float* drop, const float* save_mean, const float* save_invstd,
                          int flags, float* gx, float* ggamma, float* gbeta, void* stream);

/* Training side: the person detector on frozen trunk features.
 * The reference has no detection loss, no anchor matching and no box encoding:
 * the rules are build-defined, like the eval detector's glue, and pinned to
 * the float64 restatement tests/det_train_ref.py.  A = 28,224 anchors in the
 * candidate order (i, j, a) of the eval detector; anchor n is (ax, ay, aw, ah)
 * = (anchors[n][0], anchors[n][1], anchors[n][2] / img_w, anchors[n][3] /
 * img_h) in fp32.  GT boxes [B][G][4] are normalised (cx, cy, w, h), 0 <= G <=
 * KPD_DET_MAX_GT; a row is absent if all four values are 0, if w <= 0 or
 * h <= 0, or if any value is NaN.  Every entry checks its arguments before any
 * device work (KPD_EINVAL, the argument named), takes scratch from the
 * stream-ordered allocator and never synchronises the host.
 *
 * The detector's input: the forward's own stages -- body, laterals, FPN level
 * 0 at every pixel -- then the adaptive average pool to the 56 x 56 anchor
 * grid, summed in the order of the eval detector's pool.  image [B][C][H][W]
 * -> out [B][3136][128] (cell i * 56 + j, channel).  Needs the backbone and
 * fpn weights only; shares the plan's workspace as the ROI-feature entry does
 * (debug buffers are dropped), on the caller's stream, never captured. */
#define KPD_DET_ANCHORS 28224
#define KPD_DET_MAX_GT 64
int kpd_detector_features(kpd_plan* plan, const float* image, int B, int C, int H, int W, float* out, void* stream);

/* Anchor matching.  IoU in fp32 with the operation order of the NMS's IoU
 * (eps 1e-16), no contraction.  Per image and anchor n: best = the maximum IoU
 * over the present GTs, arg = its slot (ties: the lower slot); best >= pos_thr:
 * assign[n] = arg; neg_thr <= best < pos_thr: -2 (ignored); otherwise -1
 * (negative).  Then, for each present GT g with gmax_g = max_n IoU(n, g) > 0,
 * every anchor with IoU(n, g) >= gmax_g - min(tie_eps, gmax_g / 2) gets
 * assign[n] = its own arg (low-quality matches; overrides -1 / -2).  The band
 * is capped at half the maximum so that a sub-pixel GT, whose gmax is below
 * tie_eps, claims the anchors that tie its maximum and not every anchor of the
 * image; for gmax_g >= 2 tie_eps the band is tie_eps.  An anchor whose IoU
 * with every present GT is 0 is never positive.  A present row whose IoU is 0
 * everywhere (an infinite width or centre, a box outside the image) has gmax 0
 * and matches nothing.  n_pos[b] = the number of
 * assign >= 0; an image without a present GT is all -1.  assign [B][A] int32,
 * n_pos [B] int32, gt_best [B][G] (gmax; 0 for an absent row; nullable).
 * gt_boxes may be NULL when G = 0.  Two launches: the per-GT maxima by
 * atomicMax on the bit pattern of the non-negative IoU (order-independent),
 * then the assignment.  pos_thr in (0, 1], neg_thr in [0, pos_thr], tie_eps
 * >= 0. */
int kpd_detector_targets(const float* anchors, const float* gt_boxes, int B, int G, int img_h, int img_w,
                         float pos_thr, float neg_thr, float tie_eps, int32_t* assign, int32_t* n_pos,
                         float* gt_best, void* stream);

/* Detection loss and the gradients of box_heads[0] / cls_heads[0].  pooled
 * [B][3136][128] (the features entry above), box_w [36][128], box_b [36],
 * cls_w [9][128], cls_b [9], assign / n_pos from the matching.  Per cell, d =
 * the 36 box deltas and z = the 9 logits of the 1x1 heads (exact fp32
 * products, fp32 accumulation).  Class term, with t = [assign >= 0], p =
 * sigmoid(z): FL = -alpha (1-p)^gamma log p (t = 1), -(1-alpha) p^gamma
 * log(1-p) (t = 0), the logs through a stable softplus; ignored anchors
 * contribute 0.  Box term on positives: smooth-L1 (beta) of d - target, target
 * = ((gcx-ax)/aw, (gcy-ay)/ah, log(gw/aw), log(gh/ah)), the decode's inverse
 * without its exp clip.  N = max(1, sum_b n_pos[b]), read on the device: it
 * follows n_pos alone, not the number of non-negative entries of assign.
 * assign need not come from the matching: an entry >= G (G = 0 included) is
 * treated as -2 and an entry below -2 as -1, bit for bit; an entry in [0, G)
 * must name a present row of gt_boxes (the row is read as given: an absent
 * row's zeros or NaN go into the log targets).
 *   loss[0] = (sum FL + box_weight * sum SL1) / N, loss[1] = sum FL / N,
 *   loss[2] = sum SL1 / N
 * and g_* = d loss[0] / d parameter in closed form, each of the parameter's
 * shape; the four gradient outputs are given together, or all NULL for the
 * loss alone (the same loss bits).  One fused pass over pooled (no head map or
 * gradient map goes through memory) with per-workgroup partials, fp32 within a
 * block of 56 cells and across the blocks a workgroup owns (a map that depends
 * on B alone; the bias gradients' column sums in double), and one launch that sums the partials in index order in
 * double: no floating-point atomics, two calls are bit-identical.  alpha in
 * [0, 1], gamma >= 0, beta > 0, box_weight >= 0. */
int kpd_detector_loss(const float* pooled, const float* box_w, const float* box_b, const float* cls_w,
                      const float* cls_b, const float* anchors, const float* gt_boxes, const int32_t* assign,
                      const int32_t* n_pos, int B, int G, int img_h, int img_w, float alpha, float gamma, float beta,
                      float box_weight, float* loss, float* g_box_w, float* g_box_b, float* g_cls_w, float* g_cls_b,
                      void* stream);

/* OKS pose tracking across frames on the device: greedy OKS
 * association of every frame's poses with the live tracks of its sequence, and
 * a One-Euro filter per joint along each track.  S independent sequences of B
 * consecutive frames each, D pose slots per frame; the state is carried from
 * call to call.
 *   kpts   [S][B][D][K][2] fp32 (device);
 *   scores [S][B][D] fp32 (device): a slot whose score is not > 0 (a NaN too)
 *          is absent -- the rule of kpd_pose_nms, so a pose it suppressed is
 *          absent here;
 *   area   [S][B][D] in scaled units squared, kconf [S][B][D][K] per-keypoint
 *          confidence or NULL, scale [S][B][2] = (sx, sy), multiplied onto
 *          every x / y before differencing: all device;
 *   sigmas [K]: a host array (it travels in the kernel arguments);
 *   state  S x kpd_track_state_bytes of K bytes (device), 8-byte aligned,
 *          opaque to the caller, updated in place.  All zero = no tracks, next
 *          id 0, no frame seen.  One sequence's layout, T = KPD_TRACK_MAX_T
 *          table entries: double filter[T][K][2][2] (per coordinate: x^, dx^ in
 *          scaled units), float pose[T][K][2], float conf[T][K] (the last
 *          matched raw pose), int32 filter_valid[T][K], int32 live[T], id[T],
 *          age[T], hits[T], float area[T], sx[T], sy[T] (of the last matched
 *          pose's frame), int32 next_id, int32 frames_seen, 8 bytes unused.
 * Rules, per sequence, frames in order, all in double from the fp32 inputs.
 *   1. OKS of live track t and present pose j: the pair formula of
 *      kpd_pose_nms with the track's last matched RAW pose (its kpts, kconf,
 *      area and that frame's scale) as pose i: den = (area_t + area_j) / 2 +
 *      2^-52; keypoint k counts when kconf is NULL or both confidences are >
 *      vis_threshold; dx = sx_t x_t - sx x_j, dy likewise; e_k = (dx^2 + dy^2) /
 *      (2 sigma_k)^2 / den / 2; OKS = mean of exp(-e_k) over the counted k, 0
 *      when none counts.
 *   2. Greedy association: of the unmatched live tracks x unmatched present
 *      poses whose OKS is > threshold the pair with the greatest OKS is
 *      matched, ties to the lower track id, then the lower slot; repeated
 *      until no such pair is left.  threshold and vis_threshold enter as the
 *      fp32 values passed.
 *   3. A matched track: its last pose becomes pose j, age 0, hits + 1;
 *      track_id[j] = its id, track_hits[j] = hits, track_oks[j] = the OKS.
 *   4. An unmatched live track: age + 1; freed when the age is then > max_age
 *      (also in a frame without a present pose).
 *   5. Unmatched present poses in slot order each take a free table entry
 *      (those freed in step 4 of this frame count) as a new track: id = next
 *      id, then incremented (ids are per sequence, start at 0 and are never
 *      reused), hits 1, age 0, track_oks 0.  Without a free entry track_id =
 *      -1, track_hits = 0.
 *   6. An absent slot: track_id -1, track_hits 0, track_oks 0, kpts_out a copy.
 *   7. counts [S][B][4] = (matched, born, dropped for lack of an entry, live
 *      tracks after the frame).
 * One-Euro smoothing (smooth != 0): per track, joint and coordinate in scaled
 * units (x sx), double state.  For a matched or born track and a joint that
 * counts in the current pose (kconf NULL or > vis_threshold): without valid
 * filter state (a born track, or the joint did not count at the last match) x^
 * = x, dx^ = 0; else te = (age before the match + 1) / fps, alpha(fc) = r / (r +
 * 1) with r = 2 pi fc te, dx = (x - x^prev) / te, dx^ = alpha(d_cutoff) dx + (1 -
 * alpha(d_cutoff)) dx^prev, fc = min_cutoff + beta |dx^|, x^ = alpha(fc) x + (1 -
 * alpha(fc)) x^prev.  A joint that does not count passes through and
 * invalidates its filter state.  kpts_out [S][B][D][K][2] fp32 = x^ / sx cast to
 * fp32; a pose with track_id -1 passes through.  With smooth == 0 kpts_out may
 * be NULL and is not written.  Matching always uses raw poses.
 * Outputs (device): track_id, track_hits [S][B][D] int32, track_oks [S][B][D]
 * double (may be NULL), kpts_out, counts.
 * One launch, one 256-thread workgroup per sequence (a sequence's result does
 * not depend on the others of the call), the frames in a loop inside it: the
 * table's poses and the T x D OKS matrix in LDS, the association on one wave,
 * no atomics.  Latency-bound by construction (a sequential dependency over
 * frames on one CU per sequence).  Arguments are checked before any device
 * work (KPD_EINVAL, the message names the argument): S, B >= 0, D in [0,
 * KPD_TRACK_MAX_D], K in [1, KPD_TRACK_MAX_K], threshold in [0, 1), max_age >=
 * 0, no NaN; with smooth min_cutoff, d_cutoff, fps > 0, beta >= 0, all finite.
 * S = 0 or B = 0 returns KPD_OK without a launch; D = 0 is valid (frames still
 * age tracks), and an array of zero elements may then be NULL.  The call does
 * not synchronise.  Inputs of present poses are expected finite.  The defaults
 * of dll.utils.PoseTracker are unmeasured and parity with any external tracker
 * is not pinned.  tests/track_ref.py restates the rules in numpy.
 * The state-size query returns the bytes of one sequence's state, 0 for K
 * outside [1, KPD_TRACK_MAX_K]. */
#define KPD_TRACK_MAX_T 64
#define KPD_TRACK_MAX_D 64
#define KPD_TRACK_MAX_K 32
size_t kpd_track_state_bytes(int K);
int kpd_track_poses(const float* kpts, const float* scores, const float* area, const float* kconf,
                    const float* scale, const float* sigmas, int S, int B, int D, int K, float threshold,
                    float vis_threshold, int max_age, int smooth, float min_cutoff, float beta, float d_cutoff,
                    float fps, void* state, int32_t* track_id, int32_t* track_hits, double* track_oks,
                    float* kpts_out, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KPD_H_ */
