// What the two halves of the native runtime share (not installed): the plan,
// its packed-weight and workspace structs, and the error helpers.
//   kpd_pack.hip  weight side: BN folding, NHWC/MFMA repacking, kpd_plan_finalize
//   kpd_plan.hip  run side: workspace, kernel schedule, hipGraph replay, C ABI
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

int fail(int code, const std::string& msg);   // sets kpd_last_error (kpd_plan.hip)

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(KPD_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));               \
  } while (0)

inline int pad16(int c) { return (c + 15) / 16 * 16; }

struct HostT {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// (in, kernel, expanded, out, use_se, act(1 relu / 3 hswish), stride) -- torchvision table
struct BneckCfg { int cin, k, exp, cout; bool se; int act, s; };
const BneckCfg kBneck[11] = {
    {16, 3, 16, 16, true, ACT_RELU, 2},    {16, 3, 72, 24, false, ACT_RELU, 2},
    {24, 3, 88, 24, false, ACT_RELU, 1},   {24, 5, 96, 40, true, ACT_HSWISH, 2},
    {40, 5, 240, 40, true, ACT_HSWISH, 1}, {40, 5, 240, 40, true, ACT_HSWISH, 1},
    {40, 5, 120, 48, true, ACT_HSWISH, 1}, {48, 5, 144, 48, true, ACT_HSWISH, 1},
    {48, 5, 288, 96, true, ACT_HSWISH, 2}, {96, 5, 576, 96, true, ACT_HSWISH, 1},
    {96, 5, 576, 96, true, ACT_HSWISH, 1}};
const int kFpnIn[4] = {16, 24, 48, 576};

struct DevConv {
  int cin = 0, cout = 0, cin_p = 0, cout_p = 0, k = 1;
  bool bf16 = false;
  void* w = nullptr;
  float* b = nullptr;
  // split (fp32-accurate) copy for the heatmap-head convs: f16 [cout][9][cin/32][hi32 | lo32]
  // of w * 2^w_exp, and the output bound |y| <= bc + bs * max|x| (bc = max|b|, bs = max_co sum|w|)
  void* ws = nullptr;
  int w_exp = 0;
  float bc = 0.f, bs = 0.f;
  int ws_kc = 0;   // 1x1 split copy (kh_att2_kernel): f16 [cout_p][ws_kc][hi32 | lo32], K zero-padded to 32
};
struct DevDW { int C = 0, Cp = 0, k = 3, s = 1, act = 0; float* w = nullptr; float* b = nullptr; };
struct DevSE { int C = 0, Cp = 0, sq = 0; float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr; };
struct DevBneck {
  BneckCfg cfg;
  bool has_exp = false;
  DevConv expand, project;
  DevDW dw;
  DevSE se;
};

// KEYPOINT_HEAD conv as a split hmconv (MODE 2): several convs' columns side
// by side, f16 [cout][ntap][cin] [hi32 | lo32] weights scaled 2^w_exp, per
// column bias / second affine (ps, pt) / downsample bias (bd)
struct KhSplit {
  void* ws = nullptr;
  int w_exp = 0;
  float *b = nullptr, *ps = nullptr, *pt = nullptr, *bd = nullptr;
  int cin = 0, cout = 0, ntap = 9, ns = 0, nf = 0;
};

struct Work {  // device workspace carve for one (B,H,W,nbox,P) shape
  float* stem = nullptr;
  float* e[11] = {};
  float* d[11] = {};
  float* sesc[11] = {};
  float* o[11] = {};
  float* last = nullptr;
  float* lat[4] = {};
  float* feat = nullptr;
  float* stats = nullptr;
  int32_t* topk = nullptr;
  float* scores = nullptr;
  int32_t* slot = nullptr;
  float* roi = nullptr;
  float* roi_stats = nullptr;
  float* cw = nullptr;
  float* hsc = nullptr;   // split heatmap convs: per-ROI bounds [R][4] (max|xs|, max|h1|)
  float* smap = nullptr;
  void* xs = nullptr;
  void* h1 = nullptr;
  void* h2 = nullptr;
  float* h3 = nullptr;
  float* heat = nullptr;  // internal heat buffer when the caller passes NULL
  float* splitk = nullptr;  // split-K partial sums for small-M 1x1 convs (kSplitKFloats)
  float* pool = nullptr;    // [B][1024] SE channel means from the fused expand+depthwise kernel
  float* separt = nullptr;  // [B][kSePartFloats] SE fc1 partials (exdw_kernel -> seproj_kernel)
  float* sc = nullptr;    // split FPN scale inputs: per-image max|tap0| [B], max|lateral1| [B] (amax_publish_img)
  bool sc_dirty = true;   // sc may hold a previous forward's maxima (topk_kernel re-zeroes it)
  // person-detector glue
  float* pd_pool = nullptr;     // [B][56*56][128]
  float* pd_head = nullptr;     // [B][56*56][48]
  float* pd_boxes = nullptr;    // [B][28224][4]
  float* pd_scores = nullptr;   // [B][28224]
  int32_t* pd_keep = nullptr;   // [B][P]
  int32_t* pd_nkeep = nullptr;  // [B]
  uint8_t* pd_alive = nullptr;  // [B][28224]
  // KEYPOINT_HEAD
  float *kx = nullptr, *ksa = nullptr, *kds1 = nullptr, *krb1 = nullptr, *kds2 = nullptr, *krb2 = nullptr;
  float *kr3 = nullptr, *kv1 = nullptr, *kpr = nullptr, *kpv = nullptr, *klr = nullptr, *klv = nullptr;
  // KEYPOINT_HEAD on the split hmconv path: zero-bordered [R][57 x 57][C] f16
  // [hi32 | lo32] operands (x * att, ResidualBlock 1 / 2 outputs) and the
  // per-image FPN level-0 maximum (their scale bound, written by topk_kernel)
  void *kxs = nullptr, *kr1s = nullptr, *kr2s = nullptr;
  float* imax = nullptr;
};

struct Dims {
  int B = 0, H = 0, W = 0, NB = 0, P = 0, flags = 0;
  int h[12] = {}, w[12] = {};  // spatial dims after stem (0) and after bneck i (i+1)
  int Hf = 0, Wf = 0, tiles = 0;
  bool fused_stats = false;
  // a workspace carved for `o` serves this pass: same geometry, no larger
  // batch (kernels index by the pass's own B / NB / P; the zero borders of the
  // padded heatmap maps are written once at carve time and never overwritten)
  bool fits(const Dims& o) const {
    return H == o.H && W == o.W && flags == o.flags && tiles == o.tiles && B <= o.B && NB <= o.NB && P <= o.P &&
           (size_t)NB * P <= (size_t)o.NB * o.P;
  }
};

struct kpd_plan {
  int device = 0;
  int in_ch = 3;
  int precision = KPD_PRECISION_FP32;
  bool finalized = false;
  std::map<std::string, HostT> t;
  std::vector<void*> allocs;
  // packed device weights
  float *stem_w = nullptr, *stem_b = nullptr;
  DevBneck bn[11];
  DevConv last;
  DevConv lat[4];
  float lat_S[4] = {0.f, 0.f, 0.f, 0.f};   // max over output channels of sum |lateral weight| (lateral_chain bound)
  DevConv fpn0;
  DevConv fpn_lv[3];   // fpn_convs.1-3 (MobileNetV3Wrapper.forward only; the model's forward skips them)
  bool has_body = false, has_fpn = false, has_ca = false, has_hm = false;   // components registered
  float *ca_w0 = nullptr, *ca_b0 = nullptr, *ca_w2 = nullptr, *ca_b2 = nullptr;
  float *hca_w0 = nullptr, *hca_b0 = nullptr, *hca_w2 = nullptr, *hca_b2 = nullptr;
  float *sa_w = nullptr, *sa_b = nullptr;
  DevConv hm1, hm2, hm3;
  struct {
    _Float16* w0 = nullptr;     // composite conv3x3.L0 weights [128][5][64]
    _Float16* weff = nullptr;   // per position class [128][groups][4][64]
    int w0_bytes = 0, weff_bytes = 0, w_exp0 = 0, w_expE = 0;
    int cls_woff[16] = {}, cls_ng[16] = {}, cls_g[16][kFpn0xMaxGroups] = {};
  } fpn0x;  // FPN level 0 by linearity (conv_glds.hip, fpn0x_kernel)
  float *fin_w = nullptr, *fin_b = nullptr;
  float* zero_bias = nullptr;  // 128 zeros for bias-free laterals
  // person-detector glue: box_heads[0] ++ cls_heads[0] as one 1x1 conv (45 -> 48 ch)
  DevConv pd;
  float* anchors = nullptr;    // [28224][4] reference buffer
  float det_conf = 0.3f, det_iou = 0.3f;
  // KEYPOINT_HEAD (present when keypoint_head.* tensors were registered)
  bool has_kh = false;
  int kh_o = 14;               // regression pool size (height // 4)
  DevConv kh_sa1, kh_ds1, kh_rb1, kh_ds2, kh_rb2, kh_c3, kh_v1, kh_lr, kh_lv;
  float *kh_sa2_w = nullptr, *kh_sa2_b = nullptr;
  float *kh_bn1a_s = nullptr, *kh_bn1a_t = nullptr, *kh_bn1b_s = nullptr, *kh_bn1b_t = nullptr;
  float *kh_lnr_g = nullptr, *kh_lnr_b = nullptr, *kh_fr_w = nullptr, *kh_fr_b = nullptr;
  float *kh_lnv_g = nullptr, *kh_lnv_b = nullptr, *kh_fv_w = nullptr, *kh_fv_b = nullptr;
  // split (fp32-accurate) KEYPOINT_HEAD convs on hmconv_kernel: [ResidualBlock 1
  // (+ downsample tap) | visibility conv], [ResidualBlock 2 (+ downsample)],
  // [regression 3x3]; kh_split = all three packed (split / mixed precision)
  KhSplit kh_s[3];
  bool kh_split = false;
  // workspace, one per concurrent sub-batch (kpd_plan_set_streams)
  static constexpr int kMaxSub = 4;
  static constexpr int kOpWs = kMaxSub;   // workspace of the stand-alone operator entry points
  void* ws[kMaxSub + 1] = {};
  size_t ws_bytes[kMaxSub + 1] = {};
  Dims dims[kMaxSub + 1];
  Work work[kMaxSub + 1];
  bool have_work[kMaxSub + 1] = {};
  int streams = 1;                        // requested sub-batch streams (kpd_plan_set_streams)
  hipStream_t sub_st[kMaxSub] = {};       // [0] unused: sub-batch 0 runs on the caller's stream
  hipEvent_t fork_ev = nullptr, join_ev[kMaxSub] = {};
  // pipelined sub-batches (KPD_PIPE): sub-batch k+1 starts when sub-batch k
  // passes a stage mark, so its latency-bound body overlaps k's heavy stages
  hipEvent_t pipe_ev[kMaxSub] = {};
  // hipGraph replay of whole forwards (KPD_GRAPH=1): one executable graph per
  // call signature (shapes, flags, every buffer address, stream), valid while
  // the workspace carve and the weights are the ones it was captured on
  // never: instantiation failed for this signature -> always eager
  // done: recorded after each launch of exec on its caller's stream; retiring
  // an entry waits on it (not on the whole device) before destroying exec
  struct GraphEntry {
    hipGraphExec_t exec = nullptr; hipEvent_t done = nullptr; long epoch = -1; int seen = 0; bool never = false;
  };
  std::map<std::vector<uintptr_t>, GraphEntry> graphs;
  long ws_epoch = 0;             // bumped whenever a workspace is re-carved or the weights re-packed
  bool use_graphs = getenv("KPD_GRAPH") != nullptr && atoi(getenv("KPD_GRAPH")) != 0;   // kpd_plan_set_graphs (KPD_GRAPH=1: on)
  hipStream_t graph_st = nullptr;   // capture stream (the caller's may be the legacy default stream)
  bool graph_abandon_next = false;  // kpd_plan_set_graphs(p, 2): abandon the next capture (tests the retry)
  hipStream_t sub_st_pri[kMaxSub] = {};   // high-priority sub-batch streams (KPD_PIPE_PRI)
  std::map<std::string, std::pair<const void*, size_t>> debug;
  unsigned long long* stamps = nullptr;   // KPD_STAMPS diagnostic buffer (kStampWords)
  // per-stage HIP-event timing (kpd_plan_timing)
  struct Timer { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; };
  // dispatch path log (kpd_plan_path_log): the last forward's tokens; empty and untouched while off
  bool path_on = false;
  KpdPathLog path;
  bool timing = false;
  std::string timing_only;   // non-empty: record only this stage (kpd_plan_timing_stage)
  std::map<std::string, Timer> timers;
};
