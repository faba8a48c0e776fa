// Native runtime of the keypoint-detection hot path, run side: a shape-keyed
// device workspace, the kernel schedule of the eval forward as stages over a
// Pass, hipGraph replay and the stand-alone operators.  With kpd_pack.hip (the
// weight registry's packing) it exposes the C ABI declared in include/kpd.h.
//
// Reference call stack reproduced by kpd_forward:
//   backbone (torchvision mobilenet_v3_small features.0..12 + LightweightFPN)
//     dll/models/backbone.py:29-39, 258-264
//   select_top_k_channels          dll/models/keypoint_model.py:90, 653-661
//   per-box ROI / heatmap / decode dll/models/keypoint_model.py:143-199
#include "kpd_plan_int.h"

namespace {
thread_local std::string g_err;
}

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int kpd_fail_einval(const char* msg) { return fail(KPD_EINVAL, msg); }
int kpd_fail_hip(hipError_t e, const char* where) {
  return fail(KPD_EHIP, std::string(where) + ": " + hipGetErrorString(e));
}

// ------------------------------------------------------------------ dispatch path log
thread_local KpdPathLog* g_kpd_path = nullptr;

namespace {
struct PathRow { const char* name; unsigned sites; };
const PathRow kPathRows[KP_COUNT] = {
#define KPD_PATH_ROW(id, name, sites) {name, sites},
    KPD_PATH_TOKENS(KPD_PATH_ROW)
#undef KPD_PATH_ROW
};
const struct { unsigned site; const char* prefix; } kPathSites[] = {
    {KP_TOP, ""},       {KP_BLOCK, "f%d:"}, {KP_LAST, "last:"}, {KP_LAT, "lat%d:"},
    {KP_FPN0, "fpn0:"}, {KP_PD, "pd:"},     {KP_HM, "hm:"},     {KP_KH, "kh:"}};

// "%d" -> the value, or "*" in the listing (v < 0)
std::string path_fill(const char* fmt, int v) {
  std::string s(fmt);
  const size_t at = s.find("%d");
  if (at != std::string::npos) s.replace(at, 2, v < 0 ? "*" : std::to_string(v));
  return s;
}
std::string path_token(unsigned site, int idx, int tok, int val) {
  std::string s;
  for (const auto& ps : kPathSites)
    if (ps.site == site) s = path_fill(ps.prefix, idx);
  return s + path_fill(kPathRows[tok].name, val);
}

// forward_one's scope: the launchers log into the plan's list while it runs
struct PathScope {
  explicit PathScope(kpd_plan* p) {
    g_kpd_path = p->path_on ? &p->path : nullptr;
    kpd_path_at(KP_TOP);
  }
  ~PathScope() { g_kpd_path = nullptr; }
};
}  // namespace

// (enabled only) one entry per distinct token, in order of first use
void kpd_path_add(int tok, int val) {
  KpdPathLog& l = *g_kpd_path;
  for (const KpdPathEntry& e : l.e)
    if (e.site == l.site && e.idx == l.idx && e.tok == tok && e.val == val) return;
  l.e.push_back({l.site, l.idx, tok, val});
}

namespace {

// ------------------------------------------------------------------ workspace
constexpr long kSplitKFloats = 1L << 22;   // 16 MiB of split-K partials per workspace
constexpr int kFuseMaxPix = 32 * 24;        // input maps up to this size take the fused expand+depthwise
constexpr int kSePartFloats = 8192;         // per image: (Ep / CS) slices x sq fc1 partials

struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) / 256 * 256;
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return r;
  }
};

// mixed precision runs the HeatmapHead convs on zero-bordered ROI maps
// (hmconv_kernel); KPD_NO_HMCONV=1 keeps the unpadded generic conv (A/B)
bool hm_padded(const kpd_plan* p) {
  static const bool off = kpd_diag_env("KPD_NO_HMCONV") != nullptr;
  return (p->precision == KPD_PRECISION_MIXED || p->precision == KPD_PRECISION_SPLIT) && !off;
}

size_t carve(kpd_plan* p, const Dims& d, char* base, Work& w) {
  Carver c{base};
  const int B = d.B;
  const size_t R = (size_t)d.NB * d.P;
  w.stem = c.take<float>((size_t)B * d.h[0] * d.w[0] * 16);
  for (int i = 0; i < 11; ++i) {
    const DevBneck& bn = p->bn[i];
    const int ep = pad16(bn.cfg.exp), op = pad16(bn.cfg.cout);
    if (bn.has_exp) w.e[i] = c.take<float>((size_t)B * d.h[i] * d.w[i] * ep);
    w.d[i] = c.take<float>((size_t)B * d.h[i + 1] * d.w[i + 1] * ep);
    if (bn.cfg.se) w.sesc[i] = c.take<float>((size_t)B * ep);
    w.o[i] = c.take<float>((size_t)B * d.h[i + 1] * d.w[i + 1] * op);
  }
  w.last = c.take<float>((size_t)B * d.h[11] * d.w[11] * 576);
  const int lh[4] = {d.h[0], d.h[3], d.h[8], d.h[11]}, lw[4] = {d.w[0], d.w[3], d.w[8], d.w[11]};
  for (int i = 0; i < 4; ++i) w.lat[i] = c.take<float>((size_t)B * lh[i] * lw[i] * 128);
  w.feat = c.take<float>((size_t)B * d.Hf * d.Wf * 128);
  w.stats = c.take<float>((size_t)B * d.tiles * 2 * 128);
  w.sc = c.take<float>((size_t)2 * B * kAmaxStride);
  w.splitk = c.take<float>(kSplitKFloats);
  w.pool = c.take<float>((size_t)B * 1024);
  w.separt = c.take<float>((size_t)B * kSePartFloats);
  w.topk = c.take<int32_t>((size_t)B * 64);
  w.scores = c.take<float>((size_t)B * 128);
  w.imax = c.take<float>((size_t)B);
  if (R > 0) {
    const size_t px = R * 3136;
    const size_t es = p->precision == KPD_PRECISION_MIXED ? 2 : 4;   // bf16, or f16 hi + lo / fp32
    w.slot = c.take<int32_t>(R);
    w.roi = c.take<float>(px * 64);
    w.roi_stats = c.take<float>(R * 56 * 2 * 64);
    w.cw = c.take<float>(R * 64);
    w.hsc = c.take<float>(R * 4);
    w.smap = c.take<float>(px * 2);
    // mixed: zero-bordered ROI maps (hmconv layout, kpd_kernels.h) for the padded heatmap convs (hmconv_kernel)
    const size_t pxp = hm_padded(p) ? R * kHmRoiPos : px;
    w.xs = c.take<char>(pxp * 64 * es);
    w.h1 = c.take<char>(pxp * 256 * es);
    w.h2 = c.take<char>(pxp * 256 * es);
    w.h3 = c.take<float>(px * 64);
    w.heat = c.take<float>(R * 17 * 3136);
    if (d.flags & KPD_FLAG_DUAL_HEAD) {
      const int o = p->kh_o;
      w.kx = c.take<float>(px * 128);
      w.ksa = c.take<float>(px * 64);
      w.kds1 = c.take<float>(px * 64);
      w.krb1 = c.take<float>(px * 64);
      w.kds2 = c.take<float>(px * 32);
      w.krb2 = c.take<float>(px * 32);
      w.kr3 = c.take<float>(px * 16);
      w.kv1 = c.take<float>(px * 32);
      w.kpr = c.take<float>(R * (size_t)pad16(16 * o * o));
      w.kpv = c.take<float>(R * 512);
      w.klr = c.take<float>(R * 256);
      w.klv = c.take<float>(R * 128);
      if (p->kh_split) {
        const size_t pp = R * kHmRoiPos;
        w.kxs = c.take<char>(pp * 128 * 4);
        w.kr1s = c.take<char>(pp * (size_t)p->kh_s[0].ns * 4);
        w.kr2s = c.take<char>(pp * (size_t)p->kh_s[1].ns * 4);
      }
    }
  }
  if (d.flags & KPD_FLAG_DETECT) {
    const size_t na = (size_t)B * 3136 * 9;
    w.pd_pool = c.take<float>((size_t)B * 3136 * 128);
    w.pd_head = c.take<float>((size_t)B * 3136 * 48);
    w.pd_boxes = c.take<float>(na * 4);
    w.pd_scores = c.take<float>(na);
    w.pd_keep = c.take<int32_t>((size_t)B * std::max(d.P, 1));
    w.pd_nkeep = c.take<int32_t>(B);
    w.pd_alive = c.take<uint8_t>(na);
  }
  return c.off + 256;
}

// What the launches of one pass share: the plan, the workspace the pass runs
// in, its geometry and its stream.  The stand-alone operators fill only what
// their launches read (plan, stream, workspace or split-K scratch).
struct Pass {
  kpd_plan* p = nullptr;
  Work* w = nullptr;
  Dims d;
  hipStream_t st = nullptr;
  bool debug = false;       // record debug buffers (and KPD_STAMPS phase stamps)
  bool lin = false;         // FPN level 0 by linearity (fpn0x_ok)
  int tpc = 0;              // fpn0x tiles per (position class, image)
  float* splitk = nullptr;  // split-K partial sums (kSplitKFloats) for conv / conv_post
  std::map<std::string, std::pair<const void*, size_t>> dbg;   // replaces p->debug after top-k
  size_t stamp_off = 0;
  // KPD_STAMPS: per-workgroup phase stamps of a launch (debug buffer `name`,
  // single-stream forwards); null when off or the buffer is used up
  unsigned long long* take_stamps(const std::string& name, size_t wgs);
};

bool want_stamps() {
  static const bool on = kpd_diag_env("KPD_STAMPS") != nullptr;
  return on;
}
constexpr size_t kStampWords = 1 << 20;

unsigned long long* Pass::take_stamps(const std::string& name, size_t wgs) {
  if (!want_stamps() || !debug || stamp_off + wgs * 8 > kStampWords) return nullptr;
  unsigned long long* r = p->stamps + stamp_off;
  stamp_off += wgs * 8;
  dbg[name] = {r, wgs * 64};
  p->debug[name] = {r, wgs * 64};   // (p->debug is replaced by dbg mid-forward; heads register late)
  return r;
}

// conv with the second affine + residual + final activation epilogue
int conv_post(const Pass& ps, const DevConv& L, const void* in, int N, int H, int W, int in_cstride, void* out,
              int act, const float* post_s, const float* post_t, int act2, const float* res, int act3) {
  const hipStream_t st = ps.st;
  ConvArgs a{};
  a.in = in; a.wt = L.w; a.bias = L.b; a.out = out; a.res = res;
  a.N = N; a.H = H; a.W = W; a.cin_p = L.cin_p; a.cout_p = L.cout_p;
  a.in_cstride = in_cstride; a.out_cstride = L.cout_p;
  a.rh = H; a.rw = W; a.act = act; a.M = N * H * W;
  a.post_scale = post_s; a.post_shift = post_t; a.act2 = act2; a.act3 = act3;
  a.splitk_ws = ps.splitk; a.splitk_cap = kSplitKFloats;
  HIP_TRY(launch_conv(a, CONV_F32, L.k, st));
  return KPD_OK;
}

// RAII stage marker: records a start/end event pair on the launch stream
// when timing is enabled (events are pooled per stage and reused).
struct Stage {
  kpd_plan* p;
  hipStream_t st;
  hipEvent_t end = nullptr;
  Stage(kpd_plan* plan, const char* name, hipStream_t stream) : p(plan), st(stream) {
    if (!p->timing || (!p->timing_only.empty() && p->timing_only != name)) return;
    auto& t = p->timers[name];
    if (t.used == t.ev.size()) {
      // timing-only events: no system-scope fence when they are recorded (the
      // default event's release writes back / invalidates the L2s, ~6 us a
      // record on this device, inside the measured interval and in the way of
      // the next kernel); KPD_EVENT_FENCE=1 (diagnostic build): default events, A/B
      static const unsigned flags = kpd_diag_env("KPD_EVENT_FENCE") ? hipEventDefault : hipEventDisableSystemFence;
      hipEvent_t a, b;
      if (hipEventCreateWithFlags(&a, flags) != hipSuccess || hipEventCreateWithFlags(&b, flags) != hipSuccess) return;
      t.ev.emplace_back(a, b);
    }
    auto& pr = t.ev[t.used++];
    (void)hipEventRecord(pr.first, st);
    end = pr.second;
  }
  ~Stage() {
    if (end) (void)hipEventRecord(end, st);
  }
};

// conv()'s optional epilogue inputs: residual (nearest-upsampled from rh x rw),
// per-(image, channel) input scale, fused channel statistics (tiles per
// image), bf16 output (out_kind 1), per-image max|out| slots
struct ConvOpt {
  const float* res = nullptr;
  int rh = 0, rw = 0;
  const float* a_scale = nullptr;
  float* stats = nullptr;
  int tiles = 0;
  int out_kind = 0;
  float* amax = nullptr;
};

int conv(const Pass& ps, const DevConv& L, const void* in, int N, int H, int W, int in_cstride, void* out, int act,
         const ConvOpt& o = {}) {
  ConvArgs a{};
  a.amax = o.amax;
  a.in = in; a.wt = L.w; a.bias = L.b; a.out = out; a.res = o.res; a.a_scale = o.a_scale; a.stats = o.stats;
  a.N = N; a.H = H; a.W = W; a.cin_p = L.cin_p; a.cout_p = L.cout_p;
  a.in_cstride = in_cstride; a.out_cstride = L.cout_p;
  a.rh = o.rh; a.rw = o.rw; a.act = act; a.M = N * H * W; a.tiles_per_img = o.tiles;
  a.splitk_ws = ps.splitk; a.splitk_cap = kSplitKFloats;
  const ConvDType dt = !L.bf16 ? CONV_F32 : (o.out_kind == 1 ? CONV_BF16_OUT_BF16 : CONV_BF16_OUT_F32);
  if (L.k == 1 && !L.bf16 && o.out_kind == 0 && pw_small_ok(a)) {   // small-K 1x1: direct-to-fragment MFMA
    kpd_path(KP_CONV_PW_SMALL);
    HIP_TRY(launch_pw_small(a, ps.st));
    return KPD_OK;
  }
  HIP_TRY(launch_conv(a, dt, L.k, ps.st));
  return KPD_OK;
}

// HeatmapHead 3x3 conv + bias + BN + ReLU on the 56x56 ROI maps: bf16 weights
// go to the LDS-DMA kernel (conv_glds.hip), fp32 to the generic one.
// out_kind: 1 = bf16 output, 2 = fp32 output (bf16 weights); fp32 otherwise.
// fin (bf16 path, out_kind 2 only): fuse the final 1x1 + sigmoid into the
// epilogue and write the heatmap instead of `out` (conv_glds.hip).
struct HmFinal { const float *w, *b; const int32_t* slot; int P; float* heat; };
// split mode: per-ROI operand bounds (HmConvArgs) -- input u_in = in_c + in_s *
// hsc[r][in_idx], output u_out = out_c + out_s * hsc[r][out_idx], max|out|
// published into hsc[r][amax_idx]
struct HmSplit { float* hsc; float in_c, in_s; int in_idx; float out_c, out_s; int out_idx, amax_idx; };
int hm_conv(const Pass& ps, const DevConv& L, const void* in, int R, int in_cstride, void* out, int out_kind,
            const HmFinal* fin = nullptr, unsigned long long* stamps = nullptr, const HmSplit* sp = nullptr) {
  const kpd_plan* p = ps.p;
  const hipStream_t st = ps.st;
  if (L.ws) {   // fp32-accurate split products on the padded ROI maps
    if (!sp || !hm_padded(p)) return fail(KPD_EINVAL, "split heatmap conv needs the padded layout and bounds");
    kpd_path(KP_HM_HMCONV_SPLIT);
    HmConvArgs h{};
    h.in = in; h.wt = L.ws; h.bias = L.b; h.out = out; h.R = R; h.cin = L.cin_p; h.cout = L.cout_p;
    h.stamps = stamps;
    h.split = 1; h.hsc = sp->hsc; h.w_exp = L.w_exp;
    h.in_c = sp->in_c; h.in_s = sp->in_s; h.in_idx = sp->in_idx;
    h.out_c = sp->out_c; h.out_s = sp->out_s; h.out_idx = sp->out_idx; h.amax_idx = sp->amax_idx;
    if (fin) {
      if (L.cout_p != 64) return fail(KPD_EINVAL, "fused final layer needs the 64-channel conv");
      h.fin_w = fin->w; h.fin_b = fin->b; h.slot = fin->slot; h.P = fin->P; h.heat = fin->heat;
      h.out_idx = -1;
    }
    HIP_TRY(launch_hmconv(h, st));
    return KPD_OK;
  }
  if (!L.bf16) return conv(ps, L, in, R, 56, 56, in_cstride, out, ACT_RELU);
  if (hm_padded(p)) {
    if (in_cstride != L.cin_p) return fail(KPD_EINVAL, "hmconv: input channel stride must equal cin");
    kpd_path(KP_HM_HMCONV_BF16);
    HmConvArgs h{};
    h.in = in; h.wt = L.w; h.bias = L.b; h.out = out; h.R = R; h.cin = L.cin_p; h.cout = L.cout_p;
    h.stamps = stamps;
    if (fin) {
      if (out_kind != 2 || L.cout_p != 64) return fail(KPD_EINVAL, "fused final layer needs the 64-channel conv");
      h.fin_w = fin->w; h.fin_b = fin->b; h.slot = fin->slot; h.P = fin->P; h.heat = fin->heat;
    } else if (out_kind != 1) {
      return fail(KPD_EINVAL, "hmconv: bf16 output or the fused final layer only");
    }
    HIP_TRY(launch_hmconv(h, st));
    return KPD_OK;
  }
  kpd_path(KP_HM_CONV16);
  Conv16Args a{};
  if (fin) {
    if (out_kind != 2 || L.cout_p != 64) return fail(KPD_EINVAL, "fused final layer needs the 64-channel conv");
    a.fin_w = fin->w; a.fin_b = fin->b; a.slot = fin->slot; a.P = fin->P; a.heat = fin->heat;
  }
  a.in = in; a.wt = L.w; a.bias = L.b; a.out = out;
  a.N = R; a.H = 56; a.W = 56; a.cin_e = L.cin_p; a.cout_p = L.cout_p; a.in_cstride = in_cstride;
  a.out_cstride = L.cout_p; a.act = ACT_RELU; a.M = R * 56 * 56;
  HIP_TRY(launch_conv16(a, 0, out_kind == 1, st));
  return KPD_OK;
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

const char* kpd_last_error(void) { return g_err.c_str(); }
const char* kpd_version(void) { return "kpd 0.1 gfx950"; }
int kpd_build_flags(void) { return KPD_DIAG ? KPD_BUILD_DIAG : 0; }

int kpd_plan_create(int device, int in_channels, kpd_plan** out) {
  if (!out) return fail(KPD_EINVAL, "out is NULL");
  if (in_channels != 1 && in_channels != 3) return fail(KPD_EINVAL, "in_channels must be 1 or 3");
  auto* p = new kpd_plan();
  p->device = device;
  p->in_ch = in_channels;
  *out = p;
  return KPD_OK;
}

int kpd_plan_set_tensor(kpd_plan* p, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (!p || !name || (!host && ndim > 0)) return fail(KPD_EINVAL, "null argument");
  HostT t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return fail(KPD_EINVAL, "negative dim");
    t.shape.push_back(shape[i]);
    n *= (size_t)shape[i];
  }
  t.data.assign(host, host + n);
  p->t[name] = std::move(t);
  p->finalized = false;
  return KPD_OK;
}

// wait for a captured forward's last launch (its own event, not the device),
// then destroy it
static hipError_t retire_graph(kpd_plan::GraphEntry& g) {
  hipError_t e = hipSuccess;
  if (g.done) {
    e = hipEventSynchronize(g.done);
    (void)hipEventDestroy(g.done);
    g.done = nullptr;
  }
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  g.exec = nullptr;
  return e;
}

void kpd_plan_destroy(kpd_plan* p) {
  if (!p) return;
  int cur = 0;
  if (hipGetDevice(&cur) == hipSuccess) (void)hipSetDevice(p->device);
  for (void* a : p->allocs) (void)hipFree(a);
  for (int k = 0; k <= kpd_plan::kMaxSub; ++k)
    if (p->ws[k]) (void)hipFree(p->ws[k]);
  for (int k = 0; k < kpd_plan::kMaxSub; ++k) {
    if (p->sub_st[k]) (void)hipStreamDestroy(p->sub_st[k]);
    if (p->join_ev[k]) (void)hipEventDestroy(p->join_ev[k]);
    if (p->sub_st_pri[k]) (void)hipStreamDestroy(p->sub_st_pri[k]);
    if (p->pipe_ev[k]) (void)hipEventDestroy(p->pipe_ev[k]);
  }
  if (p->fork_ev) (void)hipEventDestroy(p->fork_ev);
  for (auto& kv : p->graphs) (void)retire_graph(kv.second);
  if (p->graph_st) (void)hipStreamDestroy(p->graph_st);
  for (auto& kv : p->timers)
    for (auto& e : kv.second.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  (void)hipSetDevice(cur);
  delete p;
}

// Images per forward pass: fpn0x_kernel's 32-bit store offsets (output and
// tap0 / lateral-1 split rows) and its per-image unscale table bound the
// batch one launch may cover; kpd_forward runs larger batches as several
// passes (images are independent, so results do not depend on the split).
static int max_pass_images(int H, int W) {
  const long hf = (H - 1) / 2 + 1, wf = (W - 1) / 2 + 1;
  const long by_extent = 0x7fffffffL / (hf * wf * 512);
  return (int)std::max(1L, std::min<long>(kFpn0xMaxImg, by_extent));
}

// FPN level 0 by linearity applies (mixed precision, packed composite weights,
// lateral 1 an exact 4x nearest upsample of the level-0 grid)
static bool fpn0x_ok(const kpd_plan* p, const Dims& d) {
  static const bool no_lin = kpd_diag_env("KPD_NO_FPN0X") != nullptr;   // A/B switch
  return p->precision != KPD_PRECISION_FP32 && !no_lin && p->fpn0x.w0 != nullptr && d.Hf == 4 * d.h[3] &&
         d.Wf == 4 * d.w[3] && (long)((d.h[3] * d.w[3] + 255) / 256) * 256 < 65536;
}

static int ensure_work(kpd_plan* p, const Dims& d, int k, hipStream_t st) {
  if (p->have_work[k] && d.fits(p->dims[k])) return KPD_OK;
  // re-carving (a larger shape) rewrites and re-zeroes the buffers: let every
  // earlier use of this workspace, on whichever stream, finish first (rare)
  if (p->have_work[k]) HIP_TRY(hipDeviceSynchronize());
  Work w;
  const size_t need = carve(p, d, nullptr, w);
  if (need > p->ws_bytes[k]) {
    if (p->ws[k]) HIP_TRY(hipFree(p->ws[k]));
    p->ws[k] = nullptr;
    HIP_TRY(hipMalloc(&p->ws[k], need));
    p->ws_bytes[k] = need;
  }
  carve(p, d, reinterpret_cast<char*>(p->ws[k]), p->work[k]);
  p->work[k].sc_dirty = true;
  ++p->ws_epoch;   // captured graphs hold the old carve's addresses
  // zero once: the padded heatmap-conv maps keep their zero border (the
  // kernels write interiors only)
  if (hm_padded(p)) HIP_TRY(hipMemsetAsync(p->ws[k], 0, need, st));
  p->dims[k] = d;
  p->have_work[k] = true;
  return KPD_OK;
}

// HeatmapHead (heatmap_head.py:81-151) on the [R][56][56][64] NHWC ROI
// features in w.roi with their per-row statistics in w.roi_stats: channel
// attention, spatial attention, the three 3x3 convs and the final 1x1 +
// sigmoid, heatmaps written at the ROIs' slots (w.slot, P).  parts selects
// the stages (KPD_HEAD_*; a disabled attention uses weights 1); sw_out
// (nullable) receives the spatial weights [R][56][56].
static int run_heatmap_head(const Pass& ps, int R, int P, float* heat_out, int parts, float* sw_out,
                            unsigned long long* stamps2, unsigned long long* stamps3,
                            unsigned long long* stamps1 = nullptr, int abs_in = 0) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const hipStream_t st = ps.st;
  std::unique_ptr<Stage> att_stage(new Stage(p, "hm_attention", st));
  // split: per-ROI operand bounds, hsc[r] = {max|xs| (written here), max|h1| (conv 1)}
  const bool hsplit = p->precision == KPD_PRECISION_SPLIT;
  HIP_TRY(launch_hm_chattn(w.roi_stats, R, p->hca_w0, p->hca_b0, p->hca_w2, p->hca_b2, w.cw,
                           hsplit ? w.hsc : nullptr, st, abs_in));
  if (!(parts & KPD_HEAD_CHANNEL_ATT)) HIP_TRY(launch_fill(w.cw, (long)R * 64, 1.f, st));
  const bool bf = p->precision == KPD_PRECISION_MIXED;
  const int xs_mode = hsplit ? 3 : bf ? (hm_padded(p) ? 2 : 1) : 0;
  static const bool att_2k = kpd_diag_env("KPD_HM_ATT_2K") != nullptr;   // A/B: pool and apply as two launches
  kpd_path(att_2k ? KP_HM_ATTN_2K : KP_HM_ATTN);
  if (att_2k) {
    HIP_TRY(launch_hm_spool(w.roi, w.cw, R, w.smap, st));
    HIP_TRY(launch_hm_sapply(w.roi, w.cw, w.smap, p->sa_w, p->sa_b, R, w.xs, xs_mode, st, w.hsc,
                             (parts & KPD_HEAD_SPATIAL_ATT) != 0, sw_out));
  } else {
    HIP_TRY(launch_hm_attn(w.roi, w.cw, p->sa_w, p->sa_b, R, w.xs, xs_mode, st, w.hsc,
                           (parts & KPD_HEAD_SPATIAL_ATT) != 0, sw_out));
  }
  att_stage.reset();
  if (!(parts & KPD_HEAD_CONVS)) return KPD_OK;
  // bounds: |xs| <= U0; |h1| <= bc1 + bs1 U0; |h2| <= bc2 + bs2 max|h1| (the
  // exponent each producer scales by and its consumer unscales by)
  const HmSplit sp1{w.hsc, 0.f, 1.f, 0, p->hm1.bc, p->hm1.bs, 0, 1};
  const HmSplit sp2{w.hsc, p->hm1.bc, p->hm1.bs, 0, p->hm2.bc, p->hm2.bs, 1, -1};
  const HmSplit sp3{w.hsc, p->hm2.bc, p->hm2.bs, 1, 0.f, 0.f, -1, -1};
  std::unique_ptr<Stage> c1(new Stage(p, "hm_conv1", st));
  if (int rc = hm_conv(ps, p->hm1, w.xs, R, 64, w.h1, 1, nullptr, stamps1, &sp1)) return rc;
  c1.reset();
  std::unique_ptr<Stage> c2(new Stage(p, "hm_conv2", st));
  if (int rc = hm_conv(ps, p->hm2, w.h1, R, p->hm1.cout_p, w.h2, 1, nullptr, stamps2, &sp2)) return rc;
  c2.reset();
  std::unique_ptr<Stage> c3(new Stage(p, "hm_conv3", st));
  // mixed / split: the final 1x1 + sigmoid runs in conv 3's epilogue (no h3 round trip)
  static const bool no_fin_fuse = kpd_diag_env("KPD_NO_FINAL_FUSE") != nullptr;   // A/B switch
  const bool fin_fused = (p->hm3.bf16 || p->hm3.ws) && p->hm3.cout_p == 64 && (!no_fin_fuse || p->hm3.ws);
  const HmFinal fin{p->fin_w, p->fin_b, w.slot, P, heat_out};
  if (int rc = hm_conv(ps, p->hm3, w.h2, R, p->hm2.cout_p, w.h3, 2, fin_fused ? &fin : nullptr, stamps3, &sp3))
    return rc;
  c3.reset();
  kpd_path(fin_fused ? KP_HM_FINAL_FUSED : KP_HM_FINAL);
  if (!fin_fused) HIP_TRY(launch_hm_final(w.h3, R, p->fin_w, p->fin_b, w.slot, P, heat_out, st));
  return KPD_OK;
}

// KEYPOINT_HEAD's convs as fp32-accurate split products on zero-bordered maps
// (hmconv_kernel MODE 2):
// [ResidualBlock 1 (+ downsample as a tenth tap) | visibility conv] ->
// ResidualBlock 2 (+ downsample) -> regression 3x3; ReLU6 bounds every
// intermediate by 6, the input by the FPN level-0 maximum.  The spatial
// attention (1x1 convs + sigmoid + apply) is one kernel writing the first
// conv's operand (KPD_KH_ATT1=1: the fp32 1x1 conv + apply kernel, A/B).
static int kh_convs_split(const Pass& ps, int R, const float* bound, int bdiv, int bstride, bool x_ready,
                          unsigned long long* const* stamps) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const hipStream_t st = ps.st;
  static const bool att1 = kpd_diag_env("KPD_KH_ATT1") != nullptr;
  if (x_ready) {
    kpd_path(KP_KH_SPLIT_XREADY);   // (roi_kh_kernel)
  } else if (att1 || !p->kh_sa1.ws) {
    kpd_path(KP_KH_SPLIT_ATT1);
    if (int rc = conv(ps, p->kh_sa1, w.kx, R, 56, 56, 128, w.ksa, ACT_RELU6)) return rc;
    HIP_TRY(launch_kh_att_split(w.kx, w.ksa, p->kh_sa2_w, p->kh_sa2_b, R, bound, bdiv, bstride, w.hsc, w.kxs, st));
  } else {
    kpd_path(KP_KH_SPLIT_ATT2);
    HIP_TRY(launch_kh_att2(w.kx, p->kh_sa1.ws, p->kh_sa1.w_exp, p->kh_sa1.b, p->kh_sa2_w, p->kh_sa2_b, R, bound,
                           bdiv, bstride, w.hsc, w.kxs, st));
  }
  const void* ins[3] = {w.kxs, w.kr1s, w.kr2s};
  void* outs[3] = {w.kr1s, w.kr2s, nullptr};
  float* outf[3] = {w.kv1, nullptr, w.kr3};
  for (int i = 0; i < 3; ++i) {
    const KhSplit& k = p->kh_s[i];
    HmConvArgs h{};
    h.in = ins[i]; h.wt = k.ws; h.bias = k.b; h.out = outs[i]; h.outf = outf[i];
    h.R = R; h.cin = k.cin; h.cout = k.cout; h.ntap = k.ntap; h.ns = k.ns; h.nf = k.nf;
    h.kh_ps = k.ps; h.kh_pt = k.pt; h.kh_bd = k.ntap == 10 ? k.bd : nullptr;
    h.split = 1; h.hsc = w.hsc; h.w_exp = k.w_exp;
    h.in_c = i == 0 ? 0.f : 6.f; h.in_s = i == 0 ? 1.f : 0.f; h.in_idx = 2;
    h.out_c = 6.f; h.out_s = 0.f; h.out_idx = k.ns > 0 ? 2 : -1; h.amax_idx = -1;
    h.stamps = stamps ? stamps[i] : nullptr;   // (KPD_STAMPS, diagnostic build)
    HIP_TRY(launch_hmconv(h, st));
  }
  return KPD_OK;
}

// KEYPOINT_HEAD's convs on the generic fp32 conv
static int kh_convs_fp32(const Pass& ps, int R) {
  kpd_plan* p = ps.p; Work& w = *ps.w;
  kpd_path(KP_KH_FP32);
  if (int rc = conv(ps, p->kh_sa1, w.kx, R, 56, 56, 128, w.ksa, ACT_RELU6)) return rc;
  HIP_TRY(launch_kh_att(w.kx, w.ksa, p->kh_sa2_w, p->kh_sa2_b, (size_t)R * 3136, ps.st));
  // ResidualBlock(128 -> 64): relu6(relu6(bn1(relu6(conv_bn(x)))) + downsample(x))
  const float* id1 = w.kx;
  if (p->kh_ds1.w) {
    if (int rc = conv(ps, p->kh_ds1, w.kx, R, 56, 56, 128, w.kds1, ACT_NONE)) return rc;
    id1 = w.kds1;
  }
  if (int rc = conv_post(ps, p->kh_rb1, w.kx, R, 56, 56, 128, w.krb1, ACT_RELU6, p->kh_bn1a_s, p->kh_bn1a_t,
                         ACT_RELU6, id1, ACT_RELU6))
    return rc;
  const float* id2 = w.krb1;
  if (p->kh_ds2.w) {
    if (int rc = conv(ps, p->kh_ds2, w.krb1, R, 56, 56, p->kh_rb1.cout_p, w.kds2, ACT_NONE)) return rc;
    id2 = w.kds2;
  }
  if (int rc = conv_post(ps, p->kh_rb2, w.krb1, R, 56, 56, p->kh_rb1.cout_p, w.krb2, ACT_RELU6, p->kh_bn1b_s,
                         p->kh_bn1b_t, ACT_RELU6, id2, ACT_RELU6))
    return rc;
  if (int rc = conv(ps, p->kh_c3, w.krb2, R, 56, 56, p->kh_rb2.cout_p, w.kr3, ACT_RELU6)) return rc;
  return conv(ps, p->kh_v1, w.kx, R, 56, 56, 128, w.kv1, ACT_RELU6);
}

// KEYPOINT_HEAD (keypoint_head.py:50-62, ResidualBlock :64-90) on the
// [R][56][56][128] NHWC ROI features in w.kx; outputs at the ROIs' slots.
// bound (split path): the bound of |x| for ROI r is bound[(r / bdiv) * bstride]
// x_ready: the first conv's split operand (x * attention) is already in
// w.kxs (roi_kh_kernel wrote it with the HeatmapHead's ROI align).
static int run_keypoint_head(const Pass& ps, int R, int P, float* kh_kpts, float* kh_vis, const float* bound,
                             int bdiv, int bstride, bool x_ready = false,
                             unsigned long long* const* stamps = nullptr) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const hipStream_t st = ps.st;
  if (int rc = p->kh_split && w.kxs ? kh_convs_split(ps, R, bound, bdiv, bstride, x_ready, stamps)
                                    : kh_convs_fp32(ps, R))
    return rc;
  const int o = p->kh_o, kr = pad16(16 * o * o);
  if (kr != 16 * o * o) HIP_TRY(hipMemsetAsync(w.kpr, 0, sizeof(float) * R * kr, st));
  HIP_TRY(launch_kh_pool(w.kr3, R, 16, o, w.kpr, kr, st));
  HIP_TRY(launch_kh_pool(w.kv1, R, 32, 4, w.kpv, 512, st));
  // the two Linear layers as 1x1 MFMA GEMMs over all ROIs (M = R)
  if (int rc = conv(ps, p->kh_lr, w.kpr, R, 1, 1, kr, w.klr, ACT_NONE)) return rc;
  if (int rc = conv(ps, p->kh_lv, w.kpv, R, 1, 1, 512, w.klv, ACT_NONE)) return rc;
  HIP_TRY(launch_kh_final(w.klr, p->kh_lr.cout_p, w.klv, p->kh_lv.cout_p, p->kh_lnr_g, p->kh_lnr_b, p->kh_fr_w,
                          p->kh_fr_b, p->kh_lnv_g, p->kh_lnv_b, p->kh_fv_w, p->kh_fv_b, w.slot, R, P, kh_kpts,
                          kh_vis, st));
  return KPD_OK;
}

// ---------------------------------------------------------------- forward schedule
// One forward's arguments, as kpd_forward receives them.
struct FwdArgs {
  const float* image;
  int B, C, H, W;
  float* boxes;
  int NB, P, flags;
  float *kpts, *vis, *heat, *kh_kpts, *kh_vis, *box_scores;
  int32_t* topk_out;
  bool detect() const { return flags & KPD_FLAG_DETECT; }
  bool dual() const { return flags & KPD_FLAG_DUAL_HEAD; }
  // given boxes for every image: the slot map rides along with the top-k launch
  bool slot_in_topk() const { return !detect() && NB == B && NB * P > 0 && boxes != nullptr; }
  // the view of images [c0, c1): every pointer at image c0, the boxes of that range
  FwdArgs images(int c0, int c1) const {
    const size_t per_kp = (size_t)P * 17;
    auto off = [c0](auto* ptr, size_t per) { return ptr ? ptr + (size_t)c0 * per : ptr; };
    FwdArgs s = *this;
    s.image = image + (size_t)c0 * C * H * W;
    s.B = c1 - c0;
    s.NB = std::max(0, std::min(NB, c1) - c0);
    s.boxes = s.NB > 0 || detect() ? off(boxes, (size_t)P * 4) : nullptr;
    s.kpts = off(kpts, per_kp * 2); s.vis = off(vis, per_kp * 3); s.heat = off(heat, per_kp * 3136);
    s.kh_kpts = off(kh_kpts, per_kp * 2); s.kh_vis = off(kh_vis, per_kp * 3);
    s.box_scores = off(box_scores, (size_t)P);
    s.topk_out = off(topk_out, 64);
    return s;
  }
};

// Level sizes of an H x W image: after the stem (0) and after bneck i (i + 1);
// FPN level 0 has the stem's
static Dims level_dims(int H, int W) {
  Dims d;
  d.H = H; d.W = W;
  d.h[0] = (H - 1) / 2 + 1; d.w[0] = (W - 1) / 2 + 1;
  for (int i = 0; i < 11; ++i) {
    const int k = kBneck[i].k, s = kBneck[i].s, pd = (k - 1) / 2;
    d.h[i + 1] = (d.h[i] + 2 * pd - k) / s + 1;
    d.w[i + 1] = (d.w[i] + 2 * pd - k) / s + 1;
  }
  d.Hf = d.h[0]; d.Wf = d.w[0];
  return d;
}

// Geometry, level-0 mode and workspace k of one pass of B images on stream st
static int begin_pass(Pass& ps, kpd_plan* p, int k, bool debug, int B, int H, int W, int NB, int P, int flags,
                      hipStream_t st) {
  ps.p = p; ps.st = st; ps.debug = debug;
  Dims& d = ps.d;
  d = level_dims(H, W);
  d.B = B; d.NB = NB; d.P = P; d.flags = flags & ~KPD_FLAG_FULL_LEVEL0;   // (no workspace effect)
  const int HWf = d.Hf * d.Wf;
  // split (fp32-accurate f16 hi + lo) FPN level 0 by linearity: when lateral 1
  // is an exact 4x nearest upsample of the level-0 grid (kpd_forward caps the
  // pass at max_pass_images, which keeps the 31-bit buffer extents); other
  // geometries run the fp32 level-0 conv
  ps.lin = fpn0x_ok(p, d) && B <= max_pass_images(H, W);
  const int TM = conv_tile_m();
  ps.tpc = (d.h[3] * d.w[3] + 255) / 256;
  d.fused_stats = ps.lin || (HWf % TM) == 0;
  d.tiles = ps.lin ? 16 * ps.tpc : (d.fused_stats ? HWf / TM : std::min(64, HWf));
  if (int rc = ensure_work(p, d, k, st)) return rc;
  ps.w = &p->work[k];
  ps.splitk = ps.w->splitk;
  if (want_stamps() && !p->stamps) {
    HIP_TRY(hipMalloc(&p->stamps, kStampWords * 8));
    p->allocs.push_back(p->stamps);
  }
  return KPD_OK;
}

// -------- MobileNet block paths.  Each tests its own eligibility on block
// b.i, fills its arguments, logs its token, launches, and returns the number
// of blocks it computed (output in w.o[b.i + that - 1]); 0: not eligible,
// nothing launched; negative: an error code.  stage_body tries them in the
// order they stand here.
struct Blk {
  const DevBneck& bn;
  int i, hi, wi, ho, wo, inp;   // block index, input / output map, input channels padded to 16
  const float* x;               // input
};

static bool no_fuse() {
  static const bool v = kpd_diag_env("KPD_NO_FUSE") != nullptr;   // A/B switch for measurements
  return v;
}

// features.1: 16 channels, no expand, SE -> depthwise + tile sums, excitation + project
static int block_dwsum(Pass& ps, const Blk& b) {
  const DevBneck& bn = b.bn; Work& w = *ps.w;
  const int B = ps.d.B, i = b.i, ho = b.ho, wo = b.wo;
  static const bool no_f1 = kpd_diag_env("KPD_NO_F1") != nullptr;   // A/B switch
  if (!(!no_f1 && !bn.has_exp && bn.cfg.se && bn.dw.Cp == 16 && bn.cfg.cout == 16 && bn.project.cout_p == 16 &&
        bn.project.cin_p == 16 && bn.project.k == 1 && !bn.project.bf16 && bn.se.sq <= 16 &&
        dwsum_has(bn.dw.k, bn.dw.s, bn.dw.act) && 4 * ((wo + 3) / 4) * 4 <= 256))
    return 0;
  int nt = 0;
  kpd_path(KP_F1_DWSUM);
  HIP_TRY(launch_dwsum(b.x, B, b.hi, b.wi, bn.dw.w, bn.dw.b, bn.dw.act, w.d[i], ho, wo, bn.dw.k, bn.dw.s, w.separt,
                       &nt, ps.st));
  HIP_TRY(launch_se16_proj(w.d[i], B, ho * wo, nt, w.separt, bn.se.w1, bn.se.b1, bn.se.w2, bn.se.b2, bn.se.sq,
                           static_cast<const float*>(bn.project.w), bn.project.b, w.o[i], ps.st));
  return 1;
}

// features.2 + features.3 (3x3 stride 2, then 3x3 stride 1 with the
// residual; no SE) in one launch: fir23.hip
static int block_fir23(Pass& ps, const Blk& b) {
  const DevBneck& bn = b.bn;
  const int i = b.i, ho = b.ho, wo = b.wo, inp = b.inp;
  static const bool no_fir23 = kpd_diag_env("KPD_NO_FIR23") != nullptr;   // A/B switch
  if (!(!no_fuse() && !no_fir23 && i + 1 < 11)) return 0;
  const DevBneck& b3 = ps.p->bn[i + 1];
  auto plain = [](const DevConv& c) { return c.k == 1 && !c.bf16; };
  const bool f23 = bn.has_exp && !bn.cfg.se && bn.dw.k == 3 && bn.dw.s == 2 && inp == 16 && plain(bn.expand) &&
                   plain(bn.project) && bn.expand.cin_p == 16 && bn.expand.cout_p == bn.dw.Cp &&
                   bn.project.cin_p == bn.dw.Cp && bn.project.cout_p == 32 && b3.has_exp && !b3.cfg.se &&
                   b3.dw.k == 3 && b3.dw.s == 1 && plain(b3.expand) && plain(b3.project) &&
                   b3.expand.cin_p == 32 && b3.expand.cout_p == b3.dw.Cp && b3.project.cin_p == b3.dw.Cp &&
                   b3.project.cout_p == 32 && b3.cfg.cin == b3.cfg.cout && bn.cfg.cout == b3.cfg.cin;
  Fir23Args fa{};
  fa.x = b.x; fa.H1 = b.hi; fa.W1 = b.wi;
  fa.we2 = static_cast<const float*>(bn.expand.w); fa.be2 = bn.expand.b; fa.wd2 = bn.dw.w; fa.bd2 = bn.dw.b;
  fa.wp2 = static_cast<const float*>(bn.project.w); fa.bp2 = bn.project.b;
  fa.we3 = static_cast<const float*>(b3.expand.w); fa.be3 = b3.expand.b; fa.wd3 = b3.dw.w; fa.bd3 = b3.dw.b;
  fa.wp3 = static_cast<const float*>(b3.project.w); fa.bp3 = b3.project.b;
  fa.E2 = bn.dw.Cp; fa.E3 = b3.dw.Cp;
  fa.act2e = bn.cfg.act; fa.act2d = bn.dw.act; fa.act3e = b3.cfg.act; fa.act3d = b3.dw.act;
  fa.out = ps.w->o[i + 1]; fa.H2 = ho; fa.W2 = wo;
  if (!(f23 && ps.d.h[i + 2] == ho && ps.d.w[i + 2] == wo && fir23_pick_rows(fa))) return 0;
  fa.stamps = ps.take_stamps("stamps_fir23_0", (size_t)((ho + fa.T - 1) / fa.T) * ps.d.B);
  kpd_path(KP_FIR23, fa.T);
  HIP_TRY(launch_fir23(fa, ps.d.B, ps.st));
  return 2;   // features.3 done too
}

// no SE: the whole block (expand, depthwise, project, residual) in one kernel on row tiles
// fused by default only at stride 2 (features.2: -31 us per step); the stride-1
// block (features.3) measured 6 us slower fused than as three kernels.
// KPD_FIR_MASK (bit i = block i) overrides for A/B runs.
static int block_fir(Pass& ps, const Blk& b) {
  const DevBneck& bn = b.bn;
  const int i = b.i, ho = b.ho;
  static const int fir_mask = kpd_diag_env("KPD_FIR_MASK") ? atoi(kpd_diag_env("KPD_FIR_MASK")) : -1;
  const bool fir_on = fir_mask < 0 ? bn.cfg.s == 2 : ((fir_mask >> i) & 1) != 0;
  if (!(!no_fuse() && fir_on && !bn.cfg.se && bn.has_exp && bn.expand.cout_p == bn.dw.Cp &&
        bn.project.cin_p == bn.dw.Cp))
    return 0;
  FirArgs fa{};
  fa.x = b.x; fa.Hi = b.hi; fa.Wi = b.wi; fa.cin_p = b.inp;
  fa.we = static_cast<const float*>(bn.expand.w); fa.be = bn.expand.b;
  fa.wd = bn.dw.w; fa.bd = bn.dw.b;
  fa.wp = static_cast<const float*>(bn.project.w); fa.bp = bn.project.b;
  fa.act_e = bn.cfg.act; fa.act_d = bn.dw.act; fa.Ep = bn.dw.Cp; fa.cout_p = bn.project.cout_p;
  fa.out = ps.w->o[i]; fa.Ho = ho; fa.Wo = b.wo;
  fa.res = bn.cfg.s == 1 && bn.cfg.cin == bn.cfg.cout;
  if (!fir_pick_rows(fa, bn.dw.k, bn.dw.s)) return 0;
  fa.stamps = ps.take_stamps("stamps_fir_" + std::to_string(i), (size_t)((ho + fa.TH - 1) / fa.TH) * ps.d.B);
  kpd_path(KP_FIR, fa.TH);
  HIP_TRY(launch_fir(fa, ps.d.B, bn.dw.k, bn.dw.s, ps.st));
  return 1;
}

// coarse maps: expand + depthwise (+ SE means) fused when the image fits LDS.
// Fills exdw_kernel's arguments (part: with the SE fc1 partials seproj_kernel
// reads); false: the block does not take the fused kernel
static bool exdw_fill(const Pass& ps, const Blk& b, ExDwArgs& xa, bool part = false) {
  const DevBneck& bn = b.bn; const Work& w = *ps.w;
  const int B = ps.d.B, i = b.i;
  xa.x = b.x; xa.Hi = b.hi; xa.Wi = b.wi; xa.cin_p = b.inp;
  xa.we = bn.has_exp ? static_cast<const float*>(bn.expand.w) : nullptr;
  xa.be = bn.has_exp ? bn.expand.b : nullptr;
  xa.act_e = bn.cfg.act; xa.wd = bn.dw.w; xa.bd = bn.dw.b; xa.act_d = bn.dw.act; xa.Ep = bn.dw.Cp;
  xa.out = w.d[i]; xa.Ho = b.ho; xa.Wo = b.wo; xa.pooled = bn.cfg.se ? w.pool : nullptr;
  if (part) { xa.part = w.separt; xa.w1 = bn.se.w1; xa.sq = bn.se.sq; xa.C = bn.se.C; }
  if (!(!no_fuse() && b.hi * b.wi <= kFuseMaxPix && bn.has_exp && bn.expand.cout_p == bn.dw.Cp && b.inp <= 96))
    return false;
  // slice width fixed per layer (never per batch: the fc1 partial sums
  // must not depend on what an image is batched with): 32 channels from 288
  // expanded channels up, else 16
  xa.CS = bn.dw.Cp >= 288 ? 32 : 16;
  // no SE and under two workgroups per CU: split the output rows in two
  // bands (features.3 at 64 images: 384 -> 768 workgroups)
  static const int nband_env = kpd_diag_env("KPD_EXDW_NBAND") ? atoi(kpd_diag_env("KPD_EXDW_NBAND")) : 0;   // A/B
  xa.nband = !bn.cfg.se && (long)(bn.dw.Cp / xa.CS) * B < 512 ? 2 : 1;
  if (nband_env > 0 && !bn.cfg.se) xa.nband = std::min(nband_env, b.ho);
  return bn.dw.Cp % xa.CS == 0 && exdw_pick(xa, bn.dw.k, bn.dw.s) >= 0;
}

static int launch_exdw_block(Pass& ps, const Blk& b, ExDwArgs& xa) {
  const DevBneck& bn = b.bn;
  xa.stamps = ps.take_stamps("stamps_exdw_" + std::to_string(b.i),
                             (size_t)(bn.dw.Cp / xa.CS) * ps.d.B * std::max(1, xa.nband));
  HIP_TRY(launch_exdw(xa, ps.d.B, bn.dw.k, bn.dw.s, ps.st));
  return KPD_OK;
}

// SE blocks on the coarse maps: fc1 partials in exdw_kernel, then the
// excitation + project (+ residual) in one seproj_kernel launch
static int block_exdw_seproj(Pass& ps, const Blk& b) {
  const DevBneck& bn = b.bn; Work& w = *ps.w;
  const int B = ps.d.B, i = b.i, ho = b.ho, wo = b.wo;
  static const bool no_seproj = kpd_diag_env("KPD_NO_SEPROJ") != nullptr;   // A/B switch
  if (!(bn.cfg.se && !no_seproj && bn.project.k == 1 && !bn.project.bf16 && bn.project.cin_p == bn.dw.Cp &&
        bn.se.sq <= 144 && bn.se.C % 4 == 0 && (ho * wo == 48 || ho * wo == 192)))
    return 0;
  ExDwArgs xa{};
  if (!exdw_fill(ps, b, xa, true) || (size_t)(bn.dw.Cp / xa.CS) * bn.se.sq > kSePartFloats) return 0;
  SeProjArgs sa{};
  sa.d = w.d[i]; sa.Po = ho * wo; sa.Ep = bn.dw.Cp;
  sa.part = w.separt; sa.nsl = bn.dw.Cp / xa.CS; sa.sq = bn.se.sq; sa.C = bn.se.C;
  sa.b1 = bn.se.b1; sa.w2t = bn.se.w2; sa.b2 = bn.se.b2;
  sa.wp = static_cast<const float*>(bn.project.w); sa.bp = bn.project.b; sa.cout_p = bn.project.cout_p;
  // 192-pixel maps: all 48 output channels per workgroup and the rows in
  // four (seproj_pick), so an image's excitation is recomputed by 4
  // workgroups instead of 6 (its fc2 weight columns are most of a
  // workgroup's L2 reads): body -8..-12 us at C2 (same-box A/B)
  sa.NT = sa.Po == 48 ? 32 : 48;
  if (sa.cout_p % sa.NT) sa.NT = 16;
  const SeProjPick pick = seproj_pick(sa, B);
  if (pick.v < 0) return 0;
  kpd_path(ho * wo == 48 ? KP_EXDW_SEPROJ48 : KP_EXDW_SEPROJ192);
  if (int rc = launch_exdw_block(ps, b, xa)) return rc;
  const bool res = bn.cfg.s == 1 && bn.cfg.cin == bn.cfg.cout;
  sa.res = res ? b.x : nullptr;
  sa.out = w.o[i];
  // wide blocks (C >= 288): the excitation as its own launch (one fc2
  // pass per image instead of one per project workgroup)
  static const int se_split_env = kpd_diag_env("KPD_SE_SPLIT") ? atoi(kpd_diag_env("KPD_SE_SPLIT")) : -1;   // A/B
  if (se_split_env == 1 || (se_split_env < 0 && bn.se.C >= 288)) {
    kpd_path(KP_SE_EXCITE);
    HIP_TRY(launch_se_excite(sa, B, w.sesc[i], ps.st));
    sa.sesc = w.sesc[i];
  }
  sa.stamps = ps.take_stamps("stamps_seproj_" + std::to_string(i), (size_t)pick.grid.x * pick.grid.y * pick.grid.z);
  HIP_TRY(launch_seproj(sa, B, ps.st));
  return 1;
}

// the tail the last two paths share: se_kernel (SE blocks; the channel means
// from exdw_kernel's pool when it ran) and the project conv (+ residual)
static int se_project(Pass& ps, const Blk& b, bool fused) {
  const DevBneck& bn = b.bn; Work& w = *ps.w;
  const int B = ps.d.B, i = b.i, ho = b.ho, wo = b.wo;
  if (bn.cfg.se)
    HIP_TRY(launch_se(w.d[i], B, ho * wo, bn.se.C, bn.se.Cp, bn.se.w1, bn.se.b1, bn.se.w2, bn.se.b2, bn.se.sq,
                      w.sesc[i], ps.st, fused ? w.pool : nullptr));
  const bool res = bn.cfg.s == 1 && bn.cfg.cin == bn.cfg.cout;
  ConvOpt o;
  o.res = res ? b.x : nullptr; o.rh = ho; o.rw = wo;
  o.a_scale = bn.cfg.se ? w.sesc[i] : nullptr;
  return conv(ps, bn.project, w.d[i], B, ho, wo, bn.dw.Cp, w.o[i], ACT_NONE, o);
}

// the fused expand + depthwise, then se_kernel and the project conv
static int block_exdw_se(Pass& ps, const Blk& b) {
  ExDwArgs xa{};
  if (!exdw_fill(ps, b, xa)) return 0;
  kpd_path(b.bn.cfg.se ? KP_EXDW_SE : KP_EXDW_PLAIN);
  if (int rc = launch_exdw_block(ps, b, xa)) return rc;
  if (int rc = se_project(ps, b, true)) return rc;
  return 1;
}

// the generic three launches: expand conv, depthwise, (se_kernel,) project conv
static int block_generic(Pass& ps, const Blk& b) {
  const DevBneck& bn = b.bn; Work& w = *ps.w;
  const int B = ps.d.B, i = b.i;
  const float* e = b.x;
  kpd_path(bn.cfg.se ? KP_GENERIC_SE : KP_GENERIC);
  if (bn.has_exp) {
    if (int rc = conv(ps, bn.expand, b.x, B, b.hi, b.wi, b.inp, w.e[i], bn.cfg.act)) return rc;
    e = w.e[i];
  }
  HIP_TRY(launch_dwconv(e, bn.dw.w, bn.dw.b, w.d[i], B, b.hi, b.wi, bn.dw.Cp, b.ho, b.wo, bn.dw.k, bn.dw.s, bn.dw.act,
                        ps.st));
  if (int rc = se_project(ps, b, false)) return rc;
  return 1;
}

// -------- stages of a pass, in the order forward_one runs them

// MobileNetV3-Small body: the stem and features.1-12; taps = the four FPN
// inputs (NHWC, channels padded to 16), left in the workspace
static int stage_body(Pass& ps, const float* image, int C, const float* taps[4]) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  const Stage stage(p, "body", ps.st);
  if (ps.lin && w.sc_dirty) HIP_TRY(hipMemsetAsync(w.sc, 0, (size_t)2 * d.B * kAmaxStride * sizeof(float), ps.st));
  if (ps.lin) w.sc_dirty = true;   // until this forward's topk_kernel zeroes the slots it used
  HIP_TRY(launch_stem(image, d.B, C, d.H, d.W, p->stem_w, p->stem_b, w.stem, d.h[0], d.w[0], ps.lin ? w.sc : nullptr,
                      ps.st));
  using BlockPath = int (*)(Pass&, const Blk&);
  static const BlockPath kPaths[] = {block_dwsum,       block_fir23,   block_fir,
                                     block_exdw_seproj, block_exdw_se, block_generic};
  const float* x = w.stem;
  taps[0] = w.stem;
  for (int i = 0; i < 11; ++i) {
    kpd_path_at(KP_BLOCK, i + 1);
    const Blk b{p->bn[i], i, d.h[i], d.w[i], d.h[i + 1], d.w[i + 1], pad16(p->bn[i].cfg.cin), x};
    int used = 0;
    for (BlockPath path : kPaths)
      if ((used = path(ps, b)) != 0) break;
    if (used < 0) return used;
    i += used - 1;
    x = w.o[i];
    if (i + 1 == 3) taps[1] = x;
    if (i + 1 == 8) taps[2] = x;
  }
  kpd_path_at(KP_LAST);
  if (int rc = conv(ps, p->last, x, d.B, d.h[11], d.w[11], pad16(96), w.last, ACT_HSWISH)) return rc;
  kpd_path_at(KP_TOP);
  taps[3] = w.last;
  return KPD_OK;
}

// lateral_chain_kernel's arguments: laterals 3 -> 1 (and the split rows of
// lateral 1 and tap 0 that fpn0x_kernel reads) in one launch
static void lateral_chain_fill(Pass& ps, const float* const taps[4], LatChainArgs& lc) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  const int B = d.B;
  lc.t1 = taps[1]; lc.t2 = taps[2]; lc.t3 = taps[3];
  lc.L1 = static_cast<const float*>(p->lat[1].w); lc.L2 = static_cast<const float*>(p->lat[2].w);
  lc.L3 = static_cast<const float*>(p->lat[3].w);
  lc.c1 = pad16(kFpnIn[1]); lc.c2 = pad16(kFpnIn[2]); lc.c3 = pad16(kFpnIn[3]);
  lc.c1r = kFpnIn[1]; lc.c2r = kFpnIn[2]; lc.c3r = kFpnIn[3];
  lc.S1 = p->lat_S[1]; lc.S2 = p->lat_S[2]; lc.S3 = p->lat_S[3];
  lc.w_exp0 = p->fpn0x.w_exp0; lc.w_expE = p->fpn0x.w_expE;
  lc.h1 = d.h[3]; lc.w1 = d.w[3]; lc.h2 = d.h[8]; lc.w2 = d.w[8]; lc.h3 = d.h[11]; lc.w3 = d.w[11];
  lc.lat1 = w.lat[1];
  // split: lateral 1 goes straight to the hi|lo rows fpn0x_kernel reads (after the tap0 rows)
  lc.lat1_split = ps.lin ? reinterpret_cast<_Float16*>(reinterpret_cast<char*>(w.lat[0]) + (size_t)B * d.h[0] * d.w[0] * 64)
                         : nullptr;
  lc.amax = ps.lin ? w.sc : nullptr;
  static const bool no_chain_t0 = kpd_diag_env("KPD_NO_CHAIN_TAP0") != nullptr;   // A/B: tap0 split as its own launch
  if (ps.lin && !no_chain_t0) {
    lc.t0 = taps[0];
    lc.t0_split = reinterpret_cast<_Float16*>(w.lat[0]);
    lc.P0 = d.h[0] * d.w[0];
  }
  lc.stamps = ps.take_stamps("stamps_latchain_0", (size_t)8 * ((B + 7) / 8 * 8));
}

// level 0 by linearity has no lateral 0: tap0 and lateral 1 go to the split
// layouts fpn0x_kernel reads, unless the chain launch wrote them
static int lateral0_split_rows(Pass& ps, const float* const taps[4], bool chain, bool chain_t0) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  char* base = reinterpret_cast<char*>(w.lat[0]);
  if (!chain || !chain_t0) {
    kpd_path(KP_SPLIT_ROWS);
    HIP_TRY(launch_split_rows(taps[0], d.B, (long)d.h[0] * d.w[0], 16, w.sc, 0, p->fpn0x.w_exp0, p->fpn0x.w_expE, base,
                              ps.st));
  }
  if (!chain) {
    kpd_path_at(KP_LAT, 1);
    kpd_path(KP_SPLIT_ROWS);
    HIP_TRY(launch_split_rows(w.lat[1], d.B, (long)d.h[3] * d.w[3], 128, w.sc, 1, p->fpn0x.w_exp0, p->fpn0x.w_expE,
                              base + (size_t)d.B * d.h[0] * d.w[0] * 64, ps.st));
  }
  return KPD_OK;
}

// FPN laterals, top-down.  keep_all: every lateral level is an output
// (kpd_backbone), so the per-level convs run; otherwise laterals 3 -> 1 go in
// one launch (lateral_chain.hip) where it applies, as only lateral 1 is consumed
static int stage_laterals(Pass& ps, const float* const taps[4], bool keep_all) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  const int B = d.B;
  const int lh[4] = {d.h[0], d.h[3], d.h[8], d.h[11]}, lw[4] = {d.w[0], d.w[3], d.w[8], d.w[11]};
  const Stage stage(p, "fpn_lateral", ps.st);
  static const bool no_chain = kpd_diag_env("KPD_NO_LAT_CHAIN") != nullptr;   // A/B switch
  LatChainArgs lc{};
  lateral_chain_fill(ps, taps, lc);
  const bool chain = !no_chain && !keep_all && !p->lat[1].bf16 && !p->lat[2].bf16 && !p->lat[3].bf16 &&
                     p->lat[1].cin_p == lc.c1 && p->lat[2].cin_p == lc.c2 && p->lat[3].cin_p == lc.c3 &&
                     p->lat[1].cout_p == 128 && p->lat[2].cout_p == 128 && p->lat[3].cout_p == 128 &&
                     lateral_chain_ok(lc);
  kpd_path(chain ? KP_LAT_CHAIN : KP_LAT_PER_LEVEL);
  if (chain) HIP_TRY(launch_lateral_chain(lc, B, ps.st));
  for (int i = 3; i >= 0; --i) {
    if (chain && i > 0) continue;
    const DevConv& L = p->lat[i];
    kpd_path_at(KP_LAT, i);
    ConvOpt o;
    o.res = i < 3 ? w.lat[i + 1] : nullptr; o.rh = i < 3 ? lh[i + 1] : 0; o.rw = i < 3 ? lw[i + 1] : 0;
    o.amax = (i == 1 && ps.lin) ? w.sc + (size_t)B * kAmaxStride : nullptr;
    if (i == 0 && ps.lin) {
      if (int rc = lateral0_split_rows(ps, taps, chain, lc.t0 != nullptr)) return rc;
    } else if (i == 0 && L.cin_p <= 32) {   // the 16-channel stem tap: a 403 MB/step stream, not a GEMM
      kpd_path(KP_LATERAL_STREAM);
      HIP_TRY(launch_lateral_stream(taps[0], L.cin_p, (const float*)L.w, L.b, o.res, B, lh[0], lw[0], lh[1], lw[1],
                                    w.lat[0], ps.st));
    } else if (int rc = conv(ps, L, taps[i], B, lh[i], lw[i], pad16(kFpnIn[i]), w.lat[i], ACT_NONE, o)) {
      return rc;
    }
  }
  kpd_path_at(KP_TOP);
  return KPD_OK;
}

// caller boxes: level 0 is stored only where the ROI aligns read it (the
// 400 MB fp32 map per 64 images otherwise; KPD_FLAG_FULL_LEVEL0 stores all)
static bool level0_footprint(const Pass& ps, const FwdArgs& a) {
  return ps.lin && !a.detect() && a.boxes && a.NB * a.P > 0 && !(a.flags & KPD_FLAG_FULL_LEVEL0) && ps.p->has_ca;
}

// FPN level 0 by linearity (fpn0x_kernel); fp: store the footprint of its boxes only
static int level0_fpn0x(Pass& ps, const FwdArgs* fp) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  const int B = d.B;
  Fpn0xArgs a{};
  char* base = reinterpret_cast<char*>(w.lat[0]);
  a.f_split = base;
  a.l_split = base + (size_t)B * d.h[0] * d.w[0] * 64;
  a.w0 = p->fpn0x.w0; a.weff = p->fpn0x.weff;
  for (int c = 0; c < 16; ++c) {
    a.cls_woff[c] = p->fpn0x.cls_woff[c];
    a.cls_ng[c] = p->fpn0x.cls_ng[c];
    for (int g = 0; g < kFpn0xMaxGroups; ++g) a.cls_g[c][g] = p->fpn0x.cls_g[c][g];
  }
  a.bias = p->fpn0.b; a.out = w.feat; a.stats = w.stats; a.sc = w.sc; a.sc_n = B;
  a.N = B; a.Hf = d.Hf; a.Wf = d.Wf; a.rh = d.h[3]; a.rw = d.w[3]; a.tpc = ps.tpc;
  a.w_exp0 = p->fpn0x.w_exp0; a.w_expE = p->fpn0x.w_expE;
  a.f_bytes = (int)std::min<size_t>((size_t)B * d.h[0] * d.w[0] * 64, 0x7fffffff);
  a.l_bytes = (int)std::min<size_t>((size_t)B * d.h[3] * d.w[3] * 512, 0x7fffffff);
  a.w0_bytes = p->fpn0x.w0_bytes; a.weff_bytes = p->fpn0x.weff_bytes;
  a.stamps = ps.take_stamps("stamps_fpn0x", (size_t)16 * B * ps.tpc);
  if (fp) {
    a.fp_boxes = fp->boxes; a.fp_NB = fp->NB; a.fp_P = fp->P;
  }
  kpd_path(KP_L0_FPN0X, ps.tpc);
  HIP_TRY(launch_fpn0x(a, ps.st));
  return KPD_OK;
}

// FPN level 0 (fpn_convs.0 on lateral 0) with the channel statistics top-k reads
static int stage_level0(Pass& ps, const FwdArgs* footprint) {
  Work& w = *ps.w; const Dims& d = ps.d;
  const Stage stage(ps.p, "fpn0", ps.st);
  if (ps.lin) return level0_fpn0x(ps, footprint);
  kpd_path(d.fused_stats ? KP_L0_CONV_STATS : KP_L0_CONV);
  kpd_path_at(KP_FPN0);
  ConvOpt o;
  o.stats = d.fused_stats ? w.stats : nullptr; o.tiles = d.tiles;
  if (int rc = conv(ps, ps.p->fpn0, w.lat[0], d.B, d.Hf, d.Wf, 128, w.feat, ACT_RELU, o)) return rc;
  kpd_path_at(KP_TOP);
  return KPD_OK;
}

// channel attention scores and the top-64 channels of level 0
static int stage_topk(Pass& ps, const FwdArgs& a) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  const int B = d.B, HWf = d.Hf * d.Wf;
  const Stage stage(p, "topk", ps.st);
  if (!d.fused_stats) {
    kpd_path(KP_CHANNEL_STATS);
    HIP_TRY(launch_channel_stats(w.feat, B, HWf, 128, d.tiles, w.stats, ps.st));
  }
  const bool slot_in_topk = a.slot_in_topk();
  if (slot_in_topk) kpd_path(KP_TOPK_SLOTMAP);
  HIP_TRY(launch_topk(w.stats, B, d.tiles, HWf, p->ca_w0, p->ca_b0, p->ca_w2, p->ca_b2, w.topk, w.scores, ps.st,
                      slot_in_topk ? a.boxes : nullptr, a.P, slot_in_topk ? w.slot : nullptr, w.imax,
                      ps.lin ? w.sc : nullptr, B));
  if (ps.lin) w.sc_dirty = false;
  return KPD_OK;
}

// the caller's top-k copy and the debug buffers of the backbone
static int publish_backbone(Pass& ps, const FwdArgs& a, const float* const taps[4]) {
  Work& w = *ps.w; const Dims& d = ps.d;
  const size_t B = d.B;
  if (a.topk_out) HIP_TRY(hipMemcpyAsync(a.topk_out, w.topk, sizeof(int32_t) * B * 64, hipMemcpyDeviceToDevice, ps.st));
  if (!level0_footprint(ps, a)) ps.dbg["feat0"] = {w.feat, sizeof(float) * B * d.Hf * d.Wf * 128};
  ps.dbg["scores"] = {w.scores, sizeof(float) * B * 128};
  ps.dbg["tap0"] = {taps[0], sizeof(float) * B * d.h[0] * d.w[0] * 16};
  ps.dbg["tap1"] = {taps[1], sizeof(float) * B * d.h[3] * d.w[3] * pad16(24)};
  ps.dbg["tap2"] = {taps[2], sizeof(float) * B * d.h[8] * d.w[8] * pad16(48)};
  ps.dbg["tap3"] = {taps[3], sizeof(float) * B * d.h[11] * d.w[11] * 576};
  if (ps.debug) ps.p->debug = ps.dbg;
  return KPD_OK;
}

// person-detector glue (boxes become an output)
static int stage_detect(Pass& ps, const FwdArgs& a) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  const int B = d.B;
  const Stage sg(p, "person_detect", ps.st);
  // pool + heads + decode in one launch (person_detect_kernel); KPD_PD_UNFUSED=1:
  // the three launches with the pooled / head maps through HBM (A/B)
  static const bool pd_unfused = kpd_diag_env("KPD_PD_UNFUSED") != nullptr;
  if (!pd_unfused && p->pd.cin == 128 && p->pd.cin_p == 128 && p->pd.cout_p == 48 && !p->pd.bf16 &&
      person_detect_fits(d.Wf)) {
    kpd_path(KP_PD_FUSED);
    HIP_TRY(launch_person_detect(w.feat, B, d.Hf, d.Wf, static_cast<const float*>(p->pd.w), p->pd.b, p->anchors, a.H,
                                 a.W, p->det_conf, w.pd_boxes, w.pd_scores, ps.st));
  } else {
    kpd_path(KP_PD_UNFUSED);
    HIP_TRY(launch_adaptive_pool56(w.feat, B, d.Hf, d.Wf, 128, w.pd_pool, ps.st));
    kpd_path_at(KP_PD);
    if (int rc = conv(ps, p->pd, w.pd_pool, B, 56, 56, 128, w.pd_head, ACT_NONE)) return rc;
    kpd_path_at(KP_TOP);
    HIP_TRY(launch_person_decode(w.pd_head, B, p->pd.cout_p, p->anchors, a.H, a.W, p->det_conf, w.pd_boxes,
                                 w.pd_scores, ps.st));
  }
  if (ps.debug) {   // the NMS's inputs: every candidate box, scores -inf where score <= conf
    p->debug["pd_boxes"] = {w.pd_boxes, sizeof(float) * (size_t)B * 56 * 56 * 9 * 4};
    p->debug["pd_scores"] = {w.pd_scores, sizeof(float) * (size_t)B * 56 * 56 * 9};
  }
  HIP_TRY(launch_nms_sets(w.pd_boxes, w.pd_scores, B, 56 * 56 * 9, p->det_iou, a.P, a.P, w.pd_keep, w.pd_nkeep,
                          w.pd_alive, ps.st, 1, a.boxes, a.box_scores));
  return KPD_OK;
}

// dual head, split: one ROI-align pass for both heads with KEYPOINT_HEAD's
// spatial attention fused (roi_kh_kernel); KPD_NO_ROI_KH=1: the separate
// launches (A/B)
static bool roi_kh_ok(const Pass& ps, const FwdArgs& a) {
  static const bool no_roi_kh = kpd_diag_env("KPD_NO_ROI_KH") != nullptr;
  return a.dual() && ps.p->kh_split && ps.w->kxs && ps.p->kh_sa1.ws && !no_roi_kh &&
         kpd_diag_env("KPD_KH_ATT1") == nullptr;
}

// slot map (unless top-k wrote it) and the ROI align of the top-64 channels
static int stage_roi(Pass& ps, const FwdArgs& a, bool roi_kh) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const Dims& d = ps.d;
  const int R = a.NB * a.P, P = a.P;
  const Stage sg(p, "roi_align", ps.st);
  if (!a.slot_in_topk()) {
    kpd_path(KP_SLOTMAP);
    HIP_TRY(launch_slotmap(a.boxes, a.NB, P, w.slot, ps.st));
  }
  kpd_path(roi_kh ? KP_ROI_KH : KP_ROI_ALIGN);
  if (roi_kh)
    HIP_TRY(launch_roi_kh(w.feat, d.Hf, d.Wf, w.topk, a.boxes, R, P, w.roi, w.roi_stats, p->kh_sa1.ws,
                          p->kh_sa1.w_exp, p->kh_sa1.b, p->kh_sa2_w, p->kh_sa2_b, w.imax, P, 1, w.hsc, w.kxs, ps.st,
                          ps.take_stamps("stamps_roikh_0", (size_t)56 * R)));
  else
    HIP_TRY(launch_roi_align(w.feat, d.Hf, d.Wf, 128, w.topk, a.boxes, R, P, w.roi, w.roi_stats, ps.st,
                             ps.take_stamps("stamps_roi_0", (size_t)56 * R)));
  return KPD_OK;
}

// per-ROI heads: HeatmapHead + decode, and KEYPOINT_HEAD with the dual-head flag.
// no output memsets: the padding slots are written (zeros / dummy person) by
// hm_final_kernel, decode_kernel and kh_final_kernel through the slot map
static int stage_heads(Pass& ps, const FwdArgs& a, bool roi_kh) {
  kpd_plan* p = ps.p; Work& w = *ps.w; const hipStream_t st = ps.st;
  const int R = a.NB * a.P, P = a.P;
  float* heat_out = a.heat ? a.heat : w.heat;
  if (ps.debug) p->debug["roi"] = {w.roi, sizeof(float) * (size_t)R * 3136 * 64};
  kpd_path_at(KP_HM);
  const long hmrows = (long)R * kHmRoiPos - kHmPitch;
  unsigned long long* st2 = ps.take_stamps("stamps_hm2", (size_t)((hmrows + 255) / 224) * 2);
  unsigned long long* st3 = ps.take_stamps("stamps_hm3", (size_t)((hmrows + 255) / 256) * 2);
  unsigned long long* st1 = ps.take_stamps("stamps_hm1", (size_t)((hmrows + 255) / 224) * 2);
  if (int rc = run_heatmap_head(ps, R, P, heat_out, KPD_HEAD_ALL, nullptr, st2, st3, st1)) return rc;
  kpd_path_at(KP_TOP);
  {
    const Stage sg(p, "hm_final_decode", st);
    HIP_TRY(launch_decode(heat_out, a.boxes, w.slot, R, P, a.kpts, a.vis, st));
  }
  if (!a.dual()) return KPD_OK;
  // KEYPOINT_HEAD on ROI-align of the 128-channel FPN level 0 (keypoint_head.py:51-62)
  const Stage sg(p, "keypoint_head", st);
  if (!roi_kh) {
    kpd_path(KP_ROI_ALIGN128);
    HIP_TRY(launch_roi_align(w.feat, ps.d.Hf, ps.d.Wf, 128, nullptr, a.boxes, R, P, w.kx, nullptr, st));
  }
  kpd_path_at(KP_KH);
  // sized for 256-row tiles, the smallest the KEYPOINT_HEAD convs take (hm_schedule,
  // conv_glds.hip: conv 1 256 rows, convs 2 / 3 384 / 512)
  unsigned long long* khst[3] = {ps.take_stamps("stamps_kh1", (size_t)((hmrows + 255) / 256)),
                                 ps.take_stamps("stamps_kh2", (size_t)((hmrows + 255) / 256)),
                                 ps.take_stamps("stamps_kh3", (size_t)((hmrows + 255) / 256))};
  return run_keypoint_head(ps, R, P, a.kh_kpts, a.kh_vis, w.imax, P, 1, roi_kh, khst);
}

// One sub-batch of the forward pass on one stream, with workspace k.
// Arguments are validated by kpd_forward; `a` is the view of the sub-batch's
// images.  Debug buffers are recorded only when debug != 0.
// pipelined sub-batches: mark_ev is recorded once this sub-batch has passed
// stage mark_at (1 body, 2 FPN laterals, 3 FPN level 0, 4 top-k, 5 ROI align)
static int forward_one(kpd_plan* p, int k, bool debug, const FwdArgs& a, hipStream_t st, hipEvent_t mark_ev = nullptr,
                       int mark_at = 0) {
  const PathScope path_scope(p);
  auto mark = [&](int at) -> int {
    if (mark_ev && mark_at == at) HIP_TRY(hipEventRecord(mark_ev, st));
    return KPD_OK;
  };
  Pass ps;
  const float* taps[4] = {};
  if (int rc = begin_pass(ps, p, k, debug, a.B, a.H, a.W, a.NB, a.P, a.flags, st)) return rc;
  if (int rc = stage_body(ps, a.image, a.C, taps)) return rc;
  if (int rc = mark(1)) return rc;
  if (int rc = stage_laterals(ps, taps, false)) return rc;
  if (int rc = mark(2)) return rc;
  if (int rc = stage_level0(ps, level0_footprint(ps, a) ? &a : nullptr)) return rc;
  if (int rc = mark(3)) return rc;
  if (int rc = stage_topk(ps, a)) return rc;
  if (int rc = mark(4)) return rc;
  if (int rc = publish_backbone(ps, a, taps)) return rc;
  if (a.detect())
    if (int rc = stage_detect(ps, a)) return rc;
  if (a.NB * a.P == 0) return KPD_OK;
  const bool roi_kh = roi_kh_ok(ps, a);
  if (int rc = stage_roi(ps, a, roi_kh)) return rc;
  if (int rc = mark(5)) return rc;
  return stage_heads(ps, a, roi_kh);
}

static int forward_impl(kpd_plan* p, const FwdArgs& a, void* stream);

// launch a captured forward on the caller's stream and mark its completion
static int launch_graph(kpd_plan::GraphEntry& g, hipStream_t st) {
  HIP_TRY(hipGraphLaunch(g.exec, st));
  if (!g.done) HIP_TRY(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(g.done, st));
  return KPD_OK;
}

// KPD_GRAPH=1: a forward is a launch-bound chain of ~60 kernels (at one image
// the launches, not the kernels, set the latency), so a repeated call with the
// same signature replays one captured hipGraph.  The first call of a
// signature runs eagerly (it may allocate the workspace); the second is
// captured on the plan's own stream (the caller's may be the legacy default
// stream, which cannot capture) and launched on the caller's; later calls
// only launch.  Stage timing and debug buffers need eager forwards: graphs
// are off while timing is on.
int kpd_forward(kpd_plan* p, const float* image, int B, int C, int H, int W, float* boxes, int NB, int P,
                int flags, float* kpts, float* vis, float* heat, float* kh_kpts, float* kh_vis, float* box_scores,
                int32_t* topk_out, void* stream) {
  const FwdArgs a{image, B, C, H, W, boxes, NB, P, flags, kpts, vis, heat, kh_kpts, kh_vis, box_scores, topk_out};
  if (!p || !p->use_graphs || !p->finalized || p->timing) return forward_impl(p, a, stream);
  const std::vector<uintptr_t> key = {
      (uintptr_t)a.image, (uintptr_t)a.B, (uintptr_t)a.C, (uintptr_t)a.H, (uintptr_t)a.W, (uintptr_t)a.boxes,
      (uintptr_t)a.NB, (uintptr_t)a.P, (uintptr_t)a.flags, (uintptr_t)a.kpts, (uintptr_t)a.vis, (uintptr_t)a.heat,
      (uintptr_t)a.kh_kpts, (uintptr_t)a.kh_vis, (uintptr_t)a.box_scores, (uintptr_t)a.topk_out, (uintptr_t)stream,
      (uintptr_t)p->streams};
  auto eager = [&](void* s_) { return forward_impl(p, a, s_); };
  if (p->graphs.size() >= 64 && !p->graphs.count(key)) {   // signatures that never repeat: bounded
    // the executable graphs may still be running on their callers' streams:
    // each waits for its own last launch only
    HIP_TRY(hipSetDevice(p->device));
    for (auto& kv : p->graphs) HIP_TRY(retire_graph(kv.second));
    p->graphs.clear();
  }
  kpd_plan::GraphEntry& g = p->graphs[key];
  if (g.never) return eager(stream);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (g.exec && g.epoch == p->ws_epoch) {
    HIP_TRY(hipSetDevice(p->device));
    // the graph assumes zeroed split-scale slots (each forward's top-k kernel
    // re-zeroes the ones it used); a forward without top-k in between
    // (kpd_backbone) leaves them set: zero them here, as an eager forward would
    for (int k = 0; k <= kpd_plan::kMaxSub; ++k)
      if (p->have_work[k] && p->work[k].sc_dirty) {
        HIP_TRY(hipMemsetAsync(p->work[k].sc, 0, (size_t)2 * p->dims[k].B * kAmaxStride * sizeof(float), st));
        p->work[k].sc_dirty = false;
      }
    if (p->path_on) p->path.e.clear();   // a replay takes no dispatch decision
    return launch_graph(g, st);
  }
  if (g.exec) {   // stale (re-carve, re-finalize, detector change): its last launch may still be running
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(retire_graph(g));
    g.seen = 0;
  }
  if (g.seen++ == 0)   // eager: allocations and first-use setup happen outside any capture
    return eager(stream);
  HIP_TRY(hipSetDevice(p->device));
  if (!p->graph_st) HIP_TRY(hipStreamCreateWithFlags(&p->graph_st, hipStreamNonBlocking));
  // The captured forward_impl updates host-side workspace state (sc_dirty,
  // and on a re-carve have_work / dims) as if its work had run.  If the
  // capture is abandoned, none of it ran: restore that state, so the eager
  // retry zeroes what it must (a dirty split-scale slot, a re-carved
  // workspace's zero borders).
  bool dirty0[kpd_plan::kMaxSub + 1], have0[kpd_plan::kMaxSub + 1];
  for (int k = 0; k <= kpd_plan::kMaxSub; ++k) {
    dirty0[k] = p->work[k].sc_dirty;
    have0[k] = p->have_work[k];
  }
  auto abandon = [&]() {
    for (int k = 0; k <= kpd_plan::kMaxSub; ++k) {
      p->work[k].sc_dirty = dirty0[k] || p->have_work[k] != have0[k];
      // a slot (re-)carved inside the capture: its memset never ran -> carve again eagerly
      if (p->have_work[k] && !have0[k]) p->have_work[k] = false;
    }
  };
  const long epoch0 = p->ws_epoch;
  HIP_TRY(hipStreamBeginCapture(p->graph_st, hipStreamCaptureModeRelaxed));
  const int rc = forward_impl(p, a, p->graph_st);
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(p->graph_st, &graph);
  const bool forced = p->graph_abandon_next;
  p->graph_abandon_next = false;
  if (rc != KPD_OK || ec != hipSuccess || p->ws_epoch != epoch0 || forced) {
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    // not capturable here (an allocation or sync inside it, the carve changed
    // under it): this call runs eagerly and reports its own errors
    abandon();
    if (p->ws_epoch != epoch0)   // a re-carve inside the capture: every slot re-carves (and re-zeroes) eagerly
      for (int k = 0; k <= kpd_plan::kMaxSub; ++k) p->have_work[k] = false;
    g.seen = 0;
    return eager(stream);
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess) {   // never capturable for this signature: eager from now on
    (void)hipGetLastError();
    abandon();
    g.never = true;
    g.seen = 0;
    return eager(stream);
  }
  g.exec = exec;
  g.epoch = p->ws_epoch;
  return launch_graph(g, st);
}

static int forward_impl(kpd_plan* p, const FwdArgs& a, void* stream) {
  const int B = a.B, H = a.H, W = a.W, NB = a.NB, P = a.P, flags = a.flags;
  if (!p) return fail(KPD_EINVAL, "null plan");
  if (!p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_body || !p->has_fpn || !p->has_ca || !p->has_hm)
    return fail(KPD_ESTATE, "plan lacks backbone / fpn / channel_attention / heatmap_head weights");
  if (!a.image || B <= 0 || H < 32 || W < 32) return fail(KPD_EINVAL, "bad image shape");
  if (a.C != p->in_ch) return fail(KPD_EINVAL, "image channels do not match backbone in_channels");
  if (flags & ~(KPD_FLAG_DETECT | KPD_FLAG_DUAL_HEAD | KPD_FLAG_FULL_LEVEL0)) return fail(KPD_EINVAL, "unknown flags");
  const bool detect = a.detect(), dual = a.dual();
  if (detect && (NB != B || P <= 0 || !a.boxes)) return fail(KPD_EINVAL, "detect mode: boxes must be [B][P>0][4]");
  if (detect && !p->anchors) return fail(KPD_ESTATE, "person detector weights missing");
  if (dual && !p->has_kh) return fail(KPD_ESTATE, "dual head requested but no keypoint_head.* weights");
  if (dual && NB * P > 0 && (!a.kh_kpts || !a.kh_vis)) return fail(KPD_EINVAL, "null dual-head output pointer");
  if (NB < 0 || NB > B || P < 0) return fail(KPD_EINVAL, "bad box batch");
  if (NB * P > 0 && (!a.boxes || !a.kpts || !a.vis)) return fail(KPD_EINVAL, "null box/output pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  p->debug.clear();
  if (p->path_on) p->path.e.clear();

  // Images are independent (eval BN, per-image ROI loops -- SURVEY §8(e)), so
  // a large batch runs as S contiguous sub-batches on S streams: the many
  // small latency-bound launches of one sub-batch (MobileNet body, heads)
  // overlap the other's.  Sub-batch 0 uses the caller's stream; the others
  // fork from it and join back before return.  A sub-batch larger than
  // max_pass_images runs as consecutive passes on its stream, reusing its
  // workspace.  Debug buffers need one pass.
  constexpr int kMinSub = 16;
  const int S = std::max(1, std::min({p->streams, kpd_plan::kMaxSub, B / kMinSub}));
  const int cap = max_pass_images(H, W);
  auto run = [&](int k, bool debug, int b0, int b1, hipStream_t sk, hipEvent_t mev = nullptr, int mat = 0) -> int {
    const int nb = b1 - b0;
    const int npass = (nb + cap - 1) / cap;
    for (int q = 0; q < npass; ++q) {
      const int c0 = b0 + (int)((long)nb * q / npass), c1 = b0 + (int)((long)nb * (q + 1) / npass);
      if (int rc = forward_one(p, k, debug && npass == 1, a.images(c0, c1), sk, q + 1 == npass ? mev : nullptr, mat))
        return rc;
    }
    return KPD_OK;
  };
  if (S == 1) return run(0, true, 0, B, st);
  // A/B (KPD_PIPE=<stage>): sub-batch k+1 waits until sub-batch k has passed
  // that stage (1 body .. 5 ROI align) instead of starting at once;
  // KPD_PIPE_PRI=1 runs sub-batches 1.. on high-priority streams, so their
  // workgroups are dispatched ahead of the running sub-batch's at every free CU
  static const int pipe_at = kpd_diag_env("KPD_PIPE") ? atoi(kpd_diag_env("KPD_PIPE")) : 0;
  static const bool pipe_pri = kpd_diag_env("KPD_PIPE_PRI") != nullptr;
  if (!p->fork_ev) HIP_TRY(hipEventCreateWithFlags(&p->fork_ev, hipEventDisableTiming));
  for (int k = 1; k < S; ++k) {
    if (!p->sub_st[k]) HIP_TRY(hipStreamCreateWithFlags(&p->sub_st[k], hipStreamNonBlocking));
    if (!p->join_ev[k]) HIP_TRY(hipEventCreateWithFlags(&p->join_ev[k], hipEventDisableTiming));
    if (pipe_pri && !p->sub_st_pri[k]) {
      int lo = 0, hi = 0;
      HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIP_TRY(hipStreamCreateWithPriority(&p->sub_st_pri[k], hipStreamNonBlocking, hi));
    }
  }
  for (int k = 0; k < S && pipe_at > 0; ++k)
    if (!p->pipe_ev[k]) HIP_TRY(hipEventCreateWithFlags(&p->pipe_ev[k], hipEventDisableTiming));
  HIP_TRY(hipEventRecord(p->fork_ev, st));
  int rc = KPD_OK;
  for (int k = 0; k < S && rc == KPD_OK; ++k) {
    const int b0 = (int)((long)B * k / S), b1 = (int)((long)B * (k + 1) / S);
    hipStream_t sk = k ? (pipe_pri ? p->sub_st_pri[k] : p->sub_st[k]) : st;
    if (k) HIP_TRY(hipStreamWaitEvent(sk, p->fork_ev, 0));
    if (k && pipe_at > 0) HIP_TRY(hipStreamWaitEvent(sk, p->pipe_ev[k - 1], 0));
    rc = run(k, false, b0, b1, sk, pipe_at > 0 && k + 1 < S ? p->pipe_ev[k] : nullptr, pipe_at);
  }
  for (int k = 1; k < S; ++k) {
    HIP_TRY(hipEventRecord(p->join_ev[k], pipe_pri ? p->sub_st_pri[k] : p->sub_st[k]));
    HIP_TRY(hipStreamWaitEvent(st, p->join_ev[k], 0));
  }
  return rc;
}

int kpd_plan_set_streams(kpd_plan* p, int n) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  if (n < 1 || n > kpd_plan::kMaxSub) return fail(KPD_EINVAL, "streams must be in [1, 4]");
  p->streams = n;
  return KPD_OK;
}

int kpd_plan_set_graphs(kpd_plan* p, int enable) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  if (enable < 0 || enable > 2) return fail(KPD_EINVAL, "enable must be 0, 1 or 2");
  p->use_graphs = enable != 0;
  p->graph_abandon_next = enable == 2;
  return KPD_OK;
}

int kpd_plan_set_detector(kpd_plan* p, float conf_threshold, float nms_iou_threshold) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  if (!(conf_threshold >= 0.f && conf_threshold <= 1.f) || !(nms_iou_threshold >= 0.f && nms_iou_threshold <= 1.f))
    return fail(KPD_EINVAL, "thresholds must be in [0, 1]");
  p->det_conf = conf_threshold;
  p->det_iou = nms_iou_threshold;
  ++p->ws_epoch;   // captured forwards hold the old thresholds
  return KPD_OK;
}

int kpd_plan_path_log(kpd_plan* p, int enable) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  p->path_on = enable != 0;
  p->path.e.clear();
  return KPD_OK;
}

int kpd_plan_path_query(kpd_plan* p, char* buf, size_t bytes, size_t* need) {
  std::string s;
  if (p) {
    for (const KpdPathEntry& e : p->path.e) s += path_token(e.site, e.idx, e.tok, e.val) + "\n";
  } else {   // every token this build can emit: each row at each of its sites
    for (int t = 0; t < KP_COUNT; ++t) {
      if ((kPathRows[t].sites & KP_DIAG) && !KPD_DIAG) continue;
      for (const auto& ps : kPathSites)
        if (kPathRows[t].sites & ps.site) s += path_token(ps.site, -1, t, -1) + "\n";
    }
  }
  if (!s.empty()) s.pop_back();
  if (need) *need = s.size() + 1;
  if (!buf) return KPD_OK;
  if (bytes < s.size() + 1) return fail(KPD_EINVAL, "destination too small");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return KPD_OK;
}

int kpd_plan_timing(kpd_plan* p, int enable) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  p->timing = enable != 0;
  if (p->timing)
    for (auto& kv : p->timers) kv.second.used = 0;
  return KPD_OK;
}

int kpd_plan_timing_stage(kpd_plan* p, const char* stage) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  p->timing_only = stage ? stage : "";
  return KPD_OK;
}

int kpd_plan_timing_query(kpd_plan* p, const char* stage, double* total_ms, int* count) {
  if (!p || !stage || !total_ms || !count) return fail(KPD_EINVAL, "null argument");
  *total_ms = 0.0;
  *count = 0;
  auto it = p->timers.find(stage);
  if (it == p->timers.end()) return KPD_OK;
  for (size_t i = 0; i < it->second.used; ++i) {
    auto& e = it->second.ev[i];
    HIP_TRY(hipEventSynchronize(e.second));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
    *total_ms += ms;
  }
  *count = (int)it->second.used;
  return KPD_OK;
}

int kpd_debug_copy(kpd_plan* p, const char* name, void* dst, size_t bytes, size_t* size_out, void* stream) {
  if (!p || !name) return fail(KPD_EINVAL, "null argument");
  auto it = p->debug.find(name);
  if (it == p->debug.end()) return fail(KPD_EINVAL, std::string("no debug buffer ") + name);
  if (size_out) *size_out = it->second.second;
  if (!dst) return KPD_OK;
  if (bytes < it->second.second) return fail(KPD_EINVAL, "destination too small");
  HIP_TRY(hipMemcpyAsync(dst, it->second.first, it->second.second, hipMemcpyDeviceToDevice,
                         reinterpret_cast<hipStream_t>(stream)));
  return KPD_OK;
}

// ---------------------------------------------------------------- stand-alone operators
// The reference's submodule forwards, called outside the model's forward
// (each on a plan holding that submodule's weights).

// the pass of a stand-alone head on R ROIs, in the operators' own workspace
static int op_pass(Pass& ps, kpd_plan* p, int R, int flags, hipStream_t st) {
  Dims& d = ps.d;
  // one carve serves both stand-alone heads: the union of their flags, so
  // alternating HeatmapHead / KEYPOINT_HEAD calls never re-carve
  d.B = 0; d.NB = R; d.P = 1; d.flags = flags | (p->has_kh ? KPD_FLAG_DUAL_HEAD : 0);
  if (int rc = ensure_work(p, d, kpd_plan::kOpWs, st)) return rc;
  ps.p = p; ps.st = st;
  ps.w = &p->work[kpd_plan::kOpWs];
  ps.splitk = ps.w->splitk;
  return KPD_OK;
}

int kpd_heatmap_head(kpd_plan* p, const float* x, int R, int H, int W, int parts, float* heat, float* ch_w,
                     float* sp_w, void* stream) {
  if (!p || !p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_hm) return fail(KPD_ESTATE, "plan has no heatmap_head weights");
  if (R < 0 || H != 56 || W != 56) return fail(KPD_EINVAL, "HeatmapHead input must be [R][64][56][56]");
  if (parts & ~KPD_HEAD_ALL) return fail(KPD_EINVAL, "unknown HeatmapHead parts");
  if (R == 0) return KPD_OK;
  if (!x || ((parts & KPD_HEAD_CONVS) && !heat)) return fail(KPD_EINVAL, "null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  Pass ps;
  if (int rc = op_pass(ps, p, R, 0, st)) return rc;
  Work* w = ps.w;
  if (p->path_on) p->path.e.clear();
  const PathScope path_scope(p);
  kpd_path_at(KP_HM);
  // any input sign: the split convs' bound is max |x| (hsc[r][2]), not the max
  const bool hsplit = p->precision == KPD_PRECISION_SPLIT;
  if (hsplit) HIP_TRY(hipMemsetAsync(w->hsc, 0, sizeof(float) * 4 * R, st));
  HIP_TRY(launch_nchw_rows_to_nhwc(x, R, 64, 56, 56, w->roi, w->roi_stats, st, hsplit ? w->hsc + 2 : nullptr, 4));
  HIP_TRY(hipMemsetAsync(w->slot, 0, sizeof(int32_t) * R, st));   // ROI r -> heat[r] (P = 1)
  if (int rc = run_heatmap_head(ps, R, 1, heat, parts, sp_w, nullptr, nullptr, nullptr, 1)) return rc;
  if (ch_w) HIP_TRY(hipMemcpyAsync(ch_w, w->cw, sizeof(float) * R * 64, hipMemcpyDeviceToDevice, st));
  return KPD_OK;
}

int kpd_keypoint_head(kpd_plan* p, const float* x, int R, int H, int W, float* kpts, float* vis, void* stream) {
  if (!p || !p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_kh) return fail(KPD_ESTATE, "plan has no keypoint_head weights");
  if (R < 0 || H != 56 || W != 56) return fail(KPD_EINVAL, "KEYPOINT_HEAD input must be [R][128][56][56]");
  if (R == 0) return KPD_OK;
  if (!x || !kpts || !vis) return fail(KPD_EINVAL, "null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  Pass ps;
  if (int rc = op_pass(ps, p, R, KPD_FLAG_DUAL_HEAD, st)) return rc;
  Work* w = ps.w;
  if (p->path_on) p->path.e.clear();
  const PathScope path_scope(p);
  kpd_path_at(KP_KH);
  // any input sign: the split path's bound is max |x| per ROI (hsc[r][2])
  if (p->kh_split) HIP_TRY(hipMemsetAsync(w->hsc, 0, sizeof(float) * 4 * R, st));
  HIP_TRY(launch_nchw_rows_to_nhwc(x, R, 128, 56, 56, w->kx, nullptr, st, p->kh_split ? w->hsc + 2 : nullptr, 4));
  HIP_TRY(hipMemsetAsync(w->slot, 0, sizeof(int32_t) * R, st));
  return run_keypoint_head(ps, R, 1, kpts, vis, w->hsc + 2, 1, 4);
}

// One pass of the stand-alone backbone operators in workspace 0: the body
// stage and, with fpn, the laterals (every level kept) and level 0
static int backbone_pass(Pass& ps, kpd_plan* p, const float* image, int nb, int C, int H, int W, hipStream_t st,
                         bool fpn, const float* taps[4]) {
  const PathScope path_scope(p);
  if (int rc = begin_pass(ps, p, 0, false, nb, H, W, 0, 0, 0, st)) return rc;
  if (int rc = stage_body(ps, image, C, taps)) return rc;
  if (!fpn) return KPD_OK;
  if (int rc = stage_laterals(ps, taps, true)) return rc;
  return stage_level0(ps, nullptr);
}

int kpd_backbone(kpd_plan* p, const float* image, int B, int C, int H, int W, float* out0, float* out1, float* out2,
                 float* out3, void* stream) {
  if (!p || !p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_body || !p->has_fpn) return fail(KPD_ESTATE, "plan lacks backbone.body / backbone.fpn weights");
  for (int i = 0; i < 3; ++i)
    if (!p->fpn_lv[i].w) return fail(KPD_ESTATE, "plan lacks backbone.fpn.fpn_convs.1-3 weights");
  if (!image || B <= 0 || H < 32 || W < 32) return fail(KPD_EINVAL, "bad image shape");
  if (C != p->in_ch) return fail(KPD_EINVAL, "image channels do not match backbone in_channels");
  float* outs[4] = {out0, out1, out2, out3};
  for (float* o : outs)
    if (!o) return fail(KPD_EINVAL, "null output pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  if (p->path_on) p->path.e.clear();
  // level sizes: stem (features.0), features.3, .8, .12
  const Dims lv = level_dims(H, W);
  const int lh[4] = {lv.h[0], lv.h[3], lv.h[8], lv.h[11]}, lw[4] = {lv.w[0], lv.w[3], lv.w[8], lv.w[11]};
  const int cap = max_pass_images(H, W), npass = (B + cap - 1) / cap;
  for (int q = 0; q < npass; ++q) {
    const int b0 = (int)((long)B * q / npass), b1 = (int)((long)B * (q + 1) / npass), nb = b1 - b0;
    // body, every lateral level, level 0; no top-k follows, so on the fpn0x
    // path the split-scale slots stay dirty for the next forward to zero
    Pass ps;
    const float* taps[4] = {};
    if (int rc = backbone_pass(ps, p, image + (size_t)b0 * C * H * W, nb, C, H, W, st, true, taps)) return rc;
    Work& w = *ps.w;
    HIP_TRY(launch_nhwc_to_nchw(w.feat, nb, lh[0] * lw[0], 128, outs[0] + (size_t)b0 * 128 * lh[0] * lw[0], st));
    for (int i = 1; i < 4; ++i) {   // fpn_convs[i] on lateral i (backbone.py:39), into the free level-0 buffer
      if (int rc = conv(ps, p->fpn_lv[i - 1], w.lat[i], nb, lh[i], lw[i], 128, w.feat, ACT_RELU)) return rc;
      HIP_TRY(launch_nhwc_to_nchw(w.feat, nb, lh[i] * lw[i], 128, outs[i] + (size_t)b0 * 128 * lh[i] * lw[i], st));
    }
  }
  return KPD_OK;
}

// The trunk's ROI features as the fused forward serves them to HeatmapHead:
// forward_one's stages up to and including stage_roi on a flags-0 pass, then
// the selected rows of w.roi (NHWC) gathered to `out` (NCHW).  Eager, on the
// caller's stream, in workspace 0; the host-side workspace state (sc_dirty
// through stage_body / stage_topk, the carve through begin_pass) moves exactly
// as in a forward of the same shapes, so later forwards and graph replays see
// what they expect.
int kpd_roi_features(kpd_plan* p, const float* image, int B, int C, int H, int W, const float* boxes, int P,
                     const int32_t* rows, int n, float* out, void* stream) {
  // kpd_forward's argument checks, ahead of the plan's state (they need no device)
  if (!p) return fail(KPD_EINVAL, "null plan");
  if (!image || B <= 0 || H < 32 || W < 32) return fail(KPD_EINVAL, "bad image shape");
  if (C != p->in_ch) return fail(KPD_EINVAL, "image channels do not match backbone in_channels");
  if (P <= 0 || !boxes) return fail(KPD_EINVAL, "boxes must be [B][P>0][4]");
  if ((long)B * P > 0x7fffffffL) return fail(KPD_EINVAL, "boxes: too many ROIs");
  if (n < 0 || (!rows && n != B * P)) return fail(KPD_EINVAL, "n must be the length of rows, or B*P without rows");
  if (n > 0 && !out) return fail(KPD_EINVAL, "null output pointer");
  if (!p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_body || !p->has_fpn || !p->has_ca)
    return fail(KPD_ESTATE, "plan lacks backbone / fpn / channel_attention weights");
  if (n == 0) return KPD_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  p->debug.clear();   // they point into the workspace this call rewrites
  if (p->path_on) p->path.e.clear();
  const FwdArgs a{image, B, C, H, W, const_cast<float*>(boxes), B, P, 0,
                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const int cap = max_pass_images(H, W), npass = (B + cap - 1) / cap;
  for (int q = 0; q < npass; ++q) {
    const int b0 = (int)((long)B * q / npass), b1 = (int)((long)B * (q + 1) / npass);
    const FwdArgs s = a.images(b0, b1);
    const PathScope path_scope(p);
    Pass ps;
    const float* taps[4] = {};
    if (int rc = begin_pass(ps, p, 0, false, s.B, H, W, s.NB, P, 0, st)) return rc;
    if (int rc = stage_body(ps, s.image, C, taps)) return rc;
    if (int rc = stage_laterals(ps, taps, false)) return rc;
    if (int rc = stage_level0(ps, level0_footprint(ps, s) ? &s : nullptr)) return rc;
    if (int rc = stage_topk(ps, s)) return rc;
    if (int rc = stage_roi(ps, s, false)) return rc;
    // rows of other passes fail the kernel's range test; without a row list output row j is ROI j
    HIP_TRY(launch_nhwc64_rows_to_nchw(ps.w->roi, s.NB * P, 3136, rows, b0 * P, n, out, st));
  }
  return KPD_OK;
}

// The detector's training input: forward_one's stages up to
// FPN level 0 at every pixel (a pass without boxes stores all of it), then the
// 56 x 56 adaptive pool of the eval detector's unfused path, whose sums round
// as the fused person_detect_kernel's.  Eager, on the caller's stream, in
// workspace 0, the host-side workspace state moving as kpd_roi_features' does.
int kpd_detector_features(kpd_plan* p, const float* image, int B, int C, int H, int W, float* out, void* stream) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  if (!image || B <= 0 || H < 32 || W < 32) return fail(KPD_EINVAL, "bad image shape");
  if (C != p->in_ch) return fail(KPD_EINVAL, "image channels do not match backbone in_channels");
  if (!out) return fail(KPD_EINVAL, "null output pointer");
  if (!p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_body || !p->has_fpn) return fail(KPD_ESTATE, "plan lacks backbone.body / backbone.fpn weights");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  p->debug.clear();   // they point into the workspace this call rewrites
  if (p->path_on) p->path.e.clear();
  const int cap = max_pass_images(H, W), npass = (B + cap - 1) / cap;
  for (int q = 0; q < npass; ++q) {
    const int b0 = (int)((long)B * q / npass), b1 = (int)((long)B * (q + 1) / npass), nb = b1 - b0;
    const PathScope path_scope(p);
    Pass ps;
    const float* taps[4] = {};
    if (int rc = begin_pass(ps, p, 0, false, nb, H, W, 0, 0, 0, st)) return rc;
    if (int rc = stage_body(ps, image + (size_t)b0 * C * H * W, C, taps)) return rc;
    if (int rc = stage_laterals(ps, taps, false)) return rc;
    if (int rc = stage_level0(ps, nullptr)) return rc;
    HIP_TRY(launch_adaptive_pool56(ps.w->feat, nb, ps.d.Hf, ps.d.Wf, 128, out + (size_t)b0 * 3136 * 128, st));
  }
  return KPD_OK;
}

int kpd_backbone_body(kpd_plan* p, const float* image, int B, int C, int H, int W, float* feat0, float* feat1,
                      float* feat2, float* feat3, void* stream) {
  if (!p || !p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_body) return fail(KPD_ESTATE, "plan lacks backbone.body weights");
  if (!image || B <= 0 || H < 32 || W < 32) return fail(KPD_EINVAL, "bad image shape");
  if (C != p->in_ch) return fail(KPD_EINVAL, "image channels do not match backbone in_channels");
  float* outs[4] = {feat0, feat1, feat2, feat3};
  for (float* o : outs)
    if (!o) return fail(KPD_EINVAL, "null output pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  if (p->path_on) p->path.e.clear();
  const Dims d = level_dims(H, W);
  const int lv[4] = {0, 3, 8, 11};
  const int cap = max_pass_images(H, W), npass = (B + cap - 1) / cap;
  for (int q = 0; q < npass; ++q) {
    const int b0 = (int)((long)B * q / npass), b1 = (int)((long)B * (q + 1) / npass), nb = b1 - b0;
    Pass ps;
    const float* taps[4] = {};
    if (int rc = backbone_pass(ps, p, image + (size_t)b0 * C * H * W, nb, C, H, W, st, false, taps)) return rc;
    for (int i = 0; i < 4; ++i) {
      const int c = kFpnIn[i], hw = d.h[lv[i]] * d.w[lv[i]];
      HIP_TRY(launch_nhwc_pad_to_nchw(taps[i], nb, hw, c, pad16(c), outs[i] + (size_t)b0 * c * hw, st));
    }
  }
  return KPD_OK;
}

int kpd_backbone_fpn(kpd_plan* p, const float* feat0, const float* feat1, const float* feat2, const float* feat3, int B,
                     const int* sizes, float* out0, float* out1, float* out2, float* out3, void* stream) {
  if (!p || !p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_fpn) return fail(KPD_ESTATE, "plan lacks backbone.fpn weights");
  for (int i = 0; i < 3; ++i)
    if (!p->fpn_lv[i].w) return fail(KPD_ESTATE, "plan lacks backbone.fpn.fpn_convs.1-3 weights");
  if (B < 0 || !sizes) return fail(KPD_EINVAL, "bad FPN arguments");
  if (B == 0) return KPD_OK;
  const float* feats[4] = {feat0, feat1, feat2, feat3};
  float* outs[4] = {out0, out1, out2, out3};
  int hh[4], ww[4];
  size_t in_f = 0, lat_f = 0, out_f = 0;
  for (int i = 0; i < 4; ++i) {
    hh[i] = sizes[2 * i]; ww[i] = sizes[2 * i + 1];
    if (!feats[i] || !outs[i]) return fail(KPD_EINVAL, "null FPN tensor");
    if (hh[i] <= 0 || ww[i] <= 0) return fail(KPD_EINVAL, "bad FPN level size");
    if (p->lat[i].cin != kFpnIn[i]) return fail(KPD_EINVAL, "lateral conv channels do not match the taps");
    const size_t hw = (size_t)B * hh[i] * ww[i];
    if (hw * 576 >= (1UL << 31)) return fail(KPD_EINVAL, "FPN tensors must stay below 2^31 elements");
    in_f += hw * p->lat[i].cin_p;
    lat_f += hw * 128;
    out_f = std::max(out_f, hw * 128);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  float* scratch = nullptr;
  const size_t total = in_f + lat_f + out_f + kSplitKFloats;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), total * sizeof(float), st));
  float *tin[4], *lat[4];
  float* cur = scratch;
  for (int i = 0; i < 4; ++i) { tin[i] = cur; cur += (size_t)B * hh[i] * ww[i] * p->lat[i].cin_p; }
  for (int i = 0; i < 4; ++i) { lat[i] = cur; cur += (size_t)B * hh[i] * ww[i] * 128; }
  float* lvl = cur;
  cur += out_f;
  Pass ps;   // (no workspace: the convs read the plan's weights, the stream and the scratch's split-K block)
  ps.p = p; ps.st = st; ps.splitk = cur;
  // LightweightFPN.forward (backbone.py:29-39): laterals top-down, each
  // nearest-upsampled to the next finer size and added, then fpn_convs[i]
  int rc = KPD_OK;
  hipError_t e = hipSuccess;
  for (int i = 0; i < 4 && e == hipSuccess; ++i)
    e = launch_nchw_to_nhwc_pad(feats[i], B, hh[i] * ww[i], kFpnIn[i], p->lat[i].cin_p, tin[i], st);
  for (int i = 3; i >= 0 && e == hipSuccess && rc == KPD_OK; --i) {
    ConvOpt o;
    o.res = i < 3 ? lat[i + 1] : nullptr; o.rh = i < 3 ? hh[i + 1] : 0; o.rw = i < 3 ? ww[i + 1] : 0;
    if (i == 0 && p->lat[i].cin_p <= 32)   // the 16-channel stem tap (as stage_laterals)
      e = launch_lateral_stream(tin[i], p->lat[i].cin_p, (const float*)p->lat[i].w, p->lat[i].b, o.res, B, hh[i],
                                ww[i], o.rh, o.rw, lat[i], st);
    else
      rc = conv(ps, p->lat[i], tin[i], B, hh[i], ww[i], p->lat[i].cin_p, lat[i], ACT_NONE, o);
  }
  for (int i = 0; i < 4 && e == hipSuccess && rc == KPD_OK; ++i) {
    const DevConv& L = i == 0 ? p->fpn0 : p->fpn_lv[i - 1];
    rc = conv(ps, L, lat[i], B, hh[i], ww[i], 128, lvl, ACT_RELU);
    if (rc == KPD_OK) e = launch_nhwc_to_nchw(lvl, B, hh[i] * ww[i], 128, outs[i], st);
  }
  (void)hipFreeAsync(scratch, st);
  HIP_TRY(e);
  return rc;
}

int kpd_channel_attention(kpd_plan* p, const float* x, int B, int C, int H, int W, float* scores, int32_t* topk,
                          int k, float* selected, void* stream) {
  if (!p || !p->finalized) return fail(KPD_ESTATE, "plan not finalized");
  if (!p->has_ca) return fail(KPD_ESTATE, "plan has no channel_attention weights");
  if (C != 128 || k != 64 || B < 0 || H <= 0 || W <= 0)
    return fail(KPD_EINVAL, "ChannelAttention path is built for 128 channels and top-64");
  if (B == 0) return KPD_OK;
  if (!x) return fail(KPD_EINVAL, "null input");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->device));
  char* scratch = nullptr;
  const size_t sb = (size_t)B * 2 * 128 * 4, tb = (size_t)B * 64 * 4, cb = (size_t)B * 128 * 4;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), sb + tb + cb, st));
  float* stats = reinterpret_cast<float*>(scratch);
  int32_t* tk = reinterpret_cast<int32_t*>(scratch + sb);
  float* sc = reinterpret_cast<float*>(scratch + sb + tb);
  hipError_t e = launch_nchw_channel_stats(x, B, 128, H * W, stats, st);
  if (e == hipSuccess)
    e = launch_topk(stats, B, 1, H * W, p->ca_w0, p->ca_b0, p->ca_w2, p->ca_b2, tk, sc, st, nullptr, 0, nullptr);
  if (e == hipSuccess && scores) e = hipMemcpyAsync(scores, sc, cb, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && topk) e = hipMemcpyAsync(topk, tk, tb, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && selected) e = launch_gather_planes(x, B, 128, H * W, tk, 64, selected, st);
  (void)hipFreeAsync(scratch, st);
  HIP_TRY(e);
  return KPD_OK;
}

int kpd_decode_heatmaps(const float* heat, int planes, int H, int W, int mode, float param, float* kpts,
                        float* scores, float* vis, void* stream) {
  if (planes < 0 || H < 2 || W < 2 || (planes > 0 && (!heat || !kpts)) || (mode == KPD_DECODE_MODEL && planes > 0 && !vis))
    return fail(KPD_EINVAL, "bad decode arguments");
  HIP_TRY(launch_decode_planes(heat, planes, H, W, mode, param, kpts, scores, vis,
                               reinterpret_cast<hipStream_t>(stream)));
  return KPD_OK;
}

int kpd_roi_align(const float* feat, int B, int C, int H, int W, const float* rois, int R, int out_h, int out_w,
                  float spatial_scale, int sampling_ratio, int aligned, float* out, void* stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || R < 0 || out_h <= 0 || out_w <= 0 || (R > 0 && (!feat || !rois || !out)))
    return fail(KPD_EINVAL, "bad roi_align arguments");
  HIP_TRY(launch_roi_align_nchw(feat, B, C, H, W, rois, R, out_h, out_w, spatial_scale, sampling_ratio, aligned, out,
                                reinterpret_cast<hipStream_t>(stream)));
  return KPD_OK;
}

int kpd_conv1x1(const float* x, int B, int Cin, int HW, const float* w, const float* b, int Cout, float* out,
                void* stream) {
  if (B < 0 || Cin <= 0 || HW < 0 || Cout <= 0 || (B > 0 && HW > 0 && (!x || !w || !out)))
    return fail(KPD_EINVAL, "bad conv1x1 arguments");
  HIP_TRY(launch_conv1x1_nchw(x, B, Cin, HW, w, b, Cout, out, reinterpret_cast<hipStream_t>(stream)));
  return KPD_OK;
}

int kpd_conv3x3_forward(const float* x, const float* w, const float* b, int N, int C, int H, int W, int O, float* y,
                        void* stream) {
  return kpd_conv3x3_forward_prec(x, w, b, N, C, H, W, O, y, KPD_PRECISION_SPLIT, stream);
}

int kpd_conv3x3_forward_prec(const float* x, const float* w, const float* b, int N, int C, int H, int W, int O,
                             float* y, int precision, void* stream) {
  if (precision != KPD_PRECISION_SPLIT && precision != KPD_PRECISION_MIXED)
    return fail(KPD_EINVAL, "conv3x3: precision must be KPD_PRECISION_SPLIT or KPD_PRECISION_MIXED");
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || O <= 0 || (N > 0 && (!x || !w || !y)))
    return fail(KPD_EINVAL, "bad conv3x3 arguments");
  if ((long)N * C * H * W >= (1L << 31) || (long)N * O * H * W >= (1L << 31) || (long)O * C * 9 >= (1L << 31))
    return fail(KPD_EINVAL, "conv3x3: tensors must stay below 2^31 elements");
  HIP_TRY(launch_conv3_forward(x, w, b, N, C, H, W, O, y, precision == KPD_PRECISION_MIXED,
                               reinterpret_cast<hipStream_t>(stream)));
  return KPD_OK;
}

int kpd_conv3x3_backward(const float* x, const float* w, const float* gy, int N, int C, int H, int W, int O,
                         float* gx, float* gw, float* gb, void* stream) {
  return kpd_conv3x3_backward_prec(x, w, gy, N, C, H, W, O, gx, gw, gb, KPD_PRECISION_SPLIT, stream);
}

int kpd_conv3x3_backward_prec(const float* x, const float* w, const float* gy, int N, int C, int H, int W, int O,
                              float* gx, float* gw, float* gb, int precision, void* stream) {
  if (precision != KPD_PRECISION_SPLIT && precision != KPD_PRECISION_MIXED)
    return fail(KPD_EINVAL, "conv3x3 backward: precision must be KPD_PRECISION_SPLIT or KPD_PRECISION_MIXED");
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || O <= 0 || (N > 0 && !gy) || (gx && !w) || (gw && !x))
    return fail(KPD_EINVAL, "bad conv3x3 backward arguments");
  if ((long)N * C * H * W >= (1L << 31) || (long)N * O * H * W >= (1L << 31) || (long)O * C * 9 >= (1L << 31))
    return fail(KPD_EINVAL, "conv3x3: tensors must stay below 2^31 elements");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (N == 0) {   // empty batch: zero parameter gradients
    if (gw) HIP_TRY(hipMemsetAsync(gw, 0, sizeof(float) * O * C * 9, st));
    if (gb) HIP_TRY(hipMemsetAsync(gb, 0, sizeof(float) * O, st));
    return KPD_OK;
  }
  float* part = nullptr;
  if (gw && conv3_wgrad_slices(N, H, W)) HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&part),
                                 sizeof(float) * conv3_wgrad_slices(N, H, W) * O * C * 9, st));
  const hipError_t e = launch_conv3_backward(x, w, gy, N, C, H, W, O, gx, gw, gb, part,
                                             precision == KPD_PRECISION_MIXED, st);
  if (part) HIP_TRY(hipFreeAsync(part, st));
  HIP_TRY(e);
  return KPD_OK;
}

int kpd_nms(const float* boxes, const float* scores, int n, float thr, int max_out, int32_t* keep, int32_t* n_keep,
            void* stream) {
  if (n < 0 || (n > 0 && (!boxes || !scores || !keep)) || !n_keep) return fail(KPD_EINVAL, "bad nms args");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  void* scratch = nullptr;
  if (n > 0) HIP_TRY(hipMallocAsync(&scratch, (size_t)n, st));
  const hipError_t e =
      launch_nms_sets(boxes, scores, 1, n, thr, max_out, std::max(n, 1), keep, n_keep, scratch, st, 0, nullptr, nullptr);
  if (scratch) HIP_TRY(hipFreeAsync(scratch, st));
  HIP_TRY(e);
  return KPD_OK;
}

}  // extern "C"
