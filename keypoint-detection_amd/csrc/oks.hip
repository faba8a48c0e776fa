// COCO keypoint matching on the GPU (kpd_oks_match): object
// keypoint similarity of every (detection, ground truth) pair of an image and
// COCOeval's greedy matching at up to 16 OKS thresholds, one workgroup per
// image, straight from a forward's output tensors and a collated batch.
//
//   phase 0: per ground truth the number of labelled keypoints k1 (k1 == 0:
//            the gt is ignored) and per detection whether it is present
//            (score > 0, which a NaN fails).
//   phase 1: the D x G OKS matrix in LDS as doubles, one pair per thread;
//            detection ranks by a counting comparison under nms.hip's
//            better(score, index) rule; the gt order (counted gts first, each
//            group in slot order) by prefix counts.
//   phase 2: wave t matches threshold t.  Lane l holds the gt at position l
//            of the gt order and its matched flag; per detection in rank order
//            COCOeval's walk over the gts is a wave64 arg-max over the
//            eligible lanes (unmatched, OKS not below the threshold): first
//            among the counted gts, and only when none of them is eligible
//            among the ignored ones (the walk stops at the first ignored gt
//            once it holds a counted one); an equal OKS replaces, so the
//            higher position wins a tie.
//
// Differences and sums of squares are formed in double from the fp32 inputs
// with no contraction, in the operation order DESIGN.md §3c writes out;
// tests/oks_ref.py follows it step for step, so the two differ only by the
// rounding of exp().
#include <string>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxK = KPD_OKS_MAX_K, kMaxT = KPD_OKS_MAX_T, kMaxD = KPD_OKS_MAX_D, kMaxG = KPD_OKS_MAX_G;
static_assert(kMaxG == 64 && kMaxD == 64, "one lane per gt in the matching, one LDS matrix of 64 x 64 doubles");
static_assert(kMaxT <= 16, "one wave per threshold, at most 1024 threads");

struct OksTables {
  float sigma[kMaxK];
  float thr[kMaxT];
};

// better(a, b): a ranks before b in a descending sort with index tie-break (nms.hip)
__device__ __forceinline__ bool better(float sa, int ia, float sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

__device__ __forceinline__ double pos_part(double v) { return v > 0.0 ? v : 0.0; }

// OKS of one detection against one ground truth; k1 = the gt's labelled keypoints
__device__ double oks_pair(const float* __restrict__ dk, const float* __restrict__ gk, const float* __restrict__ gv,
                           const float* __restrict__ box, double area, double sx, double sy, int k1, int K,
                           const OksTables& tb) {
  const double eps = 2.220446049250313e-16;   // 2^-52, np.spacing(1)
  double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
  if (k1 == 0) {   // no labelled keypoint: distance to the gt box doubled about its centre
    const double cx = box[0], cy = box[1], w = box[2], h = box[3];
    const double xtl = (cx - w / 2.0) * sx, ytl = (cy - h / 2.0) * sy;
    const double W = w * sx, H = h * sy;
    x0 = xtl - W;
    x1 = xtl + 2.0 * W;
    y0 = ytl - H;
    y1 = ytl + 2.0 * H;
  }
  double sum = 0.0;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    if (k1 > 0 && !(gv[k] > 0.f)) continue;
    const double xd = sx * (double)dk[2 * k], yd = sy * (double)dk[2 * k + 1];
    double dx, dy;
    if (k1 > 0) {
      dx = xd - sx * (double)gk[2 * k];
      dy = yd - sy * (double)gk[2 * k + 1];
    } else {
      dx = pos_part(x0 - xd) + pos_part(xd - x1);
      dy = pos_part(y0 - yd) + pos_part(yd - y1);
    }
    const double s2 = 2.0 * (double)tb.sigma[k];
    const double var = s2 * s2;
    const double e = (dx * dx + dy * dy) / var / (area + eps) / 2.0;
    sum += exp(-e);
    ++n;
  }
  return sum / (double)n;   // n >= 1: K >= 1, and k1 > 0 counts k1 keypoints
}

// grid B, block 64 * max(T, 4): wave t matches threshold t
__global__ __launch_bounds__(1024) void oks_match_kernel(
    const float* __restrict__ pred_kpts, const float* __restrict__ pred_scores, const float* __restrict__ gt_kpts,
    const float* __restrict__ gt_vis, const float* __restrict__ gt_boxes, const float* __restrict__ gt_area,
    const int32_t* __restrict__ n_gt, const float* __restrict__ scale, OksTables tb, int D, int G, int K, int T,
    int M, double* __restrict__ oks_out, float* __restrict__ det_score, int32_t* __restrict__ det_slot,
    int32_t* __restrict__ det_match, uint8_t* __restrict__ det_ignore, int32_t* __restrict__ gt_match,
    int32_t* __restrict__ counts) {
  __shared__ double s_oks[kMaxD * kMaxG];   // [d][g], row stride G
  __shared__ float s_score[kMaxD];          // 0 for an absent slot
  __shared__ int s_k1[kMaxG];
  __shared__ int s_det_order[kMaxD];        // caller slot at each rank, -1 past n_det
  __shared__ int s_gt_order[kMaxG];         // caller slot at each position of the gt order
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
  const int ngt = min(max(n_gt[b], 0), G);
  const double sx = scale[2 * b], sy = scale[2 * b + 1];

  // ---- phase 0
  if (tid < D) {
    const float s = pred_scores[(size_t)b * D + tid];
    s_score[tid] = s > 0.f ? s : 0.f;
    s_det_order[tid] = -1;
  }
  if (tid >= 64 && tid - 64 < G) {
    const int g = tid - 64;
    int k1 = 0;
    if (g < ngt) {
      const float* gv = gt_vis + ((size_t)b * G + g) * K;
      for (int k = 0; k < K; ++k) k1 += gv[k] > 0.f;
    }
    s_k1[g] = k1;
  }
  __syncthreads();

  // ---- phase 1: the OKS matrix, ranks and the gt order
  for (int i = tid; i < D * G; i += nthr) {
    const int d = i / G, g = i - d * G;
    double v = 0.0;   // an absent detection or a slot past n_gt
    if (g < ngt && s_score[d] > 0.f) {
      const size_t ig = (size_t)b * G + g;
      v = oks_pair(pred_kpts + ((size_t)b * D + d) * K * 2, gt_kpts + ig * K * 2, gt_vis + ig * K, gt_boxes + ig * 4,
                   (double)gt_area[ig], sx, sy, s_k1[g], K, tb);
    }
    s_oks[i] = v;
    if (oks_out) oks_out[(size_t)b * D * G + i] = v;
  }
  int ndet = 0, ncount = 0;   // present detections, counted (non-ignored) gts: every thread counts them
  for (int d = 0; d < D; ++d) ndet += s_score[d] > 0.f;
  for (int g = 0; g < ngt; ++g) ncount += s_k1[g] > 0;
  ndet = min(ndet, M);
  if (tid < D && s_score[tid] > 0.f) {
    const float s = s_score[tid];
    int rank = 0;
    for (int d = 0; d < D; ++d) rank += s_score[d] > 0.f && better(s_score[d], d, s, tid);
    if (rank < M) s_det_order[rank] = tid;
  }
  if (tid >= 64 && tid - 64 < ngt) {
    const int g = tid - 64;
    const bool ign = s_k1[g] == 0;
    int pos = ign ? ncount : 0;
    for (int h = 0; h < g; ++h) pos += (s_k1[h] == 0) == ign;
    s_gt_order[pos] = g;
  }
  __syncthreads();

  if (tid < M) {
    const int d = s_det_order[tid];
    det_slot[(size_t)b * M + tid] = d;
    det_score[(size_t)b * M + tid] = d >= 0 ? s_score[d] : 0.f;
  }
  if (tid == 0) {
    counts[2 * b] = ndet;
    counts[2 * b + 1] = ncount;
  }

  // ---- phase 2: wave t matches threshold t
  if (wave >= T) return;
  const int t = wave;
  const size_t bt = (size_t)b * T + t;
  const double t0 = (double)tb.thr[t];
  const double best0 = t0 < 1.0 - 1e-10 ? t0 : 1.0 - 1e-10;
  const bool have = lane < ngt;
  const int gs = have ? s_gt_order[lane] : 0;
  const bool ign = lane >= ncount;
  bool matched = false;
  int mdet = -1;
  for (int r = 0; r < M; ++r) {
    int mg = -1;
    bool mi = false;
    if (r < ndet) {   // wave-uniform
      const int d = s_det_order[r];
      const double o = have ? s_oks[d * G + gs] : 0.0;
      const bool elig = have && !matched && !(o < best0);
      const bool counted = __ballot(elig && !ign) != 0ull;
      const bool in = elig && (ign != counted);   // the counted group when it has an eligible gt, else the ignored
      double bo = in ? o : -INFINITY;
      int bp = in ? lane : -1;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double o2 = __shfl_xor(bo, off, 64);
        const int p2 = __shfl_xor(bp, off, 64);
        if (p2 >= 0 && (bp < 0 || o2 > bo || (o2 == bo && p2 > bp))) { bo = o2; bp = p2; }
      }
      bp = __shfl(bp, 0, 64);   // one winner for the wave whatever a non-finite OKS did to the comparisons
      if (bp >= 0) {
        if (lane == bp) { matched = true; mdet = d; }
        mg = s_gt_order[bp];
        mi = bp >= ncount;
      }
    }
    if (lane == 0) {
      det_match[bt * M + r] = mg;
      det_ignore[bt * M + r] = mi ? 1 : 0;
    }
  }
  if (lane < G) gt_match[bt * G + (have ? gs : lane)] = mdet;   // the order permutes 0..ngt-1; later slots keep -1
}

int fail(const std::string& what) { return kpd_fail_einval(("kpd_oks_match: " + what).c_str()); }

}  // namespace

extern "C" int kpd_oks_match(const float* pred_kpts, const float* pred_scores, const float* gt_kpts,
                             const float* gt_vis, const float* gt_boxes, const float* gt_area, const int32_t* n_gt,
                             const float* scale, const float* sigmas, const float* thresholds, int B, int D, int G,
                             int K, int T, int max_dets, double* oks, float* det_score, int32_t* det_slot,
                             int32_t* det_match, uint8_t* det_ignore, int32_t* gt_match, int32_t* counts,
                             void* stream) {
  if (B < 0) return fail("B must not be negative");
  if (D < 0 || D > kMaxD) return fail("D must be in [0, 64]");
  if (G < 0 || G > kMaxG) return fail("G must be in [0, 64]");
  if (K < 1 || K > kMaxK) return fail("K must be in [1, 32]");
  if (T < 1 || T > kMaxT) return fail("T must be in [1, 16]");
  if (max_dets < 1) return fail("max_dets must be at least 1");
  if (B == 0) return KPD_OK;
  const int M = max_dets < D ? max_dets : D;
  const struct { const void* p; bool needed; const char* name; } arrays[] = {
      {pred_kpts, D > 0, "pred_kpts"},   {pred_scores, D > 0, "pred_scores"}, {gt_kpts, G > 0, "gt_kpts"},
      {gt_vis, G > 0, "gt_vis"},         {gt_boxes, G > 0, "gt_boxes"},       {gt_area, G > 0, "gt_area"},
      {n_gt, true, "n_gt"},              {scale, true, "scale"},              {sigmas, true, "sigmas"},
      {thresholds, true, "thresholds"},  {det_score, M > 0, "det_score"},     {det_slot, M > 0, "det_slot"},
      {det_match, M > 0, "det_match"},   {det_ignore, M > 0, "det_ignore"},   {gt_match, G > 0, "gt_match"},
      {counts, true, "counts"}};
  for (const auto& a : arrays)
    if (a.needed && !a.p) return fail(std::string(a.name) + " is null");
  OksTables tb{};
  for (int k = 0; k < K; ++k) tb.sigma[k] = sigmas[k];
  for (int t = 0; t < T; ++t) tb.thr[t] = thresholds[t];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int waves = T > 4 ? T : 4;
  hipLaunchKernelGGL(oks_match_kernel, dim3((unsigned)B), dim3(64 * waves), 0, st, pred_kpts, pred_scores, gt_kpts,
                     gt_vis, gt_boxes, gt_area, n_gt, scale, tb, D, G, K, T, M, oks, det_score, det_slot, det_match,
                     det_ignore, gt_match, counts);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_oks_match");
}
