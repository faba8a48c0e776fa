// OKS pose-NMS on the GPU (kpd_pose_nms): the object keypoint
// similarity of every pair of poses of an image and the suppression of a pose
// that is too similar to a higher-scoring one -- greedy (hard) or by score
// decay (soft, Gaussian or linear) -- one workgroup per image, straight from a
// forward's output tensors.
//
//   phase 0: per slot whether the pose is present (score > 0, which a NaN
//            fails).
//   phase 1: the D(D-1)/2 pairs i < j spread over the threads, each written to
//            both halves of the D x D matrix in LDS as doubles (bit-symmetric
//            by construction; the diagonal and every pair with an absent pose
//            are 0); ranks by a counting comparison under nms.hip's
//            better(score, index) rule.
//   phase 2: wave 0.  Hard: lane l holds the pose kept at position l; per pose
//            in rank order one ballot over the kept lanes whose OKS with it
//            exceeds the threshold -- the lowest set lane is the earliest-kept
//            suppressor; no set lane appends the pose.  Soft: lane = slot with
//            its current score; per pick a wave64 arg-max over the remaining
//            lanes (ties to the lower slot), then every remaining lane decays
//            its score by its OKS with the pick.
//   phase 3: the per-slot outputs from LDS, one slot per thread.
//
// Differences, sums of squares and score products are formed in double from
// the fp32 inputs with no contraction, in the operation order DESIGN.md §3d
// writes out; tests/pose_nms_ref.py follows it step for step, so the two
// differ only by the rounding of exp().
#include <string>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxK = KPD_POSE_NMS_MAX_K, kMaxD = KPD_POSE_NMS_MAX_D, kThreads = 256;
static_assert(kMaxD == 64, "one lane per slot in the suppression, one LDS matrix of 64 x 64 doubles");

struct PoseNmsTables {
  float sigma[kMaxK];
};

// better(a, b): a ranks before b in a descending sort with index tie-break (nms.hip)
__device__ __forceinline__ bool better(float sa, int ia, float sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// OKS of two present poses of one image; ci / cj = their keypoint confidences or null
__device__ double oks_pair(const float* __restrict__ ki, const float* __restrict__ kj, const float* __restrict__ ci,
                           const float* __restrict__ cj, double area_i, double area_j, double sx, double sy,
                           float vis_threshold, int K, const PoseNmsTables& tb) {
  const double eps = 2.220446049250313e-16;   // 2^-52, np.spacing(1)
  const double den = (area_i + area_j) / 2.0 + eps;
  double sum = 0.0;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    if (ci && !(ci[k] > vis_threshold && cj[k] > vis_threshold)) continue;
    const double dx = sx * (double)ki[2 * k] - sx * (double)kj[2 * k];
    const double dy = sy * (double)ki[2 * k + 1] - sy * (double)kj[2 * k + 1];
    const double s2 = 2.0 * (double)tb.sigma[k];
    const double var = s2 * s2;
    const double e = (dx * dx + dy * dy) / var / den / 2.0;
    sum += exp(-e);
    ++n;
  }
  return n > 0 ? sum / (double)n : 0.0;
}

// grid B, block 256
__global__ __launch_bounds__(kThreads) void pose_nms_kernel(
    const float* __restrict__ kpts, const float* __restrict__ scores, const float* __restrict__ area,
    const float* __restrict__ kconf, const float* __restrict__ scale, PoseNmsTables tb, int D, int K, int mode,
    float threshold, float vis_threshold, float min_score, int max_keep, double* __restrict__ oks_out,
    int32_t* __restrict__ keep, int32_t* __restrict__ n_keep, float* __restrict__ scores_out,
    int32_t* __restrict__ suppressed_by) {
  __shared__ double s_oks[kMaxD * kMaxD];   // [i][j], row stride D
  __shared__ float s_score[kMaxD];          // 0 for an absent slot
  __shared__ int s_order[kMaxD];            // caller slot at each rank, -1 past the present poses
  __shared__ int s_keep[kMaxD];             // caller slot at each keep position, -1 past n_keep
  __shared__ float s_out[kMaxD];            // scores_out of each slot
  __shared__ int s_sup[kMaxD];              // suppressed_by of each slot
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const double sx = scale[2 * b], sy = scale[2 * b + 1];

  // ---- phase 0
  if (tid < D) {
    const float s = scores[(size_t)b * D + tid];
    s_score[tid] = s > 0.f ? s : 0.f;
    s_order[tid] = -1;
    s_keep[tid] = -1;
    s_out[tid] = 0.f;
    s_sup[tid] = -1;
    s_oks[tid * D + tid] = 0.0;
    if (oks_out) oks_out[((size_t)b * D + tid) * D + tid] = 0.0;
  }
  __syncthreads();

  // ---- phase 1: the OKS matrix and the ranks
  const int npairs = D * (D - 1) / 2;
  for (int p = tid; p < npairs; p += kThreads) {
    int i = 0, q = p;   // pair p of the rows (0,1..D-1), (1,2..D-1), ...
    while (q >= D - 1 - i) {
      q -= D - 1 - i;
      ++i;
    }
    const int j = i + 1 + q;   // i < j < D
    double v = 0.0;   // a pair with an absent pose
    if (s_score[i] > 0.f && s_score[j] > 0.f) {
      const size_t ii = (size_t)b * D + i, jj = (size_t)b * D + j;
      v = oks_pair(kpts + ii * K * 2, kpts + jj * K * 2, kconf ? kconf + ii * K : nullptr,
                   kconf ? kconf + jj * K : nullptr, (double)area[ii], (double)area[jj], sx, sy, vis_threshold, K, tb);
    }
    s_oks[i * D + j] = v;
    s_oks[j * D + i] = v;
    if (oks_out) {
      oks_out[((size_t)b * D + i) * D + j] = v;
      oks_out[((size_t)b * D + j) * D + i] = v;
    }
  }
  if (tid < D && s_score[tid] > 0.f) {
    const float s = s_score[tid];
    int rank = 0;
    for (int d = 0; d < D; ++d) rank += s_score[d] > 0.f && better(s_score[d], d, s, tid);
    s_order[rank] = tid;   // rank < the number of present poses <= D
  }
  __syncthreads();

  // ---- phase 2: wave 0 suppresses
  if (tid < 64) {
    const double thr = (double)threshold;
    int nk = 0;   // wave-uniform
    if (mode == KPD_POSE_NMS_HARD) {
      int mine = -1;   // the pose kept at position `lane`
      for (int r = 0; r < D && nk < max_keep; ++r) {
        const int d = s_order[r];
        if (d < 0) break;
        const float sd = s_score[d];
        if (!(sd > min_score)) break;
        const bool over = lane < nk && s_oks[(lane < nk ? mine : 0) * D + d] > thr;
        const unsigned long long m = __ballot(over);
        if (m != 0ull) {
          const int first = __ffsll((long long)m) - 1;   // the earliest-kept pose over the threshold
          const int by = __shfl(mine, first, 64);
          if (lane == 0) s_sup[d] = by;
        } else {
          if (lane == nk) mine = d;
          if (lane == 0) {
            s_keep[nk] = d;
            s_out[d] = sd;
          }
          ++nk;
        }
      }
    } else {
      const bool present = lane < D && s_score[lane] > 0.f;
      bool remaining = present;
      double cur = present ? (double)s_score[lane] : 0.0;
      for (int it = 0; it < D && nk < max_keep; ++it) {
        double bo = remaining ? cur : -INFINITY;
        int bp = remaining ? lane : -1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double o2 = __shfl_xor(bo, off, 64);
          const int p2 = __shfl_xor(bp, off, 64);
          if (p2 >= 0 && (bp < 0 || o2 > bo || (o2 == bo && p2 < bp))) { bo = o2; bp = p2; }
        }
        bp = __shfl(bp, 0, 64);   // one winner for the wave whatever a non-finite score did to the comparisons
        if (bp < 0) break;
        bo = __shfl(cur, bp, 64);
        if (!(bo > (double)min_score)) break;
        if (lane == bp) {
          remaining = false;
          s_keep[nk] = bp;
          s_out[bp] = (float)bo;
        }
        ++nk;
        if (remaining) {
          const double o = s_oks[bp * D + lane];
          double decay;
          if (mode == KPD_POSE_NMS_SOFT) decay = exp(-(o * o) / thr);
          else decay = o >= thr ? 1.0 - o : 1.0;
          cur = cur * decay;
        }
      }
    }
    if (lane == 0) n_keep[b] = nk;
  }
  __syncthreads();

  // ---- phase 3
  if (tid < D) {
    const size_t o = (size_t)b * D + tid;
    keep[o] = s_keep[tid];
    scores_out[o] = s_out[tid];
    suppressed_by[o] = s_sup[tid];
  }
}

int fail(const std::string& what) { return kpd_fail_einval(("kpd_pose_nms: " + what).c_str()); }

}  // namespace

extern "C" int kpd_pose_nms(const float* kpts, const float* scores, const float* area, const float* kconf,
                            const float* scale, const float* sigmas, int B, int D, int K, int mode, float threshold,
                            float vis_threshold, float min_score, int max_keep, double* oks, int32_t* keep,
                            int32_t* n_keep, float* scores_out, int32_t* suppressed_by, void* stream) {
  if (B < 0) return fail("B must not be negative");
  if (D < 0 || D > kMaxD) return fail("D must be in [0, 64]");
  if (K < 1 || K > kMaxK) return fail("K must be in [1, 32]");
  if (mode != KPD_POSE_NMS_HARD && mode != KPD_POSE_NMS_SOFT && mode != KPD_POSE_NMS_SOFT_LINEAR)
    return fail("mode must be KPD_POSE_NMS_HARD, KPD_POSE_NMS_SOFT or KPD_POSE_NMS_SOFT_LINEAR");
  if (!(threshold > 0.f && threshold <= 1.f)) return fail("threshold must be in (0, 1]");
  if (vis_threshold != vis_threshold) return fail("vis_threshold must not be NaN");
  if (min_score != min_score) return fail("min_score must not be NaN");
  if (max_keep < 1) return fail("max_keep must be at least 1");
  if (B == 0) return KPD_OK;
  const struct { const void* p; bool needed; const char* name; } arrays[] = {
      {kpts, D > 0, "kpts"},     {scores, D > 0, "scores"},         {area, D > 0, "area"},
      {scale, true, "scale"},    {sigmas, true, "sigmas"},          {keep, D > 0, "keep"},
      {n_keep, true, "n_keep"},  {scores_out, D > 0, "scores_out"}, {suppressed_by, D > 0, "suppressed_by"}};
  for (const auto& a : arrays)
    if (a.needed && !a.p) return fail(std::string(a.name) + " is null");
  PoseNmsTables tb{};
  for (int k = 0; k < K; ++k) tb.sigma[k] = sigmas[k];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pose_nms_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, kpts, scores, area, kconf, scale, tb,
                     D, K, mode, threshold, vis_threshold, min_score, max_keep, oks, keep, n_keep, scores_out,
                     suppressed_by);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_pose_nms");
}
