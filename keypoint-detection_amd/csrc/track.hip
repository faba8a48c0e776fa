// OKS pose tracking across frames on the GPU (kpd_track_poses):
// greedy OKS association of each frame's poses with the live tracks of its
// sequence and a One-Euro filter per joint along each track -- one workgroup
// per sequence, the frames of the call in a loop inside it, the state carried
// from call to call in a caller-owned device buffer.
//
//   start:   the sequence's track table (last matched raw pose of each of the
//            64 entries, its area and scale, id, age, hits) from the state
//            buffer into LDS.
//   per frame
//   phase A: per slot whether the pose is present (score > 0, which a NaN
//            fails).
//   phase B: the 64 x D matrix OKS(track entry, slot) spread over the threads,
//            in LDS as doubles, [slot][entry]; 0 for a dead entry or an absent
//            slot.
//   phase C: wave 0, lane = table entry.  Every unmatched live lane keeps its
//            best unmatched slot over the threshold (ties to the lower slot;
//            rescanned only when another track took it); per pick one wave64
//            arg-max over the lanes (ties to the lower track id).  Then the
//            ages, the deaths, and the births: the r-th unmatched present slot
//            takes the r-th free entry (ballots and popcounts).
//   phase D: thread p owns the elements (entry, joint) = p, p + 256, ... in
//            every frame: the matched or born pose becomes the entry's last
//            pose (LDS) and runs through the entry's filter state (state
//            buffer, double); per-slot outputs; untracked slots pass through.
//   end:     the table back into the state buffer.
//
// This kernel is latency-bound by construction: a sequential dependency over
// frames on one CU per sequence.  What it buys is the host round trip it
// removes, not throughput.
//
// OKS terms, the greedy comparisons and the filter are formed in double from
// the fp32 inputs with no contraction, in the operation order DESIGN.md §3m
// writes out; tests/track_ref.py follows it step for step.
#include <cmath>
#include <string>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxT = KPD_TRACK_MAX_T, kMaxD = KPD_TRACK_MAX_D, kMaxK = KPD_TRACK_MAX_K, kThreads = 256;
static_assert(kMaxT == 64 && kMaxD == 64, "one lane per table entry, one 64-bit mask of slots, 64 x 64 doubles in LDS");
constexpr int kPoseStride = 2 * kMaxK + 1, kConfStride = kMaxK + 1;   // odd LDS row strides: lane = entry reads spread over the banks

struct TrackParams {
  float sigma[kMaxK];
  float threshold, vis_threshold, min_cutoff, beta, d_cutoff, fps;
  int max_age, smooth;
};

// One sequence's state (include/kpd.h): byte offsets for K keypoints
struct StateLayout {
  size_t filt, kpts, kconf, valid, live, id, age, hits, area, sx, sy, next_id, bytes;
  __host__ __device__ explicit StateLayout(int K) {
    const size_t tk = (size_t)kMaxT * K;
    filt = 0;                        // double [T][K][2 coords][x^, dx^]
    kpts = filt + tk * 4 * 8;        // float  [T][K][2]
    kconf = kpts + tk * 2 * 4;       // float  [T][K]
    valid = kconf + tk * 4;          // int32  [T][K]
    live = valid + tk * 4;           // int32  [T] each
    id = live + kMaxT * 4;
    age = id + kMaxT * 4;
    hits = age + kMaxT * 4;
    area = hits + kMaxT * 4;         // float  [T] each
    sx = area + kMaxT * 4;
    sy = sx + kMaxT * 4;
    next_id = sy + kMaxT * 4;        // int32 next id, int32 frames seen, 8 bytes of padding
    bytes = next_id + 16;
  }
};

// OKS of a track's last matched pose (LDS) and a present pose of the current frame
__device__ double oks_track_pose(const float* tk, const float* tc, const float* __restrict__ kj,
                                 const float* __restrict__ cj, double area_t, double area_j, double tsx, double tsy,
                                 double sx, double sy, float vis_threshold, int K, const TrackParams& pr) {
  const double eps = 2.220446049250313e-16;   // 2^-52
  const double den = (area_t + area_j) / 2.0 + eps;
  double sum = 0.0;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    if (cj && !(tc[k] > vis_threshold && cj[k] > vis_threshold)) continue;
    const double dx = tsx * (double)tk[2 * k] - sx * (double)kj[2 * k];
    const double dy = tsy * (double)tk[2 * k + 1] - sy * (double)kj[2 * k + 1];
    const double s2 = 2.0 * (double)pr.sigma[k];
    const double var = s2 * s2;
    const double e = (dx * dx + dy * dy) / var / den / 2.0;
    sum += exp(-e);
    ++n;
  }
  return n > 0 ? sum / (double)n : 0.0;
}

__device__ __forceinline__ double euro_alpha(double fc, double te) {
  const double r = 2.0 * 3.141592653589793 * fc * te;
  return r / (r + 1.0);
}

// grid S, block 256
__global__ __launch_bounds__(kThreads) void track_kernel(
    const float* __restrict__ kpts, const float* __restrict__ scores, const float* __restrict__ area,
    const float* __restrict__ kconf, const float* __restrict__ scale, TrackParams pr, int B, int D, int K,
    unsigned char* __restrict__ state, int32_t* __restrict__ track_id, int32_t* __restrict__ track_hits,
    double* __restrict__ track_oks, float* __restrict__ kpts_out, int32_t* __restrict__ counts) {
  __shared__ double s_oks[kMaxD * kMaxT];            // [slot][entry]
  __shared__ float s_tk[kMaxT * kPoseStride];        // last matched raw pose of each entry
  __shared__ float s_tc[kMaxT * kConfStride];        // ... and its keypoint confidences
  __shared__ int s_live[kMaxT], s_id[kMaxT], s_age[kMaxT], s_hits[kMaxT];
  __shared__ float s_area[kMaxT], s_sx[kMaxT], s_sy[kMaxT];
  __shared__ int s_tslot[kMaxT];                     // the slot matched or born to the entry in this frame, -1: none
  __shared__ int s_tstep[kMaxT];                     // frames since its last match (age before + 1); 0 for a born track
  __shared__ int s_present[kMaxD], s_strack[kMaxD];  // per slot: present; its table entry or -1
  __shared__ double s_soks[kMaxD];                   // per slot: the OKS of its match
  __shared__ int s_next;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const StateLayout L(K);
  unsigned char* st = state + (size_t)s * L.bytes;
  double* g_filt = reinterpret_cast<double*>(st + L.filt);
  float* g_kpts = reinterpret_cast<float*>(st + L.kpts);
  float* g_kconf = reinterpret_cast<float*>(st + L.kconf);
  int32_t* g_valid = reinterpret_cast<int32_t*>(st + L.valid);
  int32_t* g_head = reinterpret_cast<int32_t*>(st + L.next_id);

  // ---- start
  for (int p = tid; p < kMaxT * K; p += kThreads) {
    const int t = p / K, k = p - t * K;
    s_tk[t * kPoseStride + 2 * k] = g_kpts[2 * p];
    s_tk[t * kPoseStride + 2 * k + 1] = g_kpts[2 * p + 1];
    s_tc[t * kConfStride + k] = g_kconf[p];
  }
  if (tid < kMaxT) {
    s_live[tid] = reinterpret_cast<const int32_t*>(st + L.live)[tid];
    s_id[tid] = reinterpret_cast<const int32_t*>(st + L.id)[tid];
    s_age[tid] = reinterpret_cast<const int32_t*>(st + L.age)[tid];
    s_hits[tid] = reinterpret_cast<const int32_t*>(st + L.hits)[tid];
    s_area[tid] = reinterpret_cast<const float*>(st + L.area)[tid];
    s_sx[tid] = reinterpret_cast<const float*>(st + L.sx)[tid];
    s_sy[tid] = reinterpret_cast<const float*>(st + L.sy)[tid];
  }
  if (tid == 0) s_next = g_head[0];
  __syncthreads();

  for (int f = 0; f < B; ++f) {
    const size_t fr = (size_t)s * B + f;   // frame index of the call
    const float fsx = scale[2 * fr], fsy = scale[2 * fr + 1];
    const double sx = fsx, sy = fsy;

    // ---- phase A
    if (tid < D) {
      const float sc = scores[fr * D + tid];
      s_present[tid] = sc > 0.f ? 1 : 0;
      s_strack[tid] = -1;
      s_soks[tid] = 0.0;
    }
    if (tid < kMaxT) {
      s_tslot[tid] = -1;
      s_tstep[tid] = 0;
    }
    __syncthreads();

    // ---- phase B: the OKS matrix
    for (int p = tid; p < kMaxT * D; p += kThreads) {
      const int t = p & (kMaxT - 1), j = p >> 6;   // a wave shares the slot: its pose is one broadcast read
      double v = 0.0;
      if (s_live[t] && s_present[j]) {
        const size_t jj = fr * D + j;
        v = oks_track_pose(s_tk + t * kPoseStride, s_tc + t * kConfStride, kpts + jj * K * 2,
                           kconf ? kconf + jj * K : nullptr, (double)s_area[t], (double)area[jj], (double)s_sx[t],
                           (double)s_sy[t], sx, sy, pr.vis_threshold, K, pr);
      }
      s_oks[j * kMaxT + t] = v;
    }
    __syncthreads();

    // ---- phase C: wave 0 associates, ages, frees and gives birth
    if (tid < 64) {
      const double thr = (double)pr.threshold;
      const int t = lane;
      bool live = s_live[t] != 0;
      int myid = s_id[t], age = s_age[t], hits = s_hits[t];
      bool open = live;                  // live and unmatched
      unsigned long long taken = 0ull;   // matched slots, wave-uniform
      int bj = -1, myslot = -1, nmatch = 0;
      double bo = 0.0, myoks = 0.0;
      bool stale = true;
      for (int it = 0; it < kMaxT; ++it) {   // at most min(64, D) picks
        if (open && stale) {
          bj = -1;
          bo = 0.0;
          for (int j = 0; j < D; ++j) {
            if ((taken >> j) & 1ull) continue;
            const double o = s_oks[j * kMaxT + t];   // 0 for an absent slot: never > thr >= 0
            if (o > thr && (bj < 0 || o > bo)) { bo = o; bj = j; }
          }
          stale = false;
        }
        const bool cand = open && bj >= 0;
        double ro = cand ? bo : -1.0;
        int rid = cand ? myid : 0x7fffffff, rl = cand ? lane : -1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double o2 = __shfl_xor(ro, off, 64);
          const int id2 = __shfl_xor(rid, off, 64);
          const int l2 = __shfl_xor(rl, off, 64);
          if (l2 >= 0 && (rl < 0 || o2 > ro || (o2 == ro && id2 < rid))) { ro = o2; rid = id2; rl = l2; }
        }
        rl = __shfl(rl, 0, 64);   // one winner for the wave
        if (rl < 0) break;
        const int wj = __shfl(bj, rl, 64);
        taken |= 1ull << wj;
        if (lane == rl) {
          open = false;
          myslot = wj;
          myoks = bo;
        } else if (bj == wj) {
          stale = true;
        }
        ++nmatch;
      }
      int step = 0;
      if (myslot >= 0) {
        step = age + 1;
        age = 0;
        hits += 1;
      } else if (live) {
        age += 1;
        if (age > pr.max_age) live = false;
      }
      const unsigned long long pmask = __ballot(lane < D && s_present[lane < D ? lane : 0] != 0);
      const unsigned long long umask = pmask & ~taken;   // unmatched present slots
      const unsigned long long fmask = __ballot(!live);  // free entries, those freed just now included
      const int nfree = __popcll(fmask), nun = __popcll(umask);
      const int born = nfree < nun ? nfree : nun;
      const int next = s_next;
      if (!live) {
        const int r = __popcll(fmask & ((1ull << lane) - 1ull));
        if (r < born) {   // the r-th unmatched slot in slot order takes the r-th free entry
          unsigned long long m = umask;
          for (int i = 0; i < r; ++i) m &= m - 1ull;
          myslot = __ffsll((long long)m) - 1;
          myoks = 0.0;
          live = true;
          myid = next + r;
          age = 0;
          hits = 1;
          step = 0;
        }
      }
      const int nlive = __popcll(__ballot(live));
      s_live[t] = live ? 1 : 0;
      s_id[t] = myid;
      s_age[t] = age;
      s_hits[t] = hits;
      s_tslot[t] = myslot;
      s_tstep[t] = step;
      if (myslot >= 0) {
        s_strack[myslot] = t;
        s_soks[myslot] = myoks;
      }
      if (lane == 0) {
        s_next = next + born;
        counts[fr * 4 + 0] = nmatch;
        counts[fr * 4 + 1] = born;
        counts[fr * 4 + 2] = nun - born;
        counts[fr * 4 + 3] = nlive;
      }
    }
    __syncthreads();

    // ---- phase D: the matched and born poses into the table and through the filters; the outputs
    for (int p = tid; p < kMaxT * K; p += kThreads) {
      const int t = p / K, k = p - t * K;
      const int j = s_tslot[t];
      if (j < 0) continue;
      const size_t jj = fr * D + j;
      const float x = kpts[(jj * K + k) * 2], y = kpts[(jj * K + k) * 2 + 1];
      const float c = kconf ? kconf[jj * K + k] : 0.f;
      s_tk[t * kPoseStride + 2 * k] = x;
      s_tk[t * kPoseStride + 2 * k + 1] = y;
      s_tc[t * kConfStride + k] = c;
      if (k == 0) {
        s_area[t] = area[jj];
        s_sx[t] = fsx;
        s_sy[t] = fsy;
      }
      if (!pr.smooth) continue;
      float ox = x, oy = y;
      if (kconf && !(c > pr.vis_threshold)) {
        g_valid[p] = 0;   // a joint that does not count passes through and loses its filter state
      } else {
        const int step = s_tstep[t];
        const bool has = step > 0 && g_valid[p] != 0;
        double* fs = g_filt + (size_t)p * 4;
        const double te = (double)step / (double)pr.fps;
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
          const double sc = c2 ? sy : sx;
          const double v = (double)(c2 ? y : x) * sc;
          double xh = v, dxh = 0.0;
          if (has) {
            const double xp = fs[2 * c2], dp = fs[2 * c2 + 1];
            const double dx = (v - xp) / te;
            const double ad = euro_alpha((double)pr.d_cutoff, te);
            dxh = ad * dx + (1.0 - ad) * dp;
            const double fc = (double)pr.min_cutoff + (double)pr.beta * fabs(dxh);
            const double a = euro_alpha(fc, te);
            xh = a * v + (1.0 - a) * xp;
          }
          fs[2 * c2] = xh;
          fs[2 * c2 + 1] = dxh;
          const float o = (float)(xh / sc);
          if (c2) oy = o; else ox = o;
        }
        g_valid[p] = 1;
      }
      kpts_out[(jj * K + k) * 2] = ox;
      kpts_out[(jj * K + k) * 2 + 1] = oy;
    }
    if (tid < D) {
      const int t = s_strack[tid];
      track_id[fr * D + tid] = t >= 0 ? s_id[t] : -1;
      track_hits[fr * D + tid] = t >= 0 ? s_hits[t] : 0;
      if (track_oks) track_oks[fr * D + tid] = s_soks[tid];
    }
    if (pr.smooth) {
      for (int q = tid; q < D * K; q += kThreads) {   // absent slots and poses without a track pass through
        const int j = q / K;
        if (s_strack[j] >= 0) continue;
        const size_t o = (fr * D * K + q) * 2;
        kpts_out[o] = kpts[o];
        kpts_out[o + 1] = kpts[o + 1];
      }
    }
    __syncthreads();
  }

  // ---- end
  for (int p = tid; p < kMaxT * K; p += kThreads) {
    const int t = p / K, k = p - t * K;
    g_kpts[2 * p] = s_tk[t * kPoseStride + 2 * k];
    g_kpts[2 * p + 1] = s_tk[t * kPoseStride + 2 * k + 1];
    g_kconf[p] = s_tc[t * kConfStride + k];
  }
  if (tid < kMaxT) {
    reinterpret_cast<int32_t*>(st + L.live)[tid] = s_live[tid];
    reinterpret_cast<int32_t*>(st + L.id)[tid] = s_id[tid];
    reinterpret_cast<int32_t*>(st + L.age)[tid] = s_age[tid];
    reinterpret_cast<int32_t*>(st + L.hits)[tid] = s_hits[tid];
    reinterpret_cast<float*>(st + L.area)[tid] = s_area[tid];
    reinterpret_cast<float*>(st + L.sx)[tid] = s_sx[tid];
    reinterpret_cast<float*>(st + L.sy)[tid] = s_sy[tid];
  }
  if (tid == 0) {
    g_head[0] = s_next;
    g_head[1] += B;
  }
}

int fail(const std::string& what) { return kpd_fail_einval(("kpd_track_poses: " + what).c_str()); }

}  // namespace

extern "C" size_t kpd_track_state_bytes(int K) {
  if (K < 1 || K > kMaxK) return 0;
  return StateLayout(K).bytes;
}

extern "C" int kpd_track_poses(const float* kpts, const float* scores, const float* area, const float* kconf,
                               const float* scale, const float* sigmas, int S, int B, int D, int K, float threshold,
                               float vis_threshold, int max_age, int smooth, float min_cutoff, float beta,
                               float d_cutoff, float fps, void* state, int32_t* track_id, int32_t* track_hits,
                               double* track_oks, float* kpts_out, int32_t* counts, void* stream) {
  if (S < 0) return fail("S must not be negative");
  if (B < 0) return fail("B must not be negative");
  if (D < 0 || D > kMaxD) return fail("D must be in [0, 64]");
  if (K < 1 || K > kMaxK) return fail("K must be in [1, 32]");
  if (!(threshold >= 0.f && threshold < 1.f)) return fail("threshold must be in [0, 1)");
  if (vis_threshold != vis_threshold) return fail("vis_threshold must not be NaN");
  if (max_age < 0) return fail("max_age must not be negative");
  if (smooth) {
    if (!(min_cutoff > 0.f && std::isfinite(min_cutoff))) return fail("min_cutoff must be positive and finite");
    if (!(beta >= 0.f && std::isfinite(beta))) return fail("beta must be finite and not negative");
    if (!(d_cutoff > 0.f && std::isfinite(d_cutoff))) return fail("d_cutoff must be positive and finite");
    if (!(fps > 0.f && std::isfinite(fps))) return fail("fps must be positive and finite");
  }
  if (S == 0 || B == 0) return KPD_OK;
  const struct { const void* p; bool needed; const char* name; } arrays[] = {
      {kpts, D > 0, "kpts"},         {scores, D > 0, "scores"},         {area, D > 0, "area"},
      {scale, true, "scale"},        {sigmas, true, "sigmas"},          {state, true, "state"},
      {track_id, D > 0, "track_id"}, {track_hits, D > 0, "track_hits"}, {kpts_out, smooth && D > 0, "kpts_out"},
      {counts, true, "counts"}};
  for (const auto& a : arrays)
    if (a.needed && !a.p) return fail(std::string(a.name) + " is null");
  TrackParams pr{};
  for (int k = 0; k < K; ++k) pr.sigma[k] = sigmas[k];
  pr.threshold = threshold;
  pr.vis_threshold = vis_threshold;
  pr.min_cutoff = min_cutoff;
  pr.beta = beta;
  pr.d_cutoff = d_cutoff;
  pr.fps = fps;
  pr.max_age = max_age;
  pr.smooth = smooth ? 1 : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(track_kernel, dim3((unsigned)S), dim3(kThreads), 0, st, kpts, scores, area, kconf, scale, pr, B, D,
                     K, static_cast<unsigned char*>(state), track_id, track_hits, track_oks, kpts_out, counts);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_track_poses");
}
