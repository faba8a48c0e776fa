// Train-mode BatchNorm2d with the ReLU and the Dropout2d multiplier that follow
// it in the heatmap head (kpd_bn_train_forward / kpd_bn_train_backward,
// include/kpd.h): batch statistics, running-statistics update,
// forward and backward on NCHW fp32.  With n = N * H * W values per channel:
//
//   mean_c   = sum x / n            var_c = sum (x - mean_c)^2 / n   (biased)
//   invstd_c = 1 / sqrt(var_c + eps)                    (sums and these in double)
//   xhat = (x - mean_c) * invstd_c      pre = fmaf(xhat, gamma_c, beta_c)
//   y    = (relu ? max(pre, 0) : pre) * drop[n][c]
//   g      = gy * drop[n][c] * [pre > 0]
//   gbeta_c = sum g                 ggamma_c = sum g * xhat          (double)
//   gx   = gamma_c * invstd_c * (g - gbeta_c / n - xhat * ggamma_c / n)
//
// Pure memory traffic: two passes each way (forward: statistics, apply; x read
// twice, y written; backward: reduce, apply; x and gy read twice, gx written).
//
// Work split.  A channel's plane of image n is cut into P = ceil(H*W / 1024)
// chunks of 1024 values (256 threads x 4); the channel's S = N * P chunks, in
// (image, chunk) order, are dealt in contiguous runs to G = min(S, max(1,
// 4096 / C)) workgroups.  The reduction is therefore cut over (image, plane
// chunk): C = 64 or N = 1 still fill the CUs.  G depends on the shape alone,
// every workgroup adds its values in a fixed order into double partials
// (thread, wave shuffle, LDS), and one wave per channel adds the G partials in
// index order: no atomics, two calls on the same input are bit-identical.
// Workgroup ids run over the channels fastest, so the workgroups resident at
// one time read neighbouring planes of a few images -- a contiguous stretch
// of the tensor, as a linear sweep would -- and not one plane of every image.
//
// The variance comes from sums of d = x - K and d^2 in double, K = the
// channel's first value: exact for a constant channel (var = 0, mean = K), and
// free of the cancellation of sum x^2 - n mean^2 when the mean is many
// standard deviations from zero.
//
// 16-byte loads and stores when H*W % 4 == 0 and the tensors are 16-byte
// aligned; otherwise the same kernels with one value per access (thread t of a
// chunk takes values t, t + 256, t + 512, t + 768, which keeps the accesses
// coalesced).  Four chunks' loads are issued before the first use.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

namespace {

constexpr int kNT = 256, kChunk = 4 * kNT, kGroupBudget = 4096, kU = 4, kCoef = 8;

// P chunks per plane, S = N * P chunks per channel, G workgroups per channel
struct BnGeom {
  int C, HW, P, S, G;
};

// The one place xhat and the pre-activation are computed: the backward's ReLU
// mask [pre > 0] is bitwise the forward's.
__device__ __forceinline__ void bn_pre(float x, float mean, float invstd, float gamma, float beta, float* xhat,
                                       float* pre) {
  const float h = (x - mean) * invstd;
  *xhat = h;
  *pre = fmaf(h, gamma, beta);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The workgroup's two sums on thread 0 (waves added in index order).
__device__ __forceinline__ void block_sum2(double* a, double* b) {
  __shared__ double sh[kNT / 64][2];
  const double wa = wave_sum_d(*a), wb = wave_sum_d(*b);
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
    sh[t >> 6][0] = wa;
    sh[t >> 6][1] = wb;
  }
  __syncthreads();
  if (t == 0) {
    double sa = sh[0][0], sb = sh[0][1];
#pragma unroll
    for (int w = 1; w < kNT / 64; ++w) {
      sa += sh[w][0];
      sb += sh[w][1];
    }
    *a = sa;
    *b = sb;
  }
}

// Thread t's four values of one chunk: VEC values e0 + 4t .. 4t + 3 (one
// 16-byte access), else e0 + t + 256 k.  m = which of them lie in the plane.
template <bool VEC>
struct Tile {
  float v[4];
  unsigned m;
  __device__ __forceinline__ void load(const float* p, size_t plane, int e0, int HW, int t) {
    if (VEC) {
      const int e = e0 + 4 * t;
      m = e < HW ? 15u : 0u;
      f32x4 q = {0.f, 0.f, 0.f, 0.f};
      if (m) q = *reinterpret_cast<const f32x4*>(p + plane + e);
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
      m = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k * kNT + t;
        v[k] = 0.f;
        if (e < HW) {
          v[k] = p[plane + e];
          m |= 1u << k;
        }
      }
    }
  }
  __device__ __forceinline__ void store(float* p, size_t plane, int e0, int HW, int t) const {
    if (VEC) {
      const int e = e0 + 4 * t;
      if (e < HW) {
        const f32x4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p + plane + e) = q;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k * kNT + t;
        if (e < HW) p[plane + e] = v[k];
      }
    }
  }
};

// the run of chunks [s0, s1) of workgroup g
__device__ __forceinline__ void bn_run(const BnGeom& q, int g, int* s0, int* s1) {
  *s0 = (int)((long)g * q.S / q.G);
  *s1 = (int)((long)(g + 1) * q.S / q.G);
}

// grid C * G: partial sums of d = x - K and d^2 of the workgroup's run
template <bool VEC>
__global__ __launch_bounds__(kNT) void bn_stats_kernel(const float* __restrict__ x, BnGeom q,
                                                       double* __restrict__ part) {
  const int g = blockIdx.x / q.C, c = blockIdx.x - g * q.C, t = threadIdx.x;   // channel fastest
  int s0, s1;
  bn_run(q, g, &s0, &s1);
  const double K = (double)x[(size_t)c * q.HW];
  double a = 0.0, b = 0.0;
  for (int s = s0; s < s1; s += kU) {
    Tile<VEC> tl[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      tl[u].m = 0u;
      if (s + u < s1) {
        const int n = (s + u) / q.P, p = (s + u) - n * q.P;
        tl[u].load(x, ((size_t)n * q.C + c) * q.HW, p * kChunk, q.HW, t);
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((tl[u].m >> k) & 1u) {
          const double d = (double)tl[u].v[k] - K;
          a += d;
          b = fma(d, d, b);
        }
  }
  block_sum2(&a, &b);
  if (t == 0) {
    part[((size_t)c * q.G + g) * 2 + 0] = a;
    part[((size_t)c * q.G + g) * 2 + 1] = b;
  }
}

// one wave per channel: the G partials of channel c in index order
__device__ __forceinline__ void bn_channel_sums(const double* __restrict__ part, int c, int G, int lane, double* a,
                                                double* b) {
  double sa = 0.0, sb = 0.0;
  for (int g = lane; g < G; g += 64) {
    sa += part[((size_t)c * G + g) * 2 + 0];
    sb += part[((size_t)c * G + g) * 2 + 1];
  }
  *a = wave_sum_d(sa);
  *b = wave_sum_d(sb);
}

__global__ __launch_bounds__(kNT) void bn_stats_finish_kernel(const float* __restrict__ x,
                                                              const double* __restrict__ part, BnGeom q, double n,
                                                              double eps, double momentum, float* running_mean,
                                                              float* running_var, float* __restrict__ save_mean,
                                                              float* __restrict__ save_invstd) {
  const int c = blockIdx.x * (kNT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= q.C) return;
  double a, b;
  bn_channel_sums(part, c, q.G, lane, &a, &b);
  if (lane != 0) return;
  const double K = (double)x[(size_t)c * q.HW];
  const double m1 = a / n, mean = K + m1, var = fmax(b / n - m1 * m1, 0.0);
  save_mean[c] = (float)mean;
  save_invstd[c] = (float)(1.0 / sqrt(var + eps));
  if (running_mean) {
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * n / (n - 1.0)));
  }
}

template <bool VEC>
__global__ __launch_bounds__(kNT) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta,
                                                       const float* __restrict__ drop,
                                                       const float* __restrict__ save_mean,
                                                       const float* __restrict__ save_invstd, BnGeom q, int relu,
                                                       float* __restrict__ y) {
  const int g = blockIdx.x / q.C, c = blockIdx.x - g * q.C, t = threadIdx.x;   // channel fastest
  int s0, s1;
  bn_run(q, g, &s0, &s1);
  const float mean = save_mean[c], invstd = save_invstd[c];
  const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
  for (int s = s0; s < s1; s += kU) {
    Tile<VEC> tl[kU];
    float dm[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      tl[u].m = 0u;
      dm[u] = 1.f;
      if (s + u < s1) {
        const int n = (s + u) / q.P, p = (s + u) - n * q.P;
        tl[u].load(x, ((size_t)n * q.C + c) * q.HW, p * kChunk, q.HW, t);
        if (drop) dm[u] = drop[(size_t)n * q.C + c];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (s + u >= s1) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float xhat, pre;
        bn_pre(tl[u].v[k], mean, invstd, ga, be, &xhat, &pre);
        tl[u].v[k] = ((relu && !(pre > 0.f)) ? 0.f : pre) * dm[u];
      }
      const int n = (s + u) / q.P, p = (s + u) - n * q.P;
      tl[u].store(y, ((size_t)n * q.C + c) * q.HW, p * kChunk, q.HW, t);
    }
  }
}

// g and xhat of one value, as the backward's two passes both need them
__device__ __forceinline__ void bn_bwd_elem(float x, float gy, float dm, float mean, float invstd, float ga, float be,
                                            int relu, float* g, float* xhat) {
  float pre;
  bn_pre(x, mean, invstd, ga, be, xhat, &pre);
  *g = (relu && !(pre > 0.f)) ? 0.f : gy * dm;
}

// grid C * G: partial sums of g and g * xhat
template <bool VEC>
__global__ __launch_bounds__(kNT) void bn_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ drop,
                                                            const float* __restrict__ save_mean,
                                                            const float* __restrict__ save_invstd, BnGeom q, int relu,
                                                            double* __restrict__ part) {
  const int g = blockIdx.x / q.C, c = blockIdx.x - g * q.C, t = threadIdx.x;   // channel fastest
  int s0, s1;
  bn_run(q, g, &s0, &s1);
  const float mean = save_mean[c], invstd = save_invstd[c];
  const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
  double a = 0.0, b = 0.0;
  for (int s = s0; s < s1; s += kU / 2) {
    Tile<VEC> tx[kU / 2], tg[kU / 2];
    float dm[kU / 2];
#pragma unroll
    for (int u = 0; u < kU / 2; ++u) {
      tx[u].m = 0u;
      dm[u] = 1.f;
      if (s + u < s1) {
        const int n = (s + u) / q.P, p = (s + u) - n * q.P;
        const size_t plane = ((size_t)n * q.C + c) * q.HW;
        tx[u].load(x, plane, p * kChunk, q.HW, t);
        tg[u].load(gy, plane, p * kChunk, q.HW, t);
        if (drop) dm[u] = drop[(size_t)n * q.C + c];
      }
    }
#pragma unroll
    for (int u = 0; u < kU / 2; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((tx[u].m >> k) & 1u) {
          float gv, xhat;
          bn_bwd_elem(tx[u].v[k], tg[u].v[k], dm[u], mean, invstd, ga, be, relu, &gv, &xhat);
          a += (double)gv;
          b = fma((double)gv, (double)xhat, b);
        }
  }
  block_sum2(&a, &b);
  if (t == 0) {
    part[((size_t)c * q.G + g) * 2 + 0] = a;
    part[((size_t)c * q.G + g) * 2 + 1] = b;
  }
}

// one wave per channel: gbeta, ggamma and the apply pass's coefficients
// coef[c] = {gamma * invstd, gbeta / n, ggamma / n, and the fp32 remainders of
// the last two}, prepared in double.  The two means travel as hi + lo pairs:
// rounded once to fp32 they would shift every gx of the channel the same way,
// and sum gx over the channel -- the gradient of a convolution bias in front
// of the BN, zero in exact arithmetic -- would pick up n times that shift.
__global__ __launch_bounds__(kNT) void bn_bwd_finish_kernel(const double* __restrict__ part,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ save_invstd, BnGeom q, double n,
                                                            float* __restrict__ ggamma, float* __restrict__ gbeta,
                                                            float* __restrict__ coef) {
  const int c = blockIdx.x * (kNT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= q.C) return;
  double a, b;
  bn_channel_sums(part, c, q.G, lane, &a, &b);
  if (lane != 0) return;
  if (gbeta) gbeta[c] = (float)a;
  if (ggamma) ggamma[c] = (float)b;
  const double mb = a / n, mg = b / n;
  const float mb_hi = (float)mb, mg_hi = (float)mg;
  float* k = coef + (size_t)c * kCoef;
  k[0] = (float)((gamma ? (double)gamma[c] : 1.0) * (double)save_invstd[c]);
  k[1] = mb_hi;
  k[2] = mg_hi;
  k[3] = (float)(mb - (double)mb_hi);
  k[4] = (float)(mg - (double)mg_hi);
}

template <bool VEC>
__global__ __launch_bounds__(kNT) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ drop,
                                                           const float* __restrict__ save_mean,
                                                           const float* __restrict__ save_invstd,
                                                           const float* __restrict__ coef, BnGeom q, int relu,
                                                           float* __restrict__ gx) {
  const int g = blockIdx.x / q.C, c = blockIdx.x - g * q.C, t = threadIdx.x;   // channel fastest
  int s0, s1;
  bn_run(q, g, &s0, &s1);
  const float mean = save_mean[c], invstd = save_invstd[c];
  const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
  const float* kf = coef + (size_t)c * kCoef;
  const float ca = kf[0], cb = kf[1], cc = kf[2], cb_lo = kf[3], cc_lo = kf[4];
  for (int s = s0; s < s1; s += kU / 2) {
    Tile<VEC> tx[kU / 2], tg[kU / 2];
    float dm[kU / 2];
#pragma unroll
    for (int u = 0; u < kU / 2; ++u) {
      tx[u].m = 0u;
      dm[u] = 1.f;
      if (s + u < s1) {
        const int n = (s + u) / q.P, p = (s + u) - n * q.P;
        const size_t plane = ((size_t)n * q.C + c) * q.HW;
        tx[u].load(x, plane, p * kChunk, q.HW, t);
        tg[u].load(gy, plane, p * kChunk, q.HW, t);
        if (drop) dm[u] = drop[(size_t)n * q.C + c];
      }
    }
#pragma unroll
    for (int u = 0; u < kU / 2; ++u) {
      if (s + u >= s1) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float gv, xhat;
        bn_bwd_elem(tx[u].v[k], tg[u].v[k], dm[u], mean, invstd, ga, be, relu, &gv, &xhat);
        tg[u].v[k] = ca * (fmaf(-xhat, cc, gv - cb) - fmaf(xhat, cc_lo, cb_lo));
      }
      const int n = (s + u) / q.P, p = (s + u) - n * q.P;
      tg[u].store(gx, ((size_t)n * q.C + c) * q.HW, p * kChunk, q.HW, t);
    }
  }
}

int einval(const char* fn, const std::string& what) { return kpd_fail_einval((std::string(fn) + ": " + what).c_str()); }

// shape checks shared by the two entry points; fills the work split
int bn_geom(const char* fn, int N, int C, int H, int W, BnGeom* q) {
  if (N < 1) return einval(fn, "N must be at least 1");
  if (C < 1) return einval(fn, "C must be at least 1");
  if (H < 1) return einval(fn, "H must be at least 1");
  if (W < 1) return einval(fn, "W must be at least 1");
  const long long HW = (long long)H * W;
  if (HW >= (1ll << 31)) return einval(fn, "H * W must stay below 2^31");
  if ((long long)N * HW <= 1)
    return einval(fn, "expected more than 1 value per channel (N * H * W = 1)");
  const long long P = (HW + kChunk - 1) / kChunk, S = (long long)N * P;
  if (S >= (1ll << 31)) return einval(fn, "N * ceil(H * W / 1024) must stay below 2^31");
  const long long G = std::min<long long>(S, std::max(1, kGroupBudget / C));
  if ((long long)C * G >= (1ll << 31)) return einval(fn, "C is too large for the launch grid");
  q->C = C;
  q->HW = (int)HW;
  q->P = (int)P;
  q->S = (int)S;
  q->G = (int)G;
  return KPD_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

bool overlaps(const void* a, const void* b, size_t bytes) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" int kpd_bn_train_forward(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta,
                                    const float* drop, float eps, float momentum, float* running_mean,
                                    float* running_var, int flags, float* y, float* save_mean, float* save_invstd,
                                    void* stream) {
  static const char* fn = "kpd_bn_train_forward";
  BnGeom q{};
  if (const int rc = bn_geom(fn, N, C, H, W, &q)) return rc;
  if (!(eps > 0.f)) return einval(fn, "eps must be positive");
  if (!(momentum >= 0.f && momentum <= 1.f)) return einval(fn, "momentum must be in [0, 1]");
  if (!x) return einval(fn, "x is null");
  if (!y) return einval(fn, "y is null");
  if (!save_mean) return einval(fn, "save_mean is null");
  if (!save_invstd) return einval(fn, "save_invstd is null");
  if ((running_mean == nullptr) != (running_var == nullptr))
    return einval(fn, "running_mean and running_var must both be given or both be null");
  const size_t bytes = (size_t)N * C * q.HW * sizeof(float);
  if (overlaps(x, y, bytes)) return einval(fn, "y must not alias x (the backward reads x again)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&part), (size_t)C * q.G * 2 * sizeof(double), st);
  if (e != hipSuccess) return kpd_fail_hip(e, fn);
  const bool vec = q.HW % 4 == 0 && aligned16(x) && aligned16(y);
  const dim3 grid((unsigned)(C * q.G)), fin((unsigned)((C + kNT / 64 - 1) / (kNT / 64)));
  const double n = (double)N * q.HW;
  const int relu = (flags & KPD_BN_RELU) ? 1 : 0;
  if (vec) hipLaunchKernelGGL(bn_stats_kernel<true>, grid, dim3(kNT), 0, st, x, q, part);
  else hipLaunchKernelGGL(bn_stats_kernel<false>, grid, dim3(kNT), 0, st, x, q, part);
  hipLaunchKernelGGL(bn_stats_finish_kernel, fin, dim3(kNT), 0, st, x, part, q, n, (double)eps, (double)momentum,
                     running_mean, running_var, save_mean, save_invstd);
  if (vec)
    hipLaunchKernelGGL(bn_apply_kernel<true>, grid, dim3(kNT), 0, st, x, gamma, beta, drop, save_mean, save_invstd, q,
                       relu, y);
  else
    hipLaunchKernelGGL(bn_apply_kernel<false>, grid, dim3(kNT), 0, st, x, gamma, beta, drop, save_mean, save_invstd, q,
                       relu, y);
  e = hipGetLastError();
  const hipError_t ef = hipFreeAsync(part, st);
  if (e != hipSuccess) return kpd_fail_hip(e, fn);
  if (ef != hipSuccess) return kpd_fail_hip(ef, fn);
  return KPD_OK;
}

extern "C" int kpd_bn_train_backward(const float* x, const float* gy, int N, int C, int H, int W, const float* gamma,
                                     const float* beta, const float* drop, const float* save_mean,
                                     const float* save_invstd, int flags, float* gx, float* ggamma, float* gbeta,
                                     void* stream) {
  static const char* fn = "kpd_bn_train_backward";
  BnGeom q{};
  if (const int rc = bn_geom(fn, N, C, H, W, &q)) return rc;
  if (!x) return einval(fn, "x is null");
  if (!gy) return einval(fn, "gy is null");
  if (!save_mean) return einval(fn, "save_mean is null");
  if (!save_invstd) return einval(fn, "save_invstd is null");
  const size_t bytes = (size_t)N * C * q.HW * sizeof(float);
  if (gx && overlaps(gx, x, bytes)) return einval(fn, "gx must not alias x");
  if (gx && overlaps(gx, gy, bytes)) return einval(fn, "gx must not alias gy");
  if (!gx && !ggamma && !gbeta) return KPD_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t pb = ((size_t)C * q.G * 2 * sizeof(double) + 255) / 256 * 256;
  char* buf = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&buf), pb + (size_t)C * kCoef * sizeof(float), st);
  if (e != hipSuccess) return kpd_fail_hip(e, fn);
  double* part = reinterpret_cast<double*>(buf);
  float* coef = reinterpret_cast<float*>(buf + pb);
  const bool vec = q.HW % 4 == 0 && aligned16(x) && aligned16(gy) && (!gx || aligned16(gx));
  const dim3 grid((unsigned)(C * q.G)), fin((unsigned)((C + kNT / 64 - 1) / (kNT / 64)));
  const double n = (double)N * q.HW;
  const int relu = (flags & KPD_BN_RELU) ? 1 : 0;
  if (vec)
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, grid, dim3(kNT), 0, st, x, gy, gamma, beta, drop, save_mean,
                       save_invstd, q, relu, part);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, grid, dim3(kNT), 0, st, x, gy, gamma, beta, drop, save_mean,
                       save_invstd, q, relu, part);
  hipLaunchKernelGGL(bn_bwd_finish_kernel, fin, dim3(kNT), 0, st, part, gamma, save_invstd, q, n, ggamma, gbeta, coef);
  if (gx) {
    if (vec)
      hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, dim3(kNT), 0, st, x, gy, gamma, beta, drop, save_mean,
                         save_invstd, coef, q, relu, gx);
    else
      hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, dim3(kNT), 0, st, x, gy, gamma, beta, drop, save_mean,
                         save_invstd, coef, q, relu, gx);
  }
  e = hipGetLastError();
  const hipError_t ef = hipFreeAsync(buf, st);
  if (e != hipSuccess) return kpd_fail_hip(e, fn);
  if (ef != hipSuccess) return kpd_fail_hip(ef, fn);
  return KPD_OK;
}
