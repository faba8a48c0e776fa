// Training-side coordinate loss: the reference's
// SpatialCoordinateLoss (dll/losses/keypoint_loss.py:117-199) applied to the
// soft-argmax decode of every heatmap plane (decode_heatmaps_soft_argmax,
// dll/models/heatmap_head.py:372-413), with its gradient with respect to the
// plane in the same pass, and the decode's own backward.
//
// Per plane (r, k), x = 0..W-1, y = 0..H-1:
//   z_i  = (h_i - max h) / T,  a_i = exp(z_i),  A = sum a_i
//   px   = sum a_i x_i / A,  py = sum a_i y_i / A            (pixels)
//   e    = (px / (W-1), py / (H-1))                          the decoded coordinate
//   l    = rho(e_x - g_x) + rho(e_y - g_y),  d = |e - g|,  f = clamp(d / tau, 1, 3)
//   term = S f l                       (vis > 0; else 0, by selection)
//   L    = sum term / (N_vis + 1e-8)
//   G    = S / (N_vis + 1e-8) (f rho' + l df/de),  df/de = (e - g) / (d tau) in 1 < d/tau < 3, else 0
//   dL/dh_i = a_i / (A T) ((x_i - px) G_x / (W-1) + (y_i - py) G_y / (H-1))
//
// One wave owns one plane and reduces with cross-lane moves only: no LDS, no
// barrier, WAVES planes per workgroup.  The production 56 x 56 plane is 784
// float4 = 12.25 per lane: it stays in 52 registers between its one read and
// its one write (coord_plane_kernel<.., true>); any other H x W >= 2 x 2 takes
// the same arithmetic in three strided passes over the plane, which its L2
// serves after the first.  The three sums of a plane and the per-plane scalar
// chain run in double (a few hundred lane-operations per plane), so what is
// left of the fp32 rounding is the exponential's and the last one to float.
// N_vis depends on vis alone (count_vis_kernel, an integer), so no pass over
// the heatmaps crosses planes; the scalar loss is a fixed-order double sum of
// the per-plane terms (coord_final_kernel).  No floating-point atomics: two
// calls on the same inputs are bit-identical.
#include <cstdint>
#include <cmath>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

namespace {

constexpr int WAVES = 4, NT = WAVES * 64;   // planes per workgroup, threads
constexpr int FAST_H = 56, FAST_W = 56;     // the register-resident plane
constexpr int FAST_V4 = FAST_H * FAST_W / 4;          // 784 float4
constexpr int FAST_ROUNDS = (FAST_V4 + 63) / 64;      // 13, the last one on lanes 0..15
constexpr int RED_NT = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int lo = __shfl_xor(__double2loint(v), o, 64), hi = __shfl_xor(__double2hiint(v), o, 64);
    v += __hiloint2double(hi, lo);
  }
  return v;
}

// vis > 0 over all planes; one workgroup, integers
__global__ __launch_bounds__(RED_NT) void count_vis_kernel(const float* __restrict__ vis, int planes,
                                                           int* __restrict__ n_vis) {
  __shared__ int red[RED_NT];
  int c = 0;
  for (int i = threadIdx.x; i < planes; i += RED_NT) c += vis[i] > 0.f ? 1 : 0;
  red[threadIdx.x] = c;
  __syncthreads();
  for (int w = RED_NT / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_vis = red[0];
}

__device__ __forceinline__ double rho(double z, int type) {
  if (type == KPD_COORD_MSE) return z * z;
  const double a = fabs(z);
  return a < 1.0 ? 0.5 * z * z : a - 0.5;
}
__device__ __forceinline__ double drho(double z, int type) {
  if (type == KPD_COORD_MSE) return 2.0 * z;
  return fabs(z) < 1.0 ? z : (z > 0.0 ? 1.0 : -1.0);
}

struct CoordArgs {
  const float* heat;
  const float* gt;        // LOSS: [planes][2]
  const float* vis;       // LOSS: [planes]
  const float* gcoords;   // BACKWARD: [planes][2]
  const int* n_vis;       // LOSS
  float* coords;          // LOSS: [planes][2]
  float* terms;           // LOSS: [planes]
  float* grad;            // nullable in LOSS
  int planes, H, W, loss_type;
  float T, scale, tau;
};

// The gradient seed (G_x / (W-1), G_y / (H-1)) of one plane from its decoded
// pixel expectation; LOSS also writes the plane's coordinate and loss term.
// Every lane computes the same values; lane 0 stores.
template <bool LOSS>
__device__ __forceinline__ bool plane_seed(const CoordArgs& a, int plane, int lane, double px, double py, float* gx,
                                           float* gy) {
  const double rw = 1.0 / (double)(a.W - 1), rh = 1.0 / (double)(a.H - 1);
  if constexpr (!LOSS) {
    *gx = (float)((double)a.gcoords[2 * plane + 0] * rw);
    *gy = (float)((double)a.gcoords[2 * plane + 1] * rh);
    return true;
  } else {
    const double ex = px * rw, ey = py * rh;
    const bool seen = a.vis[plane] > 0.f;
    double term = 0.0, Gx = 0.0, Gy = 0.0;
    if (seen) {   // selection: a masked joint's gt (arbitrary, NaN) is never read into the arithmetic
      const double dx = ex - (double)a.gt[2 * plane + 0], dy = ey - (double)a.gt[2 * plane + 1];
      const double l = rho(dx, a.loss_type) + rho(dy, a.loss_type);
      const double d = sqrt(dx * dx + dy * dy), q = d / (double)a.tau;
      const double f = fmin(fmax(q, 1.0), 3.0);
      const double S = (double)a.scale;
      term = S * f * l;
      const double sn = S / ((double)*a.n_vis + 1e-8);
      const bool band = q > 1.0 && q < 3.0;
      const double dfx = band ? dx / (d * (double)a.tau) : 0.0, dfy = band ? dy / (d * (double)a.tau) : 0.0;
      Gx = sn * (f * drho(dx, a.loss_type) + l * dfx);
      Gy = sn * (f * drho(dy, a.loss_type) + l * dfy);
    }
    if (lane == 0) {
      a.coords[2 * plane + 0] = (float)ex;
      a.coords[2 * plane + 1] = (float)ey;
      a.terms[plane] = (float)term;
    }
    *gx = (float)(Gx * rw);
    *gy = (float)(Gy * rh);
    return seen;
  }
}

template <bool LOSS, bool FAST>
__global__ __launch_bounds__(NT) void coord_plane_kernel(const CoordArgs a) {
  const int lane = threadIdx.x & 63;
  const long plane_l = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (plane_l >= a.planes) return;   // wave-uniform; nothing below crosses waves
  const int plane = (int)plane_l;
  const int H = FAST ? FAST_H : a.H, W = FAST ? FAST_W : a.W;
  const int hw = H * W;
  const float* hp = a.heat + (size_t)plane * hw;
  float* gp = a.grad ? a.grad + (size_t)plane * hw : nullptr;
  const float inv_t = (float)(1.0 / (double)a.T);
  double sa = 0.0, sx = 0.0, sy = 0.0;
  float gx, gy;

  if constexpr (FAST) {
    const float4* hp4 = reinterpret_cast<const float4*>(hp);   // plane stride 12544 B: 16-byte aligned
    float4 v[FAST_ROUNDS];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < FAST_ROUNDS; ++j) {
      const int q = j * 64 + lane;
      v[j] = q < FAST_V4 ? hp4[q] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      m = fmaxf(fmaxf(fmaxf(m, v[j].x), fmaxf(v[j].y, v[j].z)), v[j].w);
    }
    m = wave_max(m);
#pragma unroll
    for (int j = 0; j < FAST_ROUNDS; ++j) {
      const int q = j * 64 + lane;                    // a float4 never straddles a row: 56 = 14 x 4
      const int y = q / (FAST_W / 4), x0 = (q - y * (FAST_W / 4)) * 4;
      v[j].x = expf((v[j].x - m) * inv_t);            // exp(-inf) = 0 on the lanes past the plane
      v[j].y = expf((v[j].y - m) * inv_t);
      v[j].z = expf((v[j].z - m) * inv_t);
      v[j].w = expf((v[j].w - m) * inv_t);
      const float r = (v[j].x + v[j].y) + (v[j].z + v[j].w);
      const float rx = (v[j].y + 2.f * v[j].z) + 3.f * v[j].w;    // sum a_c c, c = 0..3
      sa += (double)r;
      sx += (double)r * (double)x0 + (double)rx;
      sy += (double)r * (double)y;
    }
    sa = wave_sum_f64(sa);
    sx = wave_sum_f64(sx);
    sy = wave_sum_f64(sy);
    const double px = sx / sa, py = sy / sa;
    const bool seen = plane_seed<LOSS>(a, plane, lane, px, py, &gx, &gy);
    if (!gp) return;
    float4* gp4 = reinterpret_cast<float4*>(gp);
    const float c = seen ? (float)(1.0 / (sa * (double)a.T)) : 0.f;
    const float fpx = (float)px, fpy = (float)py;
#pragma unroll
    for (int j = 0; j < FAST_ROUNDS; ++j) {
      const int q = j * 64 + lane;
      if (q >= FAST_V4) continue;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (seen) {
        const int y = q / (FAST_W / 4), x0 = (q - y * (FAST_W / 4)) * 4;
        const float by = ((float)y - fpy) * gy, xr = (float)x0 - fpx;
        o.x = v[j].x * c * fmaf(xr, gx, by);
        o.y = v[j].y * c * fmaf(xr + 1.f, gx, by);
        o.z = v[j].z * c * fmaf(xr + 2.f, gx, by);
        o.w = v[j].w * c * fmaf(xr + 3.f, gx, by);
      }
      gp4[q] = o;
    }
  } else {
    float m = -INFINITY;
    for (int i = lane; i < hw; i += 64) m = fmaxf(m, hp[i]);
    m = wave_max(m);
    for (int i = lane; i < hw; i += 64) {
      const float e = expf((hp[i] - m) * inv_t);
      const int y = i / W, x = i - y * W;
      sa += (double)e;
      sx += (double)e * (double)x;
      sy += (double)e * (double)y;
    }
    sa = wave_sum_f64(sa);
    sx = wave_sum_f64(sx);
    sy = wave_sum_f64(sy);
    const double px = sx / sa, py = sy / sa;
    const bool seen = plane_seed<LOSS>(a, plane, lane, px, py, &gx, &gy);
    if (!gp) return;
    const float c = (float)(1.0 / (sa * (double)a.T));
    const float fpx = (float)px, fpy = (float)py;
    for (int i = lane; i < hw; i += 64) {
      float o = 0.f;
      if (seen) {
        const int y = i / W, x = i - y * W;
        o = expf((hp[i] - m) * inv_t) * c * fmaf((float)x - fpx, gx, ((float)y - fpy) * gy);
      }
      gp[i] = o;
    }
  }
}

// loss = (sum of the per-plane terms, in index order per thread then a fixed tree) / (N_vis + 1e-8)
__global__ __launch_bounds__(RED_NT) void coord_final_kernel(const float* __restrict__ terms, int planes,
                                                             const int* __restrict__ n_vis,
                                                             float* __restrict__ loss) {
  __shared__ double red[RED_NT];
  double s = 0.0;
  for (int i = threadIdx.x; i < planes; i += RED_NT) s += (double)terms[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = RED_NT / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / ((double)*n_vis + 1e-8));
}

template <bool LOSS>
void launch_planes(const CoordArgs& a, hipStream_t st) {
  const unsigned grid = (unsigned)(((long)a.planes + WAVES - 1) / WAVES);
  // the float4 path needs 16-byte aligned planes (a view at an odd element offset takes the generic one)
  const bool aligned = ((reinterpret_cast<uintptr_t>(a.heat) | reinterpret_cast<uintptr_t>(a.grad)) & 15u) == 0;
  if (a.H == FAST_H && a.W == FAST_W && aligned)
    hipLaunchKernelGGL((coord_plane_kernel<LOSS, true>), dim3(grid), dim3(NT), 0, st, a);
  else
    hipLaunchKernelGGL((coord_plane_kernel<LOSS, false>), dim3(grid), dim3(NT), 0, st, a);
}

bool bad_plane_shape(int planes, int H, int W, float T) {
  return planes < 0 || H < 2 || W < 2 || !(T > 0.f) || !(T < INFINITY) || (long)H * W >= (1L << 31);
}

}  // namespace

extern "C" int kpd_coord_loss(const float* heat, const float* gt, const float* vis, int planes, int H, int W,
                              float temperature, int loss_type, float pixel_weight_scale, float distance_threshold,
                              float* coords, float* loss, float* grad, void* stream) {
  if (bad_plane_shape(planes, H, W, temperature) || !loss || !(distance_threshold > 0.f) ||
      !(distance_threshold < INFINITY) || !(fabsf(pixel_weight_scale) < INFINITY) ||
      (loss_type != KPD_COORD_SMOOTH_L1 && loss_type != KPD_COORD_MSE && loss_type != KPD_COORD_HUBER) ||
      (planes > 0 && (!heat || !gt || !vis || !coords)))
    return kpd_fail_einval("kpd_coord_loss: bad arguments");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (planes == 0) {
    hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), st);
    return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_coord_loss");
  }
  // scratch: the per-plane terms, then N_vis
  const size_t terms_bytes = (sizeof(float) * (size_t)planes + 15) & ~(size_t)15;
  char* ws = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&ws), terms_bytes + sizeof(int), st);
  if (e != hipSuccess) return kpd_fail_hip(e, "kpd_coord_loss alloc");
  CoordArgs a{};
  a.heat = heat;
  a.gt = gt;
  a.vis = vis;
  a.terms = reinterpret_cast<float*>(ws);
  a.n_vis = reinterpret_cast<int*>(ws + terms_bytes);
  a.coords = coords;
  a.grad = grad;
  a.planes = planes;
  a.H = H;
  a.W = W;
  a.loss_type = loss_type;
  a.T = temperature;
  a.scale = pixel_weight_scale;
  a.tau = distance_threshold;
  hipLaunchKernelGGL(count_vis_kernel, dim3(1), dim3(RED_NT), 0, st, vis, planes, reinterpret_cast<int*>(ws + terms_bytes));
  launch_planes<true>(a, st);
  hipLaunchKernelGGL(coord_final_kernel, dim3(1), dim3(RED_NT), 0, st, a.terms, planes, a.n_vis, loss);
  e = hipGetLastError();
  (void)hipFreeAsync(ws, st);
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_coord_loss");
}

extern "C" int kpd_softargmax_backward(const float* heat, const float* grad_coords, int planes, int H, int W,
                                       float temperature, float* grad_heat, void* stream) {
  if (bad_plane_shape(planes, H, W, temperature) || (planes > 0 && (!heat || !grad_coords || !grad_heat)))
    return kpd_fail_einval("kpd_softargmax_backward: bad arguments");
  if (planes == 0) return KPD_OK;
  CoordArgs a{};
  a.heat = heat;
  a.gcoords = grad_coords;
  a.grad = grad_heat;
  a.planes = planes;
  a.H = H;
  a.W = W;
  a.T = temperature;
  launch_planes<false>(a, reinterpret_cast<hipStream_t>(stream));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_softargmax_backward");
}
