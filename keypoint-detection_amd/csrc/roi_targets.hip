// Per-ROI training targets of the top-down HeatmapHead.
//
// The head sees one ROI and predicts an H x W map of that ROI, so its target
// is the person's own joints placed in the ROI's frame, by the convention of
// the decoders and convert_to_original_coords: map pixel i stands for
// i / (W - 1) of the unclamped box.  For output row j (ROI r = rows[j], or j)
// and joint k, in fp32 with no contraction:
//   bx = cx - w/2, by = cy - h/2;  u = (x - bx) / w, v = (y - by) / h
//   on = w > 0 && h > 0 && vis > 0 && 0 <= u <= 1 && 0 <= v <= 1   (NaN: off)
//   weight = on ? 1 : 0;  px = u * (W - 1), py = v * (H - 1)
//   heat[y][x] = on ? expf(-((x - px)^2 + (y - py)^2) / (2 sigma^2)) : 0
// the reference's _convert_keypoints_to_heatmaps Gaussian (peak 1 at a
// sub-pixel centre, no cut-off) per ROI.  One launch, one thread per four
// consecutive pixels of a row (HBM-bound: the output is the only traffic), no
// host table and no synchronisation.
#include <cmath>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void roi_targets_kernel(const float* __restrict__ kpts,
                                                          const float* __restrict__ vis,
                                                          const float* __restrict__ boxes,
                                                          const int32_t* __restrict__ rows, long planes, int K, int H,
                                                          int W, float den, float* __restrict__ heat,
                                                          float* __restrict__ weight) {
  const int Wq = (W + 3) / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= planes * H * Wq) return;
  const int xq = (int)(i % Wq), y = (int)((i / Wq) % H);
  const long p = i / ((long)Wq * H);   // output plane j * K + k
  const long j = p / K;
  const int k = (int)(p - j * K);
  const long r = rows ? (long)rows[j] : j;
  const float* b = boxes + 4 * r;
  const float cx = b[0], cy = b[1], w = b[2], h = b[3];
  const float x = kpts[(r * K + k) * 2], yy = kpts[(r * K + k) * 2 + 1], vs = vis[r * K + k];
  const float bx = cx - w / 2.f, by = cy - h / 2.f;
  const float u = (x - bx) / w, v = (yy - by) / h;
  const bool on = w > 0.f && h > 0.f && vs > 0.f && u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f;   // NaN: off
  const float px = u * (float)(W - 1), py = v * (float)(H - 1);
  if (xq == 0 && y == 0) weight[p] = on ? 1.f : 0.f;
  const float dy = (float)y - py;
  const float dy2 = dy * dy;
  float o4[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float dx = (float)(xq * 4 + t) - px;
    o4[t] = on ? expf(-(dx * dx + dy2) / den) : 0.f;
  }
  float* o = heat + ((size_t)p * H + y) * W + xq * 4;
  if ((W & 3) == 0) {
    *reinterpret_cast<float4*>(o) = make_float4(o4[0], o4[1], o4[2], o4[3]);
  } else {
    for (int t = 0; t < 4 && xq * 4 + t < W; ++t) o[t] = o4[t];
  }
}

}  // namespace

extern "C" int kpd_roi_targets(const float* kpts, const float* vis, const float* boxes, const int32_t* rows, int n,
                               int R, int K, int H, int W, float sigma, float* heat, float* weight, void* stream) {
  if (n < 0 || R < 0 || K <= 0) return kpd_fail_einval("kpd_roi_targets: n, R must be >= 0 and K > 0");
  if (H < 2 || W < 2) return kpd_fail_einval("kpd_roi_targets: H and W must be at least 2");
  if (!(sigma > 0.f) || !std::isfinite(sigma)) return kpd_fail_einval("kpd_roi_targets: sigma must be positive and finite");
  if (n > 0 && (!kpts || !vis || !boxes || !heat || !weight)) return kpd_fail_einval("kpd_roi_targets: null pointer");
  if (n > 0 && R == 0) return kpd_fail_einval("kpd_roi_targets: rows requested of an empty ROI set");
  if (!rows && n > R) return kpd_fail_einval("kpd_roi_targets: n exceeds R without a row list");
  if (n == 0) return KPD_OK;
  const long planes = (long)n * K, threads = planes * H * ((W + 3) / 4);
  if (threads > 0x7fffffffL * 256) return kpd_fail_einval("kpd_roi_targets: output too large for one launch");
  const float den = 2.f * sigma * sigma;
  hipLaunchKernelGGL(roi_targets_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), kpts, vis, boxes, rows, planes, K, H, W, den, heat, weight);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_roi_targets");
}
