// Training the person detector on frozen trunk features (the
// reference has no detection loss, no anchor matching and no box encoding, so
// the rules are build-defined like the eval detector's, §C3, and pinned to
// tests/det_train_ref.py).
//
//   kpd_detector_targets   anchor matching, two launches:
//     det_gt_max_kernel    per-(image, GT) maximum IoU over the 28,224 anchors
//                          (atomicMax on the bits of the non-negative fp32 IoU:
//                          order-independent, so deterministic);
//     det_assign_kernel    per-anchor assignment (best GT, ignore band,
//                          low-quality matches within min(tie_eps, gmax / 2) of
//                          a GT's maximum) and the per-image positive count.
//   kpd_detector_loss      focal + smooth-L1 loss and the closed-form gradients
//                          of box_heads[0] / cls_heads[0], two launches:
//     det_loss_kernel      one pass over the pooled features [B][3136][128].
//                          Per block of 56 cells (one grid row, as
//                          person_detect_kernel): x staged in LDS, the 45 head
//                          columns on v_mfma_f32_16x16x4_f32 (exact fp32
//                          products), loss and dL/dy per anchor with the box
//                          targets encoded on the fly, then dL/dW += gy^T x on
//                          the same MFMA (K = cells) and dL/db, accumulated in
//                          registers across the row blocks a workgroup owns
//                          (block = workgroup + k * workgroups: a function of B
//                          alone).  Neither the head map nor its gradient goes
//                          through HBM;
//     det_reduce_kernel    the per-workgroup partials summed in index order in
//                          double and scaled by 1 / N, N = max(1, sum n_pos)
//                          read on the device.  No floating-point atomics.
//
// kpd_detector_features (the pooled features themselves: the forward's stages
// up to FPN level 0, then launch_adaptive_pool56) lives with the plan in
// kpd_plan.hip.
#include <algorithm>
#include <cmath>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int G56 = 56, GP = G56 * G56, NA = 9, A = GP * NA;   // 28,224 anchors in candidate order (i, j, a)
constexpr int kMaxGt = KPD_DET_MAX_GT;

// iou_cxcywh of nms.hip (oracle.kpd_oracle.box_iou_cxcywh), operation for operation
__device__ __forceinline__ float iou_cxcywh(float acx, float acy, float aw, float ah, float bcx, float bcy, float bw,
                                            float bh) {
  const float ax1 = acx - aw / 2.f, ay1 = acy - ah / 2.f, ax2 = acx + aw / 2.f, ay2 = acy + ah / 2.f;
  const float bx1 = bcx - bw / 2.f, by1 = bcy - bh / 2.f, bx2 = bcx + bw / 2.f, by2 = bcy + bh / 2.f;
  const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
  const float ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  const float inter = iw * ih;
  const float a1 = (ax2 - ax1) * (ay2 - ay1);
  const float a2 = (bx2 - bx1) * (by2 - by1);
  return inter / (a1 + a2 - inter + 1e-16f);
}

// a GT row is absent if all four values are 0, if w <= 0 or h <= 0, or if any value is NaN
__device__ __forceinline__ bool gt_present(float cx, float cy, float w, float h) {
  if (cx != cx || cy != cy || w != w || h != h) return false;
  if (cx == 0.f && cy == 0.f && w == 0.f && h == 0.f) return false;
  return w > 0.f && h > 0.f;
}

// the image's GT rows into LDS: box [G][4] and a presence flag; returns nothing before the caller's barrier
__device__ __forceinline__ void stage_gts(const float* __restrict__ gt, int G, float* sbox, int* spres) {
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    const float cx = gt[g * 4], cy = gt[g * 4 + 1], w = gt[g * 4 + 2], h = gt[g * 4 + 3];
    sbox[g * 4] = cx; sbox[g * 4 + 1] = cy; sbox[g * 4 + 2] = w; sbox[g * 4 + 3] = h;
    spres[g] = gt_present(cx, cy, w, h) ? 1 : 0;
  }
}

// grid (ceil(A / 256), B).  gt_best [B][G] zeroed by the caller.
__global__ __launch_bounds__(256) void det_gt_max_kernel(const float* __restrict__ anchors,
                                                         const float* __restrict__ gt_boxes, int G, float img_w,
                                                         float img_h, float* __restrict__ gt_best) {
  __shared__ float sbox[kMaxGt * 4];
  __shared__ int spres[kMaxGt];
  __shared__ unsigned smax[kMaxGt];
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  stage_gts(gt_boxes + (size_t)b * G * 4, G, sbox, spres);
  for (int g = threadIdx.x; g < G; g += 256) smax[g] = 0u;
  __syncthreads();
  const bool in = n < A;
  const int nn = in ? n : 0;
  const float ax = anchors[nn * 4], ay = anchors[nn * 4 + 1];
  const float aw = anchors[nn * 4 + 2] / img_w, ah = anchors[nn * 4 + 3] / img_h;
  for (int g = 0; g < G; ++g) {
    if (!spres[g]) continue;   // (uniform over the workgroup)
    float v = in ? iou_cxcywh(ax, ay, aw, ah, sbox[g * 4], sbox[g * 4 + 1], sbox[g * 4 + 2], sbox[g * 4 + 3]) : 0.f;
    if (!(v > 0.f)) v = 0.f;   // (NaN from an infinite box: no match)
    v = wave_max(v);
    if (lane == 0 && v > 0.f) atomicMax(&smax[g], __float_as_uint(v));
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256)
    if (smax[g]) atomicMax(reinterpret_cast<unsigned*>(gt_best) + (size_t)b * G + g, smax[g]);
}

// grid (ceil(A / 256), B).  n_pos [B] zeroed by the caller.
__global__ __launch_bounds__(256) void det_assign_kernel(const float* __restrict__ anchors,
                                                         const float* __restrict__ gt_boxes, int G, float img_w,
                                                         float img_h, float pos_thr, float neg_thr, float tie_eps,
                                                         const float* __restrict__ gt_best,
                                                         int32_t* __restrict__ assign, int32_t* __restrict__ n_pos) {
  __shared__ float sbox[kMaxGt * 4];
  __shared__ int spres[kMaxGt];
  __shared__ float sgmax[kMaxGt];
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  stage_gts(gt_boxes + (size_t)b * G * 4, G, sbox, spres);
  for (int g = threadIdx.x; g < G; g += 256) sgmax[g] = gt_best[(size_t)b * G + g];
  __syncthreads();
  const bool in = n < A;
  const int nn = in ? n : 0;
  const float ax = anchors[nn * 4], ay = anchors[nn * 4 + 1];
  const float aw = anchors[nn * 4 + 2] / img_w, ah = anchors[nn * 4 + 3] / img_h;
  float best = -1.f;
  int arg = -1;
  bool low = false;
  for (int g = 0; g < G; ++g) {
    if (!spres[g]) continue;
    float v = iou_cxcywh(ax, ay, aw, ah, sbox[g * 4], sbox[g * 4 + 1], sbox[g * 4 + 2], sbox[g * 4 + 3]);
    if (!(v > 0.f)) v = 0.f;
    if (v > best) { best = v; arg = g; }   // ties: the lower slot
    const float gm = sgmax[g];
    // the band is capped at half the maximum: a sub-pixel GT (gmax < tie_eps) claims its tie set, not every anchor
    if (gm > 0.f && v >= gm - fminf(tie_eps, gm / 2.f)) low = true;
  }
  int a = -1;
  if (arg >= 0) {
    if (best >= pos_thr) a = arg;
    else if (best >= neg_thr) a = -2;
    if (low) a = arg;
  }
  const bool pos = in && a >= 0;
  if (in) assign[(size_t)b * A + n] = a;
  const unsigned long long m = __ballot(pos);
  if (lane == 0 && m) atomicAdd(&n_pos[b], (int)__popcll(m));
}

// ---------------------------------------------------------------- loss
constexpr int kC = 128, kPP = 128 + 4, kHS = 49, kHC = 45, kRows = 64;   // LDS pitches: x [64][132], head / gy [64][49]
constexpr int kPartFloats = 48 * kC + 48;                                // one workgroup's gradient partial
constexpr int kLossMaxWg = 256;                                          // the grid's cap: block = wg + k * grid

// softplus(x) = log(1 + e^x), stable
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float pow_gamma(float q, float gamma) { return gamma == 2.f ? q * q : powf(q, gamma); }

__global__ __launch_bounds__(512) void det_loss_kernel(
    const float* __restrict__ pooled, const float* __restrict__ box_w, const float* __restrict__ box_b,
    const float* __restrict__ cls_w, const float* __restrict__ cls_b, const float* __restrict__ anchors,
    const float* __restrict__ gt_boxes, const int32_t* __restrict__ assign, int nblocks, int G, float img_w,
    float img_h, float alpha, float gamma, float beta, int want_grad, float* __restrict__ part,
    double* __restrict__ loss_part) {
  __shared__ __attribute__((aligned(16))) float pool[kRows * kPP];
  __shared__ float hg[kRows * kHS];   // the head outputs, overwritten in place by dL/dy (un-normalised)
  __shared__ float red[8][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r16 = lane & 15;
  // zero once what no later step writes: cell rows 56..63 of both maps and columns 45..48 of hg
  for (int it = tid; it < (kRows - G56) * kPP; it += 512) pool[G56 * kPP + it] = 0.f;
  for (int it = tid; it < kRows * kHS; it += 512) hg[it] = 0.f;
  f32x4 wacc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  double bacc = 0.0;           // (threads 0..44) dL/db of one head column over the workgroup's row blocks
  double lc = 0.0, lb = 0.0;   // (thread 0) the workgroup's class and box sums
  // row of the 48 x 128 head matrix: box_heads[0] ++ cls_heads[0], rows 45..47 zero
  auto wrow = [&](int col) -> const float* {
    return col < 36 ? box_w + (size_t)col * kC : (col < kHC ? cls_w + (size_t)(col - 36) * kC : nullptr);
  };
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int b = blk / G56, i = blk - b * G56;
    __syncthreads();   // the previous block's reads of pool / hg / red are done (and the zero fill above)
    // 1. x: the row's 56 cells, 32 float4 each
    const float* src = pooled + ((size_t)b * GP + (size_t)i * G56) * kC;
    for (int it = tid; it < G56 * 32; it += 512) {
      const int j = it >> 5, q = it & 31;
      *reinterpret_cast<float4*>(pool + j * kPP + q * 4) = *reinterpret_cast<const float4*>(src + (size_t)j * kC + q * 4);
    }
    __syncthreads();
    // 2. heads, as person_detect_kernel's step 3: waves 0-3 columns 0-31 of cell block w, 4-7 columns 32-47
    {
      const int rb = wave & 3, nb0 = wave < 4 ? 0 : 2, nnb = wave < 4 ? 2 : 1;
      const int row = rb * 16 + r16;
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kc = 0; kc < kC / 16; ++kc) {
        const float4 a = *reinterpret_cast<const float4*>(pool + row * kPP + kc * 16 + g * 4);   // rows >= 56 are zero
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if (n >= nnb) continue;
          const float* wr = wrow((nb0 + n) * 16 + r16);
          const float4 bw = wr ? *reinterpret_cast<const float4*>(wr + kc * 16 + g * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bw.x, acc[n], 0, 0, 0);
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bw.y, acc[n], 0, 0, 0);
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bw.z, acc[n], 0, 0, 0);
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bw.w, acc[n], 0, 0, 0);
        }
      }
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int col = (nb0 + n) * 16 + r16;
        if (n >= nnb || col >= kHC) continue;
        const float bb = col < 36 ? box_b[col] : cls_b[col - 36];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = rb * 16 + g * 4 + e;   // D: lane holds rows 4g + e of its block, column r16
          if (j < G56) hg[j * kHS + col] = acc[n][e] + bb;
        }
      }
    }
    __syncthreads();
    // 3. loss and dL/dy per anchor (thread = (cell j, anchor a)); its five head values become its five gradients
    float fl = 0.f, sl = 0.f;
    if (tid < G56 * NA) {
      const int j = tid / NA, a = tid - j * NA;
      const int anc = (i * G56 + j) * NA + a;
      float* h = hg + j * kHS;
      int asg = assign[(size_t)b * A + anc];
      // (never from kpd_detector_targets; keeps the GT read in bounds.  kpd.h: >= G acts as -2, < -2 as -1)
      if (asg >= G) asg = -2;
      const float z = h[36 + a];
      float gz = 0.f;
      if (asg != -2) {
        const float p = 1.f / (1.f + expf(-z)), q = 1.f / (1.f + expf(z));   // q = 1 - p without the cancellation
        if (asg >= 0) {
          const float logp = -softplus_f(-z), m = alpha * pow_gamma(q, gamma);
          fl = -m * logp;
          gz = m * (gamma * p * logp - q);
        } else {
          const float logq = -softplus_f(z), m = (1.f - alpha) * pow_gamma(p, gamma);
          fl = -m * logq;
          gz = m * (p - gamma * q * logq);
        }
      }
      h[36 + a] = gz;
      float gd[4] = {0.f, 0.f, 0.f, 0.f};
      if (asg >= 0) {
        const float* gb = gt_boxes + ((size_t)b * G + asg) * 4;
        const float ax = anchors[anc * 4], ay = anchors[anc * 4 + 1];
        const float aw = anchors[anc * 4 + 2] / img_w, ah = anchors[anc * 4 + 3] / img_h;
        const float t[4] = {(gb[0] - ax) / aw, (gb[1] - ay) / ah, logf(gb[2] / aw), logf(gb[3] / ah)};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float d = h[a * 4 + c] - t[c], ad = fabsf(d);
          if (ad < beta) {
            sl += 0.5f * d * d / beta;
            gd[c] = d / beta;
          } else {
            sl += ad - 0.5f * beta;
            gd[c] = d > 0.f ? 1.f : -1.f;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) h[a * 4 + c] = gd[c];
    }
    fl = wave_sum(fl);
    sl = wave_sum(sl);
    if (lane == 0) { red[wave][0] = fl; red[wave][1] = sl; }
    __syncthreads();
    if (tid == 0) {
      float c = 0.f, x = 0.f;
      for (int w = 0; w < 8; ++w) { c += red[w][0]; x += red[w][1]; }
      lc += (double)c;
      lb += (double)x;
    }
    if (want_grad) {
      // 4. dL/db: column sums over the row's cells; dL/dW += gy^T x, wave w owning input channels 16w .. 16w+15
      //    (the column sums in double: with near-constant logits, as after the bias initialisation, the 56 addends
      //    are almost equal and an fp32 running sum rounds the same way in every block -- 7e-7 of dL/db, §3j)
      if (tid < kHC) {
        double s0 = 0.0, s1 = 0.0;
        for (int j = 0; j < G56; j += 2) {
          s0 += (double)hg[j * kHS + tid];
          s1 += (double)hg[(j + 1) * kHS + tid];
        }
        bacc += s0 + s1;
      }
#pragma unroll
      for (int kk = 0; kk < kRows / 4; ++kk) {
        const int c = kk * 4 + g;   // lane (g, r16) supplies A[col r16][cell c] and B[cell c][channel r16]
        const float xv = pool[c * kPP + wave * 16 + r16];
#pragma unroll
        for (int mb = 0; mb < 3; ++mb)
          wacc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(hg[c * kHS + mb * 16 + r16], xv, wacc[mb], 0, 0, 0);
      }
    }
  }
  if (tid == 0) {
    loss_part[(size_t)blockIdx.x * 2] = lc;
    loss_part[(size_t)blockIdx.x * 2 + 1] = lb;
  }
  if (want_grad) {
    float* o = part + (size_t)blockIdx.x * kPartFloats;
#pragma unroll
    for (int mb = 0; mb < 3; ++mb)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[(mb * 16 + g * 4 + e) * kC + wave * 16 + r16] = wacc[mb][e];
    if (tid < 48) o[48 * kC + tid] = tid < kHC ? (float)bacc : 0.f;
  }
}

// One wave per workgroup.  Workgroups 0 .. kReduceBlocks-1: lane = gradient element e, summed over the loss
// kernel's workgroups in index order; the last workgroup: the loss (the partials staged through LDS by all
// lanes, then added in index order by lane 0 -- a lone thread reading them from memory one by one was the
// launch's whole time).  N from n_pos by an integer wave sum.
constexpr int kReduceBlocks = (kPartFloats + 63) / 64;
__global__ __launch_bounds__(64) void det_reduce_kernel(const float* __restrict__ part,
                                                        const double* __restrict__ loss_part, int nwg,
                                                        const int32_t* __restrict__ n_pos, int B, float box_weight,
                                                        float* __restrict__ loss, float* __restrict__ g_box_w,
                                                        float* __restrict__ g_box_b, float* __restrict__ g_cls_w,
                                                        float* __restrict__ g_cls_b) {
  __shared__ double sl[2 * kLossMaxWg];
  const int lane = threadIdx.x;
  int np = 0;   // (at most B * 28,224 < 2^31)
  for (int b = lane; b < B; b += 64) np += n_pos[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o, 64);
  const double N = (double)(np > 1 ? np : 1);
  if (blockIdx.x == kReduceBlocks) {
    for (int it = lane; it < 2 * nwg; it += 64) sl[it] = loss_part[it];
    __syncthreads();
    if (lane == 0) {
      double c = 0.0, x = 0.0;
      for (int w = 0; w < nwg; ++w) { c += sl[w * 2]; x += sl[w * 2 + 1]; }
      loss[0] = (float)((c + (double)box_weight * x) / N);
      loss[1] = (float)(c / N);
      loss[2] = (float)(x / N);
    }
    return;
  }
  const int e = blockIdx.x * 64 + lane;
  if (e >= kPartFloats) return;
  if (!part) return;
  const int row = e < 48 * kC ? e / kC : e - 48 * kC, k = e < 48 * kC ? e - row * kC : -1;
  if (row >= kHC) return;
  // 64 partials' loads in flight at a time (they are 24 KB apart), added in index order
  double s = 0.0;
  for (int w0 = 0; w0 < nwg; w0 += 64) {
    float v[64];
#pragma unroll
    for (int u = 0; u < 64; ++u) v[u] = w0 + u < nwg ? part[(size_t)(w0 + u) * kPartFloats + e] : 0.f;
#pragma unroll
    for (int u = 0; u < 64; ++u)
      if (w0 + u < nwg) s += (double)v[u];
  }
  const float v = (float)(row < 36 ? s * (double)box_weight / N : s / N);
  if (k >= 0) {
    if (row < 36) g_box_w[row * kC + k] = v;
    else g_cls_w[(row - 36) * kC + k] = v;
  } else {
    if (row < 36) g_box_b[row] = v;
    else g_cls_b[row - 36] = v;
  }
}

}  // namespace

extern "C" int kpd_detector_targets(const float* anchors, const float* gt_boxes, int B, int G, int img_h, int img_w,
                                    float pos_thr, float neg_thr, float tie_eps, int32_t* assign, int32_t* n_pos,
                                    float* gt_best, void* stream) {
  if (B <= 0) return kpd_fail_einval("kpd_detector_targets: B must be at least 1");
  if (G < 0 || G > kMaxGt) return kpd_fail_einval("kpd_detector_targets: G must be in [0, 64]");
  if (img_h <= 0 || img_w <= 0) return kpd_fail_einval("kpd_detector_targets: img_h and img_w must be positive");
  if (!anchors) return kpd_fail_einval("kpd_detector_targets: null anchors");
  if (G > 0 && !gt_boxes) return kpd_fail_einval("kpd_detector_targets: null gt_boxes with G > 0");
  if (!assign || !n_pos) return kpd_fail_einval("kpd_detector_targets: null assign or n_pos");
  if (!(pos_thr > 0.f) || !(pos_thr <= 1.f)) return kpd_fail_einval("kpd_detector_targets: pos_thr must be in (0, 1]");
  if (!(neg_thr >= 0.f) || !(neg_thr <= pos_thr))
    return kpd_fail_einval("kpd_detector_targets: neg_thr must be in [0, pos_thr]");
  if (!(tie_eps >= 0.f) || !std::isfinite(tie_eps))
    return kpd_fail_einval("kpd_detector_targets: tie_eps must be non-negative and finite");
  if ((long)B * A > 0x7fffffffL) return kpd_fail_einval("kpd_detector_targets: B too large");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(n_pos, 0, sizeof(int32_t) * B, st);
  if (e != hipSuccess) return kpd_fail_hip(e, "kpd_detector_targets");
  float* best = gt_best;
  const size_t bytes = sizeof(float) * (size_t)B * std::max(G, 1);
  if (!best) {
    e = hipMallocAsync(reinterpret_cast<void**>(&best), bytes, st);
    if (e != hipSuccess) return kpd_fail_hip(e, "kpd_detector_targets");
  }
  const dim3 grid((A + 255) / 256, B);
  if (G > 0) e = hipMemsetAsync(best, 0, bytes, st);
  if (e == hipSuccess && G > 0) {
    hipLaunchKernelGGL(det_gt_max_kernel, grid, dim3(256), 0, st, anchors, gt_boxes, G, (float)img_w, (float)img_h, best);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(det_assign_kernel, grid, dim3(256), 0, st, anchors, gt_boxes, G, (float)img_w, (float)img_h,
                       pos_thr, neg_thr, tie_eps, best, assign, n_pos);
    e = hipGetLastError();
  }
  if (!gt_best) (void)hipFreeAsync(best, st);
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_detector_targets");
}

extern "C" int kpd_detector_loss(const float* pooled, const float* box_w, const float* box_b, const float* cls_w,
                                 const float* cls_b, const float* anchors, const float* gt_boxes,
                                 const int32_t* assign, const int32_t* n_pos, int B, int G, int img_h, int img_w,
                                 float alpha, float gamma, float beta, float box_weight, float* loss, float* g_box_w,
                                 float* g_box_b, float* g_cls_w, float* g_cls_b, void* stream) {
  if (B <= 0) return kpd_fail_einval("kpd_detector_loss: B must be at least 1");
  if (G < 0 || G > kMaxGt) return kpd_fail_einval("kpd_detector_loss: G must be in [0, 64]");
  if (img_h <= 0 || img_w <= 0) return kpd_fail_einval("kpd_detector_loss: img_h and img_w must be positive");
  if (!pooled) return kpd_fail_einval("kpd_detector_loss: null pooled");
  if (!box_w || !box_b || !cls_w || !cls_b) return kpd_fail_einval("kpd_detector_loss: null head parameter");
  if (!anchors) return kpd_fail_einval("kpd_detector_loss: null anchors");
  if (G > 0 && !gt_boxes) return kpd_fail_einval("kpd_detector_loss: null gt_boxes with G > 0");
  if (!assign || !n_pos) return kpd_fail_einval("kpd_detector_loss: null assign or n_pos");
  if (!(alpha >= 0.f) || !(alpha <= 1.f)) return kpd_fail_einval("kpd_detector_loss: alpha must be in [0, 1]");
  if (!(gamma >= 0.f) || !std::isfinite(gamma)) return kpd_fail_einval("kpd_detector_loss: gamma must be non-negative and finite");
  if (!(beta > 0.f) || !std::isfinite(beta)) return kpd_fail_einval("kpd_detector_loss: beta must be positive and finite");
  if (!(box_weight >= 0.f) || !std::isfinite(box_weight))
    return kpd_fail_einval("kpd_detector_loss: box_weight must be non-negative and finite");
  if (!loss) return kpd_fail_einval("kpd_detector_loss: null loss");
  const int ng = (g_box_w != nullptr) + (g_box_b != nullptr) + (g_cls_w != nullptr) + (g_cls_b != nullptr);
  if (ng != 0 && ng != 4) return kpd_fail_einval("kpd_detector_loss: the four gradient outputs are given together or all NULL");
  if ((long)B * A > 0x7fffffffL) return kpd_fail_einval("kpd_detector_loss: B too large");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nblocks = B * G56, nwg = std::min(nblocks, kLossMaxWg), want = ng == 4;
  const size_t lbytes = sizeof(double) * 2 * nwg, pbytes = want ? sizeof(float) * (size_t)nwg * kPartFloats : 0;
  char* scratch = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&scratch), lbytes + pbytes, st);
  if (e != hipSuccess) return kpd_fail_hip(e, "kpd_detector_loss");
  double* lpart = reinterpret_cast<double*>(scratch);
  float* part = want ? reinterpret_cast<float*>(scratch + lbytes) : nullptr;
  hipLaunchKernelGGL(det_loss_kernel, dim3(nwg), dim3(512), 0, st, pooled, box_w, box_b, cls_w, cls_b, anchors,
                     gt_boxes, assign, nblocks, G, (float)img_w, (float)img_h, alpha, gamma, beta, want, part, lpart);
  e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(det_reduce_kernel, dim3(kReduceBlocks + 1), dim3(64), 0, st, part, lpart, nwg,
                       n_pos, B, box_weight, loss, g_box_w, g_box_b, g_cls_w, g_cls_b);
    e = hipGetLastError();
  }
  (void)hipFreeAsync(scratch, st);
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_detector_loss");
}
