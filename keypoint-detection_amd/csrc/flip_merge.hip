// Flip-test merge on the GPU (kpd_flip_merge): the heatmaps of
// a forward over the images (a) and of one over their left-right mirrors (b)
// are averaged -- b mirrored back, its left / right joint planes swapped -- and
// the average is decoded as decode_kernel (head_kernels.hip) decodes a
// forward's own heatmap: one launch, one wave per (person slot, keypoint)
// plane, each input plane read once.
//
//   m[k][y][x] = 0.5f * (a[k][y][x] + b[pairs[k]][y][W-1-x])
//
// The wave walks the plane in chunks of kChunk values per lane (all loads of a
// chunk issued before its first use), keeps a running maximum per lane and
// rescales the lane's exp-weighted sums once per chunk when the maximum grew
// (online softmax), then merges the 64 lanes: E[x], E[y] under softmax(m),
// the box transform and the visibility class follow decode_kernel line by line.
// The person slots are the forward's compacted ones: the wave derives the
// compaction of its image from the caller-order boxes by slotmap_kernel's rule
// (64 boxes per ballot), so no slot map travels between the calls.
#include <string>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

namespace {

constexpr int kMaxK = KPD_FLIP_MAX_K, kMaxSide = KPD_FLIP_MAX_SIDE, kChunk = 8;

struct FlipPairs {
  int32_t pair[kMaxK];
};

// grid (n * P output slots, K), one wave.  heat_a and heat_out may be the same
// memory (a lane writes only the elements it has read), so neither is restrict.
__global__ __launch_bounds__(64) void flip_merge_kernel(const float* heat_a, const float* __restrict__ heat_b,
                                                        const float* __restrict__ boxes, FlipPairs pr, int P, int H,
                                                        int W, float* heat_out, float* __restrict__ kpts_out,
                                                        float* __restrict__ vis_out, float* __restrict__ peaks) {
  const int r = blockIdx.x, k = blockIdx.y, K = gridDim.y, lane = threadIdx.x;
  const int img = r / P, q = r - img * P;   // output slot q of image img
  const int HW = H * W;

  // the image's compaction: cnt = its non-zero boxes, src = the caller row of the q-th of them
  int cnt = 0, src = -1;
  for (int base = 0; base < P; base += 64) {
    const int p = base + lane;
    bool nz = false;
    if (p < P) {
      const float* bx = boxes + ((size_t)img * P + p) * 4;
      const float b0 = bx[0], b1 = bx[1], b2 = bx[2], b3 = bx[3];   // four loads in flight, not a short-circuit chain
      nz = !(b0 == 0.f && b1 == 0.f && b2 == 0.f && b3 == 0.f);
    }
    const unsigned long long mask = __ballot(nz);
    const int before = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    const unsigned long long sel = __ballot(nz && before == q);
    if (sel != 0ull) src = base + __ffsll((long long)sel) - 1;
    cnt += __popcll(mask);
  }

  const size_t o = (size_t)r * K + k;
  if (q >= cnt) {   // padding slot: zeros; the dummy person of a box-less image is visibility class 0
    if (heat_out) {
      float* po = heat_out + o * HW;
      for (int i = lane; i < HW; i += 64) po[i] = 0.f;
    }
    if (lane == 0) {
      kpts_out[o * 2 + 0] = 0.f;
      kpts_out[o * 2 + 1] = 0.f;
      vis_out[o * 3 + 0] = (cnt == 0 && q == 0) ? 1.f : 0.f;
      vis_out[o * 3 + 1] = 0.f;
      vis_out[o * 3 + 2] = 0.f;
      if (peaks) peaks[o] = 0.f;
    }
    return;
  }

  const float* pa = heat_a + o * HW;
  const float* pb = heat_b + ((size_t)r * K + pr.pair[k]) * HW;
  float* po = heat_out ? heat_out + o * HW : nullptr;
  // element i = lane + 64 t of the plane sits at (y, x); a step of 64 elements moves it by (dy, dx)
  const int dx = 64 % W, dy = 64 / W;
  int x = lane % W, y = lane / W;
  float m = -INFINITY, se = 0.f, sx = 0.f, sy = 0.f;
  for (int i0 = lane; i0 < HW; i0 += 64 * kChunk) {
    float v[kChunk], fx[kChunk], fy[kChunk];
#pragma unroll
    for (int t = 0; t < kChunk; ++t) {
      const int i = i0 + 64 * t;
      // loads past the plane are clamped into it, not branched around: every load of the chunk is in flight at once
      const float va = pa[min(i, HW - 1)], vb = pb[min(y * W + (W - 1 - x), HW - 1)];
      v[t] = i < HW ? 0.5f * (va + vb) : -INFINITY;
      fx[t] = (float)x;
      fy[t] = (float)y;
      x += dx;
      y += dy;
      if (x >= W) {
        x -= W;
        ++y;
      }
    }
    if (po) {
#pragma unroll
      for (int t = 0; t < kChunk; ++t) {
        const int i = i0 + 64 * t;
        if (i < HW) po[i] = v[t];
      }
    }
    float cm = v[0];   // i0 < HW: the chunk's first value is real
#pragma unroll
    for (int t = 1; t < kChunk; ++t) cm = fmaxf(cm, v[t]);
    if (cm > m) {   // one rescale per chunk; the first chunk scales zeros by exp(-inf) = 0
      const float s = expf(m - cm);
      se *= s;
      sx *= s;
      sy *= s;
      m = cm;
    }
#pragma unroll
    for (int t = 0; t < kChunk; ++t) {
      const float e = expf(v[t] - m);   // 0 for the -inf of an element past the plane
      se += e;
      sx = fmaf(e, fx[t], sx);
      sy = fmaf(e, fy[t], sy);
    }
  }
  // the lanes' partial sums brought to the wave maximum; a lane without elements contributes 0
  const float M = wave_max(m);
  const float s = lane < HW ? expf(m - M) : 0.f;
  se = wave_sum(se * s);
  sx = wave_sum(sx * s);
  sy = wave_sum(sy * s);
  if (lane == 0) {
    const float* bx = boxes + ((size_t)img * P + src) * 4;
    const float cx = bx[0], cy = bx[1], bw = bx[2], bh = bx[3];
    const float kx = W > 1 ? (sx / se) / (float)(W - 1) : 0.f;
    const float ky = H > 1 ? (sy / se) / (float)(H - 1) : 0.f;
    kpts_out[o * 2 + 0] = fminf(fmaxf(kx * bw + (cx - bw / 2.f), 0.f), 1.f);
    kpts_out[o * 2 + 1] = fminf(fmaxf(ky * bh + (cy - bh / 2.f), 0.f), 1.f);
    const float conf = kpd_sigmoid(M);
    // compared as decode_kernel does: the fp32 confidence as a double against 0.3 / 0.7
    const int cls = (double)conf < 0.3 ? 0 : ((double)conf < 0.7 ? 1 : 2);
    vis_out[o * 3 + 0] = cls == 0 ? 1.f : 0.f;
    vis_out[o * 3 + 1] = cls == 1 ? 1.f : 0.f;
    vis_out[o * 3 + 2] = cls == 2 ? 1.f : 0.f;
    if (peaks) peaks[o] = M;
  }
}

int fail(const std::string& what) { return kpd_fail_einval(("kpd_flip_merge: " + what).c_str()); }

}  // namespace

extern "C" int kpd_flip_merge(const float* heat_a, const float* heat_b, const float* boxes, const int32_t* pairs,
                              int n, int P, int K, int H, int W, float* heat_out, float* keypoints,
                              float* visibilities, float* peaks, void* stream) {
  if (n < 0) return fail("n must not be negative");
  if (P < 1) return fail("P must be at least 1");
  if (K < 1 || K > kMaxK) return fail("K must be in [1, 32]");
  if (H < 1 || H > kMaxSide) return fail("H must be in [1, 1024]");
  if (W < 1 || W > kMaxSide) return fail("W must be in [1, 1024]");
  if ((long long)n * P > 0x7FFFFFFFll) return fail("n * P must fit the launch grid (2^31 - 1 slots)");
  if (!pairs) return fail("pairs is null");
  FlipPairs pr{};
  for (int k = 0; k < K; ++k) {
    if (pairs[k] < 0 || pairs[k] >= K) return fail("pairs[" + std::to_string(k) + "] is not in [0, K)");
    pr.pair[k] = pairs[k];
  }
  for (int k = 0; k < K; ++k)
    if (pairs[pairs[k]] != k) return fail("pairs is not an involution at " + std::to_string(k));
  if (n == 0) return KPD_OK;
  const struct { const void* p; const char* name; } arrays[] = {
      {heat_a, "heat_a"}, {heat_b, "heat_b"}, {boxes, "boxes"}, {keypoints, "keypoints"},
      {visibilities, "visibilities"}};
  for (const auto& a : arrays)
    if (!a.p) return fail(std::string(a.name) + " is null");
  if (heat_out) {
    const size_t bytes = (size_t)n * P * K * H * W * sizeof(float);
    const auto overlaps = [&](const float* other) {
      const char *lo = reinterpret_cast<const char*>(heat_out), *ot = reinterpret_cast<const char*>(other);
      return lo < ot + bytes && ot < lo + bytes;
    };
    if (overlaps(heat_b)) return fail("heat_out overlaps heat_b (only heat_a may be merged in place)");
    if (heat_out != heat_a && overlaps(heat_a)) return fail("heat_out overlaps heat_a without being equal to it");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(flip_merge_kernel, dim3((unsigned)(n * P), (unsigned)K), dim3(64), 0, st, heat_a, heat_b, boxes,
                     pr, P, H, W, heat_out, keypoints, visibilities, peaks);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_flip_merge");
}
