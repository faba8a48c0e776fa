// Training augmentation on the GPU (kpd_augment_batch): a batch
// of uint8 HWC images warped by a per-image affine map (mirror, rotation,
// zoom) with optional gain / offset, and the labels moved with the pixels.
//
//   tiles:   one 256-thread workgroup per KPD_AUG_TILE_W x KPD_AUG_TILE_H
//            output tile, four consecutive pixels of a row per thread.  The
//            64-bit source coordinate is formed once per thread and stepped by
//            q00 / q10 along the row; the bilinear taps are fetched straight
//            through the vector cache from indices clamped into the image (a
//            tap outside takes the fill colour by a select, so every load is
//            in bounds and in flight at once), the two taps of a source row
//            by one unaligned load; the four pixels leave as whole dwords
//            when the row address allows.
//   labels:  extra workgroups of the same launch behind the chunk's tiles,
//            ceil(P * (K + 1) / 256) per image: one thread per (person,
//            joint) and one per (person, box), float64 arithmetic.
//
// Images and their parameters are addressed through a descriptor table that
// travels by value in the kernel arguments, one table (one launch) per chunk
// of KPD_AUG_CHUNK images.  The image rule is integer arithmetic and
// tests/augment_ref.py restates it in numpy bit for bit.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kChunk = KPD_AUG_CHUNK, kTW = KPD_AUG_TILE_W, kTH = KPD_AUG_TILE_H;
constexpr int kMaxK = KPD_AUG_MAX_K, kMaxSide = KPD_AUG_MAX_SIDE;
static_assert(kTW == 64 && kTH == 16, "augment_kernel maps 256 threads to 16 rows of 16 four-pixel groups");

struct AImg {
  const unsigned char* src;
  unsigned char* dst;
  int H, W, pitch;
  int tiles_x;
  int tile0;   // tiles of the chunk's images before this one: workgroup id -> (image, tile)
  int q[6];    // inverse map, Q16, pixel-index coordinates
  int gain, offset, mirror;
  double N[6];   // forward map, normalised coordinates
};
static_assert(sizeof(AImg) == 120, "sixteen descriptors stay well inside the kernel-argument segment");

struct ATable {
  AImg d[kChunk];
};

struct AStyle {
  unsigned char pair[kMaxK];
  unsigned char fill[4];
};

// bytes of one tap-pair load: two horizontally adjacent pixels (2 * C bytes) fit it
template <int C>
struct Pair {
  using word = unsigned long long;
};
template <>
struct Pair<1> {
  using word = unsigned;
};

// The two horizontally adjacent taps of one source row in ONE unaligned load: byte 0 of the result is pixel
// cx0's first channel and pixel cx0 + 1 follows at byte C.  The load address is clamped to `last` (the image's
// last byte + 1 - sizeof(word)) and the word shifted down by the difference, so no byte outside the image is
// read: pixel cx0 ends at most at the image's end, which bounds the shift by sizeof(word) - C bytes, and where
// pixel cx0 + 1 exists in the row the shift is at most sizeof(word) - 2 * C.
template <int C>
__device__ __forceinline__ typename Pair<C>::word tap_pair(const unsigned char* row, int cx0,
                                                           const unsigned char* last) {
  const unsigned char* a = row + cx0 * C;
  const unsigned char* p = a < last ? a : last;
  typename Pair<C>::word w;
  __builtin_memcpy(&w, p, sizeof(w));
  return w >> (8 * (int)(a - p));
}

// the four pixels of one thread: C channels each, taps from clamped indices, fill by select.  WIDE: the image
// holds at least one tap-pair word, so a row's two taps come by tap_pair; else (a few pixels) byte by byte.
template <int C, bool WIDE>
__device__ __forceinline__ void warp_pixels(const AImg& d, const AStyle& S, int x, int y, int nv,
                                            const unsigned char* last) {
  const int W = d.W, H = d.H;
  long long sx = (long long)d.q[0] * x + (long long)d.q[1] * y + d.q[2];
  long long sy = (long long)d.q[3] * x + (long long)d.q[4] * y + d.q[5];
  const long long dsx = d.q[0], dsy = d.q[3];
  int o[4 * C];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long sx5 = (sx + 1024) >> 11, sy5 = (sy + 1024) >> 11;
    const int ix = (int)(sx5 >> 5), iy = (int)(sy5 >> 5);   // |s| < 2^35: the pixel index fits 32 bits
    const int fx = (int)(sx5 & 31), fy = (int)(sy5 & 31);
    const bool x0in = ix >= 0 && ix < W, x1in = ix >= -1 && ix < W - 1;
    const bool y0in = iy >= 0 && iy < H, y1in = iy >= -1 && iy < H - 1;
    const int cx0 = min(max(ix, 0), W - 1), cx1 = min(max(ix + 1, 0), W - 1);
    const int cy0 = min(max(iy, 0), H - 1), cy1 = min(max(iy + 1, 0), H - 1);
    const unsigned char* r0 = d.src + (size_t)cy0 * d.pitch;
    const unsigned char* r1 = d.src + (size_t)cy1 * d.pitch;
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    int a[C], b[C], c[C], e[C];
    if (WIDE) {
      const auto w0 = tap_pair<C>(r0, cx0, last), w1 = tap_pair<C>(r1, cx0, last);
      const int s1 = cx1 == cx0 ? 0 : 8 * C;   // clamped at an edge: the second tap is the first (or is fill)
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        a[ch] = (int)(w0 >> (8 * ch)) & 255;
        b[ch] = (int)(w0 >> (s1 + 8 * ch)) & 255;
        c[ch] = (int)(w1 >> (8 * ch)) & 255;
        e[ch] = (int)(w1 >> (s1 + 8 * ch)) & 255;
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        a[ch] = r0[cx0 * C + ch];
        b[ch] = r0[cx1 * C + ch];
        c[ch] = r1[cx0 * C + ch];
        e[ch] = r1[cx1 * C + ch];
      }
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const int f = S.fill[ch];
      const int t00 = (y0in && x0in) ? a[ch] : f, t01 = (y0in && x1in) ? b[ch] : f;
      const int t10 = (y1in && x0in) ? c[ch] : f, t11 = (y1in && x1in) ? e[ch] : f;
      const int acc = w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11;
      const int v = (acc + 512) >> 10;
      o[j * C + ch] = min(max((v * d.gain + d.offset + 128) >> 8, 0), 255);
    }
    sx += dsx;
    sy += dsy;
  }
  unsigned char* rowp = d.dst + ((size_t)y * W + x) * C;   // destinations are dense
  if (nv == 4 && (reinterpret_cast<uintptr_t>(rowp) & 3) == 0) {
    unsigned u[C] = {};
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) u[k >> 2] |= (unsigned)o[k] << (8 * (k & 3));
    unsigned* wp = reinterpret_cast<unsigned*>(rowp);
#pragma unroll
    for (int k = 0; k < C; ++k) wp[k] = u[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4 * C; ++k)
      if (k / C < nv) rowp[k] = (unsigned char)o[k];
  }
}

__device__ __forceinline__ double map_x(const double* N, double x, double y) { return N[0] * x + N[1] * y + N[2]; }
__device__ __forceinline__ double map_y(const double* N, double x, double y) { return N[3] * x + N[4] * y + N[5]; }

// item r of one image's labels: person r / (K + 1), joint r % (K + 1), the last one being the person's box
__device__ __forceinline__ void move_label(const AImg& d, const AStyle& S, size_t gi, int r, int P, int K,
                                           const float* __restrict__ kpts, const float* __restrict__ vis,
                                           const float* __restrict__ boxes, float* __restrict__ kpts_out,
                                           float* __restrict__ vis_out, float* __restrict__ boxes_out) {
  const int p = r / (K + 1), j = r - p * (K + 1);
  const size_t ip = gi * P + p;
  if (j < K) {
    const int sk = d.mirror ? S.pair[j] : j;
    const size_t si = ip * K + sk, oi = ip * K + j;
    const float x = kpts[si * 2], y = kpts[si * 2 + 1], v = vis[si];
    float ox = x, oy = y, ov = v;
    if (!(v == 0.f || (x == 0.f && y == 0.f))) {   // an unlabelled joint passes through unchanged
      ox = (float)map_x(d.N, (double)x, (double)y);
      oy = (float)map_y(d.N, (double)x, (double)y);
      if (!(ox >= 0.f && ox < 1.f && oy >= 0.f && oy < 1.f)) ox = oy = ov = 0.f;   // it left the frame
    }
    kpts_out[oi * 2] = ox;
    kpts_out[oi * 2 + 1] = oy;
    vis_out[oi] = ov;
    return;
  }
  const float* b = boxes + ip * 4;
  const double cx = b[0], cy = b[1], w = b[2], h = b[3];
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  if (!(cx == 0. && cy == 0. && w == 0. && h == 0.)) {
    const double x0 = cx - 0.5 * w, x1 = cx + 0.5 * w, y0 = cy - 0.5 * h, y1 = cy + 0.5 * h;
    const double ax = map_x(d.N, x0, y0), bx = map_x(d.N, x1, y0), cxx = map_x(d.N, x0, y1), dx = map_x(d.N, x1, y1);
    const double ay = map_y(d.N, x0, y0), by = map_y(d.N, x1, y0), cyy = map_y(d.N, x0, y1), dy = map_y(d.N, x1, y1);
    const double lx = fmin(fmax(fmin(fmin(ax, bx), fmin(cxx, dx)), 0.), 1.);
    const double hx = fmin(fmax(fmax(fmax(ax, bx), fmax(cxx, dx)), 0.), 1.);
    const double ly = fmin(fmax(fmin(fmin(ay, by), fmin(cyy, dy)), 0.), 1.);
    const double hy = fmin(fmax(fmax(fmax(ay, by), fmax(cyy, dy)), 0.), 1.);
    const double ww = hx - lx, hh = hy - ly;
    if (ww > 0. && hh > 0.) {   // otherwise the person left the frame: a zero row, which the forward skips
      out[0] = (float)(0.5 * (lx + hx));
      out[1] = (float)(0.5 * (ly + hy));
      out[2] = (float)ww;
      out[3] = (float)hh;
    }
  }
  float* ob = boxes_out + ip * 4;
  ob[0] = out[0];
  ob[1] = out[1];
  ob[2] = out[2];
  ob[3] = out[3];
}

// grid: the chunk's tiles, image after image (AImg::tile0), then lblocks label workgroups per image
__global__ __launch_bounds__(256) void augment_kernel(ATable T, AStyle S, int m, int c0, int C, int tiles,
                                                      int lblocks, int P, int K, const float* __restrict__ kpts,
                                                      const float* __restrict__ vis,
                                                      const float* __restrict__ boxes, float* __restrict__ kpts_out,
                                                      float* __restrict__ vis_out, float* __restrict__ boxes_out) {
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= tiles) {
    const int li = (b - tiles) / lblocks, r = ((b - tiles) - li * lblocks) * 256 + tid;
    if (r < P * (K + 1)) move_label(T.d[li], S, (size_t)c0 + li, r, P, K, kpts, vis, boxes, kpts_out, vis_out, boxes_out);
    return;
  }
  int li = 0;
  for (int i = 1; i < m; ++i)
    if (b >= T.d[i].tile0) li = i;
  const AImg& d = T.d[li];
  const int t = b - d.tile0, tyi = t / d.tiles_x, txi = t - tyi * d.tiles_x;
  const int x = txi * kTW + (tid & 15) * 4, y = tyi * kTH + (tid >> 4);   // this thread's four pixels
  const int nv = y < d.H ? min(max(d.W - x, 0), 4) : 0;                   // how many lie in the image
  if (nv == 0) return;
  const size_t extent = (size_t)(d.H - 1) * d.pitch + (size_t)d.W * C;   // bytes from the image's first to its last
  if (C == 3) {
    if (extent >= 8)
      warp_pixels<3, true>(d, S, x, y, nv, d.src + extent - 8);
    else
      warp_pixels<3, false>(d, S, x, y, nv, nullptr);
  } else {
    if (extent >= 4)
      warp_pixels<1, true>(d, S, x, y, nv, d.src + extent - 4);
    else
      warp_pixels<1, false>(d, S, x, y, nv, nullptr);
  }
}

int fail(const std::string& what) { return kpd_fail_einval(("kpd_augment_batch: " + what).c_str()); }

struct Span {
  const char* lo;
  const char* hi;
  int image;
};

}  // namespace

extern "C" int kpd_augment_batch(const uint8_t* const* srcs, const int* heights, const int* widths,
                                 const int* pitches, uint8_t* const* dsts, int n, int channels, const int32_t* q,
                                 const double* N, const int* mirror, const int32_t* gain, const int32_t* offset,
                                 const uint8_t* fill, const int32_t* pairs, const float* keypoints,
                                 const float* visibilities, const float* boxes, int P, int K, float* keypoints_out,
                                 float* visibilities_out, float* boxes_out, void* stream) {
  const int C = channels;
  if (n < 0) return fail("n must not be negative");
  if (C != 1 && C != 3) return fail("channels must be 1 or 3");
  const bool labels = keypoints || visibilities || boxes;
  AStyle S{};
  if (labels) {
    if (!keypoints || !visibilities || !boxes)
      return fail("keypoints, visibilities and boxes must be given together (or all be null)");
    if (P < 1) return fail("P must be at least 1 when labels are given");
    if (K < 1 || K > kMaxK) return fail("K must be in [1, 32]");
    if (!pairs) return fail("pairs is null");
    for (int k = 0; k < K; ++k) {
      if (pairs[k] < 0 || pairs[k] >= K) return fail("pairs[" + std::to_string(k) + "] is not in [0, K)");
      S.pair[k] = (unsigned char)pairs[k];
    }
    for (int k = 0; k < K; ++k)
      if (pairs[pairs[k]] != k) return fail("pairs is not an involution at " + std::to_string(k));
    if ((long long)P * (K + 1) > (1LL << 30)) return fail("P * (K + 1) must not exceed 2^30");
  }
  if (n == 0) return KPD_OK;
  if (!srcs || !heights || !widths || !pitches || !dsts || !q || !N || !mirror || !gain || !offset || !fill)
    return fail("null array");
  if (labels && (!keypoints_out || !visibilities_out || !boxes_out))
    return fail("keypoints_out, visibilities_out and boxes_out are needed with labels");
  auto bad = [](int i, const std::string& what) { return fail("image " + std::to_string(i) + ": " + what); };
  for (int i = 0; i < n; ++i) {
    if (heights[i] < 1 || widths[i] < 1 || heights[i] > kMaxSide || widths[i] > kMaxSide)
      return bad(i, "sides must be in [1, 16384]");
    if (pitches[i] < C * widths[i]) return bad(i, "pitch below channels * width");
    for (int k : {0, 1, 3, 4})
      if (q[6 * i + k] <= -(1 << 19) || q[6 * i + k] >= (1 << 19))
        return bad(i, "q: |q00|, |q01|, |q10|, |q11| must be below 2^19");
    if (gain[i] < 0 || gain[i] > 65535) return bad(i, "gain must be in [0, 65535]");
    if (offset[i] <= -(1 << 24) || offset[i] >= (1 << 24)) return bad(i, "offset: |offset| must be below 2^24");
    if (!srcs[i]) return bad(i, "null source image");
    if (!dsts[i]) return bad(i, "null destination image");
  }
  {
    // the warp is a gather: no destination may overlap any source.  Sources sorted by start, with the running
    // maximum of their ends, answer "does any source reach into [lo, hi)" by one binary search per destination.
    std::vector<Span> ss(n);
    for (int i = 0; i < n; ++i) {
      const char* lo = reinterpret_cast<const char*>(srcs[i]);
      ss[i] = {lo, lo + (size_t)(heights[i] - 1) * pitches[i] + (size_t)widths[i] * C, i};
    }
    std::sort(ss.begin(), ss.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
    std::vector<const char*> reach(n);
    for (int i = 0; i < n; ++i) reach[i] = i ? std::max(reach[i - 1], ss[i].hi) : ss[i].hi;
    for (int i = 0; i < n; ++i) {
      const char* lo = reinterpret_cast<const char*>(dsts[i]);
      const char* hi = lo + (size_t)heights[i] * widths[i] * C;
      const auto it = std::lower_bound(ss.begin(), ss.end(), hi, [](const Span& a, const char* v) { return a.lo < v; });
      if (it != ss.begin() && reach[(it - ss.begin()) - 1] > lo) return bad(i, "destination overlaps a source image");
    }
  }
  if (labels) {
    const size_t np = (size_t)n * P;
    const struct { const float* p; size_t bytes; const char* name; } ins[] = {
        {keypoints, np * K * 8, "keypoints"}, {visibilities, np * K * 4, "visibilities"}, {boxes, np * 16, "boxes"}};
    const struct { const float* p; size_t bytes; const char* name; } outs[] = {
        {keypoints_out, np * K * 8, "keypoints_out"}, {visibilities_out, np * K * 4, "visibilities_out"},
        {boxes_out, np * 16, "boxes_out"}};
    for (const auto& o : outs)
      for (const auto& in : ins) {
        const char *a = reinterpret_cast<const char*>(o.p), *b = reinterpret_cast<const char*>(in.p);
        if (a < b + in.bytes && b < a + o.bytes) return fail(std::string(o.name) + " overlaps " + in.name);
      }
  }
  for (int c = 0; c < 3; ++c) S.fill[c] = fill[c];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int lblocks = labels ? (int)(((long long)P * (K + 1) + 255) / 256) : 0;
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int m = std::min(kChunk, n - c0);
    ATable T{};
    int tiles = 0;
    for (int i = 0; i < m; ++i) {
      AImg& d = T.d[i];
      const int g = c0 + i;
      d.src = srcs[g];
      d.dst = dsts[g];
      d.H = heights[g];
      d.W = widths[g];
      d.pitch = pitches[g];
      d.tiles_x = (d.W + kTW - 1) / kTW;
      d.tile0 = tiles;
      tiles += d.tiles_x * ((d.H + kTH - 1) / kTH);
      for (int k = 0; k < 6; ++k) {
        d.q[k] = q[6 * g + k];
        d.N[k] = N[6 * g + k];
      }
      d.gain = gain[g];
      d.offset = offset[g];
      d.mirror = mirror[g] != 0;
    }
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)(tiles + m * lblocks)), dim3(256), 0, st, T, S, m, c0, C, tiles,
                       lblocks, labels ? P : 1, labels ? K : 1, keypoints, visibilities, boxes, keypoints_out,
                       visibilities_out, boxes_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return kpd_fail_hip(e, "kpd_augment_batch");
  }
  return KPD_OK;
}
