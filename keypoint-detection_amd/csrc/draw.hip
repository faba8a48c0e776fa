// Pose overlays on the GPU (kpd_draw_poses): person boxes,
// skeleton limbs, joints and a heatmap underlay drawn in place onto uint8 HWC
// RGB images, read straight from a forward's output tensors.
//
//   setup:  one 64-byte record per (image, person, primitive) -- quantised
//           geometry, colour, pixel bounding box; a primitive that is not
//           drawn gets an empty record.  Record order is blend order: the
//           heat of persons 0..P-1, then per person its box, its limbs in
//           table order and its joints 0..K-1.
//   heatq:  the heat layer's per-person max over keypoints, quantised to a
//           byte, so a pixel reads one byte instead of K floats.
//   tile:   one 256-thread workgroup per KPD_DRAW_TILE_W x KPD_DRAW_TILE_H
//           tile, four pixels of a row per thread.  The workgroup walks the
//           image's records in blocks of 256: each lane tests one record's
//           bounding box against the tile, the survivors are compacted in
//           record order into LDS (ballot + prefix count) and every pixel
//           blends them in that order, its RGB staying in registers across
//           blocks.  A tile no record survives is neither loaded nor stored.
//
// All geometry is integer arithmetic on a 16-subpixel grid; the only
// floating-point steps are the quantisation (one fp32 multiply, rintf), the
// box corners (cx -+ 0.5f * w, each operation rounded on its own) and
// floorf(m * 256) of the heat.  tests/draw_ref.py restates the rules in numpy
// and the results are bit-equal.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kChunk = KPD_DRAW_CHUNK, kTW = KPD_DRAW_TILE_W, kTH = KPD_DRAW_TILE_H;
constexpr int kQMax = 1 << 20;   // quantised coordinates are clamped to +-2^20 subpixels
constexpr int kMaxK = 32, kMaxL = 64;
static_assert(kTW == 64 && kTH == 16, "draw_tile_kernel maps 256 threads to 16 rows of 16 four-pixel groups");

enum : int { R_NONE = 0, R_JOINT = 1, R_LIMB = 2, R_BOX = 3, R_HEAT = 4 };

// One primitive of one person.  g / q by type:
//   R_JOINT  g = {X, Y, r^2}
//   R_LIMB   g = {Ax, Ay, dx, dy}, q0 = d.d, q1 = isqrt(h^2 * d.d)
//   R_BOX    g = {X0, Y0, X1, Y1, hb}
//   R_HEAT   g = {X0, Y0, X1, Y1, image * P + person}; alpha = heat_alpha
struct __attribute__((aligned(16))) Rec {
  int type, color, alpha;
  int bx0, by0, bx1, by1;   // covered pixels lie in [bx0, bx1] x [by0, by1], clamped to the image
  int g[5];
  long long q0, q1;
};
static_assert(sizeof(Rec) == 64, "records are four 16-byte words");

struct DImg {
  unsigned char* img;
  int H, W, pitch;
  int tiles_x;
  int tile0;   // tiles of the chunk's images before this one: workgroup id -> (image, tile)
  int pad;
};

struct DTable {
  DImg d[kChunk];
};

struct Style {
  unsigned char limbs[kMaxL][2];
  unsigned char limb_colors[kMaxL][3];
  unsigned char joint_colors[3][3];
  unsigned char box_color[3];
  int L, r, h, hb, alpha, heat_alpha, min_class, flags;
};

// X = clamp(int(rintf(v * float(16 * size))), -2^20, 2^20); false for a non-finite v
__device__ __forceinline__ bool quantise(float v, int size, int* out) {
  if (!__builtin_isfinite(v)) return false;
  float t = rintf(v * (float)(16 * size));
  t = fminf(fmaxf(t, -(float)kQMax), (float)kQMax);
  *out = (int)t;
  return true;
}

// index of the first maximum of a one-hot row; -1 for the all-zero row of a padding person
__device__ __forceinline__ int joint_class(const float* v) {
  const float a = v[0], b = v[1], c = v[2];
  if (a == 0.f && b == 0.f && c == 0.f) return -1;
  int k = 0;
  float m = a;
  if (b > m) { k = 1; m = b; }
  if (c > m) k = 2;
  return k;
}

__device__ __forceinline__ bool joint_state(const float* kp, const float* vis, int W, int H, int min_class, int* X,
                                            int* Y, int* cls) {
  *cls = joint_class(vis);
  if (*cls < 0 || *cls < min_class) return false;
  const bool okx = quantise(kp[0], W, X), oky = quantise(kp[1], H, Y);
  return okx && oky;
}

// pixels p with a <= 16 p + 8 <= b: [(a + 7) >> 4, (b - 8) >> 4], clamped to [0, size)
__device__ __forceinline__ void pixel_range(int a, int b, int size, int* lo, int* hi) {
  *lo = max((a + 7) >> 4, 0);
  *hi = min((b - 8) >> 4, size - 1);
}

__device__ __forceinline__ long long isqrt64(long long v) {
  long long s = (long long)sqrt((double)v);
  while (s * s > v) --s;
  while ((s + 1) * (s + 1) <= v) ++s;
  return s;
}

__device__ __forceinline__ int pack_rgb(const unsigned char* c) { return c[0] | (c[1] << 8) | (c[2] << 16); }

// grid (ceil(R / 256), images of the chunk); recs [image][R]
__global__ __launch_bounds__(256) void draw_setup_kernel(DTable T, Style S, int c0, int P, int K,
                                                         const float* __restrict__ kpts,
                                                         const float* __restrict__ vis,
                                                         const float* __restrict__ boxes, int R,
                                                         Rec* __restrict__ recs) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= R) return;
  const DImg& d = T.d[blockIdx.y];
  const int W = d.W, H = d.H;
  const size_t gi = (size_t)c0 + blockIdx.y;
  const int per = 1 + S.L + K;
  int p, j;   // j: -1 heat, 0 box, 1..L limb, then joints
  if (s < P) {
    p = s;
    j = -1;
  } else {
    p = (s - P) / per;
    j = (s - P) - p * per;
  }
  const size_t ip = gi * P + p;
  Rec r;
  r.type = R_NONE;
  r.color = 0;
  r.alpha = S.alpha;
  r.bx0 = r.by0 = 0;
  r.bx1 = r.by1 = -1;
  for (int i = 0; i < 5; ++i) r.g[i] = 0;
  r.q0 = r.q1 = 0;
  bool person = true, box_ok = false;
  int X0 = 0, Y0 = 0, X1 = 0, Y1 = 0;
  if (boxes) {
    const float* b = boxes + ip * 4;
    const float cx = b[0], cy = b[1], w = b[2], h = b[3];
    person = cx != 0.f || cy != 0.f || w != 0.f || h != 0.f;
    if (person && j <= 0) {
      const float hw = 0.5f * w, hh = 0.5f * h;
      const float x0 = cx - hw, x1 = cx + hw, y0 = cy - hh, y1 = cy + hh;
      const bool f0 = quantise(x0, W, &X0), f1 = quantise(x1, W, &X1), f2 = quantise(y0, H, &Y0),
                 f3 = quantise(y1, H, &Y1);
      box_ok = f0 && f1 && f2 && f3 && X1 > X0 && Y1 > Y0;
    }
  }
  int ax = 0, bx = -1, ay = 0, by = -1;   // subpixel extent of the primitive
  if (j == -1) {
    if ((S.flags & KPD_DRAW_HEAT) && person && box_ok) {
      r.type = R_HEAT;
      r.alpha = S.heat_alpha;
      r.g[0] = X0; r.g[1] = Y0; r.g[2] = X1; r.g[3] = Y1;
      r.g[4] = (int)ip;
      ax = X0; bx = X1 - 1; ay = Y0; by = Y1 - 1;
    }
  } else if (j == 0) {
    if ((S.flags & KPD_DRAW_BOXES) && person && box_ok) {
      r.type = R_BOX;
      r.color = pack_rgb(S.box_color);
      r.g[0] = X0; r.g[1] = Y0; r.g[2] = X1; r.g[3] = Y1;
      r.g[4] = S.hb;
      ax = X0 - S.hb; bx = X1 + S.hb; ay = Y0 - S.hb; by = Y1 + S.hb;
    }
  } else if (j <= S.L) {
    if ((S.flags & KPD_DRAW_LIMBS) && person) {
      const int ja = S.limbs[j - 1][0], jb = S.limbs[j - 1][1];
      int Ax, Ay, Bx, By, ca, cb;
      const bool oka = joint_state(kpts + (ip * K + ja) * 2, vis + (ip * K + ja) * 3, W, H, S.min_class, &Ax, &Ay, &ca);
      const bool okb = joint_state(kpts + (ip * K + jb) * 2, vis + (ip * K + jb) * 3, W, H, S.min_class, &Bx, &By, &cb);
      if (oka && okb) {
        const int dx = Bx - Ax, dy = By - Ay;
        const long long dd = (long long)dx * dx + (long long)dy * dy;
        if (dd > 0) {
          r.type = R_LIMB;
          r.color = pack_rgb(S.limb_colors[j - 1]);
          r.g[0] = Ax; r.g[1] = Ay; r.g[2] = dx; r.g[3] = dy;
          r.q0 = dd;
          r.q1 = isqrt64((long long)S.h * S.h * dd);
          ax = min(Ax, Bx) - S.h; bx = max(Ax, Bx) + S.h; ay = min(Ay, By) - S.h; by = max(Ay, By) + S.h;
        }
      }
    }
  } else {
    if ((S.flags & KPD_DRAW_JOINTS) && person) {
      const int k = j - 1 - S.L;
      int X, Y, cls;
      if (joint_state(kpts + (ip * K + k) * 2, vis + (ip * K + k) * 3, W, H, S.min_class, &X, &Y, &cls)) {
        r.type = R_JOINT;
        r.color = pack_rgb(S.joint_colors[cls]);
        r.g[0] = X; r.g[1] = Y;
        r.g[2] = S.r * S.r;
        ax = X - S.r; bx = X + S.r; ay = Y - S.r; by = Y + S.r;
      }
    }
  }
  if (r.type != R_NONE) {
    pixel_range(ax, bx, W, &r.bx0, &r.bx1);
    pixel_range(ay, by, H, &r.by0, &r.by1);
    if (r.bx1 < r.bx0 || r.by1 < r.by0) r.type = R_NONE;
  }
  recs[gi * R + s] = r;
}

// q [plane][hh * hw] = min(255, int(floorf(m * 256))), m = the plane's maximum over its K maps with NaN
// entries ignored; 0 when m <= 0 or every entry is NaN.  plane = image * P + person.
__global__ __launch_bounds__(256) void draw_heatq_kernel(const float* __restrict__ heat, long total, int K, int hw2,
                                                         unsigned char* __restrict__ q) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long plane = i / hw2;
  const int c = (int)(i - plane * hw2);
  const float* src = heat + (size_t)plane * K * hw2 + c;
  float m = -INFINITY;
  for (int k = 0; k < K; ++k) {
    const float v = src[(size_t)k * hw2];
    if (v > m) m = v;
  }
  int qq = 0;
  if (m > 0.f) {
    const float t = floorf(m * 256.f);
    qq = t >= 255.f ? 255 : (int)t;
  }
  q[i] = (unsigned char)qq;
}

__device__ __forceinline__ int blend(int v, int c, int a) { return (v * (256 - a) + c * a + 128) >> 8; }

__device__ __forceinline__ void blend_px(int* px, int color, int a) {
  px[0] = blend(px[0], color & 255, a);
  px[1] = blend(px[1], (color >> 8) & 255, a);
  px[2] = blend(px[2], (color >> 16) & 255, a);
}

// grid: the chunk's tiles, image after image (DImg::tile0)
__global__ __launch_bounds__(256) void draw_tile_kernel(DTable T, int m, int c0, int R,
                                                        const Rec* __restrict__ recs,
                                                        const unsigned char* __restrict__ qmap, int hh, int hw) {
  __shared__ Rec list[256];
  __shared__ int wcount[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  int li = 0;
  for (int i = 1; i < m; ++i)
    if (b >= T.d[i].tile0) li = i;
  const DImg& d = T.d[li];
  const int t = b - d.tile0, tyi = t / d.tiles_x, txi = t - tyi * d.tiles_x;
  const int px0 = txi * kTW, py0 = tyi * kTH;                                   // the tile's pixels:
  const int px1 = min(px0 + kTW, d.W) - 1, py1 = min(py0 + kTH, d.H) - 1;       // [px0, px1] x [py0, py1]
  const int x = px0 + (tid & 15) * 4, y = py0 + (tid >> 4);                      // this thread's four pixels
  const int nv = y < d.H ? min(max(d.W - x, 0), 4) : 0;                          // how many lie in the image
  unsigned char* rowp = d.img + (size_t)y * d.pitch + (size_t)x * 3;             // dereferenced only when nv > 0
  const bool wide = nv == 4 && (reinterpret_cast<uintptr_t>(rowp) & 3) == 0;     // 12 bytes as three dwords
  const int Cx0 = 16 * x + 8, Cy = 16 * y + 8;
  const Rec* ir = recs + ((size_t)c0 + li) * R;
  int c[4][3];
  bool loaded = false;
  for (int r0 = 0; r0 < R; r0 += 256) {
    // cull: one record per lane against the tile, survivors compacted in record order
    const int ri = r0 + tid;
    bool keep = false;
    // the record as its four 16-byte words: w0 = (type, color, alpha, bx0), w1 = (by0, bx1, by1, g0),
    // w2 = (g1, g2, g3, g4), w3 = (q0, q1)
    int4 w0 = make_int4(0, 0, 0, 0), w1 = w0, w2 = w0, w3 = w0;
    if (ri < R) {
      const int4* rp = reinterpret_cast<const int4*>(ir + ri);
      w0 = rp[0];
      w1 = rp[1];
      w2 = rp[2];
      w3 = rp[3];
      keep = w0.x != R_NONE && w0.w <= px1 && w1.y >= px0 && w1.x <= py1 && w1.z >= py0;
      // an outline does not touch a tile whose pixel centres all lie strictly inside its inner rectangle
      if (keep && w0.x == R_BOX)
        keep = !(16 * px0 + 8 > w1.w + w2.w && 16 * px1 + 8 < w2.y - w2.w &&
                 16 * py0 + 8 > w2.x + w2.w && 16 * py1 + 8 < w2.z - w2.w);
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
      const int cnt = wcount[w];
      base += w < wave ? cnt : 0;
      total += cnt;
    }
    if (keep) {
      int4* lp = reinterpret_cast<int4*>(&list[base + __popcll(bal & ((1ull << lane) - 1ull))]);
      lp[0] = w0;
      lp[1] = w1;
      lp[2] = w2;
      lp[3] = w3;
    }
    __syncthreads();
    if (total > 0) {
      if (!loaded) {
        loaded = true;
        if (wide) {
          const unsigned* wp = reinterpret_cast<const unsigned*>(rowp);
          const unsigned u[3] = {wp[0], wp[1], wp[2]};
#pragma unroll
          for (int k = 0; k < 12; ++k) c[k / 3][k % 3] = (u[k >> 2] >> (8 * (k & 3))) & 255;
        } else {
#pragma unroll
          for (int k = 0; k < 12; ++k) c[k / 3][k % 3] = k / 3 < nv ? (int)rowp[k] : 0;
        }
      }
      for (int k = 0; k < total; ++k) {
        const Rec& q = list[k];
        const int type = q.type, color = q.color, alpha = q.alpha;
        const int g0 = q.g[0], g1 = q.g[1], g2 = q.g[2], g3 = q.g[3], g4 = q.g[4];
        const bool rowin = y >= q.by0 && y <= q.by1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // inside the record's pixel box the differences below are bounded by the primitive's own size
          if (!(rowin && x + j >= q.bx0 && x + j <= q.bx1)) continue;
          const int Cx = Cx0 + 16 * j;
          if (type == R_JOINT) {
            const int ex = Cx - g0, ey = Cy - g1;
            if (ex * ex + ey * ey <= g2) blend_px(c[j], color, alpha);
          } else if (type == R_LIMB) {
            const int ex = Cx - g0, ey = Cy - g1;
            const long long dot = (long long)ex * g2 + (long long)ey * g3;
            long long cross = (long long)ex * g3 - (long long)ey * g2;
            cross = cross < 0 ? -cross : cross;
            if (dot >= 0 && dot <= q.q0 && cross <= q.q1) blend_px(c[j], color, alpha);
          } else if (type == R_BOX) {
            const bool outer = Cx >= g0 - g4 && Cx <= g2 + g4 && Cy >= g1 - g4 && Cy <= g3 + g4;
            const bool inner = Cx > g0 + g4 && Cx < g2 - g4 && Cy > g1 + g4 && Cy < g3 - g4;
            if (outer && !inner) blend_px(c[j], color, alpha);
          } else if (Cx >= g0 && Cx < g2 && Cy >= g1 && Cy < g3) {   // R_HEAT
            const unsigned col = (unsigned)(Cx - g0) * (unsigned)hw / (unsigned)(g2 - g0);
            const unsigned row = (unsigned)(Cy - g1) * (unsigned)hh / (unsigned)(g3 - g1);
            const int qv = qmap[((size_t)g4 * hh + row) * hw + col];
            const int hc = min(255, 3 * qv) | (min(max(3 * qv - 255, 0), 255) << 8) |
                           (min(max(3 * qv - 510, 0), 255) << 16);
            blend_px(c[j], hc, (qv * alpha) >> 8);
          }
        }
      }
    }
    __syncthreads();   // the next block overwrites the list
  }
  if (!loaded) return;
  if (wide) {
    unsigned u[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 12; ++k) u[k >> 2] |= (unsigned)c[k / 3][k % 3] << (8 * (k & 3));
    unsigned* wp = reinterpret_cast<unsigned*>(rowp);
    wp[0] = u[0];
    wp[1] = u[1];
    wp[2] = u[2];
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k / 3 < nv) rowp[k] = (unsigned char)c[k / 3][k % 3];
  }
}

inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int kpd_draw_poses(uint8_t* const* images, const int* heights, const int* widths, const int* pitches, int n,
                              const float* keypoints, const float* visibilities, const float* boxes,
                              const float* heatmap, int P, int K, int hh, int hw, const int* limbs, int L,
                              const uint8_t* limb_colors, const uint8_t* joint_colors, const uint8_t* box_color,
                              int joint_radius, int limb_half_width, int box_half_width, int alpha, int heat_alpha,
                              int min_class, int flags, void* stream) {
  if (n <= 0) return kpd_fail_einval("kpd_draw_poses: n must be positive");
  if (!images || !heights || !widths || !pitches || !keypoints || !visibilities || !joint_colors || !box_color)
    return kpd_fail_einval("kpd_draw_poses: null array");
  if (P <= 0) return kpd_fail_einval("kpd_draw_poses: P must be positive");
  if (K <= 0 || K > kMaxK) return kpd_fail_einval("kpd_draw_poses: K must be in [1, 32]");
  if (L < 0 || L > kMaxL) return kpd_fail_einval("kpd_draw_poses: L must be in [0, 64]");
  if (L > 0 && (!limbs || !limb_colors)) return kpd_fail_einval("kpd_draw_poses: null array");
  if (flags & ~(KPD_DRAW_BOXES | KPD_DRAW_LIMBS | KPD_DRAW_JOINTS | KPD_DRAW_HEAT))
    return kpd_fail_einval("kpd_draw_poses: unknown flag");
  if ((flags & (KPD_DRAW_BOXES | KPD_DRAW_HEAT)) && !boxes)
    return kpd_fail_einval("kpd_draw_poses: the box and heat layers need boxes");
  if ((flags & KPD_DRAW_HEAT) && (!heatmap || hh <= 0 || hw <= 0 || hh > KPD_DRAW_MAX_HEAT || hw > KPD_DRAW_MAX_HEAT))
    return kpd_fail_einval("kpd_draw_poses: the heat layer needs a heatmap with sides in [1, 1024]");
  if (alpha < 0 || alpha > 256 || heat_alpha < 0 || heat_alpha > 256)
    return kpd_fail_einval("kpd_draw_poses: alpha and heat_alpha must be in [0, 256]");
  if (joint_radius < 0 || joint_radius > KPD_DRAW_MAX_WIDTH || limb_half_width < 0 ||
      limb_half_width > KPD_DRAW_MAX_WIDTH || box_half_width < 0 || box_half_width > KPD_DRAW_MAX_WIDTH)
    return kpd_fail_einval("kpd_draw_poses: radius and half-widths must be in [0, 512] (32 px in 1/16-pixel units)");
  if (min_class < 0 || min_class > 2) return kpd_fail_einval("kpd_draw_poses: min_class must be 0, 1 or 2");
  for (int l = 0; l < L; ++l)
    if (limbs[2 * l] < 0 || limbs[2 * l] >= K || limbs[2 * l + 1] < 0 || limbs[2 * l + 1] >= K)
      return kpd_fail_einval(("kpd_draw_poses: limb " + std::to_string(l) + ": joint index outside [0, K)").c_str());
  if ((long long)n * P > 0x7fffffffLL) return kpd_fail_einval("kpd_draw_poses: n * P too large");
  auto bad = [](int i, const char* what) {
    return kpd_fail_einval(("kpd_draw_poses: image " + std::to_string(i) + ": " + what).c_str());
  };
  for (int i = 0; i < n; ++i) {
    if (!images[i]) return bad(i, "null image");
    if (heights[i] <= 0 || widths[i] <= 0 || heights[i] > KPD_DRAW_MAX_SIDE || widths[i] > KPD_DRAW_MAX_SIDE)
      return bad(i, "sides must be in [1, 16384]");
    if (pitches[i] < 3 * widths[i]) return bad(i, "pitch below 3 * width");
  }
  if (!flags) return KPD_OK;
  Style S{};
  for (int l = 0; l < L; ++l) {
    S.limbs[l][0] = (unsigned char)limbs[2 * l];
    S.limbs[l][1] = (unsigned char)limbs[2 * l + 1];
    for (int c = 0; c < 3; ++c) S.limb_colors[l][c] = limb_colors[3 * l + c];
  }
  for (int c = 0; c < 9; ++c) S.joint_colors[c / 3][c % 3] = joint_colors[c];
  for (int c = 0; c < 3; ++c) S.box_color[c] = box_color[c];
  S.L = L;
  S.r = joint_radius;
  S.h = limb_half_width;
  S.hb = box_half_width;
  S.alpha = alpha;
  S.heat_alpha = heat_alpha;
  S.min_class = min_class;
  S.flags = flags;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int R = P * (2 + L + K);   // records per image: P heat, then P x (box, L limbs, K joints)
  const bool heat = flags & KPD_DRAW_HEAT;
  const size_t rec_bytes = (size_t)n * R * sizeof(Rec);
  const size_t q_bytes = heat ? (size_t)n * P * hh * hw : 0;
  unsigned char* base = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&base), rec_bytes + std::max<size_t>(q_bytes, 16), st);
  if (e != hipSuccess) return kpd_fail_hip(e, "kpd_draw_poses: scratch");
  Rec* recs = reinterpret_cast<Rec*>(base);
  unsigned char* qmap = base + rec_bytes;
  int rc = KPD_OK;
  auto fail_hip = [&](hipError_t err) {
    if (err != hipSuccess && rc == KPD_OK) rc = kpd_fail_hip(err, "kpd_draw_poses");
  };
  if (heat) {
    hipLaunchKernelGGL(draw_heatq_kernel, dim3(blocks((long)q_bytes)), dim3(256), 0, st, heatmap, (long)q_bytes, K,
                       hh * hw, qmap);
    fail_hip(hipGetLastError());
  }
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int m = std::min(kChunk, n - c0);
    DTable T{};
    int tiles = 0;
    for (int i = 0; i < m; ++i) {
      DImg& d = T.d[i];
      d.img = images[c0 + i];
      d.H = heights[c0 + i];
      d.W = widths[c0 + i];
      d.pitch = pitches[c0 + i];
      d.tiles_x = (d.W + kTW - 1) / kTW;
      d.tile0 = tiles;
      tiles += d.tiles_x * ((d.H + kTH - 1) / kTH);
    }
    hipLaunchKernelGGL(draw_setup_kernel, dim3(blocks(R), m), dim3(256), 0, st, T, S, c0, P, K, keypoints,
                       visibilities, boxes, R, recs);
    hipLaunchKernelGGL(draw_tile_kernel, dim3(tiles), dim3(256), 0, st, T, m, c0, R, recs, qmap, hh, hw);
    fail_hip(hipGetLastError());
  }
  (void)hipFreeAsync(base, st);
  return rc;
}
