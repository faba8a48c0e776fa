// Preprocessing on the GPU: the reference's ITransform (dll/data/transforms.py:
// 9-113) without OpenCV or PIL on the host.
//
//   uint8 HWC image (device) --[RGB->gray]--[CLAHE per plane]--[edge blend]
//       --[Gaussian 3x3]--PIL-exact bilinear resize--ToTensor/Normalize--> fp32 CHW (device)
//
// * Resize reproduces Pillow's ImagingResample for 8-bit images bit for bit
//   (Resample.c): coefficients from precompute_coeffs in double, converted to
//   22-bit fixed point by normalize_coeffs_8bpc; horizontal pass first with the
//   intermediate rounded and clipped to uint8, then the vertical pass.  The
//   coefficients are computed on the device in IEEE double with contraction
//   off, so they equal Pillow's.  Pinned by tests/golden/preprocess.npz (real
//   Pillow 12.2 outputs).
// * ToTensor / Normalize: x = (u8 / 255.f - mean) / std, the same fp32 ops as
//   torchvision (a division, not a reciprocal multiply).
// * CLAHE follows OpenCV's cv::CLAHE for CV_8U (clahe.cpp): reflect-101 pad
//   to a tile multiple, 256-bin tile histograms (integer LDS atomics, so the
//   counts are deterministic), clip + batch/strided-residual redistribution,
//   LUT = saturate_cast<uchar>(cumsum * (255 / area)), bilinear blend of four
//   tile LUTs in fp32 without contraction, round-half-even.  Gray conversion is
//   cv::cvtColor(RGB2GRAY) fixed point; Gaussian blurs follow GaussianBlur's
//   8U fixed-point path; the grayscale edge blend is GaussianBlur 5x5 ->
//   medianBlur 5 -> Canny(100, 200, L1) -> (dilate, erode) x 2 -> GaussianBlur
//   3x3 -> scale to 255 -> addWeighted(0.7, 0.3).
//   OpenCV is absent here and on the GPU box: these stages are parity
//   unpinned (see oracle/preprocess_oracle.py).
// * One pipeline: the b_* kernels work on n images per launch, and
//   kpd_preprocess is kpd_preprocess_batch with n = 1 (same kernels, same
//   launcher body).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;

__device__ __forceinline__ unsigned char clip8(int v) {
  if (v >= (1 << kPrecisionBits << 8)) return 255;
  if (v <= 0) return 0;
  return (unsigned char)(v >> kPrecisionBits);
}

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// cv::GaussianBlur for CV_8U (the fixed-point path): kernel taps carry 8
// fraction bits and sum to 256; the row sum and the column sum are exact
// integers, the result is rounded half up from 16 fraction bits.  Reflect-101.
struct GaussTaps {
  int n;
  int k[7];
};

// cv::getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED (8 bits)
GaussTaps gauss_taps(int n, double sigma) {
  double r[7] = {0};
  const int n2 = (n - 1) / 2;
  if (sigma <= 0 && n <= 7) {
    static const double t3[] = {0.25, 0.5, 0.25}, t5[] = {0.0625, 0.25, 0.375, 0.25, 0.0625},
                        t7[] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
    const double* t = n == 3 ? t3 : (n == 5 ? t5 : t7);
    for (int i = 0; i < n; ++i) r[i] = n == 1 ? 1.0 : t[i];
  } else {
    const double sig = sigma > 0 ? sigma : n * 0.15 + 0.35, scale2x = -0.125 / (sig * sig);
    double vals[3], sum = 0.0;
    for (int i = 0; i < n2; ++i) {
      const int x = 2 * i + 1 - n;
      vals[i] = std::exp((double)(x * x) * scale2x);
      sum += vals[i];
    }
    sum = sum * 2.0 + 1.0;
    const double mul1 = 1.0 / sum;
    for (int i = 0; i < n2; ++i) r[i] = r[n - 1 - i] = vals[i] * mul1;
    r[n2] = mul1;
  }
  GaussTaps g{};
  g.n = n;
  double err = 0.0;
  int s = 0;
  for (int i = 0; i < n2; ++i) {
    const double adj = r[i] * 256.0 + err;
    const int v0 = (int)std::nearbyint(adj);   // cvRound (half to even)
    err = adj - v0;
    g.k[i] = g.k[n - 1 - i] = v0;
    s += v0;
  }
  g.k[n2] = 256 - 2 * s;
  return g;
}

inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }

// host copy of precompute_coeffs' bounds for one output coordinate (same
// double arithmetic as b_resize_coeffs_kernel): first source row and count
void pil_bounds(int in_size, int out_size, int xx, int* xmin_out, int* n_out) {
  const double scale = (double)in_size / (double)out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  *xmin_out = xmin;
  *n_out = xmax - xmin;
}

// Every kernel takes the image index in its grid and reads that image's
// geometry from a descriptor table passed by value in the kernel arguments,
// one table per chunk of KPD_PRE_BATCH_CHUNK images: the launch count depends
// on the number of chunks, not on n, and no host memory is read after the call
// returns.  Pixel grids are sized to the chunk's largest image; the blocks
// past a smaller image's end exit.
constexpr int kChunk = KPD_PRE_BATCH_CHUNK;

struct BImg {
  const unsigned char* src;   // the caller's image
  long long pix;              // pixels of the images before this one: offset into every per-pixel scratch region
  long long tmp;              // offset (elements) of the horizontal pass's output
  long long kkx, kky;         // offsets (ints) of the resize coefficient tables
  int H, W, pitch;
  int tw, th, clip;           // CLAHE tile size and clip count
  int kx, ky;                 // resize kernel sizes
  int y0, y1;                 // source rows [y0, y1) the vertical pass reads
};

struct BTable {
  BImg d[kChunk];
};

// A stage's input: a per-pixel scratch region of C interleaved channels, or
// (base == nullptr) the caller's images with their own pitches.
struct BIn {
  const unsigned char* base;
  int C;
};

__device__ __forceinline__ const unsigned char* b_in(const BImg& d, BIn in, int* pitch) {
  if (in.base) {
    *pitch = d.W * in.C;
    return in.base + d.pix * in.C;
  }
  *pitch = d.pitch;
  return d.src;
}

// cv::cvtColor(RGB2GRAY), 8U fixed point (yuv coefficients << 14)
__global__ void b_rgb2gray_kernel(BTable T, unsigned char* __restrict__ dst_base) {
  const BImg& d = T.d[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.H * d.W) return;
  const int y = i / d.W, x = i - y * d.W;
  const unsigned char* p = d.src + (size_t)y * d.pitch + x * 3;
  dst_base[d.pix + i] = (unsigned char)((p[0] * 4899 + p[1] * 9617 + p[2] * 1868 + (1 << 13)) >> 14);
}

// one workgroup per (tile, plane, image): histogram -> clip/redistribute -> LUT;
// grid (tiles_x, tiles_y, C * images); luts [image][C][tiles_y][tiles_x][256]
__global__ __launch_bounds__(256) void b_clahe_lut_kernel(BTable T, BIn in, int tiles_x, int tiles_y,
                                                          unsigned char* __restrict__ luts) {
  __shared__ int hist[256];
  const int C = in.C, img = blockIdx.z / C, c = blockIdx.z - img * C;
  const BImg& d = T.d[img];
  const int tx = blockIdx.x, ty = blockIdx.y, tid = threadIdx.x;
  const int H = d.H, W = d.W, tw = d.tw, th = d.th, clip = d.clip;
  int pitch;
  const unsigned char* src = b_in(d, in, &pitch);
  hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < tw * th; i += 256) {
    const int y = reflect101(ty * th + i / tw, H), x = reflect101(tx * tw + i % tw, W);
    atomicAdd(&hist[src[(size_t)y * pitch + x * C + c]], 1);
  }
  __syncthreads();
  if (tid == 0) {
    if (clip > 0) {
      int clipped = 0;
      for (int i = 0; i < 256; ++i)
        if (hist[i] > clip) { clipped += hist[i] - clip; hist[i] = clip; }
      const int batch = clipped / 256;
      int residual = clipped - batch * 256;
      for (int i = 0; i < 256; ++i) hist[i] += batch;
      if (residual != 0) {
        const int step = max(256 / residual, 1);
        for (int i = 0; i < 256 && residual > 0; i += step, --residual) hist[i]++;
      }
    }
    const float lut_scale = 255.f / (float)(tw * th);
    int sum = 0;
    unsigned char* lut = luts + ((size_t)((img * C + c) * tiles_y + ty) * tiles_x + tx) * 256;
    for (int i = 0; i < 256; ++i) {
      sum += hist[i];
      lut[i] = (unsigned char)min(max(__float2int_rn((float)sum * lut_scale), 0), 255);
    }
  }
}

__global__ void b_clahe_apply_kernel(BTable T, BIn in, int tiles_x, int tiles_y,
                                     const unsigned char* __restrict__ luts, unsigned char* __restrict__ dst_base) {
  const BImg& d = T.d[blockIdx.y];
  const int C = in.C, H = d.H, W = d.W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)H * W * C) return;
  int pitch;
  const unsigned char* src = b_in(d, in, &pitch);
  const int c = i % C, x = (i / C) % W, y = (int)(i / ((long)C * W));
  const float inv_tw = 1.f / (float)d.tw, inv_th = 1.f / (float)d.th;
  const float tyf = (float)y * inv_th - 0.5f, txf = (float)x * inv_tw - 0.5f;
  int ty1 = (int)floorf(tyf), tx1 = (int)floorf(txf);
  const float ya = tyf - (float)ty1, ya1 = 1.f - ya, xa = txf - (float)tx1, xa1 = 1.f - xa;
  const int ty2 = min(ty1 + 1, tiles_y - 1), tx2 = min(tx1 + 1, tiles_x - 1);
  ty1 = max(ty1, 0);
  tx1 = max(tx1, 0);
  const int v = src[(size_t)y * pitch + x * C + c];
  const unsigned char* lp = luts + (size_t)(blockIdx.y * C + c) * tiles_y * tiles_x * 256;
  const float l11 = lp[(ty1 * tiles_x + tx1) * 256 + v], l12 = lp[(ty1 * tiles_x + tx2) * 256 + v];
  const float l21 = lp[(ty2 * tiles_x + tx1) * 256 + v], l22 = lp[(ty2 * tiles_x + tx2) * 256 + v];
  const float r = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
  dst_base[d.pix * C + i] = (unsigned char)min(max(__float2int_rn(r), 0), 255);
}

// N taps known at compile time: the 2 * N reflected coordinates are formed once
// per pixel and both loops unroll
template <int N>
__global__ void b_gauss_fixed_kernel(BTable T, BIn in, GaussTaps g, unsigned char* __restrict__ dst_base) {
  const BImg& d = T.d[blockIdx.y];
  const int C = in.C, H = d.H, W = d.W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)H * W * C) return;
  int pitch;
  const unsigned char* src = b_in(d, in, &pitch);
  const int c = i % C, x = (i / C) % W, y = (int)(i / ((long)C * W));
  constexpr int r = N / 2;
  int xo[N];
#pragma unroll
  for (int dx = 0; dx < N; ++dx) xo[dx] = reflect101(x + dx - r, W) * C + c;
  int v = 0;
#pragma unroll
  for (int dy = 0; dy < N; ++dy) {
    const unsigned char* row = src + (size_t)reflect101(y + dy - r, H) * pitch;
    int h = 0;
#pragma unroll
    for (int dx = 0; dx < N; ++dx) h += g.k[dx] * (int)row[xo[dx]];
    v += g.k[dy] * h;
  }
  dst_base[d.pix * C + i] = (unsigned char)min((v + (1 << 15)) >> 16, 255);
}

// cv::medianBlur(5) on one plane, replicated border
__global__ void b_median5_kernel(BTable T, const unsigned char* __restrict__ src_base,
                                 unsigned char* __restrict__ dst_base) {
  const BImg& d = T.d[blockIdx.y];
  const int H = d.H, W = d.W;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H * W) return;
  const unsigned char* src = src_base + d.pix;
  const int y = i / W, x = i - y * W;
  int v[25];
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    const unsigned char* row = src + (size_t)min(max(y + dy - 2, 0), H - 1) * W;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) v[dy * 5 + dx] = row[min(max(x + dx - 2, 0), W - 1)];
  }
  // Forgetful selection: of 14 samples neither the smallest nor the largest can
  // be the 13th of 25, so both are dropped and the next sample takes the free
  // slot; 13, 12, ... 3 samples likewise, and the middle of the last three is
  // the median.  168 compare-exchanges in registers against the 1250 compares
  // of a rank count over the 25 samples.
  int a[14];
#pragma unroll
  for (int j = 0; j < 14; ++j) a[j] = v[j];
#pragma unroll
  for (int k = 14; k >= 3; --k) {
#pragma unroll
    for (int j = 1; j < k; ++j) {
      const int lo = min(a[0], a[j]);
      a[j] = max(a[0], a[j]);
      a[0] = lo;
    }
#pragma unroll
    for (int j = 1; j < k - 1; ++j) {
      const int hi = max(a[k - 1], a[j]);
      a[j] = min(a[k - 1], a[j]);
      a[k - 1] = hi;
    }
    if (k > 3) a[0] = v[28 - k];   // 14 + (14 - k): the next sample not yet seen
  }
  dst_base[d.pix + i] = (unsigned char)a[1];
}

// Canny step 1: 3x3 Sobel (replicated border), L1 magnitude.
__global__ void b_canny_grad_kernel(BTable T, const unsigned char* __restrict__ src_base, int* __restrict__ dxy_base,
                                    int* __restrict__ mag_base) {
  const BImg& d = T.d[blockIdx.y];
  const int H = d.H, W = d.W;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H * W) return;
  const unsigned char* src = src_base + d.pix;
  const int y = i / W, x = i - y * W;
  const int y0 = max(y - 1, 0), y2 = min(y + 1, H - 1), x0 = max(x - 1, 0), x2 = min(x + 1, W - 1);
  auto at = [&](int yy, int xx) { return (int)src[(size_t)yy * W + xx]; };
  const int dx = (at(y0, x2) + 2 * at(y, x2) + at(y2, x2)) - (at(y0, x0) + 2 * at(y, x0) + at(y2, x0));
  const int dy = (at(y2, x0) + 2 * at(y2, x) + at(y2, x2)) - (at(y0, x0) + 2 * at(y0, x) + at(y0, x2));
  int* dxy = dxy_base + 2 * d.pix;
  dxy[2 * i] = dx;
  dxy[2 * i + 1] = dy;
  mag_base[d.pix + i] = abs(dx) + abs(dy);
}

// Canny step 2: non-maximum suppression with OpenCV's fixed-point sector
// test (tan 22.5 deg in Q15), magnitude 0 outside the image.  map: 0 = not
// an edge, 1 = candidate (m > low), 2 = seed (m > high, appended to queue).
// cnt [image][2]: the image's seed counter, then its edge maximum
constexpr int kCannyTg22 = 13573;   // (int)(tan(22.5 deg) * 2^15 + 0.5)

__global__ void b_canny_nms_kernel(BTable T, const int* __restrict__ dxy_base, const int* __restrict__ mag_base,
                                   int low, int high, int* __restrict__ map_base, int* __restrict__ queue_base,
                                   int* __restrict__ cnt) {
  const BImg& d = T.d[blockIdx.y];
  const int H = d.H, W = d.W;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H * W) return;
  const int* mag = mag_base + d.pix;
  const int* dxy = dxy_base + 2 * d.pix;
  const int y = i / W, x = i - y * W;
  auto M = [&](int yy, int xx) { return (yy < 0 || yy >= H || xx < 0 || xx >= W) ? 0 : mag[(size_t)yy * W + xx]; };
  const int m = mag[i];
  int state = 0;
  if (m > low) {
    const int dx = dxy[2 * i], dy = dxy[2 * i + 1];
    const long ax = abs(dx), ay = (long)abs(dy) << 15;
    const long tg22x = ax * kCannyTg22, tg67x = tg22x + (ax << 16);
    bool keep;
    if (ay < tg22x) {
      keep = m > M(y, x - 1) && m >= M(y, x + 1);
    } else if (ay > tg67x) {
      keep = m > M(y - 1, x) && m >= M(y + 1, x);
    } else {
      const int s = (dx ^ dy) < 0 ? -1 : 1;
      keep = m > M(y - 1, x - s) && m > M(y + 1, x + s);
    }
    if (keep) state = m > high ? 2 : 1;
  }
  map_base[d.pix + i] = state;
  if (state == 2) queue_base[d.pix + atomicAdd(&cnt[2 * blockIdx.y], 1)] = i;
}

// Canny step 3: hysteresis as a breadth-first flood from the seeds over
// 8-connected candidates, one workgroup per image (level-synchronous; each
// pixel enters the queue once, so the loop ends after at most H*W pushes):
// each image floods its own map from its own queue and seed counter.  The
// flood needs only the image's size and offset, so its table is compact and
// one launch covers kHystChunk images: up to four descriptor chunks flood
// side by side (a flood is bound by its levels' latency, not by the CU).
constexpr int kHystChunk = 4 * kChunk;

struct HTable {
  long long pix[kHystChunk];
  int H[kHystChunk], W[kHystChunk];
};

__global__ __launch_bounds__(1024) void b_canny_hyst_kernel(HTable T, int* __restrict__ map_base,
                                                            int* __restrict__ queue_base,
                                                            const int* __restrict__ cnt) {
  __shared__ int s_tail;
  const int H = T.H[blockIdx.x], W = T.W[blockIdx.x], tid = threadIdx.x;
  int* map = map_base + T.pix[blockIdx.x];
  int* queue = queue_base + T.pix[blockIdx.x];
  if (tid == 0) s_tail = cnt[2 * blockIdx.x];
  __syncthreads();
  int head = 0, tail = s_tail;
  while (head < tail) {
    for (int q = head + tid; q < tail; q += 1024) {
      const int p = queue[q], y = p / W, x = p - y * W;
      // the eight neighbours are read first, as independent loads (one memory
      // round trip per level instead of eight); a stale 1 only fails its CAS
      int nb[8], st[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int j = k < 4 ? k : k + 1, yy = y + j / 3 - 1, xx = x + j % 3 - 1;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        nb[k] = yy * W + xx;
        st[k] = in ? map[nb[k]] : 0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (st[k] == 1 && atomicCAS(&map[nb[k]], 1, 2) == 1) queue[atomicAdd(&s_tail, 1)] = nb[k];
    }
    __syncthreads();
    head = tail;
    tail = s_tail;
    __syncthreads();
  }
}

// The chain behind Canny in one launch: (dilate, erode) x 2 with 3x3 ones,
// GaussianBlur 3x3 (taps 64/128/64) and the image's maximum.  A workgroup
// owns a kPostW x kPostH output tile and stages it with a 5-pixel halo (one
// pixel per stage) in two 8-bit LDS planes that the stages ping-pong between;
// every stage shrinks the computed region by one pixel.  The border rules are
// the image's, not the tile's: a morphology stage visits only in-image
// neighbours (so the out-of-image value never wins), out-of-image positions
// are never written nor read, and the Gaussian reflects image coordinates (reflect-101 of y +- 1 stays within one pixel of
// y, inside the last stage's halo).  Rows are 44 bytes = 11 dwords apart: an
// odd dword stride spreads the rows a wave touches over the banks, and the
// four lanes of a dword share one broadcast read.
constexpr int kPostW = 32, kPostH = 16, kPostHalo = 5;
constexpr int kPostStride = 44;   // >= kPostW + 2 * kPostHalo, 11 dwords
constexpr int kPostRows = kPostH + 2 * kPostHalo;

template <bool DIL>
__device__ __forceinline__ void post_morph(const unsigned char* in, unsigned char* out, int halo, int ty0, int tx0,
                                           int H, int W) {
  const int rw = kPostW + 2 * halo, rh = kPostH + 2 * halo;
  for (int i = threadIdx.x; i < rw * rh; i += 256) {
    const int ry = i / rw, rx = i - ry * rw;
    const int gy = ty0 - halo + ry, gx = tx0 - halo + rx;
    if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
    int r = DIL ? 0 : 255;
    for (int yy = max(gy - 1, 0); yy <= min(gy + 1, H - 1); ++yy)
      for (int xx = max(gx - 1, 0); xx <= min(gx + 1, W - 1); ++xx) {
        const int v = in[(yy - ty0 + kPostHalo) * kPostStride + (xx - tx0 + kPostHalo)];
        r = DIL ? max(r, v) : min(r, v);
      }
    out[(gy - ty0 + kPostHalo) * kPostStride + (gx - tx0 + kPostHalo)] = (unsigned char)r;
  }
}

// grid (tiles over the largest W, tiles over the largest H, images)
__global__ __launch_bounds__(256) void b_post_canny_kernel(BTable T, const int* __restrict__ map_base,
                                                           unsigned char* __restrict__ dst_base,
                                                           int* __restrict__ cnt) {
  __shared__ unsigned char sa[kPostRows * kPostStride], sb[kPostRows * kPostStride];
  __shared__ int s_max;
  const BImg& d = T.d[blockIdx.z];
  const int H = d.H, W = d.W;
  const int tx0 = blockIdx.x * kPostW, ty0 = blockIdx.y * kPostH;
  if (tx0 >= W || ty0 >= H) return;   // the whole workgroup: this image has no such tile
  const int* map = map_base + d.pix;
  const int tid = threadIdx.x;
  if (tid == 0) s_max = 0;
  int any = 0;
  {
    constexpr int rw = kPostW + 2 * kPostHalo;
    for (int i = tid; i < rw * kPostRows; i += 256) {
      const int ry = i / rw, rx = i - ry * rw;
      const int gy = ty0 - kPostHalo + ry, gx = tx0 - kPostHalo + rx;
      if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
      const int e = map[(size_t)gy * W + gx] == 2;
      any |= e;
      sa[ry * kPostStride + rx] = e ? 255 : 0;
    }
  }
  unsigned char* dst = dst_base + d.pix;
  if (!__syncthreads_or(any)) {   // no edge within reach of this tile (most tiles of a photo): every stage gives 0
    for (int i = tid; i < kPostW * kPostH; i += 256) {
      const int gy = ty0 + i / kPostW, gx = tx0 + i % kPostW;
      if (gy < H && gx < W) dst[(size_t)gy * W + gx] = 0;
    }
    return;
  }
  post_morph<true>(sa, sb, 4, ty0, tx0, H, W);
  __syncthreads();
  post_morph<false>(sb, sa, 3, ty0, tx0, H, W);
  __syncthreads();
  post_morph<true>(sa, sb, 2, ty0, tx0, H, W);
  __syncthreads();
  post_morph<false>(sb, sa, 1, ty0, tx0, H, W);
  __syncthreads();
  int mx = 0;
  for (int i = tid; i < kPostW * kPostH; i += 256) {
    const int ry = i / kPostW, rx = i - ry * kPostW;
    const int gy = ty0 + ry, gx = tx0 + rx;
    if (gy >= H || gx >= W) continue;
    int v = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const unsigned char* row = sa + (reflect101(gy + dy - 1, H) - ty0 + kPostHalo) * kPostStride;
      int h = 0;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) h += (dx == 1 ? 128 : 64) * (int)row[reflect101(gx + dx - 1, W) - tx0 + kPostHalo];
      v += (dy == 1 ? 128 : 64) * h;
    }
    const int o = min((v + (1 << 15)) >> 16, 255);
    dst[(size_t)gy * W + gx] = (unsigned char)o;
    mx = max(mx, o);
  }
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0 && mx > 0) atomicMax(&s_max, mx);
  __syncthreads();
  if (tid == 0 && s_max > 0) atomicMax(&cnt[2 * blockIdx.z + 1], s_max);
}

// normalized_edges = uint8(edges / max * 255) in double (truncating), then
// cv::addWeighted(base, 0.7, edges, 0.3, 0): fp32 fma(a, .7f, fma(b, .3f, 0)),
// round half even, saturate.
__global__ void b_edge_blend_kernel(BTable T, BIn base_in, const unsigned char* __restrict__ edges_base,
                                    const int* __restrict__ cnt, unsigned char* __restrict__ dst_base) {
  const BImg& d = T.d[blockIdx.y];
  const int W = d.W;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.H * W) return;
  int pitch;
  const unsigned char* base = b_in(d, base_in, &pitch);
  const int y = i / W, x = i - y * W;
  const int mx = cnt[2 * blockIdx.y + 1];
  int e = edges_base[d.pix + i];
  if (mx > 0) e = (int)((double)e / (double)mx * 255.0);
  const float t = __fmaf_rn((float)base[(size_t)y * pitch + x], 0.7f, __fmaf_rn((float)e, 0.3f, 0.f));
  dst_base[d.pix + i] = (unsigned char)min(max(__float2int_rn(t), 0), 255);
}

// Pillow precompute_coeffs (bilinear, support 1) + normalize_coeffs_8bpc, one
// thread per output coordinate.
// grid (outputs, 2, images): y = 0 the horizontal table, 1 the vertical one;
// bounds [image][out][2], kk at the image's offset, [out][ksize]
__global__ void b_resize_coeffs_kernel(BTable T, int out_w, int out_h, int* __restrict__ bx, int* __restrict__ kkx,
                                       int* __restrict__ by, int* __restrict__ kky) {
  const BImg& d = T.d[blockIdx.z];
  const bool vert = blockIdx.y != 0;
  const int in_size = vert ? d.H : d.W, out_size = vert ? out_h : out_w, ksize = vert ? d.ky : d.kx;
  int* bounds = vert ? by + (size_t)blockIdx.z * 2 * out_h : bx + (size_t)blockIdx.z * 2 * out_w;
  int* kk = vert ? kky + d.kky : kkx + d.kkx;
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= out_size) return;
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filterscale;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double w[64];
  double ww = 0.0;
  for (int x = 0; x < xmax && x < 64; ++x) {
    double t = (x + xmin - center + 0.5) * ss;
    t = t < 0.0 ? -t : t;
    w[x] = t < 1.0 ? 1.0 - t : 0.0;
    ww += w[x];
  }
  for (int x = 0; x < ksize; ++x) {
    int v = 0;
    if (x < xmax) {
      const double k = ww != 0.0 ? w[x] / ww : w[x];
      v = k < 0 ? (int)(-0.5 + k * (1 << kPrecisionBits)) : (int)(0.5 + k * (1 << kPrecisionBits));
    }
    kk[(size_t)xx * ksize + x] = v;
  }
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

// horizontal pass of the images whose width changes: rows [y0, y1) -> tmp [rows][OW][C]
__global__ void b_resize_h_kernel(BTable T, BIn in, int OW, const int* __restrict__ bx, const int* __restrict__ kkx,
                                  unsigned char* __restrict__ tmp_base) {
  const BImg& d = T.d[blockIdx.y];
  if (d.W == OW) return;
  const int C = in.C, rows = d.y1 - d.y0, ksize = d.kx;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * OW * C) return;
  int pitch;
  const unsigned char* src = b_in(d, in, &pitch);
  const int* bounds = bx + (size_t)blockIdx.y * 2 * OW;
  const int* kk = kkx + d.kkx;
  const int c = i % C, xx = (i / C) % OW, y = (int)(i / ((long)C * OW));
  const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
  const unsigned char* row = src + (size_t)(d.y0 + y) * pitch;
  int acc = 1 << (kPrecisionBits - 1);
  for (int x = 0; x < n; ++x) acc += (int)row[(xmin + x) * C + c] * kk[xx * ksize + x];
  tmp_base[d.tmp + i] = clip8(acc);
}

// vertical pass + ToTensor + Normalize into dst [image][C][OH][OW]; an image
// whose width does not change is read in place (all its rows, at its pitch)
__global__ void b_resize_v_norm_kernel(BTable T, BIn in, const unsigned char* __restrict__ tmp_base, int OW, int OH,
                                       const int* __restrict__ by, const int* __restrict__ kky, float m0, float m1,
                                       float m2, float s0, float s1, float s2, float* __restrict__ dst) {
  const BImg& d = T.d[blockIdx.y];
  const int C = in.C, ksize = d.ky;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)OH * OW * C) return;
  int pitch;
  const unsigned char* tmp = b_in(d, in, &pitch);
  if (d.W != OW) {
    tmp = tmp_base + d.tmp;
    pitch = OW * C;
  }
  const int* bounds = by + (size_t)blockIdx.y * 2 * OH;
  const int* kk = kky + d.kky;
  const int xx = i % OW, yy = (i / OW) % OH, c = (int)(i / ((long)OW * OH));
  const int ymin = bounds[2 * yy] - d.y0, n = bounds[2 * yy + 1];
  int acc = 1 << (kPrecisionBits - 1);
  for (int y = 0; y < n; ++y) acc += (int)tmp[(size_t)(ymin + y) * pitch + xx * C + c] * kk[yy * ksize + y];
  const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
  const float x = (float)clip8(acc) / 255.f;
  dst[(size_t)blockIdx.y * C * OH * OW + i] = (x - mean) / sd;
}

// The launcher body of both entry points.  who: the entry point that was
// called, for error messages; index_images: a check that fails on one image
// names it ("image <i>: ...", the batched entry).
int preprocess_images(const char* who, bool index_images, const uint8_t* const* srcs, const int* heights,
                      const int* widths, const int* pitches, int n, int C, int flags, float clip_limit, int tiles_x,
                      int tiles_y, int out_h, int out_w, const float* mean, const float* std_, float* dst,
                      void* stream) {
  auto einval = [&](const std::string& what) { return kpd_fail_einval((std::string(who) + ": " + what).c_str()); };
  if (n <= 0) return einval("n must be positive");
  if (!srcs || !heights || !widths || !pitches || !dst || !mean || !std_) return einval("null pointer");
  if (out_h <= 0 || out_w <= 0 || (C != 1 && C != 3)) return einval("bad arguments");
  if ((flags & KPD_PRE_GRAY) && C != 3) return einval("GRAY needs 3-channel images");
  if ((flags & KPD_PRE_EDGES) && !((flags & KPD_PRE_GRAY) || C == 1))
    return einval("EDGES needs a single-plane (gray) pipeline");
  const int Co = (flags & KPD_PRE_GRAY) ? 1 : C;
  auto bad = [&](int i, const char* what) {
    return einval(index_images ? "image " + std::to_string(i) + ": " + what : std::string(what));
  };
  // per-image geometry and the prefix sums that carve the scratch
  std::vector<BImg> imgs((size_t)n);
  long long pix = 0, tmp = 0, kkx = 0, kky = 0;
  for (int i = 0; i < n; ++i) {
    const int H = heights[i], W = widths[i];
    if (!srcs[i] || H <= 0 || W <= 0) return bad(i, "bad arguments");
    if (pitches[i] < W * C) return bad(i, "pitch below width * channels");
    if ((flags & KPD_PRE_CLAHE) && (tiles_x <= 0 || tiles_y <= 0 || tiles_x > W || tiles_y > H))
      return bad(i, "bad CLAHE tile grid");
    BImg& d = imgs[(size_t)i];
    d = BImg{};
    d.src = srcs[i];
    d.H = H;
    d.W = W;
    d.pitch = pitches[i];
    if (flags & KPD_PRE_CLAHE) {
      const int Hp = H % tiles_y ? H + tiles_y - H % tiles_y : H, Wp = W % tiles_x ? W + tiles_x - W % tiles_x : W;
      d.tw = Wp / tiles_x;
      d.th = Hp / tiles_y;
      const int area = d.tw * d.th;
      d.clip = clip_limit > 0.f ? std::max((int)(clip_limit * area / 256), 1) : 0;
    }
    const double sx = (double)W / out_w, sy = (double)H / out_h;
    d.kx = (int)std::ceil(std::max(sx, 1.0)) * 2 + 1;
    d.ky = (int)std::ceil(std::max(sy, 1.0)) * 2 + 1;
    if (d.kx > 64 || d.ky > 64) return bad(i, "downscale factor > 31 not supported");
    d.y0 = 0;
    d.y1 = H;
    if (out_w != W && out_h != H) {   // rows the vertical pass reads: PIL's ybox [first, last)
      int f0, fn, l0, ln;
      pil_bounds(H, out_h, 0, &f0, &fn);
      pil_bounds(H, out_h, out_h - 1, &l0, &ln);
      d.y0 = f0;
      d.y1 = l0 + ln;
    }
    d.pix = pix;
    d.tmp = tmp;
    d.kkx = kkx;
    d.kky = kky;
    pix += (long long)H * W;
    if (out_w != W) tmp += (long long)(d.y1 - d.y0) * out_w * Co;
    kkx += (long long)out_w * d.kx;
    kky += (long long)out_h * d.ky;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // one stream-ordered allocation, carved into regions over all images
  size_t total = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = total;
    total += (bytes + 255) & ~(size_t)255;
    return o;
  };
  const size_t N = (size_t)pix, lut_img = (size_t)Co * tiles_y * tiles_x * 256;
  const bool gray = flags & KPD_PRE_GRAY, clahe = flags & KPD_PRE_CLAHE, edges = flags & KPD_PRE_EDGES,
             blur = flags & KPD_PRE_BLUR;
  const size_t o_gray = gray ? carve(N) : 0;
  const size_t o_luts = clahe ? carve((size_t)n * lut_img) : 0, o_clahe = clahe ? carve(N * Co) : 0;
  const size_t o_d0 = edges ? carve(N) : 0, o_d1 = edges ? carve(N) : 0, o_blend = edges ? carve(N) : 0;
  const size_t o_dxy = edges ? carve(sizeof(int) * 2 * N) : 0, o_mag = edges ? carve(sizeof(int) * N) : 0;
  const size_t o_map = edges ? carve(sizeof(int) * N) : 0, o_queue = edges ? carve(sizeof(int) * N) : 0;
  const size_t o_cnt = edges ? carve(sizeof(int) * 2 * (size_t)n) : 0;
  const size_t o_blur = blur ? carve(N * Co) : 0;
  const size_t o_bx = carve(sizeof(int) * 2 * (size_t)n * out_w), o_by = carve(sizeof(int) * 2 * (size_t)n * out_h);
  const size_t o_kkx = carve(sizeof(int) * (size_t)kkx), o_kky = carve(sizeof(int) * (size_t)kky);
  const size_t o_tmp = carve((size_t)tmp);
  unsigned char* base = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&base), total, st);
  if (e != hipSuccess) return kpd_fail_hip(e, (std::string(who) + ": scratch").c_str());
  int rc = KPD_OK;
  auto fail_hip = [&](hipError_t err) {
    if (err != hipSuccess && rc == KPD_OK) rc = kpd_fail_hip(err, who);
  };
  auto* dxy = reinterpret_cast<int*>(base + o_dxy);
  auto* mag = reinterpret_cast<int*>(base + o_mag);
  auto* map = reinterpret_cast<int*>(base + o_map);
  auto* queue = reinterpret_cast<int*>(base + o_queue);
  auto* cnt = reinterpret_cast<int*>(base + o_cnt);
  auto* bx = reinterpret_cast<int*>(base + o_bx);
  auto* by = reinterpret_cast<int*>(base + o_by);
  auto* kkxp = reinterpret_cast<int*>(base + o_kkx);
  auto* kkyp = reinterpret_cast<int*>(base + o_kky);
  if (edges) fail_hip(hipMemsetAsync(cnt, 0, sizeof(int) * 2 * (size_t)n, st));
  const float m1 = Co > 1 ? mean[1] : 0.f, m2 = Co > 2 ? mean[2] : 0.f;
  const float s1 = Co > 1 ? std_[1] : 1.f, s2 = Co > 2 ? std_[2] : 1.f;
  const dim3 tb(256);
  struct Chunk {
    BTable T;
    int c0, m, max_h, max_w;
    long max_px, max_tmp;
  };
  std::vector<Chunk> chunks;
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    Chunk c{};
    c.c0 = c0;
    c.m = std::min(kChunk, n - c0);
    for (int i = 0; i < c.m; ++i) {
      const BImg& d = c.T.d[i] = imgs[(size_t)(c0 + i)];
      c.max_px = std::max(c.max_px, (long)d.H * d.W);
      c.max_h = std::max(c.max_h, d.H);
      c.max_w = std::max(c.max_w, d.W);
      if (out_w != d.W) c.max_tmp = std::max(c.max_tmp, (long)(d.y1 - d.y0) * out_w * Co);
    }
    chunks.push_back(c);
  }
  unsigned char *d0 = base + o_d0, *d1 = base + o_d1;
  BIn cur{nullptr, C};
  // up to the Canny seeds, chunk by chunk
  for (const Chunk& c : chunks) {
    const BTable& T = c.T;
    const dim3 g1(blocks(c.max_px), c.m), gc(blocks(c.max_px * Co), c.m);
    cur = BIn{nullptr, C};
    if (gray) {
      hipLaunchKernelGGL(b_rgb2gray_kernel, g1, tb, 0, st, T, base + o_gray);
      cur = BIn{base + o_gray, 1};
    }
    if (clahe) {
      unsigned char* luts = base + o_luts + (size_t)c.c0 * lut_img;
      hipLaunchKernelGGL(b_clahe_lut_kernel, dim3(tiles_x, tiles_y, Co * c.m), tb, 0, st, T, cur, tiles_x, tiles_y,
                         luts);
      hipLaunchKernelGGL(b_clahe_apply_kernel, gc, tb, 0, st, T, cur, tiles_x, tiles_y, luts, base + o_clahe);
      cur = BIn{base + o_clahe, Co};
    }
    if (edges) {   // to_grayscale_clahe's edge blend (transforms.py:55-73), first half
      hipLaunchKernelGGL(b_gauss_fixed_kernel<5>, g1, tb, 0, st, T, cur, gauss_taps(5, 1.5), d0);
      hipLaunchKernelGGL(b_median5_kernel, g1, tb, 0, st, T, d0, d1);
      hipLaunchKernelGGL(b_canny_grad_kernel, g1, tb, 0, st, T, d1, dxy, mag);
      hipLaunchKernelGGL(b_canny_nms_kernel, g1, tb, 0, st, T, dxy, mag, 100, 200, map, queue, cnt + 2 * (size_t)c.c0);
    }
    fail_hip(hipGetLastError());
  }
  // the floods, kHystChunk images per launch
  for (int h0 = 0; edges && h0 < n; h0 += kHystChunk) {
    const int m = std::min(kHystChunk, n - h0);
    HTable T{};
    for (int i = 0; i < m; ++i) {
      const BImg& d = imgs[(size_t)(h0 + i)];
      T.pix[i] = d.pix;
      T.H[i] = d.H;
      T.W[i] = d.W;
    }
    hipLaunchKernelGGL(b_canny_hyst_kernel, dim3(m), dim3(1024), 0, st, T, map, queue, cnt + 2 * (size_t)h0);
    fail_hip(hipGetLastError());
  }
  // behind the floods, chunk by chunk
  for (const Chunk& c : chunks) {
    const BTable& T = c.T;
    const dim3 g1(blocks(c.max_px), c.m), gc(blocks(c.max_px * Co), c.m);
    BIn in = cur;
    if (edges) {
      int* ccnt = cnt + 2 * (size_t)c.c0;
      hipLaunchKernelGGL(b_post_canny_kernel,
                         dim3((c.max_w + kPostW - 1) / kPostW, (c.max_h + kPostH - 1) / kPostH, c.m), tb, 0, st, T,
                         map, d0, ccnt);
      hipLaunchKernelGGL(b_edge_blend_kernel, g1, tb, 0, st, T, in, d0, ccnt, base + o_blend);
      in = BIn{base + o_blend, 1};
    }
    if (blur) {   // GaussianBlur((3, 3), 0.5) of to_rgb_clahe
      hipLaunchKernelGGL(b_gauss_fixed_kernel<3>, gc, tb, 0, st, T, in, gauss_taps(3, 0.5), base + o_blur);
      in = BIn{base + o_blur, Co};
    }
    // PIL bilinear resize (horizontal pass first) + ToTensor + Normalize
    int* cbx = bx + (size_t)c.c0 * 2 * out_w;
    int* cby = by + (size_t)c.c0 * 2 * out_h;
    hipLaunchKernelGGL(b_resize_coeffs_kernel, dim3(blocks(std::max(out_w, out_h)), 2, c.m), tb, 0, st, T, out_w,
                       out_h, cbx, kkxp, cby, kkyp);
    if (c.max_tmp > 0)
      hipLaunchKernelGGL(b_resize_h_kernel, dim3(blocks(c.max_tmp), c.m), tb, 0, st, T, in, out_w, cbx, kkxp,
                         base + o_tmp);
    hipLaunchKernelGGL(b_resize_v_norm_kernel, dim3(blocks((long)out_h * out_w * Co), c.m), tb, 0, st, T, in,
                       base + o_tmp, out_w, out_h, cby, kkyp, mean[0], m1, m2, std_[0], s1, s2,
                       dst + (size_t)c.c0 * Co * out_h * out_w);
    fail_hip(hipGetLastError());
  }
  (void)hipFreeAsync(base, st);
  return rc;
}

}  // namespace

extern "C" int kpd_preprocess_batch(const uint8_t* const* srcs, const int* heights, const int* widths,
                                    const int* pitches, int n, int C, int flags, float clip_limit, int tiles_x,
                                    int tiles_y, int out_h, int out_w, const float* mean, const float* std_,
                                    float* dst, void* stream) {
  return preprocess_images("kpd_preprocess_batch", true, srcs, heights, widths, pitches, n, C, flags, clip_limit,
                           tiles_x, tiles_y, out_h, out_w, mean, std_, dst, stream);
}

// the n = 1 case; the one-element arrays are read before the call returns
extern "C" int kpd_preprocess(const uint8_t* src, int H, int W, int C, int pitch, int flags, float clip_limit,
                              int tiles_x, int tiles_y, int out_h, int out_w, const float* mean, const float* std_,
                              float* dst, void* stream) {
  return preprocess_images("kpd_preprocess", false, &src, &H, &W, &pitch, 1, C, flags, clip_limit, tiles_x, tiles_y,
                           out_h, out_w, mean, std_, dst, stream);
}
