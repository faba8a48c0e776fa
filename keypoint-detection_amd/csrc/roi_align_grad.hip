// ROI-align backward: the adjoint of the forward's ROI align
// (roi_row_sample in head_kernels.hip, kpd_roi_features; torchvision
// roi_align, aligned=False, sampling_ratio=-1, 56 x 56 bins) onto FPN level 0,
// as a gather -- no floating-point atomics, every gfeat element stored once.
//
// ROI align is separable: out[c] = My . F[c] . Mx^T / count with banded
// interpolation matrices My [56][H], Mx [56][W] that depend on the box alone,
// so
//   dF[c][y][x] = sum over the image's ROIs, ascending row
//                 sum_p sum_q (My[p][y] / count) Mx[q][x] G[c][p][q]       (p, q ascending)
//
// One workgroup owns (image, band of RB whole rows, CC consecutive channels):
// a thread owns up to QPT quads of 4 consecutive pixels of a row and their CC
// accumulators in registers through every ROI of the image, and stores them
// once (16-byte stores when W % 4 == 0).  Per ROI the workgroup builds the two
// matrices in LDS in a compact form: for a pixel column x the bins q with
// Mx[q][x] != 0 are consecutive, q in [qlo[x], qhi[x]], and only the columns
// of the ROI's footprint have any, so the table is footprint x (longest band)
// floats.  With s = the ROI's extent in pixels (1 <= s <= W), g = ceil(s / 56)
// and sample spacing s / (56 g) <= 1, the footprint is at most s + 3 columns
// and a band at most min(56, 112 / s + 3) bins: at most 3 W + 512 floats, and
// for the row band min(RB x 56, 3 H + 512); the host caps RB by the LDS that
// the staged planes and the column tables leave (tests/test_roi_align_backward
// sweeps the extent over [1, W] and [1, H] against the reference to pin the
// bound: the kernel clamps a band to the capacity, which would drop terms).
// An entry is gathered, not scattered: the samples i = 0 .. g-1 of bin q that
// fall on column x, their weights summed in double in ascending i and rounded
// to fp32 once (1 / count folded into My).  The
// sample coordinates are computed in fp32 in torchvision's expression order
// with contraction off, and the skip / clamp decisions are made on them, as
// roi_align_nchw_kernel (ops_kernels.hip) does and explains.  The gradient
// rows p the band needs are staged in LDS for the workgroup's selected
// channels (16-byte loads); channels that topk[b] does not select, images
// without a row and pixels outside every footprint keep their zero
// accumulators.  A workgroup reads its own image's rows only, in their order
// in `rows`: an image's gradient does not depend on its batch, and two calls
// give the same bits.
//
// Rounding: a term w G with w = fl(My') fl(Mx) carries three roundings and the
// N terms of an element are added by fma in a fixed order:
// |got - exact| <= (N + 3) 2^-24 sum|term|, inside the tests' (N + 2) 2^-23.
#include <climits>
#include <cstdint>
#include <cmath>

#include "../../include/kpd.h"
#include "kpd_common.h"
#include "kpd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int RS = 56, PLANE = RS * RS;   // ROI bins per side, one gradient plane
constexpr int NT = 256;                   // threads per workgroup
constexpr int CC = 4;                     // channels per workgroup
constexpr int QPT = 3;                    // pixel quads per thread
constexpr size_t kLdsLimit = 64 * 1024;

struct AxisGeom {
  float start, bin;
  int grid, size;
};

// Sample i of bin p along one axis: torchvision's coordinate and decisions.
__device__ __forceinline__ bool axis_sample(const AxisGeom& a, int p, int i, int* lo, int* hi, float* l) {
  const float c0 = a.start + (float)p * a.bin + ((float)i + 0.5f) * a.bin / (float)a.grid;
  if (!(c0 == c0) || c0 < -1.f || c0 > (float)a.size) return false;
  float c = c0 <= 0.f ? 0.f : c0;
  int lw = (int)c, hg;
  if (lw >= a.size - 1) {
    hg = lw = a.size - 1;
    c = (float)lw;
  } else {
    hg = lw + 1;
  }
  *lo = lw;
  *hi = hg;
  *l = c - (float)lw;
  return true;
}

// M[p][col]: the weights of bin p's samples on pixel column col, in double
__device__ __forceinline__ double axis_weight(const AxisGeom& a, int p, int col) {
  double w = 0.0;
  for (int i = 0; i < a.grid; ++i) {
    int lo, hi;
    float l;
    if (!axis_sample(a, p, i, &lo, &hi, &l)) continue;
    if (lo == col) w += 1.0 - (double)l;
    if (hi == col) w += (double)l;
  }
  return w;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

struct GradArgs {
  const float* gout;
  const float* boxes;
  const int32_t* rows;
  const int32_t* topk;
  float* gfeat;
  int n, B, P, Cs, C, H, W;
  int RB, nbands, nchunks, capx, capy;   // rows per band, grid factors, table capacities (floats)
  int vec_in, vec_out;                   // 16-byte loads of gout / stores of gfeat
};

__global__ __launch_bounds__(NT) void roi_align_backward_kernel(const GradArgs a) {
  __shared__ __attribute__((aligned(16))) float Gs[CC * PLANE];
  __shared__ int cmin[2 * RS], cmax[2 * RS];   // per bin: first / last pixel column its samples touch (x, then y)
  __shared__ int foot0[2], foot1[2];           // the ROI's footprint per axis
  __shared__ int red[4][4];
  __shared__ int slot_cc[CC], sel_slot[CC], sel_cc[CC], nsel_sm;
  extern __shared__ __attribute__((aligned(16))) int dyn[];
  const int W = a.W, H = a.H, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* qlo = dyn;                 // [W]   bins of a pixel column, relative to the footprint's first column
  int* qhi = qlo + W;             // [W]
  int* plo = qhi + W;             // [RB]
  int* phi = plo + a.RB;          // [RB]
  float* MxB = reinterpret_cast<float*>(phi + a.RB);   // [capx]
  float* MyB = MxB + a.capx;                            // [capy]

  int wg = blockIdx.x;
  const int chunk = wg % a.nchunks;
  wg /= a.nchunks;
  const int band = wg % a.nbands, b = wg / a.nbands;
  const int c0 = chunk * CC, yb0 = band * a.RB, yb1 = min(yb0 + a.RB, H);   // rows [yb0, yb1)
  const int QW = (W + 3) >> 2, nquads = (yb1 - yb0) * QW;

  // the chunk's channels that topk[b] selects, ascending, and their slots
  if (tid < CC) slot_cc[tid] = a.topk ? -1 : (c0 + tid < a.C ? c0 + tid : -1);
  __syncthreads();
  if (a.topk)
    for (int s = tid; s < a.Cs; s += NT) {
      const int c = a.topk[(size_t)b * a.Cs + s];
      if (c >= c0 && c < c0 + CC && c < a.C) slot_cc[c - c0] = s;
    }
  __syncthreads();
  if (tid == 0) {
    int k = 0;
    for (int cc = 0; cc < CC; ++cc)
      if (slot_cc[cc] >= 0) {
        sel_slot[k] = slot_cc[cc];
        sel_cc[k] = cc;
        ++k;
      }
    nsel_sm = k;
    for (; k < CC; ++k) sel_slot[k] = 0, sel_cc[k] = -1;
  }
  __syncthreads();
  const int nsel = nsel_sm;

  float acc[QPT][4][CC];
#pragma unroll
  for (int kq = 0; kq < QPT; ++kq)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < CC; ++k) acc[kq][j][k] = 0.f;

  // the image's rows: rows is ascending, so they are consecutive from the first one >= b P
  int i0 = 0;
  {
    int hi = a.n;
    const int key = b * a.P;
    while (i0 < hi) {
      const int mid = (i0 + hi) >> 1;
      if (a.rows[mid] < key) i0 = mid + 1; else hi = mid;
    }
  }
  for (int i = i0; nsel > 0 && i < a.n; ++i) {
    const int row = a.rows[i];
    if (row < b * a.P || row >= (b + 1) * a.P) break;
    // the box as a ROI: roi_row_sample's expressions
    const float* bx = a.boxes + (size_t)row * 4;
    const float cx = bx[0], cy = bx[1], bw = bx[2], bh = bx[3];
    const float x1 = fminf(fmaxf(cx - bw / 2.f, 0.f), 1.f) * (float)W;
    const float y1 = fminf(fmaxf(cy - bh / 2.f, 0.f), 1.f) * (float)H;
    const float x2 = fminf(fmaxf(cx + bw / 2.f, 0.f), 1.f) * (float)W;
    const float y2 = fminf(fmaxf(cy + bh / 2.f, 0.f), 1.f) * (float)H;
    const float roi_w = fmaxf(x2 - x1, 1.f), roi_h = fmaxf(y2 - y1, 1.f);
    AxisGeom ax, ay;
    ax.start = x1;
    ax.bin = roi_w / (float)RS;
    ax.grid = (int)ceilf(roi_w / (float)RS);
    ax.size = W;
    ay.start = y1;
    ay.bin = roi_h / (float)RS;
    ay.grid = (int)ceilf(roi_h / (float)RS);
    ay.size = H;
    const double inv_count = 1.0 / (double)max(ax.grid * ay.grid, 1);

    __syncthreads();   // the previous ROI's accumulation is done with the tables and Gs
    // A: the pixel columns every bin touches (wave 0: x, wave 1: y), and the footprint
    if (tid < 128) {
      const AxisGeom& g = wave ? ay : ax;
      int mn = INT_MAX, mx = -1;
      if (lane < RS) {
        for (int s = 0; s < g.grid; ++s) {
          int lo, hi;
          float l;
          if (axis_sample(g, lane, s, &lo, &hi, &l)) {
            mn = min(mn, lo);
            mx = max(mx, hi);
          }
        }
        cmin[wave * RS + lane] = mn;
        cmax[wave * RS + lane] = mx;
      }
      mn = wave_min_i(mn);
      mx = wave_max_i(mx);
      if (lane == 0) {
        foot0[wave] = mn;
        foot1[wave] = mx;
      }
    }
    __syncthreads();
    const int xf0 = foot0[0], xf1 = foot1[0];
    const int ya = max(foot0[1], yb0), yz = min(foot1[1], yb1 - 1);   // the footprint's rows inside the band
    if (xf0 > xf1 || ya > yz) continue;   // (uniform) nothing of this ROI lands in the band
    // B: per pixel column / row the band of bins, the longest band, the bins' range over the row band
    int lenx = 0, leny = 0, pmn = RS, pmx = -1;
    for (int x = xf0 + tid; x <= xf1; x += NT) {
      int lo = RS, hi = -1;
      for (int q = 0; q < RS; ++q)
        if (cmin[q] <= x && x <= cmax[q]) {
          lo = min(lo, q);
          hi = q;
        }
      qlo[x - xf0] = lo;
      qhi[x - xf0] = hi;
      lenx = max(lenx, hi - lo + 1);
    }
    for (int y = ya + tid; y <= yz; y += NT) {
      int lo = RS, hi = -1;
      for (int p = 0; p < RS; ++p)
        if (cmin[RS + p] <= y && y <= cmax[RS + p]) {
          lo = min(lo, p);
          hi = p;
        }
      plo[y - ya] = lo;
      phi[y - ya] = hi;
      leny = max(leny, hi - lo + 1);
      if (hi >= lo) {
        pmn = min(pmn, lo);
        pmx = max(pmx, hi);
      }
    }
    lenx = wave_max_i(lenx);
    leny = wave_max_i(leny);
    pmn = wave_min_i(pmn);
    pmx = wave_max_i(pmx);
    if (lane == 0) {
      red[wave][0] = lenx;
      red[wave][1] = leny;
      red[wave][2] = pmn;
      red[wave][3] = pmx;
    }
    __syncthreads();
    int KBx = max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0]));
    int KBy = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
    const int pmin = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
    const int pmax = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
    if (KBx <= 0 || KBy <= 0 || pmax < pmin) continue;   // (uniform)
    const int nfx = xf1 - xf0 + 1, nfy = yz - ya + 1;
    // the tables fit by the bound in the header; the clamps keep the LDS writes in range regardless
    if (nfx * KBx > a.capx) KBx = a.capx / nfx;
    if (nfy * KBy > a.capy) KBy = a.capy / nfy;
    // C: the two tables
    for (int e = tid; e < nfx * KBx; e += NT) {
      const int xi = e / KBx, q = qlo[xi] + (e - xi * KBx);
      MxB[e] = q <= qhi[xi] ? (float)axis_weight(ax, q, xf0 + xi) : 0.f;
    }
    for (int e = tid; e < nfy * KBy; e += NT) {
      const int yi = e / KBy, p = plo[yi] + (e - yi * KBy);
      MyB[e] = p <= phi[yi] ? (float)(axis_weight(ay, p, ya + yi) * inv_count) : 0.f;
    }
    // the gradient rows pmin .. pmax of the selected channels
    const int nstage = (pmax - pmin + 1) * RS;
    for (int k = 0; k < nsel; ++k) {
      const float* src = a.gout + ((size_t)i * a.Cs + sel_slot[k]) * PLANE + pmin * RS;
      float* dst = Gs + k * PLANE;
      if (a.vec_in) {
        for (int e = tid; e < nstage / 4; e += NT)
          reinterpret_cast<float4*>(dst)[e] = reinterpret_cast<const float4*>(src)[e];
      } else {
        for (int e = tid; e < nstage; e += NT) dst[e] = src[e];
      }
    }
    __syncthreads();
    // accumulate: p, then q ascending, the CC channels innermost
#pragma unroll
    for (int kq = 0; kq < QPT; ++kq) {
      const int id = tid + NT * kq;
      if (id >= nquads) continue;
      const int yl = id / QW, y = yb0 + yl, xq = (id - yl * QW) * 4;
      if (y < ya || y > yz) continue;
      const int yi = y - ya, p0 = plo[yi], p1 = min(phi[yi], p0 + KBy - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = xq + j;
        if (x >= xf0 && x <= xf1) {
          const int xi = x - xf0, q0 = qlo[xi], q1 = min(qhi[xi], q0 + KBx - 1);
          for (int p = p0; p <= p1; ++p) {
            const float wy = MyB[yi * KBy + p - p0];
            const float* gp = Gs + (p - pmin) * RS;
            for (int q = q0; q <= q1; ++q) {
              const float w = wy * MxB[xi * KBx + q - q0];
#pragma unroll
              for (int k = 0; k < CC; ++k)
                if (k < nsel) acc[kq][j][k] = fmaf(w, gp[k * PLANE + q], acc[kq][j][k]);
            }
          }
        }
      }
    }
  }

  // store: every element of the band's CC channel planes once
#pragma unroll
  for (int cc = 0; cc < CC; ++cc) {
    const int c = c0 + cc;
    if (c >= a.C) break;
    float* plane = a.gfeat + ((size_t)b * a.C + c) * H * W;
#pragma unroll
    for (int kq = 0; kq < QPT; ++kq) {
      const int id = tid + NT * kq;
      if (id >= nquads) continue;
      const int yl = id / QW, y = yb0 + yl, xq = (id - yl * QW) * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < CC; ++k)
        if (k < nsel && sel_cc[k] == cc) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = acc[kq][j][k];
        }
      float* dst = plane + (size_t)y * W + xq;
      if (a.vec_out) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (xq + j < W) dst[j] = v[j];
      }
    }
  }
}

}  // namespace

extern "C" int kpd_roi_align_backward(const float* gout, const float* boxes, const int32_t* rows, int n, int B, int P,
                                      const int32_t* topk, int Cs, int C, int H, int W, float* gfeat, void* stream) {
  if (n < 0 || B < 0 || P < 1 || Cs < 1 || C < 1 || H < 1 || W < 1 || Cs > C || (!topk && Cs != C) ||
      (long)B * P > INT_MAX || (long)n > (long)B * P || (B > 0 && !gfeat) || (n > 0 && (!gout || !boxes || !rows)))
    return kpd_fail_einval("kpd_roi_align_backward: bad arguments (need 0 <= n <= B*P, 1 <= Cs <= C, Cs == C without "
                           "topk, non-null gout / boxes / rows / gfeat)");
  if (B == 0) return KPD_OK;
  GradArgs a{};
  const int QW = (W + 3) / 4;
  // LDS: the staged gradient planes and a few hundred bytes of small tables are static; what is left holds
  // the column tables (qlo, qhi, MxB: fixed by W) and the row band's (plo, phi, MyB), which cap RB
  const size_t budget = kLdsLimit - sizeof(float) * CC * PLANE - 2048;
  a.capx = (int)(W * (long)RS < 3L * W + 512 ? W * (long)RS : 3L * W + 512);
  const size_t xbytes = sizeof(int) * 2 * (size_t)W + sizeof(float) * (size_t)a.capx;
  auto ybytes = [&](int rb) {
    const long cap = (long)rb * RS < 3L * H + 512 ? (long)rb * RS : 3L * H + 512;
    return sizeof(int) * 2 * (size_t)rb + sizeof(float) * (size_t)cap;
  };
  if (QW > NT * QPT || xbytes + ybytes(1) > budget)
    return kpd_fail_einval("kpd_roi_align_backward: the level-0 map is too wide for the workgroup's LDS tables "
                           "(W up to about 550)");
  a.RB = (NT * QPT) / QW;
  if (a.RB > H) a.RB = H;
  while (xbytes + ybytes(a.RB) > budget) --a.RB;   // narrow, tall maps: more bands of fewer rows
  a.capy = (int)((long)a.RB * RS < 3L * H + 512 ? (long)a.RB * RS : 3L * H + 512);
  const size_t dyn = xbytes + ybytes(a.RB);
  a.nbands = (H + a.RB - 1) / a.RB;
  a.nchunks = (C + CC - 1) / CC;
  const long wgs = (long)B * a.nbands * a.nchunks;
  if (wgs > INT_MAX) return kpd_fail_einval("kpd_roi_align_backward: B * C * H too large for one launch");
  a.gout = gout;
  a.boxes = boxes;
  a.rows = rows;
  a.topk = topk;
  a.gfeat = gfeat;
  a.n = n;
  a.B = B;
  a.P = P;
  a.Cs = Cs;
  a.C = C;
  a.H = H;
  a.W = W;
  a.vec_in = (reinterpret_cast<uintptr_t>(gout) & 15u) == 0;
  a.vec_out = W % 4 == 0 && (reinterpret_cast<uintptr_t>(gfeat) & 15u) == 0;
  hipLaunchKernelGGL(roi_align_backward_kernel, dim3((unsigned)wgs), dim3(NT), dyn, reinterpret_cast<hipStream_t>(stream),
                     a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KPD_OK : kpd_fail_hip(e, "kpd_roi_align_backward");
}
