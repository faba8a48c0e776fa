// Weight side of the native runtime: the registered state dict (reference
// names) -> BN-folded, NHWC/MFMA-packed device weights, the split (f16 hi + lo)
// copies and the FPN level-0 composite weights.  kpd_plan_finalize packs a
// plan; the run side is kpd_plan.hip.
#include "kpd_plan_int.h"

namespace {

int se_squeeze(int c) {
  const int v = c / 4;
  int n = std::max(8, (int)(v + 4) / 8 * 8);
  if (n < 0.9 * v) n += 8;
  return n;
}

uint16_t f2bf(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// ------------------------------------------------------------------ weight helpers
const HostT* get(kpd_plan* p, const std::string& name, std::string& missing) {
  auto it = p->t.find(name);
  if (it == p->t.end()) {
    missing += name + " ";
    return nullptr;
  }
  return &it->second;
}

template <typename T>
int upload(kpd_plan* p, const std::vector<T>& h, T** out) {
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, std::max<size_t>(h.size(), 1) * sizeof(T)));
  p->allocs.push_back(d);
  if (!h.empty()) HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = reinterpret_cast<T*>(d);
  return KPD_OK;
}

// BN fold: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (+ conv bias * scale)
void bn_fold(const HostT* g, const HostT* b, const HostT* m, const HostT* v, double eps, int n,
             const HostT* conv_bias, std::vector<double>& scale, std::vector<double>& shift) {
  scale.assign(n, 1.0);
  shift.assign(n, 0.0);
  for (int i = 0; i < n; ++i) {
    const double cb = conv_bias ? conv_bias->data[i] : 0.0;
    if (g) {
      const double s = (double)g->data[i] / std::sqrt((double)v->data[i] + eps);
      scale[i] = s;
      shift[i] = (double)b->data[i] - (double)m->data[i] * s + cb * s;
    } else {
      shift[i] = cb;
    }
  }
}

// A packed conv's fp32 weights and bias as uploaded, by conv: kept while
// kpd_plan_finalize runs, for the split packers to read
struct HostConv { std::vector<float> w, b; };
using HostPack = std::map<const DevConv*, HostConv>;

// Dense conv weights [cout][cin][k][k] -> packed [cout_p][k*k][cin_p] with BN scale.
int pack_conv(kpd_plan* p, const std::string& wname, const std::string& bias_name, const std::string& bn,
              double eps, int k, bool bf16, DevConv& dc, std::string& missing, HostPack& host) {
  const HostT* w = get(p, wname, missing);
  const HostT* cb = bias_name.empty() ? nullptr : get(p, bias_name, missing);
  const HostT *g = nullptr, *b = nullptr, *m = nullptr, *v = nullptr;
  if (!bn.empty()) {
    g = get(p, bn + ".weight", missing); b = get(p, bn + ".bias", missing);
    m = get(p, bn + ".running_mean", missing); v = get(p, bn + ".running_var", missing);
  }
  if (!w || (!bias_name.empty() && !cb) || (!bn.empty() && (!g || !b || !m || !v))) return KPD_ESTATE;
  const bool linear = w->shape.size() == 2 && k == 1;   // nn.Linear [out][in] as a 1x1 conv
  if (!linear && (w->shape.size() != 4 || w->shape[2] != k || w->shape[3] != k))
    return fail(KPD_EINVAL, "bad shape for " + wname);
  dc.ws = nullptr;   // split copies belong to the previous finalize's (freed) allocations
  dc.w_exp = 0;
  dc.ws_kc = 0;
  dc.cout = (int)w->shape[0];
  dc.cin = (int)w->shape[1];
  dc.k = k;
  dc.bf16 = bf16;
  dc.cin_p = bf16 ? (dc.cin + 63) / 64 * 64 : pad16(dc.cin);
  dc.cout_p = pad16(dc.cout);
  std::vector<double> scale, shift;
  bn_fold(g, b, m, v, eps, dc.cout, cb, scale, shift);
  const int kk = k * k;
  std::vector<float> pw((size_t)dc.cout_p * kk * dc.cin_p, 0.f);
  for (int co = 0; co < dc.cout; ++co)
    for (int ci = 0; ci < dc.cin; ++ci)
      for (int t = 0; t < kk; ++t)
        pw[((size_t)co * kk + t) * dc.cin_p + ci] =
            (float)((double)w->data[((size_t)co * dc.cin + ci) * kk + t] * scale[co]);
  std::vector<float> pb(dc.cout_p, 0.f);
  for (int co = 0; co < dc.cout; ++co) pb[co] = (float)shift[co];
  if (bf16) {
    std::vector<uint16_t> hb(pw.size());
    for (size_t i = 0; i < pw.size(); ++i) hb[i] = f2bf(pw[i]);
    uint16_t* d = nullptr;
    if (int rc = upload(p, hb, &d)) return rc;
    dc.w = d;
  } else {
    float* d = nullptr;
    if (int rc = upload(p, pw, &d)) return rc;
    dc.w = d;
  }
  if (int rc = upload(p, pb, &dc.b)) return rc;
  host[&dc] = {std::move(pw), std::move(pb)};
  return KPD_OK;
}

int pack_dw(kpd_plan* p, const std::string& pre, int k, int s, int act, DevDW& dw, std::string& missing) {
  const HostT* w = get(p, pre + ".0.weight", missing);
  const HostT *g = get(p, pre + ".1.weight", missing), *b = get(p, pre + ".1.bias", missing);
  const HostT *m = get(p, pre + ".1.running_mean", missing), *v = get(p, pre + ".1.running_var", missing);
  if (!w || !g || !b || !m || !v) return KPD_ESTATE;
  dw.C = (int)w->shape[0];
  dw.Cp = pad16(dw.C);
  dw.k = k; dw.s = s; dw.act = act;
  std::vector<double> scale, shift;
  bn_fold(g, b, m, v, 1e-3, dw.C, nullptr, scale, shift);
  std::vector<float> pw((size_t)k * k * dw.Cp, 0.f), pb(dw.Cp, 0.f);
  for (int c = 0; c < dw.C; ++c) {
    for (int t = 0; t < k * k; ++t) pw[(size_t)t * dw.Cp + c] = (float)(w->data[(size_t)c * k * k + t] * scale[c]);
    pb[c] = (float)shift[c];
  }
  if (int rc = upload(p, pw, &dw.w)) return rc;
  return upload(p, pb, &dw.b);
}

// [rows][cols] (a 1x1 conv / linear weight) -> uploaded as [cols][rows]
int pack_transposed(kpd_plan* p, const std::string& name, int rows, int cols, float** out, std::string& missing) {
  const HostT* w = get(p, name, missing);
  if (!w) return KPD_ESTATE;
  if (w->data.size() != (size_t)rows * cols) return fail(KPD_EINVAL, "bad size for " + name);
  std::vector<float> t((size_t)rows * cols);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = w->data[(size_t)r * cols + c];
  return upload(p, t, out);
}

// BatchNorm as a per-channel affine (scale, shift), padded to cout_p -- for a
// BN that sits behind a non-linearity and cannot be folded into a conv.
// s, t: the host copies (for pack_split_kh).
int pack_bn_affine(kpd_plan* p, const std::string& bn, int cout_p, float** s_out, float** t_out,
                   std::vector<float>& s, std::vector<float>& t, std::string& missing) {
  const HostT *g = get(p, bn + ".weight", missing), *b = get(p, bn + ".bias", missing);
  const HostT *m = get(p, bn + ".running_mean", missing), *v = get(p, bn + ".running_var", missing);
  if (!g || !b || !m || !v) return KPD_ESTATE;
  const int n = (int)g->data.size();
  std::vector<double> sc, sh;
  bn_fold(g, b, m, v, 1e-5, n, nullptr, sc, sh);
  s.assign(cout_p, 0.f);
  t.assign(cout_p, 0.f);
  for (int i = 0; i < n; ++i) { s[i] = (float)sc[i]; t[i] = (float)sh[i]; }
  if (int rc = upload(p, s, s_out)) return rc;
  return upload(p, t, t_out);
}

int pack_plain(kpd_plan* p, const std::string& name, float** out, std::string& missing, size_t expect = 0) {
  const HostT* w = get(p, name, missing);
  if (!w) return KPD_ESTATE;
  if (expect && w->data.size() != expect) return fail(KPD_EINVAL, "bad size for " + name);
  return upload(p, w->data, out);
}

// ------------------------------------------------------------------ split (f16 hi + lo) weights
// The power-of-two scale of a weight set: max|w| * 2^split_exp < 2^15
int split_exp(double max_abs) {
  int e = 0;
  if (max_abs > 0.0) std::frexp(max_abs, &e);
  return std::min(std::max(14 - e, -100), 100);
}

// x = hi + lo to f16 precision each, the difference taken in x's own type
template <typename T>
void split_hl(T x, _Float16* hi, _Float16* lo) {
  *hi = (_Float16)x;
  *lo = (_Float16)(x - (T)*hi);
}

// rows x K values times 2^w_exp -> dst [row][Kp / 32][hi32 | lo32] (one
// 128-byte K-step row per 32 values; dst zeroed by the caller where K < Kp)
template <typename T>
void write_split_rows(const T* src, size_t rows, int K, int Kp, int w_exp, _Float16* dst) {
  for (size_t row = 0; row < rows; ++row)
    for (int k = 0; k < K; ++k) {
      _Float16* o = dst + row * 2 * Kp + (size_t)(k / 32) * 64 + k % 32;
      split_hl(std::ldexp(src[row * K + k], w_exp), o, o + 32);
    }
}

// The split copy of rows x K fp32 weights on the device: one power-of-two
// scale for the set (max|w| * 2^w_exp < 2^15), rows as write_split_rows lays them
int upload_split(kpd_plan* p, const std::vector<float>& w, size_t rows, int K, int Kp, void** ws, int* w_exp) {
  float mx = 0.f;
  for (float v : w) mx = std::max(mx, std::fabs(v));
  *w_exp = split_exp(mx);
  std::vector<_Float16> hl(rows * 2 * Kp, (_Float16)0.f);
  write_split_rows(w.data(), rows, K, Kp, *w_exp, hl.data());
  _Float16* d = nullptr;
  if (int rc = upload(p, hl, &d)) return rc;
  *ws = d;
  return KPD_OK;
}

// Split (fp32-accurate) weights of a heatmap-head 3x3 conv (hmconv_kernel
// SPLIT): the packed fp32 weights [cout_p][9][cin_p] scaled by 2^w_exp so
// max|w| < 2^15, each value as f16 hi + lo, stored per 32 input channels as
// [hi32 | lo32] (one 128-byte K-step row).  Also the output bound constants:
// |y_co| <= |b_co| + sum|w_co| * max|x| <= bc + bs * max|x| (rounded up).
int pack_split_hm(kpd_plan* p, DevConv& dc, const HostPack& host) {
  const int cin = dc.cin_p, kk = dc.k * dc.k;
  if (cin % 32 != 0) return fail(KPD_EINVAL, "split heatmap conv needs cin % 32 == 0");
  const std::vector<float>&w = host.at(&dc).w, &b = host.at(&dc).b;
  double bs = 0.0, bc = 0.0;
  for (int co = 0; co < dc.cout_p; ++co) {
    double sa = 0.0;
    for (size_t i = 0; i < (size_t)kk * cin; ++i) {
      const float v = w[(size_t)co * kk * cin + i];
      sa += std::fabs((double)v);
    }
    bs = std::max(bs, sa);
    bc = std::max(bc, std::fabs((double)b[co]));
  }
  if (int rc = upload_split(p, w, (size_t)dc.cout_p * kk, cin, cin, &dc.ws, &dc.w_exp)) return rc;
  dc.bc = std::nextafter((float)(bc * (1.0 + 1e-6)), INFINITY);
  dc.bs = std::nextafter((float)(bs * (1.0 + 1e-6)), INFINITY);
  return KPD_OK;
}

// Split (fp32-accurate) copy of a 1x1 conv (kh_att2_kernel: KEYPOINT_HEAD's
// spatial-attention 1x1 128 -> 64): the packed fp32
// weights [cout_p][cin_p] scaled by 2^w_exp (max|w| < 2^15), each value as f16
// hi + lo, stored per 32 input channels as [hi32 | lo32] (K zero-padded to 32).
int pack_split_1x1(kpd_plan* p, DevConv& dc, const HostPack& host) {
  if (dc.k != 1 || dc.bf16) return fail(KPD_EINVAL, "split 1x1 copy of a non-1x1 conv");
  const int cin = dc.cin_p, kc = (cin + 31) / 32;
  if (int rc = upload_split(p, host.at(&dc).w, (size_t)dc.cout_p, cin, kc * 32, &dc.ws, &dc.w_exp)) return rc;
  dc.ws_kc = kc;
  return KPD_OK;
}

// KEYPOINT_HEAD convs for hmconv_kernel MODE 2 (keypoint_head.py:22-48,
// 64-90): the parts' output columns side by side from column `col`, taps 0-8
// their 3x3 weights (BN folded), tap 9 (ntap 10) the ResidualBlock's 1x1
// downsample (BN folded) for its own columns, zero elsewhere; columns beyond
// the parts are zero padding.  Per column: bias, the ResidualBlock.bn1 affine
// (ps, pt; 1 and 0 for plain conv + BN + ReLU6 columns) and the downsample
// bias.  Split into f16 hi + lo after one power-of-two scale (as pack_split_hm).
struct KhPart { const DevConv* conv; const DevConv* ds; const std::vector<float>*ps, *pt; int col; };
int pack_split_kh(kpd_plan* p, KhSplit& ks, int cin, int cout, int ntap, std::initializer_list<KhPart> parts,
                  const HostPack& host) {
  std::vector<float> W((size_t)cout * ntap * cin, 0.f), b(cout, 0.f), ps(cout, 1.f), pt(cout, 0.f), bd(cout, 0.f);
  for (const KhPart& q : parts) {
    const DevConv& c = *q.conv;
    if (c.k != 3 || c.bf16 || c.cin_p != cin || q.col + c.cout > cout) return fail(KPD_EINVAL, "KH split pack: shape");
    const std::vector<float>&w = host.at(&c).w, &cb = host.at(&c).b;
    for (int co = 0; co < c.cout; ++co) {
      for (int t = 0; t < 9; ++t)
        for (int ci = 0; ci < cin; ++ci)
          W[((size_t)(q.col + co) * ntap + t) * cin + ci] = w[((size_t)co * 9 + t) * cin + ci];
      b[q.col + co] = cb[co];
    }
    if (q.ps)
      for (int co = 0; co < c.cout; ++co) { ps[q.col + co] = (*q.ps)[co]; pt[q.col + co] = (*q.pt)[co]; }
    if (q.ds) {
      const DevConv& d = *q.ds;
      if (ntap != 10 || d.k != 1 || d.bf16 || d.cin_p != cin || d.cout != c.cout) return fail(KPD_EINVAL, "KH split pack: ds");
      const std::vector<float>&dw = host.at(&d).w, &db = host.at(&d).b;
      for (int co = 0; co < d.cout; ++co) {
        for (int ci = 0; ci < cin; ++ci) W[((size_t)(q.col + co) * ntap + 9) * cin + ci] = dw[(size_t)co * cin + ci];
        bd[q.col + co] = db[co];
      }
    }
  }
  if (int rc = upload_split(p, W, (size_t)cout * ntap, cin, cin, &ks.ws, &ks.w_exp)) return rc;
  ks.cin = cin; ks.cout = cout; ks.ntap = ntap;
  if (int rc = upload(p, b, &ks.b)) return rc;
  if (int rc = upload(p, ps, &ks.ps)) return rc;
  if (int rc = upload(p, pt, &ks.pt)) return rc;
  return upload(p, bd, &ks.bd);
}

// the lateral-1 row (column) offset tap d = -1, 0, 1 of output row (column) 4Y + a reads
static int fpn0x_off(int a, int d) { return a + d < 0 ? -1 : (a + d > 3 ? 1 : 0); }

// Class tables (kpd_kernels.h): groups in order of the first tap that reads
// them; one weight block per distinct lateral term -- the second member of a
// pair must have its first member's groups and takes its offset.  Returns the
// number of group blocks (26), -1 if a class has more than kFpn0xMaxGroups
// groups or a pair's groups differ.
int fpn0x_class_table(int cls_ng[16], int cls_g[16][kFpn0xMaxGroups], int cls_woff[16]) {
  int woff = 0, blocks = 0;
  for (int cls = 0; cls < 16; ++cls) {
    const int a = cls >> 2, b = cls & 3;
    int ng = 0;
    for (int g = 0; g < kFpn0xMaxGroups; ++g) cls_g[cls][g] = 0;
    for (int t = 0; t < 9; ++t) {
      const int gg = (fpn0x_off(a, t / 3 - 1) + 1) * 3 + (fpn0x_off(b, t % 3 - 1) + 1);
      int g = 0;
      while (g < ng && cls_g[cls][g] != gg) ++g;
      if (g == ng) {
        if (ng == kFpn0xMaxGroups) return -1;
        cls_g[cls][ng++] = gg;
      }
    }
    cls_ng[cls] = ng;
    if (const int first = kFpn0xPairFirst[cls]; first >= 0) {
      if (first >= cls || kFpn0xPairFirst[first] >= 0 || cls_ng[first] != ng) return -1;
      for (int g = 0; g < ng; ++g)
        if (cls_g[first][g] != cls_g[cls][g]) return -1;
      cls_woff[cls] = cls_woff[first];
      continue;
    }
    cls_woff[cls] = woff;
    woff += 128 * ng * 128 * 2;   // f16 elements (hi + lo)
    blocks += ng;
  }
  return blocks;
}

// FPN level 0 by linearity (fpn0x_kernel): W0 = W3 . L0 (the 3x3 conv on the
// 16-channel stem tap through the bias-free lateral 0) and, per output position
// class (y % 4, x % 4), the 3x3 taps summed by the lateral-1 pixel they read
// after the exact 4x nearest upsample.  Products in double; split into f16
// hi + lo after a power-of-two scale (one per weight set).
// One weight block per distinct lateral term: the second member of a class
// pair (kFpn0xPairFirst) is checked bit-equal to the first and dropped.
int pack_fpn0x(kpd_plan* p, const DevConv& dc, const DevConv& lat0, const HostPack& host) {
  if (dc.cin_p != 128 || dc.cout_p != 128 || lat0.cin_p != 16 || lat0.cout_p != 128) return KPD_OK;   // path unused
  const std::vector<float>&w3 = host.at(&dc).w, &l0 = host.at(&lat0).w;
  auto W3 = [&](int co, int t, int k) { return (double)w3[((size_t)co * 9 + t) * 128 + k]; };
  // composite tap0 weights [co][t][c]
  std::vector<double> w0((size_t)128 * 9 * 16, 0.0);
  double m0 = 0.0;
  for (int co = 0; co < 128; ++co)
    for (int t = 0; t < 9; ++t)
      for (int c = 0; c < 16; ++c) {
        double acc = 0.0;
        for (int k = 0; k < 128; ++k) acc += W3(co, t, k) * (double)l0[(size_t)k * 16 + c];
        w0[((size_t)co * 9 + t) * 16 + c] = acc;
        m0 = std::max(m0, std::fabs(acc));
      }
  // per class: tap groups by lateral-1 pixel offset; the second member of a
  // class pair (kFpn0xPairFirst) shares the first member's block
  if (fpn0x_class_table(p->fpn0x.cls_ng, p->fpn0x.cls_g, p->fpn0x.cls_woff) < 0)
    return fail(KPD_ESTATE, "fpn0x: more than 4 tap groups, or a class pair with different groups");
  std::vector<double> weff;
  std::vector<size_t> src_of(16, 0);   // each class's block in weff (doubles)
  double mE = 0.0;
  int woff = 0;
  for (int cls = 0; cls < 16; ++cls) {
    const int a = cls >> 2, b = cls & 3, ng = p->fpn0x.cls_ng[cls];
    std::vector<double> blk((size_t)128 * ng * 128, 0.0);   // [co][g][k]
    for (int co = 0; co < 128; ++co)
      for (int t = 0; t < 9; ++t) {
        const int gg = (fpn0x_off(a, t / 3 - 1) + 1) * 3 + (fpn0x_off(b, t % 3 - 1) + 1);
        int g = 0;
        while (p->fpn0x.cls_g[cls][g] != gg) ++g;
        for (int k = 0; k < 128; ++k) blk[((size_t)co * ng + g) * 128 + k] += W3(co, t, k);
      }
    if (const int first = kFpn0xPairFirst[cls]; first >= 0) {
      // dropped only if bit-equal to the first member's (a changed fpn0x_off must not pass silently)
      if (p->fpn0x.cls_ng[first] != ng ||
          std::memcmp(blk.data(), weff.data() + src_of[first], blk.size() * sizeof(double)) != 0)
        return fail(KPD_ESTATE, "fpn0x: the weights of a class pair differ");
      src_of[cls] = src_of[first];
      continue;
    }
    if (p->fpn0x.cls_woff[cls] != woff) return fail(KPD_ESTATE, "fpn0x: class table offsets");
    for (double v : blk) mE = std::max(mE, std::fabs(v));
    src_of[cls] = weff.size();
    weff.insert(weff.end(), blk.begin(), blk.end());
    woff += 128 * ng * 128 * 2;   // f16 elements (hi + lo)
  }
  const int e0 = split_exp(m0), eE = split_exp(mE);
  // W0 rows [co][kt][hi16(2kt) hi16(2kt+1) lo16(2kt) lo16(2kt+1)], tap 9 = zero
  std::vector<_Float16> h0((size_t)128 * 5 * 64, (_Float16)0.f);
  for (int co = 0; co < 128; ++co)
    for (int t = 0; t < 9; ++t)
      for (int c = 0; c < 16; ++c) {
        _Float16* o = h0.data() + ((size_t)co * 5 + t / 2) * 64 + (t & 1) * 16 + c;
        split_hl(std::ldexp(w0[((size_t)co * 9 + t) * 16 + c], e0), o, o + 32);
      }
  // W_eff rows [co][g][kc][hi32 | lo32]
  std::vector<_Float16> hE((size_t)woff, (_Float16)0.f);
  for (int cls = 0; cls < 16; ++cls) {
    if (kFpn0xPairFirst[cls] >= 0) continue;   // the first member's block
    write_split_rows(weff.data() + src_of[cls], (size_t)128 * p->fpn0x.cls_ng[cls], 128, 128, eE,
                     hE.data() + p->fpn0x.cls_woff[cls]);
  }
  if (int rc = upload(p, h0, &p->fpn0x.w0)) return rc;
  if (int rc = upload(p, hE, &p->fpn0x.weff)) return rc;
  p->fpn0x.w0_bytes = (int)(h0.size() * 2);
  p->fpn0x.weff_bytes = (int)(hE.size() * 2);
  p->fpn0x.w_exp0 = e0;
  p->fpn0x.w_expE = eE;
  return KPD_OK;
}

}  // namespace

extern "C" {

int kpd_fpn0x_class_table(int* cls_ng, int* cls_g, int* cls_woff, int* blocks) {
  if (!cls_ng || !cls_g || !cls_woff || !blocks) return fail(KPD_EINVAL, "NULL output");
  const int nb = fpn0x_class_table(cls_ng, reinterpret_cast<int(*)[kFpn0xMaxGroups]>(cls_g), cls_woff);
  if (nb < 0) return fail(KPD_ESTATE, "fpn0x: inconsistent class table");
  *blocks = nb;
  return KPD_OK;
}

int kpd_plan_finalize(kpd_plan* p, int precision) {
  if (!p) return fail(KPD_EINVAL, "null plan");
  if (precision != KPD_PRECISION_FP32 && precision != KPD_PRECISION_MIXED && precision != KPD_PRECISION_SPLIT)
    return fail(KPD_EINVAL, "unknown precision");
  HIP_TRY(hipSetDevice(p->device));
  for (void* a : p->allocs) (void)hipFree(a);
  p->allocs.clear();
  p->fpn0x.w0 = p->fpn0x.weff = nullptr;
  p->stamps = nullptr;
  p->pd = DevConv();
  p->anchors = nullptr;
  p->hm1 = DevConv();
  p->hm2 = DevConv();
  p->hm3 = DevConv();
  for (auto& c : p->fpn_lv) c = DevConv();
  p->kh_ds1 = DevConv();
  p->kh_ds2 = DevConv();
  for (auto& k : p->kh_s) k = KhSplit();
  p->kh_split = false;
  p->has_kh = false;
  for (int k = 0; k <= kpd_plan::kMaxSub; ++k) {
    if (p->ws[k]) { (void)hipFree(p->ws[k]); p->ws[k] = nullptr; p->ws_bytes[k] = 0; }
    p->have_work[k] = false;
  }
  p->precision = precision;
  std::string missing;
  HostPack host;   // the packed fp32 weights, until the split packers have read them
  int rc = KPD_OK;
  auto chk =[&](int r) { if (r != KPD_OK && rc == KPD_OK) rc = r; };
  // Components present in the registered state dict (a submodule's own plan
  // -- HeatmapHead, KEYPOINT_HEAD, the backbone -- registers only its part);
  // a present component must be complete.
  auto has = [&](const char* prefix) {
    auto it = p->t.lower_bound(prefix);
    return it != p->t.end() && it->first.compare(0, strlen(prefix), prefix) == 0;
  };
  p->has_body = has("backbone.body.");
  p->has_fpn = has("backbone.fpn.");
  p->has_ca = has("channel_attention.");
  p->has_hm = has("heatmap_head.");
  const bool has_pd = has("person_detector.");
  const std::string F = "backbone.body.features.";
  // stem: [16][Cin][3][3] + BN, packed [16][Cin*9]
  if (p->has_body) {
    const HostT* w = get(p, F + "0.0.weight", missing);
    const HostT *g = get(p, F + "0.1.weight", missing), *b = get(p, F + "0.1.bias", missing);
    const HostT *m = get(p, F + "0.1.running_mean", missing), *v = get(p, F + "0.1.running_var", missing);
    if (w && g && b && m && v) {
      if (w->shape.size() != 4 || w->shape[0] != 16 || w->shape[1] != p->in_ch)
        return fail(KPD_EINVAL, "stem weight shape does not match in_channels");
      std::vector<double> sc, sh;
      bn_fold(g, b, m, v, 1e-3, 16, nullptr, sc, sh);
      std::vector<float> pw(w->data.size()), pb(16);
      const size_t per = w->data.size() / 16;
      for (int co = 0; co < 16; ++co) {
        for (size_t k = 0; k < per; ++k) pw[co * per + k] = (float)(w->data[co * per + k] * sc[co]);
        pb[co] = (float)sh[co];
      }
      chk(upload(p, pw, &p->stem_w));
      chk(upload(p, pb, &p->stem_b));
    } else {
      chk(KPD_ESTATE);
    }
  for (int i = 0; i < 11; ++i) {
    DevBneck& bn = p->bn[i];
    bn.cfg = kBneck[i];
    bn.has_exp = bn.cfg.exp != bn.cfg.cin;
    const std::string pre = F + std::to_string(i + 1) + ".block.";
    int j = 0;
    if (bn.has_exp) {
      chk(pack_conv(p, pre + "0.0.weight", "", pre + "0.1", 1e-3, 1, false, bn.expand, missing, host));
      ++j;
    }
    chk(pack_dw(p, pre + std::to_string(j), bn.cfg.k, bn.cfg.s, bn.cfg.act, bn.dw, missing));
    ++j;
    if (bn.cfg.se) {
      const std::string s = pre + std::to_string(j);
      bn.se.C = bn.cfg.exp; bn.se.Cp = pad16(bn.cfg.exp); bn.se.sq = se_squeeze(bn.cfg.exp);
      chk(pack_plain(p, s + ".fc1.weight", &bn.se.w1, missing, (size_t)bn.se.sq * bn.se.C));
      chk(pack_plain(p, s + ".fc1.bias", &bn.se.b1, missing, bn.se.sq));
      chk(pack_transposed(p, s + ".fc2.weight", bn.se.C, bn.se.sq, &bn.se.w2, missing));
      chk(pack_plain(p, s + ".fc2.bias", &bn.se.b2, missing, bn.se.C));
      ++j;
    }
    const std::string pj = pre + std::to_string(j);
    chk(pack_conv(p, pj + ".0.weight", "", pj + ".1", 1e-3, 1, false, bn.project, missing, host));
  }
  chk(pack_conv(p, F + "12.0.weight", "", F + "12.1", 1e-3, 1, false, p->last, missing, host));
  }
  if (p->has_fpn) {
  for (int i = 0; i < 4; ++i) {
    const std::string wn = "backbone.fpn.lateral_convs." + std::to_string(i) + ".weight";
    chk(pack_conv(p, wn, "", "", 0, 1, false, p->lat[i], missing, host));
    if (const HostT* lw = get(p, wn, missing)) {
      const size_t cout = (size_t)lw->shape[0], cin = lw->data.size() / std::max<size_t>(cout, 1);
      double smax = 0.0;
      for (size_t o = 0; o < cout; ++o) {
        double sum = 0.0;
        for (size_t k = 0; k < cin; ++k) sum += std::fabs((double)lw->data[o * cin + k]);
        smax = std::max(smax, sum);
      }
      float sf = (float)smax;
      if ((double)sf < smax) sf = std::nextafter(sf, INFINITY);
      p->lat_S[i] = sf;
    }
  }
  chk(pack_conv(p, "backbone.fpn.fpn_convs.0.0.weight", "", "backbone.fpn.fpn_convs.0.1", 1e-5, 3, false,
                p->fpn0, missing, host));
  if (precision != KPD_PRECISION_FP32 && rc == KPD_OK && missing.empty()) chk(pack_fpn0x(p, p->fpn0, p->lat[0], host));
  // levels 1-3 (dead in the model's forward; MobileNetV3Wrapper.forward returns them)
  for (int i = 1; i < 4; ++i) {
    const std::string c = "backbone.fpn.fpn_convs." + std::to_string(i);
    if (p->t.count(c + ".0.weight"))
      chk(pack_conv(p, c + ".0.weight", "", c + ".1", 1e-5, 3, false, p->fpn_lv[i - 1], missing, host));
  }
  }
  if (p->has_ca) {
  chk(pack_plain(p, "channel_attention.fc.0.weight", &p->ca_w0, missing, 8 * 128));
  chk(pack_plain(p, "channel_attention.fc.0.bias", &p->ca_b0, missing, 8));
  chk(pack_plain(p, "channel_attention.fc.2.weight", &p->ca_w2, missing, 128 * 8));
  chk(pack_plain(p, "channel_attention.fc.2.bias", &p->ca_b2, missing, 128));
  }
  const std::string Hh = "heatmap_head.";
  if (p->has_hm) {
  chk(pack_plain(p, Hh + "channel_attention.fc.0.weight", &p->hca_w0, missing, 4 * 64));
  chk(pack_plain(p, Hh + "channel_attention.fc.0.bias", &p->hca_b0, missing, 4));
  chk(pack_plain(p, Hh + "channel_attention.fc.2.weight", &p->hca_w2, missing, 64 * 4));
  chk(pack_plain(p, Hh + "channel_attention.fc.2.bias", &p->hca_b2, missing, 64));
  chk(pack_plain(p, Hh + "spatial_attention.conv.weight", &p->sa_w, missing, 98));
  chk(pack_plain(p, Hh + "spatial_attention.conv.bias", &p->sa_b, missing, 1));
  const bool bf = precision == KPD_PRECISION_MIXED;
  chk(pack_conv(p, Hh + "deconv_layers.0.weight", Hh + "deconv_layers.0.bias", Hh + "deconv_layers.1", 1e-5, 3,
                bf, p->hm1, missing, host));
  chk(pack_conv(p, Hh + "deconv_layers.4.weight", Hh + "deconv_layers.4.bias", Hh + "deconv_layers.5", 1e-5, 3,
                bf, p->hm2, missing, host));
  chk(pack_conv(p, Hh + "final_layer.0.weight", Hh + "final_layer.0.bias", Hh + "final_layer.1", 1e-5, 3, bf,
                p->hm3, missing, host));
  if (precision == KPD_PRECISION_SPLIT && rc == KPD_OK && missing.empty()) {
    chk(pack_split_hm(p, p->hm1, host));
    chk(pack_split_hm(p, p->hm2, host));
    chk(pack_split_hm(p, p->hm3, host));
  }
  chk(pack_plain(p, Hh + "final_layer.3.weight", &p->fin_w, missing, 17 * 64));
  chk(pack_plain(p, Hh + "final_layer.3.bias", &p->fin_b, missing, 17));
  }
  {
    std::vector<float> z(128, 0.f);
    chk(upload(p, z, &p->zero_bias));
  }
  // person-detector glue: box_heads[0] ++ cls_heads[0] -> one 1x1 conv (45 outputs)
  if (has_pd) {
    const HostT* bw = get(p, "person_detector.box_heads.0.weight", missing);
    const HostT* bb = get(p, "person_detector.box_heads.0.bias", missing);
    const HostT* cw = get(p, "person_detector.cls_heads.0.weight", missing);
    const HostT* cb = get(p, "person_detector.cls_heads.0.bias", missing);
    const HostT* an = get(p, "person_detector.anchors", missing);
    if (bw && bb && cw && cb && an) {
      if (bw->shape[0] != 36 || cw->shape[0] != 9 || an->data.size() != (size_t)56 * 56 * 9 * 4)
        return fail(KPD_EINVAL, "person head expects 9 anchors on the 56x56 grid (1 class)");
      HostT w, b;
      w.shape = {45, bw->shape[1], 1, 1};
      w.data = bw->data;
      w.data.insert(w.data.end(), cw->data.begin(), cw->data.end());
      b.shape = {45};
      b.data = bb->data;
      b.data.insert(b.data.end(), cb->data.begin(), cb->data.end());
      p->t["__pd.weight"] = std::move(w);
      p->t["__pd.bias"] = std::move(b);
      chk(pack_conv(p, "__pd.weight", "__pd.bias", "", 0, 1, false, p->pd, missing, host));
      chk(upload(p, an->data, &p->anchors));
    }
  }
  // KEYPOINT_HEAD (optional)
  p->has_kh = p->t.count("keypoint_head.spatial_attention.0.weight") > 0;
  if (p->has_kh) {
    const std::string K = "keypoint_head.", R = K + "regression_branch.", V = K + "visibility_branch.";
    chk(pack_conv(p, K + "spatial_attention.0.weight", K + "spatial_attention.0.bias", "", 0, 1, false, p->kh_sa1,
                  missing, host));
    chk(pack_plain(p, K + "spatial_attention.2.weight", &p->kh_sa2_w, missing, 64));
    chk(pack_plain(p, K + "spatial_attention.2.bias", &p->kh_sa2_b, missing, 1));
    DevConv* ds[2] = {&p->kh_ds1, &p->kh_ds2};
    DevConv* rb[2] = {&p->kh_rb1, &p->kh_rb2};
    float** bs[2] = {&p->kh_bn1a_s, &p->kh_bn1b_s};
    float** bt[2] = {&p->kh_bn1a_t, &p->kh_bn1b_t};
    std::vector<float> bn1_s[2], bn1_t[2];
    for (int i = 0; i < 2; ++i) {
      const std::string B = R + std::to_string(i) + ".";
      chk(pack_conv(p, B + "conv1.0.weight", B + "conv1.0.bias", B + "conv1.1", 1e-5, 3, false, *rb[i], missing, host));
      if (p->t.count(B + "downsample.0.weight"))
        chk(pack_conv(p, B + "downsample.0.weight", B + "downsample.0.bias", B + "downsample.1", 1e-5, 1, false,
                      *ds[i], missing, host));
      chk(pack_bn_affine(p, B + "bn1", rb[i]->cout_p ? rb[i]->cout_p : 64, bs[i], bt[i], bn1_s[i], bn1_t[i],
                         missing));
    }
    chk(pack_conv(p, R + "2.weight", R + "2.bias", R + "3", 1e-5, 3, false, p->kh_c3, missing, host));
    chk(pack_conv(p, R + "7.weight", R + "7.bias", "", 0, 1, false, p->kh_lr, missing, host));
    chk(pack_plain(p, R + "8.weight", &p->kh_lnr_g, missing, 256));
    chk(pack_plain(p, R + "8.bias", &p->kh_lnr_b, missing, 256));
    chk(pack_plain(p, R + "11.weight", &p->kh_fr_w, missing, 34 * 256));
    chk(pack_plain(p, R + "11.bias", &p->kh_fr_b, missing, 34));
    chk(pack_conv(p, V + "0.weight", V + "0.bias", V + "1", 1e-5, 3, false, p->kh_v1, missing, host));
    chk(pack_conv(p, V + "5.weight", V + "5.bias", "", 0, 1, false, p->kh_lv, missing, host));
    chk(pack_plain(p, V + "6.weight", &p->kh_lnv_g, missing, 128));
    chk(pack_plain(p, V + "6.bias", &p->kh_lnv_b, missing, 128));
    chk(pack_plain(p, V + "9.weight", &p->kh_fv_w, missing, 51 * 128));
    chk(pack_plain(p, V + "9.bias", &p->kh_fv_b, missing, 51));
    if (rc == KPD_OK && missing.empty()) {
      const int in = p->kh_lr.cin;
      int o = 1;
      while (16 * (o + 1) * (o + 1) <= in) ++o;
      if (16 * o * o != in || p->kh_c3.cout != 16 || p->kh_v1.cout != 32 || p->kh_lv.cin != 512 ||
          p->kh_sa1.cin != 128 || p->kh_sa1.cout != 64)
        return fail(KPD_EINVAL, "KEYPOINT_HEAD shape not supported (needs in 128, regression 32, square pool)");
      p->kh_o = o;
    }
    // split KEYPOINT_HEAD convs (the default channel plan: ResidualBlocks
    // 128 -> 64 -> 32 with downsamples, 3x3 32 -> 16, visibility 128 -> 32)
    const bool std_kh = p->kh_rb1.cin == 128 && p->kh_rb1.cout == 64 && p->kh_ds1.w && p->kh_rb2.cin == 64 &&
                        p->kh_rb2.cout == 32 && p->kh_ds2.w && p->kh_c3.cin == 32 && p->kh_v1.cin == 128;
    static const bool no_kh_split = kpd_diag_env("KPD_NO_KH_SPLIT") != nullptr;   // A/B switch
    if (precision != KPD_PRECISION_FP32 && rc == KPD_OK && missing.empty() && std_kh && !no_kh_split) {
      chk(pack_split_kh(p, p->kh_s[0], 128, 128, 10, {{&p->kh_rb1, &p->kh_ds1, &bn1_s[0], &bn1_t[0], 0},
                                                      {&p->kh_v1, nullptr, nullptr, nullptr, 64}}, host));
      p->kh_s[0].ns = 64; p->kh_s[0].nf = 32;
      chk(pack_split_kh(p, p->kh_s[1], 64, 64, 10, {{&p->kh_rb2, &p->kh_ds2, &bn1_s[1], &bn1_t[1], 0}}, host));
      p->kh_s[1].ns = 32; p->kh_s[1].nf = 0;
      chk(pack_split_kh(p, p->kh_s[2], 32, 64, 9, {{&p->kh_c3, nullptr, nullptr, nullptr, 0}}, host));
      p->kh_s[2].ns = 0; p->kh_s[2].nf = 16;
      if (p->kh_sa1.cin_p == 128 && p->kh_sa1.cout_p == 64) chk(pack_split_1x1(p, p->kh_sa1, host));   // kh_att2_kernel
      p->kh_split = rc == KPD_OK;
    }
  }
  if (!missing.empty()) return fail(KPD_ESTATE, "missing tensors: " + missing);
  if (rc != KPD_OK) return rc;
  // shape checks the kernels rely on
  if (p->has_fpn && (p->fpn0.cin != 128 || p->fpn0.cout != 128)) return fail(KPD_EINVAL, "fpn_convs.0 must be 128->128");
  if (p->has_hm && (p->hm1.cin != 64 || p->hm3.cout != 64 || p->hm1.cout != p->hm2.cin || p->hm2.cout != p->hm3.cin))
    return fail(KPD_EINVAL, "heatmap head channel chain mismatch");
  if (p->has_body && p->bn[0].cfg.cin != 16) return fail(KPD_EINVAL, "bad body");
  p->finalized = true;
  ++p->ws_epoch;
  return KPD_OK;
}

}  // extern "C"
