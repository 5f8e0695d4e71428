// conv_teeth — drives the conv parity checker's reference and compare functions (conv_check.hpp,
// gemm_check.hpp) with a CPU stand-in conv and seeded faults: every fault must trip the field that names
// it, and the clean stand-in must pass.  Host only.  One JSON line per run: {"run": name, c_ratio,
// c_nonfinite, rows_written, cnt_ok, cnt_sum_ok, sum_ratio, m2_ratio}.  The stand-in works as the device
// kernels do: the view in fp32 (expf / division for swish), fmaf taps in row-then-column order from zero,
// output tiles of 4 x 8 each writing one sink partial row (sum, M2 about the tile's own mean; cnt).
#include <cstdio>
#include <string>

#include "conv_check.hpp"

using namespace gck;
using cck::Geo;

enum Fault {
  CLEAN,
  PAD_OFF_ODD_S2,    // pt one short at stride 2 when the input height is odd
  HALO_COL_ZERO,     // the left halo column of the second x tile read as zero
  TAP_TRANSPOSED,    // taps w[1][3] and w[3][1] of a 5x5 kernel exchanged
  BWD_UNFLIPPED,     // the data gradient gathers with w[K-1-i][K-1-j]
  CNT_FULL_TILE,     // cnt of the last (partial) tile counts a full tile
  PART_ROW_SHIFTED,  // one tile's partial row written to p + 1
  ACC_IGNORED,       // the data gradient overwrites where it should accumulate
  FUSE_NO_EPS,       // the fuse view's denominator without its 1e-4
  VIEW_ON_PAD,       // the padding run through the view: act(be) where 0 belongs
  NO_BIAS,           // the separable conv's bias missing on the last output column
  BF_TWO_QUANTA      // one bf16-stored output two quanta off
};

constexpr int kTH = 4, kTW = 8;  // the stand-in's tile

static float act32(float z, int act) {
  if (act == 1) return z / (1.0f + std::exp(-z));
  if (act == 2) return std::fmin(std::fmax(z, 0.0f), 6.0f);
  return z;
}
static float actgrad32(float z, int act) {
  if (act == 1) {
    const float s = 1.0f / (1.0f + std::exp(-z));
    return s * (1.0f + z * (1.0f - s));
  }
  if (act == 2) return (z > 0.0f && z < 6.0f) ? 1.0f : 0.0f;
  return 1.0f;
}

struct Data {
  Geo g;
  int N = 0;                  // separable: pointwise outputs
  int view = 0, act = 0;      // 0 raw, 1 BN, 2 fuse, 3 gradient view
  int nin = 3;
  bool acc = false, bf = false, bias = false;
  std::vector<float> x[3], da, yv, prev, y2, w, bt, wp, bv;
  std::vector<float> mu[3], sc[3], be[3], rstd, mdz, mdzx, smu, ssc, sbe, srstd;
  float fw[3] = {0.7f, -0.4f, 1.1f};
};

static void params(int n, int act, uint64_t seed, std::vector<float>& mu, std::vector<float>& sc, std::vector<float>& be) {
  mu.resize(n); sc.resize(n); be.resize(n);
  fill_uni(mu, seed, 0.3f);
  fill_uni(sc, seed + 1, act == 2 ? 3.5f : 0.5f, act == 2 ? 4.5f : 1.0f);
  for (int k = 0; k < n; ++k) if (k % 3 == 1) sc[k] = -sc[k];
  fill_uni(be, seed + 2, act == 2 ? 3.0f : 0.5f, act == 2 ? 2.0f : 0.0f);
}

static Data make(int H, int W, int C, int k, int s, int view, int act, bool acc = false, bool bf = false, int N = 0) {
  Data d;
  d.g = cck::make_geo(2, H, W, C, k, s);
  d.N = N; d.view = view; d.act = act; d.acc = acc; d.bf = bf; d.bias = N > 0;
  const Geo& g = d.g;
  const int G = N ? N : C;  // channels of the gradient a backward reads
  for (int i = 0; i < 3; ++i) {
    d.x[i].resize((size_t)g.in_px() * C);
    fill_uni(d.x[i], 1 + i);
    if (bf) for (auto& v : d.x[i]) v = round_bf(v);
    params(C, act, 10 + 3 * i, d.mu[i], d.sc[i], d.be[i]);
  }
  d.da.resize((size_t)g.out_px() * G); d.yv.resize(d.da.size());
  fill_uni(d.da, 4); fill_uni(d.yv, 5);
  d.prev.resize((size_t)g.in_px() * C); d.y2.resize(d.prev.size());
  fill_uni(d.prev, 6); fill_uni(d.y2, 7);
  d.w.resize((size_t)k * k * C); fill_uni(d.w, 8);
  d.bt.resize((size_t)std::max(N, 1) * C); fill_uni(d.bt, 9);
  d.wp.resize(d.bt.size()); fill_uni(d.wp, 20);
  d.bv.resize(std::max(N, 1)); fill_uni(d.bv, 21);
  std::vector<float> gmu, gsc, gbe;
  params(G, act, 30, gmu, gsc, gbe);
  d.mu[2].swap(gmu); d.sc[2].swap(gsc); d.be[2].swap(gbe);  // slot 2 doubles as the gradient view's BN
  params(C, act, 40, d.smu, d.ssc, d.sbe);
  d.rstd.resize(G); d.mdz.resize(G); d.mdzx.resize(G); d.srstd.resize(C);
  fill_uni(d.rstd, 33, 0.5f, 1.0f); fill_uni(d.mdz, 34, 0.1f); fill_uni(d.mdzx, 35, 0.1f); fill_uni(d.srstd, 43, 0.5f, 1.0f);
  return d;
}
// (the fuse view's third input is raw, so slot 2's parameters are free for the gradient view)

// ---- the fp64 side -----------------------------------------------------------------------------
static cck::Val ref_view(const Data& d) {
  const Geo& g = d.g;
  if (d.view == 2) {
    cck::FuseRef f;
    f.nin = d.nin; f.method = 0; f.act = d.act;
    for (int i = 0; i < d.nin; ++i) {
      f.w[i] = d.fw[i];
      f.x[i].x = d.x[i].data();
      if (i < 2) { f.x[i].mu = d.mu[i].data(); f.x[i].sc = d.sc[i].data(); f.x[i].be = d.be[i].data(); }
    }
    return cck::view_fuse(f, g.in_px(), g.C);
  }
  cck::BnView b;
  b.x = d.x[0].data();
  b.act = d.act;
  if (d.view == 1) { b.mu = d.mu[0].data(); b.sc = d.sc[0].data(); b.be = d.be[0].data(); }
  return cck::view_inx(b, g.in_px(), g.C);
}
static Reference ref_fwd(const Data& d) {
  Reference r = cck::dw_fwd_ref(d.g, ref_view(d), d.w.data());
  if (d.N) r = cck::pw_fwd_ref(r, d.g.out_px(), d.g.C, d.N, d.bt.data(), d.bias ? d.bv.data() : nullptr);
  if (d.bf) cck::bf_store(r);
  return r;
}
static Reference ref_bwd(const Data& d) {
  const int G = d.N ? d.N : d.g.C;
  cck::GradRef gr;
  gr.da = d.da.data();
  gr.act = d.act;
  if (d.view == 3) {
    gr.y = d.yv.data(); gr.mu = d.mu[2].data(); gr.rstd = d.rstd.data(); gr.sc = d.sc[2].data(); gr.be = d.be[2].data();
    gr.mdz = d.mdz.data(); gr.mdzx = d.mdzx.data();
  }
  cck::Val gy = cck::view_grad(gr, d.g.out_px(), G);
  if (d.N) gy = cck::pw_bwd_ref(gy, d.g.out_px(), d.N, d.g.C, d.wp.data());
  return cck::dw_bwd_ref(d.g, gy, d.w.data(), d.acc ? d.prev.data() : nullptr);
}

// ---- the fp32 stand-in -------------------------------------------------------------------------
struct Out {
  std::vector<float> C, part, cnt;
  int P = 0;
};

static float inx32(const Data& d, int i, long e, int c, bool bn, int act) {
  const float x = d.x[i][e];
  return bn ? act32((x - d.mu[i][c]) * d.sc[i][c] + d.be[i][c], act) : x;
}
// the staged input element (b, iy, ix, c): the view inside the image, zero outside
static float staged(const Data& d, int b, int iy, int ix, int c, Fault f) {
  const Geo& g = d.g;
  if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W)
    return (f == VIEW_ON_PAD && d.view == 1) ? act32(d.be[0][c], d.act) : 0.f;
  const long e = (((long)b * g.H + iy) * g.W + ix) * g.C + c;
  if (d.view != 2) return inx32(d, 0, e, c, d.view == 1, d.act);
  float wv[3], s = 0.f;
  for (int i = 0; i < d.nin; ++i) s += (wv[i] = std::fmax(d.fw[i], 0.f));
  const float den = f == FUSE_NO_EPS ? s : s + 0.0001f;
  float v = 0.f;
  for (int i = 0; i < d.nin; ++i) v += inx32(d, i, e, c, i < 2, 0) * wv[i] / den;
  return act32(v, d.act);
}

// per-tile StatSink partials of the stored values
static void stat_tiles(const Geo& g, int rows_h, int rows_w, int N, const std::vector<float>& C, Fault f, Out& o) {
  const int tx = (rows_w + kTW - 1) / kTW, ty = (rows_h + kTH - 1) / kTH, nt = tx * ty;
  o.P = g.B * nt;
  o.part.assign((size_t)2 * N * o.P, u2f(kUnwritten));
  o.cnt.assign(o.P, u2f(kUnwritten));
  for (int b = 0; b < g.B; ++b)
    for (int t = 0; t < nt; ++t) {
      const int y0 = (t / tx) * kTH, x0 = (t % tx) * kTW;
      const int y1 = std::min(y0 + kTH, rows_h), x1 = std::min(x0 + kTW, rows_w);
      long p = (long)b * nt + t;
      const float n = (float)((y1 - y0) * (x1 - x0));
      const bool last = b == g.B - 1 && t == nt - 1;
      o.cnt[p] = (f == CNT_FULL_TILE && last) ? (float)(kTH * kTW) : n;
      if (f == PART_ROW_SHIFTED && p == 1) p = 2;
      for (int c = 0; c < N; ++c) {
        float s = 0.f, q = 0.f;
        for (int y = y0; y < y1; ++y)
          for (int x = x0; x < x1; ++x) s += C[(((long)b * rows_h + y) * rows_w + x) * N + c];
        const float mean = s / n;
        for (int y = y0; y < y1; ++y)
          for (int x = x0; x < x1; ++x) {
            const float dlt = C[(((long)b * rows_h + y) * rows_w + x) * N + c] - mean;
            q = std::fmaf(dlt, dlt, q);
          }
        o.part[2 * ((long)c * o.P + p)] = n * mean;
        o.part[2 * ((long)c * o.P + p) + 1] = q;
      }
    }
}

static Out standin_fwd(const Data& d, Fault f, bool stats) {
  const Geo& g = d.g;
  const int C = g.C, k = g.k;
  const int pt = (f == PAD_OFF_ODD_S2 && g.s == 2 && (g.H & 1)) ? g.pt - 1 : g.pt;
  std::vector<float> dw((size_t)g.out_px() * C);
  for (int b = 0; b < g.B; ++b)
    for (int oy = 0; oy < g.Ho; ++oy)
      for (int ox = 0; ox < g.Wo; ++ox)
        for (int c = 0; c < C; ++c) {
          float a = 0.f;
          for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) {
              const int iy = oy * g.s - pt + i, ix = ox * g.s - g.pl + j;
              float v = staged(d, b, iy, ix, c, f);
              // the window of x tile 1 starts at column kTW s - pl
              if (f == HALO_COL_ZERO && ox / kTW == 1 && ix == kTW * g.s - g.pl) v = 0.f;
              int ti = i, tj = j;
              if (f == TAP_TRANSPOSED && ((i == 1 && j == 3) || (i == 3 && j == 1))) std::swap(ti, tj);
              a = std::fmaf(v, d.w[(ti * k + tj) * C + c], a);
            }
          dw[((((long)b * g.Ho + oy) * g.Wo) + ox) * C + c] = a;
        }
  Out o;
  int N = C;
  if (d.N) {
    N = d.N;
    o.C.assign((size_t)g.out_px() * N, 0.f);
    for (long p = 0; p < g.out_px(); ++p)
      for (int n = 0; n < N; ++n) {
        float a = 0.f;
        for (int c = 0; c < C; ++c) a = std::fmaf(dw[p * C + c], d.bt[(long)n * C + c], a);
        if (d.bias && !(f == NO_BIAS && n == N - 1)) a += d.bv[n];
        o.C[p * N + n] = a;
      }
  } else {
    o.C = dw;
  }
  if (d.bf) {
    for (auto& v : o.C) v = round_bf(v);
    if (f == BF_TWO_QUANTA) o.C[o.C.size() / 2] = u2f(f2u(o.C[o.C.size() / 2]) + 0x20000u);
  }
  if (stats) stat_tiles(g, g.Ho, g.Wo, N, o.C, f, o);
  return o;
}

static Out standin_bwd(const Data& d, Fault f, bool gsink) {
  const Geo& g = d.g;
  const int C = g.C, k = g.k, G = d.N ? d.N : C;
  // the gradient through its view (fp32, gx_one's order)
  std::vector<float> gy((size_t)g.out_px() * G);
  for (long p = 0; p < g.out_px(); ++p)
    for (int c = 0; c < G; ++c) {
      const long e = p * G + c;
      if (d.view != 3) {
        gy[e] = d.da[e];
        continue;
      }
      const float yc = d.yv[e] - d.mu[2][c];
      float dz = d.da[e];
      if (d.act) dz *= actgrad32(yc * d.sc[2][c] + d.be[2][c], d.act);
      gy[e] = d.sc[2][c] * (dz - d.mdz[c] - (yc * d.rstd[c]) * d.mdzx[c]);
    }
  std::vector<float> dd;
  if (d.N) {  // dd = gy W^T
    dd.assign((size_t)g.out_px() * C, 0.f);
    for (long p = 0; p < g.out_px(); ++p)
      for (int c = 0; c < C; ++c) {
        float a = 0.f;
        for (int n = 0; n < G; ++n) a = std::fmaf(gy[p * G + n], d.wp[(long)c * G + n], a);
        dd[p * C + c] = a;
      }
  } else {
    dd.swap(gy);
  }
  Out o;
  o.C.assign((size_t)g.in_px() * C, 0.f);
  for (int b = 0; b < g.B; ++b)
    for (int iy = 0; iy < g.H; ++iy)
      for (int ix = 0; ix < g.W; ++ix)
        for (int c = 0; c < C; ++c) {
          float a = 0.f;
          for (int i = 0; i < k; ++i) {
            const int t = iy + g.pt - i;
            if (t < 0 || t % g.s || t / g.s >= g.Ho) continue;
            for (int j = 0; j < k; ++j) {
              const int u = ix + g.pl - j;
              if (u < 0 || u % g.s || u / g.s >= g.Wo) continue;
              // the window of x tile 1 starts at dy column (kTW + pl - (k - 1)) / s
              if (f == HALO_COL_ZERO && ix / kTW == 1 && u / g.s == (kTW + g.pl - (k - 1)) / g.s) continue;
              const int wi = f == BWD_UNFLIPPED ? (k - 1 - i) * k + (k - 1 - j) : i * k + j;
              a = std::fmaf(dd[((((long)b * g.Ho + t / g.s) * g.Wo) + u / g.s) * C + c], d.w[wi * C + c], a);
            }
          }
          const long e = ((((long)b * g.H + iy) * g.W) + ix) * C + c;
          o.C[e] = (d.acc && f != ACC_IGNORED) ? a + d.prev[e] : a;
        }
  if (gsink) {  // per-tile GradSink partials (gs_one's order)
    const int tx = (g.W + kTW - 1) / kTW, ty = (g.H + kTH - 1) / kTH, nt = tx * ty;
    o.P = g.B * nt;
    o.part.assign((size_t)2 * C * o.P, u2f(kUnwritten));
    for (int b = 0; b < g.B; ++b)
      for (int t = 0; t < nt; ++t) {
        const int y0 = (t / tx) * kTH, x0 = (t % tx) * kTW;
        long p = (long)b * nt + t;
        if (f == PART_ROW_SHIFTED && p == 1) p = 2;
        for (int c = 0; c < C; ++c) {
          float s1 = 0.f, s2 = 0.f;
          for (int y = y0; y < std::min(y0 + kTH, g.H); ++y)
            for (int x = x0; x < std::min(x0 + kTW, g.W); ++x) {
              const long e = ((((long)b * g.H + y) * g.W) + x) * C + c;
              const float yc = d.y2[e] - d.smu[c];
              float dz = o.C[e];
              if (d.act) dz *= actgrad32(yc * d.ssc[c] + d.sbe[c], d.act);
              s1 += dz;
              s2 = std::fmaf(dz, yc * d.srstd[c], s2);
            }
          o.part[2 * ((long)c * o.P + p)] = s1;
          o.part[2 * ((long)c * o.P + p) + 1] = s2;
        }
      }
  }
  return o;
}

// ---- runs --------------------------------------------------------------------------------------
static void report(const char* name, const Reference& r, const Out& o, const Data& d, int sink) {
  const CCheck c = check_c(r, o.C.data(), (long)o.C.size());
  SinkCheck s;
  if (sink == 1)
    s = check_statsink(o.C.data(), d.g.out_px(), d.N ? d.N : d.g.C, o.part.data(), o.cnt.data(), o.P);
  else if (sink == 2)
    s = check_gradsink(o.C.data(), d.g.in_px(), d.g.C, d.y2.data(), d.smu.data(), d.srstd.data(), d.ssc.data(),
                       d.sbe.data(), d.act, o.part.data(), o.P, true);
  auto num = [](double x) { return std::isfinite(x) ? x : 1e308; };
  printf("{\"run\":\"%s\",\"c_ratio\":%.6g,\"c_nonfinite\":%ld,\"rows_written\":%s,\"cnt_ok\":%s,\"cnt_sum_ok\":%s,"
         "\"sum_ratio\":%.6g,\"m2_ratio\":%.6g}\n",
         name, num(c.ratio), c.nonfinite, s.rows_written ? "true" : "false", s.cnt_ok ? "true" : "false",
         s.cnt_sum_ok ? "true" : "false", num(s.sum_ratio), num(s.m2_ratio));
}
static void fwd(const char* name, const Data& d, Fault f, bool stats) {
  report(name, ref_fwd(d), standin_fwd(d, f, stats), d, stats ? 1 : 0);
}
static void bwd(const char* name, const Data& d, Fault f, bool gsink) {
  report(name, ref_bwd(d), standin_bwd(d, f, gsink), d, gsink ? 2 : 0);
}

int main() {
  // (H, W, C, k, s, view, act, acc, bf, N)
  const Data f32o = make(15, 19, 8, 3, 2, 1, 1);          // odd input at stride 2: pt = 1
  const Data f32e = make(16, 19, 8, 3, 2, 1, 1);          // even: pt = 0
  const Data f51 = make(13, 19, 8, 5, 1, 1, 2);
  const Data f52 = make(13, 19, 8, 5, 2, 0, 0);
  const Data ffu = make(9, 11, 8, 3, 1, 2, 1);
  const Data fbf = make(9, 11, 8, 3, 1, 1, 1, false, true);
  const Data b31 = make(13, 19, 8, 3, 1, 3, 1, true);
  const Data b32 = make(15, 19, 8, 3, 2, 3, 2, true);
  const Data b52 = make(14, 19, 8, 5, 2, 3, 1);
  const Data b51 = make(9, 11, 8, 5, 1, 0, 0);
  const Data b11 = make(1, 1, 64, 3, 1, 3, 1, true);      // a 1x1 level: two rows under the GradSink
  const Data sep = make(9, 19, 8, 3, 1, 1, 1, false, false, 12);
  const Data sepb = make(9, 19, 8, 3, 1, 3, 1, true, false, 12);

  fwd("clean_fwd_k3s2_odd_stat", f32o, CLEAN, true);
  fwd("clean_fwd_k3s2_even_stat", f32e, CLEAN, true);
  fwd("clean_fwd_k5s1_relu6_stat", f51, CLEAN, true);
  fwd("clean_fwd_k5s2_raw", f52, CLEAN, false);
  fwd("clean_fwd_fuse_swish", ffu, CLEAN, false);
  fwd("clean_fwd_bf16_stat", fbf, CLEAN, true);
  bwd("clean_bwd_k3s1_gx_swish_gs_acc", b31, CLEAN, true);
  bwd("clean_bwd_k3s2_gx_relu6_gs_acc", b32, CLEAN, true);
  bwd("clean_bwd_k5s2_gx_swish", b52, CLEAN, false);
  bwd("clean_bwd_k5s1_raw_gs", b51, CLEAN, true);
  bwd("clean_bwd_1x1_gx_swish_gs_acc", b11, CLEAN, true);
  fwd("clean_sep_fwd_stat", sep, CLEAN, true);
  bwd("clean_sep_bwd_gs_acc", sepb, CLEAN, true);
  // the odd-input fault leaves an even input alone
  fwd("clean_pad_fault_even_input", f32e, PAD_OFF_ODD_S2, true);

  fwd("pad_off_odd_s2", f32o, PAD_OFF_ODD_S2, true);
  fwd("halo_col_zero", f51, HALO_COL_ZERO, true);
  fwd("tap_transposed_k5", f52, TAP_TRANSPOSED, false);
  bwd("bwd_unflipped", b52, BWD_UNFLIPPED, false);
  bwd("bwd_halo_col_zero", b31, HALO_COL_ZERO, true);
  fwd("cnt_full_tile", f51, CNT_FULL_TILE, true);
  fwd("part_row_shifted", f32o, PART_ROW_SHIFTED, true);
  bwd("part_row_shifted_gs", b31, PART_ROW_SHIFTED, true);
  bwd("acc_ignored", b31, ACC_IGNORED, true);
  fwd("fuse_no_eps", ffu, FUSE_NO_EPS, false);
  fwd("view_on_pad", f51, VIEW_ON_PAD, true);
  fwd("sep_no_bias_last_col", sep, NO_BIAS, true);
  bwd("sep_bwd_halo_col_zero", sepb, HALO_COL_ZERO, true);
  fwd("bf16_two_quanta", fbf, BF_TWO_QUANTA, true);
  printf("{\"done\":true}\n");
  return 0;
}
