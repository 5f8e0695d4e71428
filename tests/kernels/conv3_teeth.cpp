// conv3_teeth — the teeth of the dense 3x3 conv parity checker's references and compare functions
// (conv3_check.hpp), without a GPU: a CPU fp32 stand-in that works the way the device does (a gathered
// column matrix times a prepared B operand, 16-row tiles; a direct stem; a sliced and folded weight
// gradient) runs clean and with one seeded fault at a time through the same fp64 references, bounds and
// comparisons conv3_parity applies to the device's output.  One JSON line per run, then a `done` line;
// tests/test_conv3_parity_host.py asserts that every clean run passes and every fault trips its own field.
// Build: make -C tests/kernels.
#include <cstdio>
#include <string>
#include <vector>

#include "conv3_check.hpp"

using c3k::pad4;

enum Fault {
  F_NONE = 0, F_DGRAD_UNFLIPPED, F_KIND2_AS_KIND0, F_TOP_PAD_ZERO, F_TCONV_ODD_TAP, F_STEM_BR_TAP, F_RAGGED_TILE,
  F_LAST_K_QUAD, F_BIAS, F_ROW_TWICE, F_DEAD_TILE, F_SINK_SENTINEL
};

static std::vector<float> uni(size_t n, uint64_t seed, float scale = 1.f) {
  std::vector<float> v(n);
  gck::fill_uni(v, seed, scale);
  return v;
}
static const float kNaN = gck::u2f(0x7fc00000u);

// ---- the stand-in: gather + B operand + a K-ordered fp32 product in 16-row tiles -----------------
static std::vector<float> st_im2col(c3k::Gather g, const float* x, int Kp, Fault f) {
  if (f == F_TOP_PAD_ZERO) g.pt = 0;
  std::vector<float> col((size_t)g.out_px() * Kp, 0.f);
  for (int b = 0; b < g.B; ++b)
    for (int oy = 0; oy < g.Ho; ++oy)
      for (int ox = 0; ox < g.Wo; ++ox)
        for (int t = 0; t < 9; ++t) {
          int iy, ix;
          bool ok;
          if (g.mode == 1 && f == F_TCONV_ODD_TAP) {  // the parity test on the row difference forgotten
            const int dy = oy - t / 3, dx = ox - t % 3;
            iy = dy >> 1;
            ix = dx >> 1;
            ok = dy >= 0 && dx >= 0 && !(dx & 1) && iy < g.H && ix < g.W;
          } else {
            ok = c3k::tap_at(g, oy, ox, t / 3, t % 3, &iy, &ix);
          }
          if (!ok) continue;
          for (int c = 0; c < g.C; ++c)
            col[((((size_t)b * g.Ho + oy) * g.Wo) + ox) * Kp + t * g.C + c] = x[(((long)b * g.H + iy) * g.W + ix) * g.C + c];
        }
  return col;
}
// un_wprep's table (kernels_unet.hip's header comment), with the flip of kind 1 optional
static std::vector<float> st_wprep(const float* w, int kind, int ci, int co, int Kp, Fault f) {
  const bool dg = kind & 1;
  const int N = dg ? ci : co, Kin = dg ? co : ci;
  std::vector<float> bt((size_t)N * Kp, 0.f);
  for (int n = 0; n < N; ++n)
    for (int t = 0; t < 9; ++t)
      for (int c = 0; c < Kin; ++c) {
        const int ky = t / 3, kx = t % 3;
        long src;
        if (kind == 0) src = ((long)t * ci + c) * co + n;
        else if (kind == 1) src = f == F_DGRAD_UNFLIPPED ? ((long)t * ci + n) * co + c : (((long)(2 - ky) * 3 + (2 - kx)) * ci + n) * co + c;
        else if (kind == 2) src = ((long)t * co + n) * ci + c;
        else src = ((long)t * co + c) * ci + n;
        bt[(size_t)n * Kp + t * Kin + c] = w[src];
      }
  return bt;
}
static std::vector<float> st_gemm(const std::vector<float>& col, long M, int Kp, int K9, const std::vector<float>& bt, int N,
                                  const float* bias, Fault f) {
  std::vector<float> out((size_t)M * N, kNaN);
  const long tiles = (M + 15) / 16;
  for (long tile = 0; tile < tiles; ++tile) {
    if (f == F_RAGGED_TILE && tile == tiles - 1 && M % 16) continue;
    for (long m = tile * 16; m < std::min(M, tile * 16 + 16); ++m)
      for (int n = 0; n < N; ++n) {
        float s = 0.f;
        const int kend = f == F_LAST_K_QUAD ? K9 - 4 : Kp;
        for (int k = 0; k < kend; ++k) s = std::fmaf(col[m * Kp + k], bt[(size_t)n * Kp + k], s);
        out[m * N + n] = s + ((bias && f != F_BIAS) ? bias[n] : 0.f);
      }
  }
  return out;
}

struct Line {
  std::string run;
  double y = 0, dx = 0, g = 0, g_if_M = 0, sum_ratio = 0, m2_ratio = 0;
  long nonfinite = 0, dead_bad = 0, bt_bad = 0;
  bool rows_written = true, cnt_ok = true, cnt_sum_ok = true;
  void print() const {
    auto n = [](double x) { return std::isfinite(x) ? x : 1e308; };
    printf("{\"run\":\"%s\",\"y\":%.6g,\"dx\":%.6g,\"g\":%.6g,\"g_if_M\":%.6g,\"nonfinite\":%ld,\"dead_bad\":%ld,\"bt_bad\":%ld,"
           "\"rows_written\":%s,\"cnt_ok\":%s,\"cnt_sum_ok\":%s,\"sum_ratio\":%.6g,\"m2_ratio\":%.6g}\n",
           run.c_str(), n(y), n(dx), n(g), n(g_if_M), nonfinite, dead_bad, bt_bad, rows_written ? "true" : "false",
           cnt_ok ? "true" : "false", cnt_sum_ok ? "true" : "false", n(sum_ratio), n(m2_ratio));
  }
};

// a conv (tconv: transposed conv) forward with its data gradient, as conv3_parity's CONV3 cases
static void run_conv(const char* name, bool tconv, int B, int H, int W, int ci, int co, bool bias, Fault f, uint64_t seed) {
  Line L;
  L.run = name;
  const c3k::Gather gf = c3k::make_gather(tconv ? 2 : 0, B, H, W, ci);
  const c3k::Gather gb = c3k::make_gather(tconv ? 1 : 0, B, gf.Ho, gf.Wo, co);
  const int Kf = pad4(9 * ci), Kb = pad4(9 * co);
  const std::vector<float> x = uni((size_t)gf.in_px() * ci, seed + 1), w = uni((size_t)9 * ci * co, seed + 2, 0.5f),
                           bv = uni(co, seed + 3), dy = uni((size_t)gf.out_px() * co, seed + 4);
  const std::vector<float> btf = st_wprep(w.data(), tconv ? 2 : 0, ci, co, Kf, f);
  const std::vector<float> btd = st_wprep(w.data(), tconv ? 3 : 1, ci, co, Kb, f);
  const std::vector<float> y = st_gemm(st_im2col(gf, x.data(), Kf, f), gf.out_px(), Kf, 9 * ci, btf, co,
                                       bias ? bv.data() : nullptr, f);
  // (the gather and GEMM faults are seeded into the forward only, the flip into the data gradient only)
  const std::vector<float> gx = st_gemm(st_im2col(gb, dy.data(), Kb, F_NONE), gb.out_px(), Kb, 9 * co, btd, ci, nullptr, F_NONE);
  c3k::Weights wt;
  wt.w = w.data(); wt.tconv = tconv; wt.ci = ci; wt.co = co;
  const gck::Reference rf = c3k::conv_fwd_ref(gf, x.data(), wt, co, bias ? bv.data() : nullptr, Kf);
  const gck::Reference rb = c3k::conv_adj_ref(gf, dy.data(), wt, co, Kb);
  const gck::CCheck cy = gck::check_c(rf, y.data(), (long)y.size()), cx = gck::check_c(rb, gx.data(), (long)gx.size());
  L.y = cy.ratio;
  L.dx = cx.ratio;
  L.nonfinite = cy.nonfinite + cx.nonfinite;
  const std::vector<float> r0 = c3k::wprep_ref(w.data(), tconv ? 2 : 0, ci, co, Kf), r1 = c3k::wprep_ref(w.data(), tconv ? 3 : 1, ci, co, Kb);
  L.bt_bad = c3k::count_diff_bits(r0.data(), btf.data(), (long)r0.size()) + c3k::count_diff_bits(r1.data(), btd.data(), (long)r1.size());
  L.print();
}

// the stem forward with its StatSink (256-row blocks), and the tiled data gradient
static void run_stem_fwd(const char* name, int B, int H, int W, int Co, Fault f, uint64_t seed) {
  Line L;
  L.run = name;
  const int Ho = H / 2, Wo = W / 2;
  const long rows = (long)B * Ho * Wo;
  const std::vector<float> x = uni((size_t)B * H * W * 3, seed + 1), w = uni((size_t)27 * Co, seed + 2, 0.3f);
  std::vector<float> y((size_t)rows * Co, kNaN);
  for (int b = 0; b < B; ++b)
    for (int oy = 0; oy < Ho; ++oy)
      for (int ox = 0; ox < Wo; ++ox)
        for (int c = 0; c < Co; ++c) {
          float s = 0.f;
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
              int iy = 2 * oy + i, ix = 2 * ox + j;
              if (f == F_STEM_BR_TAP) {  // the bottom / right pad read as the last row / column
                iy = std::min(iy, H - 1);
                ix = std::min(ix, W - 1);
              }
              if (iy >= H || ix >= W) continue;
              for (int k = 0; k < 3; ++k) s = std::fmaf(x[(((long)b * H + iy) * W + ix) * 3 + k], w[((i * 3 + j) * 3 + k) * Co + c], s);
            }
          y[((((long)b * Ho + oy) * Wo) + ox) * Co + c] = s;
        }
  const int P = (int)((rows + 255) / 256);
  std::vector<float> part((size_t)Co * P * 2, gck::u2f(gck::kUnwritten)), cnt(P, gck::u2f(gck::kUnwritten));
  for (int p = 0; p < P; ++p) {
    const long r0 = (long)p * 256, r1 = std::min(rows, r0 + 256);
    cnt[p] = (float)(r1 - r0);
    for (int c = 0; c < Co; ++c) {
      if (f == F_SINK_SENTINEL && p == P - 1 && c == Co - 1) continue;
      double s = 0, q = 0;
      for (long r = r0; r < r1; ++r) s += y[r * Co + c];
      const double m = s / (double)(r1 - r0);
      for (long r = r0; r < r1; ++r) q += (y[r * Co + c] - m) * (y[r * Co + c] - m);
      part[2 * ((size_t)c * P + p)] = (float)s;
      part[2 * ((size_t)c * P + p) + 1] = (float)q;
    }
  }
  const gck::Reference r = c3k::stem_fwd_ref(B, H, W, Co, x.data(), w.data());
  const gck::CCheck cy = gck::check_c(r, y.data(), (long)y.size());
  const gck::SinkCheck sk = gck::check_statsink(y.data(), rows, Co, part.data(), cnt.data(), P);
  L.y = cy.ratio;
  L.nonfinite = cy.nonfinite;
  L.rows_written = sk.rows_written; L.cnt_ok = sk.cnt_ok; L.cnt_sum_ok = sk.cnt_sum_ok;
  L.sum_ratio = sk.sum_ratio; L.m2_ratio = sk.m2_ratio;
  L.print();
}

static void run_stem_gx(const char* name, int B, int H, int W, int Co, Fault f, uint64_t seed) {
  Line L;
  L.run = name;
  const int Ho = H / 2, Wo = W / 2;
  const std::vector<float> dy = uni((size_t)B * Ho * Wo * Co, seed + 1), w = uni((size_t)27 * Co, seed + 2, 0.3f);
  std::vector<int16_t> owner((size_t)B * H * W * 3, -1);
  owner[((size_t)(B - 1) * H * W + (size_t)(H - 1) * W + (W - 1)) * 3 + 2] = 1;  // the corner tile of the last image
  const c3k::TileMap t = c3k::stem_tiles(B, H, W, owner.data());
  std::vector<float> dx((size_t)B * H * W * 3, kNaN);
  for (int b = 0; b < B; ++b)
    for (int iy = 0; iy < H; ++iy)
      for (int ix = 0; ix < W; ++ix)
        for (int k = 0; k < 3; ++k) {
          float s = 0.f;
          if (t.at(b, iy, ix))
            for (int i = 0; i < 3; ++i)
              for (int j = 0; j < 3; ++j) {
                if ((iy - i) < 0 || (ix - j) < 0 || (iy - i) % 2 || (ix - j) % 2) continue;
                const int oy = (iy - i) / 2, ox = (ix - j) / 2;
                if (oy >= Ho || ox >= Wo) continue;
                for (int c = 0; c < Co; ++c)
                  s = std::fmaf(dy[((((long)b * Ho + oy) * Wo) + ox) * Co + c], w[((i * 3 + j) * 3 + k) * Co + c], s);
              }
          dx[(((long)b * H + iy) * W + ix) * 3 + k] = s;
        }
  if (f == F_DEAD_TILE) dx[(5 * W + 7) * 3 + 1] = 1e-30f;  // image 0, tile (0, 0): dead
  cck::Val g;
  g.v.assign(dy.begin(), dy.end());
  g.e.assign(dy.size(), 0.0);
  gck::Reference r = c3k::stem_bwd_ref(B, H, W, Co, g, w.data(), nullptr);
  const c3k::TileCheck tc = c3k::apply_tiles(B, H, W, t, r, dx.data());
  const gck::CCheck cx = gck::check_c(r, dx.data(), (long)dx.size());
  L.dx = cx.ratio;
  L.nonfinite = cx.nonfinite;
  L.dead_bad = tc.dead_bad;
  L.print();
}

// the weight gradient: 64-row slices of fp32 sums, folded in order, scattered to the Keras layout
static void run_wgrad(const char* name, int src, int B, int H, int W, int C, int Co, Fault f, uint64_t seed) {
  Line L;
  L.run = name;
  c3k::WgradGeo q;
  q.src = src; q.B = B; q.H = H; q.W = W; q.C = C; q.M = (long)B * H * W; q.Co = Co; q.Kin = C; q.taps = 9;
  q.kind = src == 1 ? 0 : 2; q.ldy = Co;
  const c3k::Gather g = src == 1 ? c3k::make_gather(0, B, H, W, C) : c3k::make_gather(2, B, H / 2, W / 2, C);
  const std::vector<float> dy = uni((size_t)q.M * Co, seed + 1), x = uni((size_t)g.in_px() * C, seed + 2);
  const int K = 9 * C;
  const std::vector<float> col = c3k::im2col_ref(g, x.data(), K);
  const long rps = 64;
  const int ns = (int)((q.M + rps - 1) / rps);
  std::vector<float> out((size_t)q.g_elems(), kNaN);
  for (int co = 0; co < Co; ++co)
    for (int k = 0; k < K; ++k) {
      float tot = 0.f;
      for (int z = 0; z < ns; ++z) {
        float s = 0.f;
        for (long m = z * rps; m < std::min(q.M, (z + 1) * rps); ++m) {
          s = std::fmaf(dy[m * Co + co], col[m * K + k], s);
          if (f == F_ROW_TWICE && m == q.M / 2) s = std::fmaf(dy[m * Co + co], col[m * K + k], s);
        }
        tot += s;
      }
      const int tap = k / C, c = k % C;
      const bool lay2 = q.kind == 2 && f != F_KIND2_AS_KIND0;
      out[lay2 ? ((size_t)tap * Co + co) * C + c : ((size_t)tap * C + c) * Co + co] = tot;
    }
  const int depth = c3k::wgrad_depth(rps, ns);
  const gck::Reference r = c3k::wgrad_ref(q, dy.data(), x.data(), depth);
  const gck::CCheck cg = gck::check_c(r, out.data(), (long)out.size());
  L.g = cg.ratio;
  L.g_if_M = cg.ratio * (depth + 16) / (double)(q.M + 16);  // what a bound with M for the constant would report
  L.nonfinite = cg.nonfinite;
  L.print();
}

int main() {
  run_conv("clean_conv_c8_n17_bias", false, 3, 15, 15, 8, 17, true, F_NONE, 11);
  run_conv("clean_conv_c3_n3", false, 1, 6, 8, 3, 3, false, F_NONE, 12);
  run_conv("clean_tconv_c6_n16_bias", true, 1, 10, 13, 6, 16, true, F_NONE, 13);
  run_stem_fwd("clean_stem_fwd_c40", 2, 34, 30, 40, F_NONE, 14);
  run_stem_fwd("clean_stem_fwd_c32_one_lane_block", 1, 2, 514, 32, F_NONE, 15);
  run_stem_gx("clean_stem_gx_c32", 2, 34, 34, 32, F_NONE, 16);
  run_wgrad("clean_wgrad_src1_m4608", 1, 2, 48, 48, 8, 16, F_NONE, 17);
  run_wgrad("clean_wgrad_src2_c6_co5", 2, 2, 22, 24, 6, 5, F_NONE, 18);
  run_conv("dgrad_unflipped", false, 3, 15, 15, 8, 17, true, F_DGRAD_UNFLIPPED, 11);
  run_wgrad("kind2_as_kind0", 2, 2, 22, 24, 6, 5, F_KIND2_AS_KIND0, 18);
  run_conv("top_pad_zero", false, 3, 15, 15, 8, 17, true, F_TOP_PAD_ZERO, 11);
  run_conv("tconv_odd_tap", true, 1, 10, 13, 6, 16, true, F_TCONV_ODD_TAP, 13);
  run_stem_fwd("stem_bottom_right_tap", 2, 34, 30, 40, F_STEM_BR_TAP, 14);
  run_conv("ragged_tile_dropped", false, 3, 15, 15, 8, 17, true, F_RAGGED_TILE, 11);
  run_conv("last_k_quad_dropped", false, 3, 15, 15, 8, 17, true, F_LAST_K_QUAD, 11);
  run_conv("bias_dropped", false, 3, 15, 15, 8, 17, true, F_BIAS, 11);
  run_wgrad("row_twice_m4608", 1, 2, 48, 48, 8, 16, F_ROW_TWICE, 17);
  run_stem_gx("dead_tile_nonzero", 2, 34, 34, 32, F_DEAD_TILE, 16);
  run_stem_fwd("sink_row_sentinel", 2, 34, 30, 40, F_SINK_SENTINEL, 14);
  printf("{\"done\":true}\n");
  return 0;
}
