// gemm_teeth — drives the parity checker's compare functions (gemm_check.hpp) with a CPU stand-in GEMM
// and seeded faults: every fault must trip the field that names it, and the clean stand-in must pass.
// Host only.  One JSON line per run: {"run": name, c_ratio, rows_written, cnt_ok, cnt_sum_ok, sum_ratio,
// m2_ratio}.  The stand-in works as the device kernels do: fp32 view, fp32 accumulation in k order,
// 32-row tiles each writing one sink partial row.
#include <cstdio>
#include <string>

#include "gemm_check.hpp"

using namespace gck;

enum Fault {
  CLEAN,
  DROP_LAST_QUAD,     // the last K quad never multiplied
  CLAMPED_ROW,        // the rows past M of the last tile enter its statistics as copies of row M - 1
  NO_BIAS_LAST_NTILE, // the bias missing on the last 32-column tile
  SE_NEXT_IMAGE,      // the first row of image 1 scaled with image 0's SE scale
  CNT_FULL_TILE,      // cnt of the last partial counts a full tile
  PART_ROW_SHIFTED,   // one partial row written to p + 1
  SLICE_TWICE,        // one split-K slice added twice
  BF16_QUANTUM        // one bf16 C element off by one quantum
};

struct Data {
  int M, N, K;
  std::vector<float> A, Y, Bt, bias, Cprev, rs, mu, sc, be, rstd, mdz, mdzx, Y2, mu2, sc2, be2, rstd2;
  Problem p;
};

static void make(Data& d, int M, int N, int K, int mode, int act, bool bf16, bool acc, int rpi, bool positive) {
  d.M = M; d.N = N; d.K = K;
  d.A.resize((size_t)M * K); d.Y.resize((size_t)M * K); d.Bt.resize((size_t)N * K); d.bias.resize(N);
  d.Cprev.resize((size_t)M * N); d.rs.resize((size_t)((M + rpi - 1) / rpi) * K);
  for (auto* v : {&d.mu, &d.sc, &d.be, &d.rstd, &d.mdz, &d.mdzx}) v->resize(K);
  for (auto* v : {&d.mu2, &d.sc2, &d.be2, &d.rstd2}) v->resize(N);
  d.Y2.resize((size_t)M * N);
  fill_uni(d.A, 1); fill_uni(d.Y, 2); fill_uni(d.Bt, 3); fill_uni(d.bias, 4); fill_uni(d.Cprev, 5);
  fill_uni(d.rs, 6, 0.45f, 0.55f);
  fill_uni(d.mu, 7, 0.3f); fill_uni(d.sc, 8, 0.5f, 1.0f); fill_uni(d.be, 9, 0.5f);
  for (int k = 0; k < K; ++k) if (k % 3 == 1) d.sc[k] = -d.sc[k];
  fill_uni(d.rstd, 10, 0.5f, 1.0f); fill_uni(d.mdz, 11, 0.1f); fill_uni(d.mdzx, 12, 0.1f);
  fill_uni(d.Y2, 13); fill_uni(d.mu2, 14, 0.3f); fill_uni(d.sc2, 15, 0.5f, 1.0f); fill_uni(d.be2, 16, 0.5f);
  fill_uni(d.rstd2, 17, 0.5f, 1.0f);
  if (positive) {
    for (auto& x : d.A) x = 0.5f + 0.5f * std::fabs(x);
    for (auto& x : d.Bt) x = 0.5f + 0.5f * std::fabs(x);
  }
  if (bf16 && mode != 3) {  // forward on bf16 activations
    for (auto& x : d.A) x = round_bf(x);
    for (auto& x : d.Cprev) x = round_bf(x);
  }
  Problem& p = d.p;
  p.M = M; p.N = N; p.K = K; p.mode = mode; p.act = act; p.bf16 = bf16; p.cbf = bf16 && mode != 3; p.acc = acc;
  p.rpi = rpi; p.A = d.A.data(); p.Y = d.Y.data(); p.Bt = d.Bt.data(); p.bias = positive ? nullptr : d.bias.data();
  p.Cprev = d.Cprev.data(); p.rowscale = d.rs.data(); p.mu = d.mu.data(); p.sc = d.sc.data(); p.be = d.be.data();
  p.rstd = d.rstd.data(); p.mdz = d.mdz.data(); p.mdzx = d.mdzx.data();
}

struct Out {
  std::vector<float> C, part, cnt;  // part [N][P] float2
  int P;
};

// sink: 0 none, 1 StatSink, 2 GradSink
static Out standin(const Data& d, int sink, Fault f) {
  const Problem& p = d.p;
  const int M = p.M, N = p.N, K = p.K;
  Out o;
  o.C.assign((size_t)M * N, 0.f);
  const int kuse = f == DROP_LAST_QUAD ? K - 4 : K;
  const int khalf = (K / 2 + 3) / 4 * 4;  // the two split-K slices of SLICE_TWICE
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      float s = 0.f, s0 = 0.f;
      for (int k = 0; k < kuse; ++k) {
        double j;
        const long srow = (f == SE_NEXT_IMAGE && m == p.rpi) ? m - 1 : -1;
        float a = (float)view_one(p, m, k, &j, srow);
        float b = p.Bt[(size_t)n * K + k];
        if (p.bf16) {
          a = round_bf(a);
          b = round_bf(b);
        }
        s = std::fmaf(a, b, s);
        if (k == khalf - 1) s0 = s;
      }
      if (f == SLICE_TWICE) s += s0;
      const bool last_ntile = n >= (N - 1) / 32 * 32;
      if (p.bias && !(f == NO_BIAS_LAST_NTILE && last_ntile)) s += p.bias[n];
      if (p.acc) s += p.Cprev[(size_t)m * N + n];
      o.C[(size_t)m * N + n] = p.cbf ? round_bf(s) : s;
    }
  if (f == BF16_QUANTUM) {
    // the element whose value sits lowest in its binade (a quantum is largest against it), moved one
    // quantum away from the exact value
    const Reference r = reference(p);
    size_t best = 0;
    double bm = 2.0;
    for (size_t i = 0; i < o.C.size(); ++i) {
      int e;
      const double fr = 2.0 * std::frexp(std::fabs((double)o.C[i]), &e);
      if (fr < bm) {
        bm = fr;
        best = i;
      }
    }
    uint16_t h = f2bf(o.C[best]);
    const bool up = (double)o.C[best] >= r.c[best];
    h = (uint16_t)(h + ((up == (o.C[best] > 0.f)) ? 1 : -1));
    o.C[best] = bf2f(h);
  }
  o.P = (M + 31) / 32;
  if (!sink) return o;
  const int P = o.P;
  o.part.assign((size_t)N * P * 2, u2f(kUnwritten));
  o.cnt.assign(P, u2f(kUnwritten));
  for (int t = 0; t < P; ++t) {
    const int r0 = 32 * t, rows = std::min(32, M - r0);
    const int span = (f == CLAMPED_ROW && t == P - 1) ? 32 : rows;
    for (int n = 0; n < N; ++n) {
      float a = 0.f, b = 0.f;
      if (sink == 1) {
        for (int r = 0; r < span; ++r) a += o.C[(size_t)std::min(r0 + r, M - 1) * N + n];
        const float mean = a / (float)rows;
        for (int r = 0; r < span; ++r) {
          const float dv = o.C[(size_t)std::min(r0 + r, M - 1) * N + n] - mean;
          b = std::fmaf(dv, dv, b);
        }
      } else {
        for (int r = 0; r < span; ++r) {
          const size_t e = (size_t)std::min(r0 + r, M - 1) * N + n;
          const float yc = d.Y2[e] - d.mu2[n];
          const float dz = o.C[e] * (float)act_grad((double)(yc * d.sc2[n] + d.be2[n]), p.act);
          a += dz;
          b = std::fmaf(dz, yc * d.rstd2[n], b);
        }
      }
      // (the shifted row's own tile overwrites it afterwards: row t of this column stays unwritten)
      int row = t;
      if (f == PART_ROW_SHIFTED && n == N / 2 && t == P / 2) row = t + 1;
      o.part[2 * ((size_t)n * P + row)] = a;
      o.part[2 * ((size_t)n * P + row) + 1] = b;
    }
    o.cnt[t] = (float)((f == CNT_FULL_TILE && t == P - 1) ? 32 : rows);
  }
  return o;
}

static void report(const char* name, const Data& d, int sink, const Out& o) {
  const Reference r = reference(d.p);
  const CCheck c = check_c(r, o.C.data(), (long)d.M * d.N);
  SinkCheck s;
  if (sink == 1) s = check_statsink(o.C.data(), d.M, d.N, o.part.data(), o.cnt.data(), o.P);
  if (sink == 2)
    s = check_gradsink(o.C.data(), d.M, d.N, d.Y2.data(), d.mu2.data(), d.rstd2.data(), d.sc2.data(), d.be2.data(),
                       d.p.act, o.part.data(), o.P);
  auto num = [](double x) { return std::isfinite(x) ? x : 1e308; };
  printf("{\"run\":\"%s\",\"c_ratio\":%.6g,\"c_nonfinite\":%ld,\"rows_written\":%s,\"cnt_ok\":%s,\"cnt_sum_ok\":%s,"
         "\"sum_ratio\":%.6g,\"m2_ratio\":%.6g}\n",
         name, num(c.ratio), c.nonfinite, s.rows_written ? "true" : "false", s.cnt_ok ? "true" : "false",
         s.cnt_sum_ok ? "true" : "false", num(s.sum_ratio), num(s.m2_ratio));
  fflush(stdout);
}

int main() {
  // ragged everywhere: 100 rows (last 32-row tile holds 4), 40 columns (last tile 8), K = 36, images of 30 rows
  Data se;
  make(se, 100, 40, 36, 2, 1, false, false, 30, false);
  report("clean_se_stat", se, 1, standin(se, 1, CLEAN));
  report("drop_last_quad", se, 1, standin(se, 1, DROP_LAST_QUAD));
  report("clamped_row", se, 1, standin(se, 1, CLAMPED_ROW));
  report("no_bias_last_ntile", se, 1, standin(se, 1, NO_BIAS_LAST_NTILE));
  report("se_next_image", se, 1, standin(se, 1, SE_NEXT_IMAGE));
  report("cnt_full_tile", se, 1, standin(se, 1, CNT_FULL_TILE));
  report("part_row_shifted", se, 1, standin(se, 1, PART_ROW_SHIFTED));
  report("slice_twice", se, 1, standin(se, 1, SLICE_TWICE));
  Data acc;
  make(acc, 100, 40, 36, 1, 2, false, true, 1, false);
  report("clean_bn_relu6_acc", acc, 0, standin(acc, 0, CLEAN));
  Data g;
  make(g, 100, 40, 36, 3, 1, false, false, 1, false);
  report("clean_dgrad_gs", g, 2, standin(g, 2, CLEAN));
  report("clamped_row_gs", g, 2, standin(g, 2, CLAMPED_ROW));
  report("part_row_shifted_gs", g, 2, standin(g, 2, PART_ROW_SHIFTED));
  Data g6;
  make(g6, 100, 40, 36, 3, 2, false, true, 1, false);
  report("clean_dgrad_relu6_gs", g6, 2, standin(g6, 2, CLEAN));
  // bf16: every product positive, so sum |a b| = |C| and one quantum stands clear of the bound
  Data bf;
  make(bf, 100, 40, 36, 0, 0, true, false, 1, true);
  report("clean_bf16", bf, 1, standin(bf, 1, CLEAN));
  report("bf16_quantum", bf, 1, standin(bf, 1, BF16_QUANTUM));
  Data bfv;
  make(bfv, 100, 40, 36, 1, 1, true, true, 1, false);
  report("clean_bf16_bn_swish_acc", bfv, 0, standin(bfv, 0, CLEAN));
  printf("{\"done\":true}\n");
  return 0;
}
