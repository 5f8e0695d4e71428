// gemm_check.hpp — the host side of the GEMM kernel parity checker: the fp64 reference of
//   C[M,N] (+)= A'[M,K] * Bt[N,K]^T (+ bias)
// with the four A views of the product's 1x1-conv GEMM, the derived per-element bound, and the
// comparisons of C, the guard regions and the StatSink / GradSink partials.  Plain C++ (no HIP): the
// checker binary (gemm_parity.cpp) runs these on what the device wrote, gemm_teeth.cpp runs them on a
// CPU stand-in with seeded faults.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

namespace gck {

// ---- number formats ----------------------------------------------------------------------------
inline uint32_t f2u(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
inline float u2f(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// round to nearest even, as v_cvt_pk_bf16_f32 (finite inputs)
inline uint16_t f2bf(float f) {
  const uint32_t u = f2u(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf2f(uint16_t h) { return u2f((uint32_t)h << 16); }
inline float round_bf(float f) { return bf2f(f2bf(f)); }

constexpr double kEps24 = 1.0 / 16777216.0;  // 2^-24, the fp32 unit roundoff

// ---- threads -----------------------------------------------------------------------------------
constexpr int kMaxThreads = 16;
inline void par_rows(long rows, const std::function<void(long, long)>& fn) {
  const int nt = (int)std::max<long>(1, std::min<long>({(long)kMaxThreads, rows / 64 + 1,
                                                       (long)std::max(1u, std::thread::hardware_concurrency())}));
  if (nt == 1) return fn(0, rows);
  std::vector<std::thread> th;
  const long per = (rows + nt - 1) / nt;
  for (int t = 0; t < nt; ++t) {
    const long a = t * per, b = std::min(rows, a + per);
    if (a < b) th.emplace_back(fn, a, b);
  }
  for (auto& t : th) t.join();
}

// ---- the operation -----------------------------------------------------------------------------
// mode 0 raw, 1 BN + act view, 2 the same times the SE row scale, 3 the BN-backward gradient view.
// Every array holds the values the device reads (bf16-stored tensors already widened to float).
struct Problem {
  int M = 0, N = 0, K = 0;
  int mode = 0, act = 0;
  bool bf16 = false;  // bf16 matrix cores: A' and B rounded to bf16, fp32 accumulation
  bool cbf = false;   // C stored as bf16
  bool acc = false;
  int rpi = 1;        // rows per image of the SE scale
  const float* A = nullptr;     // [M][K] the raw operand (mode 3: da)
  const float* Y = nullptr;     // [M][K] mode 3: the BN input
  const float* Bt = nullptr;    // [N][K]
  const float* bias = nullptr;  // [N] or null
  const float* Cprev = nullptr; // [M][N] when acc
  const float* rowscale = nullptr;  // [M / rpi][K]
  const float *mu = nullptr, *sc = nullptr, *be = nullptr;        // [K] view parameters
  const float *rstd = nullptr, *mdz = nullptr, *mdzx = nullptr;   // [K] mode 3
};

inline double act_fwd(double z, int act) {
  if (act == 1) return z / (1.0 + std::exp(-z));
  if (act == 2) return std::min(std::max(z, 0.0), 6.0);
  return z;
}
inline double act_grad(double z, int act) {
  if (act == 1) {
    const double s = 1.0 / (1.0 + std::exp(-z));
    return s * (1.0 + z * (1.0 - s));
  }
  if (act == 2) return (z > 0.0 && z < 6.0) ? 1.0 : 0.0;
  return 1.0;
}
// relu6's derivative jumps at 0 and 6: an element whose fp64 z lies within fp32 rounding of a kink may
// take either side on the device.  zmag = |yc*sc| + |be|, the magnitude z was rounded at.
inline bool near_kink(double z, double zmag, int act) {
  if (act != 2) return false;
  const double tol = 8 * kEps24 * zmag;
  return std::fabs(z) <= tol || std::fabs(z - 6.0) <= tol;
}

// A'[m][k] in fp64; *jump = how far A' moves if a relu6-derivative kink falls on the other side
// (srow >= 0: the row whose image's SE scale is used — gemm_teeth's seeded fault)
inline double view_one(const Problem& p, long m, int k, double* jump, long srow = -1) {
  const long e = m * p.K + k;
  *jump = 0.0;
  const double a = p.A[e];
  if (p.mode == 0) return a;
  if (p.mode == 1 || p.mode == 2) {
    double v = act_fwd((a - (double)p.mu[k]) * (double)p.sc[k] + (double)p.be[k], p.act);
    if (p.mode == 2) v *= (double)p.rowscale[((srow >= 0 ? srow : m) / p.rpi) * p.K + k];
    return v;
  }
  // gx_one (common.hpp): sc * (da * act'(z) - mdz - xhat * mdzx)
  const double yc = (double)p.Y[e] - (double)p.mu[k];
  const double z = yc * (double)p.sc[k] + (double)p.be[k];
  const double dz = a * act_grad(z, p.act);
  if (near_kink(z, std::fabs(yc * (double)p.sc[k]) + std::fabs((double)p.be[k]), p.act))
    *jump = std::fabs((double)p.sc[k] * a);
  return (double)p.sc[k] * (dz - (double)p.mdz[k] - yc * (double)p.rstd[k] * (double)p.mdzx[k]);
}

struct Reference {
  std::vector<double> c;      // [M][N] the fp64 result
  std::vector<double> bound;  // [M][N] the per-element bound on |device - c|
};

// bound = (K + 16) 2^-24 (sum_k |a'_k b_k| + |bias| + |C_prev|)
//   K: worst-case fp32 accumulation; 16: the view's few fp32 roundings and the 1-ulp exp / rcp of swish
// bf16 compute: A' and B rounded to bf16 here, + 2^-8 sum_k |a'_k b_k| (an A' that the device's fp32
//   view puts on the other side of a bf16 rounding boundary), + 2^-9 |C| when C is stored as bf16
// (+ the full jump of any relu6-derivative kink element, see near_kink)
inline Reference reference(const Problem& p) {
  Reference r;
  const long M = p.M;
  const int N = p.N, K = p.K;
  std::vector<double> ap((size_t)M * K), aj;
  bool any_jump = false;
  if (p.mode == 3 && p.act == 2) aj.assign((size_t)M * K, 0.0);
  for (long m = 0; m < M; ++m)
    for (int k = 0; k < K; ++k) {
      double j;
      double v = view_one(p, m, k, &j);
      if (p.bf16) v = (double)round_bf((float)v);
      ap[m * K + k] = v;
      if (j != 0.0) {
        aj[m * K + k] = j;
        any_jump = true;
      }
    }
  std::vector<double> b((size_t)N * K);
  for (size_t i = 0; i < b.size(); ++i) b[i] = p.bf16 ? (double)round_bf(p.Bt[i]) : (double)p.Bt[i];
  r.c.assign((size_t)M * N, 0.0);
  r.bound.assign((size_t)M * N, 0.0);
  par_rows(M, [&](long m0, long m1) {
    for (long m = m0; m < m1; ++m) {
      const double* am = &ap[m * K];
      for (int n = 0; n < N; ++n) {
        const double* bn = &b[(size_t)n * K];
        double s = 0.0, sa = 0.0, sj = 0.0;
        for (int k = 0; k < K; ++k) {
          const double t = am[k] * bn[k];
          s += t;
          sa += std::fabs(t);
        }
        if (any_jump)
          for (int k = 0; k < K; ++k) sj += aj[m * K + k] * std::fabs(bn[k]);
        const double bv = p.bias ? (double)p.bias[n] : 0.0;
        const double cp = p.acc ? (double)p.Cprev[m * N + n] : 0.0;
        const double c = s + bv + cp;
        double bd = (K + 16) * kEps24 * (sa + std::fabs(bv) + std::fabs(cp)) + sj;
        if (p.bf16) bd += sa / 256.0;
        if (p.cbf) bd += std::fabs(c) / 512.0;
        r.c[m * N + n] = c;
        r.bound[m * N + n] = bd;
      }
    }
  });
  return r;
}

// ---- C against the reference -------------------------------------------------------------------
struct CCheck {
  double ratio = 0.0;    // max err / bound over every element (must be <= 1)
  long nonfinite = 0;    // elements of C that are not finite
  long worst = -1;       // flat index of the worst element
  double worst_err = 0.0, worst_bound = 0.0;
};
inline CCheck check_c(const Reference& r, const float* C, long MN) {
  CCheck k;
  for (long i = 0; i < MN; ++i) {
    if (!std::isfinite(C[i])) {
      ++k.nonfinite;
      continue;
    }
    const double err = std::fabs((double)C[i] - r.c[i]);
    // a zero bound (an all-zero row of products) admits only the exact value
    const double q = r.bound[i] > 0.0 ? err / r.bound[i] : (err == 0.0 ? 0.0 : INFINITY);
    if (q > k.ratio) {
      k.ratio = q;
      k.worst = i;
      k.worst_err = err;
      k.worst_bound = r.bound[i];
    }
  }
  return k;
}

// ---- guard regions -----------------------------------------------------------------------------
constexpr size_t kGuardBytes = 256;
constexpr uint8_t kGuardByte = 0xCB;
// a guarded host image: [guard | payload | guard]
inline bool guards_intact(const uint8_t* img, size_t payload) {
  for (size_t i = 0; i < kGuardBytes; ++i)
    if (img[i] != kGuardByte || img[kGuardBytes + payload + i] != kGuardByte) return false;
  return true;
}
// the sinks' "never written" word: a NaN with a payload no kernel produces
constexpr uint32_t kUnwritten = 0x7fc5a5a5u;

// ---- StatSink ----------------------------------------------------------------------------------
// part [N][P] (sum, M2 about the partial's own mean), cnt [P] rows covered.  The layout's channel pitch
// is P itself, so a row written past P lands in the next channel's rows (or the tail guard): every row
// is pre-filled with kUnwritten and must have been overwritten, and the folded totals must match.
struct SinkCheck {
  bool rows_written = true;  // every part[c][p < P] (and cnt[p]) was written
  bool cnt_ok = true;        // every cnt[p] a non-negative integer
  bool cnt_sum_ok = true;    // sum_p cnt[p] == M exactly
  double sum_ratio = 0.0;    // max over columns of |sum - ref| / bound
  double m2_ratio = 0.0;     // (GradSink: the dz*xhat sum)
  int worst_col = -1;
};

// (n, mean, M2) += (nb, mb, m2b): common.hpp's chan_merge in fp64
inline void chan_merge(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
  const double nt = n + nb;
  if (nb <= 0.0) return;
  const double f = nb / nt;
  const double d = mb - mean;
  mean += d * f;
  m2 += m2b + d * d * n * f;
  n = nt;
}

// C: what the device itself stored (so the epilogue is judged apart from the GEMM's rounding)
inline SinkCheck check_statsink(const float* C, long M, int N, const float* part2, const float* cnt, int P) {
  SinkCheck k;
  double csum = 0.0;
  for (int p = 0; p < P; ++p) {
    if (f2u(cnt[p]) == kUnwritten) {
      k.rows_written = false;
      k.cnt_ok = false;
      continue;
    }
    if (!(cnt[p] >= 0.f) || cnt[p] != std::floor(cnt[p])) k.cnt_ok = false;
    csum += cnt[p];
  }
  k.cnt_sum_ok = k.cnt_ok && csum == (double)M;
  for (int c = 0; c < N; ++c) {
    double n = 0.0, mean = 0.0, m2 = 0.0, sum = 0.0;
    bool ok = true;
    for (int p = 0; p < P; ++p) {
      const float s = part2[2 * ((long)c * P + p)], q = part2[2 * ((long)c * P + p) + 1];
      if (f2u(s) == kUnwritten || f2u(q) == kUnwritten) {
        k.rows_written = ok = false;
        continue;
      }
      const double nb = f2u(cnt[p]) == kUnwritten ? 0.0 : (double)cnt[p];
      sum += s;
      chan_merge(n, mean, m2, nb, nb > 0.0 ? (double)s / nb : 0.0, q);
    }
    double rs = 0.0, ra = 0.0;
    for (long m = 0; m < M; ++m) {
      rs += C[m * N + c];
      ra += std::fabs((double)C[m * N + c]);
    }
    const double rmean = rs / (double)M;
    double rq = 0.0;
    for (long m = 0; m < M; ++m) {
      const double d = C[m * N + c] - rmean;
      rq += d * d;
    }
    const double bs = (M + 8) * kEps24 * ra;
    const double bq = (M + 8) * kEps24 * rq + 4 * kEps24 * rmean * rmean * (double)M;
    auto ratio = [](double err, double b) { return b > 0.0 ? err / b : (err == 0.0 ? 0.0 : (double)INFINITY); };
    double r1 = ratio(std::fabs(sum - rs), bs), r2 = ratio(std::fabs(m2 - rq), bq);
    if (!ok || !std::isfinite(sum) || !std::isfinite(m2)) r1 = r2 = INFINITY;
    if (r1 > k.sum_ratio || r2 > k.m2_ratio) k.worst_col = c;
    k.sum_ratio = std::max(k.sum_ratio, r1);
    k.m2_ratio = std::max(k.m2_ratio, r2);
  }
  return k;
}

// ---- GradSink ----------------------------------------------------------------------------------
// part [N][P] (sum dz, sum dz*xhat) of the dgrad's result C through the BN whose input is y [M][N]
// (gs_one, common.hpp); bounds of the same form over |dz| and |dz*xhat| (+ relu6 kink elements)
// How far the device's act'(z) may lie from the fp64 one when its z is within ez of z.  swish' =
// s (1 + z (1 - s)): with E = (|z| + 2)(1 - s) + 3 <= |z| + 5 the relative error of s in units of 2^-24
// (v_exp of a rounded -z log2 e, the add, v_rcp), the evaluation is off by at most
// 2^-24 (E + 2)(|g| + s |z|), and |swish''| <= 0.5.  relu6' is piecewise constant (its kinks: near_kink).
inline double actgrad_err(double z, double ez, int act) {
  if (act != 1) return 0.0;
  const double s = 1.0 / (1.0 + std::exp(-z));
  const double g = s * (1.0 + z * (1.0 - s));
  return kEps24 * (std::fabs(z) + 7.0) * (std::fabs(g) + s * std::fabs(z)) + 0.5 * ez;
}

// act_err: add |da| actgrad_err (times |xhat|) per element.  That error is absolute in da, not relative
// to dz: where swish' is near its zero (z = -1.28) it exceeds any multiple of 2^-24 |dz|.  Over the GEMM
// cases' thousands of rows the (M + 8) term hides it; the conv checker's 1x1 and 2x2 members (2 and 8
// rows) need it (conv_parity, conv_teeth pass true; the GEMM checker's bounds are as they were).
inline SinkCheck check_gradsink(const float* C, long M, int N, const float* y, const float* mu, const float* rstd,
                                const float* sc, const float* be, int act, const float* part2, int P,
                                bool act_err = false) {
  SinkCheck k;
  for (int c = 0; c < N; ++c) {
    double s1 = 0.0, s2 = 0.0;
    bool ok = true;
    for (int p = 0; p < P; ++p) {
      const float a = part2[2 * ((long)c * P + p)], b = part2[2 * ((long)c * P + p) + 1];
      if (f2u(a) == kUnwritten || f2u(b) == kUnwritten) {
        k.rows_written = ok = false;
        continue;
      }
      s1 += a;
      s2 += b;
    }
    double r1 = 0.0, r2 = 0.0, a1 = 0.0, a2 = 0.0, j1 = 0.0, j2 = 0.0;
    for (long m = 0; m < M; ++m) {
      const double yc = (double)y[m * N + c] - (double)mu[c];
      const double z = yc * (double)sc[c] + (double)be[c];
      const double da = C[m * N + c];
      const double dz = da * act_grad(z, act), xh = yc * (double)rstd[c];
      r1 += dz;
      r2 += dz * xh;
      a1 += std::fabs(dz);
      a2 += std::fabs(dz * xh);
      if (near_kink(z, std::fabs(yc * (double)sc[c]) + std::fabs((double)be[c]), act)) {
        j1 += std::fabs(da);
        j2 += std::fabs(da * xh);
      }
      if (act_err) {
        const double eg = actgrad_err(z, kEps24 * (2.0 * std::fabs(yc * (double)sc[c]) + std::fabs(z)), act);
        j1 += std::fabs(da) * eg;
        j2 += std::fabs(da * xh) * eg;
      }
    }
    const double b1 = (M + 8) * kEps24 * a1 + j1, b2 = (M + 8) * kEps24 * a2 + j2;
    auto ratio = [](double err, double b) { return b > 0.0 ? err / b : (err == 0.0 ? 0.0 : (double)INFINITY); };
    double q1 = ratio(std::fabs(s1 - r1), b1), q2 = ratio(std::fabs(s2 - r2), b2);
    if (!ok || !std::isfinite(s1) || !std::isfinite(s2)) q1 = q2 = INFINITY;
    if (q1 > k.sum_ratio || q2 > k.m2_ratio) k.worst_col = c;
    k.sum_ratio = std::max(k.sum_ratio, q1);
    k.m2_ratio = std::max(k.m2_ratio, q2);
  }
  return k;
}

// ---- deterministic inputs ----------------------------------------------------------------------
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull) {}
  uint32_t next() {  // splitmix64, high word
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
  }
  float uni() { return (float)(next() >> 8) * (2.0f / 16777216.0f) - 1.0f; }  // U[-1, 1)
};
inline void fill_uni(std::vector<float>& v, uint64_t seed, float scale = 1.f, float shift = 0.f) {
  Rng r(seed);
  for (auto& x : v) x = r.uni() * scale + shift;
}

}  // namespace gck
