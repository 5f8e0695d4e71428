// norm_check.hpp — the host side of the BN / squeeze-excite / elementwise / resampling parity checker
// (kernels_norm.hip): the fp64 reference of every operation with the per-element bound derived from the
// kernel's arithmetic ("Norm kernel parity"), and exact replays where the operation only moves
// or selects values.  Plain C++ (no HIP).  norm_parity.cpp runs these on what the device wrote,
// norm_teeth.cpp on a CPU stand-in with seeded faults.  The views, the activation error terms, the
// guard regions and the GradSink comparison are conv_check.hpp's and gemm_check.hpp's.
#pragma once
#include "conv_check.hpp"

namespace nck {

using gck::kEps24;
constexpr double kEps53 = 1.0 / 9007199254740992.0;  // 2^-53, the fp64 unit roundoff

inline double ratio(double err, double b) { return b > 0.0 ? err / b : (err == 0.0 ? 0.0 : (double)INFINITY); }
// a value known to within err, stored as float: |fl(a) - v| <= |a - v| + 2^-24 |a|
inline double fstore(double v, double err) { return err + kEps24 * (std::fabs(v) + err); }

// one output array against its reference, any element type
struct Field {
  double ratio = 0.0;
  long nonfinite = 0, worst = -1;
  void add(double got, double ref, double bound, long i) {
    if (!std::isfinite(got)) {
      ++nonfinite;
      return;
    }
    const double q = nck::ratio(std::fabs(got - ref), bound);
    if (q > ratio || worst < 0) {
      ratio = std::max(ratio, q);
      worst = i;
    }
  }
  void merge(const Field& f) {
    ratio = std::max(ratio, f.ratio);
    nonfinite += f.nonfinite;
  }
};
template <class T>
inline Field check_arr(const gck::Reference& r, const T* got) {
  Field f;
  for (size_t i = 0; i < r.c.size(); ++i) f.add((double)got[i], r.c[i], r.bound[i], (long)i);
  return f;
}

// ---- column reductions -------------------------------------------------------------------------
// k_colred_part adds a lane's rows in fp32 runs of at most 64 and folds the runs, the lanes and the
// chunks in fp64: a sum of terms t_i (each known to e_i) is off by at most
//   sum e_i + 64 2^-24 sum |t_i|        (63 roundings of partial sums no larger than sum |t|, one spare)
// plus the fp64 folds' 2^-53 per addition (kFold of them at the very most).
constexpr double kRun = 64.0;
constexpr double kFold = 4096.0;

// BN statistics about the shift r = y[0][c]: s0 = sum d, s1 = sum d^2, d = fl(y - r) (one rounding:
// 2^-24 |d|; its square carries two more and the product's own: 3 2^-24 d^2)
struct Sums {
  double s0 = 0, s1 = 0, e0 = 0, e1 = 0, ref = 0;
};
inline Sums shifted_sums(const float* y, long M, int C, int c) {
  Sums s;
  s.ref = y[c];
  long double a0 = 0, a1 = 0, b0 = 0;
  for (long m = 0; m < M; ++m) {
    const long double d = (long double)y[m * C + c] - (long double)s.ref;
    a0 += d;
    a1 += d * d;
    b0 += std::fabs((double)d);
  }
  s.s0 = (double)a0;
  s.s1 = (double)a1;
  s.e0 = (kRun + 1.0) * kEps24 * (double)b0 + kFold * kEps53 * (double)b0;
  s.e1 = (kRun + 3.0) * kEps24 * (double)a1 + kFold * kEps53 * (double)a1;
  return s;
}

// StatsEpi (common.hpp) in fp64 with the sums' errors carried through:
//   dm = s0 / M, var = max(s1 / M - dm^2, 0), mu = ref + dm, rs = (var + eps)^-1/2, sc = rs gamma,
//   uvar = var M / (M - 1), moving <- fl(m - (m - batch) 0.01)
struct StatVals {
  double mu, rs, sc, uvar, mm, mv;            // values
  double e_mu, e_rs, e_sc, e_uvar;            // how far the device's fp64 values may lie from them
};
inline StatVals stats_from(const Sums& s, long M, double gamma, double eps, double mm0, double mv0) {
  StatVals v;
  const double dm = s.s0 / (double)M, e_dm = s.e0 / (double)M;
  double var = s.s1 / (double)M - dm * dm;
  const double e_var = s.e1 / (double)M + 2.0 * std::fabs(dm) * e_dm + e_dm * e_dm +
                       8.0 * kEps53 * (s.s1 / (double)M + dm * dm);
  if (var < 0.0) var = 0.0;
  v.mu = s.ref + dm;
  v.e_mu = e_dm + 2.0 * kEps53 * (std::fabs(s.ref) + std::fabs(dm));
  v.rs = 1.0 / std::sqrt(var + eps);
  // |d rs / d var| = rs / (2 (var + eps)), largest at the low end of the interval
  v.e_rs = 0.5 * e_var * std::pow(std::max(var - e_var, 0.0) + eps, -1.5) + 4.0 * kEps53 * v.rs;
  v.sc = v.rs * gamma;
  v.e_sc = std::fabs(gamma) * v.e_rs + 2.0 * kEps53 * std::fabs(v.sc);
  const double bes = M > 1 ? (double)M / (double)(M - 1) : 1.0;
  v.uvar = var * bes;
  v.e_uvar = e_var * bes + 2.0 * kEps53 * v.uvar;
  v.mm = mm0 - (mm0 - v.mu) * 0.01;
  v.mv = mv0 - (mv0 - v.uvar) * 0.01;
  return v;
}

// what a statistics launch writes, per channel
struct StatOut {
  const float *mean = nullptr, *rstd = nullptr, *sc = nullptr, *mmean = nullptr, *mvar = nullptr;
  const double* side = nullptr;
};
struct StatCheck {
  Field mean, rstd, sc, moving, side;
};
inline void check_stat_chan(const StatVals& v, const StatOut& o, int c, StatCheck& k) {
  k.mean.add(o.mean[c], v.mu, fstore(v.mu, v.e_mu), c);
  k.rstd.add(o.rstd[c], v.rs, fstore(v.rs, v.e_rs), c);
  k.sc.add(o.sc[c], v.sc, fstore(v.sc, v.e_sc), c);
  if (o.side) {
    k.side.add(o.side[2 * c], v.mu, v.e_mu, c);
    k.side.add(o.side[2 * c + 1], v.uvar, v.e_uvar, c);
  }
  if (o.mmean) {
    k.moving.add(o.mmean[c], v.mm, fstore(v.mm, 0.01 * v.e_mu + 4.0 * kEps53 * std::fabs(v.mm)), c);
    k.moving.add(o.mvar[c], v.mv, fstore(v.mv, 0.01 * v.e_uvar + 4.0 * kEps53 * std::fabs(v.mv)), c);
  }
}
// launch_bn_stats over y [M][C] (bf16 storage: already widened)
inline StatCheck check_stats(const float* y, long M, int C, const float* gamma, float eps, const float* mm0,
                             const float* mv0, const StatOut& o) {
  StatCheck k;
  for (int c = 0; c < C; ++c)
    check_stat_chan(stats_from(shifted_sums(y, M, C, c), M, gamma[c], (double)eps, mm0 ? mm0[c] : 0.0,
                               mv0 ? mv0[c] : 0.0),
                    o, c, k);
  return k;
}
// launch_bn_stats_sums: sums[c] = (rows, sum y, sum y^2), the shifted sums un-shifted in fp64:
//   S0 = s0 + M r, S1 = s1 + 2 r s0 + M r^2   ->   e(S0) = e0, e(S1) = e1 + 2 |r| e0  (+ fp64 roundings)
// The reference sums y and y^2 directly.
inline Field check_stats_sums(const float* y, long M, int C, const double* sums) {
  Field f;
  for (int c = 0; c < C; ++c) {
    const Sums s = shifted_sums(y, M, C, c);
    long double S0 = 0, S1 = 0;
    for (long m = 0; m < M; ++m) {
      S0 += (long double)y[m * C + c];
      S1 += (long double)y[m * C + c] * (long double)y[m * C + c];
    }
    const double r = s.ref;
    const double mag = std::fabs(s.s1) + 2.0 * std::fabs(r * s.s0) + (double)M * r * r;
    f.add(sums[3 * c], (double)M, 0.0, c);
    f.add(sums[3 * c + 1], (double)S0, s.e0 + 8.0 * kEps53 * (std::fabs(s.s0) + (double)M * std::fabs(r)), c);
    f.add(sums[3 * c + 2], (double)S1, s.e1 + 2.0 * std::fabs(r) * s.e0 + 8.0 * kEps53 * mag, c);
  }
  return f;
}

// BwdAcc: xh = (y - mu) rs (two roundings), z = xh gamma + beta (two more), dz = da act'(z),
// sums of dz and dz xh.  |z_dev - z| <= 2^-24 (3 |t| + |z|), t = xh gamma.
struct BwdSums {
  double s1 = 0, s2 = 0, e1 = 0, e2 = 0;
  long kinks = 0;
};
struct BnPar {
  const float *mean, *rstd, *gamma, *beta;
  int act;
};
inline void bwd_elem(double da, double y, const BnPar& p, int c, double* dz, double* e_dz, double* xh, bool* kink) {
  *xh = (y - (double)p.mean[c]) * (double)p.rstd[c];
  const double t = *xh * (double)p.gamma[c], z = t + (double)p.beta[c];
  const double ez = kEps24 * (3.0 * std::fabs(t) + std::fabs(z));
  const double g = gck::act_grad(z, p.act);
  *dz = da * g;
  *e_dz = p.act ? std::fabs(da) * gck::actgrad_err(z, ez, p.act) + kEps24 * std::fabs(*dz) : 0.0;
  *kink = gck::near_kink(z, std::fabs(t) + std::fabs((double)p.beta[c]), p.act);
}
inline BwdSums bwd_sums(const float* da, const float* y, long M, int C, int c, const BnPar& p) {
  BwdSums s;
  double a1 = 0, a2 = 0;
  for (long m = 0; m < M; ++m) {
    double dz, e_dz, xh;
    bool kink;
    bwd_elem(da[m * C + c], y[m * C + c], p, c, &dz, &e_dz, &xh, &kink);
    s.s1 += dz;
    s.s2 += dz * xh;
    a1 += std::fabs(dz);
    a2 += std::fabs(dz * xh);
    s.e1 += e_dz;
    s.e2 += std::fabs(xh) * e_dz + 3.0 * kEps24 * std::fabs(dz * xh);
    if (kink) {  // the derivative may take either side: the whole element
      s.e1 += std::fabs((double)da[m * C + c]);
      s.e2 += std::fabs((double)da[m * C + c] * xh);
      ++s.kinks;
    }
  }
  s.e1 += (kRun + kFold * kEps53 / kEps24) * kEps24 * a1;
  s.e2 += (kRun + kFold * kEps53 / kEps24) * kEps24 * a2;
  return s;
}

// k_bn_bwd_apply with the coefficients the device stored: o = c0 (dz - c1 - xh c2) (+ prev); frozen:
// o = (gamma rstd) dz.  Roundings in order: dz, the first difference, xh c2 (xh carries two), the
// second difference, the product; the accumulation one more.
inline gck::Reference bwd_apply_ref(const float* da, const float* y, long M, int C, const BnPar& p, const float* coef,
                                    bool frozen, const float* prev, long* kinks) {
  gck::Reference r;
  r.c.resize((size_t)M * C);
  r.bound.resize((size_t)M * C);
  for (long m = 0; m < M; ++m)
    for (int c = 0; c < C; ++c) {
      const long e = m * C + c;
      double dz, e_dz, xh, o, b;
      bool kink;
      bwd_elem(da[e], y[e], p, c, &dz, &e_dz, &xh, &kink);
      double c0;
      if (frozen) {
        c0 = (double)p.gamma[c] * (double)p.rstd[c];
        o = c0 * dz;
        b = std::fabs(c0) * e_dz + 2.0 * kEps24 * std::fabs(o);
      } else {
        c0 = coef[3 * c];
        const double d1 = dz - (double)coef[3 * c + 1], xm = xh * (double)coef[3 * c + 2], d2 = d1 - xm;
        o = c0 * d2;
        b = std::fabs(c0) * (e_dz + kEps24 * (std::fabs(d1) + 3.0 * std::fabs(xm) + std::fabs(d2))) +
            kEps24 * std::fabs(o);
      }
      if (kink) {
        b += std::fabs(c0 * (double)da[e]);
        ++*kinks;
      }
      if (prev) {
        o += (double)prev[e];
        b += kEps24 * std::fabs(o);
      }
      r.c[e] = o;
      r.bound[e] = b;
    }
  return r;
}

// ---- k_bn_finalize -----------------------------------------------------------------------------
// P partials per channel, part [C][P] (float pairs), folded in fp64 in a fixed order: forward
// S1 = sum x, S2 = sum (m2 + x^2 / n) over the partials with cnt > 0; backward plain sums.  Only the
// fp64 additions round: (P + 8) 2^-53 of the absolute sums.
inline Sums fold_partials(const float* part2, const float* cnt, int P, int c, bool bwd) {
  Sums s;
  long double a = 0, b = 0, aa = 0, ba = 0;
  for (int p = 0; p < P; ++p) {
    const long double x = part2[2 * ((long)c * P + p)], q = part2[2 * ((long)c * P + p) + 1];
    if (bwd) {
      a += x;
      b += q;
      aa += std::fabs((double)x);
      ba += std::fabs((double)q);
    } else if (cnt[p] > 0.f) {
      a += x;
      const long double t = q + x * x / (long double)cnt[p];
      b += t;
      aa += std::fabs((double)x);
      ba += std::fabs((double)t);
    }
  }
  s.s0 = (double)a;
  s.s1 = (double)b;
  s.e0 = (P + 8) * kEps53 * (double)aa;
  s.e1 = (P + 8) * kEps53 * (double)ba;
  return s;
}

// synthetic partials of P producers over C channels: counts of 1..60 rows (zero_cnt: every seventh
// partial covers no rows and holds NaN, which must not leak), (sum, M2) pairs of plausible size
inline void gen_partials(int C, int P, bool zero_cnt, bool bwd, uint64_t seed, std::vector<float>& part,
                         std::vector<float>& cnt, long* M, long* zeros) {
  part.resize((size_t)C * P * 2);
  cnt.resize(P);
  gck::Rng rng(seed);
  *M = 0;
  *zeros = 0;
  for (int p = 0; p < P; ++p) {
    const bool zero = zero_cnt && P > 1 && p % 7 == 3;
    cnt[p] = bwd ? 1.f : zero ? 0.f : (float)(1 + rng.next() % 60);
    *M += (long)cnt[p];
    *zeros += zero;
    for (int ch = 0; ch < C; ++ch) {
      float* q = &part[2 * ((size_t)ch * P + p)];
      if (bwd) {
        q[0] = rng.uni();
        q[1] = rng.uni() * 3.f;
      } else if (zero) {
        q[0] = q[1] = gck::u2f(0x7fc00000u);
      } else {
        q[0] = cnt[p] * ((float)(ch % 5) - 2.f + 0.3f * rng.uni());                // the sum of cnt rows
        q[1] = cnt[p] > 1.f ? (cnt[p] - 1.f) * (0.5f + 0.3f * rng.uni()) : 0.f;  // M2 about the partial's mean
      }
    }
  }
}
// one moving-average step as common.hpp states it: fl(m - (m - batch) 0.01), the arithmetic in fp64
inline float moving_update(float m, double batch) { return (float)((double)m - ((double)m - batch) * 0.01); }

// ---- squeeze-excite ----------------------------------------------------------------------------
// a dot product of n terms summed in fp32 along a path of at most `depth` additions:
//   sum e_i |w_i| + depth 2^-24 sum |v_i w_i|
// The SE kernels split a sum over lane groups (G of them), an 8-way unrolled chain inside a lane and a
// tree over the 8: depth = ceil(n / G) + G + 8 covers the chain, the tree and the group fold.
inline int dot_depth(int n, int G) { return (n + G - 1) / G + G + 8; }

struct SeShape {
  int B, HW, C, N, act;     // act: the hidden activation
  int s1, cs1, jg;          // se_plan_info
};
struct SeFwdRef {
  gck::Reference pool, hidden, scale;
};
// xv: the view's values and allowances, [B][HW][C].  w1 [C][N], w2 [N][C].
inline SeFwdRef se_fwd_ref(const SeShape& s, const cck::Val& xv, const float* w1, const float* b1, const float* w2,
                           const float* b2) {
  SeFwdRef r;
  const int B = s.B, C = s.C, N = s.N;
  r.pool.c.resize((size_t)B * C); r.pool.bound.resize((size_t)B * C);
  r.hidden.c.resize((size_t)B * N); r.hidden.bound.resize((size_t)B * N);
  r.scale.c.resize((size_t)B * C); r.scale.bound.resize((size_t)B * C);
  const int G = 256 / N;
  const int d1 = dot_depth(s.cs1, G) + dot_depth(s.s1, G) + 1, d2 = dot_depth(N, s.jg) + 1;
  for (int b = 0; b < B; ++b) {
    for (int c = 0; c < C; ++c) {
      double S = 0, Sa = 0, Se = 0;
      for (int m = 0; m < s.HW; ++m) {
        const size_t e = ((size_t)b * s.HW + m) * C + c;
        S += xv.v[e];
        Sa += std::fabs(xv.v[e]);
        Se += xv.e[e];
      }
      // pool = fl(fl(S) fl(1 / HW)): three roundings
      const double eS = Se + (kRun + kFold * kEps53 / kEps24) * kEps24 * Sa;
      r.pool.c[b * C + c] = S / s.HW;
      r.pool.bound[b * C + c] = eS / s.HW * (1.0 + 4.0 * kEps24) + 3.0 * kEps24 * std::fabs(S / s.HW);
    }
    std::vector<double> a(N), ea(N);
    for (int j = 0; j < N; ++j) {
      double h = b1[j], ha = std::fabs((double)b1[j]), he = 0;
      for (int c = 0; c < C; ++c) {
        const double w = w1[(long)c * N + j];
        h += r.pool.c[b * C + c] * w;
        ha += std::fabs(r.pool.c[b * C + c] * w);
        he += r.pool.bound[b * C + c] * std::fabs(w);
      }
      r.hidden.c[b * N + j] = h;
      r.hidden.bound[b * N + j] = he + d1 * kEps24 * ha;
      cck::act_val(h, r.hidden.bound[b * N + j], s.act, &a[j], &ea[j]);
    }
    for (int c = 0; c < C; ++c) {
      double t = b2[c], ta = std::fabs((double)b2[c]), te = 0;
      for (int j = 0; j < N; ++j) {
        const double w = w2[(long)j * C + c];
        t += a[j] * w;
        ta += std::fabs(a[j] * w);
        te += ea[j] * std::fabs(w);
      }
      const double et = te + d2 * kEps24 * ta;
      // sigmoid by v_exp / v_rcp: relative 2^-24 (|t| + 5) as in act_val, slope at most 1/4
      const double sg = 1.0 / (1.0 + std::exp(-t));
      r.scale.c[b * C + c] = sg;
      r.scale.bound[b * C + c] = 0.25 * et + kEps24 * sg * (std::fabs(t) + 6.0);
    }
  }
  return r;
}

struct SeBwdRef {
  gck::Reference gsum, dx;
};
// dy, prev [B][HW][C]; scale [B][C], hidden [B][N] are inputs here (what the forward stored);
// w2t [C][N], w1 [C][N].
inline SeBwdRef se_bwd_ref(const SeShape& s, const float* dy, const cck::Val& xv, const float* scale,
                           const float* hidden, const float* w2t, const float* w1, const float* prev) {
  SeBwdRef r;
  const int B = s.B, C = s.C, N = s.N, HW = s.HW;
  r.gsum.c.resize((size_t)B * C); r.gsum.bound.resize((size_t)B * C);
  r.dx.c.resize((size_t)B * HW * C); r.dx.bound.resize((size_t)B * HW * C);
  const int G = 256 / N;
  const int d1 = dot_depth(s.cs1, G) + dot_depth(s.s1, G) + 1, d2 = dot_depth(N, s.jg) + 1;
  std::vector<double> v(C), ev(C), dh(N), edh(N);
  for (int b = 0; b < B; ++b) {
    for (int c = 0; c < C; ++c) {
      double S = 0, Sa = 0, Se = 0;
      for (int m = 0; m < HW; ++m) {
        const size_t e = ((size_t)b * HW + m) * C + c;
        const double t = (double)dy[e] * xv.v[e];
        S += t;
        Sa += std::fabs(t);
        Se += std::fabs((double)dy[e]) * xv.e[e];
      }
      const double eS = Se + (kRun + 1.0 + kFold * kEps53 / kEps24) * kEps24 * Sa;
      const double sg = scale[b * C + c], f = sg * (1.0 - sg);
      v[c] = S * f;  // fl(S), 1 - sg and two products: four roundings
      ev[c] = std::fabs(f) * eS + 4.0 * kEps24 * std::fabs(v[c]);
    }
    for (int j = 0; j < N; ++j) {
      double q = 0, qa = 0, qe = 0;
      for (int c = 0; c < C; ++c) {
        const double w = w2t[(long)c * N + j];
        q += v[c] * w;
        qa += std::fabs(v[c] * w);
        qe += ev[c] * std::fabs(w);
      }
      const double eq = qe + d1 * kEps24 * qa;
      const double h = hidden[b * N + j], g = gck::act_grad(h, s.act);
      dh[j] = q * g;  // the device evaluates act' on the same stored float: no kink ambiguity
      edh[j] = std::fabs(g) * eq + std::fabs(q) * gck::actgrad_err(h, 0.0, s.act) + kEps24 * std::fabs(dh[j]);
    }
    for (int c = 0; c < C; ++c) {
      double d = 0, da = 0, de = 0;
      for (int j = 0; j < N; ++j) {
        const double w = w1[(long)c * N + j];
        d += dh[j] * w;
        da += std::fabs(dh[j] * w);
        de += edh[j] * std::fabs(w);
      }
      const double ed = de + d2 * kEps24 * da;
      r.gsum.c[b * C + c] = d;
      r.gsum.bound[b * C + c] = ed;
      // dx = fma(dy, scale, fl(dpool fl(1 / HW))) (+ prev)
      const double dp = d / HW, edp = ed / HW + 2.0 * kEps24 * std::fabs(dp);
      for (int m = 0; m < HW; ++m) {
        const size_t e = ((size_t)b * HW + m) * C + c;
        double o = (double)dy[e] * (double)scale[b * C + c] + dp;
        double bd = edp + kEps24 * std::fabs(o);
        if (prev) {
          o += (double)prev[e];
          bd += kEps24 * std::fabs(o);
        }
        r.dx.c[e] = o;
        r.dx.bound[e] = bd;
      }
    }
  }
  return r;
}

// ---- max-pool ----------------------------------------------------------------------------------
// The forward takes the first maximum of the window in row-major scan order and records its tap.  With
// a raw input the values are exact, so value and tap are; through a BN view a tap's value is known to
// its allowance e (0 where relu6 saturates whatever the rounding), and where another tap comes within
// the allowances of the maximum — a near tie — either may win: such outputs are counted (the kink
// share) and any candidate tap is accepted with its own value.
struct PoolGeo {
  int B, H, W, C, Ho, Wo, k, s, pt, pl;
};
inline PoolGeo pool_geo(int B, int H, int W, int C, int k, int s) {
  PoolGeo g{B, H, W, C, 0, 0, k, s, 0, 0};
  cck::same_pad(H, k, s, &g.Ho, &g.pt);
  cck::same_pad(W, k, s, &g.Wo, &g.pl);
  return g;
}
// relu6 through a BN view: exact where z lies beyond the kinks by more than its rounding
inline void pool_tap(const cck::BnView& v, long e, int c, double* a, double* ea) {
  cck::inx_one(v, e, c, a, ea);
  if (v.mu && v.act == 2 && (*a == 0.0 || *a == 6.0)) {
    const double t = ((double)v.x[e] - (double)v.mu[c]) * (double)v.sc[c], z = t + (double)v.be[c];
    const double ez = kEps24 * (2.0 * std::fabs(t) + std::fabs(z));
    if (z + ez < 0.0 || z - ez > 6.0) *ea = 0.0;
  }
}
struct PoolCheck {
  Field y;
  long amax_bad = 0, ties = 0, total = 0;
};
// y: the stored values widened to float (bf: bf16 storage, compared after the same rounding)
inline PoolCheck check_maxpool_fwd(const PoolGeo& g, const cck::BnView& v, bool bf, const float* y,
                                   const uint8_t* amax) {
  PoolCheck k;
  std::vector<double> tv(g.k * g.k), te(g.k * g.k);
  std::vector<int> tap(g.k * g.k);
  for (int b = 0; b < g.B; ++b)
    for (int oy = 0; oy < g.Ho; ++oy)
      for (int ox = 0; ox < g.Wo; ++ox)
        for (int c = 0; c < g.C; ++c) {
          int n = 0;
          for (int i = 0; i < g.k; ++i) {
            const int iy = oy * g.s - g.pt + i;
            if (iy < 0 || iy >= g.H) continue;
            for (int j = 0; j < g.k; ++j) {
              const int ix = ox * g.s - g.pl + j;
              if (ix < 0 || ix >= g.W) continue;
              pool_tap(v, (((long)b * g.H + iy) * g.W + ix) * g.C + c, c, &tv[n], &te[n]);
              tap[n++] = i * g.k + j;
            }
          }
          int best = 0;
          for (int q = 1; q < n; ++q)
            if (tv[q] > tv[best]) best = q;  // the first maximum
          bool tie = false;
          for (int q = 0; q < n; ++q)
            if (q != best && tv[q] + te[q] >= tv[best] - te[best] && (te[q] > 0.0 || te[best] > 0.0)) tie = true;
          const long o = (((long)b * g.Ho + oy) * g.Wo + ox) * g.C + c;
          ++k.total;
          int got = -1;
          for (int q = 0; q < n; ++q)
            if (tap[q] == amax[o]) got = q;
          if (got < 0) {
            ++k.amax_bad;
            continue;
          }
          if (tie) {
            ++k.ties;
            if (tv[got] + te[got] < tv[best] - te[best]) ++k.amax_bad;  // not among the candidates
          } else if (got != best) {
            ++k.amax_bad;
          }
          double ref = tv[got], bd = te[got];
          if (bf) {
            const double m = std::fabs(ref) + bd;
            ref = (double)gck::round_bf((float)ref);
            if (bd > 0.0 && m > 0.0) bd += std::ldexp(1.0, std::ilogb(m) - 7);
          }
          k.y.add(y[o], ref, bd, o);
        }
  return k;
}
// the forward evaluated in float on the host (the view as common.hpp's inx_load1 forms it, libm's exp
// for swish): --plan's tie share and norm_teeth's stand-in.  last_max: the teeth's seeded fault.
inline float view_f32(const cck::BnView& v, long e, int c) {
  float x = v.x[e];
  if (!v.mu) return x;
  const float z = (x - v.mu[c]) * v.sc[c] + v.be[c];
  if (v.act == 1) return z * (1.0f / (1.0f + std::exp(-z)));
  if (v.act == 2) return std::fmin(std::fmax(z, 0.0f), 6.0f);
  return z;
}
inline void maxpool_fwd_cpu(const PoolGeo& g, const cck::BnView& v, bool last_max, std::vector<float>& y,
                            std::vector<uint8_t>& amax) {
  const size_t n = (size_t)g.B * g.Ho * g.Wo * g.C;
  y.resize(n);
  amax.resize(n);
  for (int b = 0; b < g.B; ++b)
    for (int oy = 0; oy < g.Ho; ++oy)
      for (int ox = 0; ox < g.Wo; ++ox)
        for (int c = 0; c < g.C; ++c) {
          float m = 0.f;
          int am = -1;
          for (int i = 0; i < g.k; ++i) {
            const int iy = oy * g.s - g.pt + i;
            if (iy < 0 || iy >= g.H) continue;
            for (int j = 0; j < g.k; ++j) {
              const int ix = ox * g.s - g.pl + j;
              if (ix < 0 || ix >= g.W) continue;
              const float t = view_f32(v, (((long)b * g.H + iy) * g.W + ix) * g.C + c, c);
              if (am < 0 || t > m || (last_max && t == m)) {
                m = t;
                am = i * g.k + j;
              }
            }
          }
          const size_t o = (((size_t)b * g.Ho + oy) * g.Wo + ox) * g.C + c;
          y[o] = m;
          amax[o] = (uint8_t)am;
        }
}
// the backward in the kernel's own fp32 order: windows by ascending oy, then ox; prev added last
inline std::vector<float> maxpool_bwd_replay(const PoolGeo& g, const uint8_t* amax, const float* dy, const float* prev) {
  std::vector<float> dx((size_t)g.B * g.H * g.W * g.C);
  for (int b = 0; b < g.B; ++b)
    for (int iy = 0; iy < g.H; ++iy)
      for (int ix = 0; ix < g.W; ++ix)
        for (int c = 0; c < g.C; ++c) {
          float acc = 0.f;
          for (int oy = 0; oy < g.Ho; ++oy) {
            const int i = iy - (oy * g.s - g.pt);
            if (i < 0 || i >= g.k) continue;
            for (int ox = 0; ox < g.Wo; ++ox) {
              const int j = ix - (ox * g.s - g.pl);
              if (j < 0 || j >= g.k) continue;
              const long o = (((long)b * g.Ho + oy) * g.Wo + ox) * g.C + c;
              if (amax[o] == i * g.k + j) acc += dy[o];
            }
          }
          const size_t e = (((size_t)b * g.H + iy) * g.W + ix) * g.C + c;
          if (prev) acc += prev[e];
          dx[e] = acc;
        }
  return dx;
}

// ---- nearest upsample --------------------------------------------------------------------------
// TF's legacy nearest neighbour: src = min(floor(dst * fl(in / out)), in - 1), evaluated in float as TF does
inline int nn_src(int d, int in, int out) {
  const float scale = (float)in / (float)out;
  const int s = (int)std::floor((float)d * scale);
  return s < in - 1 ? s : in - 1;
}
// the exact adjoint of that map in the kernel's order (ascending oy, then ox; prev last).
// short_by: norm_teeth's fault (the last contributing output row is left out)
inline std::vector<float> upsample_bwd_replay(int B, int H, int W, int C, int Ho, int Wo, const float* dy,
                                              const float* prev, int short_by = 0) {
  std::vector<float> dx((size_t)B * H * W * C);
  for (int b = 0; b < B; ++b)
    for (int iy = 0; iy < H; ++iy) {
      std::vector<int> oys;
      for (int oy = 0; oy < Ho; ++oy)
        if (nn_src(oy, H, Ho) == iy) oys.push_back(oy);
      if (short_by && oys.size() > 1) oys.pop_back();
      for (int ix = 0; ix < W; ++ix)
        for (int c = 0; c < C; ++c) {
          float acc = 0.f;
          for (int oy : oys)
            for (int ox = 0; ox < Wo; ++ox)
              if (nn_src(ox, W, Wo) == ix) acc += dy[(((long)b * Ho + oy) * Wo + ox) * C + c];
          const size_t e = (((size_t)b * H + iy) * W + ix) * C + c;
          if (prev) acc += prev[e];
          dx[e] = acc;
        }
    }
  return dx;
}

// ---- residual add ------------------------------------------------------------------------------
// y = (a / p) keep + b: the division is IEEE (div_surv), keep is 0 or 1, one addition
inline gck::Reference add_ref(const cck::Val& a, const cck::Val& b, long rows, int C, const float* keep, float p,
                              long rows_per_image) {
  gck::Reference r;
  r.c.resize(a.v.size());
  r.bound.resize(a.v.size());
  for (long m = 0; m < rows; ++m)
    for (int c = 0; c < C; ++c) {
      const size_t e = (size_t)m * C + c;
      double u = a.v[e], eu = a.e[e];
      if (keep) {
        const double k = keep[m / rows_per_image];
        u = u / (double)p * k;
        eu = (eu / (double)p + kEps24 * std::fabs(u)) * k;
      }
      r.c[e] = u + b.v[e];
      r.bound[e] = eu + b.e[e] + kEps24 * std::fabs(r.c[e]);
    }
  return r;
}
// ---- BiFPN fuse backward -----------------------------------------------------------------------
// dv = dy act'(v) with v the fused pre-activation (view_fuse's value and allowance before the activation);
// method 0: g_k = (dv / den) w_k — den in fp32 (three roundings), an IEEE division, a product: 5 2^-24 of
// the result; method 1: g_k = dv.  (+ prev: one more rounding.)  An element whose v lies within its
// allowance of a relu6 kink may take either side: the whole |dy| w_k / den, counted as a kink.
// prev[k] empty: no accumulation.  Returns the kink count; out[k] for every k < nin.
inline long fuse_bwd_ref(const cck::FuseRef& f, long px, int C, const float* dy, const std::vector<float>* prev,
                         gck::Reference* out) {
  double wv[3] = {1.0, 1.0, 1.0}, den = 1.0;
  if (f.method == 0) {
    den = 0.0;
    for (int i = 0; i < f.nin; ++i) {
      wv[i] = std::max((double)f.w[i], 0.0);
      den += wv[i];
    }
    den += (double)0.0001f;
  }
  for (int k = 0; k < f.nin; ++k) {
    out[k].c.assign((size_t)px * C, 0.0);
    out[k].bound.assign((size_t)px * C, 0.0);
  }
  long kinks = 0;
  for (long p = 0; p < px; ++p)
    for (int c = 0; c < C; ++c) {
      const long e = p * C + c;
      double v = 0.0, ev = 0.0;
      for (int i = 0; i < f.nin; ++i) {
        double a, ea;
        cck::inx_one(f.x[i], e, c, &a, &ea);
        const double t = a * wv[i] / den;
        v += t;
        ev += ea * wv[i] / den + (f.method == 0 ? 7.0 : 2.0) * kEps24 * std::fabs(t);
      }
      const double g = gck::act_grad(v, f.act), d = dy[e];
      const bool kink = f.act == 2 && (std::fabs(v) <= ev || std::fabs(v - 6.0) <= ev);
      const double dv = d * g, e_dv = std::fabs(d) * gck::actgrad_err(v, ev, f.act) + kEps24 * std::fabs(dv);
      kinks += kink;
      for (int k = 0; k < f.nin; ++k) {
        const double s = f.method == 0 ? wv[k] / den : 1.0;
        double o = dv * s, b = e_dv * s + (f.method == 0 ? 5.0 * kEps24 * std::fabs(o) : 0.0);
        if (kink) b += std::fabs(d) * s;
        if (!prev[k].empty()) {
          o += (double)prev[k][e];
          b += kEps24 * std::fabs(o);
        }
        out[k].c[e] = o;
        out[k].bound[e] = b;
      }
    }
  return kinks;
}

// dst (+)= (src keep) / p, replayed in float: the product is exact, the division IEEE, prev added last
inline std::vector<float> copy_grad_replay(const float* src, long rows, int C, const float* keep, float p,
                                           long rows_per_image, const float* prev) {
  std::vector<float> o((size_t)rows * C);
  for (long m = 0; m < rows; ++m)
    for (int c = 0; c < C; ++c) {
      const size_t e = (size_t)m * C + c;
      float v = src[e];
      if (keep) v = (v * keep[m / rows_per_image]) / p;
      if (prev) v += prev[e];
      o[e] = v;
    }
  return o;
}

}  // namespace nck
