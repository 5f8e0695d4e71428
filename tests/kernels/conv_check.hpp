// conv_check.hpp — the host side of the depthwise / fused separable conv parity checker: the input views
// (BN view, BiFPN fuse view, BN-backward gradient view) in fp64 with a per-element allowance for the fp32
// roundings of the device's view, the fp64 depthwise forward and its exact adjoint, the pointwise
// products of the separable conv, and the derived per-element bounds ("Conv kernel parity").
// Plain C++ (no HIP).  The comparisons themselves — check_c, check_statsink, check_gradsink, the guard
// regions — are gemm_check.hpp's: conv_parity.cpp runs them on what the device wrote, conv_teeth.cpp on
// a CPU stand-in with seeded faults.
#pragma once
#include "gemm_check.hpp"

namespace cck {

using gck::kEps24;

// ---- geometry ----------------------------------------------------------------------------------
// TF SAME: out = ceil(in / s), pad = max((out - 1) s + k - in, 0), the smaller half in front
inline void same_pad(int in, int k, int s, int* out, int* before) {
  *out = (in + s - 1) / s;
  const int pad = std::max((*out - 1) * s + k - in, 0);
  *before = pad / 2;
}
struct Geo {
  int B = 0, H = 0, W = 0, C = 0;  // conv input [B][H][W][C]
  int Ho = 0, Wo = 0;              // conv output [B][Ho][Wo][C]
  int k = 3, s = 1, pt = 0, pl = 0;
  long in_px() const { return (long)B * H * W; }
  long out_px() const { return (long)B * Ho * Wo; }
};
inline Geo make_geo(int B, int H, int W, int C, int k, int s) {
  Geo g;
  g.B = B; g.H = H; g.W = W; g.C = C; g.k = k; g.s = s;
  same_pad(H, k, s, &g.Ho, &g.pt);
  same_pad(W, k, s, &g.Wo, &g.pl);
  return g;
}

// ---- views -------------------------------------------------------------------------------------
// a tensor as the conv sees it: the fp64 value of every element and e, how far the device's fp32
// evaluation of the view may lie from it (0 for a raw tensor; the full jump where a relu6-derivative
// kink may fall on either side)
struct Val {
  std::vector<double> v, e;
  long kinks = 0;  // elements under the kink allowance
};

// a = act(z) given |z_dev - z| <= ez.
//   swish = z * rcp(1 + exp(-z)) with v_exp_f32 / v_rcp_f32 (1 ulp = 2 * 2^-24 each).  exp(-z) is
//   exp2(-z * log2 e): the product's rounding moves the exponent by 2^-24 |z| log2 e, so the result by
//   (|z| + 2) 2^-24 relative; 1 + e one rounding, rcp 2, the product with z one more:
//     |a_dev - a| <= 2^-24 |a| (|z| + 6) + 1.1 ez          (|d swish / dz| <= 1.0999)
//   relu6 is exact and 1-Lipschitz.
inline void act_val(double z, double ez, int act, double* a, double* ea) {
  *a = gck::act_fwd(z, act);
  if (act == 1) *ea = kEps24 * std::fabs(*a) * (std::fabs(z) + 6.0) + 1.1 * ez;
  else *ea = ez;
}
// g = act'(z) and how far the device's evaluation may lie from it (gck::actgrad_err)
inline void actgrad_val(double z, double ez, int act, double* g, double* eg) {
  *g = gck::act_grad(z, act);
  *eg = gck::actgrad_err(z, ez, act);
}

struct BnView {  // InX: act((x - mu) sc + be); mu == nullptr: the raw tensor
  const float* x = nullptr;
  const float *mu = nullptr, *sc = nullptr, *be = nullptr;
  int act = 0;
};
// z = (x - mu) sc + be: the difference, the product and the sum round once each,
//   |z_dev - z| <= 2^-24 (2 |yc sc| + |z|)
inline void inx_one(const BnView& b, long e, int c, double* a, double* ea) {
  const double x = b.x[e];
  if (!b.mu) {
    *a = x;
    *ea = 0.0;
    return;
  }
  const double t = (x - (double)b.mu[c]) * (double)b.sc[c];
  const double z = t + (double)b.be[c];
  act_val(z, kEps24 * (2.0 * std::fabs(t) + std::fabs(z)), b.act, a, ea);
}
inline Val view_inx(const BnView& b, long px, int C) {
  Val r;
  r.v.resize((size_t)px * C);
  r.e.resize((size_t)px * C);
  for (long p = 0; p < px; ++p)
    for (int c = 0; c < C; ++c) inx_one(b, p * C + c, c, &r.v[p * C + c], &r.e[p * C + c]);
  return r;
}

// BiFPN node fuse: method 0 act(sum_i x_i relu(w_i) / (sum_j relu(w_j) + 1e-4)), method 1 act(sum_i x_i).
// The device forms den = (w0 + w1 (+ w2)) + 1e-4f in fp32 (three roundings) and each term as
// x_i * w_i / den with a correctly rounded division (hipcc's default for `/`: no fast-math flag in the
// library's build), then adds the terms: a term is off by its input's own allowance plus 5 * 2^-24 of
// itself (product, quotient, den), and the two additions by 2^-24 of the partial sums:
//   |v_dev - v| <= sum_i (e_i w_i / den + 7 2^-24 |term_i|)
struct FuseRef {
  BnView x[3];
  int nin = 2;
  float w[3] = {0.f, 0.f, 0.f};
  int method = 0, act = 0;
};
inline Val view_fuse(const FuseRef& f, long px, int C) {
  Val r;
  r.v.resize((size_t)px * C);
  r.e.resize((size_t)px * C);
  double wv[3] = {1.0, 1.0, 1.0}, den = 1.0;
  if (f.method == 0) {
    den = 0.0;
    for (int i = 0; i < f.nin; ++i) {
      wv[i] = std::max((double)f.w[i], 0.0);
      den += wv[i];
    }
    den += (double)0.0001f;
  }
  for (long p = 0; p < px; ++p)
    for (int c = 0; c < C; ++c) {
      double v = 0.0, ev = 0.0;
      for (int i = 0; i < f.nin; ++i) {
        double a, ea;
        inx_one(f.x[i], p * C + c, c, &a, &ea);
        const double t = a * wv[i] / den;
        v += t;
        ev += ea * wv[i] / den + (f.method == 0 ? 7.0 : 2.0) * kEps24 * std::fabs(t);
      }
      act_val(v, ev, f.act, &r.v[p * C + c], &r.e[p * C + c]);
    }
  return r;
}

// GradX: sc (dz - mdz - xhat mdzx), dz = da act'(z), z = (y - mu) sc + be, xhat = (y - mu) rstd;
// y == nullptr: da itself.  Roundings of gx_one (common.hpp), in order: dz one (+ act' as above), the
// first difference one, xhat two, its product with mdzx one more, the second difference one, the
// product with sc one.
struct GradRef {
  const float *da = nullptr, *y = nullptr;
  const float *mu = nullptr, *rstd = nullptr, *sc = nullptr, *be = nullptr, *mdz = nullptr, *mdzx = nullptr;
  int act = 0;
};
inline Val view_grad(const GradRef& g, long px, int C) {
  Val r;
  r.v.resize((size_t)px * C);
  r.e.assign((size_t)px * C, 0.0);
  for (long p = 0; p < px; ++p)
    for (int c = 0; c < C; ++c) {
      const long e = p * C + c;
      const double d = g.da[e];
      if (!g.y) {
        r.v[e] = d;
        continue;
      }
      const double yc = (double)g.y[e] - (double)g.mu[c];
      const double t = yc * (double)g.sc[c], z = t + (double)g.be[c];
      double ga, ega;
      actgrad_val(z, kEps24 * (2.0 * std::fabs(t) + std::fabs(z)), g.act, &ga, &ega);
      const double dz = d * ga;
      const double xm = yc * (double)g.rstd[c] * (double)g.mdzx[c];
      const double d1 = dz - (double)g.mdz[c], d2 = d1 - xm;
      const double sc = g.sc[c];
      r.v[e] = sc * d2;
      r.e[e] = std::fabs(sc) * (std::fabs(d) * ega +
                                kEps24 * (std::fabs(dz) + std::fabs(d1) + 3.0 * std::fabs(xm) + std::fabs(d2))) +
               kEps24 * std::fabs(r.v[e]);
      if (gck::near_kink(z, std::fabs(t) + std::fabs((double)g.be[c]), g.act)) {
        r.e[e] += std::fabs(sc * d);
        ++r.kinks;
      }
    }
  return r;
}
// elements of a GradSink's BN input that fall under check_gradsink's kink allowance
inline long gradsink_kinks(const float* y, long px, int C, const float* mu, const float* sc, const float* be,
                           int act) {
  long n = 0;
  for (long p = 0; p < px; ++p)
    for (int c = 0; c < C; ++c) {
      const double t = ((double)y[p * C + c] - (double)mu[c]) * (double)sc[c];
      n += gck::near_kink(t + (double)be[c], std::fabs(t) + std::fabs((double)be[c]), act);
    }
  return n;
}

// ---- depthwise conv ----------------------------------------------------------------------------
// y[oy][ox] = sum_ij a[oy s - pt + i][ox s - pl + j] w[i][j], zero outside the image (after the view).
//   bound = k k 2^-24 sum |a w| + sum e |w|
// (k k fmas from zero: at most k k roundings of partial sums no larger than sum |a w|)
inline gck::Reference dw_fwd_ref(const Geo& g, const Val& a, const float* w) {
  gck::Reference r;
  const int C = g.C, k = g.k;
  r.c.assign((size_t)g.out_px() * C, 0.0);
  r.bound.assign((size_t)g.out_px() * C, 0.0);
  gck::par_rows((long)g.B * g.Ho, [&](long r0, long r1) {
    for (long row = r0; row < r1; ++row) {
      const int b = (int)(row / g.Ho), oy = (int)(row % g.Ho);
      for (int ox = 0; ox < g.Wo; ++ox)
        for (int c = 0; c < C; ++c) {
          double s = 0.0, sa = 0.0, se = 0.0;
          for (int i = 0; i < k; ++i) {
            const int iy = oy * g.s - g.pt + i;
            if (iy < 0 || iy >= g.H) continue;
            for (int j = 0; j < k; ++j) {
              const int ix = ox * g.s - g.pl + j;
              if (ix < 0 || ix >= g.W) continue;
              const long e = (((long)b * g.H + iy) * g.W + ix) * C + c;
              const double wv = w[(i * k + j) * C + c];
              s += a.v[e] * wv;
              sa += std::fabs(a.v[e] * wv);
              se += a.e[e] * std::fabs(wv);
            }
          }
          const long o = (row * g.Wo + ox) * C + c;
          r.c[o] = s;
          r.bound[o] = k * k * kEps24 * sa + se;
        }
    }
  });
  return r;
}

// the exact adjoint: dx[iy][ix] (+)= sum over (oy, i), (ox, j) with oy s - pt + i = iy, ox s - pl + j = ix
// of gy[oy][ox] w[i][j].  prev != nullptr: accumulate (one more rounding of the sum).
inline gck::Reference dw_bwd_ref(const Geo& g, const Val& gy, const float* w, const float* prev) {
  gck::Reference r;
  const int C = g.C, k = g.k;
  const size_t n = (size_t)g.in_px() * C;
  r.c.assign(n, 0.0);
  r.bound.assign(n, 0.0);
  std::vector<double> sa(n, 0.0);
  for (int b = 0; b < g.B; ++b)
    for (int oy = 0; oy < g.Ho; ++oy)
      for (int ox = 0; ox < g.Wo; ++ox) {
        const long o = (((long)b * g.Ho + oy) * g.Wo + ox) * C;
        for (int i = 0; i < k; ++i) {
          const int iy = oy * g.s - g.pt + i;
          if (iy < 0 || iy >= g.H) continue;
          for (int j = 0; j < k; ++j) {
            const int ix = ox * g.s - g.pl + j;
            if (ix < 0 || ix >= g.W) continue;
            const long e = (((long)b * g.H + iy) * g.W + ix) * C;
            for (int c = 0; c < C; ++c) {
              const double wv = w[(i * k + j) * C + c];
              r.c[e + c] += gy.v[o + c] * wv;
              sa[e + c] += std::fabs(gy.v[o + c] * wv);
              r.bound[e + c] += gy.e[o + c] * std::fabs(wv);
            }
          }
        }
      }
  for (size_t e = 0; e < n; ++e) {
    r.bound[e] += k * k * kEps24 * sa[e];
    if (prev) {
      r.c[e] += (double)prev[e];
      r.bound[e] += kEps24 * (sa[e] + std::fabs((double)prev[e]));
    }
  }
  return r;
}

// an output stored as bf16: the reference rounds as the store does, and a device value on the other side
// of a rounding boundary lands one quantum away (the spacing of bf16 at the largest magnitude the bound admits)
inline void bf_store(gck::Reference& r) {
  for (size_t i = 0; i < r.c.size(); ++i) {
    const double m = std::fabs(r.c[i]) + r.bound[i];
    r.c[i] = (double)gck::round_bf((float)r.c[i]);
    if (m > 0.0) r.bound[i] += std::ldexp(1.0, std::ilogb(m) - 7);
  }
}
// as a view input (value, allowance)
inline Val as_val(const gck::Reference& r) {
  Val v;
  v.v = r.c;
  v.e = r.bound;
  return v;
}

// ---- the separable conv's pointwise halves -----------------------------------------------------
// y[p][n] = sum_c d[p][c] bt[n][c] + bias[n]:
//   bound = sum_c bound_d |bt| + (C + 2) 2^-24 sum_c |d bt| + 2^-24 |bias|
// (C accumulations on the fp32 matrix core, the bias add, one spare)
inline gck::Reference pw_fwd_ref(const gck::Reference& d, long px, int C, int N, const float* bt,
                                 const float* bias) {
  gck::Reference r;
  r.c.assign((size_t)px * N, 0.0);
  r.bound.assign((size_t)px * N, 0.0);
  gck::par_rows(px, [&](long p0, long p1) {
    for (long p = p0; p < p1; ++p)
      for (int n = 0; n < N; ++n) {
        double s = 0.0, sa = 0.0, se = 0.0;
        for (int c = 0; c < C; ++c) {
          const double b = bt[(long)n * C + c];
          s += d.c[p * C + c] * b;
          sa += std::fabs(d.c[p * C + c] * b);
          se += d.bound[p * C + c] * std::fabs(b);
        }
        const double bv = bias ? (double)bias[n] : 0.0;
        r.c[p * N + n] = s + bv;
        r.bound[p * N + n] = se + (C + 2) * kEps24 * sa + kEps24 * std::fabs(bv);
      }
  });
  return r;
}
// dd[p][c] = sum_n g[p][n] wp[c][n]: allowance sum_n e_g |wp| + N 2^-24 sum_n |g wp|
inline Val pw_bwd_ref(const Val& g, long px, int N, int C, const float* wp) {
  Val r;
  r.v.assign((size_t)px * C, 0.0);
  r.e.assign((size_t)px * C, 0.0);
  r.kinks = g.kinks;
  gck::par_rows(px, [&](long p0, long p1) {
    for (long p = p0; p < p1; ++p)
      for (int c = 0; c < C; ++c) {
        double s = 0.0, sa = 0.0, se = 0.0;
        for (int n = 0; n < N; ++n) {
          const double wv = wp[(long)c * N + n];
          s += g.v[p * N + n] * wv;
          sa += std::fabs(g.v[p * N + n] * wv);
          se += g.e[p * N + n] * std::fabs(wv);
        }
        r.v[p * C + c] = s;
        r.e[p * C + c] = se + N * kEps24 * sa;
      }
  });
  return r;
}

}  // namespace cck
