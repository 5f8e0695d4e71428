// conv3_check.hpp — the host side of the dense 3x3 conv parity checker: the fp64 references of the stem
// (3x3, stride 2, TF SAME on even sides) and its exact adjoint, of the U-Net's conv / transposed conv as
// k_im2col's header comment defines its two modes, of their data gradients (written as the adjoint of the
// forward, not as the gather the device runs) and of the weight gradient in the Keras layouts, the exact
// images of the value-moving kernels (un_im2col, un_wprep), the stem data gradient's per-tile ownership
// rule, and the derived per-element bounds ("Dense 3x3 conv kernel parity").  Plain C++ (no
// HIP).  The comparisons — check_c, check_statsink, the guard regions — are gemm_check.hpp's, the gradient
// view is conv_check.hpp's: conv3_parity.cpp runs them on what the device wrote, conv3_teeth.cpp on a CPU
// stand-in with seeded faults.
#pragma once
#include "conv_check.hpp"

namespace c3k {

using gck::kEps24;

// ---- the gathers ---------------------------------------------------------------------------------
// mode 0: conv, out (oy, ox) tap (ky, kx) reads x[oy s + ky - pt][ox s + kx - pl]
// mode 1: transposed conv (stride 2): out (oy, ox) tap (ky, kx) reads x[(oy - ky) / 2][(ox - kx) / 2] when
//         both differences are even and >= 0
// zero outside the H x W input
struct Gather {
  int B = 1, H = 0, W = 0, C = 0;  // input [B][H][W][C]
  int Ho = 0, Wo = 0;              // output pixels
  int mode = 0, s = 1, pt = 0, pl = 0;
  long in_px() const { return (long)B * H * W; }
  long out_px() const { return (long)B * Ho * Wo; }
};
// the three gathers of the defender: 0 conv stride 1 pads (1, 1); 1 stride 2 pads (0, 0) over an input
// twice the output (the transposed conv's data gradient; reads row iy == H); 2 the transposed conv
inline Gather make_gather(int kind, int B, int H, int W, int C) {
  Gather g;
  g.B = B; g.H = H; g.W = W; g.C = C;
  if (kind == 0) { g.Ho = H; g.Wo = W; g.mode = 0; g.s = 1; g.pt = g.pl = 1; }
  else if (kind == 1) { g.Ho = H / 2; g.Wo = W / 2; g.mode = 0; g.s = 2; }
  else { g.Ho = 2 * H; g.Wo = 2 * W; g.mode = 1; g.s = 2; }
  return g;
}
inline bool tap_at(const Gather& g, int oy, int ox, int ky, int kx, int* iy, int* ix) {
  if (g.mode == 0) {
    *iy = oy * g.s + ky - g.pt;
    *ix = ox * g.s + kx - g.pl;
  } else {
    const int dy = oy - ky, dx = ox - kx;
    if (dy < 0 || dx < 0 || dy % 2 != 0 || dx % 2 != 0) return false;
    *iy = dy / 2;
    *ix = dx / 2;
  }
  return *iy >= 0 && *iy < g.H && *ix >= 0 && *ix < g.W;
}

inline int pad4(int k) { return (k + 3) / 4 * 4; }

// ---- exact moves ---------------------------------------------------------------------------------
// col [out_px][Kp], k = (ky 3 + kx) C + c, zero for k >= 9C
inline std::vector<float> im2col_ref(const Gather& g, const float* x, int Kp) {
  std::vector<float> col((size_t)g.out_px() * Kp, 0.f);
  for (int b = 0; b < g.B; ++b)
    for (int oy = 0; oy < g.Ho; ++oy)
      for (int ox = 0; ox < g.Wo; ++ox) {
        float* row = &col[((((size_t)b * g.Ho + oy) * g.Wo) + ox) * Kp];
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            int iy, ix;
            if (!tap_at(g, oy, ox, ky, kx, &iy, &ix)) continue;
            const float* xp = x + (((long)b * g.H + iy) * g.W + ix) * g.C;
            for (int c = 0; c < g.C; ++c) row[(ky * 3 + kx) * g.C + c] = xp[c];
          }
      }
  return col;
}

// The Keras kernels: conv W[ky][kx][ci][co], transposed conv Wt[ky][kx][co][ci], 1x1 W[ci][co].
// wk(kernel, tconv, ci, co, tap, c_in, c_out): the weight that multiplies input channel c_in into output
// channel c_out at tap (ky 3 + kx) of the layer's FORWARD
inline float wk(const float* w, bool tconv, int ci, int co, int tap, int c_in, int c_out) {
  return tconv ? w[((long)tap * co + c_out) * ci + c_in] : w[((long)tap * ci + c_in) * co + c_out];
}
// The GEMM B operands un_wprep derives (bt [N][Kp], zero for k >= taps * channels), each written from what
// the operand must be for the gather it is used with:
//   kind 0 / 2 / 4 (forward): N = co, k = (tap, c_in): the forward's own weight
//   kind 1: the conv's data gradient runs as a stride-1 pads-(1, 1) conv of dy: dx[p] = sum_t' dy[p + t' - 1] B[t'],
//           and the forward sends x[p] to y[p - (t - 1)] through W[t], so t' = 2 - t on both axes
//   kind 3: the transposed conv's data gradient gathers dy[2 i + t], the pixel the forward wrote x[i] to
//           through Wt[t]: the tap is kept
//   kind 5: 1x1, N = ci, k = c_out
inline std::vector<float> wprep_ref(const float* w, int kind, int ci, int co, int Kp) {
  const bool dg = kind & 1, tconv = kind == 2 || kind == 3;
  const int N = dg ? ci : co, Kin = dg ? co : ci, taps = kind >= 4 ? 1 : 9;
  std::vector<float> bt((size_t)N * Kp, 0.f);
  for (int n = 0; n < N; ++n)
    for (int tap = 0; tap < taps; ++tap)
      for (int c = 0; c < Kin; ++c) {
        const int c_in = dg ? n : c, c_out = dg ? c : n;
        int ft = tap;  // the forward's tap
        if (kind == 1) ft = (2 - tap / 3) * 3 + (2 - tap % 3);
        bt[(size_t)n * Kp + tap * Kin + c] = wk(w, tconv, ci, co, ft, c_in, c_out);
      }
  return bt;
}

// ---- conv / transposed conv forward and its adjoint ------------------------------------------------
// y[b][oy][ox][n] = bias[n] + sum over taps and c of x[tap's pixel][c] wk(tap, c, n)
//   bound = (Kc + 16) 2^-24 (sum |x w| + |bias|): Kc accumulations on the fp32 matrix core (the K the
//   device walks, zero columns included), 16 as for the GEMM
struct Weights {
  const float* w = nullptr;  // a Keras kernel (wk) ...
  bool tconv = false;
  int ci = 0, co = 0;
  const float* bt = nullptr;  // ... or a ready B operand [N][ldb], k = (tap, c)
  int ldb = 0;
  double at(int tap, int c_in, int c_out) const {
    return bt ? (double)bt[(long)c_out * ldb + tap * ci + c_in] : (double)wk(w, tconv, ci, co, tap, c_in, c_out);
  }
};
inline gck::Reference conv_fwd_ref(const Gather& g, const float* x, const Weights& wt, int N, const float* bias,
                                   int Kc) {
  gck::Reference r;
  r.c.assign((size_t)g.out_px() * N, 0.0);
  r.bound.assign((size_t)g.out_px() * N, 0.0);
  std::vector<double> wd((size_t)9 * g.C * N);
  for (int t = 0; t < 9; ++t)
    for (int c = 0; c < g.C; ++c)
      for (int n = 0; n < N; ++n) wd[((size_t)t * g.C + c) * N + n] = wt.at(t, c, n);
  gck::par_rows((long)g.B * g.Ho, [&](long r0, long r1) {
    std::vector<double> s(N), sa(N);
    for (long row = r0; row < r1; ++row) {
      const int b = (int)(row / g.Ho), oy = (int)(row % g.Ho);
      for (int ox = 0; ox < g.Wo; ++ox) {
        for (int n = 0; n < N; ++n) {
          s[n] = bias ? (double)bias[n] : 0.0;
          sa[n] = std::fabs(s[n]);
        }
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            int iy, ix;
            if (!tap_at(g, oy, ox, ky, kx, &iy, &ix)) continue;
            const float* xp = x + (((long)b * g.H + iy) * g.W + ix) * g.C;
            for (int c = 0; c < g.C; ++c) {
              const double* wr = &wd[((size_t)(ky * 3 + kx) * g.C + c) * N];
              const double xv = xp[c];
              for (int n = 0; n < N; ++n) {
                const double t = xv * wr[n];
                s[n] += t;
                sa[n] += std::fabs(t);
              }
            }
          }
        const long o = (row * g.Wo + ox) * N;
        for (int n = 0; n < N; ++n) {
          r.c[o + n] = s[n];
          r.bound[o + n] = (Kc + 16) * kEps24 * sa[n];
        }
      }
    }
  });
  return r;
}
// the exact adjoint: dx[tap's pixel][c] += dy[b][oy][ox][n] wk(tap, c, n) over the same (pixel, tap) pairs
inline gck::Reference conv_adj_ref(const Gather& g, const float* dy, const Weights& wt, int N, int Kc) {
  gck::Reference r;
  const size_t n_in = (size_t)g.in_px() * g.C;
  r.c.assign(n_in, 0.0);
  r.bound.assign(n_in, 0.0);
  for (int b = 0; b < g.B; ++b)
    for (int oy = 0; oy < g.Ho; ++oy)
      for (int ox = 0; ox < g.Wo; ++ox) {
        const float* gp = dy + (((long)b * g.Ho + oy) * g.Wo + ox) * N;
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            int iy, ix;
            if (!tap_at(g, oy, ox, ky, kx, &iy, &ix)) continue;
            const long e = (((long)b * g.H + iy) * g.W + ix) * g.C;
            for (int c = 0; c < g.C; ++c)
              for (int n = 0; n < N; ++n) {
                const double t = (double)gp[n] * wt.at(ky * 3 + kx, c, n);
                r.c[e + c] += t;
                r.bound[e + c] += std::fabs(t);
              }
          }
      }
  for (size_t e = 0; e < n_in; ++e) r.bound[e] *= (Kc + 16) * kEps24;
  return r;
}

// ---- the stem ------------------------------------------------------------------------------------
// 3x3 stride 2, TF SAME on even sides: pads 0 top / left, 1 bottom / right.  x [B][H][W][3], w HWIO
// [3][3][3][Co].  27 fmas from zero: bound = (27 + 16) 2^-24 sum |x w|
inline gck::Reference stem_fwd_ref(int B, int H, int W, int Co, const float* x, const float* w) {
  Gather g;
  g.B = B; g.H = H; g.W = W; g.C = 3; g.Ho = H / 2; g.Wo = W / 2; g.mode = 0; g.s = 2;
  Weights wt;
  wt.w = w; wt.ci = 3; wt.co = Co;
  return conv_fwd_ref(g, x, wt, Co, nullptr, 27);
}
// the exact adjoint through a gradient view gy (value, allowance): per element at most four dy pixels of
// Co products each: bound = (4 Co + 16) 2^-24 (sum |g w| + |prev|) + sum e |w|
inline gck::Reference stem_bwd_ref(int B, int H, int W, int Co, const cck::Val& gy, const float* w,
                                   const float* prev) {
  gck::Reference r;
  const int Ho = H / 2, Wo = W / 2;
  const size_t n = (size_t)B * H * W * 3;
  r.c.assign(n, 0.0);
  r.bound.assign(n, 0.0);
  std::vector<double> se(n, 0.0);
  for (int b = 0; b < B; ++b)
    for (int oy = 0; oy < Ho; ++oy)
      for (int ox = 0; ox < Wo; ++ox) {
        const long o = (((long)b * Ho + oy) * Wo + ox) * Co;
        for (int i = 0; i < 3; ++i) {
          const int iy = 2 * oy + i;
          if (iy >= H) continue;
          for (int j = 0; j < 3; ++j) {
            const int ix = 2 * ox + j;
            if (ix >= W) continue;
            const long e = (((long)b * H + iy) * W + ix) * 3;
            for (int ci = 0; ci < 3; ++ci)
              for (int c = 0; c < Co; ++c) {
                const double wv = w[((i * 3 + j) * 3 + ci) * Co + c];
                r.c[e + ci] += gy.v[o + c] * wv;
                r.bound[e + ci] += std::fabs(gy.v[o + c] * wv);
                se[e + ci] += gy.e[o + c] * std::fabs(wv);
              }
          }
        }
      }
  for (size_t e = 0; e < n; ++e) {
    const double p = prev ? (double)prev[e] : 0.0;
    r.c[e] += p;
    r.bound[e] = (4 * Co + 16) * kEps24 * (r.bound[e] + std::fabs(p)) + se[e];
  }
  return r;
}

// launch_stem_bwd_gx's ownership rule, per 32 x 32-pixel tile (16 x 16 quads from the top left): live[b][ty][tx]
// = any element of the tile's in-range pixels has owner >= 0 (owner == nullptr: all live)
constexpr int kTileQ = 16;
struct TileMap {
  int tx = 0, ty = 0;
  std::vector<uint8_t> live;  // [B][ty][tx]
  bool at(int b, int iy, int ix) const { return live[((size_t)b * ty + iy / (2 * kTileQ)) * tx + ix / (2 * kTileQ)] != 0; }
};
inline TileMap stem_tiles(int B, int H, int W, const int16_t* owner) {
  TileMap t;
  t.tx = (W / 2 + kTileQ - 1) / kTileQ;
  t.ty = (H / 2 + kTileQ - 1) / kTileQ;
  t.live.assign((size_t)B * t.tx * t.ty, owner ? 0 : 1);
  if (owner)
    for (int b = 0; b < B; ++b)
      for (int iy = 0; iy < H; ++iy)
        for (int ix = 0; ix < W; ++ix)
          for (int c = 0; c < 3; ++c)
            if (owner[(((long)b * H + iy) * W + ix) * 3 + c] >= 0)
              t.live[((size_t)b * t.ty + iy / (2 * kTileQ)) * t.tx + ix / (2 * kTileQ)] = 1;
  return t;
}
// the dy pixels some live tile's quads read: output pixel (oy, ox) feeds input rows 2 oy .. 2 oy + 2
inline std::vector<uint8_t> stem_dy_read(int B, int H, int W, const TileMap& t) {
  const int Ho = H / 2, Wo = W / 2;
  std::vector<uint8_t> rd((size_t)B * Ho * Wo, 0);
  for (int b = 0; b < B; ++b)
    for (int oy = 0; oy < Ho; ++oy)
      for (int ox = 0; ox < Wo; ++ox)
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            const int iy = 2 * oy + i, ix = 2 * ox + j;
            if (iy < H && ix < W && t.at(b, iy, ix)) rd[((size_t)b * Ho + oy) * Wo + ox] = 1;
          }
  return rd;
}
struct TileCheck {
  long dead_bad = 0;   // elements of dead tiles that are not +0.0 bit for bit
  long dead = 0, livep = 0;
};
// dead tiles must hold +0.0; the reference is zeroed there with a zero bound so check_c sees the same rule
inline TileCheck apply_tiles(int B, int H, int W, const TileMap& t, gck::Reference& r, const float* dx) {
  TileCheck k;
  for (int b = 0; b < B; ++b)
    for (int iy = 0; iy < H; ++iy)
      for (int ix = 0; ix < W; ++ix) {
        const long e = (((long)b * H + iy) * W + ix) * 3;
        if (t.at(b, iy, ix)) {
          k.livep += 3;
          continue;
        }
        for (int c = 0; c < 3; ++c) {
          ++k.dead;
          r.c[e + c] = 0.0;
          r.bound[e + c] = 0.0;
          if (dx && gck::f2u(dx[e + c]) != 0u) ++k.dead_bad;
        }
      }
  return k;
}

// ---- weight gradient -----------------------------------------------------------------------------
// g = col^T dy over the M rows, scattered to the Keras layout: kind 0 [ky][kx][ci][co], kind 2
// [ky][kx][co][ci], kind 4 [ci][co] (ci = Kin, the channels along K; co = Co).  col: src 0 the matrix
// x[m ldx + k]; src 1 gather 0 over x [B][H][W][C]; src 2 gather 2 (the transposed conv) over x [B][H/2][W/2][C].
// The summation tree of the device (k_wgrad_mfma + k_wgrad_fold), for `rps` rows per slice and ns slices:
//   a wave takes every fourth 4-row step of its slice: rps / 16 MFMAs, each adding four products to the
//   accumulator (at most four roundings each, whatever the order inside the matrix core): rps / 4;
//   the four waves' tiles are added in order: 3;
//   the fold's 16 lanes add every 16th slice: ceil(ns / 16); lane 0 adds the 16 lane sums: 15.
// No term passes through more additions than D = rps / 4 + 3 + ceil(ns / 16) + 15, so
//   bound = (D + 16) 2^-24 sum_m |dy col|
// (16: the products' roundings and slack, as for the GEMM).  D does not grow with M beyond the slice.
inline int wgrad_depth(long rps, int ns) { return (int)(rps / 4) + 3 + (ns + 15) / 16 + 15; }
struct WgradGeo {
  int src = 0, B = 1, H = 0, W = 0, C = 0;  // src 1 / 2: rows = the B H W outputs
  long M = 0;
  int Co = 0, Kin = 0, taps = 1, kind = 4;
  int ldx = 0, ldy = 0;
  long g_elems() const { return (long)Co * taps * Kin; }
};
// depth: wgrad_depth of the launch's plan (un_wgrad_rows_per_slice, un_wgrad_slices)
inline gck::Reference wgrad_ref(const WgradGeo& q, const float* dy, const float* x, int depth) {
  gck::Reference r;
  const long n = q.g_elems();
  r.c.assign((size_t)n, 0.0);
  r.bound.assign((size_t)n, 0.0);
  Gather g;
  if (q.src == 1) g = make_gather(0, q.B, q.H, q.W, q.C);
  if (q.src == 2) g = make_gather(2, q.B, q.H / 2, q.W / 2, q.C);
  const int K = q.taps * q.Kin;
  // by output column k (threads over k): every (co, k) sum runs over the rows in order
  gck::par_rows(K, [&](long k0, long k1) {
    for (long k = k0; k < k1; ++k) {
      const int tap = (int)(k / q.Kin), c = (int)(k % q.Kin);
      std::vector<double> s(q.Co, 0.0), sa(q.Co, 0.0);
      for (long m = 0; m < q.M; ++m) {
        double cv;
        if (q.src == 0) {
          cv = x[m * q.ldx + k];
        } else {
          const int ox = (int)(m % g.Wo), oy = (int)((m / g.Wo) % g.Ho), b = (int)(m / ((long)g.Wo * g.Ho));
          int iy, ix;
          if (!tap_at(g, oy, ox, tap / 3, tap % 3, &iy, &ix)) continue;
          cv = x[(((long)b * g.H + iy) * g.W + ix) * g.C + c];
        }
        for (int co = 0; co < q.Co; ++co) {
          const double t = (double)dy[m * q.ldy + co] * cv;
          s[co] += t;
          sa[co] += std::fabs(t);
        }
      }
      for (int co = 0; co < q.Co; ++co) {
        const long dst = q.kind == 2 ? ((long)tap * q.Co + co) * q.Kin + c : ((long)tap * q.Kin + c) * q.Co + co;
        r.c[dst] = s[co];
        r.bound[dst] = (depth + 16) * kEps24 * sa[co];
      }
    }
  });
  return r;
}

// ---- helpers -------------------------------------------------------------------------------------
// max over elements of |a - b| / (2 bound): two device results that each lie within the bound of the
// same reference
inline double pair_ratio(const gck::Reference& r, const float* a, const float* b, long n) {
  double q = 0.0;
  for (long i = 0; i < n; ++i) {
    const double d = std::fabs((double)a[i] - (double)b[i]), bd = 2.0 * r.bound[i];
    q = std::max(q, bd > 0.0 ? d / bd : (d == 0.0 ? 0.0 : (double)INFINITY));
  }
  return q;
}
inline long count_diff_bits(const float* a, const float* b, long n) {
  long d = 0;
  for (long i = 0; i < n; ++i) d += gck::f2u(a[i]) != gck::f2u(b[i]);
  return d;
}

}  // namespace c3k
