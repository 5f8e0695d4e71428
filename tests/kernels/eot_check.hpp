// eot_check.hpp — host side of the EOT patch pipeline's kernel parity checker (kernels_eot.hip: placement
// and its lists, the brightness matcher, the banded resize, the compositor, the rotation gradient, the
// resize adjoint, the patch gradient, TV).  No HIP call is made here.
//
// One body of code states every operation once, templated on the number type:
//   T = float  the fp32 restatement in the kernels' own operation order (FP contraction off, as the kernel
//              file is built): the CPU stand-in of eot_teeth, and the exact reference of what is made of IEEE
//              basic operations alone (the placement's integers and lists, the spans, the resize in "exact
//              mode").  It takes seeded faults.
//   T = E      the fp64 reference: every value carries a running bound of the error an fp32 evaluation of the
//              same expression can have (u = 2^-24 per rounding, propagated to first order through sums and
//              products: a length-n sum comes out as (n + c) u sum|w x|).  DESIGN.md, "EOT kernel parity".
// A stage's reference is computed from what the device wrote in the stages before it, so each stage is judged
// on its own.  Outputs that hinge on a comparison are compared against both outcomes when the deciding
// quantity lies within twice its own error bound of the threshold (the decision allowance); the share of such
// elements is reported.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "common.hpp"  // philox4x32_10, u01, u01_open0 (host-callable), the RNG streams
#include "gemm_check.hpp"
#include "post.hpp"

#pragma clang fp contract(off)

namespace eck {
using namespace phx;

constexpr double kU = 5.9604644775390625e-8;  // 2^-24: one fp32 rounding, relative
constexpr double kTiny = 1.1754943508222875e-38;  // the smallest normal fp32: the floor of every bound
constexpr uint32_t kFillWord = gck::kUnwritten;  // "never written": a NaN no kernel produces
constexpr int kFillInt = (int)0xCBCBCBCB;
// output rows per resize work item, as eot_plan_info().rows_per_tile says (eot_parity --plan prints that value and
// tests/test_eot_parity_host.py holds it to this one; eot_teeth does not link the library)
constexpr int kRowsPerTile = 4;

// ---- E: an fp64 value with the running error bound of its fp32 evaluation ---------------------------------
struct E {
  double v = 0, e = 0;
  E() = default;
  E(double v_, double e_ = 0) : v(v_), e(e_) {}
};
inline E rnd(double v, double ep) { return E(v, ep + kU * (std::fabs(v) + ep)); }
inline E operator+(E a, E b) { return rnd(a.v + b.v, a.e + b.e); }
inline E operator-(E a, E b) { return rnd(a.v - b.v, a.e + b.e); }
inline E operator*(E a, E b) { return rnd(a.v * b.v, std::fabs(a.v) * b.e + std::fabs(b.v) * a.e + a.e * b.e); }
inline E operator-(E a) { return E(-a.v, a.e); }
inline E& operator+=(E& a, E b) { a = a + b; return a; }
inline E& operator-=(E& a, E b) { a = a - b; return a; }

inline float tmin(float a, float b) { return fminf(a, b); }
inline float tmax(float a, float b) { return fmaxf(a, b); }
// min / max are 1-Lipschitz in both arguments; where the two cannot cross, the result is the winner itself (a
// clamp deep in saturation returns its exact limit)
inline E tmin(E a, E b) {
  if (b.v - a.v > a.e + b.e) return a;
  if (a.v - b.v > a.e + b.e) return b;
  return E(std::min(a.v, b.v), std::max(a.e, b.e));
}
inline E tmax(E a, E b) {
  if (a.v - b.v > a.e + b.e) return a;
  if (b.v - a.v > a.e + b.e) return b;
  return E(std::max(a.v, b.v), std::max(a.e, b.e));
}
inline float tabs(float a) { return fabsf(a); }
inline E tabs(E a) { return E(std::fabs(a.v), a.e); }
inline double val(float a) { return a; }
inline double val(E a) { return a.v; }
template <class T> T clampT(T x, float lo, float hi) { return tmin(tmax(x, T(lo)), T(hi)); }

// the gates of one element: a decision whose quantity lies within 2 e of its threshold is ambiguous, numbered
// in evaluation order, and taken the other way when its bit of `flip` is set
struct Gates {
  unsigned flip = 0;
  int n = 0;
};
inline bool gate_ge(Gates&, float q, float thr) { return q >= thr; }
inline bool gate_le(Gates&, float q, float thr) { return q <= thr; }
inline bool gate_lt(Gates&, float q, float thr) { return q < thr; }
inline bool amb(Gates& g, E q, double thr, bool nominal) {
  if (q.e > 0 && std::fabs(q.v - thr) <= 2 * q.e) {
    const int k = g.n++;
    return nominal ^ (k < 32 && ((g.flip >> k) & 1u));
  }
  return nominal;
}
inline bool gate_ge(Gates& g, E q, float thr) { return amb(g, q, thr, q.v >= thr); }
inline bool gate_le(Gates& g, E q, float thr) { return amb(g, q, thr, q.v <= thr); }
inline bool gate_lt(Gates& g, E q, float thr) { return amb(g, q, thr, q.v < thr); }

// ---- seeded faults of the stand-in ------------------------------------------------------------------------
enum Fault {
  F_NONE = 0, F_ADJ_NARROW, F_OWNER_FIRST, F_FILL_LE, F_RAGGED_TILE, F_BAND_SKIP, F_INV_TRANSPOSED, F_NO_NOISE,
  F_DELTA_FIRST, F_GATE_STRICT, F_TV_LAST_ROW, F_NO_MEAN_DYC, F_IMG_FIRST
};

// ---- a case -----------------------------------------------------------------------------------------------
enum Layout { L_RANDOM = 0, L_CORNERS, L_CLUSTER, L_GRID };
enum Refuse { R_NONE = 0, R_PLACE_129, R_COMPOSITE_101, R_RESIZE_BWD_101 };
struct Case {
  std::string name;
  int B = 1, H = 64, W = 64, maxb = 4, P = 24;
  std::vector<int> counts;      // boxes per image (B entries)
  std::vector<int> ps;          // target patch sides, cycled over the boxes in slot order
  int layout = L_RANDOM;
  int defender = 0;             // PlaceRule of the defender's Masker (tolerance 0.5, scale U(0.3, 0.5) per box)
  float scale = 0.4f;           // params[NPATCH] under the attacker's rule
  int span_stride = 0;          // 0: the largest ps rounded up to 4
  int apply_print = 1, batch = 0;  // launch_eot_match's apply_print; batch: launch_eot_match_batch
  int clipw = 0;                // the harness's own ImgParams with w around 1.5 (the print clip bites)
  float amp = 0.01f;            // resize noise amplitude
  float img_amp = 1.0f;         // images uniform in [-img_amp, img_amp]
  int add_tv = 1, add_loss = 1;
  int plant = 0;                // exact -1 / +1 values planted in the R block the compositor and rot_bwd read
  int refuse = R_NONE;
  int place_only = 0;           // maxb beyond what composite and resize_bwd take: the placement stage alone
  uint64_t seed = 1;
  int64_t step = 3;
  int gimg0 = 0;
};

inline PlaceRule rule_of(const Case& c) {
  PlaceRule r;
  if (c.defender) { r.tol = 0.5f; r.random_scale = 1; r.scale_lo = 0.3f; r.scale_hi = 0.5f; }
  return r;
}

// ---- the RNG helpers as the kernel file has them ----------------------------------------------------------
inline u32x4 rng(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, int64_t step, uint32_t stream) {
  return philox4x32_10(u32x4{c0, c1, c2, (uint32_t)((uint64_t)step << 8) | stream}, (uint32_t)seed, (uint32_t)(seed >> 32));
}
inline float runif(uint32_t v, float lo, float hi) { return u01(v) * (hi - lo) + lo; }
inline float rnorm32(uint32_t a, uint32_t b, float mean, float sd) {
  float u1 = u01_open0(a), u2 = u01(b);
  float z = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
  return z * sd + mean;
}
// fp64 with the bound: logf, cosf within 3 and 4 u, sqrtf correctly rounded
inline E rnorm64(uint32_t a, uint32_t b, float mean, float sd) {
  const double u1 = u01_open0(a), u2 = u01(b);
  const double l = std::log(u1);
  const E ln(l, 3 * kU * std::fabs(l));
  const E m2 = E(-2.0) * ln;
  const double sq = std::sqrt(m2.v);
  const E s(sq, (sq > 0 ? 0.5 * m2.e / sq : std::sqrt(m2.e)) + kU * sq);
  const E arg = E((double)6.28318530717958647692f) * E(u2);
  const E c(std::cos(arg.v), arg.e + 4 * kU);
  return (s * c) * E(sd) + E(mean);
}

// ---- the place block: B * maxb BoxPlace, then the lists ----------------------------------------------------
struct Lists {
  int *nvalid, *total_chunks, *img_n, *img_first, *vlist, *cprefix, *tprefix, *bcnt, *bvpre;
  long nints;
};
inline Lists lists_at(int* l, int B, int maxb) {
  const long n = (long)B * maxb;
  Lists v;
  v.nvalid = l; v.total_chunks = l + 1; v.img_n = l + 2; v.img_first = v.img_n + B; v.vlist = v.img_first + B;
  v.cprefix = v.vlist + n; v.tprefix = v.cprefix + n + 1; v.bcnt = v.tprefix + n + 1; v.bvpre = v.bcnt + 8 * B;
  v.nints = (v.bvpre + 8 * n) - l;
  return v;
}
struct PlaceBlock {
  int B = 0, maxb = 0;
  std::vector<uint8_t> bytes;  // eot_place_bytes(B, maxb)
  void init(int B_, int maxb_) {
    B = B_; maxb = maxb_;
    bytes.assign(eot_place_bytes(B, maxb), gck::kGuardByte);
  }
  long nslot() const { return (long)B * maxb; }
  BoxPlace* place() { return reinterpret_cast<BoxPlace*>(bytes.data()); }
  const BoxPlace* place() const { return reinterpret_cast<const BoxPlace*>(bytes.data()); }
  Lists lists() const {
    return lists_at(reinterpret_cast<int*>(const_cast<uint8_t*>(bytes.data()) + nslot() * sizeof(BoxPlace)), B, maxb);
  }
};

// ---- placement, fp32 (k_eot_place, k_eot_bands) -----------------------------------------------------------
// margin (optional): the smallest distance to an integer of a quantity the placement truncates (longer *
// scale, diag, yp, xp); a value a clamp set exactly (0, or H - diag with an integral diag) is exempt
struct PlaceOpt {
  Fault f = F_NONE;
  double* margin = nullptr;
};
inline void note_margin(double* m, float x, bool exempt) {
  if (!m || exempt) return;
  const double d = std::fabs((double)x - std::nearbyint((double)x));
  *m = std::min(*m, d);
}
inline BoxPlace place_one(const EotDims& d, const float* bx, int k, int gimg, float scale, uint64_t seed, int64_t step,
                          const PlaceRule& rule, PlaceOpt o) {
  BoxPlace P{};
  const float Hf = (float)d.H, Wf = (float)d.W;
  const float ymin = bx[0], xmin = bx[1], ymax = bx[2], xmax = bx[3];
  const float h = ymax - ymin, w = xmax - xmin;
  const float longer = fmaxf(h, w);
  u32x4 r = rng(seed, 0, (uint32_t)k, (uint32_t)gimg, step, RNG_PLACE);
  const float bscale = rule.random_scale ? runif(r.z, rule.scale_lo, rule.scale_hi) : scale;
  const float psraw = longer * bscale;
  const float psf = floorf(psraw);
  const float draw = 1.41421354f * psf;
  const float diag = fminf(draw, Wf);
  const float tol = rule.tol;
  const float oy = (ymin + h / 2.0f) + runif(r.x, (-tol * h) / 2.0f, (tol * h) / 2.0f);
  const float ox = (xmin + w / 2.0f) + runif(r.y, (-tol * w) / 2.0f, (tol * w) / 2.0f);
  float yp = fmaxf(oy - diag / 2.0f, 0.0f);
  float xp = fmaxf(ox - diag / 2.0f, 0.0f);
  bool ycl = yp == 0.0f, xcl = xp == 0.0f;
  if (yp + diag > Hf) { yp = Hf - diag; ycl = diag == floorf(diag); }
  if (xp + diag > Wf) { xp = Wf - diag; xcl = diag == floorf(diag); }
  note_margin(o.margin, psraw, false);
  note_margin(o.margin, diag, draw >= Wf);
  note_margin(o.margin, yp, ycl);
  note_margin(o.margin, xp, xcl);
  P.ymin = (int)yp;
  P.xmin = (int)xp;
  P.ps = (int)psf;
  P.diag = (int)diag;
  P.valid = (psf * psf > 4.0f) && P.ps <= d.span_stride ? 1 : 0;
  P.pad = (P.diag - P.ps) >= 0 ? (P.diag - P.ps) / 2 : -(((P.ps - P.diag) + 1) / 2);
  u32x4 q = rng(seed, 1, (uint32_t)k, (uint32_t)gimg, step, RNG_BOX);
  P.delta = runif(q.x, -0.3f, 0.3f);
  const float amax = 0.34906584f;
  P.angle = runif(q.y, -amax, amax);
  const float side = (float)P.diag;
  const float c = cosf(P.angle), s = sinf(P.angle);
  const float xo = ((side - 1.0f) - (c * (side - 1.0f) - s * (side - 1.0f))) / 2.0f;
  const float yo = ((side - 1.0f) - (s * (side - 1.0f) + c * (side - 1.0f))) / 2.0f;
  P.fwd[0] = c; P.fwd[1] = -s; P.fwd[2] = xo;
  P.fwd[3] = s; P.fwd[4] = c; P.fwd[5] = yo;
  double a = c, bb = -s, tx = xo, dd = s, e = c, ty = yo;
  double det = a * e - bb * dd;
  P.inv[0] = (float)(e / det);
  P.inv[1] = (float)(-bb / det);
  P.inv[2] = (float)((bb * ty - e * tx) / det);
  P.inv[3] = (float)(-dd / det);
  P.inv[4] = (float)(a / det);
  P.inv[5] = (float)((dd * tx - a * ty) / det);
  if (o.f == F_INV_TRANSPOSED) { std::swap(P.inv[1], P.inv[3]); }
  return P;
}

// tf_span, restated (span.hpp)
inline SpanEntry span_of(int i, int ps, int in_size) {
  const float scale = (float)ps / (float)in_size;
  const float inv_scale = (float)(1.0 / (double)scale);
  const float kscale = fmaxf(inv_scale, 1.0f);
  const float one_over_k = 1.0f / kscale;
  const float sample_f = ((float)i + 0.5f) * inv_scale + (-inv_scale * 0.0f);
  long start = (long)ceilf(sample_f - 1.0f * kscale - 0.5f);
  long end = (long)floorf(sample_f + 1.0f * kscale - 0.5f);
  start = start < 0 ? 0 : (start > in_size - 1 ? in_size - 1 : start);
  end = (end < 0 ? 0 : (end > in_size - 1 ? in_size - 1 : end)) + 1;
  float total = 0.0f;
  for (long src = start; src < end; ++src) {
    float pos = (float)src + 0.5f - sample_f;
    float x = fabsf(pos * one_over_k);
    total += x < 1.0f ? 1.0f - x : 0.0f;
  }
  SpanEntry o;
  o.start = (int)start;
  o.end = (int)end;
  o.inv_total = fabsf(total) >= 1000.0f * 1.17549435e-38f ? 1.0f / total : 0.0f;
  o.sample_f = sample_f;
  return o;
}
inline float one_over_k_of(int ps, int P) {
  const float scale = (float)ps / (float)P;
  const float inv_scale = (float)(1.0 / (double)scale);
  return 1.0f / fmaxf(inv_scale, 1.0f);
}
inline float span_weight(const SpanEntry& sp, int src, float one_over_k, float) {
  float pos = (float)src + 0.5f - sp.sample_f;
  float x = fabsf(pos * one_over_k);
  float w = x < 1.0f ? 1.0f - x : 0.0f;
  return w * sp.inv_total;
}
// (src + 0.5 is exact; the hat is continuous at |x| = 1, so its branch needs no allowance)
inline E span_weight(const SpanEntry& sp, int src, float one_over_k, E) {
  E pos = E((double)src + 0.5) - E(sp.sample_f);
  E x = tabs(pos * E(one_over_k));
  E w = x.v < 1.0 ? E(1.0) - x : E(0.0, std::max(0.0, x.e - (x.v - 1.0)));
  return w * E(sp.inv_total);
}

struct PlaceOut {
  std::vector<ImgParams> img;
  PlaceBlock pb;
  std::vector<SpanEntry> spans;  // [B*maxb][span_stride]; unwritten entries keep the fill
};
inline void fill_spans(std::vector<SpanEntry>& s, size_t n) {
  SpanEntry f;
  std::memset(&f, gck::kGuardByte, sizeof f);
  s.assign(n, f);
}
inline PlaceOut sim_place(const EotDims& d, const std::vector<float>& boxes, const std::vector<int>& count, float scale,
                          uint64_t seed, int64_t step, int gimg0, const PlaceRule& rule, PlaceOpt o = PlaceOpt{}) {
  PlaceOut out;
  out.img.resize(d.B);
  for (int b = 0; b < d.B; ++b) {
    u32x4 r = rng(seed, 0, 0, (uint32_t)(gimg0 + b), step, RNG_PRINT);
    u32x4 r2 = rng(seed, 1, 0, (uint32_t)(gimg0 + b), step, RNG_PRINT);
    u32x4 r3 = rng(seed, 2, 0, (uint32_t)(gimg0 + b), step, RNG_PRINT);
    ImgParams p;
    p.w[0] = rnorm32(r.x, r.y, 0.5f, 0.1f);
    p.w[1] = rnorm32(r.z, r.w, 0.5f, 0.1f);
    p.w[2] = rnorm32(r2.x, r2.y, 0.5f, 0.1f);
    p.b[0] = rnorm32(r2.z, r2.w, 0.0f, 0.01f);
    p.b[1] = rnorm32(r3.x, r3.y, 0.0f, 0.01f);
    p.b[2] = rnorm32(r3.z, r3.w, 0.0f, 0.01f);
    out.img[b] = p;
  }
  out.pb.init(d.B, d.maxb);
  const long nslot = out.pb.nslot();
  BoxPlace* place = out.pb.place();
  for (long sl = 0; sl < nslot; ++sl) {
    const int b = (int)(sl / d.maxb), k = (int)(sl % d.maxb);
    BoxPlace P{};
    if (k < count[b]) P = place_one(d, &boxes[sl * 4], k, gimg0 + b, scale, seed, step, rule, o);
    place[sl] = P;
  }
  Lists L = out.pb.lists();
  long run_off = 0;
  int run_ch = 0, run_v = 0, run_tl = 0;
  for (long sl = 0; sl < nslot; ++sl) {
    if (sl % d.maxb == 0) L.img_first[sl / d.maxb] = run_v;
    if (!place[sl].valid) continue;
    const int ps = place[sl].ps;
    place[sl].roff = run_off;
    L.vlist[run_v] = (int)sl;
    L.cprefix[run_v] = run_ch;
    L.tprefix[run_v] = run_tl;
    run_off += (long)ps * ps * 3;
    run_ch += (ps * ps + 255) / 256;
    run_tl += (ps + kRowsPerTile - 1) / kRowsPerTile;
    run_v += 1;
  }
  *L.nvalid = run_v;
  *L.total_chunks = run_ch;
  L.cprefix[run_v] = run_ch;
  L.tprefix[run_v] = run_tl;
  if (o.f == F_IMG_FIRST)
    for (int b = 1; b < d.B; ++b)
      if (L.img_first[b] == L.img_first[b - 1]) { L.img_first[b] += 1; break; }
  for (int b = 0; b < d.B; ++b) L.img_n[b] = (b + 1 < d.B ? L.img_first[b + 1] : run_v) - L.img_first[b];
  fill_spans(out.spans, (size_t)nslot * d.span_stride);
  for (long sl = 0; sl < nslot; ++sl)
    if (place[sl].valid)
      for (int i = 0; i < place[sl].ps; ++i) out.spans[sl * d.span_stride + i] = span_of(i, place[sl].ps, d.P);
  // k_eot_bands
  for (int b = 0; b < d.B; ++b)
    for (int x = 0; x < 8; ++x) {
      int acc = 0;
      const int n = std::max(0, std::min(L.img_n[b], d.maxb));
      for (int j = 0; j < n; ++j) {
        const int v = L.img_first[b] + j;
        if (v < 0 || v >= run_v) break;
        L.bvpre[x * nslot + v] = acc;
        acc += EotPlanInfo::band_tiles(place[L.vlist[v]].ps, x, kRowsPerTile);
      }
      L.bcnt[x * d.B + b] = acc;
    }
  return out;
}

// ---- the brightness matcher -------------------------------------------------------------------------------
constexpr float kTo01 = 127.0f / 255.0f;
constexpr float kBack = 255.0f / 127.0f;
template <class T> struct Yuv { T y, u, v; };
template <class T> Yuv<T> rgb2yuv(T r, T g, T b) {
  Yuv<T> o;
  o.y = r * T(0.299f) + g * T(0.587f) + b * T(0.114f);
  o.u = r * T(-0.14714119f) + g * T(-0.28886916f) + b * T(0.43601035f);
  o.v = r * T(0.61497538f) + g * T(-0.51496512f) + b * T(-0.10001026f);
  return o;
}
template <class T> T print_px(float x, const ImgParams& p, int c, bool apply) {
  if (!apply) return T(x);
  T v = T(p.w[c]) * T(x) + T(p.b[c]);
  return clampT(v, -1.0f, 1.0f);
}
template <class T> void match_px(T p0, T p1, T p2, T mus, T mut, T* o) {
  Yuv<T> s = rgb2yuv((p0 + T(1.0f)) * T(kTo01), (p1 + T(1.0f)) * T(kTo01), (p2 + T(1.0f)) * T(kTo01));
  T yc = (s.y - mus) + mut;
  T yp = clampT(yc, 0.0f, 1.0f);
  T r = yp + T(1.13988303f) * s.v;
  T g = yp + T(-0.394642334f) * s.u + T(-0.58062185f) * s.v;
  T bl = yp + T(2.03206185f) * s.u;
  o[0] = clampT(r, 0.0f, 1.0f) * T(kBack) - T(1.0f);
  o[1] = clampT(g, 0.0f, 1.0f) * T(kBack) - T(1.0f);
  o[2] = clampT(bl, 0.0f, 1.0f) * T(kBack) - T(1.0f);
}
// the Y means: fp32 values summed in fp64 (per lane in grid-stride order, a 256-lane tree, 64 partials in
// order); in fp64 the order does not show.  depth: the additions on one value's path (the fp64 sum's bound)
template <class T> T ymean_of(const float* base, long npx, const ImgParams* p, bool apply, bool source) {
  double s = 0, se = 0, sa = 0;
  for (long i = 0; i < npx; ++i) {
    T r, g, bl;
    if (source) {
      r = (print_px<T>(base[i * 3 + 0], *p, 0, apply) + T(1.0f)) * T(kTo01);
      g = (print_px<T>(base[i * 3 + 1], *p, 1, apply) + T(1.0f)) * T(kTo01);
      bl = (print_px<T>(base[i * 3 + 2], *p, 2, apply) + T(1.0f)) * T(kTo01);
    } else {
      r = (T(base[i * 3 + 0]) + T(1.0f)) * T(kTo01);
      g = (T(base[i * 3 + 1]) + T(1.0f)) * T(kTo01);
      bl = (T(base[i * 3 + 2]) + T(1.0f)) * T(kTo01);
    }
    T y = rgb2yuv(r, g, bl).y;
    s += val(y);
    sa += std::fabs(val(y));
    if constexpr (std::is_same<T, E>::value) se += y.e;
  }
  const double m = s / (double)npx;
  if constexpr (std::is_same<T, E>::value) {
    const double depth = (double)((npx + 64 * 256 - 1) / (64 * 256)) + 8 + 64 + 1;
    return E(m, (se + depth * 1.1102230246251565e-16 * sa) / (double)npx + kU * std::fabs(m));
  } else {
    return (float)m;
  }
}
struct MatchIn {
  EotDims d;
  const float* src;     // apply_print && !batch: one patch [P,P,3]; else [B,P,P,3]
  long stride;          // 0 or P*P*3
  const ImgParams* img;
  const float* tgt;     // [B,H,W,3]
  bool apply;
};
template <class T> void ymean_all(const MatchIn& m, std::vector<T>& ymean) {
  ymean.resize((size_t)m.d.B * 2);
  for (int b = 0; b < m.d.B; ++b) {
    ymean[b * 2] = ymean_of<T>(m.src + b * m.stride, (long)m.d.P * m.d.P, &m.img[b], m.apply, true);
    ymean[b * 2 + 1] = ymean_of<T>(m.tgt + (long)b * m.d.H * m.d.W * 3, (long)m.d.H * m.d.W, nullptr, false, false);
  }
}
template <class T> void match_all(const MatchIn& m, const float* ymean, std::vector<T>& out) {
  const long npx = (long)m.d.P * m.d.P;
  out.resize((size_t)m.d.B * npx * 3);
  for (int b = 0; b < m.d.B; ++b)
    for (long i = 0; i < npx; ++i) {
      const float* base = m.src + b * m.stride;
      match_px<T>(print_px<T>(base[i * 3], m.img[b], 0, m.apply), print_px<T>(base[i * 3 + 1], m.img[b], 1, m.apply),
                  print_px<T>(base[i * 3 + 2], m.img[b], 2, m.apply), T(ymean[b * 2]), T(ymean[b * 2 + 1]),
                  &out[((size_t)b * npx + i) * 3]);
    }
}

// ---- the banded resize (k_eot_resize) ---------------------------------------------------------------------
template <class T> T unwritten();
template <> inline float unwritten<float>() { return gck::u2f(kFillWord); }
template <> inline E unwritten<E>() { return E(std::nan(""), 0); }

inline long r_total(const EotDims& d, const PlaceBlock& pb) {
  const BoxPlace* place = pb.place();
  long t = 0;
  for (long sl = 0; sl < pb.nslot(); ++sl)
    if (place[sl].valid) t = std::max(t, place[sl].roff + (long)place[sl].ps * place[sl].ps * 3);
  (void)d;
  return t;
}
// rows i0 .. i0 + ni - 1 of one box: the vertical pass over the box's columns, then the horizontal one
template <class T>
void resize_tile(const EotDims& d, const float* m, const BoxPlace& P, const SpanEntry* sp, int b, int k, int i0, int ni,
                 uint64_t seed, int64_t step, int gimg0, float amp, T* rstore, Fault f) {
  const float one_over_k = one_over_k_of(P.ps, d.P);
  const int xlo = sp[0].start, nx = sp[P.ps - 1].end - xlo;
  std::vector<T> V((size_t)ni * nx * 3);
  for (int ii = 0; ii < ni; ++ii) {
    const SpanEntry si = sp[i0 + ii];
    for (int x = 0; x < nx; ++x) {
      T a0 = T(0.f), a1 = T(0.f), a2 = T(0.f);
      for (int y = si.start; y < si.end; ++y) {
        const T wy = span_weight(si, y, one_over_k, T());
        const float* q = m + ((long)y * d.P + xlo + x) * 3;
        a0 += wy * T(q[0]);
        a1 += wy * T(q[1]);
        a2 += wy * T(q[2]);
      }
      T* o = &V[((size_t)ii * nx + x) * 3];
      o[0] = a0; o[1] = a1; o[2] = a2;
    }
  }
  for (int ii = 0; ii < ni; ++ii)
    for (int j = 0; j < P.ps; ++j) {
      const SpanEntry sj = sp[j];
      T a[3] = {T(0.f), T(0.f), T(0.f)};
      for (int x = sj.start; x < sj.end; ++x) {
        const T wx = span_weight(sj, x, one_over_k, T());
        const T* row = &V[((size_t)ii * nx + (x - xlo)) * 3];
        a[0] += wx * row[0];
        a[1] += wx * row[1];
        a[2] += wx * row[2];
      }
      const int px = (i0 + ii) * P.ps + j;
      u32x4 r = rng(seed, (uint32_t)px, (uint32_t)k, (uint32_t)(gimg0 + b), step, RNG_NOISE);
      const uint32_t rr[3] = {r.x, r.y, r.z};
      T* o = rstore + P.roff + (long)px * 3;
      for (int c = 0; c < 3; ++c) {
        const float n = f == F_NO_NOISE ? 0.0f : runif(rr[c], -amp, amp);
        o[c] = f == F_DELTA_FIRST ? (a[c] + T(P.delta)) + T(n) : (a[c] + T(n)) + T(P.delta);
      }
    }
}
template <class T>
void resize_all(const EotDims& d, const float* matched, const PlaceBlock& pb, const SpanEntry* spans, uint64_t seed,
                int64_t step, int gimg0, float amp, std::vector<T>& rstore, Fault f = F_NONE) {
  rstore.assign((size_t)std::max(r_total(d, pb), 4L), unwritten<T>());
  const BoxPlace* place = pb.place();
  const Lists L = pb.lists();
  for (int xb = 0; xb < 8; ++xb) {
    if (f == F_BAND_SKIP && xb == 5) continue;
    for (int b = 0; b < d.B; ++b)
      for (int q = 0; q < L.img_n[b]; ++q) {
        const int sl = L.vlist[L.img_first[b] + q];
        const BoxPlace& P = place[sl];
        const int nt = (P.ps + kRowsPerTile - 1) / kRowsPerTile;
        const int t0 = EotPlanInfo::band_first(P.ps, xb, kRowsPerTile);
        for (int t = t0; t < t0 + EotPlanInfo::band_tiles(P.ps, xb, kRowsPerTile); ++t) {
          const int i0 = t * kRowsPerTile, ni = std::min(kRowsPerTile, P.ps - i0);
          if (f == F_RAGGED_TILE && ni < kRowsPerTile) continue;
          resize_tile<T>(d, matched + (long)b * d.P * d.P * 3, P, spans + (long)sl * d.span_stride, b, sl % d.maxb, i0, ni,
                         seed, step, gimg0, amp, rstore.data(), f);
        }
      }
  }
}

// ---- the compositor ---------------------------------------------------------------------------------------
// TF's bilinear sample in the kernel's order.  a + b == 1 exactly in fp32 (x_ceil - x and x - x_floor are exact
// for |x| >= 1 by Sterbenz; inside (-1, 1) one of them is exact and the other rounds by at most 2^-25, which
// the sum absorbs), so four equal taps t with t a power of two or zero come out as t exactly: no bound, no
// allowance.  Where a coordinate lies within its own error of an integer the fp32 evaluation may have taken the
// neighbouring cell; the sample is continuous and piecewise linear, so that costs at most e * 2 tmax more.
template <class Read> float bilinear(float x, float y, float, Read rd) {
  const float y_floor = floorf(y), x_floor = floorf(x);
  const float y_ceil = y_floor + 1.0f, x_ceil = x_floor + 1.0f;
  const int yf = (int)y_floor, xf = (int)x_floor, yc = (int)y_ceil, xc = (int)x_ceil;
  const float v_yf = (x_ceil - x) * rd(yf, xf) + (x - x_floor) * rd(yf, xc);
  const float v_yc = (x_ceil - x) * rd(yc, xf) + (x - x_floor) * rd(yc, xc);
  return (y_ceil - y) * v_yf + (y - y_floor) * v_yc;
}
template <class Read> E bilinear(E x, E y, double tmax_, Read rd) {
  const double yfl = std::floor(y.v), xfl = std::floor(x.v);
  const int yf = (int)yfl, xf = (int)xfl, yc = yf + 1, xc = xf + 1;
  const double t00 = rd(yf, xf), t01 = rd(yf, xc), t10 = rd(yc, xf), t11 = rd(yc, xc);
  double extra = 0;
  if (std::min(x.v - xfl, xfl + 1 - x.v) <= x.e) extra += 2 * tmax_ * x.e;
  if (std::min(y.v - yfl, yfl + 1 - y.v) <= y.e) extra += 2 * tmax_ * y.e;
  if (t00 == t01 && t00 == t10 && t00 == t11) {
    int ex;
    const bool pow2 = t00 == 0 || std::frexp(std::fabs(t00), &ex) == 0.5;
    return E(t00, (pow2 ? 0.0 : 3 * kU * std::fabs(t00)) + extra);
  }
  const E a = E(xfl + 1) - x, b = x - E(xfl);
  const E v_yf = a * E(t00) + b * E(t01);
  const E v_yc = a * E(t10) + b * E(t11);
  E r = (E(yfl + 1) - y) * v_yf + (y - E(yfl)) * v_yc;
  r.e += extra;
  return r;
}
inline double rread(const float* R, const BoxPlace& P, int yy, int xx, int c) {
  int ry = yy - P.pad, rx = xx - P.pad;
  if (yy < 0 || yy >= P.diag || xx < 0 || xx >= P.diag) return -2.0;
  if (ry < 0 || ry >= P.ps || rx < 0 || rx >= P.ps) return -2.0;
  float v = R[((long)ry * P.ps + rx) * 3 + c];
  return fminf(fmaxf(v, -1.0f), 1.0f);
}
template <class T> struct Px { T v; int own; bool covered; };
// what the fold met, for --plan: a later box's fill over a pixel an earlier box owns (the earlier paste stays)
struct FoldStats { long fill_over_owned = 0; };
// one pixel-channel's fold over the boxes of its image, in paste order
template <class T>
Px<T> composite_px(const EotDims& d, const PlaceBlock& pb, const float* rstore, int b, int y, int x, int c, float in, Gates& g,
                   Fault f = F_NONE, FoldStats* st = nullptr) {
  const BoxPlace* place = pb.place();
  const Lists L = pb.lists();
  Px<T> o{T(in), -1, false};
  for (int q = 0; q < L.img_n[b]; ++q) {
    const int sl = L.vlist[L.img_first[b] + q];
    const BoxPlace& P = place[sl];
    const int qy = y - P.ymin, qx = x - P.xmin;
    if (qy < 0 || qy >= P.diag || qx < 0 || qx >= P.diag) continue;
    o.covered = true;
    const T ox = T((float)qx), oy = T((float)qy);
    T inx = T(P.fwd[0]) * ox + T(P.fwd[1]) * oy + T(P.fwd[2]);
    T iny = T(P.fwd[3]) * ox + T(P.fwd[4]) * oy + T(P.fwd[5]);
    const float* R = rstore + P.roff;
    T r;
    if constexpr (std::is_same<T, E>::value)
      r = bilinear(inx, iny, 2.0, [&](int yy, int xx) { return rread(R, P, yy, xx, c); });
    else
      r = bilinear(inx / 1.0f, iny / 1.0f, 0.f, [&](int yy, int xx) { return (float)rread(R, P, yy, xx, c); });
    const bool fill = f == F_FILL_LE ? gate_le(g, r, -1.0f) : gate_lt(g, r, -1.0f);
    if (fill) {
      if (st && o.own >= 0) st->fill_over_owned++;
      o.v = clampT(o.v, -1.0f, 1.0f);
    } else {
      if (f == F_OWNER_FIRST && o.own >= 0) { o.v = clampT(o.v, -1.0f, 1.0f); continue; }
      o.v = clampT(r, -1.0f, 1.0f);
      o.own = sl % d.maxb;
    }
  }
  return o;
}

// ---- the rotation gradient --------------------------------------------------------------------------------
template <class T>
void rot_bwd_all(const EotDims& d, const float* dimg, const int16_t* owner, const PlaceBlock& pb, const float* rstore,
                 double gmax, std::vector<T>& dstore, Fault f = F_NONE) {
  dstore.assign((size_t)std::max(r_total(d, pb), 4L), unwritten<T>());
  const BoxPlace* place = pb.place();
  const Lists L = pb.lists();
  for (int v = 0; v < *L.nvalid; ++v) {
    const int sl = L.vlist[v];
    const BoxPlace& P = place[sl];
    const int b = sl / d.maxb, k = sl % d.maxb;
    for (int px = 0; px < P.ps * P.ps; ++px) {
      const int i = px / P.ps, j = px % P.ps;
      const T ox = T((float)(j + P.pad)), oy = T((float)(i + P.pad));
      T inx = T(P.inv[0]) * ox + T(P.inv[1]) * oy + T(P.inv[2]);
      T iny = T(P.inv[3]) * ox + T(P.inv[4]) * oy + T(P.inv[5]);
      for (int c = 0; c < 3; ++c) {
        auto tap = [&](int yy, int xx) -> double {
          if (yy < 0 || yy >= P.diag || xx < 0 || xx >= P.diag) return 0.0;
          long e = (((long)b * d.H + (P.ymin + yy)) * d.W + (P.xmin + xx)) * 3 + c;
          return owner[e] == k ? (double)dimg[e] : 0.0;
        };
        T gv;
        if constexpr (std::is_same<T, E>::value) gv = bilinear(inx, iny, gmax, tap);
        else gv = bilinear(inx / 1.0f, iny / 1.0f, 0.f, [&](int yy, int xx) { return (float)tap(yy, xx); });
        const float pre = rstore[P.roff + (long)px * 3 + c];
        const bool open = f == F_GATE_STRICT ? (pre > -1.0f && pre < 1.0f) : (pre >= -1.0f && pre <= 1.0f);
        dstore[P.roff + (long)px * 3 + c] = open ? gv : T(0.0f);
      }
    }
  }
}

// ---- the resize adjoint -----------------------------------------------------------------------------------
// adj_range as the kernel has it (fp32)
inline void adj_range(int src, float inv_scale, float ks, int ps, int* lo, int* hi) {
  *lo = std::max((int)floorf(((float)src - ks - 0.5f) / inv_scale - 0.5f) - 1, 0);
  *hi = std::min((int)ceilf(((float)src + ks + 1.5f) / inv_scale - 0.5f) + 1, ps - 1);
}
// the output indices whose span holds each source index, from the spans themselves: [lo[s], hi[s]]
inline void tight_range(const SpanEntry* sp, int ps, int P, std::vector<int>& lo, std::vector<int>& hi) {
  lo.assign(P, ps);
  hi.assign(P, -1);
  for (int i = 0; i < ps; ++i)
    for (int s = sp[i].start; s < sp[i].end; ++s) {
      lo[s] = std::min(lo[s], i);
      hi[s] = std::max(hi[s], i);
    }
}
// the smallest slack of adj_range against the tight range over a box's source indices (>= 0: conservative)
inline int adj_slack(const SpanEntry* sp, int ps, int P) {
  std::vector<int> lo, hi;
  tight_range(sp, ps, P, lo, hi);
  const float scale = (float)ps / (float)P;
  const float inv_scale = (float)(1.0 / (double)scale);
  const float ks = fmaxf(inv_scale, 1.0f);
  int slack = 1 << 20;
  for (int s = 0; s < P; ++s) {
    if (hi[s] < 0) continue;
    int a, b;
    adj_range(s, inv_scale, ks, ps, &a, &b);
    slack = std::min(slack, std::min(lo[s] - a, b - hi[s]));
  }
  return slack;
}
inline long t_total(const EotDims& d, const PlaceBlock& pb) {
  const Lists L = pb.lists();
  return (long)L.tprefix[*L.nvalid] * 4 * d.P * 3;
}
// T = float follows the kernels (adj_range, then the containment test); T = E takes every output index whose
// span holds the source index: the transpose of the resize matrix itself
template <class T>
void resize_bwd_all(const EotDims& d, const PlaceBlock& pb, const SpanEntry* spans, const float* dstore, std::vector<T>* tstore,
                    const float* tdev, std::vector<T>& dmatched, Fault f = F_NONE) {
  const BoxPlace* place = pb.place();
  const Lists L = pb.lists();
  const long npx = (long)d.P * d.P;
  if (tstore) tstore->assign((size_t)std::max(t_total(d, pb), 4L), unwritten<T>());
  dmatched.assign((size_t)d.B * npx * 3, T(0.f));
  std::vector<int> lo, hi;
  for (int b = 0; b < d.B; ++b)
    for (int q = 0; q < L.img_n[b]; ++q) {
      const int v = L.img_first[b] + q;
      const int sl = L.vlist[v];
      const BoxPlace& P = place[sl];
      const SpanEntry* sp = spans + (long)sl * d.span_stride;
      const float scale = (float)P.ps / (float)d.P;
      const float inv_scale = (float)(1.0 / (double)scale);
      const float ks = fmaxf(inv_scale, 1.0f);
      const float one_over_k = 1.0f / ks;
      tight_range(sp, P.ps, d.P, lo, hi);
      auto range = [&](int s, int* a, int* z) {
        if constexpr (std::is_same<T, E>::value) { *a = lo[s]; *z = hi[s]; }
        else if (f == F_ADJ_NARROW) { *a = lo[s]; *z = hi[s] - 1; }
        else adj_range(s, inv_scale, ks, P.ps, a, z);
      };
      const long ub = (long)L.tprefix[v] * 4 * d.P * 3;
      // rows: U[i][x] = sum_j Wc[j,x] dR[i,j]
      if (tstore)
        for (int i = 0; i < P.ps; ++i)
          for (int x = 0; x < d.P; ++x) {
            int jlo, jhi;
            range(x, &jlo, &jhi);
            T a0 = T(0.f), a1 = T(0.f), a2 = T(0.f);
            for (int j = jlo; j <= jhi; ++j) {
              const SpanEntry sj = sp[j];
              if (x < sj.start || x >= sj.end) continue;
              const T w = span_weight(sj, x, one_over_k, T());
              const float* gq = dstore + P.roff + ((long)i * P.ps + j) * 3;
              a0 += w * T(gq[0]);
              a1 += w * T(gq[1]);
              a2 += w * T(gq[2]);
            }
            T* o = tstore->data() + ub + ((long)i * d.P + x) * 3;
            o[0] = a0; o[1] = a1; o[2] = a2;
          }
      // cols: dmatched[y,x] += sum_i Wr[i,y] U[i][x], boxes ascending, then i ascending
      for (int y = 0; y < d.P; ++y) {
        int ilo, ihi;
        range(y, &ilo, &ihi);
        for (int i = ilo; i <= ihi; ++i) {
          const SpanEntry si = sp[i];
          if (y < si.start || y >= si.end) continue;
          const T wy = span_weight(si, y, one_over_k, T());
          for (int x = 0; x < d.P; ++x)
            for (int c = 0; c < 3; ++c) {
              const long ui = ub + ((long)i * d.P + x) * 3 + c;
              T u;
              if constexpr (std::is_same<T, E>::value) u = E(tdev[ui]);
              else u = (*tstore)[ui];
              dmatched[((size_t)b * npx + (long)y * d.P + x) * 3 + c] += wy * u;
            }
        }
      }
    }
}

// ---- the patch gradient -----------------------------------------------------------------------------------
template <class T> struct MatchBwd { T dp[3]; T dyc; T dyp; bool dyc_amb; };
template <class T>
MatchBwd<T> match_bwd_px(const T* p, T mus, T mut, const float* dm, T mean_dyc, Gates& g) {
  Yuv<T> s = rgb2yuv((p[0] + T(1.0f)) * T(kTo01), (p[1] + T(1.0f)) * T(kTo01), (p[2] + T(1.0f)) * T(kTo01));
  T yc = (s.y - mus) + mut;
  T yp = clampT(yc, 0.0f, 1.0f);
  T rgb[3] = {yp + T(1.13988303f) * s.v, yp + T(-0.394642334f) * s.u + T(-0.58062185f) * s.v, yp + T(2.03206185f) * s.u};
  T drgb[3];
  const int n0 = g.n;
  for (int c = 0; c < 3; ++c) {
    const bool lo = gate_ge(g, rgb[c], 0.0f), hi = gate_le(g, rgb[c], 1.0f);  // both evaluated: the gates keep their numbers
    drgb[c] = lo && hi ? T(dm[c]) * T(kBack) : T(0.0f);
  }
  T dyp = drgb[0] + drgb[1] + drgb[2];
  T du = T(-0.394642334f) * drgb[1] + T(2.03206185f) * drgb[2];
  T dv = T(1.13988303f) * drgb[0] + T(-0.58062185f) * drgb[1];
  const bool ylo = gate_ge(g, yc, 0.0f), yhi = gate_le(g, yc, 1.0f);
  T dyc = ylo && yhi ? dyp : T(0.0f);
  T dy = dyc - mean_dyc;
  MatchBwd<T> o;
  o.dyc = dyc;
  o.dyp = dyp;
  o.dyc_amb = g.n != n0;
  o.dp[0] = (dy * T(0.299f) + du * T(-0.14714119f) + dv * T(0.61497538f)) * T(kTo01);
  o.dp[1] = (dy * T(0.587f) + du * T(-0.28886916f) + dv * T(-0.51496512f)) * T(kTo01);
  o.dp[2] = (dy * T(0.114f) + du * T(0.43601035f) + dv * T(-0.10001026f)) * T(kTo01);
  return o;
}
struct PatchBwdIn {
  EotDims d;
  const float* patch;
  const ImgParams* img;
  const float* ymean;
  const float* dmatched;
  bool add_tv;
};
// mean dYc per image: fp32 terms summed in fp64.  A term whose gates are ambiguous may be there or not: its
// size goes into the bound
template <class T> std::vector<T> mean_dyc_all(const PatchBwdIn& in) {
  const long npx = (long)in.d.P * in.d.P;
  std::vector<T> out(in.d.B);
  for (int b = 0; b < in.d.B; ++b) {
    double s = 0, se = 0, sa = 0;
    for (long i = 0; i < npx; ++i) {
      T p[3];
      for (int c = 0; c < 3; ++c) p[c] = print_px<T>(in.patch[i * 3 + c], in.img[b], c, true);
      Gates g;
      MatchBwd<T> mb = match_bwd_px<T>(p, T(in.ymean[b * 2]), T(in.ymean[b * 2 + 1]), in.dmatched + ((long)b * npx + i) * 3, T(0.0f), g);
      s += val(mb.dyc);
      sa += std::fabs(val(mb.dyc));
      if constexpr (std::is_same<T, E>::value) {
        const float* dm = in.dmatched + ((long)b * npx + i) * 3;  // |dYc| <= 255/127 sum|dm|
        se += mb.dyc.e + (mb.dyc_amb ? 2.1 * (std::fabs(dm[0]) + std::fabs(dm[1]) + std::fabs(dm[2])) : 0.0);
      }
    }
    const double m = s / (double)npx;
    if constexpr (std::is_same<T, E>::value) {
      const double depth = (double)((npx + 64 * 256 - 1) / (64 * 256)) + 8 + 64 + 1;
      out[b] = E(m, (se + depth * 1.1102230246251565e-16 * sa) / (double)npx + kU * std::fabs(m));
    } else {
      out[b] = (float)m;
    }
  }
  return out;
}
inline float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
// one patch pixel's gradient; the sign of a difference of two fp32 values is the same in every precision, so
// the TV term has no gate
template <class T>
void patch_grad_px(const PatchBwdIn& in, const std::vector<T>& mdyc, long i, Gates& g, T* out, Fault f = F_NONE) {
  const long npx = (long)in.d.P * in.d.P;
  const int P = in.d.P;
  T gr[3] = {T(0.f), T(0.f), T(0.f)};
  for (int b = 0; b < in.d.B; ++b) {
    const ImgParams& ip = in.img[b];
    T p[3], pre[3];
    for (int c = 0; c < 3; ++c) {
      pre[c] = T(ip.w[c]) * T(in.patch[i * 3 + c]) + T(ip.b[c]);
      p[c] = clampT(pre[c], -1.0f, 1.0f);
    }
    MatchBwd<T> mb = match_bwd_px<T>(p, T(in.ymean[b * 2]), T(in.ymean[b * 2 + 1]), in.dmatched + ((long)b * npx + i) * 3,
                                     f == F_NO_MEAN_DYC ? T(0.0f) : mdyc[b], g);
    for (int c = 0; c < 3; ++c) {
      const bool lo = gate_ge(g, pre[c], -1.0f), hi = gate_le(g, pre[c], 1.0f);
      if (lo && hi) gr[c] += mb.dp[c] * T(ip.w[c]);
    }
  }
  if (in.add_tv) {
    const int y = (int)(i / P), x = (int)(i % P);
    for (int c = 0; c < 3; ++c) {
      const float v = in.patch[i * 3 + c];
      float t = 0.f;
      if (y > 0) t += sgnf(v - in.patch[(i - P) * 3 + c]);
      if (y < P - 1) t -= sgnf(in.patch[(i + P) * 3 + c] - v);
      if (x > 0) t += sgnf(v - in.patch[(i - 1) * 3 + c]);
      if (x < P - 1) t -= sgnf(in.patch[(i + 1) * 3 + c] - v);
      gr[c] += T(1e-5f) * T(t);
    }
  }
  for (int c = 0; c < 3; ++c) out[c] = gr[c];
}

// ---- TV ---------------------------------------------------------------------------------------------------
// fp32 differences summed in fp64, rounded to fp32 once; metrics[LOSS] += 1e-5f * (float)tv
template <class T> T tv_of(const float* p, int P, Fault f = F_NONE) {
  const long n = (long)P * P * 3;
  double s = 0, se = 0;
  for (long e = 0; e < n; ++e) {
    const long px = e / 3;
    const int y = (int)(px / P), x = (int)(px % P);
    const bool down = f == F_TV_LAST_ROW ? y + 2 < P : y + 1 < P;
    if (down) { T t = tabs(T(p[e + (long)P * 3]) - T(p[e])); s += val(t); if constexpr (std::is_same<T, E>::value) se += t.e; }
    if (x + 1 < P) { T t = tabs(T(p[e + 3]) - T(p[e])); s += val(t); if constexpr (std::is_same<T, E>::value) se += t.e; }
  }
  if constexpr (std::is_same<T, E>::value) {
    const double depth = (double)((n + 256 * 256 - 1) / (256 * 256)) + 8 + 4 + 64 + 1;
    return E(s, se + depth * 1.1102230246251565e-16 * s + kU * s);
  } else {
    return (float)s;
  }
}

// ---- comparing ------------------------------------------------------------------------------------------
struct Fld {
  double ratio = 0;
  long nonfinite = 0;
};
inline double ratio_of(double got, const E& r) {
  const double err = std::fabs(got - r.v), bound = r.e + kTiny;
  if (!(err == err) || !(bound == bound)) return 1e300;
  return err <= bound ? err / bound : (err / bound > 1e300 ? 1e300 : err / bound);
}
inline void cmp(Fld& f, float got, const E& r) {
  if (!std::isfinite(got)) { f.nonfinite++; f.ratio = std::max(f.ratio, 1e300); return; }
  f.ratio = std::max(f.ratio, ratio_of(got, r));
}
inline long ulp_diff(float a, float b) {
  int32_t x, y;
  std::memcpy(&x, &a, 4);
  std::memcpy(&y, &b, 4);
  if (x < 0) x = (int32_t)0x80000000 - x;
  if (y < 0) y = (int32_t)0x80000000 - y;
  return std::labs((long)x - (long)y);
}

// ---- inputs -------------------------------------------------------------------------------------------------
struct Inputs {
  Case c;
  EotDims d;
  PlaceRule rule;
  std::vector<float> boxes;  // [B, maxb, 4]
  std::vector<int> count;
  std::vector<float> patch;  // [P,P,3]; with batch or !apply_print: [B,P,P,3] in src
  std::vector<float> src;
  std::vector<float> imgs;   // [B,H,W,3]
  std::vector<float> dimg;   // [B,H,W,3]
  std::vector<ImgParams> clip_img;
  double margin = 1e9;       // the placement's smallest truncation margin, by the reference
  double gmax = 1.0;
};
inline uint64_t lcg(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 11;
}
inline float uni01(uint64_t& s) { return (float)(lcg(s) & 0xFFFFFF) / 16777216.0f; }
inline void fill_sym(std::vector<float>& v, size_t n, uint64_t seed, float ampl, float clip = 1e9f) {
  v.resize(n);
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 12345;
  for (auto& x : v) x = fminf(fmaxf((2.0f * uni01(s) - 1.0f) * ampl, -clip), clip);
}
inline Inputs make_inputs(const Case& c) {
  Inputs in;
  in.c = c;
  in.rule = rule_of(c);
  EotDims& d = in.d;
  d.B = c.B; d.H = c.H; d.W = c.W; d.maxb = c.maxb; d.P = c.P;
  int psmax = 4;
  for (int p : c.ps) psmax = std::max(psmax, p);
  d.span_stride = c.span_stride ? c.span_stride : (psmax + 3) / 4 * 4;
  in.count = c.counts;
  in.count.resize(c.B, 0);
  in.boxes.assign((size_t)c.B * c.maxb * 4, 0.f);
  uint64_t s = c.seed * 7919 + 17;
  size_t nth = 0;
  for (int b = 0; b < c.B; ++b)
    for (int k = 0; k < in.count[b] && k < c.maxb; ++k, ++nth) {
      const int ps = c.ps.empty() ? 8 : c.ps[nth % c.ps.size()];
      u32x4 r = rng(c.seed, 0, (uint32_t)k, (uint32_t)(c.gimg0 + b), c.step, RNG_PLACE);
      const float bscale = in.rule.random_scale ? runif(r.z, in.rule.scale_lo, in.rule.scale_hi) : c.scale;
      const float longer = ((float)ps + 0.5f) / bscale, shorter = 0.7f * longer;
      const float h = (nth & 1) ? shorter : longer, w = (nth & 1) ? longer : shorter;
      float cy, cx;
      if (c.layout == L_CORNERS) {
        cy = (nth & 2) ? (float)c.H - 1.3f : 1.3f;
        cx = ((nth + 1) & 2) ? (float)c.W - 1.7f : 1.7f;
      } else if (c.layout == L_CLUSTER) {
        cy = 0.5f * c.H + 6.0f * (uni01(s) - 0.5f);
        cx = 0.5f * c.W + 6.0f * (uni01(s) - 0.5f);
      } else if (c.layout == L_GRID) {
        const int cols = std::max(1, c.W / 12);
        cy = 7.3f + 12.0f * (float)((k / cols) % std::max(1, c.H / 12));
        cx = 7.6f + 12.0f * (float)(k % cols);
      } else {
        cy = (0.15f + 0.7f * uni01(s)) * c.H;
        cx = (0.15f + 0.7f * uni01(s)) * c.W;
      }
      float* bx = &in.boxes[((size_t)b * c.maxb + k) * 4];
      for (int tries = 0; tries < 60; ++tries) {
        bx[0] = cy - h / 2; bx[1] = cx - w / 2; bx[2] = cy + h / 2; bx[3] = cx + w / 2;
        double m = 1e9;
        PlaceOpt o;
        o.margin = &m;
        place_one(d, bx, k, c.gimg0 + b, c.scale, c.seed, c.step, in.rule, o);
        if (m >= 2e-3) break;
        cy += 0.137f;
        cx += 0.211f;
      }
    }
  {
    PlaceOpt o;
    o.margin = &in.margin;
    sim_place(d, in.boxes, in.count, c.scale, c.seed, c.step, c.gimg0, in.rule, o);
  }
  // a colourful patch with saturated elements (28 %) and constant blocks for TV's sgn(0) ties: 3 x 3 in the top
  // left corner (ties on the first row and column and, at (1,1)-(2,1) and (1,1)-(1,2), away from every edge) and
  // 2 x 2 in the other three corners (the last row and column); tv_ties counts them for --plan
  const size_t pp = (size_t)c.P * c.P * 3;
  fill_sym(in.patch, pp, c.seed + 101, 1.4f, 1.0f);
  auto block = [&](int y0, int x0, int n, float shift) {
    for (int y = y0; y < y0 + n; ++y)
      for (int x = x0; x < x0 + n; ++x)
        for (int ch = 0; ch < 3; ++ch) in.patch[((size_t)y * c.P + x) * 3 + ch] = 0.25f * (ch + 1) - 0.6f + shift;
  };
  block(0, 0, 3, 0.0f);
  block(0, c.P - 2, 2, 0.05f);
  block(c.P - 2, 0, 2, -0.05f);
  block(c.P - 2, c.P - 2, 2, 0.1f);
  const bool per_image = c.batch || !c.apply_print;
  if (per_image) fill_sym(in.src, pp * c.B, c.seed + 102, 1.4f, 1.0f);
  fill_sym(in.imgs, (size_t)c.B * c.H * c.W * 3, c.seed + 103, c.img_amp);
  fill_sym(in.dimg, (size_t)c.B * c.H * c.W * 3, c.seed + 104, 1.0f);
  in.gmax = 1.0;
  in.clip_img.resize(c.B);
  for (int b = 0; b < c.B; ++b)
    for (int ch = 0; ch < 3; ++ch) {
      // w around 1.5: the print clip bites on both sides; the red offset keeps red below +1, so no pixel prints
      // as pure white (u = v = 0 up to rounding, which would put its RGB gates on their thresholds)
      in.clip_img[b].w[ch] = 1.5f + 0.05f * (float)(b - ch);
      in.clip_img[b].b[ch] = (ch == 0 ? -0.7f : 0.03f * (float)(ch - 1)) + 0.01f * b;
    }
  return in;
}

// TV's ties by the reference alone: equal neighbour pairs, vertical (y, y + 1) and horizontal (x, x + 1), by the
// edge the pair touches (a corner pair counts for both of its edges), pairs touching none, and the elements one
// of whose up to four TV-gradient terms is sgn(0)
struct TvTies {
  long v[5] = {0, 0, 0, 0, 0}, h[5] = {0, 0, 0, 0, 0};  // first row, last row, first column, last column, interior
  long zero_term_elems = 0;
};
inline TvTies tv_ties(const float* p, int P) {
  TvTies t;
  auto at = [&](int y, int x, int c) { return p[((long)y * P + x) * 3 + c]; };
  for (int y = 0; y < P; ++y)
    for (int x = 0; x < P; ++x)
      for (int c = 0; c < 3; ++c) {
        const float v = at(y, x, c);
        if (y + 1 < P && at(y + 1, x, c) == v) {
          const bool e[4] = {y == 0, y + 1 == P - 1, x == 0, x == P - 1};
          for (int k = 0; k < 4; ++k) t.v[k] += e[k];
          t.v[4] += !(e[0] || e[1] || e[2] || e[3]);
        }
        if (x + 1 < P && at(y, x + 1, c) == v) {
          const bool e[4] = {y == 0, y == P - 1, x == 0, x + 1 == P - 1};
          for (int k = 0; k < 4; ++k) t.h[k] += e[k];
          t.h[4] += !(e[0] || e[1] || e[2] || e[3]);
        }
        t.zero_term_elems += (y > 0 && at(y - 1, x, c) == v) || (y + 1 < P && at(y + 1, x, c) == v) ||
                             (x > 0 && at(y, x - 1, c) == v) || (x + 1 < P && at(y, x + 1, c) == v);
      }
  return t;
}

// exact -1 / +1 values planted into R: a block of -1 (r == -1 under the compositor's fill test) and single
// values on the gate of the rotation gradient
inline void plant(const EotDims& d, const PlaceBlock& pb, std::vector<float>& R) {
  const BoxPlace* place = pb.place();
  (void)d;
  for (long sl = 0; sl < pb.nslot(); ++sl) {
    const BoxPlace& P = place[sl];
    if (!P.valid) continue;
    const int n = P.ps;
    for (int i = n / 4; i < n / 4 + std::max(2, n / 3) && i < n; ++i)
      for (int j = n / 4; j < n / 4 + std::max(2, n / 3) && j < n; ++j)
        for (int c = 0; c < 3; ++c) R[P.roff + ((long)i * n + j) * 3 + c] = -1.0f;
    for (long e = 0; e < (long)n * n * 3; e += 7) R[P.roff + e] = (e / 7) % 2 ? 1.0f : -1.0f;
  }
}

// ---- the verdict ------------------------------------------------------------------------------------------
struct Verdict {
  std::vector<std::pair<std::string, double>> fields;  // ratios (<= 1) and *_bad counts (== 0)
  long nonfinite = 0;
  bool place_ok = false;     // integers, roff, lists, spans' start / end: the later stages ran
  long amb_elems = 0, all_elems = 0;   // decision allowance
  double pre_outside = 0;    // share of pre outside [-1, 1]
  bool stopped = false;
  void ratio(const char* n, const Fld& f) {
    fields.emplace_back(n, f.ratio);
    nonfinite += f.nonfinite;
  }
  void bad(const char* n, long k) { fields.emplace_back(std::string(n) + "_bad", (double)k); }
  double allow_share() const { return all_elems ? (double)amb_elems / (double)all_elems : 0.0; }
  bool pass() const {
    if (nonfinite || !place_ok) return false;
    for (auto& f : fields) {
      const bool isbad = f.first.size() > 4 && f.first.compare(f.first.size() - 4, 4, "_bad") == 0;
      if (isbad ? f.second != 0 : !(f.second <= 1.0)) return false;
    }
    return allow_share() <= 0.01;
  }
};

// ---- the stage checks -------------------------------------------------------------------------------------
// placement: integers, roff and every list against the fp32 restatement, exactly; angle and delta within 2 ulp;
// the print parameters, fwd and inv against fp64 (from the device's own angle); spans: start / end exact,
// inv_total and sample_f within 1 ulp
inline void check_place(const Inputs& in, const PlaceOut& got, Verdict& V) {
  const EotDims& d = in.d;
  const Case& c = in.c;
  const PlaceOut ref = sim_place(d, in.boxes, in.count, c.scale, c.seed, c.step, c.gimg0, in.rule);
  long ibad = 0, lbad = 0, sbad = 0, abad = 0;
  Fld fw, fb, ffwd, finv, fspan;
  for (int b = 0; b < d.B; ++b) {
    u32x4 r = rng(c.seed, 0, 0, (uint32_t)(c.gimg0 + b), c.step, RNG_PRINT);
    u32x4 r2 = rng(c.seed, 1, 0, (uint32_t)(c.gimg0 + b), c.step, RNG_PRINT);
    u32x4 r3 = rng(c.seed, 2, 0, (uint32_t)(c.gimg0 + b), c.step, RNG_PRINT);
    cmp(fw, got.img[b].w[0], rnorm64(r.x, r.y, 0.5f, 0.1f));
    cmp(fw, got.img[b].w[1], rnorm64(r.z, r.w, 0.5f, 0.1f));
    cmp(fw, got.img[b].w[2], rnorm64(r2.x, r2.y, 0.5f, 0.1f));
    cmp(fb, got.img[b].b[0], rnorm64(r2.z, r2.w, 0.0f, 0.01f));
    cmp(fb, got.img[b].b[1], rnorm64(r3.x, r3.y, 0.0f, 0.01f));
    cmp(fb, got.img[b].b[2], rnorm64(r3.z, r3.w, 0.0f, 0.01f));
  }
  const BoxPlace* gp = got.pb.place();
  const BoxPlace* rp = ref.pb.place();
  for (long sl = 0; sl < got.pb.nslot(); ++sl) {
    const BoxPlace &g = gp[sl], &r = rp[sl];
    if (g.valid != r.valid) { ibad++; continue; }
    const bool drawn = (sl % d.maxb) < in.count[sl / d.maxb];
    if (!drawn) {  // an empty slot is all zero
      BoxPlace z{};
      if (std::memcmp(&g, &z, sizeof z) != 0) ibad++;
      continue;
    }
    if (g.ymin != r.ymin || g.xmin != r.xmin || g.ps != r.ps || g.diag != r.diag || g.pad != r.pad) ibad++;
    if (g.valid && g.roff != r.roff) ibad++;
    if (ulp_diff(g.angle, r.angle) > 2 || ulp_diff(g.delta, r.delta) > 2) abad++;
    // tfa's transform and its inverse from the device's own angle; cosf / sinf within 4 u
    const double ang = g.angle;
    const E cs(std::cos(ang), 4 * kU), sn(std::sin(ang), 4 * kU), s1((double)g.diag - 1.0);
    const E xo = (s1 - (cs * s1 - sn * s1)) * E(0.5), yo = (s1 - (sn * s1 + cs * s1)) * E(0.5);
    const E fwd[6] = {cs, -sn, xo, sn, cs, yo};
    for (int q = 0; q < 6; ++q) cmp(ffwd, g.fwd[q], fwd[q]);
    // the inverse of [c -s xo; s c yo]: det = c^2 + s^2; formed in fp64 from fp32 entries and rounded once, so
    // the entries' own errors dominate
    const E det = cs * cs + sn * sn;
    const double id = 1.0 / det.v, ide = det.e / (det.v * det.v);
    auto dv = [&](E n) { return rnd(n.v * id, n.e * id + std::fabs(n.v) * ide); };
    const E inv[6] = {dv(cs), dv(sn), dv(-sn * yo - cs * xo), dv(-sn), dv(cs), dv(sn * xo - cs * yo)};
    for (int q = 0; q < 6; ++q) cmp(finv, g.inv[q], inv[q]);
  }
  const Lists gl = got.pb.lists(), rl = ref.pb.lists();
  const long nslot = got.pb.nslot();
  const int nv = *rl.nvalid;
  lbad += *gl.nvalid != nv;
  lbad += *gl.total_chunks != *rl.total_chunks;
  for (int b = 0; b < d.B; ++b) lbad += (gl.img_n[b] != rl.img_n[b]) + (gl.img_first[b] != rl.img_first[b]);
  for (int v = 0; v < nv; ++v) lbad += (gl.vlist[v] != rl.vlist[v]);
  for (int v = 0; v <= nv; ++v) lbad += (gl.cprefix[v] != rl.cprefix[v]) + (gl.tprefix[v] != rl.tprefix[v]);
  for (int x = 0; x < 8; ++x) {
    for (int b = 0; b < d.B; ++b) lbad += gl.bcnt[x * d.B + b] != rl.bcnt[x * d.B + b];
    for (int v = 0; v < nv; ++v) lbad += gl.bvpre[x * nslot + v] != rl.bvpre[x * nslot + v];
  }
  // what no kernel writes keeps its fill: vlist, cprefix, tprefix and every band's bvpre past the valid boxes, and
  // the block's two spare ints
  for (long v = nv; v < nslot; ++v) lbad += gl.vlist[v] != kFillInt;
  for (long v = nv + 1; v <= nslot; ++v) lbad += (gl.cprefix[v] != kFillInt) + (gl.tprefix[v] != kFillInt);
  for (int x = 0; x < 8; ++x)
    for (long v = nv; v < nslot; ++v) lbad += gl.bvpre[x * nslot + v] != kFillInt;
  {
    const int* l0 = gl.nvalid;
    const long total = (long)((got.pb.bytes.size() - nslot * sizeof(BoxPlace)) / sizeof(int));
    for (long k = gl.nints; k < total; ++k) lbad += l0[k] != kFillInt;
  }
  for (long sl = 0; sl < nslot; ++sl) {
    const int ps = rp[sl].valid ? rp[sl].ps : 0;
    for (int i = 0; i < d.span_stride; ++i) {
      const SpanEntry &g = got.spans[sl * d.span_stride + i], &r = ref.spans[sl * d.span_stride + i];
      if (i >= ps) { sbad += std::memcmp(&g, &r, sizeof g) != 0; continue; }
      if (g.start != r.start || g.end != r.end) { sbad++; continue; }
      const long u = std::max(ulp_diff(g.inv_total, r.inv_total), ulp_diff(g.sample_f, r.sample_f));
      fspan.ratio = std::max(fspan.ratio, (double)u);
      if (!std::isfinite(g.inv_total) || !std::isfinite(g.sample_f)) fspan.nonfinite++;
    }
  }
  V.ratio("img_w", fw);
  V.ratio("img_b", fb);
  V.ratio("fwd", ffwd);
  V.ratio("inv", finv);
  V.ratio("span_ulp", fspan);
  V.bad("place_int", ibad);
  V.bad("angle_delta", abad);
  V.bad("lists", lbad);
  V.bad("span_int", sbad);
  V.place_ok = ibad == 0 && lbad == 0 && sbad == 0;
}

inline void check_match(const MatchIn& m, const std::vector<float>& ymean, const std::vector<float>& matched, Verdict& V) {
  std::vector<E> ry, rm;
  ymean_all<E>(m, ry);
  Fld fy, fm;
  for (size_t i = 0; i < ry.size(); ++i) cmp(fy, ymean[i], ry[i]);
  match_all<E>(m, ymean.data(), rm);
  for (size_t i = 0; i < rm.size(); ++i) cmp(fm, matched[i], rm[i]);
  V.ratio("ymean", fy);
  V.ratio("matched", fm);
}

inline bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// resize: against fp64 with the derived bound, and bit for bit against the fp32 restatement ("exact mode":
// the kernel is IEEE basic operations in a fixed order)
inline void check_resize(const Inputs& in, const PlaceOut& po, const std::vector<float>& matched, float amp,
                         const std::vector<float>& rstore, Verdict& V) {
  const Case& c = in.c;
  std::vector<E> r;
  std::vector<float> r32;
  resize_all<E>(in.d, matched.data(), po.pb, po.spans.data(), c.seed, c.step, c.gimg0, amp, r);
  resize_all<float>(in.d, matched.data(), po.pb, po.spans.data(), c.seed, c.step, c.gimg0, amp, r32);
  Fld f;
  long xbad = 0, outside = 0;
  const long n = r_total(in.d, po.pb);
  for (long i = 0; i < n; ++i) {
    cmp(f, rstore[i], r[i]);
    xbad += !same_bits(rstore[i], r32[i]);
    outside += !(r[i].v >= -1.0 && r[i].v <= 1.0);
  }
  for (size_t i = n; i < rstore.size(); ++i) xbad += !same_bits(rstore[i], unwritten<float>());
  V.pre_outside = n ? (double)outside / (double)n : 0.0;
  V.ratio("resize", f);
  V.bad("resize_exact", xbad);
}

// an element against every outcome of its ambiguous gates: the smallest ratio counts
template <class Eval> double best_ratio(Eval ev, int* namb) {
  Gates g0;
  double best = ev(g0);
  *namb = g0.n;
  const int n = std::min(g0.n, 6);
  for (unsigned m = 1; m < (1u << n) && best > 1.0; ++m) {
    Gates g;
    g.flip = m;
    best = std::min(best, ev(g));
  }
  return best;
}

inline void check_composite(const Inputs& in, const PlaceOut& po, const std::vector<float>& R, const std::vector<float>& img_out,
                            const std::vector<int16_t>& owner, const std::vector<float>& mask, Verdict& V) {
  const EotDims& d = in.d;
  Fld fo, fm;
  long obad = 0;
  for (int b = 0; b < d.B; ++b)
    for (int y = 0; y < d.H; ++y)
      for (int x = 0; x < d.W; ++x)
        for (int c = 0; c < 3; ++c) {
          const long e = ((((long)b * d.H + y) * d.W) + x) * 3 + c;
          const float inp = in.imgs[e];
          if (!std::isfinite(img_out[e])) fo.nonfinite++;
          if (!std::isfinite(mask[e])) fm.nonfinite++;
          double ro = 0, rm = 0, bw = 2e300;
          bool own_ok = false;
          int namb = 0;
          best_ratio([&](Gates& g) {
            Px<E> p = composite_px<E>(d, po.pb, R.data(), b, y, x, c, inp, g);
            const E m = p.covered ? E(inp) - p.v : E(0.0);
            const double a = ratio_of(img_out[e], p.v), k = ratio_of(mask[e], m);
            const bool ok = owner[e] == p.own;
            const double w = std::max(std::max(a, k), ok ? 0.0 : 1e300);
            if (w < bw) { bw = w; ro = a; rm = k; own_ok = ok; }
            return w;
          }, &namb);
          fo.ratio = std::max(fo.ratio, ro);
          fm.ratio = std::max(fm.ratio, rm);
          obad += !own_ok;
          V.amb_elems += namb > 0;
          V.all_elems += 1;
        }
  V.ratio("img_out", fo);
  V.ratio("mask", fm);
  V.bad("owner", obad);
}

inline void check_rot_bwd(const Inputs& in, const PlaceOut& po, const std::vector<float>& R, const std::vector<int16_t>& owner,
                          const std::vector<float>& dstore, Verdict& V) {
  std::vector<E> r;
  rot_bwd_all<E>(in.d, in.dimg.data(), owner.data(), po.pb, R.data(), in.gmax, r);
  Fld f;
  long tail = 0;
  const long n = r_total(in.d, po.pb);
  for (long i = 0; i < n; ++i) cmp(f, dstore[i], r[i]);
  for (size_t i = n; i < dstore.size(); ++i) tail += !same_bits(dstore[i], unwritten<float>());
  V.ratio("drot", f);
  V.bad("drot_tail", tail);
}

// the adjoint against the fp64 transpose (the rows stage from the device's dR, the cols stage from the device's
// U), and <resize(m), g> = <m, resize_bwd(g)> with the device's two results, summed in fp64: the noise and the
// brightness shift are taken off R exactly, and the bound is sum|g| bound(R) + sum|m| bound(dm)
inline void check_resize_bwd(const Inputs& in, const PlaceOut& po, const std::vector<float>& matched, float amp,
                             const std::vector<float>& rstore, const std::vector<float>& dstore, const std::vector<float>& tstore,
                             const std::vector<float>& dmatched, Verdict& V) {
  const EotDims& d = in.d;
  const Case& c = in.c;
  std::vector<E> rt, rdm;
  resize_bwd_all<E>(d, po.pb, po.spans.data(), dstore.data(), &rt, tstore.data(), rdm);
  Fld ft, fd;
  long tail = 0;
  const long nt = t_total(d, po.pb);
  // rows of U past a box's ps (the ragged tile's) are never written
  const Lists L = po.pb.lists();
  const BoxPlace* place = po.pb.place();
  for (int v = 0; v < *L.nvalid; ++v) {
    const BoxPlace& P = place[L.vlist[v]];
    const long ub = (long)L.tprefix[v] * 4 * d.P * 3, rows = (long)(L.tprefix[v + 1] - L.tprefix[v]) * 4;
    for (long i = 0; i < rows * d.P * 3; ++i) {
      if (i < (long)P.ps * d.P * 3) cmp(ft, tstore[ub + i], rt[ub + i]);
      else tail += !same_bits(tstore[ub + i], unwritten<float>());
    }
  }
  for (size_t i = nt; i < tstore.size(); ++i) tail += !same_bits(tstore[i], unwritten<float>());
  for (size_t i = 0; i < rdm.size(); ++i) cmp(fd, dmatched[i], rdm[i]);
  V.ratio("urows", ft);
  V.ratio("dmatched", fd);
  V.bad("urows_tail", tail);
  // the adjoint identity
  std::vector<E> rr;
  resize_all<E>(d, matched.data(), po.pb, po.spans.data(), c.seed, c.step, c.gimg0, amp, rr);
  double lhs = 0, rhs = 0, bound = 0;
  for (int v = 0; v < *L.nvalid; ++v) {
    const int sl = L.vlist[v];
    const BoxPlace& P = place[sl];
    for (long px = 0; px < (long)P.ps * P.ps; ++px) {
      u32x4 r = rng(c.seed, (uint32_t)px, (uint32_t)(sl % d.maxb), (uint32_t)(c.gimg0 + sl / d.maxb), c.step, RNG_NOISE);
      const uint32_t rw[3] = {r.x, r.y, r.z};
      for (int ch = 0; ch < 3; ++ch) {
        const long e = P.roff + px * 3 + ch;
        const double lin = (double)rstore[e] - (double)runif(rw[ch], -amp, amp) - (double)P.delta;
        lhs += lin * dstore[e];
        bound += std::fabs((double)dstore[e]) * rr[e].e;
      }
    }
  }
  // dmatched's own bound from the device's dR through both stages: the cols stage's (from the device's U) plus
  // the rows stage's carried through the column weights, which sum to at most 1 + ps / P per source row
  for (size_t i = 0; i < rdm.size(); ++i) {
    rhs += (double)matched[i] * dmatched[i];
    bound += std::fabs((double)matched[i]) * rdm[i].e;
  }
  for (int v = 0; v < *L.nvalid; ++v) {
    const BoxPlace& P = place[L.vlist[v]];
    const long ub = (long)L.tprefix[v] * 4 * d.P * 3;
    double se = 0;
    for (long i = 0; i < (long)P.ps * d.P * 3; ++i) se += rt[ub + i].e;
    bound += se * 1.0;  // |m| <= 1 and every row weight <= 1
  }
  Fld fa;
  fa.ratio = ratio_of(lhs, E(rhs, bound + 1e-13 * (std::fabs(lhs) + std::fabs(rhs))));
  V.ratio("adjoint", fa);
}

inline void check_patch_bwd(const PatchBwdIn& in, const std::vector<float>& grad, Verdict& V) {
  const std::vector<E> md = mean_dyc_all<E>(in);
  const long npx = (long)in.d.P * in.d.P;
  Fld f;
  for (long i = 0; i < npx; ++i) {
    int namb = 0;
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(grad[i * 3 + c])) f.nonfinite++;
    const double r = best_ratio([&](Gates& g) {
      E o[3];
      patch_grad_px<E>(in, md, i, g, o);
      return std::max(std::max(ratio_of(grad[i * 3], o[0]), ratio_of(grad[i * 3 + 1], o[1])), ratio_of(grad[i * 3 + 2], o[2]));
    }, &namb);
    f.ratio = std::max(f.ratio, r);
    V.amb_elems += 3 * (namb > 0);
    V.all_elems += 3;
  }
  V.ratio("grad", f);
}

// metrics row: [PHX_M_LOSS] started at loss0; with add_to_loss the TV lands in [PHX_M_TV] and 1e-5f * tv is added
inline void check_tv(const float* patch, int P, bool add, float loss0, const std::vector<float>& metrics,
                     const std::vector<float>& metrics0, Verdict& V) {
  Fld ft, fl;
  long other = 0;
  if (add) {
    const E tv = tv_of<E>(patch, P);
    cmp(ft, metrics[PHX_M_TV], tv);
    cmp(fl, metrics[PHX_M_LOSS], E(loss0) + E(1e-5f) * E(metrics[PHX_M_TV]));
  }
  for (int k = 0; k < PHX_NMETRIC; ++k)
    if (!add || (k != PHX_M_TV && k != PHX_M_LOSS)) other += !same_bits(metrics[k], metrics0[k]);
  V.ratio("tv", ft);
  V.ratio("loss", fl);
  V.bad("metrics_other", other);
}

// ---- a case through a backend -----------------------------------------------------------------------------
// Backend: place / match / resize / composite / rot_bwd / resize_bwd / patch_bwd / tv over host vectors (the
// device one uploads, launches and reads back; the stand-in computes in fp32).  Each stage's reference is
// computed from the backend's own earlier outputs.
struct StageOut {
  PlaceOut po;
  std::vector<ImgParams> img_used;
  std::vector<float> ymean, matched, rstore, rin, img_out, mask, dstore, tstore, dmatched, grad, metrics;
  std::vector<int16_t> owner;
};
inline MatchIn match_in(const Inputs& in, const std::vector<ImgParams>& img) {
  MatchIn m;
  m.d = in.d;
  const bool per_image = in.c.batch || !in.c.apply_print;
  m.src = per_image ? in.src.data() : in.patch.data();
  m.stride = per_image ? (long)in.d.P * in.d.P * 3 : 0;
  m.img = img.data();
  m.tgt = in.imgs.data();
  m.apply = in.c.batch || in.c.apply_print;
  return m;
}
inline std::vector<float> metrics0() {
  std::vector<float> m(PHX_NMETRIC);
  for (int k = 0; k < PHX_NMETRIC; ++k) m[k] = 0.5f + 0.25f * k;
  return m;
}
template <class Backend> Verdict run_case(const Inputs& in, Backend& be, StageOut& so) {
  Verdict V;
  const Case& c = in.c;
  be.place(in, so.po);
  check_place(in, so.po, V);
  if (!V.place_ok) {  // nothing downstream may index by a placement that is not the expected one
    V.stopped = true;
    return V;
  }
  so.img_used = c.clipw ? in.clip_img : so.po.img;
  const MatchIn m = match_in(in, so.img_used);
  be.match(in, m, so.ymean, so.matched);
  check_match(m, so.ymean, so.matched, V);
  be.resize(in, so.po, so.matched, so.rstore);
  check_resize(in, so.po, so.matched, c.amp, so.rstore, V);
  so.rin = so.rstore;
  if (c.plant) plant(in.d, so.po.pb, so.rin);
  be.composite(in, so.po, so.rin, so.img_out, so.owner, so.mask);
  check_composite(in, so.po, so.rin, so.img_out, so.owner, so.mask, V);
  be.rot_bwd(in, so.po, so.rin, so.owner, so.dstore);
  check_rot_bwd(in, so.po, so.rin, so.owner, so.dstore, V);
  be.resize_bwd(in, so.po, so.dstore, so.tstore, so.dmatched);
  check_resize_bwd(in, so.po, so.matched, c.amp, so.rstore, so.dstore, so.tstore, so.dmatched, V);
  PatchBwdIn pi{in.d, in.patch.data(), so.img_used.data(), so.ymean.data(), so.dmatched.data(), c.add_tv != 0};
  be.patch_bwd(in, pi, so.grad);
  check_patch_bwd(pi, so.grad, V);
  be.tv(in, so.metrics);
  check_tv(in.patch.data(), in.d.P, c.add_loss != 0, metrics0()[PHX_M_LOSS], so.metrics, metrics0(), V);
  return V;
}

// ---- the stand-in backend -----------------------------------------------------------------------------------
struct Sim {
  Fault f = F_NONE;
  void place(const Inputs& in, PlaceOut& po) {
    PlaceOpt o;
    o.f = f;
    po = sim_place(in.d, in.boxes, in.count, in.c.scale, in.c.seed, in.c.step, in.c.gimg0, in.rule, o);
  }
  void match(const Inputs&, const MatchIn& m, std::vector<float>& ymean, std::vector<float>& matched) {
    ymean_all<float>(m, ymean);
    match_all<float>(m, ymean.data(), matched);
  }
  void resize(const Inputs& in, const PlaceOut& po, const std::vector<float>& matched, std::vector<float>& rstore) {
    resize_all<float>(in.d, matched.data(), po.pb, po.spans.data(), in.c.seed, in.c.step, in.c.gimg0, in.c.amp, rstore, f);
  }
  void composite(const Inputs& in, const PlaceOut& po, const std::vector<float>& R, std::vector<float>& out,
                 std::vector<int16_t>& owner, std::vector<float>& mask) {
    const EotDims& d = in.d;
    const size_t n = (size_t)d.B * d.H * d.W * 3;
    out.resize(n); owner.resize(n); mask.resize(n);
    for (int b = 0; b < d.B; ++b)
      for (int y = 0; y < d.H; ++y)
        for (int x = 0; x < d.W; ++x)
          for (int c = 0; c < 3; ++c) {
            const size_t e = ((((size_t)b * d.H + y) * d.W) + x) * 3 + c;
            Gates g;
            Px<float> p = composite_px<float>(d, po.pb, R.data(), b, y, x, c, in.imgs[e], g, f);
            out[e] = p.v;
            owner[e] = (int16_t)p.own;
            mask[e] = p.covered ? in.imgs[e] - p.v : 0.f;
          }
  }
  void rot_bwd(const Inputs& in, const PlaceOut& po, const std::vector<float>& R, const std::vector<int16_t>& owner,
               std::vector<float>& dstore) {
    rot_bwd_all<float>(in.d, in.dimg.data(), owner.data(), po.pb, R.data(), 0, dstore, f);
  }
  void resize_bwd(const Inputs& in, const PlaceOut& po, const std::vector<float>& dstore, std::vector<float>& tstore,
                  std::vector<float>& dmatched) {
    resize_bwd_all<float>(in.d, po.pb, po.spans.data(), dstore.data(), &tstore, nullptr, dmatched, f);
  }
  void patch_bwd(const Inputs&, const PatchBwdIn& pi, std::vector<float>& grad) {
    const std::vector<float> md = mean_dyc_all<float>(pi);
    const long npx = (long)pi.d.P * pi.d.P;
    grad.resize(npx * 3);
    for (long i = 0; i < npx; ++i) {
      Gates g;
      patch_grad_px<float>(pi, md, i, g, &grad[i * 3], f);
    }
  }
  void tv(const Inputs& in, std::vector<float>& metrics) {
    metrics = metrics0();
    if (!in.c.add_loss) return;
    const float s = tv_of<float>(in.patch.data(), in.d.P, f);
    metrics[PHX_M_TV] = s;
    metrics[PHX_M_LOSS] += 1e-5f * s;
  }
};

// ---- JSON -------------------------------------------------------------------------------------------------
inline std::string jnum(double x) {
  char b[40];
  if (std::isfinite(x)) snprintf(b, sizeof b, "%.6g", x < 1e300 ? x : 1e300);
  else snprintf(b, sizeof b, "1e300");
  return b;
}
inline std::string verdict_json(const Verdict& V) {
  std::string s = "\"fields\":{";
  for (size_t i = 0; i < V.fields.size(); ++i) s += (i ? ",\"" : "\"") + V.fields[i].first + "\":" + jnum(V.fields[i].second);
  double ratio = 0;
  for (auto& f : V.fields)
    if (!(f.first.size() > 4 && f.first.compare(f.first.size() - 4, 4, "_bad") == 0)) ratio = std::max(ratio, f.second);
  s += "},\"ratio\":" + jnum(ratio) + ",\"nonfinite\":" + std::to_string(V.nonfinite) + ",\"place_ok\":" + (V.place_ok ? "true" : "false") +
       ",\"stopped\":" + (V.stopped ? "true" : "false") + ",\"allow_share\":" + jnum(V.allow_share()) +
       ",\"pre_outside\":" + jnum(V.pre_outside);
  return s;
}

}  // namespace eck
