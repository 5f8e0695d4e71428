// post_check.hpp — references, bounds and compare functions of the post-processing kernel parity checker
// (post_parity.cpp) and its teeth (post_teeth.cpp): pre_nms with the validity filter and the candidate lists,
// soft-NMS, the per-image max, the loss, count_ge, zero_segs, the sparse class-head backward and Adam.
//
// kernels_post.hip and k_adam are built with FP contraction off, so everything made of IEEE basic operations
// and comparisons is restated here once, as a template over the number type:
//   float  the exact reference (compared bit for bit, or as a set where the kernel's order is free) and, with a
//          seeded Fault, the CPU stand-in of the teeth;
//   E      an fp64 value with the running error bound of its fp32 evaluation.
// expf is the one library function: its error is g_exp_ulp ulps (set by the harness, DESIGN.md "Post-processing
// kernel parity"); expf(0) is taken as exactly 1.
// Host code only: no HIP header, so the teeth build with the host compiler.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "gemm_check.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pck {
using gck::f2u;
using gck::u2f;

constexpr double kU = 5.9604644775390625e-8;  // 2^-24: one fp32 rounding, relative
constexpr double kDen = 7.1e-46;              // half the smallest subnormal: the absolute floor of a rounding
constexpr uint32_t kFillWord = gck::kUnwritten;  // "never written": a NaN no kernel produces
constexpr double kInf = std::numeric_limits<double>::infinity();
// harness-only copies of the library's constants (the teeth do not link it): post_parity --plan prints these
// beside post_plan_info()'s and tests/test_post_parity_host.py holds them equal
constexpr int kPreTile = 128;
constexpr int kImaxChunks = 48;
constexpr int kNmsFl = 24;
constexpr int kMaxOutDev = 100;
constexpr long kNPatch = 640L * 640 * 3;
constexpr int kNMetric = 9;
enum { M_LOSS = 0, M_SCALE_LOSS = 1, M_SUM_M = 3, M_SUM_M2 = 4, M_NIMG = 8 };

inline double g_exp_ulp = 1.0;  // expf's error in ulps: twice the measured maximum, at least 1

// ---- E: an fp64 value with the running error bound of its fp32 evaluation ---------------------------------
struct E {
  double v = 0, e = 0;
  E() = default;
  E(double v_, double e_ = 0) : v(v_), e(e_) {}
};
inline bool is_f32(double v) { return (double)(float)v == v; }
// one fp32 rounding of the exact result v whose operands carried ep; exact operands whose exact result is an
// fp32 number give that number (a planted edge stays an edge)
inline E rnd(double v, double ep) {
  if (ep == 0 && is_f32(v)) return E(v, 0);
  return E(v, ep + kU * (std::fabs(v) + ep) + kDen);
}
inline E operator+(E a, E b) { return rnd(a.v + b.v, a.e + b.e); }
inline E operator-(E a, E b) { return rnd(a.v - b.v, a.e + b.e); }
inline E operator*(E a, E b) { return rnd(a.v * b.v, std::fabs(a.v) * b.e + std::fabs(b.v) * a.e + a.e * b.e); }
inline E operator/(E a, E b) {
  const double v = a.v / b.v, den = std::fabs(b.v) - b.e;
  return rnd(v, (a.e == 0 && b.e == 0) ? 0.0 : den > 0 ? (a.e + std::fabs(v) * b.e) / den : kInf);
}
inline E operator-(E a) { return E(-a.v, a.e); }
inline E tsqrt(E a) {
  const double v = std::sqrt(a.v);
  return rnd(v, a.e == 0 ? 0.0 : v - std::sqrt(std::max(0.0, a.v - a.e)));
}
inline float tsqrt(float a) { return sqrtf(a); }
inline E texp(E x) {
  if (x.v == 0 && x.e == 0) return E(1.0, 0);
  const double v = std::exp(x.v);
  return E(v, v * std::expm1(x.e) + g_exp_ulp * 2 * kU * v + kDen);
}
inline float texp(float x) { return expf(x); }
inline float tmin(float a, float b) { return fminf(a, b); }
inline float tmax(float a, float b) { return fmaxf(a, b); }
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
inline double val(float a) { return a; }
inline double val(E a) { return a.v; }
// |got - want| over its bound: 0 when equal, above 1 when outside; an exact want asks for the exact value
inline double ratio_of(float got, E want) {
  if (!std::isfinite(got) || !std::isfinite(want.v)) return (double)got == want.v ? 0.0 : kInf;
  const double d = std::fabs((double)got - want.v);
  if (d == 0) return 0;
  return want.e > 0 ? d / want.e : kInf;
}

// ---- seeded faults of the CPU stand-in ---------------------------------------------------------------------
enum Fault {
  F_NONE = 0,
  F_HALF_GE,         // the second class half wins on equality
  F_RAGGED_LAST,     // a ragged tile's last anchor dropped
  F_LEVEL_OFF1,      // the level lookup off by one at a tile0 boundary
  F_AREA_GE,         // area >= 100
  F_PERSON_AFTER,    // the person bit (4) set after the validity filter
  F_CAND_GE,         // the candidate gate sc >= cand.thresh
  F_CAND_TWICE,      // a candidate appended twice
  F_IMAX_NOADD,      // tie counts of equal chunks not added
  F_IMAX_FIRST,      // the first index not the smallest
  F_LOSS_GRAD0,      // loss gradient 0 at raw == 0
  F_TIE_NODIV,       // tied classes not divided by their number
  F_TIE_FIRST,       // only the first tied class gets the gradient
  F_DX_OVERWRITE,    // dx overwritten instead of accumulated
  F_NMS_TIE_HI,      // soft-NMS score ties broken by the higher index
  F_NO_CLIP,         // the output clip omitted
  F_COUNT_KEEP,      // cand.count not reset
  F_ADAM_SCALE_CLIP  // Adam's scale slot clipped to [-1, 1]
};

// ---- deterministic inputs ---------------------------------------------------------------------------------
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
  uint32_t u32() {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return (uint32_t)(s >> 24);
  }
  float uni(float lo, float hi) { return lo + (hi - lo) * ((u32() & 0xffffff) / 16777216.0f); }
  int below(int n) { return (int)(u32() % (uint32_t)n); }
};

enum Kind { K_CHAIN, K_NMS, K_IMAX, K_LOSS, K_ZERO, K_COUNT, K_ADAM, K_REFUSE };
enum Refuse { R_NONE = 0, R_NMS_MAXOUT101, R_ZERO_9, R_ZERO_MISALIGNED, R_SCATTER_NA33, R_SCATTER_AMODNA };
enum NmsMode { NM_MASK = 0, NM_PREFIX = 1, NM_M2 = 2 };

struct Case {
  std::string name;
  int kind = K_CHAIN, refuse = R_NONE;
  uint32_t seed = 1;
  // chain
  int B = 2, nclass = 90, na = 9, bf = 0;
  int cand_mask = 2, cand_list = 1;
  float cand_thresh = 0.001f, thresh = 0.5f;
  int K = 64, max_out = 100, nseg = 1;
  float scale = 0.3f;
  // direct
  int N = 0, nms_mode = NM_MASK, plant = 0;
  std::vector<int> counts;
  long n = 0;
  int t = 1, clip = 0;
};

struct Lev {  // LevelDesc's layout (kernels.hpp; post_parity.cpp holds the two to the same size)
  long cls_off, box_off;
  int h, w, anchor0, tile0;
};

inline void store(std::vector<float>& v, bool bf) {
  if (bf) for (float& x : v) x = gck::round_bf(x);
}

// The chain's inputs.  Pyramid 8x8, 4x4, 3x3, 2x2, 1x1 on a 64 x 64 image; the levels' logits and box
// regressions lie packed one after the other ([B][h w na][nclass] and [B][h w na][4] per level).
struct Plant { std::string what; int b, a; };
struct Chain {
  Case c;
  int A = 0, ntiles = 0, nlev = 0, PT = 0;
  float img = 64.f;
  std::vector<Lev> lev;
  std::vector<float> anchors, cls, box, wpred, dx0;
  std::vector<long> dx_off;
  std::vector<Plant> plants;
  int nloc(int l) const { return lev[l].h * lev[l].w * c.na; }
  int level_of(int a) const {
    int l = 0;
    while (l + 1 < nlev && a >= lev[l + 1].anchor0) ++l;
    return l;
  }
  long lg_off(int b, int a) const {
    const int l = level_of(a);
    return lev[l].cls_off + ((long)b * nloc(l) + (a - lev[l].anchor0)) * c.nclass;
  }
  long bx_off(int b, int a) const {
    const int l = level_of(a);
    return lev[l].box_off + ((long)b * nloc(l) + (a - lev[l].anchor0)) * 4;
  }
  int anchor_at(int l, int pix, int k) const { return lev[l].anchor0 + pix * c.na + k; }
};

inline Chain make_chain(const Case& c) {
  Chain ch;
  ch.c = c;
  const int hw[5] = {8, 4, 3, 2, 1};
  ch.nlev = 5;
  long co = 0, bo = 0, dxo = 0;
  for (int l = 0; l < 5; ++l) {
    Lev L;
    L.h = L.w = hw[l];
    L.cls_off = co; L.box_off = bo; L.anchor0 = ch.A; L.tile0 = ch.ntiles;
    const int nloc = L.h * L.w * c.na;
    co += (long)c.B * nloc * c.nclass;
    bo += (long)c.B * nloc * 4;
    ch.dx_off.push_back(dxo);
    dxo += (long)c.B * L.h * L.w * c.K;
    ch.A += nloc;
    ch.ntiles += (nloc + kPreTile - 1) / kPreTile;
    ch.lev.push_back(L);
  }
  ch.PT = ch.A / c.na;
  Rng r(c.seed);
  ch.anchors.resize((size_t)ch.A * 4);
  // Every pixel's anchors sit in a 64 x 64 cell of their own on a grid ten cells wide (cells 0 and 1 are left to
  // the planted boxes), concentric, 12 to 33 on a side: with regressions within +-0.2 the boxes of one pixel overlap
  // by at least a fifth of their extents and boxes of different pixels never touch, so no soft-NMS decay argument
  // is close to 0.  (Boxes may lie outside the 64 x 64 image: pre_nms does not clip, soft-NMS's output does.)
  for (int l = 0, pg = 2; l < 5; ++l)
    for (int p = 0; p < hw[l] * hw[l]; ++p, ++pg)
      for (int k = 0; k < c.na; ++k) {
        const float cy = 32.f + 64.f * (pg / 10), cx = 32.f + 64.f * (pg % 10);
        const float sy = 12.f + 3.f * (k % 8), sx = 12.f + 3.f * ((k + 3) % 8);
        float* an = &ch.anchors[(size_t)ch.anchor_at(l, p, k) * 4];
        an[0] = cy - sy / 2; an[1] = cx - sx / 2; an[2] = cy + sy / 2; an[3] = cx + sx / 2;
      }
  ch.cls.resize((size_t)co);
  ch.box.resize((size_t)bo);
  for (float& x : ch.box) x = r.uni(-0.2f, 0.2f);
  const int nc = c.nclass, hc = (nc + 1) / 2;
  for (int b = 0; b < c.B; ++b)
    for (int a = 0; a < ch.A; ++a) {
      float* lg = &ch.cls[(size_t)ch.lg_off(b, a)];
      for (int q = 0; q < nc; ++q) lg[q] = r.uni(-6.5f, -0.2f);  // (the maximum of 90 stays below 0: scores on both sides of 0.5, all above 0.001)
      if (r.below(4) == 0) lg[0] = r.uni(-1.f, 3.f);
      // the second image of three carries no person: its list (mask 1 / 2) is empty, its max is -FLT_MAX, dm 0
      if (c.B >= 3 && b == 1 && nc >= 2) lg[1] = 5.f;
    }
  auto plant = [&](const char* what, int b, int a) { ch.plants.push_back({what, b, a}); };
  auto logits = [&](int b, int a) { return &ch.cls[(size_t)ch.lg_off(b, a)]; };
  auto zero_reg = [&](int b, int a) { for (int q = 0; q < 4; ++q) ch.box[(size_t)ch.bx_off(b, a) + q] = 0.f; };
  auto person = [&](int b, int a, float v) {  // class 0 the single maximum at v
    float* lg = logits(b, a);
    for (int q = 1; q < nc; ++q) lg[q] = std::min(lg[q], v - 1.f);
    lg[0] = v;
  };
  const int b0 = 0;
  // argmax ties, on level 0 (full tiles) and on the single short tiles of the small levels
  for (int rep = 0; rep < 2; ++rep) {
    const int base = rep == 0 ? 7 * c.na : ch.lev[2].anchor0;  // pixel 7 of the 8x8 level; the 3x3 level
    for (int b = 0; b < c.B; ++b) {
      if (c.B >= 3 && b == 1) continue;
      if (hc >= 2) { float* lg = logits(b, base + 0); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[0] = lg[hc - 1] = 2.5f; plant("tie_first_half", b, base + 0); }
      if (nc >= 2 && c.na * 1 > 1) { float* lg = logits(b, base + 1); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[0] = lg[hc] = 2.5f; plant("tie_both_halves", b, base + 1); }
      if (nc >= 2 && c.na > 2) { float* lg = logits(b, base + 2); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[0] = 2.5f; lg[hc] = 2.75f; plant("second_half_greater", b, base + 2); }
      if (c.na > 3) { float* lg = logits(b, base + 3); for (int q = 0; q < nc; ++q) lg[q] = 1.5f; plant("all_equal", b, base + 3); }
      if (c.na > 4) { float* lg = logits(b, base + 4); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[nc - 1] = 2.5f; plant("max_last_class", b, base + 4); }
    }
  }
  if (c.na == 1 && nc >= 3) {  // one anchor per pixel: the same plants on consecutive pixels of level 0
    for (int b = 0; b < c.B; ++b) {
      float* lg = logits(b, 10); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[0] = lg[hc - 1] = 2.5f; plant("tie_first_half", b, 10);
      lg = logits(b, 11); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[0] = lg[hc] = 2.5f; plant("tie_both_halves", b, 11);
      lg = logits(b, 12); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[0] = 2.5f; lg[hc] = 2.75f; plant("second_half_greater", b, 12);
      lg = logits(b, 13); for (int q = 0; q < nc; ++q) lg[q] = 1.5f; plant("all_equal", b, 13);
      lg = logits(b, 14); for (int q = 0; q < nc; ++q) lg[q] = std::min(lg[q], 2.f); lg[nc - 1] = 2.5f; plant("max_last_class", b, 14);
    }
  }
  // validity edges: regression 0 on anchors of exact size (expf(0) == 1: exact extents), class 0 the winner
  {
    const int p = 20 * c.na;  // pixel 20 of the 8x8 level
    struct { const char* what; float an[4]; } ed[3] = {
        {"bw_over_w_eq_1", {0.f, 0.f, 64.f, 64.f}},
        {"area_eq_100", {3.f, 3.f, 13.f, 13.f}},
        {"area_just_above_100", {3.f, 3.f, 13.f, 13.f + 1.9073486328125e-6f}}};
    for (int i = 0; i < 3 && i < std::max(c.na, 3); ++i) {
      const int a = c.na >= 3 ? p + i : (20 + i) * c.na;
      std::memcpy(&ch.anchors[(size_t)a * 4], ed[i].an, 16);
      zero_reg(b0, a);
      person(b0, a, 1.25f + 0.25f * i);  // (different scores: under mask -1 all three are soft-NMS candidates)
      plant(ed[i].what, b0, a);
    }
  }
  // scores on the thresholds: logit 0 -> 1 / (1 + 1) = 0.5 exactly (>= thresh; not > a 0.5 list threshold)
  {
    const int a = 30 * c.na;
    person(b0, a, 0.f);
    plant("score_eq_half", b0, a);
    if (c.na > 1) { person(b0, a + 1, 1e-7f); plant("score_near_half", b0, a + 1); }  // within the bound of 0.5: under the allowance
  }
  // the image maximum of image 0 shared by three anchors with tied classes: two anchors of one pixel (level 0,
  // pixel 40) and one of the 2x2 level; ties across the 31/32 and 63/64 mask words and with the last class
  {
    const float top = 4.f;
    std::vector<int> ws;
    if (c.na >= 6) ws = {ch.anchor_at(0, 40, 2), ch.anchor_at(0, 40, 5), ch.anchor_at(3, 1, 0)};
    else ws = {ch.anchor_at(0, 40, 0), ch.anchor_at(0, 41, 0), ch.anchor_at(3, 1, 0)};
    for (int b = 0; b < c.B; b += 2) {
      for (size_t i = 0; i < ws.size(); ++i) {
        person(b, ws[i], top);
        float* lg = logits(b, ws[i]);
        if (i == 0 && nc > 32) lg[31] = lg[32] = top;
        else if (i == 0 && nc >= 3) lg[1] = lg[2] = top;
        if (i == 1 && nc > 64) lg[63] = lg[64] = top;
        if (i == 2 && nc >= 2) lg[nc - 1] = top;
        for (int q = 0; q < 4; ++q) ch.box[(size_t)ch.bx_off(b, ws[i]) + q] = 0.0625f;
        plant(i == 0 ? "win_ties_3" : i == 1 ? "win_same_pixel" : "win_other_level", b, ws[i]);
      }
      if (b > 0) break;  // image 2 of three: same plants (a second image with ties)
    }
  }
  store(ch.cls, c.bf);
  store(ch.box, c.bf);
  ch.wpred.resize((size_t)c.K * c.na * nc);
  for (float& x : ch.wpred) x = r.uni(-1.f, 1.f);
  ch.dx0.resize((size_t)dxo);
  for (float& x : ch.dx0) x = r.uni(0.5f, 1.5f);
  return ch;
}

// ---- verdicts -----------------------------------------------------------------------------------------------
struct Verdict {
  std::map<std::string, double> fields;  // ratios (max err / bound) and *_bad counts
  long allow = 0, allow_of = 0;          // anchors under the decision allowance
  bool stopped = false;                  // pre_nms was wrong: nothing downstream was launched
  long nonfinite = 0;
  void ratio(const char* k, double r) {
    double& f = fields[k];
    if (!(r <= f)) f = std::isnan(r) ? kInf : r;
  }
  void bad(const char* k, long n = 1) { fields[k] += (double)n; }
  void touch(const char* k) { fields[k] += 0.0; }
  double allow_share() const { return allow_of ? (double)allow / allow_of : 0.0; }
  bool pass() const {
    if (stopped || allow_share() > 0.01) return false;
    for (auto& kv : fields) {
      const bool is_bad = kv.first.size() > 4 && kv.first.compare(kv.first.size() - 4, 4, "_bad") == 0;
      if (is_bad ? kv.second != 0 : !(kv.second <= 1.0)) return false;
    }
    return true;
  }
};
inline std::string jnum(double x) {
  char b[40];
  if (std::isfinite(x)) snprintf(b, sizeof b, "%.6g", x);
  else snprintf(b, sizeof b, "1e308");
  return b;
}
inline std::string verdict_json(const Verdict& V) {
  std::string s = "\"fields\":{";
  bool first = true;
  for (auto& kv : V.fields) {
    s += std::string(first ? "\"" : ",\"") + kv.first + "\":" + jnum(kv.second);
    first = false;
  }
  s += std::string("},\"stopped\":") + (V.stopped ? "true" : "false") + ",\"allow_share\":" + jnum(V.allow_share());
  return s;
}

// ---- pre_nms --------------------------------------------------------------------------------------------------
struct PreOut {
  std::vector<float> scores, boxes;
  std::vector<int> classes, list, count;
  std::vector<uint8_t> keep;
  void init(int B, int A, bool with_list) {
    scores.assign((size_t)B * A, u2f(kFillWord));
    boxes.assign((size_t)B * A * 4, u2f(kFillWord));
    classes.assign((size_t)B * A, (int)kFillWord);
    keep.assign((size_t)B * A, (uint8_t)0xA5);
    list.assign(with_list ? (size_t)B * A : 0, (int)kFillWord);
    count.assign(with_list ? B : 0, 0);
  }
};

template <class T> struct Dec { T box[4], bh, bw, area, qw, qh, sc; };
template <class T> Dec<T> decode(const float* an, const float* bx, float m, float img_h, float img_w) {
  Dec<T> d;
  const T two(2.0f);
  const T yca = (T(an[0]) + T(an[2])) / two, xca = (T(an[1]) + T(an[3])) / two;
  const T ha = T(an[2]) - T(an[0]), wa = T(an[3]) - T(an[1]);
  const T w = texp(T(bx[3])) * wa, h = texp(T(bx[2])) * ha;
  const T yc = T(bx[0]) * ha + yca, xc = T(bx[1]) * wa + xca;
  d.box[0] = yc - h / two; d.box[1] = xc - w / two; d.box[2] = yc + h / two; d.box[3] = xc + w / two;
  d.sc = T(1.0f) / (T(1.0f) + texp(-T(m)));
  d.bh = d.box[2] - d.box[0];
  d.bw = d.box[3] - d.box[1];
  d.area = d.bh * d.bw;
  d.qw = d.bw / T(img_w);
  d.qh = d.bh / T(img_h);
  return d;
}
// (max, first argmax) of one anchor's logits by the kernel's two halves
inline void argmax2(const float* lg, int nclass, bool second_wins_ties, float& m, int& am) {
  const int hc = (nclass + 1) / 2;
  m = lg[0]; am = 0;
  for (int q = 1; q < hc; ++q) if (lg[q] > m) { m = lg[q]; am = q; }
  if (hc < nclass) {
    float m2 = lg[hc]; int a2 = hc;
    for (int q = hc + 1; q < nclass; ++q) if (lg[q] > m2) { m2 = lg[q]; a2 = q; }
    if (second_wins_ties ? m2 >= m : m2 > m) { m = m2; am = a2; }
  }
}
inline uint8_t keep_bits(int am, bool valid, bool ge, bool person_after) {
  uint8_t kf = 0;
  if (am == 0 && valid) { kf = 1; if (ge) kf |= 2; }
  if (am == 0 && (!person_after || valid)) kf |= 4;
  return kf;
}

// the stand-in: the kernel's tiles, levels and appends in fp32 (tiles in launch order; any order is allowed)
inline void sim_pre_nms(const Chain& ch, PreOut& o, Fault f) {
  const Case& c = ch.c;
  o.init(c.B, ch.A, c.cand_list != 0);
  for (int b = 0; b < c.B; ++b)
    for (int x = ch.ntiles - 1; x >= 0; --x) {  // (descending: the lists come out in another order than the anchors')
      int l = 0;
      while (l + 1 < ch.nlev && (f == F_LEVEL_OFF1 ? x > ch.lev[l + 1].tile0 : x >= ch.lev[l + 1].tile0)) ++l;
      const Lev& L = ch.lev[l];
      const int nloc = ch.nloc(l), a0 = (x - L.tile0) * kPreTile;
      int n = std::min(kPreTile, nloc - a0);
      if (f == F_RAGGED_LAST && n < kPreTile) --n;
      for (int t = 0; t < n; ++t) {
        const int a = L.anchor0 + a0 + t;
        if (a >= ch.A) continue;
        const float* lg = &ch.cls[(size_t)(L.cls_off + ((long)b * nloc + a0 + t) * c.nclass)];
        float m; int am;
        argmax2(lg, c.nclass, f == F_HALF_GE, m, am);
        const Dec<float> d = decode<float>(&ch.anchors[(size_t)a * 4], &ch.box[(size_t)(L.box_off + ((long)b * nloc + a0 + t) * 4)], m, ch.img, ch.img);
        const size_t idx = (size_t)b * ch.A + a;
        o.scores[idx] = d.sc;
        o.classes[idx] = am;
        for (int q = 0; q < 4; ++q) o.boxes[idx * 4 + q] = d.box[q];
        const bool valid = d.qw <= 1.0f && d.qh <= 1.0f && (f == F_AREA_GE ? d.area >= 100.0f : d.area > 100.0f);
        const uint8_t kf = keep_bits(am, valid, d.sc >= c.thresh, f == F_PERSON_AFTER);
        o.keep[idx] = kf;
        const bool want = (c.cand_mask < 0 || (kf & c.cand_mask) != 0) && (f == F_CAND_GE ? d.sc >= c.cand_thresh : d.sc > c.cand_thresh);
        if (c.cand_list && want)
          for (int rep = 0; rep < (f == F_CAND_TWICE ? 2 : 1); ++rep) {
            const int pos = o.count[b]++;
            if (pos < ch.A) o.list[(size_t)b * ch.A + pos] = a;
          }
      }
    }
}

struct PreStats {  // coverage by the reference alone
  long tie_first_half = 0, tie_both_halves = 0, second_greater = 0, all_equal = 0, max_last = 0;
  long keep_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cls_nonzero = 0, sc_eq_thresh = 0, sc_ge = 0, sc_lt = 0;
  long bw_eq_1 = 0, area_eq_100 = 0, area_just_above = 0;
  std::vector<long> cand;  // definite candidates per image
};
struct Gate { bool v, amb; };
inline Gate gate(E q, double thr, int op /*0: <=, 1: >, 2: >=*/) {
  Gate g;
  g.v = op == 0 ? q.v <= thr : op == 1 ? q.v > thr : q.v >= thr;
  g.amb = q.e > 0 && std::fabs(q.v - thr) <= 2 * q.e;
  return g;
}

// returns false when classes, keep bits or lists are not the expected ones (nothing downstream may run)
inline bool check_pre_nms(const Chain& ch, const PreOut& o, Verdict& V, PreStats* st = nullptr) {
  const Case& c = ch.c;
  for (const char* k : {"cls_bad", "score", "box", "keep_bad", "list_bad"}) V.touch(k);
  if (st) st->cand.assign(c.B, 0);
  const int hc = (c.nclass + 1) / 2;
  bool ok = true;
  V.allow_of += (long)c.B * ch.A;
  for (int b = 0; b < c.B; ++b) {
    std::vector<int> in_list(ch.A, 0);
    if (c.cand_list) {
      const int cnt = o.count[b];
      if (cnt < 0 || cnt > ch.A) { V.bad("list_bad"); ok = false; }
      for (int i = 0; i < ch.A; ++i) {
        const int a = o.list[(size_t)b * ch.A + i];
        if (i < std::min(std::max(cnt, 0), ch.A)) {
          if (a < 0 || a >= ch.A || in_list[a]) { V.bad("list_bad"); ok = false; }
          else in_list[a] = 1;
        } else if (a != (int)kFillWord) { V.bad("list_bad"); ok = false; }  // entries past the count keep their fill
      }
    }
    for (int a = 0; a < ch.A; ++a) {
      const size_t idx = (size_t)b * ch.A + a;
      const float* lg = &ch.cls[(size_t)ch.lg_off(b, a)];
      float m; int am;
      argmax2(lg, c.nclass, false, m, am);
      if (o.classes[idx] != am) { V.bad("cls_bad"); ok = false; }
      const float* an = &ch.anchors[(size_t)a * 4];
      const float* bx = &ch.box[(size_t)ch.bx_off(b, a)];
      const Dec<E> d = decode<E>(an, bx, m, ch.img, ch.img);
      V.ratio("score", ratio_of(o.scores[idx], d.sc));
      for (int q = 0; q < 4; ++q) V.ratio("box", ratio_of(o.boxes[idx * 4 + q], d.box[q]));
      const Gate g[5] = {gate(d.qw, 1.0, 0), gate(d.qh, 1.0, 0), gate(d.area, 100.0, 1), gate(d.sc, c.thresh, 2), gate(d.sc, c.cand_thresh, 1)};
      // every outcome of the ambiguous gates (a gate that cannot reach the result is not counted as ambiguous)
      uint8_t allowed[2] = {0, 0};
      for (int mask = 0; mask < 32; ++mask) {
        bool v[5], legal = true;
        for (int i = 0; i < 5; ++i) {
          v[i] = g[i].v != (bool)(mask >> i & 1);
          legal &= g[i].amb || !(mask >> i & 1);
        }
        if (!legal) continue;
        const uint8_t kf = keep_bits(am, v[0] && v[1] && v[2], v[3], false);
        const bool want = (c.cand_mask < 0 || (kf & c.cand_mask) != 0) && v[4];
        allowed[want] |= (uint8_t)(1u << kf);
      }
      const bool amb = (allowed[0] | allowed[1]) & ((allowed[0] | allowed[1]) - 1) || (c.cand_list && allowed[0] && allowed[1]);
      V.allow += amb;
      const uint8_t kf = o.keep[idx];
      if (kf > 7 || !((allowed[0] | allowed[1]) >> kf & 1)) { V.bad("keep_bad"); ok = false; }
      else if (c.cand_list && !(allowed[in_list[a]] >> kf & 1)) { V.bad("list_bad"); ok = false; }
      if (st) {
        int nmax_first = 0, nmax_second = 0, nmax = 0;
        for (int q = 0; q < c.nclass; ++q) if (lg[q] == m) { ++nmax; (q < hc ? nmax_first : nmax_second)++; }
        st->all_equal += nmax == c.nclass && c.nclass > 1;
        st->tie_first_half += nmax_first >= 2 && nmax < c.nclass;
        st->tie_both_halves += nmax_first >= 1 && nmax_second >= 1;
        st->second_greater += nmax_first == 0;
        st->max_last += am == c.nclass - 1 && c.nclass > 1;
        const Dec<float> df = decode<float>(an, bx, m, ch.img, ch.img);
        const bool valid = df.qw <= 1.0f && df.qh <= 1.0f && df.area > 100.0f;
        st->keep_hist[keep_bits(am, valid, df.sc >= c.thresh, false)]++;
        st->cls_nonzero += am != 0;
        st->sc_eq_thresh += df.sc == c.thresh;
        st->sc_ge += df.sc >= c.thresh;
        st->sc_lt += df.sc < c.thresh;
        st->bw_eq_1 += df.qw == 1.0f && !g[0].amb;
        st->area_eq_100 += df.area == 100.0f && !g[2].amb;
        st->area_just_above += df.area > 100.0f && df.area < 100.001f && !g[2].amb;
        st->cand[b] += allowed[1] && !allowed[0];
      }
    }
  }
  if (!ok) V.stopped = true;
  return ok;
}

// ---- soft-NMS: TF's NonMaxSuppressionV5 lazy queue in fp32, TF's product order --------------------------------
struct NmsIn {
  int B = 0, N = 0, max_out = 100;
  float thresh = 0.001f, sigma = 0.5f, clip = 64.f;
  std::vector<float> boxes, scores;
  std::vector<std::vector<int>> cand;  // per image, ascending index: the candidates (score > thresh applied)
};
struct NmsOut {
  std::vector<float> boxes, scores;
  std::vector<int> count, index, cand_count;  // index empty: no selected-index output; cand_count: after the run
};
struct NmsStats {
  double min_margin = kInf;  // smallest (relative margin to a flipped decision) / (the products' relative bound)
  double min_arg = kInf;     // smallest |scale iou^2| of an overlapping pair: expf of it must differ from 1
  long pops = 0, requeues = 0, tie_pops = 0, dup_visits = 0, max_first_overlaps = 0, selected = 0, candidates = 0;
};
inline float tf_iou(const float* bi, const float* bj) {
  const float ymin_i = fminf(bi[0], bi[2]), xmin_i = fminf(bi[1], bi[3]);
  const float ymax_i = fmaxf(bi[0], bi[2]), xmax_i = fmaxf(bi[1], bi[3]);
  const float ymin_j = fminf(bj[0], bj[2]), xmin_j = fminf(bj[1], bj[3]);
  const float ymax_j = fmaxf(bj[0], bj[2]), xmax_j = fmaxf(bj[1], bj[3]);
  const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
  const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
  if (area_i <= 0.f || area_j <= 0.f) return 0.f;
  const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
  const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
  const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
  return inter / (area_i + area_j - inter);
}
struct NmsImg {
  std::vector<int> sel;
  std::vector<float> sc;
  std::vector<E> scE;
};
// One image.  The decay argument scale * iou * iou is made of basic operations on the inputs, so it is the same
// fp32 number on every conforming evaluation; only expf differs.  The E product carries expf's bound per factor
// other than exp(0) and one rounding per multiply.
inline NmsImg nms_image(const NmsIn& in, int b, Fault f = F_NONE, NmsStats* st = nullptr) {
  NmsImg R;
  const std::vector<int>& cd = in.cand[b];
  const int n = (int)cd.size();
  const float* bb = &in.boxes[(size_t)b * in.N * 4];
  const float* sb = &in.scores[(size_t)b * in.N];
  const float scale = in.sigma > 0.f ? -0.5f / in.sigma : 0.f;
  std::vector<float> s(n);
  std::vector<E> se(n);
  std::vector<int> from(n, 0);
  std::vector<char> decayed(n, 0), popped(n, 0);
  for (int i = 0; i < n; ++i) { s[i] = sb[cd[i]]; se[i] = E(s[i], 0); }
  if (st) st->candidates += n;
  auto better = [&](int i, int j) {  // i before j in the queue
    if (s[i] != s[j]) return s[i] > s[j];
    return f == F_NMS_TIE_HI ? i > j : i < j;
  };
  while ((int)R.sel.size() < in.max_out) {
    int top = -1, second = -1;
    for (int i = 0; i < n; ++i) {
      if (s[i] <= 0.f) continue;
      if (top < 0 || better(i, top)) { second = top; top = i; }
      else if (second < 0 || better(i, second)) second = i;
    }
    if (top < 0) break;
    const float orig = s[top];
    if (!(orig > in.thresh)) break;
    if (st) {
      ++st->pops;
      if (second >= 0 && s[second] == orig) ++st->tie_pops;
      if (second >= 0 && (decayed[top] || decayed[second])) {
        const double rel = std::fabs(se[top].v - se[second].v) / se[top].v;
        const double bound = se[top].e / se[top].v + se[second].e / se[second].v;
        st->min_margin = std::min(st->min_margin, bound > 0 ? rel / bound : kInf);
      }
    }
    float sc = orig;
    E sce = se[top];
    const int nsel = (int)R.sel.size();
    int novl = 0;
    for (int j = nsel - 1; j >= from[top]; --j) {
      const float sim = tf_iou(bb + (size_t)cd[top] * 4, bb + (size_t)R.sel[j] * 4);
      const float arg = scale * sim * sim;
      if (arg != 0.f) {
        ++novl;
        if (st) {
          st->min_arg = std::min(st->min_arg, (double)std::fabs(arg));
          st->dup_visits += sim == 1.0f;
        }
        sc *= expf(arg);
        sce = sce * texp(E(arg, 0));
      }
      if (sc <= in.thresh) break;
    }
    if (st) {
      if (!popped[top]) st->max_first_overlaps = std::max<long>(st->max_first_overlaps, novl);
      if (novl) {
        const double rel = std::fabs(sce.v - in.thresh) / sce.v;
        st->min_margin = std::min(st->min_margin, sce.e > 0 ? rel / (sce.e / sce.v) : kInf);
      }
    }
    popped[top] = 1;
    if (sc == orig) {
      R.sel.push_back(cd[top]);
      R.sc.push_back(sc);
      R.scE.push_back(se[top]);
      s[top] = 0.f;
    } else if (sc > in.thresh) {
      s[top] = sc;
      se[top] = sce;
      decayed[top] = 1;
      from[top] = nsel;
      if (st) ++st->requeues;
    } else {
      s[top] = 0.f;
    }
  }
  if (st) st->selected += (long)R.sel.size();
  return R;
}
inline void sim_soft_nms(const NmsIn& in, bool with_index, bool with_list, NmsOut& o, Fault f) {
  o.boxes.assign((size_t)in.B * in.max_out * 4, u2f(kFillWord));
  o.scores.assign((size_t)in.B * in.max_out, u2f(kFillWord));
  o.count.assign(in.B, (int)kFillWord);
  o.index.assign(with_index ? (size_t)in.B * in.max_out : 0, (int)kFillWord);
  o.cand_count.clear();
  for (int b = 0; b < in.B; ++b) {
    const NmsImg R = nms_image(in, b, f);
    for (int k = 0; k < in.max_out; ++k) {
      const size_t r = (size_t)b * in.max_out + k;
      if (k < (int)R.sel.size()) {
        for (int q = 0; q < 4; ++q) {
          const float v = in.boxes[((size_t)b * in.N + R.sel[k]) * 4 + q];
          o.boxes[r * 4 + q] = f == F_NO_CLIP ? v : fminf(fmaxf(v, 0.0f), in.clip);
        }
        o.scores[r] = R.sc[k];
        if (with_index) o.index[r] = R.sel[k];
      } else {
        for (int q = 0; q < 4; ++q) o.boxes[r * 4 + q] = 0.f;
        o.scores[r] = 0.f;
        if (with_index) o.index[r] = -1;
      }
    }
    o.count[b] = (int)R.sel.size();
    if (with_list) o.cand_count.push_back(f == F_COUNT_KEEP ? (int)in.cand[b].size() : 0);
  }
}
inline void check_soft_nms(const NmsIn& in, const NmsOut& o, Verdict& V, NmsStats* st = nullptr) {
  for (const char* k : {"nms_index_bad", "nms_count_bad", "nms_box_bad", "nms_score", "nms_tail_bad", "nms_reset_bad"}) V.touch(k);
  for (int b = 0; b < in.B; ++b) {
    const NmsImg R = nms_image(in, b, F_NONE, st);
    const int cnt = (int)R.sel.size();
    if (o.count[b] != cnt) V.bad("nms_count_bad");
    for (int k = 0; k < in.max_out; ++k) {
      const size_t r = (size_t)b * in.max_out + k;
      if (k < cnt) {
        if (!o.index.empty() && o.index[r] != R.sel[k]) V.bad("nms_index_bad");
        for (int q = 0; q < 4; ++q) {
          const float want = fminf(fmaxf(in.boxes[((size_t)b * in.N + R.sel[k]) * 4 + q], 0.0f), in.clip);
          if (f2u(o.boxes[r * 4 + q]) != f2u(want)) V.bad("nms_box_bad");
        }
        V.ratio("nms_score", ratio_of(o.scores[r], R.scE[k]));
      } else {
        for (int q = 0; q < 4; ++q) if (f2u(o.boxes[r * 4 + q]) != 0u) V.bad("nms_tail_bad");
        if (f2u(o.scores[r]) != 0u) V.bad("nms_tail_bad");
        if (!o.index.empty() && o.index[r] != -1) V.bad("nms_tail_bad");
      }
    }
  }
  for (int x : o.cand_count) if (x != 0) V.bad("nms_reset_bad");
}
// direct soft-NMS inputs: integer box corners (every overlap's decay argument is far from 0), scores in (0, 1)
inline NmsIn make_nms(const Case& c, std::vector<uint8_t>& keep, std::vector<int>& count) {
  NmsIn in;
  in.B = c.B; in.N = c.N; in.max_out = c.max_out; in.thresh = 0.001f; in.sigma = 0.5f; in.clip = 300.f;
  Rng r(c.seed);
  in.boxes.resize((size_t)c.B * c.N * 4);
  in.scores.resize((size_t)c.B * c.N);
  keep.assign(c.nms_mode == NM_PREFIX ? 0 : (size_t)c.B * c.N, 0);
  count.clear();
  const int span = c.nms_mode == NM_M2 ? 2000 : 320;
  for (int b = 0; b < c.B; ++b)
    for (int i = 0; i < c.N; ++i) {
      const size_t e = (size_t)b * c.N + i;
      const int y = r.below(span) - 8, x = r.below(span) - 8, h = 4 + r.below(28), w = 4 + r.below(28);
      float* bx = &in.boxes[e * 4];
      bx[0] = (float)y; bx[1] = (float)x; bx[2] = (float)(y + h); bx[3] = (float)(x + w);
      if (r.below(16) == 0) std::swap(bx[0], bx[2]);  // corners in either order (TF sorts them)
      in.scores[e] = r.below(50) == 0 ? 0.0005f : r.uni(0.002f, 0.999f);
      if (c.nms_mode == NM_M2) keep[e] = (r.below(87) == 0 ? 1 : 0) | (r.below(3) ? 2 : 0) | 4;
      else if (c.nms_mode == NM_MASK) keep[e] = (r.below(4) ? 1 : 0) | (r.below(2) ? 6 : 0);
    }
  if (c.plant && c.N >= 512) {
    // image 0: score ties broken by candidate order, duplicate boxes, and one low-scoring box over 30 disjoint
    // selections (more than kNmsFl decay factors before its first pop)
    float* bx = &in.boxes[0];
    float* sc = &in.scores[0];
    const float q4[4] = {0.9996f, 0.9997f, 0.9998f, 0.9999f};
    for (int i = 0; i < 64; ++i) { sc[100 + i] = q4[i % 4]; keep[100 + i] |= 1; }
    for (int i = 0; i < 12; ++i) {
      float* a4 = bx + (size_t)(200 + 2 * i) * 4;
      if (i % 2) { a4[0] = 600.f + 40 * i; a4[1] = 600.f; a4[2] = a4[0] + 10.f; a4[3] = 610.f; }  // away from every other box
      std::memcpy(a4 + 4, a4, 16);
      keep[200 + 2 * i] |= 1; keep[200 + 2 * i + 1] |= 1;
      sc[200 + 2 * i] = 0.9987f - 0.0003f * i;
      sc[200 + 2 * i + 1] = i % 2 ? sc[200 + 2 * i] : sc[200 + 2 * i] - 0.00005f;
    }
    for (int i = 0; i < 30; ++i) {
      float* s4 = bx + (size_t)(300 + i) * 4;
      s4[0] = 400.f + 8 * (i / 6); s4[1] = 400.f + 8 * (i % 6); s4[2] = s4[0] + 4.f; s4[3] = s4[1] + 4.f;
      sc[300 + i] = 0.99955f - 2e-6f * i;
      keep[300 + i] |= 1;
    }
    float* big = bx + (size_t)400 * 4;
    big[0] = 396.f; big[1] = 396.f; big[2] = 460.f; big[3] = 460.f;
    sc[400] = 0.99935f;
    keep[400] |= 1;
  }
  if (c.nms_mode == NM_PREFIX) count = c.counts;
  in.cand.assign(c.B, {});
  for (int b = 0; b < c.B; ++b) {
    const int n_in = c.nms_mode == NM_PREFIX ? std::min(count[b], c.N) : c.N;
    for (int i = 0; i < n_in; ++i) {
      const size_t e = (size_t)b * c.N + i;
      if (in.scores[e] > in.thresh && (keep.empty() || (keep[e] & 1))) in.cand[b].push_back(i);
    }
  }
  return in;
}

// ---- per-image max ---------------------------------------------------------------------------------------------
struct ImaxOut { std::vector<float> m; std::vector<int> argm, nties; };
inline void ref_image_max(const float* scores, const uint8_t* keep, int B, int A, ImaxOut& o) {
  o.m.assign(B, -FLT_MAX); o.argm.assign(B, -1); o.nties.assign(B, 0);
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < A; ++a) {
      const size_t e = (size_t)b * A + a;
      if (!(keep[e] & 1)) continue;
      const float v = scores[e];
      if (o.argm[b] < 0 || v > o.m[b]) { o.m[b] = v; o.argm[b] = a; o.nties[b] = 1; }
      else if (v == o.m[b]) ++o.nties[b];
    }
}
inline void sim_image_max(const float* scores, const uint8_t* keep, int B, int A, ImaxOut& o, Fault f) {
  o.m.assign(B, -FLT_MAX); o.argm.assign(B, -1); o.nties.assign(B, 0);
  const int per = (A + kImaxChunks - 1) / kImaxChunks;
  for (int b = 0; b < B; ++b) {
    float mx = -FLT_MAX; int mi = 0x7fffffff, cnt = 0;
    for (int chn = 0; chn < kImaxChunks; ++chn) {
      const int a0 = chn * per, a1 = std::min(A, a0 + per);
      float best = -FLT_MAX; int bi = 0x7fffffff, n = 0;
      for (int a = a0; a < a1; ++a) {
        const size_t e = (size_t)b * A + a;
        if (!(keep[e] & 1)) continue;
        const float v = scores[e];
        if (bi == 0x7fffffff || v > best || (f == F_IMAX_FIRST && v == best)) { best = v; bi = a; }
      }
      if (bi == 0x7fffffff) continue;
      for (int a = a0; a < a1; ++a) n += (keep[(size_t)b * A + a] & 1) && scores[(size_t)b * A + a] == best;
      if (mi == 0x7fffffff || best > mx) { mx = best; mi = bi; cnt = n; }
      else if (best == mx) { mi = f == F_IMAX_FIRST ? std::max(mi, bi) : std::min(mi, bi); cnt = f == F_IMAX_NOADD ? cnt : cnt + n; }
    }
    if (mi != 0x7fffffff) { o.m[b] = mx; o.argm[b] = mi; o.nties[b] = cnt; }
  }
}
struct ImaxStats { long empty_images = 0, ties_in_chunk = 0, ties_2_chunks = 0, ties_3_chunks = 0, empty_chunks = 0, max_zero = 0, max_neg = 0, bits_without_1 = 0; };
inline void check_image_max(const float* scores, const uint8_t* keep, int B, int A, const ImaxOut& o, Verdict& V, ImaxStats* st = nullptr) {
  V.touch("imax_exact_bad");
  ImaxOut r;
  ref_image_max(scores, keep, B, A, r);
  for (int b = 0; b < B; ++b) {
    if (f2u(o.m[b]) != f2u(r.m[b])) V.bad("imax_exact_bad");
    if (o.argm[b] != r.argm[b]) V.bad("imax_exact_bad");
    if (o.nties[b] != r.nties[b]) V.bad("imax_exact_bad");
    if (st) {
      const int per = (A + kImaxChunks - 1) / kImaxChunks;
      std::set<int> chunks;
      bool two_in_one = false;
      for (int a = 0; a < A; ++a) {
        const size_t e = (size_t)b * A + a;
        st->bits_without_1 += (keep[e] & 6) && !(keep[e] & 1) && scores[e] > r.m[b];
        if ((keep[e] & 1) && scores[e] == r.m[b]) two_in_one |= !chunks.insert(a / per).second;
      }
      st->empty_images += r.argm[b] < 0;
      st->ties_in_chunk += two_in_one;
      st->ties_2_chunks += chunks.size() == 2;
      st->ties_3_chunks += chunks.size() >= 3;
      st->max_zero += r.argm[b] >= 0 && r.m[b] == 0.f;
      st->max_neg += r.argm[b] >= 0 && r.m[b] < 0.f;
      if (b == 0) for (int chn = 0; chn < kImaxChunks; ++chn) st->empty_chunks += chn * per >= A;
    }
  }
}

// ---- loss --------------------------------------------------------------------------------------------------------
struct LossOut { std::vector<float> dm, metrics; float dscale = 0; };
template <class T> struct LossRef { std::vector<T> dm; T dscale, loss, scale_loss, sm, sm2; };
template <class T> LossRef<T> ref_loss(const float* mraw, int B, float s, Fault f = F_NONE) {
  LossRef<T> r;
  T sum_sq(0.f), scale_loss(0.f), sm(0.f), sm2(0.f), dsc(0.f);
  for (int b = 0; b < B; ++b) {
    const float raw = mraw[b];
    const T mb(raw > 0.0f ? raw : 0.0f);  // max(raw, 0): +0 for raw == -0 (the sign of that zero reaches no output)
    const T d = mb - T(s);
    sum_sq = sum_sq + mb * mb;
    scale_loss = scale_loss + d * d;
    sm = sm + mb;
    sm2 = sm2 + mb * mb;
    dsc = dsc + T(-2.0f) * d;
    const bool on = f == F_LOSS_GRAD0 ? raw > 0.0f : raw >= 0.0f;
    r.dm.push_back(on ? T(2.0f) * mb + T(2.0f) * d : T(0.0f));
  }
  r.dscale = dsc; r.loss = sum_sq + scale_loss; r.scale_loss = scale_loss; r.sm = sm; r.sm2 = sm2;
  return r;
}
inline std::vector<float> metrics0() {
  std::vector<float> m(kNMetric);
  for (int i = 0; i < kNMetric; ++i) m[i] = 100.f + i;
  return m;
}
inline void sim_loss(const float* mraw, int B, float s, LossOut& o, Fault f) {
  const LossRef<float> r = ref_loss<float>(mraw, B, s, f);
  o.dm = r.dm; o.dscale = r.dscale; o.metrics = metrics0();
  o.metrics[M_LOSS] = r.loss; o.metrics[M_SCALE_LOSS] = r.scale_loss; o.metrics[M_SUM_M] = r.sm; o.metrics[M_SUM_M2] = r.sm2;
  o.metrics[M_NIMG] = (float)B;
}
inline void check_loss(const float* mraw, int B, float s, const LossOut& o, Verdict& V) {
  for (const char* k : {"loss", "loss_exact_bad", "metrics_other_bad"}) V.touch(k);
  const LossRef<float> rf = ref_loss<float>(mraw, B, s);
  const LossRef<E> re = ref_loss<E>(mraw, B, s);
  auto one = [&](float got, float exact, E want) {
    V.ratio("loss", ratio_of(got, want));
    if (got != exact) V.bad("loss_exact_bad");  // (== : a zero of either sign is the same gradient)
  };
  for (int b = 0; b < B; ++b) one(o.dm[b], rf.dm[b], re.dm[b]);
  one(o.dscale, rf.dscale, re.dscale);
  one(o.metrics[M_LOSS], rf.loss, re.loss);
  one(o.metrics[M_SCALE_LOSS], rf.scale_loss, re.scale_loss);
  one(o.metrics[M_SUM_M], rf.sm, re.sm);
  one(o.metrics[M_SUM_M2], rf.sm2, re.sm2);
  one(o.metrics[M_NIMG], (float)B, E((double)B, 0));
  const std::vector<float> m0 = metrics0();
  for (int i = 0; i < kNMetric; ++i)
    if (i != M_LOSS && i != M_SCALE_LOSS && i != M_SUM_M && i != M_SUM_M2 && i != M_NIMG && f2u(o.metrics[i]) != f2u(m0[i])) V.bad("metrics_other_bad");
}

// ---- count_ge ------------------------------------------------------------------------------------------------------
inline float ref_count_ge(const float* sc, const int* cnt, int B, int maxo, float th) {
  int n = 0;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < cnt[b]; ++k) n += sc[(size_t)b * maxo + k] >= th;
  return (float)n;
}
inline void check_count_ge(const float* sc, const int* cnt, int B, int maxo, float th, float got, Verdict& V) {
  V.touch("count_ge_exact_bad");
  if (f2u(got) != f2u(ref_count_ge(sc, cnt, B, maxo, th))) V.bad("count_ge_exact_bad");
}

// ---- zero_segs: the segments zero, every other byte as filled ---------------------------------------------------
struct Segs { std::vector<size_t> off, bytes; size_t total = 0; };
inline Segs make_segs(int nseg) {
  Segs s;
  const size_t sizes[9] = {16, 4096 + 16, 48, 1024, 16, 65536 + 32, 160, 16 * 257, 64};
  size_t o = 32;
  for (int i = 0; i < nseg; ++i) {
    s.off.push_back(o);
    s.bytes.push_back(sizes[i % 9]);
    o += sizes[i % 9] + 16 * (1 + i % 3);  // gaps: the neighbours of each segment
  }
  s.total = o + 16;
  return s;
}
inline void check_zero_segs(const Segs& s, const uint8_t* fill, const uint8_t* got, Verdict& V) {
  V.touch("zero_bad");
  std::vector<uint8_t> want(fill, fill + s.total);
  for (size_t i = 0; i < s.off.size(); ++i) std::memset(want.data() + s.off[i], 0, s.bytes[i]);
  for (size_t i = 0; i < s.total; ++i) if (got[i] != want[i]) V.bad("zero_bad");
}

// ---- the sparse class-head backward ---------------------------------------------------------------------------------
struct ScatterIn {
  const Chain* ch;
  const float* scores;
  const uint8_t* keep;
  const float* mraw;
  const int* nties;
  const float* dm;
};
template <class T> void ref_cls_scatter(const ScatterIn& si, std::vector<T>& dx, std::vector<char>& touched, Fault f = F_NONE) {
  const Chain& ch = *si.ch;
  const Case& c = ch.c;
  dx.clear();
  for (float x : ch.dx0) dx.push_back(T(x));
  touched.assign(ch.dx0.size(), 0);
  const int N = c.na * c.nclass;
  for (int b = 0; b < c.B; ++b) {
    if (si.dm[b] == 0.0f) continue;
    const float mx = si.mraw[b];
    const T ds = T(si.dm[b]) / T((float)si.nties[b]);
    for (int p = 0; p < ch.PT; ++p) {
      const int l = ch.level_of(p * c.na);
      const Lev& L = ch.lev[l];
      const int pix = p - L.anchor0 / c.na;
      const long prow = (long)b * L.h * L.w + pix;
      T* row = &dx[(size_t)(ch.dx_off[l] + prow * c.K)];
      char* trow = &touched[(size_t)(ch.dx_off[l] + prow * c.K)];
      const long abase = (long)b * ch.A + L.anchor0 + (long)pix * c.na;
      for (int k = 0; k < c.na; ++k) {
        if (!((si.keep[abase + k] & 1) && si.scores[abase + k] == mx)) continue;
        const T s(si.scores[abase + k]);
        const T dl = ds * s * (T(1.0f) - s);
        const float* lg = &ch.cls[(size_t)(L.cls_off + prow * N + (long)k * c.nclass)];
        float m = lg[0];
        for (int q = 1; q < c.nclass; ++q) m = fmaxf(m, lg[q]);
        int nt = 0;
        for (int q = 0; q < c.nclass; ++q) nt += lg[q] == m;
        const T dlc = f == F_TIE_NODIV ? dl : dl / T((float)nt);
        for (int q = 0; q < c.nclass; ++q) {
          if (lg[q] != m) continue;
          const int col = k * c.nclass + q;
          for (int j = 0; j < c.K; ++j) {
            const T add = T(ch.wpred[(size_t)j * N + col]) * dlc;
            row[j] = f == F_DX_OVERWRITE ? add : row[j] + add;
            trow[j] = 1;
          }
          if (f == F_TIE_FIRST) break;
        }
      }
    }
  }
}
struct ScatterStats { long rows_written = 0, win_anchors = 0, max_class_ties = 0, pixels_2_winners = 0, levels_hit = 0, images_dm0 = 0; };
inline void check_cls_scatter(const ScatterIn& si, const std::vector<float>& got, Verdict& V, ScatterStats* st = nullptr) {
  for (const char* k : {"dx", "dx_exact_bad", "dx_untouched_bad"}) V.touch(k);
  std::vector<E> re;
  std::vector<float> rf;
  std::vector<char> touched, t2;
  ref_cls_scatter<E>(si, re, touched);
  ref_cls_scatter<float>(si, rf, t2);
  const Chain& ch = *si.ch;
  for (size_t i = 0; i < got.size(); ++i) {
    if (!touched[i]) {
      if (f2u(got[i]) != f2u(ch.dx0[i])) V.bad("dx_untouched_bad");
      continue;
    }
    V.ratio("dx", ratio_of(got[i], re[i]));
    if (f2u(got[i]) != f2u(rf[i])) V.bad("dx_exact_bad");
  }
  if (st) {
    const Case& c = ch.c;
    std::set<int> levels;
    for (int b = 0; b < c.B; ++b) {
      st->images_dm0 += si.dm[b] == 0.0f;
      if (si.dm[b] == 0.0f) continue;
      for (int p = 0; p < ch.PT; ++p) {
        int w = 0;
        for (int k = 0; k < c.na; ++k) {
          const size_t e = (size_t)b * ch.A + (size_t)p * c.na + k;
          if ((si.keep[e] & 1) && si.scores[e] == si.mraw[b]) {
            ++w;
            const float* lg = &ch.cls[(size_t)ch.lg_off(b, p * c.na + k)];
            float m = lg[0];
            for (int q = 1; q < c.nclass; ++q) m = fmaxf(m, lg[q]);
            long nt = 0;
            for (int q = 0; q < c.nclass; ++q) nt += lg[q] == m;
            st->max_class_ties = std::max(st->max_class_ties, nt);
          }
        }
        st->win_anchors += w;
        st->pixels_2_winners += w >= 2;
        st->rows_written += w > 0;
        if (w) levels.insert(ch.level_of(p * c.na));
      }
    }
    st->levels_hit = (long)levels.size();
  }
}

// ---- Adam ------------------------------------------------------------------------------------------------------------
struct AdamIO { std::vector<float> p, g, m, v; };
inline float adam_alpha(float lr, int64_t t) {  // the launcher's host arithmetic
  const float b1p = powf(0.9f, (float)t), b2p = powf(0.999f, (float)t);
  return lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
}
template <class T> void ref_adam(const AdamIO& in, float alpha, long npatch, std::vector<T>& p, std::vector<T>& m, std::vector<T>& v, Fault f = F_NONE) {
  const size_t n = in.p.size();
  p.resize(n); m.resize(n); v.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const T g(in.g[i]);
    T mi(in.m[i]), vi(in.v[i]);
    mi = mi + (g - mi) * T(1.0f - 0.9f);
    vi = vi + (g * g - vi) * T(1.0f - 0.999f);
    m[i] = mi; v[i] = vi;
    T x = T(in.p[i]) - (mi * T(alpha)) / (tsqrt(vi) + T(1e-7f));
    if (npatch >= 0) {
      if ((long)i < npatch || f == F_ADAM_SCALE_CLIP) x = tmin(tmax(x, T(-1.0f)), T(1.0f));
      else x = tmin(tmax(x, T(0.0f)), T(1.0f));
    }
    p[i] = x;
  }
}
inline AdamIO make_adam(const Case& c) {
  AdamIO io;
  Rng r(c.seed);
  const size_t n = (size_t)c.n;
  io.p.resize(n); io.g.resize(n); io.m.resize(n); io.v.resize(n);
  if (c.clip) {
    // the patch part is large: most of it idle (g = m = v = 0: 0 / eps, the value unchanged), a random slice live
    for (size_t i = 0; i < n; ++i) io.p[i] = ((i * 2654435761u) >> 8 & 0xffff) / 32768.0f - 1.0f;
    for (size_t i = 0; i < 4096 && i < n; ++i) {
      const size_t e = (i * 293) % (n - 1);
      io.g[e] = r.uni(-1.f, 1.f); io.m[e] = r.uni(-0.5f, 0.5f); io.v[e] = r.uni(0.f, 0.5f);
    }
    // updates that cross -1 and +1 in the patch part, 0 and 1 in the scale slot
    io.p[0] = -0.99995f; io.g[0] = 1.f; io.m[0] = 1.f; io.v[0] = 1.f;
    io.p[1] = 0.99995f; io.g[1] = -1.f; io.m[1] = -1.f; io.v[1] = 1.f;
    io.p[2] = -0.5f; io.g[2] = 1.f; io.m[2] = 1.f; io.v[2] = 1.f;   // stays inside, below 0: the patch keeps negatives
    io.p[n - 1] = c.t == 1 ? 0.00005f : 0.99995f;
    io.g[n - 1] = c.t == 1 ? 1.f : -1.f; io.m[n - 1] = io.g[n - 1]; io.v[n - 1] = 1.f;
    return io;
  }
  for (size_t i = 0; i < n; ++i) {
    io.p[i] = r.uni(-2.f, 2.f); io.g[i] = r.uni(-1.f, 1.f); io.m[i] = r.uni(-0.5f, 0.5f); io.v[i] = r.uni(0.f, 0.5f);
  }
  io.g[0] = 0.f; io.m[0] = 0.f; io.v[0] = 0.f;  // v = 0 with g = 0: 0 / eps
  if (n > 1) { io.g[n - 1] = 1e-4f; io.m[n - 1] = 0.f; io.v[n - 1] = 0.f; }
  return io;
}
inline void check_adam(const AdamIO& in, float alpha, long npatch, const AdamIO& got, Verdict& V) {
  for (const char* k : {"adam", "adam_exact_bad"}) V.touch(k);
  std::vector<E> pe, me, ve;
  std::vector<float> pf, mf, vf;
  ref_adam<E>(in, alpha, npatch, pe, me, ve);
  ref_adam<float>(in, alpha, npatch, pf, mf, vf);
  for (size_t i = 0; i < in.p.size(); ++i) {
    V.ratio("adam", ratio_of(got.p[i], pe[i]));
    V.ratio("adam", ratio_of(got.m[i], me[i]));
    V.ratio("adam", ratio_of(got.v[i], ve[i]));
    if (got.p[i] != pf[i] || got.m[i] != mf[i] || got.v[i] != vf[i]) V.bad("adam_exact_bad");
  }
}

// ---- direct image_max / loss / count_ge inputs ------------------------------------------------------------------------
inline void make_imax(const Case& c, std::vector<float>& scores, std::vector<uint8_t>& keep) {
  const int A = c.N, B = c.B;
  Rng r(c.seed);
  scores.resize((size_t)B * A);
  keep.resize((size_t)B * A);
  for (size_t i = 0; i < scores.size(); ++i) {
    scores[i] = r.uni(-0.5f, 0.9f);
    keep[i] = (uint8_t)r.below(8);
  }
  const int per = (A + kImaxChunks - 1) / kImaxChunks;
  auto put = [&](int b, int a, float v, uint8_t k) { if (b < B && a < A) { scores[(size_t)b * A + a] = v; keep[(size_t)b * A + a] = k; } };
  // image 0: the maximum tied inside one chunk and across three chunks; higher values with bits 2 / 4 only
  put(0, A - 1, 0.95f, 1); put(0, std::max(0, A - 2), 0.95f, 3);
  put(0, std::min(A - 1, 2 * per + 1), 0.95f, 5); put(0, std::min(A - 1, per), 0.95f, 7);
  put(0, 0, 0.99f, 6); put(0, std::min(A - 1, 3), 0.99f, 4);
  if (B >= 2) {  // image 1: no kept anchor
    for (int a = 0; a < A; ++a) keep[(size_t)A + a] &= 6;
  }
  if (B >= 3) {  // image 2: a maximum of exactly 0 shared by 0.0 and -0.0 across two chunks, the rest negative
    for (int a = 0; a < A; ++a) scores[(size_t)2 * A + a] = -std::fabs(scores[(size_t)2 * A + a]) - 0.01f;
    put(2, std::min(A - 1, per + 2), 0.0f, 1); put(2, std::min(A - 1, 5 * per), -0.0f, 1);
  }
  if (B >= 4) {  // image 3: every score negative
    for (int a = 0; a < A; ++a) scores[(size_t)3 * A + a] = -std::fabs(scores[(size_t)3 * A + a]) - 0.01f;
  }
}

inline std::vector<float> make_mraw() { return {0.7f, 0.0f, -0.0f, -0.3f, -FLT_MAX, 0.25f}; }
inline void make_count(const Case& c, std::vector<float>& sc, std::vector<int>& cnt) {
  Rng r(c.seed);
  cnt = {0, 3, c.max_out, std::min(5, c.max_out)};
  sc.resize((size_t)4 * c.max_out);
  for (float& x : sc) x = r.uni(0.f, 1.f);
  sc[(size_t)1 * c.max_out + 1] = 0.5f;   // exactly on the threshold: counted
  sc[(size_t)1 * c.max_out + 2] = 0.49999997f;
  for (int k = 3; k < c.max_out; ++k) sc[(size_t)1 * c.max_out + k] = 0.9f;  // rows past the count: ignored
  for (int k = 0; k < c.max_out; ++k) sc[k] = 0.75f;                          // an image with count 0
}

// ---- the expf figure: max |f(x) - exp(x)| in ulps over the arguments the table uses ------------------------------
inline std::vector<float> exp_args() {
  std::vector<float> x;
  for (int i = 0; i <= (1 << 16); ++i) x.push_back(-8.f + 16.f * i / (1 << 16));  // logits, box regressions
  for (int i = 0; i <= (1 << 15); ++i) x.push_back(-2.f * i / (1 << 15));          // soft-NMS decay arguments
  for (int k = 1; k < 24; ++k) { x.push_back(-std::ldexp(1.f, -k)); x.push_back(std::ldexp(1.f, -k)); }
  return x;
}
inline double exp_max_ulp(const std::vector<float>& x, const std::vector<float>& y) {
  double worst = 0;
  for (size_t i = 0; i < x.size(); ++i) {
    const double v = std::exp((double)x[i]);
    int ex;
    std::frexp(v, &ex);
    worst = std::max(worst, std::fabs((double)y[i] - v) / std::ldexp(1.0, ex - 24));
  }
  return worst;
}
inline void set_exp_ulp(double measured) { g_exp_ulp = std::max(1.0, 2 * measured); }

// ---- one case through a backend (the device, or the CPU stand-in with a seeded fault) ---------------------------
struct CaseStats {
  PreStats pre;
  NmsStats nms;
  ImaxStats imax;
  ScatterStats sc;
  long elems = 0;  // elements of all the case's device buffers
  long unaligned_tiles = 0, aligned_tiles = 0, ragged_tiles = 0, short_tiles = 0;
};
inline std::vector<std::vector<int>> cand_of_list(const PreOut& po, int B, int A) {
  std::vector<std::vector<int>> cd(B);
  for (int b = 0; b < B; ++b) {
    cd[b].assign(po.list.begin() + (size_t)b * A, po.list.begin() + (size_t)b * A + po.count[b]);
    std::sort(cd[b].begin(), cd[b].end());
  }
  return cd;
}
struct Sim {
  Fault f = F_NONE;
  void pre_nms(const Chain& ch, PreOut& o) { sim_pre_nms(ch, o, f); }
  void soft_nms(const NmsIn& in, const std::vector<uint8_t>*, int, const std::vector<int>*, const PreOut* lists, NmsOut& o) {
    sim_soft_nms(in, true, lists != nullptr, o, f);
  }
  void image_max(const std::vector<float>& sc, const std::vector<uint8_t>& keep, int B, int A, ImaxOut& o) {
    sim_image_max(sc.data(), keep.data(), B, A, o, f);
  }
  void loss(const std::vector<float>& mraw, float s, LossOut& o) { sim_loss(mraw.data(), (int)mraw.size(), s, o, f); }
  float count_ge(const std::vector<float>& sc, const std::vector<int>& cnt, int maxo, float th) {
    return ref_count_ge(sc.data(), cnt.data(), (int)cnt.size(), maxo, th);
  }
  void zero_segs(const Segs& s, std::vector<uint8_t>& fill, std::vector<uint8_t>& got) {
    fill.assign(s.total, 0xA5);
    got = fill;
    for (size_t i = 0; i < s.off.size(); ++i) std::memset(got.data() + s.off[i], 0, s.bytes[i]);
  }
  void cls_scatter(const ScatterIn& si, std::vector<float>& dx) {
    std::vector<char> t;
    ref_cls_scatter<float>(si, dx, t, f);
  }
  void adam(const AdamIO& in, float lr, int t, bool clip, AdamIO& o) {
    ref_adam<float>(in, adam_alpha(lr, t), clip ? kNPatch : -1, o.p, o.m, o.v, f);
  }
};

template <class Backend> void run_case(const Case& c, Backend& be, Verdict& V, CaseStats* st = nullptr) {
  if (c.kind == K_CHAIN) {
    const Chain ch = make_chain(c);
    const int B = c.B, A = ch.A;
    if (st) {
      st->elems = (long)(ch.cls.size() + ch.box.size() + ch.anchors.size() + ch.wpred.size() + ch.dx0.size()) + (long)B * A * 16;
      for (int b = 0; b < B; ++b)
        for (int x = 0; x < ch.ntiles; ++x) {
          int l = 0;
          while (l + 1 < ch.nlev && x >= ch.lev[l + 1].tile0) ++l;
          const Lev& L = ch.lev[l];
          const int a0 = (x - L.tile0) * kPreTile, n = std::min(kPreTile, ch.nloc(l) - a0);
          const long e0 = L.cls_off + ((long)b * ch.nloc(l) + a0) * c.nclass;
          (e0 & 3 ? st->unaligned_tiles : st->aligned_tiles)++;
          st->ragged_tiles += n < kPreTile && a0 > 0;
          st->short_tiles += n < kPreTile && a0 == 0;
        }
    }
    PreOut po;
    be.pre_nms(ch, po);
    if (!check_pre_nms(ch, po, V, st ? &st->pre : nullptr)) return;
    NmsIn ni;
    ni.B = B; ni.N = A; ni.max_out = c.max_out; ni.thresh = c.cand_thresh; ni.sigma = 0.5f; ni.clip = ch.img;
    ni.boxes = po.boxes; ni.scores = po.scores;
    if (c.cand_list) ni.cand = cand_of_list(po, B, A);
    else {
      ni.cand.assign(B, {});
      for (int b = 0; b < B; ++b)
        for (int a = 0; a < A; ++a)
          if (po.scores[(size_t)b * A + a] > ni.thresh && (po.keep[(size_t)b * A + a] & 1)) ni.cand[b].push_back(a);
    }
    NmsOut no;
    be.soft_nms(ni, c.cand_list ? nullptr : &po.keep, 1, nullptr, c.cand_list ? &po : nullptr, no);
    check_soft_nms(ni, no, V, st ? &st->nms : nullptr);
    check_count_ge(no.scores.data(), no.count.data(), B, c.max_out, 0.5f, be.count_ge(no.scores, no.count, c.max_out, 0.5f), V);
    ImaxOut io;
    be.image_max(po.scores, po.keep, B, A, io);
    check_image_max(po.scores.data(), po.keep.data(), B, A, io, V, st ? &st->imax : nullptr);
    LossOut lo;
    be.loss(io.m, c.scale, lo);
    check_loss(io.m.data(), B, c.scale, lo, V);
    const Segs sg = make_segs(c.nseg);
    std::vector<uint8_t> zf, zg;
    be.zero_segs(sg, zf, zg);
    check_zero_segs(sg, zf.data(), zg.data(), V);
    const ScatterIn si{&ch, po.scores.data(), po.keep.data(), io.m.data(), io.nties.data(), lo.dm.data()};
    std::vector<float> dx;
    be.cls_scatter(si, dx);
    check_cls_scatter(si, dx, V, st ? &st->sc : nullptr);
  } else if (c.kind == K_NMS) {
    std::vector<uint8_t> keep;
    std::vector<int> count;
    const NmsIn ni = make_nms(c, keep, count);
    if (st) st->elems = (long)c.B * c.N * (4 + 1 + 7) + (long)keep.size() / 4;
    NmsOut no;
    be.soft_nms(ni, keep.empty() ? nullptr : &keep, 1, count.empty() ? nullptr : &count, nullptr, no);
    check_soft_nms(ni, no, V, st ? &st->nms : nullptr);
  } else if (c.kind == K_IMAX) {
    std::vector<float> sc;
    std::vector<uint8_t> keep;
    make_imax(c, sc, keep);
    if (st) st->elems = (long)sc.size() + (long)keep.size() / 4;
    ImaxOut io;
    be.image_max(sc, keep, c.B, c.N, io);
    check_image_max(sc.data(), keep.data(), c.B, c.N, io, V, st ? &st->imax : nullptr);
    LossOut lo;
    be.loss(io.m, c.scale, lo);
    check_loss(io.m.data(), c.B, c.scale, lo, V);
  } else if (c.kind == K_LOSS) {
    const std::vector<float> mraw = make_mraw();
    LossOut lo;
    be.loss(mraw, c.scale, lo);
    check_loss(mraw.data(), (int)mraw.size(), c.scale, lo, V);
  } else if (c.kind == K_ZERO) {
    const Segs sg = make_segs(c.nseg);
    if (st) st->elems = (long)sg.total / 4;
    std::vector<uint8_t> zf, zg;
    be.zero_segs(sg, zf, zg);
    check_zero_segs(sg, zf.data(), zg.data(), V);
  } else if (c.kind == K_COUNT) {
    std::vector<float> sc;
    std::vector<int> cnt;
    make_count(c, sc, cnt);
    check_count_ge(sc.data(), cnt.data(), 4, c.max_out, 0.5f, be.count_ge(sc, cnt, c.max_out, 0.5f), V);
  } else if (c.kind == K_ADAM) {
    const AdamIO in = make_adam(c);
    if (st) st->elems = 4 * c.n;
    AdamIO out;
    be.adam(in, 0.01f, c.t, c.clip != 0, out);
    check_adam(in, adam_alpha(0.01f, c.t), c.clip ? kNPatch : -1, out, V);
  }
}

}  // namespace pck
