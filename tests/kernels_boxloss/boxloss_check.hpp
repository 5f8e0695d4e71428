// boxloss_check.hpp — the host reference of the box-regression term (regression_loss.py:16-142 as
// kernels_boxloss.hip states it), shared by boxloss_parity (device against host) and boxloss_teeth (seeded
// faults against the unfaulted reference; host only).
//
// The reference runs in fp64 on the same fp32 inputs and carries, beside every value, a bound on what fp32
// arithmetic in the same operation order can have lost (running error analysis, unit roundoff u = 2^-24):
// an input has bound 0; z = x op y gets the propagated bound plus u |z| for its own rounding (max / min:
// the larger operand bound, no rounding).  The bound of one diou is therefore derived from its ~45
// operations and the magnitudes they met, not measured.  Decisions (which corner wins, clamp at 0, zero
// denominators) compare exact inputs or the sign of one rounded difference, so fp32 and fp64 take them
// alike; a case whose zero test is not exact (a denominator that is 0 with a non-zero bound) is refused.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

namespace boxloss {

constexpr double kU = 5.9604644775390625e-08;  // 2^-24
constexpr int kMaxGt = 100;

struct EB {
  double v = 0, e = 0;
};
inline EB in(double v) { return EB{v, 0.0}; }
inline EB rnd(double v, double e) { return EB{v, e + kU * std::fabs(v)}; }
// a sum, difference or product of operands that carry no error is the same operation on the same fp32
// numbers: what fp32 loses is exactly its rounding of the fp64 result (0 for small integers, so a zero
// test on integer-valued boxes stays exact)
inline EB rnd_exact(double v, double e) { return e == 0 ? EB{v, std::fabs((double)(float)v - v)} : rnd(v, e); }
inline EB operator+(EB a, EB b) { return rnd_exact(a.v + b.v, a.e + b.e); }
inline EB operator-(EB a, EB b) { return rnd_exact(a.v - b.v, a.e + b.e); }
inline EB operator*(EB a, EB b) {
  return rnd_exact(a.v * b.v, std::fabs(a.v) * b.e + std::fabs(b.v) * a.e + a.e * b.e);
}
inline EB operator/(EB a, EB b) {
  const double den = std::fabs(b.v) - b.e;
  if (!(den > 0)) throw std::runtime_error("reference: a denominator is not bounded away from 0");
  const double z = a.v / b.v;
  return rnd(z, (a.e + std::fabs(z) * b.e) / den);
}
inline EB emax(EB a, EB b) { return EB{std::max(a.v, b.v), std::max(a.e, b.e)}; }
inline EB emin(EB a, EB b) { return EB{std::min(a.v, b.v), std::max(a.e, b.e)}; }
inline EB div_no_nan(EB a, EB b) {
  if (b.v == 0) {
    if (b.e != 0) throw std::runtime_error("reference: a zero denominator is not exact");
    return EB{};
  }
  return a / b;
}

// seeded faults (boxloss_teeth): each must change the answer on at least one case of the table
struct Faults {
  bool real_centres = false;   // (ymin + h / 2, xmin + w / 2) in place of the far corner
  bool clamp_gt = false;       // the gt's height clamped at 0
  bool tie_to_pred = false;    // tf.maximum / tf.minimum ties send the gradient to the pred
  bool first_tie_only = false; // reduce_max's gradient to the first tie only
  bool no_epsilon = false;     // the per-image epsilon missing
  bool max_over_gts = false;   // sum over preds of max over gts
};

struct Box {
  float ymin, xmin, ymax, xmax;
};

struct PairRef {
  EB v;       // 1 - diou_loss
  EB g[4];    // d v / d (pred ymin, xmin, ymax, xmax)
};

// regression_loss.py:101-142 + :84, with the gradient under the rules of kernels_boxloss.hip's header
inline PairRef pair_ref(const Box& G, const Box& P, const Faults& f = Faults{}) {
  const EB gy0 = in(G.ymin), gx0 = in(G.xmin), gy1 = in(G.ymax), gx1 = in(G.xmax);
  const EB py0 = in(P.ymin), px0 = in(P.xmin), py1 = in(P.ymax), px1 = in(P.xmax);
  const EB zero{};
  EB gh = gy1 - gy0;
  const EB gw = gx1 - gx0;
  if (f.clamp_gt) gh = emax(zero, gh);
  const EB ga = gh * gw;
  const EB rw = px1 - px0, rh = py1 - py0;
  const EB pw = emax(zero, rw), ph = emax(zero, rh);
  const EB pa = pw * ph;
  const EB iy0 = emax(gy0, py0), ix0 = emax(gx0, px0), iy1 = emin(gy1, py1), ix1 = emin(gx1, px1);
  const EB riw = ix1 - ix0, rih = iy1 - iy0;
  const EB iw = emax(zero, riw), ih = emax(zero, rih);
  const EB ia = iw * ih;
  const EB ua = (ga + pa) - ia;
  const EB iou = div_no_nan(ia, ua);
  const EB half = in(0.5);
  const EB c1y = gy0 + (f.real_centres ? gh * half : gh), c1x = gx0 + (f.real_centres ? gw * half : gw);
  const EB c2y = py0 + (f.real_centres ? ph * half : ph), c2x = px0 + (f.real_centres ? pw * half : pw);
  const EB dy = c1y - c2y, dx = c1x - c2x;
  const EB cd = dy * dy + dx * dx;
  const EB ey0 = emin(gy0, py0), ex0 = emin(gx0, px0), ey1 = emax(gy1, py1), ex1 = emax(gx1, px1);
  const EB rew = ex1 - ex0, reh = ey1 - ey0;
  const EB ew = emax(zero, rew), eh = emax(zero, reh);
  const EB diag = eh * eh + ew * ew;
  const EB diou = iou - div_no_nan(cd, diag);
  const EB one = in(1.0);
  PairRef r;
  r.v = one - (one - diou);
  // gradient
  const bool t = f.tie_to_pred;
  auto wins_gt = [&](float p, float g) { return t ? p >= g : p > g; };  // the pred takes a maximum's gradient
  auto wins_lt = [&](float p, float g) { return t ? p <= g : p < g; };  // ... a minimum's
  EB Gy0{}, Gx0{}, Gy1{}, Gx1{}, Gph{}, Gpw{};
  const EB two = in(2.0);
  if (ua.v != 0) {
    const EB ua2 = ua * ua;
    const EB dia = one / ua + ia / ua2;
    const EB dpa = zero - ia / ua2;
    Gph = Gph + dpa * pw;
    Gpw = Gpw + dpa * ph;
    const EB dih = dia * iw, diw = dia * ih;
    if (rih.v > 0) {
      if (wins_lt(P.ymax, G.ymax)) Gy1 = Gy1 + dih;
      if (wins_gt(P.ymin, G.ymin)) Gy0 = Gy0 - dih;
    }
    if (riw.v > 0) {
      if (wins_lt(P.xmax, G.xmax)) Gx1 = Gx1 + diw;
      if (wins_gt(P.xmin, G.xmin)) Gx0 = Gx0 - diw;
    }
  }
  if (diag.v != 0) {
    const EB dcd = zero - one / diag;
    const EB ddiag = cd / (diag * diag);
    const EB cs = f.real_centres ? half : one;  // d centre / d (clamped) extent
    const EB dc2y = zero - dcd * two * dy, dc2x = zero - dcd * two * dx;
    Gy0 = Gy0 + dc2y;
    Gph = Gph + dc2y * cs;
    Gx0 = Gx0 + dc2x;
    Gpw = Gpw + dc2x * cs;
    const EB deh = ddiag * two * eh, dew = ddiag * two * ew;
    if (reh.v > 0) {
      if (wins_gt(P.ymax, G.ymax)) Gy1 = Gy1 + deh;
      if (wins_lt(P.ymin, G.ymin)) Gy0 = Gy0 - deh;
    }
    if (rew.v > 0) {
      if (wins_gt(P.xmax, G.xmax)) Gx1 = Gx1 + dew;
      if (wins_lt(P.xmin, G.xmin)) Gx0 = Gx0 - dew;
    }
  }
  if (rh.v > 0) {
    Gy1 = Gy1 + Gph;
    Gy0 = Gy0 - Gph;
  }
  if (rw.v > 0) {
    Gx1 = Gx1 + Gpw;
    Gx0 = Gx0 - Gpw;
  }
  r.g[0] = Gy0;
  r.g[1] = Gx0;
  r.g[2] = Gy1;
  r.g[3] = Gx1;
  return r;
}

// one image: per gt the maximum over the kept preds, the anchors that reach it exactly (and the largest
// bound among them), the best value among the others (the runner-up) and the highest value + bound any of
// the others can reach in fp32
struct GtRef {
  double max = 0, bound = 0, runner = -INFINITY, runner_hi = -INFINITY;
  std::vector<int> ties;  // ascending; empty: no kept pred
};
struct ImageRef {
  std::vector<GtRef> gt;
  double value = 0;                 // sum_g max + epsilon
  std::vector<double> dpred;        // [A][4] d value / d pred box (kept anchors; others 0)
  std::vector<double> dpred_bound;  // [A][4]
};

inline ImageRef image_ref(const Box* gts, int G, const Box* preds, const uint8_t* keep, int A,
                          const Faults& f = Faults{}, bool want_grad = true) {
  ImageRef R;
  R.gt.resize(G);
  if (want_grad) {
    R.dpred.assign((size_t)A * 4, 0.0);
    R.dpred_bound.assign((size_t)A * 4, 0.0);
  }
  std::vector<int> kept;
  for (int a = 0; a < A; ++a)
    if (keep[a] & 1) kept.push_back(a);
  double sum = 0;
  if (f.max_over_gts) {
    // (fault) sum over preds of the max over gts: value only
    for (int a : kept) {
      double m = -INFINITY;
      for (int g = 0; g < G; ++g) m = std::max(m, pair_ref(gts[g], preds[a], f).v.v);
      if (G) sum += m;
    }
    R.value = sum + (f.no_epsilon ? 0.0 : 1e-7);
    return R;
  }
  std::vector<double> vals(kept.size()), bnds(kept.size());
  for (int g = 0; g < G; ++g) {
    GtRef& r = R.gt[g];
    if (kept.empty()) continue;
    for (size_t i = 0; i < kept.size(); ++i) {
      const PairRef p = pair_ref(gts[g], preds[kept[i]], f);
      vals[i] = p.v.v;
      bnds[i] = p.v.e;
    }
    double m = -INFINITY;
    for (double v : vals) m = std::max(m, v);
    r.max = m;
    for (size_t i = 0; i < kept.size(); ++i) {
      if (vals[i] == m) {
        r.ties.push_back(kept[i]);
        r.bound = std::max(r.bound, bnds[i]);
      } else {
        r.runner = std::max(r.runner, vals[i]);
        r.runner_hi = std::max(r.runner_hi, vals[i] + bnds[i]);
      }
    }
    sum += m;
    if (!want_grad) continue;
    const size_t nt = f.first_tie_only ? 1 : r.ties.size();
    for (size_t k = 0; k < nt; ++k) {
      const int a = r.ties[k];
      const PairRef p = pair_ref(gts[g], preds[a], f);
      for (int j = 0; j < 4; ++j) {
        R.dpred[(size_t)a * 4 + j] += p.g[j].v / (double)nt;
        R.dpred_bound[(size_t)a * 4 + j] += (p.g[j].e + kU * std::fabs(p.g[j].v)) / (double)nt;
      }
    }
  }
  R.value = sum + (f.no_epsilon ? 0.0 : 1e-7);
  return R;
}

// ---- cases ---------------------------------------------------------------------------------
struct Case {
  std::string name;
  int B = 1, A = 0, K = 64;
  std::vector<int> G;  // per image
  // inputs (fp32): anchors [A][4], logits [B][A][4] (ty, tx, th, tw), decoded boxes [B][A][4] (pre_nms's
  // arithmetic), keep [B][A], gts [B][100][4], the box-predict kernel [K][na*4]
  std::vector<float> anchors, logits, boxes, gts, wpred;
  std::vector<uint8_t> keep;
  int seed_used = 0;
};

constexpr int kNa = 9;

// decode_box_outputs in pre_nms's fp32 operation order (kernels_post.hip k_pre_nms)
inline void decode32(const float* an, const float* lg, float* out) {
  const float yca = (an[0] + an[2]) / 2.0f, xca = (an[1] + an[3]) / 2.0f;
  const float ha = an[2] - an[0], wa = an[3] - an[1];
  const float w = std::exp(lg[3]) * wa, h = std::exp(lg[2]) * ha;
  const float yc = lg[0] * ha + yca, xc = lg[1] * wa + xca;
  out[0] = yc - h / 2.0f;
  out[1] = xc - w / 2.0f;
  out[2] = yc + h / 2.0f;
  out[3] = xc + w / 2.0f;
}

struct Spec {
  std::string name;
  int B, A, K;
  std::vector<int> G;
  double keep_frac;        // share of kept anchors
  int mode;                // 0 random; 1 image 1 keeps nothing; 2 one kept anchor, the last; 3 duplicates; 4 degenerate gts
};

inline std::vector<Spec>& specs() {
  static std::vector<Spec> t;
  if (!t.empty()) return t;
  auto add = [&](const char* name, int B, int A, int K, std::vector<int> G, double kf, int mode) {
    t.push_back(Spec{name, B, A, K, std::move(G), kf, mode});
  };
  // ---- the table
  add("a3069_g7_b1", 1, 3069, 64, {7}, 0.3, 0);
  add("a3069_g100_b3", 3, 3069, 64, {100, 100, 100}, 0.3, 0);
  add("a49104_g7_b1", 1, 49104, 64, {7}, 0.05, 0);
  add("a76725_g0_1_7_b3", 3, 76725, 40, {7, 0, 1}, 0.03, 0);
  add("no_kept_image_b3", 3, 3069, 64, {7, 7, 7}, 0.3, 1);
  add("last_chunk_only_a3069", 1, 3069, 64, {7}, 0.0, 2);
  add("last_chunk_only_a76725", 1, 76725, 64, {7}, 0.0, 2);
  add("duplicate_ties_b1", 1, 3069, 64, {7}, 0.5, 3);
  add("degenerate_gts_b3", 3, 3069, 88, {7, 7, 7}, 0.3, 4);
  // ---- end of the table
  return t;
}

// the margin every (image, gt) must keep: whatever fp32 lost, no other kept anchor reaches the maximum
inline bool margin_holds(const GtRef& r) { return r.ties.empty() || r.max - r.bound > r.runner_hi; }
inline bool margins_hold(const ImageRef& R) {
  for (const GtRef& r : R.gt)
    if (!margin_holds(r)) return false;
  return true;
}

inline Case make_case_seed(const Spec& s, int seed) {
  Case c;
  c.name = s.name;
  c.B = s.B;
  c.A = s.A;
  c.K = s.K;
  c.G = s.G;
  c.seed_used = seed;
  std::mt19937 rng(1234u + 977u * (unsigned)seed + (unsigned)std::hash<std::string>{}(s.name) % 100000u);
  auto U = [&](double a, double b) { return (float)std::uniform_real_distribution<double>(a, b)(rng); };
  auto I = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
  const int A = s.A, B = s.B;
  const float S = 512.0f;
  c.anchors.resize((size_t)A * 4);
  c.logits.assign((size_t)B * A * 4, 0.0f);
  c.boxes.resize((size_t)B * A * 4);
  c.keep.assign((size_t)B * A, 0);
  c.gts.assign((size_t)B * kMaxGt * 4, 0.0f);
  c.wpred.resize((size_t)s.K * kNa * 4);
  for (float& w : c.wpred) w = U(-0.2, 0.2);
  const bool integer = s.mode == 4;  // integer coordinates: every product and sum below 2^24 is exact in fp32
  for (int a = 0; a < A; ++a) {
    float y = U(0, S - 40), x = U(0, S - 40), h = U(12, 160), w = U(12, 160);
    if (integer) { y = (float)I(0, 400); x = (float)I(0, 400); h = (float)I(0, 60); w = (float)I(0, 60); }
    if (s.mode == 3) {  // a pool of eight anchor boxes: exact duplicates by the hundred
      const int k = I(0, 7);
      y = 20.0f + 37.0f * k; x = 300.0f - 31.0f * k; h = 40.0f + 9.0f * k; w = 90.0f - 7.0f * k;
    }
    float* an = &c.anchors[(size_t)a * 4];
    an[0] = y; an[1] = x; an[2] = y + h; an[3] = x + w;
  }
  for (int b = 0; b < B; ++b) {
    const int G = s.G[b];
    for (int g = 0; g < G; ++g) {
      float* q = &c.gts[((size_t)b * kMaxGt + g) * 4];
      float y = U(0, S - 60), x = U(0, S - 60), h = U(20, 200), w = U(20, 200);
      if (integer) {
        y = (float)I(0, 400); x = (float)I(0, 400); h = (float)I(1, 80); w = (float)I(1, 80);
        if (g % 3 == 0) h = 0.0f;          // zero area
        if (g % 3 == 1) h = -h;            // flipped: ymax < ymin
        if (g == 5) { h = 0.0f; w = 0.0f; }  // a point
      }
      q[0] = y; q[1] = x; q[2] = y + h; q[3] = x + w;
    }
    for (int a = 0; a < A; ++a) {
      float* lg = &c.logits[((size_t)b * A + a) * 4];
      if (!integer && s.mode != 3)
        for (int j = 0; j < 4; ++j) lg[j] = U(-0.4, 0.4);
      decode32(&c.anchors[(size_t)a * 4], lg, &c.boxes[((size_t)b * A + a) * 4]);
      bool k = U(0, 1) < s.keep_frac;
      if (s.mode == 1 && b == 1) k = false;
      if (s.mode == 2) k = a == A - 1;
      c.keep[(size_t)b * A + a] = k ? (uint8_t)(1 | (I(0, 1) << 1) | 4) : (uint8_t)(I(0, 1) ? 4 : 0);
    }
  }
  return c;
}

inline std::vector<ImageRef> refs_of(const Case& c, const Faults& f = Faults{}, bool want_grad = true) {
  std::vector<ImageRef> out;
  for (int b = 0; b < c.B; ++b)
    out.push_back(image_ref(reinterpret_cast<const Box*>(&c.gts[(size_t)b * kMaxGt * 4]), c.G[b],
                            reinterpret_cast<const Box*>(&c.boxes[(size_t)b * c.A * 4]), &c.keep[(size_t)b * c.A],
                            c.A, f, want_grad));
  return out;
}

// the first seed under which every non-tie (image, gt) keeps its margin (the checker asserts it again)
inline Case make_case(const Spec& s, std::vector<ImageRef>* refs = nullptr) {
  for (int seed = 0; seed < 16; ++seed) {
    Case c = make_case_seed(s, seed);
    std::vector<ImageRef> r;
    bool ok = true;
    try {
      r = refs_of(c);
    } catch (const std::runtime_error&) {
      ok = false;  // (a zero test that is not exact: next seed)
    }
    for (size_t b = 0; ok && b < r.size(); ++b) ok = margins_hold(r[b]);
    if (!ok) continue;
    if (refs) *refs = std::move(r);
    return c;
  }
  throw std::runtime_error("no seed gives case " + s.name + " its margins");
}

}  // namespace boxloss
