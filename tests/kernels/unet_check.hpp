// unet_check.hpp — the host side of the U-Net kernel parity checker (unet_parity.cpp, unet_teeth.cpp): plain C++
// fp64 references of the operations behind the launchers of unet.hpp below un_wgrad (column reductions with the BN
// statistics and backward, the elementwise kernels, pool + Dropout, the attention gate, the output layer with its
// loss, the Masker's permutation, crops and box filter), written from the operation, with derived bounds
// ("U-Net kernel parity").  A case runs through a Backend: the device (unet_parity.cpp) or the CPU
// stand-in below (Sim), which restates the kernels in fp32 with the reduction's block / lane-group / wave-fold
// geometry and takes seeded faults.  Host code only: no HIP header.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "gemm_check.hpp"

namespace uck {
using gck::f2u;
using gck::u2f;
using VF = std::vector<float>;
using VD = std::vector<double>;
using VI = std::vector<int>;
using VB = std::vector<uint8_t>;

constexpr double kU = 5.9604644775390625e-8;      // 2^-24: one fp32 rounding, relative
constexpr double kU64 = 1.1102230246251565e-16;   // 2^-53
constexpr double kDen = 7.1e-46;                  // half the smallest subnormal
constexpr double kInf = std::numeric_limits<double>::infinity();
constexpr uint32_t kFillWord = gck::kUnwritten;   // "never written": a NaN no kernel produces
// harness-only copies of the launcher's constants (the teeth do not link the library): unet_parity --plan holds
// colred_plan() equal to the library's un_colred_plan_info() case by case
constexpr long kRedElems = 8192, kRedMaxBlk = 1024, kGridCap = 8192, kLossMaxBlk = 1024;
constexpr float kDropP = 0.2f, kDropScale = 1.25f;
enum { RNG_DSHUF = 7, RNG_DFLIP = 8, RNG_DROPOUT = 9 };

// expf / tanhf are library functions: their error is twice the maximum the harness measured on the device, at
// least 1 ulp (post_check.hpp's pattern)
inline double g_exp_ulp = 1.0, g_tanh_ulp = 1.0;
inline void set_ulps(double exp_measured, double tanh_measured) {
  g_exp_ulp = std::max(1.0, 2 * exp_measured);
  g_tanh_ulp = std::max(1.0, 2 * tanh_measured);
}
inline double ulp_err(float got, double want) {  // |got - want| in ulps of want (normal range)
  int ex;
  std::frexp(want, &ex);
  return std::fabs((double)got - want) / std::ldexp(1.0, std::max(ex, -125) - 24);
}
inline VF exp_args() {  // -z of the attention cases: the saturated gates, and the range of the ordinary ones
  VF x = {20.f, -20.f, 87.f, -87.f};
  for (int i = 0; i <= 4096; ++i) x.push_back(-12.f + 24.f * (float)i / 4096.f);
  return x;
}
inline VF tanh_args() {  // the output layer's pre-activations: |z| = 12 and past it, where tanhf is +-1
  VF x;
  for (int i = 0; i <= 16384; ++i) x.push_back(-32.f + 64.f * (float)i / 16384.f);
  return x;
}

// ---- E: an fp64 value with the running error bound of its fp32 evaluation -------------------------------------------
struct E {
  double v = 0, e = 0;
  E() = default;
  E(double v_, double e_ = 0) : v(v_), e(e_) {}
};
inline bool is_f32(double v) { return (double)(float)v == v; }
inline E rnd(double v, double ep) {
  if (ep == 0 && is_f32(v)) return E(v, 0);
  return E(v, ep + kU * (std::fabs(v) + ep) + kDen);
}
inline E operator+(E a, E b) { return rnd(a.v + b.v, a.e + b.e); }
inline E operator-(E a, E b) { return rnd(a.v - b.v, a.e + b.e); }
// a * b + c written with these two admits the contracted form too: one rounding of a b + c errs by at most
// 2^-24 |a b + c|, which the second rounding's term alone covers (kernels_unet.hip is built with contraction on)
inline E operator*(E a, E b) { return rnd(a.v * b.v, std::fabs(a.v) * b.e + std::fabs(b.v) * a.e + a.e * b.e); }
inline E operator/(E a, E b) {
  const double v = a.v / b.v, den = std::fabs(b.v) - b.e;
  return rnd(v, (a.e == 0 && b.e == 0) ? 0.0 : den > 0 ? (a.e + std::fabs(v) * b.e) / den : kInf);
}
inline E operator-(E a) { return E(-a.v, a.e); }
inline E tfma(E a, E b, E c) {  // fmaf: one rounding
  return rnd(a.v * b.v + c.v, std::fabs(a.v) * b.e + std::fabs(b.v) * a.e + a.e * b.e + c.e);
}
inline E texp(E x) {
  if (x.v == 0 && x.e == 0) return E(1.0, 0);
  const double v = std::exp(x.v);
  return E(v, v * std::expm1(x.e) + g_exp_ulp * 2 * kU * v + kDen + (v < 2.4e-38 ? v : 0.0));  // a subnormal may flush
}
inline E tsigmoid(E z) {  // 1 / (1 + expf(-z))
  const E ev = texp(-z);
  if (ev.v + ev.e >= (double)FLT_MAX) {  // expf overflows to inf (a = 0) or stays huge (a subnormal)
    const double v = 1.0 / (1.0 + ev.v);
    return E(v, v + 1.2e-38);
  }
  E a = E(1.0) / (E(1.0) + ev);
  if (a.v < 2.4e-38) a.e += 1.2e-38;
  return a;
}
inline E ttanh(E x) {
  const double v = std::tanh(x.v), lo = std::tanh(std::max(0.0, std::fabs(x.v) - x.e));
  return E(v, (1.0 - lo * lo) * x.e + g_tanh_ulp * 2 * kU * std::fabs(v) + kDen);
}
// leaky (slope 0.2f) and its derivative; an element within its rounding of the kink may fall either side
constexpr float kSlope = 0.2f;
inline E tleaky(E z, long* kinks) {
  if (std::fabs(z.v) <= z.e) {
    ++*kinks;
    return E(z.v > 0 ? z.v : (double)kSlope * z.v, 2 * z.e + kDen);
  }
  return z.v > 0 ? z : E((double)kSlope) * z;
}
inline E tleaky_grad(E z, long* kinks) {
  if (std::fabs(z.v) <= z.e) {
    ++*kinks;
    return E(0.5 * (1.0 + kSlope), 0.5 * (1.0 - kSlope));
  }
  return E(z.v > 0 ? 1.0 : (double)kSlope);
}
inline double ratio_of(float got, E want) {
  if (!std::isfinite(got) || !std::isfinite(want.v)) return kInf;
  const double d = std::fabs((double)got - want.v);
  if (d == 0) return 0;
  return want.e > 0 ? d / want.e : kInf;
}
inline E fstore(double v, double e) { return E(v, e + kU * std::fabs(v) + kDen); }  // an fp64 value stored as float

// ---- Philox4x32-10 (Salmon et al.), restated; tests/golden/unet holds it equal to oracle/philox.py's draws -----------
inline void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
inline float u01(uint32_t v) { return (float)(v >> 8) * (1.0f / 16777216.0f); }
struct Rk {  // a draw's key: the run's seed and step, the first image's global index, the Dropout layer
  uint64_t seed = 0;
  int64_t step = 0;
  int gimg0 = 0, layer = -1;
};
inline void draw(const Rk& k, uint32_t e, uint32_t c1, int img, int stream, uint32_t out[4]) {
  out[0] = e; out[1] = c1; out[2] = (uint32_t)(k.gimg0 + img); out[3] = (uint32_t)((uint64_t)k.step << 8) | (uint32_t)stream;
  philox(out, (uint32_t)k.seed, (uint32_t)(k.seed >> 32));
}
// Keras Dropout(0.2) keep flag of element e of image b (oracle/defender.py: dropout_mask)
inline bool keep_flag(const Rk& k, long e, int b) {
  uint32_t q[4];
  draw(k, (uint32_t)e, (uint32_t)k.layer, b, RNG_DROPOUT, q);
  return u01(q[0]) >= kDropP;
}
inline VI shuffle_perm(const Rk& k, int B) {  // tf.random.shuffle: a stable sort by one key per image
  std::vector<std::pair<uint32_t, int>> key(B);
  for (int b = 0; b < B; ++b) {
    uint32_t q[4];
    draw(k, 0, 0, b, RNG_DSHUF, q);
    key[b] = {q[0], b};
  }
  std::stable_sort(key.begin(), key.end());
  VI p(B);
  for (int b = 0; b < B; ++b) p[b] = key[b].second;
  return p;
}
inline void flips(const Rk& k, int b, int* lr, int* ud) {
  uint32_t q[4];
  draw(k, 0, 0, b, RNG_DFLIP, q);
  *lr = u01(q[0]) >= 0.5f;
  *ud = u01(q[1]) >= 0.5f;
}

// ---- the golden draws (tests/golden/unet) ---------------------------------------------------------------------------
// drop_keep.txt: records "seed(hex) step gimg0 layer B n" + B strings of n keep flags; perm_flip.txt: records
// "seed(hex) step gimg0 B" + B sources + B (lr, ud) pairs.  Both drawn by oracle/defender.py.
struct Golden {
  struct Drop { Rk k; int B; long n; std::vector<std::string> keep; };
  struct Perm { Rk k; int B; VI perm, lr, ud; };
  std::vector<Drop> drops;
  std::vector<Perm> perms;
  bool read = false;
  void load(const std::string& dir) {
    FILE* fp = fopen((dir + "/drop_keep.txt").c_str(), "r");
    if (!fp) return;
    unsigned long long sd;
    long step, n;
    int g, l, B;
    while (fscanf(fp, "%llx %ld %d %d %d %ld", &sd, &step, &g, &l, &B, &n) == 6) {
      Drop d;
      d.k = Rk{sd, step, g, l}; d.B = B; d.n = n;
      std::vector<char> buf(n + 2);
      for (int b = 0; b < B; ++b) {
        if (fscanf(fp, "%s", buf.data()) != 1) { fclose(fp); return; }
        d.keep.emplace_back(buf.data());
      }
      drops.push_back(d);
    }
    fclose(fp);
    fp = fopen((dir + "/perm_flip.txt").c_str(), "r");
    if (!fp) return;
    while (fscanf(fp, "%llx %ld %d %d", &sd, &step, &g, &B) == 4) {
      Perm p;
      p.k = Rk{sd, step, g, 0}; p.B = B;
      p.perm.resize(B); p.lr.resize(B); p.ud.resize(B);
      for (int b = 0; b < B; ++b) if (fscanf(fp, "%d", &p.perm[b]) != 1) { fclose(fp); return; }
      for (int b = 0; b < B; ++b) if (fscanf(fp, "%d %d", &p.lr[b], &p.ud[b]) != 2) { fclose(fp); return; }
      perms.push_back(p);
    }
    fclose(fp);
    read = true;
  }
  const Drop* drop(const Rk& k, int B, long n) const {
    for (auto& d : drops)
      if (d.k.seed == k.seed && d.k.step == k.step && d.k.gimg0 == k.gimg0 && d.k.layer == k.layer && d.B == B && d.n == n) return &d;
    return nullptr;
  }
  const Perm* perm(const Rk& k, int B) const {
    for (auto& p : perms)
      if (p.k.seed == k.seed && p.k.step == k.step && p.k.gimg0 == k.gimg0 && p.B == B) return &p;
    return nullptr;
  }
};
inline Golden g_golden;
constexpr long kGoldenMaxFlags = 40000;  // cases with more Dropout draws than this take keep_flag() alone

// ---- verdicts -------------------------------------------------------------------------------------------------------
struct Verdict {
  std::map<std::string, double> fields;  // ratio fields: max(err / bound), must be <= 1
  std::map<std::string, bool> flags;     // exact fields: must be true
  long nonfinite = 0, kinks = 0, elems = 0;
  bool threw = false, untouched = true, golden_used = false;
  std::string what;
  void field(const std::string& k, double r) {
    auto it = fields.find(k);
    if (it == fields.end()) fields[k] = r;
    else it->second = std::max(it->second, r);
  }
  void flag(const std::string& k, bool ok) {
    auto it = flags.find(k);
    if (it == flags.end()) flags[k] = ok;
    else it->second = it->second && ok;
  }
  void cmp(const std::string& k, float got, E want) {
    if (!std::isfinite(got)) ++nonfinite;
    field(k, ratio_of(got, want));
  }
  double ratio() const {
    double r = 0;
    for (auto& f : fields) r = std::max(r, f.second);
    return r;
  }
  bool exact_ok() const {
    for (auto& f : flags) if (!f.second) return false;
    return true;
  }
  double kink_share() const { return elems ? (double)kinks / (double)elems : 0.0; }
};
inline bool same_bits(const VF& a, const VF& b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * 4)); }
inline bool is_fill(float f) { return f2u(f) == kFillWord; }
inline VF filled(size_t n) { return VF(n, u2f(kFillWord)); }

// ---- geometry -------------------------------------------------------------------------------------------------------
inline long cdivl(long a, long b) { return (a + b - 1) / b; }
struct ColredPlan { int blocks; long rpb; int lane_rows, idle; long last_rows; };
inline ColredPlan colred_plan(long M, int C) {
  ColredPlan p;
  p.blocks = (int)std::min<long>(std::max<long>(std::min<long>(cdivl(M * C, kRedElems), M), 1), kRedMaxBlk);
  p.rpb = cdivl(M, p.blocks);
  p.lane_rows = 256 / C;
  p.idle = 256 - p.lane_rows * C;
  p.last_rows = M - (long)(p.blocks - 1) * p.rpb;
  return p;
}
inline long grid_blocks(long n) { return std::min<long>(std::max<long>(cdivl(n, 256), 1), kGridCap); }
inline int loss_blocks(long M) { return (int)std::min<long>(cdivl(M, 256), kLossMaxBlk); }

// ---- seeded faults of the CPU stand-in ------------------------------------------------------------------------------
enum Fault {
  F_NONE = 0,
  F_BLOCK_LAST_ROW,   // a block's last row dropped
  F_IDLE_ROWS,        // the idle threads' rows added
  F_SKIP_BLOCK64,     // block 64 skipped in the fold
  F_NO_SHIFT,         // the shift not added back to the mean
  F_NO_BESSEL,        // Bessel's factor missing
  F_LAST_MAX,         // the last maximum instead of the first
  F_BWD_NO_SCALE,     // the Dropout scale missing in the pool's backward
  F_NO_RESTART,       // the image's element index not restarted
  F_XOR_SHORT,        // the xor tree one step short
  F_CLAMP_STORES,     // a clamped lane storing
  F_NO_DSIG,          // a (1 - a) missing
  F_LOSS_M,           // the loss divided by M * 3 instead of HW * 3
  F_OUT_ORDER,        // un_out summing in another order
  F_AREA_GE,          // the filter's > taken as >=
  F_TAIL_ROWS         // the tail rows left unzeroed
};

struct Bn { VF mu, sc, be; };

// ---- the backend: unet.hpp's launchers on host vectors.  Every output arrives sized and holding its fill (or the
// old value of an accumulating call); pool_bwd and att_cat_bwd return true when the launcher threw ------------------
struct Backend {
  virtual ~Backend() {}
  virtual void bn_stats(const VF& y, long M, int C, const VF& gamma, bool moving, VF& mm, VF& mv, VF& mean, VF& rstd, VF& sc, VD& part) = 0;
  virtual void bn_bwd(const VF& da, const VF& y, long M, int C, const VF& mu, const VF& rstd, const VF& sc, const VF& be, int act,
                      VF& mdz, VF& mdzx, VF& dgamma, VF& dbeta, VF& dy, VD& part) = 0;
  virtual void colsum(const VF& v, long M, int C, VF& out, VD& part) = 0;
  virtual void bnact(const VF& y, const Bn& b, long M, int C, int act, VF& a) = 0;
  virtual void pool(const VF& x, int B, int H, int W, int C, const Rk& k, VF& out, VB& arg) = 0;
  virtual bool pool_bwd(const VF& dout, const VB& arg, VF& dx, int B, int H, int W, int C, const Rk& k, bool acc) = 0;
  virtual void att_s(const VF& g, const VF& x, const Bn& b1, const Bn& b2, long M, int C, VF& s) = 0;
  virtual void att_t(const VF& s, const VF& w, float b, long M, int C, VF& t) = 0;
  virtual void att_cat(const VF& up, const VF& skip, const VF& t, const float bn3[3], int B, long HW, int C, const Rk& k, VF& cat) = 0;
  virtual bool att_cat_bwd(const VF& dcat, const VF& skip, const VF& t, const float bn3[3], int B, long HW, int C, const Rk& k, VF& dup,
                           VF& dskip, VF& dz3) = 0;
  virtual void att_s_bwd(const VF& dt, const VF& w3, const VF& g, const VF& x, const Bn& b1, const Bn& b2, long M, int C, VF& dsum) = 0;
  virtual void out_loss(const VF& x, const VF& w, const VF& b, const VF& tgt, long M, long HW, int C, VF& upd, VF& dz, VD& lpart, VF& loss) = 0;
  virtual void out(const VF& x, const VF& w, const VF& b, long M, int C, VF& upd) = 0;
  virtual void small_dgrad(const VF& dz, const VF& w, VF& dx, long M, int C, int O, bool acc) = 0;
  virtual void add(VF& a, const VF& b, long n) = 0;
  virtual void perm_crops(const VF& images, int B, int H, int W, int P, const Rk& k, VI& info, VF& crops) = 0;
  // sets: 1 the score output, 2 / 4 / 8 the second set's boxes / scores / count
  virtual void filter(const VF& nb, const VF& ns, const VI& nc, int B, int maxo, float H, float W, float thresh, int sets, VF& ob, VI& oc,
                      VF& os, VF& b2, VF& s2, VI& c2) = 0;
};

// ---- the CPU stand-in ------------------------------------------------------------------------------------------------
struct Sim : Backend {
  Fault f = F_NONE;
  explicit Sim(Fault f_ = F_NONE) : f(f_) {}
  static float lk(float x) { return x > 0.f ? x : kSlope * x; }
  static float lg(float z) { return z > 0.f ? 1.f : kSlope; }
  // k_colred64's geometry: block z, lane groups of C threads, thread c folds its groups
  template <class Term> void colred(long M, int C, VD& part, Term term) {
    const ColredPlan p = colred_plan(M, C);
    for (int z = 0; z < p.blocks; ++z) {
      const long r0 = (long)z * p.rpb;
      long r1 = std::min(M, r0 + p.rpb);
      if (f == F_BLOCK_LAST_ROW && z == 0) --r1;
      std::vector<double> s0(256, 0.0), s1(256, 0.0);
      for (int t = 0; t < 256; ++t) {
        const int c = t % C, ro = t / C;
        if (ro >= p.lane_rows && f != F_IDLE_ROWS) continue;
        for (long row = r0 + ro; row < r1; row += p.lane_rows) term(row, c, s0[t], s1[t]);
      }
      for (int c = 0; c < C; ++c) {
        double b0 = 0, b1 = 0;
        const int groups = f == F_IDLE_ROWS ? (255 - c) / C + 1 : p.lane_rows;
        for (int j = 0; j < groups; ++j) { b0 += s0[c + j * C]; b1 += s1[c + j * C]; }
        part[((long)z * C + c) * 2] = b0;
        part[((long)z * C + c) * 2 + 1] = b1;
      }
    }
  }
  void wave_fold(const VD& part, int nblk, int C, int c, double& s0, double& s1) const {
    double l0[64], l1[64];
    for (int l = 0; l < 64; ++l) {
      l0[l] = l1[l] = 0;
      for (int z = l; z < nblk; z += 64) {
        if (f == F_SKIP_BLOCK64 && z == 64) continue;
        l0[l] += part[((long)z * C + c) * 2];
        l1[l] += part[((long)z * C + c) * 2 + 1];
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      double n0[64], n1[64];
      for (int l = 0; l < 64; ++l) { n0[l] = l0[l] + l0[l ^ o]; n1[l] = l1[l] + l1[l ^ o]; }
      std::memcpy(l0, n0, sizeof l0);
      std::memcpy(l1, n1, sizeof l1);
    }
    s0 = l0[0]; s1 = l1[0];
  }
  void bn_stats(const VF& y, long M, int C, const VF& gamma, bool moving, VF& mm, VF& mv, VF& mean, VF& rstd, VF& sc, VD& part) override {
    colred(M, C, part, [&](long row, int c, double& a0, double& a1) {
      const double d = (double)y[row * C + c] - (double)y[c];
      a0 += d; a1 += d * d;
    });
    const int nb = colred_plan(M, C).blocks;
    for (int c = 0; c < C; ++c) {
      double s0, s1;
      wave_fold(part, nb, C, c, s0, s1);
      const double dm = s0 / (double)M;
      double var = s1 / (double)M - dm * dm;
      if (var < 0) var = 0;
      const double mu = (f == F_NO_SHIFT ? 0.0 : (double)y[c]) + dm, rs = 1.0 / std::sqrt(var + 1e-3);
      mean[c] = (float)mu; rstd[c] = (float)rs; sc[c] = (float)(rs * (double)gamma[c]);
      if (moving) {
        const double uvar = (M > 1 && f != F_NO_BESSEL) ? var * (double)M / (double)(M - 1) : var;
        mm[c] = (float)(mm[c] - (mm[c] - mu) * 0.01);
        mv[c] = (float)(mv[c] - (mv[c] - uvar) * 0.01);
      }
    }
  }
  void bn_bwd(const VF& da, const VF& y, long M, int C, const VF& mu, const VF& rstd, const VF& sc, const VF& be, int act, VF& mdz,
              VF& mdzx, VF& dgamma, VF& dbeta, VF& dy, VD& part) override {
    colred(M, C, part, [&](long row, int c, double& a0, double& a1) {
      const float yc = y[row * C + c] - mu[c];
      float dz = da[row * C + c];
      if (act) dz *= lg(yc * sc[c] + be[c]);
      a0 += (double)dz; a1 += (double)dz * (double)(yc * rstd[c]);
    });
    const int nb = colred_plan(M, C).blocks;
    for (int c = 0; c < C; ++c) {
      double s0, s1;
      wave_fold(part, nb, C, c, s0, s1);
      mdz[c] = (float)(s0 / (double)M); mdzx[c] = (float)(s1 / (double)M);
      dgamma[c] = (float)s1; dbeta[c] = (float)s0;
    }
    for (long i = 0; i < M * C; ++i) {
      const int c = (int)(i % C);
      const float yc = y[i] - mu[c];
      float dz = da[i];
      if (act) dz *= lg(yc * sc[c] + be[c]);
      dy[i] = sc[c] * (dz - mdz[c] - (yc * rstd[c]) * mdzx[c]);
    }
  }
  void colsum(const VF& v, long M, int C, VF& out, VD& part) override {
    colred(M, C, part, [&](long row, int c, double& a0, double&) { a0 += (double)v[row * C + c]; });
    const int nb = colred_plan(M, C).blocks;
    for (int c = 0; c < C; ++c) {
      double s0, s1;
      wave_fold(part, nb, C, c, s0, s1);
      out[c] = (float)s0;
    }
  }
  void bnact(const VF& y, const Bn& b, long M, int C, int act, VF& a) override {
    for (long i = 0; i < M * C; ++i) {
      const int c = (int)(i % C);
      const float z = (y[i] - b.mu[c]) * b.sc[c] + b.be[c];
      a[i] = act ? lk(z) : z;
    }
  }
  void pool(const VF& x, int B, int H, int W, int C, const Rk& k, VF& out, VB& arg) override {
    const int Ho = H / 2, Wo = W / 2;
    const long per = (long)Ho * Wo * C;
    for (long i = 0; i < B * per; ++i) {
      const int c = (int)(i % C), ox = (int)(i / C % Wo), oy = (int)(i / C / Wo % Ho), b = (int)(i / per);
      const float* base = &x[(((long)b * H + 2 * oy) * W + 2 * ox) * C + c];
      const float v[4] = {base[0], base[C], base[(long)W * C], base[(long)W * C + C]};
      float m = v[0];
      int am = 0;
      for (int q = 1; q < 4; ++q)
        if (f == F_LAST_MAX ? v[q] >= m : v[q] > m) { m = v[q]; am = q; }
      arg[i] = (uint8_t)am;
      if (k.layer < 0) { out[i] = m; continue; }
      const long e = f == F_NO_RESTART ? i : i - b * per;
      out[i] = keep_flag(k, e, b) ? m * kDropScale : 0.f;
    }
  }
  bool pool_bwd(const VF& dout, const VB& arg, VF& dx, int B, int H, int W, int C, const Rk& k, bool acc) override {
    if (!acc && ((H | W) & 1)) return true;
    const int Ho = H / 2, Wo = W / 2;
    const long per = (long)Ho * Wo * C;
    for (long i = 0; i < B * per; ++i) {
      const int c = (int)(i % C), ox = (int)(i / C % Wo), oy = (int)(i / C / Wo % Ho), b = (int)(i / per);
      const float g = keep_flag(k, i - b * per, b) ? (f == F_BWD_NO_SCALE ? dout[i] : dout[i] * kDropScale) : 0.f;
      float* base = &dx[(((long)b * H + 2 * oy) * W + 2 * ox) * C + c];
      const long off[4] = {0, C, (long)W * C, (long)W * C + C};
      for (int q = 0; q < 4; ++q) {
        const float v = q == arg[i] ? g : 0.f;
        if (acc) base[off[q]] += v;
        else base[off[q]] = v;
      }
    }
    return false;
  }
  void att_s(const VF& g, const VF& x, const Bn& b1, const Bn& b2, long M, int C, VF& s) override {
    for (long i = 0; i < M * C; ++i) {
      const int c = (int)(i % C);
      s[i] = lk(((g[i] - b1.mu[c]) * b1.sc[c] + b1.be[c]) + ((x[i] - b2.mu[c]) * b2.sc[c] + b2.be[c]));
    }
  }
  void att_t(const VF& s, const VF& w, float b, long M, int C, VF& t) override {
    for (long m = 0; m < M; ++m) {
      float acc = 0.f;
      for (int c = 0; c < C; ++c) acc = fmaf(s[m * C + c], w[c], acc);
      t[m] = acc + b;
    }
  }
  static float sig(float z) { return 1.0f / (1.0f + expf(-z)); }
  void att_cat(const VF& up, const VF& skip, const VF& t, const float bn3[3], int B, long HW, int C, const Rk& k, VF& cat) override {
    for (long i = 0; i < (long)B * HW * 2 * C; ++i) {
      const int c2 = (int)(i % (2 * C));
      const long m = i / (2 * C);
      float v;
      if (c2 < C) v = up[m * C + c2];
      else v = skip[m * C + c2 - C] * sig((t[m] - bn3[0]) * bn3[1] + bn3[2]);
      if (k.layer < 0) { cat[i] = v; continue; }
      const int b = (int)(m / HW);
      cat[i] = keep_flag(k, i - (long)b * HW * 2 * C, b) ? v * kDropScale : 0.f;
    }
  }
  bool att_cat_bwd(const VF& dcat, const VF& skip, const VF& t, const float bn3[3], int B, long HW, int C, const Rk& k, VF& dup, VF& dskip,
                   VF& dz3) override {
    if (C < 1 || C > 64 || (C & (C - 1))) return true;
    const long M = (long)B * HW;
    const long lanes = cdivl(M * C, 256) * 256;
    std::vector<float> da(64);
    for (long g0 = 0; g0 < lanes; g0 += 64) {  // a wave at a time: the xor tree runs over its lanes
      float a_l[64];
      long m_l[64];
      bool ok_l[64];
      for (int l = 0; l < 64; ++l) {
        const long gi = g0 + l, m = gi / C;
        const int c = (int)(gi - m * C);
        const bool ok = m < M;
        const long mc = ok ? m : M - 1;
        const int b = (int)(mc / HW);
        const float a = sig((t[mc] - bn3[0]) * bn3[1] + bn3[2]);
        const long e = (mc - (long)b * HW) * 2 * C;
        const float g0v = keep_flag(k, e + c, b) ? dcat[mc * 2 * C + c] * kDropScale : 0.f;
        const float g1v = keep_flag(k, e + C + c, b) ? dcat[mc * 2 * C + C + c] * kDropScale : 0.f;
        if (ok || f == F_CLAMP_STORES) {
          // a clamped lane that stores writes its own (wrong) channel's value over pixel M - 1
          dup[mc * C + c] = ok ? g0v : g0v + 1.f;
          dskip[mc * C + c] = g1v * a;
        }
        da[l] = g1v * skip[mc * C + c];
        a_l[l] = a; m_l[l] = mc; ok_l[l] = ok;
      }
      for (int o = 1; o < (f == F_XOR_SHORT ? C / 2 : C); o <<= 1) {
        float n[64];
        for (int l = 0; l < 64; ++l) n[l] = da[l] + da[l ^ o];
        std::memcpy(da.data(), n, sizeof n);
      }
      for (int l = 0; l < 64; ++l)
        if (ok_l[l] && (g0 + l) % C == 0) dz3[m_l[l]] = f == F_NO_DSIG ? da[l] : da[l] * (a_l[l] * (1.0f - a_l[l]));
    }
    return false;
  }
  void att_s_bwd(const VF& dt, const VF& w3, const VF& g, const VF& x, const Bn& b1, const Bn& b2, long M, int C, VF& dsum) override {
    for (long i = 0; i < M * C; ++i) {
      const int c = (int)(i % C);
      const float zg = (g[i] - b1.mu[c]) * b1.sc[c] + b1.be[c], zx = (x[i] - b2.mu[c]) * b2.sc[c] + b2.be[c];
      dsum[i] = dt[i / C] * w3[c] * lg(zg + zx);
    }
  }
  void out_loss(const VF& x, const VF& w, const VF& b, const VF& tgt, long M, long HW, int C, VF& upd, VF& dz, VD& lpart, VF& loss) override {
    const int nb = loss_blocks(M);
    const float inv = 1.0f / (float)(HW * 3);
    for (int z = 0; z < nb; ++z) {
      double blk = 0;
      for (int t = 0; t < 256; ++t) {
        double acc = 0;
        for (long m = (long)z * 256 + t; m < M; m += (long)nb * 256)
          for (int o = 0; o < 3; ++o) {
            float zz = b[o];
            for (int c = 0; c < C; ++c) zz = fmaf(x[m * C + c], w[c * 3 + o], zz);
            const float th = tanhf(zz), u = 2.0f * th, d = tgt[m * 3 + o] - u;
            acc += (double)d * (double)d;
            upd[m * 3 + o] = u;
            dz[m * 3 + o] = (-2.0f * d * inv) * 2.0f * (1.0f - th * th);
          }
        blk += acc / (double)((f == F_LOSS_M ? M : HW) * 3);
      }
      lpart[z] = blk;
    }
    double s = 0;
    for (int z = 0; z < nb; ++z) s += lpart[z];
    loss[0] = (float)s;
  }
  void out(const VF& x, const VF& w, const VF& b, long M, int C, VF& upd) override {
    for (long m = 0; m < M; ++m)
      for (int o = 0; o < 3; ++o) {
        float zz = b[o];
        if (f == F_OUT_ORDER) {
          zz = 0.f;
          for (int c = C - 1; c >= 0; --c) zz = fmaf(x[m * C + c], w[c * 3 + o], zz);
          zz += b[o];
        } else {
          for (int c = 0; c < C; ++c) zz = fmaf(x[m * C + c], w[c * 3 + o], zz);
        }
        upd[m * 3 + o] = 2.0f * tanhf(zz);
      }
  }
  void small_dgrad(const VF& dz, const VF& w, VF& dx, long M, int C, int O, bool acc) override {
    for (long i = 0; i < M * C; ++i) {
      float v = 0.f;
      for (int o = 0; o < O; ++o) v = fmaf(dz[i / C * O + o], w[i % C * O + o], v);
      if (acc) dx[i] += v;
      else dx[i] = v;
    }
  }
  void add(VF& a, const VF& b, long n) override {
    for (long i = 0; i < n; ++i) a[i] += b[i];
  }
  void perm_crops(const VF& images, int B, int H, int W, int P, const Rk& k, VI& info, VF& crops) override {
    const VI p = shuffle_perm(k, B);
    for (int b = 0; b < B; ++b) {
      int lr, ud;
      flips(k, b, &lr, &ud);
      info[b * 3] = p[b]; info[b * 3 + 1] = lr; info[b * 3 + 2] = ud;
      for (int y = 0; y < P; ++y)
        for (int x = 0; x < P; ++x)
          for (int q = 0; q < 3; ++q)
            crops[(((long)b * P + y) * P + x) * 3 + q] = images[(((long)p[b] * H + (ud ? P - 1 - y : y)) * W + (lr ? P - 1 - x : x)) * 3 + q];
    }
  }
  void filter(const VF& nb, const VF& ns, const VI& nc, int B, int maxo, float H, float W, float thresh, int sets, VF& ob, VI& oc, VF& os,
              VF& b2, VF& s2, VI& c2) override {
    for (int b = 0; b < B; ++b) {
      int k = 0;
      for (int i = 0; i < nc[b]; ++i) {
        const float* bx = &nb[((long)b * maxo + i) * 4];
        const float h = bx[2] - bx[0], w = bx[3] - bx[1];
        const bool area = f == F_AREA_GE ? h * w >= 100.0f : h * w > 100.0f;
        if (!((w / W <= 1.0f) && (h / H <= 1.0f) && area && ns[(long)b * maxo + i] >= thresh)) continue;
        for (int q = 0; q < 4; ++q) {
          ob[((long)b * maxo + k) * 4 + q] = bx[q];
          if (sets & 2) b2[((long)b * maxo + k) * 4 + q] = bx[q];
        }
        if (sets & 1) os[(long)b * maxo + k] = ns[(long)b * maxo + i];
        if (sets & 4) s2[(long)b * maxo + k] = ns[(long)b * maxo + i];
        ++k;
      }
      oc[b] = k;
      if (sets & 8) c2[b] = k;
      if (f == F_TAIL_ROWS) continue;
      for (int i = k; i < maxo; ++i) {
        for (int q = 0; q < 4; ++q) {
          ob[((long)b * maxo + i) * 4 + q] = 0.f;
          if (sets & 2) b2[((long)b * maxo + i) * 4 + q] = 0.f;
        }
        if (sets & 1) os[(long)b * maxo + i] = 0.f;
        if (sets & 4) s2[(long)b * maxo + i] = 0.f;
      }
    }
  }
};

// ---- cases ----------------------------------------------------------------------------------------------------------
enum Op { STATS, BNBWD, COLSUM, BNACT, ATT_S, ATT_S_BWD, SMALL_DGRAD, ADD, POOL, ATT_T, ATT_CAT, OUT, PERM, FILTER, REFUSE, OP_COUNT };
inline const char* const kOpName[] = {"bn_stats", "bn_bwd", "colsum", "bnact", "att_s", "att_s_bwd", "small_dgrad", "add", "pool_drop",
                                      "att_t", "att_cat", "out_loss", "def_perm_crops", "def_filter", "refuse"};
enum Refuse { R_NONE = 0, R_POOL_BWD_ODD_H, R_POOL_BWD_ODD_W, R_CAT_BWD_C0, R_CAT_BWD_C3, R_CAT_BWD_C128 };
struct Case {
  std::string name;
  int op = STATS, refuse = R_NONE;
  uint32_t seed = 1;
  long M = 1;      // rows (column reductions, elementwise, att_t, out: B * HW)
  int C = 1;
  int B = 1, H = 2, W = 2;
  long HW = 1;
  int act = 1;     // 1 leaky, 0 identity
  int flav = 0;    // bn_stats: 1 moving statistics; out: 1 target = the output; att_cat: 1 saturated gates; filter: planted edges
  int data = 0;    // column reductions: 1 a channel at 1e3 x its spread and a constant channel
  int acc = 0;
  int layer = -1, gimg0 = 0;
  long step = 0;
  int O = 3, P = 1, maxo = 8, sets = 0, nc_mode = 0;  // nc_mode 0 mixed, 1 all zero, 2 all maxo, 3 all rejected
};

// ---- inputs ---------------------------------------------------------------------------------------------------------
inline VF uni(size_t n, uint64_t seed, float scale = 1.f, float shift = 0.f) {
  VF v(n);
  gck::fill_uni(v, seed, scale, shift);
  return v;
}
inline Bn make_bn(int C, uint64_t seed) {
  Bn b;
  b.mu = uni(C, seed, 0.3f, 0.1f);
  b.sc = uni(C, seed + 1, 0.5f, 1.2f);
  b.be = uni(C, seed + 2, 0.4f);
  return b;
}
inline E bn_z(float y, const Bn& b, int c) { return (E(y) - E(b.mu[c])) * E(b.sc[c]) + E(b.be[c]); }

// sum of fp64 terms folded in any order over `depth` additions each: depth 2^-53 sum |t|
inline double fold_bound(const ColredPlan& p, long double sabs) { return (double)((p.rpb + p.blocks + 72) * kU64 * sabs); }

// ---- column reductions ----------------------------------------------------------------------------------------------
inline VF colred_data(const Case& c, uint64_t seed) {
  VF y = uni((size_t)c.M * c.C, seed, 2.f, 0.3f);
  if (c.data) {
    for (long m = 0; m < c.M; ++m) {
      y[m * c.C] += 1000.f;                                  // a channel at 1e3 x its spread
      if (c.C > 1) y[m * c.C + c.C - 1] = 0.75f;            // a constant channel
    }
    if (c.data == 2) for (long m = 0; m < c.M; ++m) y[m * c.C] = -3.5f;  // C = 1: constant
  }
  return y;
}
inline bool part_written(const VD& part) {
  for (double d : part) if (std::isnan(d)) return false;
  return true;
}
inline void run_stats(const Case& c, Backend& be, Verdict& v) {
  const long M = c.M;
  const int C = c.C;
  const ColredPlan p = colred_plan(M, C);
  const VF y = colred_data(c, c.seed), gamma = uni(C, c.seed + 7, 0.5f, 1.1f);
  VF mm = uni(C, c.seed + 8, 0.5f), mv = uni(C, c.seed + 9, 0.4f, 1.f);
  const VF mm0 = mm, mv0 = mv;
  VF mean = filled(C), rstd = filled(C), sc = filled(C);
  VD part((size_t)p.blocks * C * 2, std::nan(""));
  be.bn_stats(y, M, C, gamma, c.flav == 1, mm, mv, mean, rstd, sc, part);
  v.flag("part_written", part_written(part));
  v.elems += M * C;
  for (int ch = 0; ch < C; ++ch) {
    // the terms t = y - y[0] are exact in fp64; mean = y[0] + sum t / M, var = sum (t - mean t)^2 / M
    const double y0 = y[ch];
    long double st = 0, sa = 0;
    for (long m = 0; m < M; ++m) { const double t = (double)y[m * C + ch] - y0; st += t; sa += std::fabs(t); }
    const long double mt = st / M;
    long double sq = 0, sq0 = 0;
    for (long m = 0; m < M; ++m) {
      const long double t = (double)y[m * C + ch] - y0;
      sq += (t - mt) * (t - mt); sq0 += t * t;
    }
    const double dm = (double)mt, var = (double)(sq / M), mu = y0 + dm;
    const double e_dm = fold_bound(p, sa) / M + kU64 * std::fabs(dm);
    const double e_mu = e_dm + kU64 * std::fabs(mu);
    const double e_var = fold_bound(p, sq0) / M + 2 * std::fabs(dm) * e_dm + e_dm * e_dm + 4 * kU64 * (double)(sq0 / M + dm * dm);
    const double rs = 1.0 / std::sqrt(var + 1e-3), e_rs = 0.5 * rs * rs * rs * e_var + 4 * kU64 * rs;
    v.cmp("mean", mean[ch], fstore(mu, e_mu));
    v.cmp("rstd", rstd[ch], fstore(rs, e_rs));
    v.cmp("sc", sc[ch], fstore(rs * gamma[ch], std::fabs(gamma[ch]) * e_rs + kU64 * rs * std::fabs(gamma[ch])));
    if (c.flav == 1) {
      const double f = M > 1 ? (double)M / (double)(M - 1) : 1.0, uvar = var * f;
      v.cmp("moving", mm[ch], fstore(mm0[ch] - (mm0[ch] - mu) * 0.01, 0.01 * e_mu + 4 * kU64 * (std::fabs(mm0[ch]) + std::fabs(mu))));
      v.cmp("moving", mv[ch], fstore(mv0[ch] - (mv0[ch] - uvar) * 0.01, 0.01 * f * e_var + 4 * kU64 * (std::fabs(mv0[ch]) + uvar)));
    }
  }
  if (c.flav != 1) v.flag("moving_untouched", same_bits(mm, mm0) && same_bits(mv, mv0));
}

inline void run_bnbwd(const Case& c, Backend& be, Verdict& v) {
  const long M = c.M;
  const int C = c.C;
  const ColredPlan p = colred_plan(M, C);
  const VF y = colred_data(c, c.seed), da = uni((size_t)M * C, c.seed + 3, 1.5f);
  VF mu(C), rstd(C), sc(C);
  const VF bet = uni(C, c.seed + 5, 0.4f), gamma = uni(C, c.seed + 7, 0.5f, 1.1f);
  for (int ch = 0; ch < C; ++ch) {  // the statistics a forward would have stored
    double s = 0, q = 0;
    for (long m = 0; m < M; ++m) s += y[m * C + ch];
    s /= M;
    for (long m = 0; m < M; ++m) q += (y[m * C + ch] - s) * (y[m * C + ch] - s);
    mu[ch] = (float)s; rstd[ch] = (float)(1.0 / std::sqrt(q / M + 1e-3)); sc[ch] = rstd[ch] * gamma[ch];
  }
  VF mdz = filled(C), mdzx = filled(C), dgamma = filled(C), dbeta = filled(C), dy = filled((size_t)M * C);
  VD part((size_t)p.blocks * C * 2, std::nan(""));
  be.bn_bwd(da, y, M, C, mu, rstd, sc, bet, c.act, mdz, mdzx, dgamma, dbeta, dy, part);
  v.flag("part_written", part_written(part));
  v.elems += M * C;
  for (int ch = 0; ch < C; ++ch) {
    long double s0 = 0, s1 = 0, a0 = 0, a1 = 0, e0 = 0, e1 = 0;
    for (long m = 0; m < M; ++m) {
      const long i = m * C + ch;
      const E yc = E(y[i]) - E(mu[ch]);
      E dz = E(da[i]);
      if (c.act) dz = dz * tleaky_grad(yc * E(sc[ch]) + E(bet[ch]), &v.kinks);
      const E xh = yc * E(rstd[ch]);
      const double t1 = dz.v * xh.v;
      s0 += dz.v; a0 += std::fabs(dz.v); e0 += dz.e;
      s1 += t1; a1 += std::fabs(t1); e1 += std::fabs(dz.v) * xh.e + std::fabs(xh.v) * dz.e + dz.e * xh.e + kU64 * std::fabs(t1);
      // dy from the coefficients the device itself stored: only the elementwise roundings remain
      v.cmp("dy", dy[i], E(sc[ch]) * (dz - E(mdz[ch]) - xh * E(mdzx[ch])));
    }
    const double b0 = (double)e0 + fold_bound(p, a0), b1 = (double)e1 + fold_bound(p, a1);
    v.cmp("dbeta", dbeta[ch], fstore((double)s0, b0));
    v.cmp("dgamma", dgamma[ch], fstore((double)s1, b1));
    v.cmp("mdz", mdz[ch], fstore((double)s0 / M, b0 / M + kU64 * std::fabs((double)s0 / M)));
    v.cmp("mdzx", mdzx[ch], fstore((double)s1 / M, b1 / M + kU64 * std::fabs((double)s1 / M)));
  }
}

inline void run_colsum(const Case& c, Backend& be, Verdict& v) {
  const ColredPlan p = colred_plan(c.M, c.C);
  const VF x = colred_data(c, c.seed);
  VF out = filled(c.C);
  VD part((size_t)p.blocks * c.C * 2, std::nan(""));
  be.colsum(x, c.M, c.C, out, part);
  v.flag("part_written", part_written(part));
  v.elems += c.M * c.C;
  for (int ch = 0; ch < c.C; ++ch) {
    long double s = 0, a = 0;
    for (long m = 0; m < c.M; ++m) { s += x[m * c.C + ch]; a += std::fabs(x[m * c.C + ch]); }
    v.cmp("sum", out[ch], fstore((double)s, fold_bound(p, a)));
  }
}

// ---- elementwise ----------------------------------------------------------------------------------------------------
inline void run_bnact(const Case& c, Backend& be, Verdict& v) {
  const long n = c.M * c.C;
  const VF y = uni(n, c.seed, 2.f, 0.2f);
  const Bn b = make_bn(c.C, c.seed + 10);
  VF a = filled(n);
  be.bnact(y, b, c.M, c.C, c.act, a);
  v.elems += n;
  for (long i = 0; i < n; ++i) {
    const E z = bn_z(y[i], b, (int)(i % c.C));
    v.cmp("a", a[i], c.act ? tleaky(z, &v.kinks) : z);
  }
}
inline void run_att_s(const Case& c, Backend& be, Verdict& v, bool bwd) {
  const long n = c.M * c.C;
  const VF g = uni(n, c.seed, 2.f), x = uni(n, c.seed + 1, 1.5f, 0.3f);
  const Bn b1 = make_bn(c.C, c.seed + 10), b2 = make_bn(c.C, c.seed + 20);
  v.elems += n;
  if (!bwd) {
    VF s = filled(n);
    be.att_s(g, x, b1, b2, c.M, c.C, s);
    for (long i = 0; i < n; ++i) {
      const int ch = (int)(i % c.C);
      v.cmp("s", s[i], tleaky(bn_z(g[i], b1, ch) + bn_z(x[i], b2, ch), &v.kinks));
    }
    return;
  }
  const VF dt = uni(c.M, c.seed + 2, 1.5f), w3 = uni(c.C, c.seed + 3, 0.8f);
  VF ds = filled(n);
  be.att_s_bwd(dt, w3, g, x, b1, b2, c.M, c.C, ds);
  for (long i = 0; i < n; ++i) {
    const int ch = (int)(i % c.C);
    v.cmp("dsum", ds[i], E(dt[i / c.C]) * E(w3[ch]) * tleaky_grad(bn_z(g[i], b1, ch) + bn_z(x[i], b2, ch), &v.kinks));
  }
}
inline void run_small_dgrad(const Case& c, Backend& be, Verdict& v) {
  const long n = c.M * c.C;
  const VF dz = uni(c.M * c.O, c.seed, 1.5f), w = uni((size_t)c.C * c.O, c.seed + 1, 0.9f), old = uni(n, c.seed + 2, 2.f);
  VF dx = c.acc ? old : filled(n);
  be.small_dgrad(dz, w, dx, c.M, c.C, c.O, c.acc != 0);
  v.elems += n;
  for (long i = 0; i < n; ++i) {
    E s(0.0);
    for (int o = 0; o < c.O; ++o) s = tfma(E(dz[i / c.C * c.O + o]), E(w[i % c.C * c.O + o]), s);
    v.cmp("dx", dx[i], c.acc ? E(old[i]) + s : s);
  }
}
inline void run_add(const Case& c, Backend& be, Verdict& v) {
  const long n = c.M;
  const VF a0 = uni(n, c.seed, 2.f), b = uni(n, c.seed + 1, 3.f);
  VF a = a0;
  be.add(a, b, n);
  bool ok = true;
  for (long i = 0; i < n; ++i) ok &= f2u(a[i]) == f2u(a0[i] + b[i]);  // one IEEE addition: exact
  v.flag("a_exact", ok);
  v.elems += n;
}
inline void run_att_t(const Case& c, Backend& be, Verdict& v) {
  const VF s = uni(c.M * c.C, c.seed, 2.f), w = uni(c.C, c.seed + 1, 0.9f);
  const float b = 0.37f;
  VF t = filled(c.M);
  be.att_t(s, w, b, c.M, c.C, t);
  v.elems += c.M;
  for (long m = 0; m < c.M; ++m) {
    E acc(0.0);
    for (int ch = 0; ch < c.C; ++ch) acc = tfma(E(s[m * c.C + ch]), E(w[ch]), acc);
    v.cmp("t", t[m], acc + E(b));
  }
}

// ---- pool + Dropout -------------------------------------------------------------------------------------------------
inline bool keep_of(const Rk& k, const Golden::Drop* g, long e, int b) { return g ? g->keep[b][e] == '1' : keep_flag(k, e, b); }
// every keep flag of the case: the golden file's where it holds the draw, held equal to keep_flag()
inline const Golden::Drop* golden_drop(const Rk& k, int B, long per, Verdict& v) {
  if (k.layer < 0 || B * per > kGoldenMaxFlags) return nullptr;
  const Golden::Drop* g = g_golden.drop(k, B, per);
  v.flag("golden_found", g != nullptr);
  if (!g) return nullptr;
  bool same = true;
  for (int b = 0; b < B; ++b)
    for (long e = 0; e < per; ++e) same &= (g->keep[b][e] == '1') == keep_flag(k, e, b);
  v.flag("golden_is_philox", same);
  v.golden_used = true;
  return g;
}
inline void run_pool(const Case& c, Backend& be, Verdict& v) {
  const int B = c.B, H = c.H, W = c.W, C = c.C, Ho = H / 2, Wo = W / 2;
  const long per = (long)Ho * Wo * C, n = B * per, nin = (long)B * H * W * C;
  const Rk k{0x5eed0000beefull, c.step, c.gimg0, c.layer};
  VF x(nin);
  {  // eighths, so exact ties occur
    gck::Rng r(c.seed);
    for (auto& e : x) e = (float)((int)(r.next() % 33) - 16) * 0.125f;
  }
  VF out = filled(n);
  VB arg(n, 0xEE);
  be.pool(x, B, H, W, C, k, out, arg);
  const Golden::Drop* gd = golden_drop(k, B, per, v);
  v.elems += n;
  bool out_ok = true, arg_ok = true;
  long ties = 0;
  VB want_arg(n);
  for (long i = 0; i < n; ++i) {
    const int ch = (int)(i % C), ox = (int)(i / C % Wo), oy = (int)(i / C / Wo % Ho), b = (int)(i / per);
    const long base = (((long)b * H + 2 * oy) * W + 2 * ox) * C + ch;
    const float t[4] = {x[base], x[base + C], x[base + (long)W * C], x[base + (long)W * C + C]};
    int am = 0;
    for (int q = 1; q < 4; ++q) if (t[q] > t[am]) am = q;  // the first maximum in row-major order
    for (int q = 0; q < 4; ++q) ties += q != am && t[q] == t[am];
    want_arg[i] = (uint8_t)am;
    // m * 1.25 is exact for eighths
    const float want = c.layer < 0 ? t[am] : keep_of(k, gd, i - b * per, b) ? t[am] * kDropScale : 0.f;
    out_ok &= f2u(out[i]) == f2u(want);
    arg_ok &= arg[i] == am;
  }
  v.flag("out_exact", out_ok);
  v.flag("arg_exact", arg_ok);
  v.flag("has_ties", ties > 0 || n < 4);
  if (c.layer < 0) return;
  // the backward: the exact adjoint, replayed store by store; taps from the forward and from a map holding all four
  const VF dout = uni(n, c.seed + 1, 2.f), old = uni(nin, c.seed + 2, 3.f);
  VB map4(n);
  for (long i = 0; i < n; ++i) map4[i] = (uint8_t)((i * 7 + i / 3) & 3);
  const bool odd = (H | W) & 1;
  for (int which = 0; which < 2; ++which)
    for (int acc = odd ? 1 : 0; acc < 2; ++acc) {
      const VB& ar = which ? map4 : want_arg;
      VF dx = acc ? old : filled(nin);
      v.threw |= be.pool_bwd(dout, ar, dx, B, H, W, C, k, acc != 0);
      VF want = acc ? old : filled(nin);
      bool dropped_zero = true;
      for (long i = 0; i < n; ++i) {
        const int ch = (int)(i % C), ox = (int)(i / C % Wo), oy = (int)(i / C / Wo % Ho), b = (int)(i / per);
        const long base = (((long)b * H + 2 * oy) * W + 2 * ox) * C + ch;
        const long off[4] = {0, C, (long)W * C, (long)W * C + C};
        const bool kp = keep_of(k, gd, i - b * per, b);
        const float g = kp ? dout[i] * kDropScale : 0.f;
        for (int q = 0; q < 4; ++q) {
          const float val = q == ar[i] ? g : 0.f;
          if (acc) want[base + off[q]] += val;
          else want[base + off[q]] = val;
          if (!acc && !kp) dropped_zero &= f2u(dx[base + off[q]]) == 0u;
        }
      }
      v.flag(std::string("dx_exact_") + (which ? "map" : "fwd") + (acc ? "_acc" : ""), same_bits(dx, want));
      if (!acc) v.flag("dropped_taps_zero", dropped_zero);
    }
}

// ---- the attention gate's concat ------------------------------------------------------------------------------------
struct CatIn {
  VF up, skip, t, dcat;
  float bn3[3];
};
inline CatIn cat_inputs(const Case& c) {
  const long M = (long)c.B * c.HW;
  CatIn in;
  in.up = uni(M * c.C, c.seed, 2.f);
  in.skip = uni(M * c.C, c.seed + 1, 1.5f, 0.2f);
  in.t = uni(M, c.seed + 2, 1.5f, 0.25f);
  in.dcat = uni(M * 2 * c.C, c.seed + 3, 2.f);
  in.bn3[0] = 0.25f; in.bn3[1] = 2.f; in.bn3[2] = -0.5f;
  if (c.flav == 1) {  // bn3 outputs of +-20 and +-90: z = (t - 0.25) * 2 - 0.5
    const float zs[4] = {20.f, -20.f, 90.f, -90.f};
    for (long m = 0; m < M; ++m) if (m % 2 == 0) in.t[m] = (zs[(m / 2) % 4] + 0.5f) / 2.f + 0.25f;
  }
  return in;
}
inline void run_att_cat(const Case& c, Backend& be, Verdict& v) {
  const int B = c.B, C = c.C;
  const long HW = c.HW, M = B * HW, per = HW * 2 * C;
  const Rk k{0x5eed0000cafeull, c.step, c.gimg0, c.layer};
  const CatIn in = cat_inputs(c);
  VF cat = filled(M * 2 * C);
  be.att_cat(in.up, in.skip, in.t, in.bn3, B, HW, C, k, cat);
  const Golden::Drop* gd = golden_drop(k, B, per, v);
  v.elems += M * 2 * C;
  std::vector<E> a(M);
  for (long m = 0; m < M; ++m) a[m] = tsigmoid((E(in.t[m]) - E(in.bn3[0])) * E(in.bn3[1]) + E(in.bn3[2]));
  bool up_ok = true, zero_ok = true;
  for (long i = 0; i < M * 2 * C; ++i) {
    const int c2 = (int)(i % (2 * C)), b = (int)(i / per);
    const long m = i / (2 * C);
    const bool kp = c.layer < 0 || keep_of(k, gd, i - b * per, b);
    if (!kp) { zero_ok &= f2u(cat[i]) == 0u; continue; }
    if (c2 < C) {  // a move (times the Dropout scale: one IEEE product)
      const float u = in.up[m * C + c2];
      up_ok &= f2u(cat[i]) == f2u(c.layer < 0 ? u : u * kDropScale);
    } else {
      E want = E(in.skip[m * C + c2 - C]) * a[m];
      if (c.layer >= 0) want = want * E(kDropScale);
      v.cmp("cat", cat[i], want);
    }
  }
  v.flag("up_exact", up_ok);
  v.flag("dropped_zero", zero_ok);
  if (c.layer < 0) return;
  VF dup = filled(M * C), dskip = filled(M * C), dz3 = filled(M);
  v.threw |= be.att_cat_bwd(in.dcat, in.skip, in.t, in.bn3, B, HW, C, k, dup, dskip, dz3);
  bool dup_ok = true;
  int levels = 0;
  while ((1 << levels) < C) ++levels;
  for (long m = 0; m < M; ++m) {
    const int b = (int)(m / HW);
    const long e = (m - b * HW) * 2 * C;
    double s = 0, sa = 0, se = 0;
    for (int ch = 0; ch < C; ++ch) {
      const float d0 = in.dcat[m * 2 * C + ch], d1 = in.dcat[m * 2 * C + C + ch];
      const float g0 = keep_of(k, gd, e + ch, b) ? d0 * kDropScale : 0.f;
      dup_ok &= f2u(dup[m * C + ch]) == f2u(g0);
      const E g1 = keep_of(k, gd, e + C + ch, b) ? E(d1) * E(kDropScale) : E(0.0);
      v.cmp("dskip", dskip[m * C + ch], g1 * a[m]);
      const E t = g1 * E(in.skip[m * C + ch]);
      s += t.v; sa += std::fabs(t.v); se += t.e;
    }
    // the dot product folds in a tree of log2 C levels
    const E da(s, se + levels * kU * (sa + se) + kDen);
    v.cmp("dz3", dz3[m], da * (a[m] * (E(1.0) - a[m])));
  }
  v.flag("dup_exact", dup_ok);
}
// the analytic backward above against central differences of the fp64 forward (M 3, C 4): worst relative gap
inline double cat_bwd_fd_gap() {
  const int M = 3, C = 4;
  const double h = 1e-6;
  Case c;
  c.B = 1; c.HW = M; c.C = C; c.seed = 77;
  const CatIn in = cat_inputs(c);
  const Rk k{0x5eed0000cafeull, 3, 1, 5};
  std::vector<double> skip(in.skip.begin(), in.skip.end()), z(M);
  for (int m = 0; m < M; ++m) z[m] = ((double)in.t[m] - in.bn3[0]) * in.bn3[1] + in.bn3[2];
  auto loss = [&](const std::vector<double>& sk, const std::vector<double>& zz) {  // sum dcat . cat over the skip half
    double L = 0;
    for (int m = 0; m < M; ++m)
      for (int ch = 0; ch < C; ++ch)
        if (keep_flag(k, (long)m * 2 * C + C + ch, 0)) L += (double)in.dcat[m * 2 * C + C + ch] * 1.25 * sk[m * C + ch] / (1.0 + std::exp(-zz[m]));
    return L;
  };
  double gap = 0;
  for (int m = 0; m < M; ++m) {
    const double a = 1.0 / (1.0 + std::exp(-z[m]));
    double dz3 = 0;
    for (int ch = 0; ch < C; ++ch) {
      const double g1 = keep_flag(k, (long)m * 2 * C + C + ch, 0) ? (double)in.dcat[m * 2 * C + C + ch] * 1.25 : 0.0;
      dz3 += g1 * skip[m * C + ch];
      auto sp = skip, sm = skip;
      sp[m * C + ch] += h; sm[m * C + ch] -= h;
      const double num = (loss(sp, z) - loss(sm, z)) / (2 * h), ana = g1 * a;
      gap = std::max(gap, std::fabs(num - ana) / std::max(1.0, std::fabs(ana)));
    }
    dz3 *= a * (1.0 - a);
    auto zp = z, zm = z;
    zp[m] += h; zm[m] -= h;
    const double num = (loss(skip, zp) - loss(skip, zm)) / (2 * h);
    gap = std::max(gap, std::fabs(num - dz3) / std::max(1.0, std::fabs(dz3)));
  }
  return gap;
}

// ---- the output layer and its loss ----------------------------------------------------------------------------------
inline void run_out(const Case& c, Backend& be, Verdict& v) {
  const long M = c.M, HW = c.HW;
  const int C = c.C;
  // pre-activations out to |z| = 12: rows scaled up towards the end of the range
  VF x = uni(M * C, c.seed, 1.f);
  for (long m = 0; m < M; ++m) {
    const float s = 0.5f + 11.5f * (float)(m % 97) / 96.f;
    for (int ch = 0; ch < C; ++ch) x[m * C + ch] *= s;
  }
  VF w = uni((size_t)C * 3, c.seed + 1, 1.f), b = uni(3, c.seed + 2, 0.3f);
  for (auto& e : w) e /= (float)std::sqrt((double)C);
  if (C == 1) w[0] = 1.0f;
  VF upd1 = filled(M * 3);
  be.out(x, w, b, M, C, upd1);
  VF tgt = uni(M * 3, c.seed + 3, 2.f);
  if (c.flav == 1) tgt = upd1;  // a target equal to the output
  const int nb = loss_blocks(M);
  VF upd = filled(M * 3), dz = filled(M * 3), loss = filled(1);
  VD lpart(nb, std::nan(""));
  be.out_loss(x, w, b, tgt, M, HW, C, upd, dz, lpart, loss);
  v.flag("upd_bit_equal", same_bits(upd, upd1));
  v.flag("part_written", part_written(lpart));
  v.elems += M * 3;
  const E inv = E(1.0) / E((double)(float)(HW * 3));
  double zmax = 0;
  long double L = 0, Le = 0;
  for (long m = 0; m < M; ++m)
    for (int o = 0; o < 3; ++o) {
      E z(b[o]);
      for (int ch = 0; ch < C; ++ch) z = tfma(E(x[m * C + ch]), E(w[ch * 3 + o]), z);
      zmax = std::max(zmax, std::fabs(z.v));
      const E th = ttanh(z), u = E(2.0) * th;
      v.cmp("upd", upd[m * 3 + o], u);
      if (c.flav == 1) continue;
      const E d = E(tgt[m * 3 + o]) - u;
      v.cmp("dz", dz[m * 3 + o], (E(-2.0) * d * inv) * E(2.0) * (E(1.0) - th * th));
      L += d.v * d.v / (double)(HW * 3);
      Le += (2 * std::fabs(d.v) * d.e + d.e * d.e) / (double)(HW * 3);
    }
  v.flag("z_reaches_8", zmax >= 8.0 || M < 4);
  if (c.flav == 1) {
    bool z0 = true;
    for (float e : dz) z0 &= (f2u(e) & 0x7fffffffu) == 0u;
    v.flag("loss_zero", f2u(loss[0]) == 0u && z0);
    return;
  }
  // each thread adds its rows' terms, the workgroup folds 256 lanes, one thread adds the blocks
  const double depth = (double)cdivl(M, (long)nb * 256) * 3 + 8 + nb + 4;
  v.cmp("loss", loss[0], fstore((double)L, (double)Le + depth * kU64 * (double)(L + Le)));
}

// ---- the Masker's extras --------------------------------------------------------------------------------------------
inline void run_perm(const Case& c, Backend& be, Verdict& v) {
  const int B = c.B, H = c.H, W = c.W, P = c.P;
  const Rk k{0x5eed0000d00dull, c.step, c.gimg0, 0};
  VF img((size_t)B * H * W * 3);
  for (size_t i = 0; i < img.size(); ++i) img[i] = (float)(i % 100003) * 0.25f - 7.f;  // every element its own value
  VI info((size_t)B * 3, (int)0xCBCBCBCB);
  VF crops = filled((size_t)B * P * P * 3);
  be.perm_crops(img, B, H, W, P, k, info, crops);
  const Golden::Perm* g = g_golden.perm(k, B);
  v.flag("golden_found", g != nullptr);
  v.golden_used = g != nullptr;
  const VI mine = shuffle_perm(k, B);
  std::vector<char> seen(B, 0);
  bool perm_ok = true, info_ok = true, crops_ok = true, gold_ok = g != nullptr;
  for (int b = 0; b < B; ++b) {
    int lr, ud;
    flips(k, b, &lr, &ud);
    if (g) gold_ok &= g->perm[b] == mine[b] && g->lr[b] == lr && g->ud[b] == ud;
    const int src = g ? g->perm[b] : mine[b];
    const int got = info[b * 3];
    if (got < 0 || got >= B || seen[got]) perm_ok = false;
    else seen[got] = 1;
    info_ok &= got == src && info[b * 3 + 1] == (g ? g->lr[b] : lr) && info[b * 3 + 2] == (g ? g->ud[b] : ud);
    for (int y = 0; y < P; ++y)
      for (int x = 0; x < P; ++x)
        for (int q = 0; q < 3; ++q)
          crops_ok &= f2u(crops[(((long)b * P + y) * P + x) * 3 + q]) ==
                      f2u(img[(((long)src * H + (ud ? P - 1 - y : y)) * W + (lr ? P - 1 - x : x)) * 3 + q]);
  }
  v.flag("golden_is_philox", gold_ok);
  v.flag("perm_is_permutation", perm_ok);
  v.flag("info_exact", info_ok);
  v.flag("crops_exact", crops_ok);
  v.elems += B;
}

struct FilterIn { VF nb, ns; VI nc; };
inline FilterIn filter_inputs(const Case& c, float Hf, float Wf, float thresh) {
  const int B = c.B, maxo = c.maxo;
  FilterIn in;
  in.nb.resize((size_t)B * maxo * 4); in.ns.resize((size_t)B * maxo); in.nc.resize(B);
  gck::Rng r(c.seed);
  for (int b = 0; b < B; ++b) {
    in.nc[b] = c.nc_mode == 1 ? 0 : c.nc_mode == 2 ? maxo : (int)(r.next() % (maxo + 1));
    for (int i = 0; i < maxo; ++i) {
      // quarter-pixel corners: the differences and the area are exact in fp32
      const float y0 = (float)(r.next() % 400) * 0.25f, x0 = (float)(r.next() % 400) * 0.25f;
      float h = (float)(r.next() % 240 + 1) * 0.25f, w = (float)(r.next() % 240 + 1) * 0.25f;
      float s = (float)(r.next() % 1000) * 0.001f;
      float yy = y0, xx = x0;
      switch (c.nc_mode == 3 ? 100 + (int)(r.next() % 3) : (int)(r.next() % 12)) {
        case 0: w = Wf; xx = 0.f; break;               // w / W exactly 1: kept
        case 1: h = 10.f; w = 10.f; break;             // area exactly 100: rejected
        case 2: s = thresh; break;                     // the score exactly at the threshold: kept
        case 3: h = Hf; yy = 0.f; break;
        case 4: w = Wf + 0.25f; xx = 0.f; break;       // just wider than the image
        case 100: h = 8.f; w = 12.5f; break;           // all rejected: area 100, low score, too tall
        case 101: s = thresh * 0.5f; break;
        case 102: h = Hf + 1.f; yy = 0.f; break;
        default: break;
      }
      float* bx = &in.nb[((size_t)b * maxo + i) * 4];
      bx[0] = yy; bx[1] = xx; bx[2] = yy + h; bx[3] = xx + w;
      in.ns[(size_t)b * maxo + i] = s;
    }
  }
  return in;
}
inline void run_filter(const Case& c, Backend& be, Verdict& v) {
  const int B = c.B, maxo = c.maxo;
  const float Hf = 64.f, Wf = 96.f, thresh = 0.375f;
  const FilterIn in = filter_inputs(c, Hf, Wf, thresh);
  VF ob = filled((size_t)B * maxo * 4), os = filled((size_t)B * maxo), b2 = filled((size_t)B * maxo * 4), s2 = filled((size_t)B * maxo);
  VI oc(B, (int)0xCBCBCBCB), c2(B, (int)0xCBCBCBCB);
  const VF os0 = os, b20 = b2, s20 = s2;
  const VI c20 = c2;
  be.filter(in.nb, in.ns, in.nc, B, maxo, Hf, Wf, thresh, c.sets, ob, oc, os, b2, s2, c2);
  VF wb((size_t)B * maxo * 4, 0.f), ws((size_t)B * maxo, 0.f);  // rows past the count are +0
  VI wc(B);
  long kept = 0, edge_w1 = 0, edge_a100 = 0, edge_thr = 0;
  for (int b = 0; b < B; ++b) {
    int k = 0;
    for (int i = 0; i < in.nc[b]; ++i) {
      const float* bx = &in.nb[((size_t)b * maxo + i) * 4];
      const double h = (double)bx[2] - bx[0], w = (double)bx[3] - bx[1], s = in.ns[(size_t)b * maxo + i];
      edge_w1 += w == Wf; edge_a100 += h * w == 100.0; edge_thr += s == thresh;
      if (!(w <= Wf && h <= Hf && h * w > 100.0 && s >= thresh)) continue;
      std::memcpy(&wb[((size_t)b * maxo + k) * 4], bx, 16);
      ws[(size_t)b * maxo + k] = (float)s;
      ++k;
    }
    wc[b] = k;
    kept += k;
  }
  v.flag("boxes_exact", same_bits(ob, wb));
  v.flag("count_exact", oc == wc);
  v.flag("scores_exact", (c.sets & 1) ? same_bits(os, ws) : same_bits(os, os0));
  v.flag("set2_exact", ((c.sets & 2) ? same_bits(b2, wb) : same_bits(b2, b20)) && ((c.sets & 4) ? same_bits(s2, ws) : same_bits(s2, s20)) &&
                           ((c.sets & 8) ? c2 == wc : c2 == c20));
  if (c.flav == 1) v.flag("edges_planted", edge_w1 > 0 && edge_a100 > 0 && edge_thr > 0 && kept > 0);
  if (c.nc_mode == 3) v.flag("all_rejected", kept == 0);
  v.elems += (long)B * maxo;
}

// ---- refusals: the launcher throws before anything is launched, every output keeps its fill -------------------------
inline void run_refuse(const Case& c, Backend& be, Verdict& v) {
  const Rk k{0x5eed0000f00dull, 1, 0, c.layer};
  if (c.refuse == R_POOL_BWD_ODD_H || c.refuse == R_POOL_BWD_ODD_W) {
    const long n = (long)c.B * (c.H / 2) * (c.W / 2) * c.C, nin = (long)c.B * c.H * c.W * c.C;
    const VF dout = uni(n, c.seed, 1.f);
    const VB arg(n, 1);
    VF dx = filled(nin);
    v.threw = be.pool_bwd(dout, arg, dx, c.B, c.H, c.W, c.C, k, false);
    v.untouched = same_bits(dx, filled(nin));
    return;
  }
  // att_cat_bwd with C 0, 3, 128: buffers sized for C = max(C, 1)
  const int Cb = std::max(c.C, 1);
  const long M = (long)c.B * c.HW;
  const VF dcat = uni(M * 2 * Cb, c.seed, 1.f), skip = uni(M * Cb, c.seed + 1, 1.f), t = uni(M, c.seed + 2, 1.f);
  const float bn3[3] = {0.f, 1.f, 0.f};
  VF dup = filled(M * Cb), dskip = filled(M * Cb), dz3 = filled(M);
  v.threw = be.att_cat_bwd(dcat, skip, t, bn3, c.B, c.HW, c.C, k, dup, dskip, dz3);
  v.untouched = same_bits(dup, filled(M * Cb)) && same_bits(dskip, filled(M * Cb)) && same_bits(dz3, filled(M));
}

inline void run_case(const Case& c, Backend& be, Verdict& v) {
  switch (c.op) {
    case STATS: run_stats(c, be, v); break;
    case BNBWD: run_bnbwd(c, be, v); break;
    case COLSUM: run_colsum(c, be, v); break;
    case BNACT: run_bnact(c, be, v); break;
    case ATT_S: run_att_s(c, be, v, false); break;
    case ATT_S_BWD: run_att_s(c, be, v, true); break;
    case SMALL_DGRAD: run_small_dgrad(c, be, v); break;
    case ADD: run_add(c, be, v); break;
    case POOL: run_pool(c, be, v); break;
    case ATT_T: run_att_t(c, be, v); break;
    case ATT_CAT: run_att_cat(c, be, v); break;
    case OUT: run_out(c, be, v); break;
    case PERM: run_perm(c, be, v); break;
    case FILTER: run_filter(c, be, v); break;
    default: run_refuse(c, be, v); break;
  }
}

inline std::string jnum(double x) {
  char b[40];
  if (std::isfinite(x)) snprintf(b, sizeof b, "%.6g", x);
  else snprintf(b, sizeof b, "1e308");
  return b;
}
inline std::string verdict_json(const Verdict& v) {
  std::string s = "\"fields\":{";
  bool first = true;
  for (auto& f : v.fields) { s += (first ? "\"" : ",\"") + f.first + "\":" + jnum(f.second); first = false; }
  s += "},\"flags\":{";
  first = true;
  for (auto& f : v.flags) { s += (first ? "\"" : ",\"") + f.first + "\":" + (f.second ? "true" : "false"); first = false; }
  s += "},\"ratio\":" + jnum(v.ratio()) + ",\"exact_ok\":" + (v.exact_ok() ? "true" : "false") + ",\"nonfinite\":" + std::to_string(v.nonfinite) +
       ",\"kink_share\":" + jnum(v.kink_share()) + ",\"threw\":" + (v.threw ? "true" : "false") + ",\"untouched\":" + (v.untouched ? "true" : "false") +
       ",\"golden_used\":" + (v.golden_used ? "true" : "false");
  return s;
}

}  // namespace uck
