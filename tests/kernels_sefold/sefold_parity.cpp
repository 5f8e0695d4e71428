// sefold_parity.cpp — kernel-level parity of the squeeze-excite backward whose input gradient is formed on
// load by the depthwise dgrad (launch_se_bwd_sums, launch_dw_bwd_se, launch_se_da)
// against an fp64 host reference and, bit for bit, against the launchers it stands in for, after the
// pattern of tests/kernels/norm_parity: one process, one stream, only the launchers of kernels.hpp, one
// JSON line per named case and a `done` line.  The references, views and bounds are those of
// norm_check.hpp / conv_check.hpp / gemm_check.hpp (read-only).
#include <cmath>
#include <cstring>
#include <functional>
#include <stdexcept>

#include "../kernels/norm_check.hpp"
#include "../kernels/parity_dev.hpp"
#include "kernels.hpp"

using namespace phx;
using gck::kEps24;
using nck::kEps53;

static hipStream_t g_st;

static const float* F(const Guarded& g) { return reinterpret_cast<const float*>(g.out()); }
static void outf(Guarded& g, size_t floats) {
  g.alloc(floats * 4);
  g.fill32(gck::kUnwritten);
  g.upload();
}
static bool untouched(Guarded& g) {
  g.download();
  return g.got == g.init;
}

// a training-mode BN's stored parameters: mean, rstd, gamma * rstd, beta, and backward means
struct Bn {
  std::vector<float> mu, rs, sc, be, m1, m2;
  Dev dmu, drs, dsc, dbe, dm1, dm2;
  void gen(int C, uint64_t seed) {
    mu.resize(C); rs.resize(C); sc.resize(C); be.resize(C); m1.resize(C); m2.resize(C);
    gck::fill_uni(mu, seed, 0.3f);
    gck::fill_uni(rs, seed + 1, 0.4f, 1.2f);
    gck::fill_uni(sc, seed + 2, 0.3f, 1.0f);
    for (int c = 0; c < C; ++c) sc[c] *= rs[c];
    gck::fill_uni(be, seed + 3, 0.4f);
    gck::fill_uni(m1, seed + 4, 0.05f);
    gck::fill_uni(m2, seed + 5, 0.05f);
    put_f(dmu, mu); put_f(drs, rs); put_f(dsc, sc); put_f(dbe, be); put_f(dm1, m1); put_f(dm2, m2);
  }
};

struct Verdict {
  std::string name, what;
  bool refuse = false, threw = false, untouched_ok = true, guards_ok = true, slot_ok = true;
  std::vector<std::pair<std::string, nck::Field>> fields;
  double sink1 = 0, sink2 = 0;
  bool has_sink = false, rows_written = true;
  void field(const char* n, const nck::Field& f) { fields.emplace_back(n, f); }
  void print() const {
    double ratio = 0;
    long nonfinite = 0;
    std::string fs;
    for (auto& kv : fields) {
      ratio = std::max(ratio, kv.second.ratio);
      nonfinite += kv.second.nonfinite;
      fs += (fs.empty() ? "\"" : ",\"") + kv.first + "\":" + num(kv.second.ratio);
    }
    bool pass;
    if (refuse) pass = threw && untouched_ok;
    else
      pass = !threw && ratio <= 1.0 && nonfinite == 0 && guards_ok && slot_ok &&
             (!has_sink || (rows_written && sink1 <= 1.0 && sink2 <= 1.0));
    printf("{\"case\":\"%s\",\"refuse\":%s,\"threw\":%s,\"what\":\"%s\",\"untouched\":%s,\"ratio\":%s,\"nonfinite\":%ld,"
           "\"fields\":{%s},\"guards_ok\":%s,\"slot_ok\":%s,\"has_sink\":%s,\"rows_written\":%s,\"sum_ratio\":%s,"
           "\"m2_ratio\":%s,\"pass\":%s}\n",
           name.c_str(), refuse ? "true" : "false", threw ? "true" : "false", esc(what).c_str(),
           untouched_ok ? "true" : "false", num(ratio).c_str(), nonfinite, fs.c_str(), guards_ok ? "true" : "false",
           slot_ok ? "true" : "false", has_sink ? "true" : "false", rows_written ? "true" : "false", num(sink1).c_str(),
           num(sink2).c_str(), pass ? "true" : "false");
    fflush(stdout);
  }
};

static bool go(Verdict& v, const std::function<void()>& fn) {
  try {
    fn();
  } catch (const std::exception& e) {
    v.threw = true;
    v.what = e.what();
  }
  CK(hipStreamSynchronize(g_st));
  return !v.threw;
}

// ---- the sums pass --------------------------------------------------------------------------------
struct SeIn {
  int B, HW, C, N;
  bool bf;
  std::vector<float> y, dy, scale, hidden, w1, w2t;
  Dev dY, dDy, dScale, dHidden, dW1, dW2t;
  Bn bn;
  void gen(int B_, int HW_, int C_, int N_, bool bf_, uint64_t seed) {
    B = B_; HW = HW_; C = C_; N = N_; bf = bf_;
    const size_t n = (size_t)B * HW * C;
    y.resize(n); dy.resize(n); scale.resize((size_t)B * C); hidden.resize((size_t)B * N);
    w1.resize((size_t)C * N); w2t.resize((size_t)C * N);
    gck::fill_uni(y, seed, 1.5f, 0.2f);
    gck::fill_uni(dy, seed + 1);
    gck::fill_uni(scale, seed + 2, 0.45f, 0.5f);  // distinct per image
    gck::fill_uni(hidden, seed + 3, 3.0f);
    gck::fill_uni(w1, seed + 4, 2.0f / std::sqrt((float)C));
    gck::fill_uni(w2t, seed + 5, 2.0f / std::sqrt((float)N));
    bn.gen(C, seed + 10);
    if (bf) put_bf(dY, y);
    else put_f(dY, y);
    put_f(dDy, dy); put_f(dScale, scale); put_f(dHidden, hidden); put_f(dW1, w1); put_f(dW2t, w2t);
  }
  InX inx() const { return InX{dY.f(), bn.dmu.f(), bn.dsc.f(), bn.dbe.f(), 1, bf ? 1 : 0}; }
  GradSink sink(Guarded& part) const {
    return GradSink{reinterpret_cast<float2*>(part.ptr()), C, 0, dY.f(), bn.dmu.f(), bn.drs.f(), bn.dsc.f(), bn.dbe.f(), 1,
                    bf ? 1 : 0};
  }
  nck::SeShape shape() const {
    const SePlanInfo sp = se_plan_info(B, C, N, red_plan_info(HW, C, B).chunks);
    return nck::SeShape{B, HW, C, N, 1, sp.s1, sp.cs1, sp.jg};
  }
};

// one SE backward: the sums pass (STORE = false) or launch_se_bwd (the apply pass, which also stores da)
struct SeOut {
  Guarded scratch, dpool, part, da;
  int P = 0, Pexp = 0;
  void alloc(const SeIn& in, bool store) {
    scratch.alloc(colred_scratch_doubles(in.HW, in.C, in.B) * 8);
    scratch.fill32(gck::kUnwritten);
    scratch.upload();
    outf(dpool, (size_t)in.B * in.C);
    Pexp = ew_gstats_partials(in.HW, in.C, in.B);
    outf(part, (size_t)in.C * Pexp * 2);
    if (store) outf(da, (size_t)in.B * in.HW * in.C);
  }
  void sums(const SeIn& in) {
    P = launch_se_bwd_sums(in.dDy.f(), in.inx(), in.B, in.HW, in.C, in.N, in.dW1.f(), in.dW2t.f(), 1, in.dHidden.f(),
                           in.dScale.f(), dpool.ptr(), g_st, reinterpret_cast<double*>(scratch.ptr()), in.sink(part));
  }
  void apply(const SeIn& in) {
    P = launch_se_bwd(in.dDy.f(), in.inx(), da.ptr(), in.B, in.HW, in.C, in.N, in.dW1.f(), nullptr, in.dW2t.f(), nullptr, 1,
                      nullptr, in.dHidden.f(), in.dScale.f(), dpool.ptr(), false, g_st,
                      reinterpret_cast<double*>(scratch.ptr()), in.sink(part));
  }
  bool download() {
    scratch.download(); dpool.download(); part.download();
    bool ok = scratch.intact() && dpool.intact() && part.intact();
    if (da.d) {
      da.download();
      ok = ok && da.intact();
    }
    return ok;
  }
};

static std::vector<float> se_da(const float* dy, const float* s, const float* dpool, float inv, int B, long px_per_img,
                                int C) {
  std::vector<float> da((size_t)B * px_per_img * C);
  for (int b = 0; b < B; ++b)
    for (long p = 0; p < px_per_img; ++p)
      for (int c = 0; c < C; ++c) {
        const size_t e = ((size_t)b * px_per_img + p) * C + c;
        const float q = dpool[b * C + c] * inv;  // one rounding, as the device's
        da[e] = std::fmaf(dy[e], s[b * C + c], q);
      }
  return da;
}

static nck::Field bits_equal(const void* a, const void* b, size_t bytes) {
  nck::Field f;
  f.ratio = std::memcmp(a, b, bytes) == 0 ? 0.0 : (double)INFINITY;
  return f;
}

// dpool against fp64 (se_bwd_ref) and the GradSink partials against fp64 (check_gradsink over the float
// da = fmaf(dy, s, fl(dpool fl(1 / HW))) formed on the host from the dpool the device stored: one
// correctly rounded operation each, so the host holds the device's da bit for bit)
static void check_sums(Verdict& v, const SeIn& in, SeOut& o) {
  v.guards_ok = v.guards_ok && o.download();
  const cck::Val xv = cck::view_inx(cck::BnView{in.y.data(), in.bn.mu.data(), in.bn.sc.data(), in.bn.be.data(), 1},
                                    (long)in.B * in.HW, in.C);
  const nck::SeBwdRef sr = nck::se_bwd_ref(in.shape(), in.dy.data(), xv, in.scale.data(), in.hidden.data(), in.w2t.data(),
                                           in.w1.data(), nullptr);
  v.field("dpool", nck::check_arr(sr.gsum, F(o.dpool)));
  const std::vector<float> da = se_da(in.dy.data(), in.scale.data(), F(o.dpool), 1.0f / (float)in.HW, in.B, in.HW, in.C);
  v.has_sink = true;
  const gck::SinkCheck k = gck::check_gradsink(da.data(), (long)in.B * in.HW, in.C, in.y.data(), in.bn.mu.data(),
                                               in.bn.rs.data(), in.bn.sc.data(), in.bn.be.data(), 1, F(o.part), o.Pexp, true);
  v.rows_written = k.rows_written && o.P == o.Pexp;
  v.sink1 = k.sum_ratio;
  v.sink2 = k.m2_ratio;
}

// the sums pass against fp64, and bit for bit against launch_se_bwd on the same inputs
static void run_sums(const char* name, int B, int HW, int C, int N, bool bf, uint64_t seed) {
  g_case = name;
  Verdict v;
  v.name = name;
  SeIn in;
  in.gen(B, HW, C, N, bf, seed);
  SeOut o, old;
  o.alloc(in, false);
  old.alloc(in, true);
  if (go(v, [&] {
        o.sums(in);
        old.apply(in);
      })) {
    check_sums(v, in, o);
    v.guards_ok = v.guards_ok && old.download();
    v.field("dpool_bits", bits_equal(F(o.dpool), F(old.dpool), (size_t)B * C * 4));
    v.field("partials_bits", bits_equal(F(o.part), F(old.part), (size_t)C * o.Pexp * 8));
    const std::vector<float> da = se_da(in.dy.data(), in.scale.data(), F(o.dpool), 1.0f / (float)HW, B, HW, C);
    v.field("da_bits", bits_equal(da.data(), F(old.da), da.size() * 4));
  }
  v.print();
}

// ---- k_dw_bwd with the SE source ---------------------------------------------------------------
struct DwIn {
  cck::Geo g;
  bool bf;
  std::vector<float> dy, y, s, q, w;  // q: the pool gradient (dpool), before the 1 / HW
  Dev dDy, dY, dS, dQ, dW;
  Bn bn;
  void gen(int B, int H, int W, int C, int k, int st, bool bf_, uint64_t seed) {
    g = cck::make_geo(B, H, W, C, k, st);
    bf = bf_;
    const size_t n = (size_t)g.out_px() * C;
    dy.resize(n); y.resize(n); s.resize((size_t)B * C); q.resize((size_t)B * C); w.resize((size_t)k * k * C);
    gck::fill_uni(dy, seed);
    gck::fill_uni(y, seed + 1, 1.5f, 0.2f);
    gck::fill_uni(s, seed + 2, 0.45f, 0.5f);  // s and q differ between the images
    gck::fill_uni(q, seed + 3, 20.0f);
    gck::fill_uni(w, seed + 4, 0.5f);
    bn.gen(C, seed + 10);
    put_f(dDy, dy);
    if (bf) put_bf(dY, y);
    else put_f(dY, y);
    put_f(dS, s); put_f(dQ, q); put_f(dW, w);
  }
  GradX gx(const float* da) const {
    return GradX{da, dY.f(), bn.dmu.f(), bn.drs.f(), bn.dsc.f(), bn.dbe.f(), bn.dm1.f(), bn.dm2.f(), 1, bf ? 1 : 0};
  }
};

// dx against the exact adjoint over view_grad(da), da the float the kernel stages: fmaf(dy, s, q) is one
// correctly rounded operation on both sides, so the host forms the same float and the existing bound holds
static nck::Field check_dw(const cck::Geo& g, const float* da, const float* y, const Bn& bn, const float* mdz,
                           const float* mdzx, const float* w, const float* dx) {
  const cck::GradRef gr{da, y, bn.mu.data(), bn.rs.data(), bn.sc.data(), bn.be.data(), mdz, mdzx, 1};
  const cck::Val gv = cck::view_grad(gr, g.out_px(), g.C);
  return nck::check_arr(cck::dw_bwd_ref(g, gv, w, nullptr), dx);
}
static void run_dw(const char* name, int B, int H, int W, int C, int k, int st, bool sink, bool bf, uint64_t seed) {
  g_case = name;
  Verdict v;
  v.name = name;
  DwIn in;
  in.gen(B, H, W, C, k, st, bf, seed);
  const cck::Geo& g = in.g;
  Guarded dx, part, tap;
  const float inv = 1.0f / (float)(g.Ho * g.Wo);
  outf(dx, (size_t)g.in_px() * C);
  outf(tap, (size_t)g.out_px() * C);
  // the GradSink of the expand BN whose output the depthwise conv reads
  Bn bn2;
  std::vector<float> y2;
  Dev dY2;
  GradSink gs{};
  int Pexp = 0, P = 0;
  if (sink) {
    bn2.gen(C, seed + 30);
    y2.resize((size_t)g.in_px() * C);
    gck::fill_uni(y2, seed + 31, 1.5f, 0.2f);
    put_f(dY2, y2);
    Pexp = dw_bwd_partials(B, H, W, C, g.Ho, g.Wo, k, st, g.pt, g.pl);
    outf(part, (size_t)C * Pexp * 2);
    gs = GradSink{reinterpret_cast<float2*>(part.ptr()), C, 0, dY2.f(), bn2.dmu.f(), bn2.drs.f(), bn2.dsc.f(), bn2.dbe.f(), 1, 0};
  }
  const bool ran = go(v, [&] {
    P = launch_dw_bwd_se(in.gx(in.dDy.f()), in.dS.f(), in.dQ.f(), inv, in.dW.f(), dx.ptr(), B, H, W, C, g.Ho, g.Wo, k, st,
                         g.pt, g.pl, false, g_st, gs);
    launch_se_da(in.dDy.f(), in.dS.f(), in.dQ.f(), tap.ptr(), B, g.Ho * g.Wo, C, g_st);
  });
  if (ran) {
    dx.download();
    tap.download();
    v.guards_ok = dx.intact() && tap.intact();
    const std::vector<float> da = se_da(in.dy.data(), in.s.data(), in.q.data(), inv, B, (long)g.Ho * g.Wo, C);
    v.field("dx", check_dw(g, da.data(), in.y.data(), in.bn, in.bn.m1.data(), in.bn.m2.data(), in.w.data(), F(dx)));
    // the tap's materialisation is the same fmaf: bit for bit
    v.field("tap", bits_equal(F(tap), da.data(), da.size() * 4));
    if (sink) {
      part.download();
      v.guards_ok = v.guards_ok && part.intact();
      v.has_sink = true;
      const gck::SinkCheck k2 = gck::check_gradsink(F(dx), g.in_px(), C, y2.data(), bn2.mu.data(), bn2.rs.data(),
                                                    bn2.sc.data(), bn2.be.data(), 1, F(part), Pexp, true);
      v.rows_written = k2.rows_written && P == Pexp;
      v.sink1 = k2.sum_ratio;
      v.sink2 = k2.m2_ratio;
    }
  }
  v.print();
}

// ---- chain equivalence: se_bwd_sums + bn_bwd_finalize + dw_bwd_se against se_bwd + bn_bwd_finalize + dw_bwd
static void run_chain(const char* name, int B, int H, int W, int C, int N, int k, uint64_t seed) {
  g_case = name;
  Verdict v;
  v.name = name;
  const int HW = H * W;
  SeIn in;
  in.gen(B, HW, C, N, false, seed);
  const cck::Geo g = cck::make_geo(B, H, W, C, k, 1);
  std::vector<float> w((size_t)k * k * C);
  gck::fill_uni(w, seed + 40, 0.5f);
  Dev dW;
  put_f(dW, w);
  SeOut o, old;
  o.alloc(in, false);
  old.alloc(in, true);
  Guarded dx_new, dx_old, m1n, m2n, m1o, m2o;
  const size_t n = (size_t)B * HW * C;
  outf(dx_new, n); outf(dx_old, n); outf(m1n, C); outf(m2n, C); outf(m1o, C); outf(m2o, C);
  auto gx = [&](const float* da, const float* m1, const float* m2) {
    return GradX{da, in.dY.f(), in.bn.dmu.f(), in.bn.drs.f(), in.bn.dsc.f(), in.bn.dbe.f(), m1, m2, 1, 0};
  };
  const bool ran = go(v, [&] {
    o.sums(in);
    launch_bn_bwd_finalize(reinterpret_cast<const float2*>(o.part.ptr()), o.P, (long)B * HW, C, m1n.ptr(), m2n.ptr(), g_st);
    launch_dw_bwd_se(gx(in.dDy.f(), m1n.ptr(), m2n.ptr()), in.dScale.f(), o.dpool.ptr(), 1.0f / (float)HW, dW.f(),
                     dx_new.ptr(), B, H, W, C, g.Ho, g.Wo, k, 1, g.pt, g.pl, false, g_st);
    old.apply(in);
    launch_bn_bwd_finalize(reinterpret_cast<const float2*>(old.part.ptr()), old.P, (long)B * HW, C, m1o.ptr(), m2o.ptr(), g_st);
    launch_dw_bwd(gx(old.da.ptr(), m1o.ptr(), m2o.ptr()), dW.f(), dx_old.ptr(), B, H, W, C, g.Ho, g.Wo, k, 1, g.pt, g.pl,
                  false, g_st);
  });
  if (ran) {
    check_sums(v, in, o);
    v.guards_ok = v.guards_ok && old.download();
    for (Guarded* p : {&dx_new, &dx_old, &m1n, &m2n, &m1o, &m2o}) {
      p->download();
      v.guards_ok = v.guards_ok && p->intact();
    }
    // both data gradients against fp64, each through the means its own chain stored ...
    const std::vector<float> da = se_da(in.dy.data(), in.scale.data(), F(o.dpool), 1.0f / (float)HW, B, HW, C);
    v.field("dx_new", check_dw(g, da.data(), in.y.data(), in.bn, F(m1n), F(m2n), w.data(), F(dx_new)));
    v.field("dx_old", check_dw(g, F(old.da), in.y.data(), in.bn, F(m1o), F(m2o), w.data(), F(dx_old)));
    // ... and the two chains bit for bit: the same operations on the same operands in the same order
    v.field("mdz_bits", bits_equal(F(m1n), F(m1o), (size_t)C * 4));
    v.field("mdzx_bits", bits_equal(F(m2n), F(m2o), (size_t)C * 4));
    v.field("dx_bits", bits_equal(F(dx_new), F(dx_old), n * 4));
  }
  v.print();
}

// ---- the refusal: without a GradSink the sums pass would produce nothing ---------------------------
static void run_refuse(const char* name, int B, int HW, int C, int N, uint64_t seed) {
  g_case = name;
  Verdict v;
  v.name = name;
  v.refuse = true;
  SeIn in;
  in.gen(B, HW, C, N, false, seed);
  SeOut o;
  o.alloc(in, false);
  go(v, [&] {
    launch_se_bwd_sums(in.dDy.f(), in.inx(), B, HW, C, N, in.dW1.f(), in.dW2t.f(), 1, in.dHidden.f(), in.dScale.f(),
                       o.dpool.ptr(), g_st, reinterpret_cast<double*>(o.scratch.ptr()), GradSink{});
  });
  v.untouched_ok = untouched(o.scratch) && untouched(o.dpool) && untouched(o.part);
  v.print();
}

int main() {
  CK(hipStreamCreate(&g_st));
  printf("{\"knobs_unset\":%s,\"red_depth\":%d}\n",
         (!getenv("PHX_RED_BLOCKS") && !getenv("PHX_RED_DEPTH") && !getenv("PHX_RED_MINROWS")) ? "true" : "false",
         red_plan_info(64, 8, 2).depth);
  // ---- the table (tests/test_gpu_sefold_kernels.py reads the names from here) ----
  // pool sums + MLP backward + the BN-backward sums without the store; every input distinct per image
  run_sums("sums_b2_hw49_c8", 2, 49, 8, 4, false, 101);           // one ragged chunk, two lanes per row
  run_sums("sums_b3_hw256_c1152", 3, 256, 1152, 48, false, 102);  // two channel groups, the second 32 lanes wide
  run_sums("sums_b2_hw1024_c40", 2, 1024, 40, 10, false, 103);    // tpr 10: 6 idle lanes, three chunks
  run_sums("sums_b2_hw49_c8_bf16", 2, 49, 8, 4, true, 104);       // y in bf16 storage
  run_sums("sums_b2_hw1024_c40_bf16", 2, 1024, 40, 10, true, 105);
  // k_dw_bwd with the SE source; s and dpool differ between the images
  run_dw("dw_k3s1_16x16_c8", 2, 16, 16, 8, 3, 1, false, false, 201);
  run_dw("dw_k5s2_15x15_c12", 2, 15, 15, 12, 5, 2, false, false, 202);  // odd size, padding, column parity
  run_dw("dw_k5s1_9x9_c16_sink", 2, 9, 9, 16, 5, 1, true, false, 203);  // the expand BN's GradSink on
  run_dw("dw_k3s2_16x16_c32_sink", 2, 16, 16, 32, 3, 2, true, false, 204);
  run_dw("dw_k3s1_16x16_c8_bf16", 2, 16, 16, 8, 3, 1, false, true, 205);
  // the new sequence against launch_se_bwd + launch_bn_bwd_finalize + launch_dw_bwd
  run_chain("chain_k3_8x8_c16", 2, 8, 8, 16, 4, 3, 301);
  run_chain("chain_k5_16x16_c40", 3, 16, 16, 40, 10, 5, 302);
  // no GradSink: throws before any launch
  run_refuse("refuse_no_sink", 2, 4, 8, 4, 401);
  // ---- end of the table
  CK(hipStreamSynchronize(g_st));
  printf("{\"done\":true}\n");
  return 0;
}
