// batch_invariance — does an image's result depend on the batch it shares a launch with?  The launchers
// of the inference forward whose result involves a sum are run as a batch-invariant forward runs them
// (gemm_plan_images() = B, kernels.hpp) on B images, and on each image alone; image p's slice of every
// output must be the same bytes.  No reference is needed: both sides are the device's.
//   batch_invariance --plan            the order-relevant plan of every case and batch size, under
//                                      gemm_plan_images() = B ("img") and = 0 ("launch").  Host code only:
//                                      no HIP call (tests/test_batch_invariance_host.py holds the table
//                                      to its classes with it)
//   batch_invariance                   run the table on the GPU: a flushed JSON line per case, then `done`
//   batch_invariance --shape Mi N K B...   the GEMM plans of one shape (for choosing table entries)
//   batch_invariance --fused H C B...      launch_dw_fwd_fused's plan of one H x H x C shape
// Per case: Bmax images of seeded inputs and one set of weights; for every B of the case's list the first
// B images in one launch; the largest B once more in reversed image order; every image alone at B = 1.
// Verdict: diff_words (32-bit words that differ between a batch run and the single runs, over all
// outputs: must be 0), first_diff (output:B:image:index), canary_ok (guard regions, the rows past the
// launch's images and nothing else untouched), inputs_ok (inputs as uploaded afterwards), repeat_ok (the
// largest batch run twice gives the same bytes).  A HIP error ends the process at once with a `fatal`
// line and status 3.  Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "parity_dev.hpp"

using namespace phx;

enum Op { SE, GEMM, GROUP, SEP, DW, DWF };
static const char* op_name(Op o) {
  switch (o) {
    case SE: return "se";
    case GEMM: return "gemm";
    case GROUP: return "group";
    case SEP: return "sep";
    case DW: return "dw";
    default: return "dwf";
  }
}

struct Case {
  std::string name;
  Op op;
  std::vector<int> Bs;
  // SE: C, Cse, HW, view (0 raw, 1 BN + swish)        GEMM: mode (1 BN view, 2 + SE row scale), Mi, N, K
  // GROUP: N, K and the members' rows Ms               SEP: N and the members' sides Ms (C = 64)
  // DW: H (= W), C, k, stride                          DWF: H (= W), C, inputs of the fuse
  int a = 0, b = 0, c = 0, d = 0;
  std::vector<int> Ms;
};

// ---- the table ---------------------------------------------------------------------------------
// A case's device memory is its verdict's `bytes` (inputs in both image orders, weights, outputs, scratch): under
// 7 MB for every case but four, whose classes begin at a size: gemm_deepk_flip (256 output tiles of 128 x 128
// floats for the launch alone to run unsplit: 17 MB of C, 35 MB in all), gemm_res (512 tiles of 64 x 128 for runs
// of 2 N tiles, twice that for runs of 3: 35 MB of C, 41 MB in all) and the two fused depthwise cases past the
// switch (512 workgroups of 33 x 4 pixels x 16 channels: 4.5 MB a tensor, 31 and 22 MB in all).
static std::vector<Case> table() {
  std::vector<Case> t;
  auto bc = [&](const char* name, Op op, std::vector<int> Bs, int a, int b, int c, int d, std::vector<int> Ms = {}) {
    t.push_back(Case{name, op, std::move(Bs), a, b, c, d, std::move(Ms)});
  };
  // a. launch_se_fwd at the backbones' (C, Cse) pairs and the batch sizes at which se_plan(B, ...) moves
  // (D0: 8 and 16; D4: 4 and 8), at HW = 17 (the pool's chunks: 2 as planned for 16 images, 3 for a
  // launch of one) and HW = 1; raw and BN-view input
  bc("se_d0_c1152_n48_hw17_view", SE, {1, 4, 8, 16}, 1152, 48, 17, 1);
  bc("se_d0_c1152_n48_hw1_raw", SE, {1, 4, 8, 16}, 1152, 48, 1, 0);
  bc("se_d0_c672_n28_hw17_raw", SE, {1, 4, 8, 16}, 672, 28, 17, 0);
  bc("se_d0_c672_n28_hw1_view", SE, {1, 4, 8, 16}, 672, 28, 1, 1);
  bc("se_d4_c2688_n112_hw17_view", SE, {1, 3, 4, 8}, 2688, 112, 17, 1);
  bc("se_d4_c2688_n112_hw1_raw", SE, {1, 3, 4, 8}, 2688, 112, 1, 0);
  bc("se_d2_c2112_n88_hw17_raw", SE, {1, 3, 4, 8}, 2112, 88, 17, 0);
  // b. launch_gemm forward, one case per order class; Mi is no multiple of the tile rows, so an image's
  // rows sit elsewhere in a tile at every position of the batch.
  // deep K over few tiles (k_gemm2k as planned for one image: 2 x 10 tiles); at B = 17 the launch alone has
  // 27 x 10 >= 256 tiles and would run k_gemm2 unsplit.  D0's head conv (320 -> 1280)
  bc("gemm_deepk_flip_m196_n1280_k320_se", GEMM, {1, 4, 17}, 2, 196, 1280, 320);
  bc("gemm_deepk_m9_n64_k320_view", GEMM, {1, 4, 16}, 1, 9, 64, 320);
  // K < 256 over few tiles: k_gemm2k for the launch alone, k_gemm2 in a batch-invariant forward
  bc("gemm_fewtile_m9_n64_k64_view", GEMM, {1, 4, 16}, 1, 9, 64, 64);
  bc("gemm_fewtile_m49_n240_k40_se", GEMM, {1, 4, 16}, 2, 49, 240, 40);
  // K < 256 over many tiles: k_gemm2 either way, the tile follows the launch
  bc("gemm_manytile_m1369_n144_k24_view", GEMM, {1, 2, 4}, 1, 1369, 144, 24);
  // A-resident sweeps (k_gemm2r: two K chunks, 7 N tiles): k_gemm2 on 32 x 128 tiles for one image, runs of
  // 2 N tiles at B = 3 (86 M tiles) and of 3 at B = 6 (172).  D0's class-predict conv (64 -> 810)
  bc("gemm_res_m1825_n810_k64_se", GEMM, {1, 3, 6}, 2, 1825, 810, 64);
  // c. gemm_group_run: three head levels sharing weights
  bc("group_m64_16_4_n64_k64", GROUP, {1, 4, 16}, 64, 64, 0, 0, {64, 16, 4});
  // d. launch_sep_fwd, single and grouped members (K and tap orders are fixed: this pins it)
  bc("sep_single_5x5_n64", SEP, {1, 4, 16}, 64, 0, 0, 0, {5});
  bc("sep_single_20x20_n36", SEP, {1, 3, 4}, 36, 0, 0, 0, {20});
  bc("sep_group_16_8_4_2_1_n64", SEP, {1, 4, 16}, 64, 0, 0, 0, {16, 8, 4, 2, 1});
  // e. launch_dw_fwd (B-free tile plan) and launch_dw_fwd_fused on both sides of its few-workgroups switch
  bc("dw_k5_s1_7x7_c96", DW, {1, 4, 16}, 7, 96, 5, 1);
  bc("dw_k3_s2_9x9_c32", DW, {1, 4, 16}, 9, 32, 3, 2);
  // (the one-row, one-quad plan below 512 workgroups: B = 16 and B = 4 are past it)
  bc("dwf_33x33_c64_n3", DWF, {1, 4, 16}, 33, 64, 3, 0);
  bc("dwf_33x33_c256_n2", DWF, {1, 2, 4}, 33, 256, 2, 0);
  bc("dwf_8x8_c64_n2", DWF, {1, 4, 16}, 8, 64, 2, 0);
  return t;
}
// ---- end of the table

// ---- plans (host only) --------------------------------------------------------------------------
static std::string kv(const char* k, long v, bool last = false) {
  char b[64];
  snprintf(b, sizeof b, "\"%s\":%ld%s", k, v, last ? "" : ",");
  return b;
}
static std::string gemm_plan_json(int M, int N, int K, bool allow_wsk) {
  const Gemm2Plan p = plan_gemm2(M, N, K, gemm2_target_wgs(), false, true, allow_wsk);
  return "{" + kv("M", M) + kv("wsk", p.wsk > 0) + kv("splits", p.splits) + kv("res", p.res_lds > 0) +
         kv("nper", p.res_lds ? p.kslice : 0) + kv("wm", p.wm) + kv("tm", p.tm) + kv("tn", p.tn) +
         kv("mtiles", p.mtiles) + kv("gy", p.gy) + kv("impl", gemm_impl_for(N), true) + "}";
}
static void dw_same(int H, int k, int s, int* Ho, int* pt) {
  *Ho = (H + s - 1) / s;
  const int total = std::max((*Ho - 1) * s + k - H, 0);
  *pt = total / 2;
}
// the plan of a case's launch of B images, under the gemm_plan_images() in force
static std::string plan_of(const Case& c, int B) {
  switch (c.op) {
    case SE: {
      const RedPlanInfo r = red_plan_info(c.c, c.a, B);
      const SePlanInfo s = se_plan_info(B, c.a, c.b, r.chunks);
      return "{" + kv("B", B) + kv("s1", s.s1) + kv("cs1", s.cs1) + kv("s2", s.s2) + kv("cs2", s.cs2) + kv("kg", s.kg) +
             kv("jg", s.jg) + kv("rpc", r.rpc) + kv("chunks", r.chunks, true) + "}";
    }
    case GEMM: return "{" + kv("B", B) + "\"g\":" + gemm_plan_json(B * c.b, c.c, c.d, true) + "}";
    case GROUP: {
      std::string s = "{" + kv("B", B) + "\"members\":[";
      for (size_t i = 0; i < c.Ms.size(); ++i) s += (i ? "," : "") + gemm_plan_json(B * c.Ms[i], c.a, c.b, false);
      return s + "]}";
    }
    case SEP: {
      std::string s = "{" + kv("B", B) + "\"ntiles\":[";
      for (size_t i = 0; i < c.Ms.size(); ++i) s += (i ? "," : "") + std::to_string(sep_tile_info(c.Ms[i], c.Ms[i]).ntiles);
      return s + "]}";
    }
    case DW: {
      int Ho, pt;
      dw_same(c.a, c.c, c.d, &Ho, &pt);
      const DwTileInfo t = dw_tile_info(c.a, c.a, c.b, Ho, Ho, pt, pt, c.c, c.d, false);
      return "{" + kv("B", B) + kv("ntiles", t.ntiles) + kv("ncg", t.ncg) + kv("otw", t.otw) + kv("oth", t.oth, true) + "}";
    }
    default: {
      const DwTileInfo t = dw_fused_tile_info(B, c.a, c.a, c.b, c.a, c.a, 1, 1);
      return "{" + kv("B", B) + kv("small", t.small) + kv("wgs", t.wgs) + kv("ntiles", t.ntiles) + kv("ncg", t.ncg, true) + "}";
    }
  }
}
struct PlanImages {  // as run_forward sets it for a batch-invariant forward
  explicit PlanImages(int v) { gemm_plan_images() = v; }
  ~PlanImages() { gemm_plan_images() = 0; }
};
static std::string plans_json(const Case& c) {
  std::string img, launch;
  for (size_t i = 0; i < c.Bs.size(); ++i) {
    {
      PlanImages pi(c.Bs[i]);
      img += (i ? "," : "") + plan_of(c, c.Bs[i]);
    }
    launch += (i ? "," : "") + plan_of(c, c.Bs[i]);
  }
  return "{\"img\":[" + img + "],\"launch\":[" + launch + "]}";
}
static std::string head_json(const Case& c) {
  std::string s = "{\"case\":\"" + c.name + "\",\"op\":\"" + op_name(c.op) + "\",\"Bs\":[";
  for (size_t i = 0; i < c.Bs.size(); ++i) s += (i ? "," : "") + std::to_string(c.Bs[i]);
  return s + "]," + kv("a", c.a) + kv("b", c.b) + kv("c", c.c) + kv("d", c.d) + "\"plans\":" + plans_json(c);
}

// ---- a case on the device -------------------------------------------------------------------------
// in: per-image inputs ([Bmax][per floats], one device copy in order and one reversed); wt: what every
// image shares; out: per-image outputs.  run(B, in, wt, out, scratch) launches B images on the stream.
struct Job {
  std::vector<size_t> in_per, out_per;
  std::vector<std::string> out_name;
  std::vector<std::vector<float>> in, wt;
  size_t scratch_bytes = 16;
  std::function<void(int, const std::vector<const float*>&, const std::vector<const float*>&, const std::vector<float*>&,
                     float*, hipStream_t)>
      run;
};

static std::vector<float> uni(size_t n, uint64_t seed, float scale = 1.f, float shift = 0.f) {
  std::vector<float> v(n);
  gck::fill_uni(v, seed, scale, shift);
  return v;
}
// BN view parameters of C channels into wt (mu, sc, be): returns the index of mu
static size_t add_bn(Job& j, int C, uint64_t seed) {
  j.wt.push_back(uni(C, seed, 0.3f));
  j.wt.push_back(uni(C, seed + 1, 0.4f, 1.0f));
  j.wt.push_back(uni(C, seed + 2, 0.3f));
  return j.wt.size() - 3;
}
static InX bn_inx(const float* p, const std::vector<const float*>& w, size_t at, int act = 1) {
  return InX{p, w[at], w[at + 1], w[at + 2], act};
}

static Job make_job(const Case& c, uint64_t seed) {
  Job j;
  const int Bmax = c.Bs.back();
  auto in = [&](size_t per, uint64_t s, float scale = 1.f, float shift = 0.f) {
    j.in_per.push_back(per);
    j.in.push_back(uni(per * Bmax, seed + s, scale, shift));
  };
  auto out = [&](const char* name, size_t per) {
    j.out_name.push_back(name);
    j.out_per.push_back(per);
  };
  switch (c.op) {
    case SE: {
      const int C = c.a, N = c.b, HW = c.c, view = c.d;
      in((size_t)HW * C, 1);
      j.wt.push_back(uni((size_t)C * N, seed + 2, 2.0f / std::sqrt((float)C)));
      j.wt.push_back(uni(N, seed + 3, 0.5f));
      j.wt.push_back(uni((size_t)N * C, seed + 4, 2.0f / std::sqrt((float)N)));
      j.wt.push_back(uni(C, seed + 5, 0.5f));
      const size_t bn = add_bn(j, C, seed + 10);
      out("pool", C); out("hidden", N); out("scale", C);
      j.scratch_bytes = colred_scratch_doubles(HW, C, Bmax) * 8;
      j.run = [=](int B, const std::vector<const float*>& x, const std::vector<const float*>& w, const std::vector<float*>& o,
                  float* scratch, hipStream_t st) {
        const InX xin = view ? bn_inx(x[0], w, bn) : InX{x[0], nullptr, nullptr, nullptr, 0};
        launch_se_fwd(xin, nullptr, B, HW, C, N, w[0], w[1], w[2], w[3], 1, o[0], o[1], o[2], st,
                      reinterpret_cast<double*>(scratch));
      };
      break;
    }
    case GEMM: {
      const int mode = c.a, Mi = c.b, N = c.c, K = c.d;
      in((size_t)Mi * K, 1);
      in((size_t)K, 2, 0.45f, 0.5f);  // the SE excitation of each image (mode 2)
      j.wt.push_back(uni((size_t)N * K, seed + 3, 1.0f / std::sqrt((float)K)));
      j.wt.push_back(uni(N, seed + 4, 0.5f));
      const size_t bn = add_bn(j, K, seed + 10);
      out("C", (size_t)Mi * N);
      size_t pf = 0;
      for (int B : c.Bs) {
        pf = std::max(pf, gemm_partial_floats(B * Mi, N, K));
        PlanImages pi(B);
        pf = std::max(pf, gemm_partial_floats(B * Mi, N, K));
      }
      j.scratch_bytes = std::max<size_t>(16, pf * 4);
      j.run = [=](int B, const std::vector<const float*>& x, const std::vector<const float*>& w, const std::vector<float*>& o,
                  float* scratch, hipStream_t st) {
        launch_gemm(bn_inx(x[0], w, bn), w[0], w[1], o[0], B * Mi, N, K, false, mode == 2 ? x[1] : nullptr, Mi, st,
                    scratch);
      };
      break;
    }
    case GROUP: {
      const int N = c.a, K = c.b;
      const std::vector<int> Ms = c.Ms;
      for (size_t i = 0; i < Ms.size(); ++i) in((size_t)Ms[i] * K, 1 + i);
      j.wt.push_back(uni((size_t)N * K, seed + 7, 1.0f / std::sqrt((float)K)));
      j.wt.push_back(uni(N, seed + 8, 0.5f));
      const size_t bn = add_bn(j, K, seed + 10);
      for (size_t i = 0; i < Ms.size(); ++i) out(i == 0 ? "C0" : i == 1 ? "C1" : "C2", (size_t)Ms[i] * N);
      j.run = [=](int B, const std::vector<const float*>& x, const std::vector<const float*>& w, const std::vector<float*>& o,
                  float*, hipStream_t st) {
        std::vector<GemmSeg> segs(Ms.size());
        for (size_t i = 0; i < Ms.size(); ++i)
          segs[i] = GemmSeg{bn_inx(x[i], w, bn), GradX{}, w[1], o[i], B * Ms[i], false, StatSink{}, GradSink{}};
        gemm_group_run(1, segs.data(), (int)segs.size(), w[0], N, K, st);
      };
      break;
    }
    case SEP: {
      const int N = c.a, C = 64;
      const std::vector<int> Hs = c.Ms;
      static const char* names[kMaxSeg] = {"y0", "y1", "y2", "y3", "y4"};
      for (size_t i = 0; i < Hs.size(); ++i) in((size_t)Hs[i] * Hs[i] * C, 1 + i);
      j.wt.push_back(uni(9 * C, seed + 7, 0.4f));
      j.wt.push_back(uni((size_t)N * C, seed + 8, 1.0f / std::sqrt((float)C)));
      j.wt.push_back(uni(N, seed + 9, 0.5f));
      const size_t bn = add_bn(j, C, seed + 10);
      for (size_t i = 0; i < Hs.size(); ++i) out(names[i], (size_t)Hs[i] * Hs[i] * N);
      j.run = [=](int B, const std::vector<const float*>& x, const std::vector<const float*>& w, const std::vector<float*>& o,
                  float*, hipStream_t st) {
        std::vector<SepMember> mem(Hs.size());
        for (size_t i = 0; i < Hs.size(); ++i)
          mem[i] = SepMember{bn_inx(x[i], w, bn), FuseView{}, false, o[i], Hs[i], Hs[i], StatSink{}};
        int nps[kMaxSeg];
        launch_sep_fwd(mem.data(), (int)mem.size(), B, C, N, w[0], w[1], w[2], st, nps);
      };
      break;
    }
    case DW: {
      const int H = c.a, C = c.b, k = c.c, s = c.d;
      int Ho, pt;
      dw_same(H, k, s, &Ho, &pt);
      in((size_t)H * H * C, 1);
      j.wt.push_back(uni((size_t)k * k * C, seed + 2, 0.4f));
      const size_t bn = add_bn(j, C, seed + 10);
      out("y", (size_t)Ho * Ho * C);
      j.run = [=](int B, const std::vector<const float*>& x, const std::vector<const float*>& w, const std::vector<float*>& o,
                  float*, hipStream_t st) {
        launch_dw_fwd(bn_inx(x[0], w, bn), w[0], o[0], B, H, H, C, Ho, Ho, k, s, pt, pt, st);
      };
      break;
    }
    case DWF: {
      const int H = c.a, C = c.b, nin = c.c;
      for (int i = 0; i < nin; ++i) in((size_t)H * H * C, 1 + i);
      j.wt.push_back(uni(9 * C, seed + 5, 0.4f));
      j.wt.push_back(uni(4, seed + 6, 0.4f, 0.8f));  // the fuse weights (positive)
      const size_t bn = add_bn(j, C, seed + 10);
      out("y", (size_t)H * H * C);
      j.run = [=](int B, const std::vector<const float*>& x, const std::vector<const float*>& w, const std::vector<float*>& o,
                  float*, hipStream_t st) {
        FuseView f{};
        for (int i = 0; i < 3; ++i) {
          // (an unused slot holds a valid view); the first two inputs through a BN view without activation
          f.x[i] = i < 2 ? bn_inx(x[i], w, bn, 0) : InX{x[i < nin ? i : 0], nullptr, nullptr, nullptr, 0};
          f.w[i] = w[1] + i;
        }
        f.nin = nin;
        f.method = 0;
        f.act = 1;
        launch_dw_fwd_fused(f, w[0], o[0], B, H, H, C, H, H, 3, 1, 1, 1, st);
      };
      break;
    }
  }
  return j;
}

static bool bytes_same(const Dev& d, const std::vector<float>& h) {
  std::vector<float> g(h.size());
  CK(hipMemcpy(g.data(), d.d, h.size() * 4, hipMemcpyDeviceToHost));
  return std::memcmp(g.data(), h.data(), h.size() * 4) == 0;
}

static std::string run_case(const Case& c, uint64_t seed, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const Job j = make_job(c, seed);
  const int Bmax = c.Bs.back();
  const size_t ni = j.in.size(), no = j.out_per.size();
  // inputs in order and in reversed image order
  std::vector<std::unique_ptr<Dev>> din(ni), drev(ni), dwt(j.wt.size());
  std::vector<std::vector<float>> rev(ni);
  double bytes = (double)j.scratch_bytes;
  for (size_t i = 0; i < ni; ++i) {
    const size_t per = j.in_per[i];
    rev[i].resize(j.in[i].size());
    for (int b = 0; b < Bmax; ++b)
      std::memcpy(&rev[i][b * per], &j.in[i][(size_t)(Bmax - 1 - b) * per], per * 4);
    din[i].reset(new Dev);
    drev[i].reset(new Dev);
    put_f(*din[i], j.in[i]);
    put_f(*drev[i], rev[i]);
    bytes += 2.0 * j.in[i].size() * 4;
  }
  std::vector<const float*> w(j.wt.size());
  for (size_t i = 0; i < j.wt.size(); ++i) {
    dwt[i].reset(new Dev);
    put_f(*dwt[i], j.wt[i]);
    w[i] = dwt[i]->f();
    bytes += j.wt[i].size() * 4.0;
  }
  std::vector<std::unique_ptr<Guarded>> dout(no);
  std::vector<float*> o(no);
  for (size_t k = 0; k < no; ++k) {
    dout[k].reset(new Guarded);
    dout[k]->alloc(j.out_per[k] * Bmax * 4);
    dout[k]->fill32(gck::kUnwritten);
    o[k] = dout[k]->ptr();
    bytes += j.out_per[k] * Bmax * 4.0;
  }
  Guarded scratch;
  scratch.alloc(j.scratch_bytes);

  bool canary_ok = true, threw = false;
  std::string what;
  int runs = 0;
  // one launch of B images reading `x`; leaves the downloaded outputs in dout[k]->out()
  auto launch = [&](int B, const std::vector<const float*>& x) {
    for (auto& g : dout) g->upload();
    scratch.upload();
    {
      PlanImages pi(B);
      j.run(B, x, w, o, scratch.ptr(), st);
    }
    CK(hipStreamSynchronize(st));
    ++runs;
    for (size_t k = 0; k < no; ++k) {
      dout[k]->download();
      if (!dout[k]->intact()) canary_ok = false;
      // the rows of the images this launch does not have
      const uint32_t* q = reinterpret_cast<const uint32_t*>(dout[k]->out());
      for (size_t e = j.out_per[k] * B; e < j.out_per[k] * Bmax; ++e)
        if (q[e] != gck::kUnwritten) canary_ok = false;
    }
    scratch.download();
    if (!scratch.intact()) canary_ok = false;
  };
  long diff = 0;
  std::string first;
  bool repeat_ok = true;
  try {
    // every image alone
    std::vector<std::vector<std::vector<uint8_t>>> single(no, std::vector<std::vector<uint8_t>>(Bmax));
    for (int p = 0; p < Bmax; ++p) {
      std::vector<const float*> x(ni);
      for (size_t i = 0; i < ni; ++i) x[i] = din[i]->f() + j.in_per[i] * p;
      launch(1, x);
      for (size_t k = 0; k < no; ++k) single[k][p].assign(dout[k]->out(), dout[k]->out() + j.out_per[k] * 4);
    }
    auto compare = [&](int B, bool reversed, const char* tag) {
      for (size_t k = 0; k < no; ++k) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(dout[k]->out());
        for (int b = 0; b < B; ++b) {
          const int img = reversed ? Bmax - 1 - b : b;
          const uint32_t* r = reinterpret_cast<const uint32_t*>(single[k][img].data());
          for (size_t e = 0; e < j.out_per[k]; ++e) {
            if (q[j.out_per[k] * b + e] == r[e]) continue;
            if (!diff++) first = j.out_name[k] + ":" + tag + std::to_string(B) + ":" + std::to_string(img) + ":" + std::to_string(e);
          }
        }
      }
    };
    std::vector<const float*> x(ni), xr(ni);
    for (size_t i = 0; i < ni; ++i) x[i] = din[i]->f(), xr[i] = drev[i]->f();
    std::vector<std::vector<uint8_t>> last(no);
    for (int B : c.Bs) {
      launch(B, x);
      compare(B, false, "B");
      if (B == Bmax)
        for (size_t k = 0; k < no; ++k) last[k].assign(dout[k]->out(), dout[k]->out() + dout[k]->n);
    }
    launch(Bmax, x);
    for (size_t k = 0; k < no; ++k) repeat_ok = repeat_ok && std::memcmp(last[k].data(), dout[k]->out(), dout[k]->n) == 0;
    if (Bmax > 1) {
      launch(Bmax, xr);
      compare(Bmax, true, "R");
    }
  } catch (const std::exception& e) {
    threw = true;
    what = e.what();
    (void)hipStreamSynchronize(st);
  }
  bool inputs_ok = true;
  for (size_t i = 0; i < ni; ++i) inputs_ok = inputs_ok && bytes_same(*din[i], j.in[i]) && bytes_same(*drev[i], rev[i]);
  for (size_t i = 0; i < j.wt.size(); ++i) inputs_ok = inputs_ok && bytes_same(*dwt[i], j.wt[i]);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const bool pass = !threw && diff == 0 && canary_ok && inputs_ok && repeat_ok;
  return head_json(c) + "," + kv("diff_words", diff) + "\"first_diff\":\"" + first + "\"," + kv("canary_ok", canary_ok) +
         kv("inputs_ok", inputs_ok) + kv("repeat_ok", repeat_ok) + kv("threw", threw) + "\"what\":\"" + esc(what) + "\"," +
         kv("runs", runs) + "\"bytes\":" + num(bytes) + ",\"ms\":" + num(ms) + "," + kv("pass", pass, true) + "}";
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  const std::vector<Case> t = table();
  if (argc == 2 && std::string(argv[1]) == "--plan") {
    for (const Case& c : t) printf("%s}\n", head_json(c).c_str());
    printf("{\"done\":true,\"cases\":%zu}\n", t.size());
    return 0;
  }
  if (argc > 5 && std::string(argv[1]) == "--shape") {
    Case c{"shape", GEMM, {}, 1, atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
    for (int i = 5; i < argc; ++i) c.Bs.push_back(atoi(argv[i]));
    printf("%s}\n", head_json(c).c_str());
    return 0;
  }
  if (argc > 4 && std::string(argv[1]) == "--fused") {
    Case c{"fused", DWF, {}, atoi(argv[2]), atoi(argv[3]), 2, 0};
    for (int i = 4; i < argc; ++i) c.Bs.push_back(atoi(argv[i]));
    printf("%s}\n", head_json(c).c_str());
    return 0;
  }
  if (argc > 1) {
    fprintf(stderr, "usage: batch_invariance [--plan | --shape Mi N K B... | --fused H C B...]\n");
    return 2;
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t st;
  CK(hipStreamCreate(&st));
  uint64_t seed = 9000;
  for (const Case& c : t) {
    g_case = c.name.c_str();
    printf("%s\n", run_case(c, seed, st).c_str());
    fflush(stdout);
    seed += 100;
  }
  CK(hipStreamDestroy(st));
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("{\"done\":true,\"cases\":%zu,\"seconds\":%s}\n", t.size(), num(sec).c_str());
  return 0;
}
