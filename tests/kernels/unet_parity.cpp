// unet_parity — kernel-level parity of kernels_unet.hip below k_wgrad_fold against the fp64 references of
// unet_check.hpp: the fp64 column reductions with their three finals (BN statistics, BN backward, column sums),
// k_un_bnact / k_un_bnb_apply, pool + Dropout and its backward, the attention gate, the output layer with its loss,
// k_un_small_dgrad, k_un_add, and the Masker's permutation, crops and box filter.
//
//   unet_parity --plan   the case table with each case's geometry (the column reductions' row blocks from the
//                        library's own un_colred_plan_info, held equal to the harness's copy), the share of elements
//                        under a kink allowance by the reference alone, the golden draws against the restated
//                        Philox, and the CPU stand-in's verdict (no GPU is touched)
//   unet_parity          run the table on the GPU: a head line with the measured expf / tanhf figures, one flushed
//                        JSON line per case, then a `done` line
//
// Only the launchers of unet.hpp are called, on one stream.  Every output (and the fp64 scratch, allocated at
// exactly un_colred_doubles / un_loss_blocks) sits between guard regions and starts NaN-filled or at a known old
// value; every launch runs twice over fresh fills and must repeat bit for bit; inputs are read back.  The exit
// status is 0 when every case ran (the verdicts are in the lines); a HIP error ends the process at once with a
// `fatal` line and status 3.  Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "unet.hpp"
#include "unet_check.hpp"
#include "parity_dev.hpp"

using namespace uck;
using namespace phx;

// ---- the case table ----------------------------------------------------------------------------
static std::vector<Case> table() {
  std::vector<Case> t;
  auto add = [&](const std::string& name, int op, const std::function<void(Case&)>& more) {
    Case c;
    c.name = name; c.op = op; c.seed = 500 + (uint32_t)t.size();
    more(c);
    t.push_back(c);
  };
  auto nm = [](const char* fmt, long a, long b = 0, long c = 0, long d = 0, long e = 0) {
    char buf[96];
    snprintf(buf, sizeof buf, fmt, a, b, c, d, e);
    return std::string(buf);
  };
  const int Cs[9] = {1, 3, 8, 24, 64, 100, 128, 129, 256};
  // a. BN statistics: every C around the 8-deep body (8 * (256 / C) - 1, the same, + 1), moving statistics on the
  // odd M; one row, fewer rows than lane groups; the block counts 1, 2, 64, 65, 193, 257 and the capped 1024 whose
  // last blocks start past M; an empty last block below the cap; C = 1 and C = 3 with many blocks; a constant C = 1
  for (int C : Cs)
    for (int d = -1; d <= 1; ++d) {
      const long M = 8 * (256 / C) + d;
      add(nm("st_c%ld_m%ld", C, M), STATS, [&](Case& c) { c.C = C; c.M = M; c.flav = M & 1; c.data = 1; });
    }
  add("st_c1_m1", STATS, [](Case& c) { c.C = 1; c.M = 1; });
  add("st_c3_m1_moving", STATS, [](Case& c) { c.C = 3; c.M = 1; c.flav = 1; });
  add("st_c256_m1", STATS, [](Case& c) { c.C = 256; c.M = 1; c.data = 1; });
  add("st_c8_m5", STATS, [](Case& c) { c.C = 8; c.M = 5; c.data = 1; });
  add("st_c24_m3_moving", STATS, [](Case& c) { c.C = 24; c.M = 3; c.flav = 1; c.data = 1; });
  add("st_c1_m100", STATS, [](Case& c) { c.C = 1; c.M = 100; c.data = 1; });
  add("st_c1_m2048_const", STATS, [](Case& c) { c.C = 1; c.M = 2048; c.data = 2; c.flav = 1; });
  add("st_c256_m33_blk2", STATS, [](Case& c) { c.C = 256; c.M = 33; c.data = 1; });
  add("st_c256_m2048_blk64", STATS, [](Case& c) { c.C = 256; c.M = 2048; c.data = 1; c.flav = 1; });
  add("st_c256_m2049_blk65", STATS, [](Case& c) { c.C = 256; c.M = 2049; c.data = 1; });
  add("st_c256_m6145_blk193", STATS, [](Case& c) { c.C = 256; c.M = 6145; c.data = 1; c.flav = 1; });
  add("st_c256_m8193_blk257", STATS, [](Case& c) { c.C = 256; c.M = 8193; c.data = 1; });
  add("st_c256_m32769_blk1024_capped", STATS, [](Case& c) { c.C = 256; c.M = 32769; c.data = 1; c.flav = 1; });
  add("st_c1_m8193_blk2", STATS, [](Case& c) { c.C = 1; c.M = 8193; c.data = 1; });
  add("st_c1_m532475_blk65", STATS, [](Case& c) { c.C = 1; c.M = 532475; c.data = 1; c.flav = 1; });
  add("st_c3_m175000_blk65", STATS, [](Case& c) { c.C = 3; c.M = 175000; c.data = 1; });
  add("st_c3_m526000_blk193", STATS, [](Case& c) { c.C = 3; c.M = 526000; c.data = 1; c.flav = 1; });
  add("st_c24_m700_blk3", STATS, [](Case& c) { c.C = 24; c.M = 700; c.data = 1; });
  // the last block empty below the cap: ceil(M / nb) * (nb - 1) reaches M (65 blocks of 64 rows hold 4096 in 64)
  add("st_c129_m4096_blk65_empty_last", STATS, [](Case& c) { c.C = 129; c.M = 4096; c.data = 1; c.flav = 1; });
  add("st_c100_m1000_blk13", STATS, [](Case& c) { c.C = 100; c.M = 1000; c.data = 1; c.flav = 1; });
  // b. BN backward (reduction, final, apply): leaky and identity; the apply's n = 1, 255, 256, 257 and a second
  // grid-stride pass (8193 x 256 elements)
  for (int i = 0; i < 9; ++i) {
    const int C = Cs[i];
    const long M = 8 * (256 / C) + 1;
    add(nm("bw_c%ld_m%ld_act%ld", C, M, i & 1), BNBWD, [&](Case& c) { c.C = C; c.M = M; c.act = i & 1; c.data = 1; });
  }
  add("bw_c1_m1_n1", BNBWD, [](Case& c) { c.C = 1; c.M = 1; });
  add("bw_c3_m1", BNBWD, [](Case& c) { c.C = 3; c.M = 1; c.act = 0; });
  add("bw_c3_m85_n255", BNBWD, [](Case& c) { c.C = 3; c.M = 85; });
  add("bw_c64_m4_n256", BNBWD, [](Case& c) { c.C = 64; c.M = 4; c.act = 0; });
  add("bw_c1_m257_n257", BNBWD, [](Case& c) { c.C = 1; c.M = 257; });
  add("bw_c8_m5", BNBWD, [](Case& c) { c.C = 8; c.M = 5; c.data = 1; });
  add("bw_c256_m33_blk2", BNBWD, [](Case& c) { c.C = 256; c.M = 33; c.data = 1; });
  add("bw_c256_m2049_blk65", BNBWD, [](Case& c) { c.C = 256; c.M = 2049; c.data = 1; c.act = 0; });
  add("bw_c256_m6145_blk193", BNBWD, [](Case& c) { c.C = 256; c.M = 6145; c.data = 1; });
  add("bw_c256_m8193_blk257_two_passes", BNBWD, [](Case& c) { c.C = 256; c.M = 8193; c.data = 1; });
  add("bw_c100_m6724_blk83_empty_last", BNBWD, [](Case& c) { c.C = 100; c.M = 6724; c.data = 1; });
  add("bw_c1_m532475_blk65", BNBWD, [](Case& c) { c.C = 1; c.M = 532475; });
  add("bw_c3_m175000_blk65", BNBWD, [](Case& c) { c.C = 3; c.M = 175000; c.act = 0; });
  // c. column sums (bias gradients)
  for (int C : Cs) {
    const long M = 8 * (256 / C) - 1;
    add(nm("cs_c%ld_m%ld", C, M), COLSUM, [&](Case& c) { c.C = C; c.M = M; c.data = 1; });
  }
  add("cs_c3_m1", COLSUM, [](Case& c) { c.C = 3; c.M = 1; });
  add("cs_c8_m5", COLSUM, [](Case& c) { c.C = 8; c.M = 5; c.data = 1; });
  add("cs_c256_m33_blk2", COLSUM, [](Case& c) { c.C = 256; c.M = 33; c.data = 1; });
  add("cs_c3_m175000_blk65", COLSUM, [](Case& c) { c.C = 3; c.M = 175000; c.data = 1; });
  add("cs_c1_m532475_blk65", COLSUM, [](Case& c) { c.C = 1; c.M = 532475; c.data = 1; });
  add("cs_c256_m2049_blk65", COLSUM, [](Case& c) { c.C = 256; c.M = 2049; c.data = 1; });
  add("cs_c129_m4096_blk65_empty_last", COLSUM, [](Case& c) { c.C = 129; c.M = 4096; c.data = 1; });
  add("cs_c256_m6145_blk193", COLSUM, [](Case& c) { c.C = 256; c.M = 6145; c.data = 1; });
  // d. elementwise: n = 1, 255, 256, 257 and past 8192 * 256 elements; C 1, 3, 8, 64
  const long ew[6][2] = {{1, 1}, {85, 3}, {32, 8}, {257, 1}, {4, 64}, {32769, 64}};
  for (int i = 0; i < 6; ++i) {
    const long M = ew[i][0];
    const int C = (int)ew[i][1];
    add(nm("bnact_m%ld_c%ld_act%ld", M, C, i & 1), BNACT, [&](Case& c) { c.M = M; c.C = C; c.act = i & 1; });
    add(nm("atts_m%ld_c%ld", M, C), ATT_S, [&](Case& c) { c.M = M; c.C = C; });
    add(nm("attsb_m%ld_c%ld", M, C), ATT_S_BWD, [&](Case& c) { c.M = M; c.C = C; });
    add(nm("sdg_m%ld_c%ld_o%ld_acc%ld", M, C, i % 2 ? 3 : 1, (i / 2) & 1), SMALL_DGRAD,
        [&](Case& c) { c.M = M; c.C = C; c.O = i % 2 ? 3 : 1; c.acc = (i / 2) & 1; });
  }
  add("sdg_m32_c8_o3_acc0", SMALL_DGRAD, [](Case& c) { c.M = 32; c.C = 8; c.O = 3; c.acc = 0; });
  add("sdg_m85_c3_o1_acc1", SMALL_DGRAD, [](Case& c) { c.M = 85; c.C = 3; c.O = 1; c.acc = 1; });
  for (long n : {1L, 255L, 256L, 257L, 2097153L}) add(nm("add_n%ld", n), ADD, [&](Case& c) { c.M = n; });
  // e. pool + Dropout and its backward: inference and the layers 0 .. 3, odd sizes whose last row and column are
  // unread, a batch offset and two steps with B >= 2, one case past the first grid-stride pass
  auto pool = [&](const char* name, int B, int H, int W, int C, int layer, int gimg0, long step) {
    add(name, POOL, [&](Case& c) { c.B = B; c.H = H; c.W = W; c.C = C; c.layer = layer; c.gimg0 = gimg0; c.step = step; });
  };
  pool("pool_b1_2x2_c1_inf", 1, 2, 2, 1, -1, 0, 0);
  pool("pool_b1_2x2_c1_l0", 1, 2, 2, 1, 0, 0, 0);
  pool("pool_b2_4x6_c3_l0_g3", 2, 4, 6, 3, 0, 3, 0);
  pool("pool_b2_4x6_c3_l0_g3_step1", 2, 4, 6, 3, 0, 3, 1);
  pool("pool_b1_5x7_c8_l1", 1, 5, 7, 8, 1, 0, 0);
  pool("pool_b1_5x7_c8_inf", 1, 5, 7, 8, -1, 0, 0);
  pool("pool_b3_16x16_c16_l2_g5", 3, 16, 16, 16, 2, 5, 0);
  pool("pool_b3_16x16_c16_l3_step2", 3, 16, 16, 16, 3, 0, 2);
  pool("pool_b2_1026x1026_c4_l1_two_passes", 2, 1026, 1026, 4, 1, 1, 1);
  // f. the attention's 1-channel conv
  for (long M : {1L, 257L})
    for (int C : {1, 8, 64}) add(nm("attt_m%ld_c%ld", M, C), ATT_T, [&](Case& c) { c.M = M; c.C = C; });
  add("attt_m2097153_c1_two_passes", ATT_T, [](Case& c) { c.M = 2097153; c.C = 1; });
  // g. the gate, the concat and its backward: every C, pixel counts that leave clamped lanes beside live ones, an
  // image boundary inside a workgroup, saturated gates, inference (forward only) and the layers 4 .. 7
  auto cat = [&](const char* name, int C, int B, long HW, int layer, int flav, int gimg0, long step) {
    add(name, ATT_CAT, [&](Case& c) { c.C = C; c.B = B; c.HW = HW; c.layer = layer; c.flav = flav; c.gimg0 = gimg0; c.step = step; });
  };
  cat("cat_c1_b1_hw7_l4", 1, 1, 7, 4, 0, 0, 0);
  cat("cat_c2_b2_hw9_l5", 2, 2, 9, 5, 0, 0, 0);
  cat("cat_c4_b1_hw70_l6", 4, 1, 70, 6, 0, 0, 0);
  cat("cat_c8_b1_hw5_l7", 8, 1, 5, 7, 0, 0, 0);
  cat("cat_c8_b1_hw33_l4", 8, 1, 33, 4, 0, 0, 0);
  cat("cat_c8_b2_hw5_l5_g2_step1", 8, 2, 5, 5, 0, 2, 1);
  cat("cat_c16_b2_hw17_l6", 16, 2, 17, 6, 0, 0, 0);
  cat("cat_c32_b1_hw9_l7", 32, 1, 9, 7, 0, 0, 0);
  cat("cat_c64_b2_hw3_l4", 64, 2, 3, 4, 0, 0, 0);
  cat("cat_c8_b1_hw40_l5_saturated", 8, 1, 40, 5, 1, 0, 0);
  cat("cat_c4_b2_hw33_l6_saturated", 4, 2, 33, 6, 1, 1, 0);
  cat("cat_c8_b2_hw6_inf", 8, 2, 6, -1, 0, 0, 0);
  cat("cat_c64_b1_hw5_inf_saturated", 64, 1, 5, -1, 1, 0, 0);
  // h. the output layer, its loss and un_out: C 1, 5, 8; one row, 255, 3 x 257, and 262 145 rows (the second sweep)
  auto out = [&](const char* name, int C, int B, long HW, int flav) {
    add(name, OUT, [&](Case& c) { c.C = C; c.B = B; c.HW = HW; c.M = B * HW; c.flav = flav; });
  };
  out("out_c1_b1_hw1", 1, 1, 1, 0);
  out("out_c8_b1_hw1", 8, 1, 1, 0);
  out("out_c1_b1_hw255", 1, 1, 255, 0);
  out("out_c5_b1_hw255", 5, 1, 255, 0);
  out("out_c5_b3_hw257", 5, 3, 257, 0);
  out("out_c8_b3_hw257", 8, 3, 257, 0);
  out("out_c8_b3_hw257_target_is_output", 8, 3, 257, 1);
  out("out_c1_b1_hw262145_second_sweep", 1, 1, 262145, 0);
  out("out_c5_b1_hw262145_second_sweep", 5, 1, 262145, 0);
  out("out_c8_b1_hw262145_target_is_output", 8, 1, 262145, 1);
  // i. the Masker's permutation and crops: more images than threads, H != W, P = 1, P < min(H, W), P = H = W
  auto perm = [&](const char* name, int B, int H, int W, int P, int gimg0, long step) {
    add(name, PERM, [&](Case& c) { c.B = B; c.H = H; c.W = W; c.P = P; c.gimg0 = gimg0; c.step = step; });
  };
  perm("perm_b1_h3_w5_p1", 1, 3, 5, 1, 0, 0);
  perm("perm_b2_h6_w9_p4", 2, 6, 9, 4, 0, 0);
  perm("perm_b5_h6_w6_p6", 5, 6, 6, 6, 0, 0);
  perm("perm_b5_h7_w4_p3_g7_step2", 5, 7, 4, 3, 7, 2);
  perm("perm_b257_h3_w4_p2", 257, 3, 4, 2, 0, 1);
  // j. the box filter
  auto flt = [&](const char* name, int B, int maxo, int sets, int nc_mode, int flav) {
    add(name, FILTER, [&](Case& c) { c.B = B; c.maxo = maxo; c.sets = sets; c.nc_mode = nc_mode; c.flav = flav; });
  };
  flt("flt_b1_sets0", 1, 8, 0, 0, 0);
  flt("flt_b64_edges_sets15", 64, 100, 15, 2, 1);
  flt("flt_b65_edges_sets1", 65, 100, 1, 0, 1);
  flt("flt_b65_nc0_sets15", 65, 8, 15, 1, 0);
  flt("flt_b64_ncmax_sets6", 64, 8, 6, 2, 0);
  flt("flt_b5_all_rejected_sets15", 5, 16, 15, 3, 0);
  flt("flt_b65_sets8", 65, 8, 8, 0, 0);
  // k. refusals: the launcher throws before anything is launched
  add("refuse_pool_bwd_odd_h", REFUSE, [](Case& c) { c.refuse = R_POOL_BWD_ODD_H; c.B = 1; c.H = 5; c.W = 6; c.C = 3; c.layer = 0; });
  add("refuse_pool_bwd_odd_w", REFUSE, [](Case& c) { c.refuse = R_POOL_BWD_ODD_W; c.B = 2; c.H = 4; c.W = 7; c.C = 1; c.layer = 1; });
  add("refuse_cat_bwd_c0", REFUSE, [](Case& c) { c.refuse = R_CAT_BWD_C0; c.C = 0; c.B = 1; c.HW = 5; c.layer = 4; });
  add("refuse_cat_bwd_c3", REFUSE, [](Case& c) { c.refuse = R_CAT_BWD_C3; c.C = 3; c.B = 1; c.HW = 5; c.layer = 4; });
  add("refuse_cat_bwd_c128", REFUSE, [](Case& c) { c.refuse = R_CAT_BWD_C128; c.C = 128; c.B = 1; c.HW = 5; c.layer = 4; });
  return t;
}
// ---- end of the table --------------------------------------------------------------------------

// ---- device buffers ----------------------------------------------------------------------------
struct In {  // an input: what was uploaded is kept, to show the launch left it alone
  uint8_t* d = nullptr;
  std::vector<uint8_t> h;
  In() = default;
  In(const In&) = delete;
  In& operator=(const In&) = delete;
  ~In() { if (d) (void)hipFree(d); }
  void put(const void* p, size_t bytes) {
    h.assign((const uint8_t*)p, (const uint8_t*)p + bytes);
    CK(hipMalloc(reinterpret_cast<void**>(&d), std::max<size_t>(bytes, 16)));
    if (bytes) CK(hipMemcpy(d, p, bytes, hipMemcpyHostToDevice));
  }
  const float* f() const { return reinterpret_cast<const float*>(d); }
  template <class T> const T* as() const { return reinterpret_cast<const T*>(d); }
  bool same() const {
    std::vector<uint8_t> g(h.size());
    if (!g.empty()) CK(hipMemcpy(g.data(), d, g.size(), hipMemcpyDeviceToHost));
    return g == h;
  }
};
struct Flags {
  bool canary_ok = true, inputs_ok = true, repeat_ok = true, scratch_ok = true;
};
struct Job {
  hipStream_t st;
  std::vector<std::unique_ptr<In>> ins;
  std::vector<std::unique_ptr<Guarded>> outs;
  explicit Job(hipStream_t s) : st(s) {}
  template <class T> In* in(const std::vector<T>& v) {
    ins.emplace_back(new In);
    ins.back()->put(v.data(), v.size() * sizeof(T));
    return ins.back().get();
  }
  // an output: the payload starts as `v` (its fill, or the old value of an accumulating call)
  template <class T> Guarded* io(const std::vector<T>& v) {
    outs.emplace_back(new Guarded);
    outs.back()->alloc(v.size() * sizeof(T));
    std::memcpy(outs.back()->fill(), v.data(), v.size() * sizeof(T));
    return outs.back().get();
  }
  // launch, read back, check guards and inputs; launch again over fresh fills: bit-equal.  true = the launcher threw
  bool run(const std::function<void()>& launch, Flags& F) {
    bool threw = false;
    std::vector<std::vector<uint8_t>> first;
    for (int rep = 0; rep < 2; ++rep) {
      for (auto& o : outs) o->upload();
      try {
        launch();
      } catch (const std::runtime_error&) {
        threw = true;
      }
      CK(hipStreamSynchronize(st));
      for (size_t i = 0; i < outs.size(); ++i) {
        outs[i]->download();
        F.canary_ok &= outs[i]->intact();
        if (rep == 0) first.push_back(outs[i]->got);
        else F.repeat_ok &= outs[i]->got == first[i];
      }
    }
    for (auto& i : ins) F.inputs_ok &= i->same();
    return threw;
  }
};
template <class T> static void back(const Guarded* g, std::vector<T>& v) {
  if (!v.empty()) std::memcpy(v.data(), g->out(), v.size() * sizeof(T));
}

// the library's expf and tanhf on the device, for the two figures (not kernels under test)
__global__ void k_expf(const float* __restrict__ x, float* __restrict__ y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = expf(x[i]);
}
__global__ void k_tanhf(const float* __restrict__ x, float* __restrict__ y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = tanhf(x[i]);
}
static double max_ulp(const VF& x, const VF& y, bool is_exp) {
  double w = 0;
  for (size_t i = 0; i < x.size(); ++i) w = std::max(w, ulp_err(y[i], is_exp ? std::exp((double)x[i]) : std::tanh((double)x[i])));
  return w;
}
static double measure_device(bool is_exp, hipStream_t st) {
  const VF x = is_exp ? exp_args() : tanh_args();
  VF y = filled(x.size());
  Job j(st);
  In* xi = j.in(x);
  Guarded* yo = j.io(y);
  yo->upload();
  if (is_exp) hipLaunchKernelGGL(k_expf, dim3((unsigned)((x.size() + 255) / 256)), dim3(256), 0, st, xi->f(), yo->ptr(), (int)x.size());
  else hipLaunchKernelGGL(k_tanhf, dim3((unsigned)((x.size() + 255) / 256)), dim3(256), 0, st, xi->f(), yo->ptr(), (int)x.size());
  CK(hipGetLastError());
  CK(hipStreamSynchronize(st));
  yo->download();
  back(yo, y);
  return max_ulp(x, y, is_exp);
}

// ---- the device backend ------------------------------------------------------------------------
struct Gpu : Backend {
  Flags F;
  hipStream_t st;
  explicit Gpu(hipStream_t s) : st(s) {}
  Guarded* scratch(Job& j, VD& part, size_t want) {
    F.scratch_ok &= part.size() == want;  // the harness's geometry is the launcher's
    part.assign(want, std::nan(""));
    Guarded* g = j.io(part);
    g->fill32(kFillWord);
    return g;
  }
  void bn_stats(const VF& y, long M, int C, const VF& gamma, bool moving, VF& mm, VF& mv, VF& mean, VF& rstd, VF& sc, VD& part) override {
    Job j(st);
    In *yi = j.in(y), *gi = j.in(gamma);
    Guarded *o1 = j.io(mean), *o2 = j.io(rstd), *o3 = j.io(sc), *o4 = j.io(mm), *o5 = j.io(mv), *pp = scratch(j, part, un_colred_doubles(M, C));
    j.run([&] {
      un_bn_stats(yi->f(), M, C, gi->f(), o1->ptr(), o2->ptr(), o3->ptr(), moving ? o4->ptr() : nullptr, moving ? o5->ptr() : nullptr,
                  reinterpret_cast<double*>(pp->ptr()), st);
    }, F);
    back(o1, mean); back(o2, rstd); back(o3, sc); back(o4, mm); back(o5, mv); back(pp, part);
  }
  void bn_bwd(const VF& da, const VF& y, long M, int C, const VF& mu, const VF& rstd, const VF& sc, const VF& be, int act, VF& mdz,
              VF& mdzx, VF& dgamma, VF& dbeta, VF& dy, VD& part) override {
    Job j(st);
    In *i1 = j.in(da), *i2 = j.in(y), *i3 = j.in(mu), *i4 = j.in(rstd), *i5 = j.in(sc), *i6 = j.in(be);
    Guarded *o1 = j.io(mdz), *o2 = j.io(mdzx), *o3 = j.io(dgamma), *o4 = j.io(dbeta), *o5 = j.io(dy), *pp = scratch(j, part, un_colred_doubles(M, C));
    j.run([&] {
      un_bn_bwd(i1->f(), i2->f(), M, C, i3->f(), i4->f(), i5->f(), i6->f(), act, o1->ptr(), o2->ptr(), o3->ptr(), o4->ptr(), o5->ptr(),
                reinterpret_cast<double*>(pp->ptr()), st);
    }, F);
    back(o1, mdz); back(o2, mdzx); back(o3, dgamma); back(o4, dbeta); back(o5, dy); back(pp, part);
  }
  void colsum(const VF& v, long M, int C, VF& out, VD& part) override {
    Job j(st);
    In* i1 = j.in(v);
    Guarded *o1 = j.io(out), *pp = scratch(j, part, un_colred_doubles(M, C));
    j.run([&] { un_colsum(i1->f(), M, C, o1->ptr(), reinterpret_cast<double*>(pp->ptr()), st); }, F);
    back(o1, out); back(pp, part);
  }
  void bnact(const VF& y, const Bn& b, long M, int C, int act, VF& a) override {
    Job j(st);
    In *i1 = j.in(y), *i2 = j.in(b.mu), *i3 = j.in(b.sc), *i4 = j.in(b.be);
    Guarded* o1 = j.io(a);
    j.run([&] { un_bnact(i1->f(), i2->f(), i3->f(), i4->f(), o1->ptr(), M, C, act, st); }, F);
    back(o1, a);
  }
  void pool(const VF& x, int B, int H, int W, int C, const Rk& k, VF& out, VB& arg) override {
    Job j(st);
    In* i1 = j.in(x);
    Guarded *o1 = j.io(out), *o2 = j.io(arg);
    j.run([&] { un_pool_drop(i1->f(), o1->ptr(), reinterpret_cast<uint8_t*>(o2->ptr()), B, H, W, C, k.seed, k.step, k.gimg0, k.layer, st); }, F);
    back(o1, out); back(o2, arg);
  }
  bool pool_bwd(const VF& dout, const VB& arg, VF& dx, int B, int H, int W, int C, const Rk& k, bool acc) override {
    Job j(st);
    In *i1 = j.in(dout), *i2 = j.in(arg);
    Guarded* o1 = j.io(dx);
    const bool threw = j.run([&] { un_pool_drop_bwd(i1->f(), i2->as<uint8_t>(), o1->ptr(), B, H, W, C, k.seed, k.step, k.gimg0, k.layer, acc, st); }, F);
    back(o1, dx);
    return threw;
  }
  void att_s(const VF& g, const VF& x, const Bn& b1, const Bn& b2, long M, int C, VF& s) override {
    Job j(st);
    In *i1 = j.in(g), *i2 = j.in(x), *a1 = j.in(b1.mu), *a2 = j.in(b1.sc), *a3 = j.in(b1.be), *c1 = j.in(b2.mu), *c2 = j.in(b2.sc), *c3 = j.in(b2.be);
    Guarded* o1 = j.io(s);
    j.run([&] { un_att_s(i1->f(), i2->f(), a1->f(), a2->f(), a3->f(), c1->f(), c2->f(), c3->f(), o1->ptr(), M, C, st); }, F);
    back(o1, s);
  }
  void att_t(const VF& s, const VF& w, float b, long M, int C, VF& t) override {
    Job j(st);
    const VF bv(1, b);
    In *i1 = j.in(s), *i2 = j.in(w), *i3 = j.in(bv);
    Guarded* o1 = j.io(t);
    j.run([&] { un_att_t(i1->f(), i2->f(), i3->f(), o1->ptr(), M, C, st); }, F);
    back(o1, t);
  }
  void att_cat(const VF& up, const VF& skip, const VF& t, const float bn3[3], int B, long HW, int C, const Rk& k, VF& cat) override {
    Job j(st);
    const VF m3(1, bn3[0]), s3(1, bn3[1]), b3(1, bn3[2]);
    In *i1 = j.in(up), *i2 = j.in(skip), *i3 = j.in(t), *i4 = j.in(m3), *i5 = j.in(s3), *i6 = j.in(b3);
    Guarded* o1 = j.io(cat);
    j.run([&] { un_att_cat(i1->f(), i2->f(), i3->f(), i4->f(), i5->f(), i6->f(), o1->ptr(), B, HW, C, k.seed, k.step, k.gimg0, k.layer, st); }, F);
    back(o1, cat);
  }
  bool att_cat_bwd(const VF& dcat, const VF& skip, const VF& t, const float bn3[3], int B, long HW, int C, const Rk& k, VF& dup, VF& dskip,
                   VF& dz3) override {
    Job j(st);
    const VF m3(1, bn3[0]), s3(1, bn3[1]), b3(1, bn3[2]);
    In *i1 = j.in(dcat), *i2 = j.in(skip), *i3 = j.in(t), *i4 = j.in(m3), *i5 = j.in(s3), *i6 = j.in(b3);
    Guarded *o1 = j.io(dup), *o2 = j.io(dskip), *o3 = j.io(dz3);
    const bool threw = j.run([&] {
      un_att_cat_bwd(i1->f(), i2->f(), i3->f(), i4->f(), i5->f(), i6->f(), o1->ptr(), o2->ptr(), o3->ptr(), B, HW, C, k.seed, k.step, k.gimg0,
                     k.layer, st);
    }, F);
    back(o1, dup); back(o2, dskip); back(o3, dz3);
    return threw;
  }
  void att_s_bwd(const VF& dt, const VF& w3, const VF& g, const VF& x, const Bn& b1, const Bn& b2, long M, int C, VF& dsum) override {
    Job j(st);
    In *i0 = j.in(dt), *iw = j.in(w3), *i1 = j.in(g), *i2 = j.in(x), *a1 = j.in(b1.mu), *a2 = j.in(b1.sc), *a3 = j.in(b1.be), *c1 = j.in(b2.mu),
       *c2 = j.in(b2.sc), *c3 = j.in(b2.be);
    Guarded* o1 = j.io(dsum);
    j.run([&] { un_att_s_bwd(i0->f(), iw->f(), i1->f(), i2->f(), a1->f(), a2->f(), a3->f(), c1->f(), c2->f(), c3->f(), o1->ptr(), M, C, st); }, F);
    back(o1, dsum);
  }
  void out_loss(const VF& x, const VF& w, const VF& b, const VF& tgt, long M, long HW, int C, VF& upd, VF& dz, VD& lpart, VF& loss) override {
    Job j(st);
    In *i1 = j.in(x), *i2 = j.in(w), *i3 = j.in(b), *i4 = j.in(tgt);
    Guarded *o1 = j.io(upd), *o2 = j.io(dz), *o3 = j.io(loss), *pp = scratch(j, lpart, (size_t)un_loss_blocks(M));
    j.run([&] { un_out_loss(i1->f(), i2->f(), i3->f(), i4->f(), o1->ptr(), o2->ptr(), reinterpret_cast<double*>(pp->ptr()), o3->ptr(), M, HW, C, st); }, F);
    back(o1, upd); back(o2, dz); back(o3, loss); back(pp, lpart);
  }
  void out(const VF& x, const VF& w, const VF& b, long M, int C, VF& upd) override {
    Job j(st);
    In *i1 = j.in(x), *i2 = j.in(w), *i3 = j.in(b);
    Guarded* o1 = j.io(upd);
    j.run([&] { un_out(i1->f(), i2->f(), i3->f(), o1->ptr(), M, C, st); }, F);
    back(o1, upd);
  }
  void small_dgrad(const VF& dz, const VF& w, VF& dx, long M, int C, int O, bool acc) override {
    Job j(st);
    In *i1 = j.in(dz), *i2 = j.in(w);
    Guarded* o1 = j.io(dx);
    j.run([&] { un_small_dgrad(i1->f(), i2->f(), o1->ptr(), M, C, O, acc, st); }, F);
    back(o1, dx);
  }
  void add(VF& a, const VF& b, long n) override {
    Job j(st);
    In* i1 = j.in(b);
    Guarded* o1 = j.io(a);
    j.run([&] { un_add(o1->ptr(), i1->f(), n, st); }, F);
    back(o1, a);
  }
  void perm_crops(const VF& images, int B, int H, int W, int P, const Rk& k, VI& info, VF& crops) override {
    Job j(st);
    In* i1 = j.in(images);
    Guarded *o1 = j.io(info), *o2 = j.io(crops);
    j.run([&] { def_perm_crops(i1->f(), reinterpret_cast<int*>(o1->ptr()), o2->ptr(), B, H, W, P, k.seed, k.step, k.gimg0, st); }, F);
    back(o1, info); back(o2, crops);
  }
  void filter(const VF& nb, const VF& ns, const VI& nc, int B, int maxo, float H, float W, float thresh, int sets, VF& ob, VI& oc, VF& os,
              VF& b2, VF& s2, VI& c2) override {
    Job j(st);
    In *i1 = j.in(nb), *i2 = j.in(ns), *i3 = j.in(nc);
    Guarded *o1 = j.io(ob), *o2 = j.io(oc), *o3 = j.io(os), *o4 = j.io(b2), *o5 = j.io(s2), *o6 = j.io(c2);
    j.run([&] {
      DefKeep k2;
      if (sets & 2) k2.boxes = o4->ptr();
      if (sets & 4) k2.scores = o5->ptr();
      if (sets & 8) k2.count = reinterpret_cast<int*>(o6->ptr());
      def_filter(i1->f(), i2->f(), i3->as<int>(), B, maxo, H, W, thresh, o1->ptr(), reinterpret_cast<int*>(o2->ptr()), st,
                 (sets & 1) ? o3->ptr() : nullptr, k2);
    }, F);
    back(o1, ob); back(o2, oc); back(o3, os); back(o4, b2); back(o5, s2); back(o6, c2);
  }
};

// ---- lines -------------------------------------------------------------------------------------
static const char* tf(bool b) { return b ? "true" : "false"; }
static long sweep_elems(const Case& c) {  // the elements the launch's grid-stride loop runs over (0: no such loop)
  switch (c.op) {
    case BNBWD: case BNACT: case ATT_S: case ATT_S_BWD: case SMALL_DGRAD: return c.M * c.C;
    case ADD: case ATT_T: case OUT: return c.M;
    case POOL: return (long)c.B * (c.H / 2) * (c.W / 2) * c.C;
    case ATT_CAT: return (long)c.B * c.HW * 2 * c.C;
    default: return 0;
  }
}
static std::string case_json(const Case& c) {
  char b[640];
  const long n = sweep_elems(c);
  const long per_sweep = c.op == OUT ? (long)loss_blocks(c.M) * 256 : grid_blocks(n) * 256;
  snprintf(b, sizeof b,
           "\"case\":\"%s\",\"op\":\"%s\",\"refuse\":%d,\"M\":%ld,\"C\":%d,\"B\":%d,\"H\":%d,\"W\":%d,\"HW\":%ld,\"act\":%d,\"flav\":%d,"
           "\"data\":%d,\"acc\":%d,\"layer\":%d,\"gimg0\":%d,\"step\":%ld,\"O\":%d,\"P\":%d,\"maxo\":%d,\"sets\":%d,\"nc_mode\":%d,\"n\":%ld,"
           "\"sweeps\":%ld",
           c.name.c_str(), kOpName[c.op], c.refuse, c.M, c.C, c.B, c.H, c.W, c.HW, c.act, c.flav, c.data, c.acc, c.layer, c.gimg0, c.step, c.O,
           c.P, c.maxo, c.sets, c.nc_mode, n, n ? cdivl(n, per_sweep) : 0);
  std::string s = b;
  if (c.op == STATS || c.op == BNBWD || c.op == COLSUM) {
    const ColredPlanInfo L = un_colred_plan_info(c.M, c.C);  // the library's own
    const ColredPlan p = colred_plan(c.M, c.C);
    const bool same = L.blocks == p.blocks && L.rows_per_block == p.rpb && L.lane_rows == p.lane_rows && L.idle == p.idle &&
                      L.last_rows == p.last_rows && un_colred_doubles(c.M, c.C) == (size_t)L.blocks * c.C * 2;
    snprintf(b, sizeof b, ",\"red\":{\"blocks\":%d,\"rpb\":%ld,\"lane_rows\":%d,\"idle\":%d,\"last_rows\":%ld,\"check_same\":%s}", L.blocks,
             L.rows_per_block, L.lane_rows, L.idle, L.last_rows, tf(same));
    s += b;
  }
  if (c.op == OUT) s += ",\"loss_blocks\":" + std::to_string(un_loss_blocks(c.M)) + ",\"check_loss_blocks\":" + std::to_string(loss_blocks(c.M));
  return s;
}

int main(int argc, char** argv) {
  const bool plan = argc > 1 && std::string(argv[1]) == "--plan";
  {
    const std::string self = argv[0];
    const size_t sl = self.rfind('/');
    g_golden.load((sl == std::string::npos ? std::string(".") : self.substr(0, sl)) + "/../golden/unet");
  }
  const std::vector<Case> t = table();
  const auto t0 = std::chrono::steady_clock::now();
  if (plan) {
    // the host's expf / tanhf through the same measurement, for the stand-in's bounds
    VF xe = exp_args(), ye(xe.size()), xt = tanh_args(), yt(xt.size());
    for (size_t i = 0; i < xe.size(); ++i) ye[i] = expf(xe[i]);
    for (size_t i = 0; i < xt.size(); ++i) yt[i] = tanhf(xt[i]);
    set_ulps(max_ulp(xe, ye, true), max_ulp(xt, yt, false));
    printf("{\"head\":true,\"red_elems\":%ld,\"red_maxblk\":%ld,\"golden_read\":%s,\"fd_gap\":%s}\n", kRedElems, kRedMaxBlk, tf(g_golden.read),
           jnum(cat_bwd_fd_gap()).c_str());
    for (const Case& c : t) {
      Sim sim;
      Verdict v;
      run_case(c, sim, v);
      const bool pass = c.refuse ? (v.threw && v.untouched) : (!v.threw && v.ratio() <= 1.0 && v.exact_ok() && v.nonfinite == 0);
      printf("{%s,%s,\"standin_pass\":%s}\n", case_json(c).c_str(), verdict_json(v).c_str(), tf(pass));
      fflush(stdout);
    }
    printf("{\"done\":true,\"cases\":%d}\n", (int)t.size());
    return 0;
  }
  hipStream_t st;
  CK(hipStreamCreate(&st));
  const double eu = measure_device(true, st), tu = measure_device(false, st);
  set_ulps(eu, tu);
  printf("{\"head\":true,\"exp_ulp_measured\":%s,\"tanh_ulp_measured\":%s,\"exp_ulp_used\":%s,\"tanh_ulp_used\":%s,\"golden_read\":%s}\n",
         jnum(eu).c_str(), jnum(tu).c_str(), jnum(g_exp_ulp).c_str(), jnum(g_tanh_ulp).c_str(), tf(g_golden.read));
  fflush(stdout);
  int ran = 0;
  for (const Case& c : t) {
    g_case = c.name.c_str();
    Gpu gpu(st);
    Verdict v;
    try {
      run_case(c, gpu, v);
    } catch (const std::exception& e) {
      v.threw = true;
      v.what = e.what();
    }
    const Flags& F = gpu.F;
    const bool common = F.canary_ok && F.repeat_ok && F.inputs_ok && F.scratch_ok;
    const bool pass = common && (c.refuse ? (v.threw && v.untouched)
                                          : (!v.threw && v.ratio() <= 1.0 && v.exact_ok() && v.nonfinite == 0 && v.kink_share() <= 0.01));
    printf("{%s,%s,\"canary_ok\":%s,\"repeat_ok\":%s,\"inputs_ok\":%s,\"scratch_ok\":%s,\"what\":\"%s\",\"pass\":%s}\n", case_json(c).c_str(),
           verdict_json(v).c_str(), tf(F.canary_ok), tf(F.repeat_ok), tf(F.inputs_ok), tf(F.scratch_ok), esc(v.what).c_str(), tf(pass));
    fflush(stdout);
    ++ran;
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("{\"done\":true,\"cases\":%d,\"seconds\":%s}\n", ran, jnum(sec).c_str());
  CK(hipStreamDestroy(st));
  return 0;
}
