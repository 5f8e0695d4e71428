// gemm_parity — kernel-level parity of the 1x1-conv GEMM family against an fp64 host reference.
//
//   gemm_parity --plan     what plan_gemm2 / plan_gemm chooses for every case of the table (host code
//                          only: runs without a GPU)
//   gemm_parity            run the table on the GPU: one flushed JSON line per case, then a `done` line
//   gemm_parity --shape M N K [bf16]   the plan of one shape (for choosing table entries)
//
// Only the product's launchers (kernels.hpp) are called: launch_gemm, launch_gemm_dgrad,
// gemm_group_run, and gemm2_run(..., allow_wsk = false) for the cross-workgroup split-K the im2col and
// U-Net callers use.  The exit status is 0 when every case ran (the verdicts are in the lines); a HIP
// error ends the process at once with a `fatal` line and status 3.  Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gemm_check.hpp"
#include "kernels.hpp"
#include "parity_dev.hpp"

using namespace phx;

// ---- the case table ----------------------------------------------------------------------------
enum Route { FWD, DGRAD, SPLIT, GROUP, REFUSE };
enum Sink { NONE = 0, STAT = 1, GRAD = 2 };
enum Refuse { R_K4 = 1, R_STATS_ACC, R_STATS_N3, R_GSINK_MODE1, R_NULL_VIEW, R_GROUP_ROWS };

struct Case {
  const char* name;
  const char* expect;  // the path the entry was chosen for (tests/test_gemm_parity_host.py holds --plan to it)
  Route route;
  int M, N, K;
  int mode, act;
  bool bias, acc;
  int sink;
  bool bf16;
  int rpi = 1;
  int force_wsk = 0;  // tm * 10 + tn through gemm2_force_wsk (only where wsk_pick returns the tile at no small shape)
  int nseg = 0;
  int Ms[kMaxSeg] = {0, 0, 0, 0, 0};
  int refuse = 0;
};

static std::vector<Case> table() {
  std::vector<Case> t;
  auto add = [&](const char* name, const char* expect, Route r, int M, int N, int K, int mode, int act, bool bias,
                 bool acc, int sink, bool bf16 = false, int rpi = 1, int force = 0) {
    Case c{name, expect, r, M, N, K, mode, act, bias, acc, sink, bf16};
    c.rpi = rpi;
    c.force_wsk = force;
    t.push_back(c);
  };
  auto grp = [&](const char* name, const char* expect, int n, std::initializer_list<int> Ms, int N, int K, int mode,
                 int act, bool bias, int sink, int refuse = 0) {
    Case c{name, expect, refuse ? REFUSE : GROUP, *Ms.begin(), N, K, mode, act, bias, false, sink, false};
    c.nseg = n;
    int i = 0;
    for (int m : Ms) c.Ms[i++] = m;
    c.refuse = refuse;
    t.push_back(c);
  };
  // a. k_gemm2 unsplit, every tile key (M ragged against the block rows, N no multiple of 32)
  add("g2_411_k4_plain_n22", "g2:411", FWD, 16385, 22, 4, 0, 0, true, false, NONE);   // last tile: one row
  add("g2_411_k20_stat_bn_swish", "g2:411", FWD, 16300, 20, 20, 1, 1, true, false, STAT);
  add("g2_411_k52_dgrad_gs_relu6", "g2:411", DGRAD, 16300, 20, 52, 3, 2, false, false, GRAD);
  add("g2_412_k20_stat", "g2:412", FWD, 65425, 52, 20, 0, 0, false, false, STAT);      // last tile: 17 rows
  add("g2_412_k36_acc_bias_relu6", "g2:412", FWD, 65425, 50, 36, 1, 2, true, true, NONE);
  add("g2_211_k52_stat_se", "g2:211", FWD, 8145, 36, 52, 2, 1, true, false, STAT, false, 100);
  add("g2_211_k4_dgrad_acc", "g2:211", DGRAD, 8145, 36, 4, 3, 1, false, true, NONE);
  add("g2_413_k20_plain_n82", "g2:413", FWD, 16385, 82, 20, 1, 1, true, false, NONE);  // 810's N % 4 == 2
  add("g2_413_k52_stat", "g2:413", FWD, 16290, 84, 52, 1, 2, false, false, STAT);
  add("g2_222_k52_stat", "g2:222", FWD, 65425, 100, 52, 1, 1, true, false, STAT);
  add("g2_222_k20_dgrad_gs", "g2:222", DGRAD, 65409, 100, 20, 3, 1, false, false, GRAD);
  add("g2_212_k12_stat", "g2:212", FWD, 32730, 100, 12, 1, 1, false, false, STAT);
  add("g2_212_k16_acc", "g2:212", FWD, 32705, 102, 16, 0, 0, true, true, NONE);
  add("g2_111_k52_stat_se", "g2:111", FWD, 4097, 100, 52, 2, 1, true, false, STAT, false, 1);
  add("g2_111_k20_dgrad_gs_acc", "g2:111", DGRAD, 4100, 100, 20, 3, 2, false, true, GRAD);
  add("g2_415_k20_stat", "g2:415", FWD, 16385, 148, 20, 1, 1, true, false, STAT);
  add("g2_415_k52_plain_n150", "g2:415", FWD, 16290, 150, 52, 0, 0, false, false, NONE);
  // a'. the same kernels at few rows and wide N (the sinks' bounds grow with M: at M <= ~2000 they are
  // tight enough that one row too many or too few in a column's sums fails them)
  add("g2_111_wide_stat", "g2:111", FWD, 100, 4004, 20, 1, 1, true, false, STAT);
  add("g2_212_wide_k12_stat", "g2:212", FWD, 1000, 4004, 12, 1, 2, true, false, STAT);
  add("g2_222_wide_stat", "g2:222", FWD, 1950, 4004, 68, 1, 1, false, false, STAT);
  add("g2_413_wide_dgrad_gs", "g2:413", DGRAD, 400, 4032, 20, 3, 1, false, false, GRAD);
  add("g2_415_wide_dgrad_gs", "g2:415", DGRAD, 700, 4000, 36, 3, 2, false, true, GRAD);
  add("res_212_wide_stat", "res:212", FWD, 1950, 4004, 36, 1, 1, true, false, STAT);
  add("res_212_wide_dgrad_gs", "res:212", DGRAD, 1950, 4004, 20, 3, 1, false, false, GRAD);
  // b. k_gemm2r, every resident tile
  add("res_222_stat", "res:222", FWD, 32796, 300, 36, 1, 1, true, false, STAT);
  add("res_222_dgrad_gs", "res:222", DGRAD, 32796, 300, 20, 3, 1, false, false, GRAD);
  add("res_413_plain_acc", "res:413", FWD, 32700, 288, 36, 1, 2, true, true, NONE);
  add("res_413_stat", "res:413", FWD, 32700, 288, 52, 0, 0, false, false, STAT);
  add("res_415_stat", "res:415", FWD, 65420, 320, 36, 1, 1, false, false, STAT);
  add("res_415_dgrad_gs", "res:415", DGRAD, 65420, 320, 20, 3, 2, false, false, GRAD);
  add("res_212_plain_n530", "res:212", FWD, 8162, 530, 20, 2, 1, true, false, NONE, false, 100);
  add("res_212_stat", "res:212", FWD, 8162, 532, 52, 1, 1, true, false, STAT);
  add("res_212_dgrad_gs", "res:212", DGRAD, 8162, 532, 36, 3, 1, false, true, GRAD);
  // c. k_gemm2k, every tile wsk_pick returns, by the few route (small M, K = 64) and the deep-K route
  add("wsk_11_few_stat", "wsk:11:few", FWD, 1000, 52, 64, 1, 1, true, false, STAT);
  add("wsk_11_deep_dgrad_gs", "wsk:11:deep", DGRAD, 1000, 52, 328, 3, 1, false, false, GRAD);
  add("wsk_21_few_plain", "wsk:21:few", FWD, 16250, 22, 64, 0, 0, true, true, NONE);
  add("wsk_21_deep_stat", "wsk:21:deep", FWD, 16250, 20, 264, 1, 2, false, false, STAT);
  add("wsk_13_few_stat", "wsk:13:few", FWD, 16250, 84, 64, 1, 1, true, false, STAT);
  add("wsk_13_deep_dgrad_gs", "wsk:13:deep", DGRAD, 16250, 84, 260, 3, 2, false, false, GRAD);
  add("wsk_22_few_dgrad_gs", "wsk:22:few", DGRAD, 16250, 148, 64, 3, 1, false, true, GRAD);
  add("wsk_22_deep_stat", "wsk:22:deep", FWD, 16250, 148, 324, 1, 1, true, false, STAT);
  add("wsk_12_few_stat", "wsk:12:few", FWD, 2700, 192, 64, 1, 2, true, false, STAT);
  add("wsk_12_deep_stat", "wsk:12:deep", FWD, 2700, 180, 260, 1, 1, true, false, STAT);
  add("wsk_12_deep_dgrad", "wsk:12:deep", DGRAD, 2700, 180, 392, 3, 1, false, false, NONE);
  // d. cross-workgroup split-K (allow_wsk = false)
  add("split_k260_plain_acc_bias", "split", SPLIT, 300, 52, 260, 1, 1, true, true, NONE);
  add("split_k388_stat", "split", SPLIT, 333, 84, 388, 1, 2, true, false, STAT);
  add("split_k260_stat_se", "split", SPLIT, 300, 100, 260, 2, 1, false, false, STAT, false, 100);
  // e. the SE row scale across images (rows_per_img no multiple of the block rows)
  add("se_rpi100_3img", "wsk:11:few", FWD, 300, 36, 36, 2, 1, false, false, NONE, false, 100);
  add("se_rpi100_wsk", "wsk:11:few", FWD, 300, 52, 64, 2, 1, true, false, STAT, false, 100);
  add("se_rpi1", "wsk:11:few", FWD, 333, 36, 36, 2, 2, false, false, NONE, false, 1);
  // f. grouped
  grp("group3_stat", "group", 3, {4113, 1000, 20}, 36, 36, 1, 1, true, STAT);
  grp("group3_411_stat", "group", 3, {16385, 300, 7}, 20, 20, 1, 2, false, STAT);
  grp("group5_stat_raw", "group", 5, {16385, 4100, 1030, 260, 7}, 52, 20, 0, 0, true, STAT);
  grp("group5_dgrad_gs", "group", 5, {16385, 4100, 1030, 260, 7}, 52, 36, 3, 1, false, GRAD);
  grp("group3_res_stat", "group_res", 3, {8162, 1601, 40}, 532, 36, 1, 1, true, STAT);
  grp("group5_res_dgrad_gs", "group_res", 5, {8162, 3000, 1601, 401, 40}, 532, 20, 3, 2, false, GRAD);
  // g. N <= 16: the 16x16x4 kernel
  add("g1_n8_stat", "g1", FWD, 1001, 8, 36, 1, 1, true, false, STAT);
  add("g1_n16_stat", "g1", FWD, 4099, 16, 20, 0, 0, false, false, STAT);
  add("g1_n8_dgrad_gs", "g1", DGRAD, 1001, 8, 52, 3, 2, false, false, GRAD);
  add("g1_n16_dgrad_gs_acc", "g1", DGRAD, 4099, 16, 4, 3, 1, false, true, GRAD);
  // h. bf16 matrix cores: storage 1 (forward, A and C bf16) and 2 (gradient view, bf16 y)
  add("bf_g2_411_k36_stat", "g2:411", FWD, 16300, 20, 36, 1, 1, true, false, STAT, true);
  add("bf_g2_413_k4_plain", "g2:413", FWD, 16385, 82, 4, 0, 0, false, false, NONE, true);
  add("bf_g2_222_k100_dgrad_gs", "g2:222", DGRAD, 65409, 100, 100, 3, 1, false, false, GRAD, true);
  add("bf_res_222_stat", "res:222", FWD, 32796, 300, 68, 1, 1, true, false, STAT, true);
  add("bf_res_212_dgrad_gs", "res:212", DGRAD, 8162, 532, 68, 3, 2, false, false, GRAD, true);
  add("bf_wsk_13_few_stat", "wsk:13:few", FWD, 16250, 84, 64, 1, 1, true, false, STAT, true);
  add("bf_wsk_11_deep_dgrad_gs", "wsk:11:deep", DGRAD, 1000, 52, 328, 3, 1, false, false, GRAD, true);
  add("bf_split_k388_stat", "split", SPLIT, 333, 84, 388, 1, 1, true, false, STAT, true);
  add("bf_split_k260_acc", "split", SPLIT, 300, 52, 260, 1, 2, true, true, NONE, true);
  // i. argument refusals: host throws, nothing launched
  {
    Case c{"refuse_k_mod4", "refuse", REFUSE, 100, 36, 18, 0, 0, false, false, NONE, false};
    c.refuse = R_K4;
    t.push_back(c);
    c = Case{"refuse_stats_acc", "refuse", REFUSE, 100, 36, 20, 0, 0, false, true, STAT, false};
    c.refuse = R_STATS_ACC;
    t.push_back(c);
    c = Case{"refuse_stats_n_and_3", "refuse", REFUSE, 100, 38, 20, 0, 0, false, false, STAT, false};
    c.refuse = R_STATS_N3;
    t.push_back(c);
    c = Case{"refuse_gradsink_mode1", "refuse", REFUSE, 100, 36, 20, 1, 1, false, false, GRAD, false};
    c.refuse = R_GSINK_MODE1;
    t.push_back(c);
    c = Case{"refuse_null_view", "refuse", REFUSE, 100, 36, 20, 1, 1, false, false, NONE, false};
    c.refuse = R_NULL_VIEW;
    t.push_back(c);
  }
  grp("refuse_group_part_rows", "refuse", 3, {4113, 1000, 20}, 36, 36, 1, 1, true, STAT, R_GROUP_ROWS);
  return t;
}

// ---- the planner's choice ----------------------------------------------------------------------
struct Path {
  std::string path;
  int key = 0, splits = 1, wsk = 0, P = 0, gx = 0, gy = 0, gz = 1, kslice = 0;
  size_t res_lds = 0;
};

static Path path_of(const Case& c) {
  Path r;
  if (c.refuse && c.refuse != R_GROUP_ROWS) {
    r.path = "refuse";
    return r;
  }
  const int wgs = gemm2_target_wgs();
  if (c.route != GROUP && c.route != REFUSE && gemm_impl_for(c.N, c.bf16) == 1) {
    const GemmPlan p = plan_gemm(c.M, c.N, c.K);
    r.path = p.splits > 1 ? "g1:split" : "g1";
    r.key = p.wm * 100 + p.nt;
    r.splits = p.splits;
    r.gx = p.gx; r.gy = p.gy; r.gz = p.splits; r.kslice = p.kslice;
    r.P = p.gx;
    return r;
  }
  const bool nowsk = c.route == SPLIT || c.route == GROUP || c.route == REFUSE;
  if (c.force_wsk) gemm2_force_wsk(c.force_wsk / 10, c.force_wsk % 10);
  const Gemm2Plan p = plan_gemm2(c.M, c.N, c.K, wgs, c.bf16, true, !nowsk);
  if (c.force_wsk) gemm2_force_wsk(0, 0);
  const Gemm2Plan q = plan_gemm2(c.M, c.N, c.K, wgs, c.bf16, true, false);  // what the wave split replaces
  r.key = p.wm * 100 + p.tm * 10 + p.tn;
  r.splits = p.splits; r.wsk = p.wsk; r.P = p.P; r.res_lds = p.res_lds;
  r.gx = p.gx; r.gy = p.gy; r.gz = p.splits; r.kslice = p.kslice;
  char b[64];
  if (c.route == GROUP || c.route == REFUSE) {
    r.path = p.res_lds ? "group_res" : "group";
    r.gz = c.nseg;
    int gx = 1;
    for (int i = 0; i < c.nseg; ++i) gx = std::max(gx, plan_gemm2(c.Ms[i], c.N, c.K, wgs, c.bf16, true, false).gx);
    r.gx = gx;
    if (c.refuse) r.path = "refuse";
  } else if (p.wsk) {
    snprintf(b, sizeof b, "wsk:%d:%s", p.wsk, q.splits > 1 ? "deep" : "few");
    r.path = b;
  } else if (p.res_lds) {
    snprintf(b, sizeof b, "res:%d", r.key);
    r.path = b;
  } else if (p.splits > 1) {
    r.path = "split";
  } else {
    snprintf(b, sizeof b, "g2:%d", r.key);
    r.path = b;
  }
  return r;
}

// partial rows member i of a grouped launch gets (gemm_group_run's rule, from the members' plans)
static int group_rows(const Case& c, int i) {
  const int wgs = gemm2_target_wgs();
  const Gemm2Plan p0 = plan_gemm2(c.Ms[0], c.N, c.K, wgs, c.bf16, true, false);
  if (p0.res_lds) return cdiv(c.Ms[i], p0.wm * p0.tm * 32) * p0.wm;
  int gx = 1;
  for (int j = 0; j < c.nseg; ++j) gx = std::max(gx, plan_gemm2(c.Ms[j], c.N, c.K, wgs, c.bf16, true, false).gx);
  return gx;
}

static size_t split_floats(const Case& c) {
  if (c.route == SPLIT) {
    const Gemm2Plan p = plan_gemm2(c.M, c.N, c.K, gemm2_target_wgs(), c.bf16, true, false);
    return p.splits > 1 ? (size_t)p.splits * c.M * c.N : 0;
  }
  if (c.route == GROUP || c.route == REFUSE) return 0;
  return gemm_partial_floats(c.M, c.N, c.K, c.bf16);
}

// device bytes a case allocates (the cap of the table: under 256 MB)
static double device_bytes(const Case& c) {
  double rows = 0;
  if (c.nseg) for (int i = 0; i < c.nseg; ++i) rows += c.Ms[i];
  else rows = c.M;
  double b = rows * c.K * 4 * (c.mode == 3 ? 2 : 1) + (double)c.N * c.K * 4 + rows * c.N * 4 + split_floats(c) * 4.0;
  if (c.sink == GRAD) b += rows * c.N * 4;
  if (c.mode == 2) b += rows / c.rpi * c.K * 4;
  return b + 64 * 1024;  // parameters, sinks, guards
}

static void print_plan(const Case& c, FILE* f) {
  const Path p = path_of(c);
  double macs = 0;
  if (c.nseg) for (int i = 0; i < c.nseg; ++i) macs += (double)c.Ms[i] * c.N * c.K;
  else macs = (double)c.M * c.N * c.K;
  fprintf(f,
          "{\"case\":\"%s\",\"expect\":\"%s\",\"path\":\"%s\",\"route\":%d,\"M\":%d,\"N\":%d,\"K\":%d,\"mode\":%d,"
          "\"act\":%d,\"bias\":%d,\"acc\":%d,\"sink\":%d,\"bf16\":%d,\"rpi\":%d,\"forced\":%d,\"nseg\":%d,\"key\":%d,"
          "\"splits\":%d,\"kslice\":%d,\"wsk\":%d,\"res_lds\":%zu,\"P\":%d,\"grid\":[%d,%d,%d],\"macs\":%.0f,"
          "\"device_bytes\":%.0f}\n",
          c.name, c.expect, p.path.c_str(), (int)c.route, c.M, c.N, c.K, c.mode, c.act, (int)c.bias, (int)c.acc,
          c.sink, (int)c.bf16, c.rpi, c.force_wsk, c.nseg, p.key, p.splits, p.kslice, p.wsk, p.res_lds, p.P, p.gx,
          p.gy, p.gz, macs, device_bytes(c));
  fflush(f);
}

// one GEMM operand set (a member of a group, or the whole case)
struct Member {
  int M;
  std::vector<float> A, Y, Cprev, Y2;
  Dev dA, dY, dY2;
  Guarded C, part, cnt;
  int Pexp = 0;
};

struct Shared {
  std::vector<float> Bt, bias, rowscale, mu, sc, be, rstd, mdz, mdzx, mu2, sc2, be2, rstd2;
  Dev dBt, dbias, drs, dmu, dsc, dbe, drstd, dmdz, dmdzx, dmu2, dsc2, dbe2, drstd2;
};

struct Verdict {
  bool threw = false;
  std::string what;
  bool P_ok = true, canary_ok = true, repeat_ok = true;
  int P = 0, Pexp = 0;
  gck::CCheck c;
  gck::SinkCheck s;
  bool has_sink = false;
};

static void merge(Verdict& v, const gck::CCheck& c, const gck::SinkCheck& s) {
  if (c.ratio > v.c.ratio || v.c.worst < 0) {
    const long nf = v.c.nonfinite;
    v.c = c;
    v.c.nonfinite = nf;
  }
  v.c.nonfinite += c.nonfinite;
  v.s.rows_written &= s.rows_written;
  v.s.cnt_ok &= s.cnt_ok;
  v.s.cnt_sum_ok &= s.cnt_sum_ok;
  v.s.sum_ratio = std::max(v.s.sum_ratio, s.sum_ratio);
  v.s.m2_ratio = std::max(v.s.m2_ratio, s.m2_ratio);
}

static void make_shared(const Case& c, uint64_t seed, int max_rows, Shared& s) {
  const int K = c.K, N = c.N;
  s.Bt.resize((size_t)N * K);
  gck::fill_uni(s.Bt, seed + 1);
  s.bias.resize(N);
  gck::fill_uni(s.bias, seed + 2);
  // per-channel view parameters, all distinct; sc of both signs; relu6 views reach z < 0 and z > 6
  s.mu.resize(K); s.sc.resize(K); s.be.resize(K); s.rstd.resize(K); s.mdz.resize(K); s.mdzx.resize(K);
  gck::fill_uni(s.mu, seed + 3, 0.3f);
  gck::fill_uni(s.sc, seed + 4, c.act == 2 ? 3.5f : 0.5f, c.act == 2 ? 4.5f : 1.0f);
  for (int k = 0; k < K; ++k) if (k % 3 == 1) s.sc[k] = -s.sc[k];
  gck::fill_uni(s.be, seed + 5, c.act == 2 ? 3.0f : 0.5f, c.act == 2 ? 2.0f : 0.0f);
  gck::fill_uni(s.rstd, seed + 6, 0.5f, 1.0f);
  gck::fill_uni(s.mdz, seed + 7, 0.1f);
  gck::fill_uni(s.mdzx, seed + 8, 0.1f);
  s.mu2.resize(N); s.sc2.resize(N); s.be2.resize(N); s.rstd2.resize(N);
  gck::fill_uni(s.mu2, seed + 9, 0.3f);
  gck::fill_uni(s.sc2, seed + 10, c.act == 2 ? 3.5f : 0.5f, c.act == 2 ? 4.5f : 1.0f);
  for (int n = 0; n < N; ++n) if (n % 3 == 2) s.sc2[n] = -s.sc2[n];
  gck::fill_uni(s.be2, seed + 11, c.act == 2 ? 3.0f : 0.5f, c.act == 2 ? 2.0f : 0.0f);
  gck::fill_uni(s.rstd2, seed + 12, 0.5f, 1.0f);
  if (c.mode == 2) {
    s.rowscale.resize((size_t)cdiv(max_rows, c.rpi) * K);
    gck::fill_uni(s.rowscale, seed + 13, 0.5f, 0.5f);
  }
  put_f(s.dBt, s.Bt); put_f(s.dbias, s.bias); put_f(s.drs, s.rowscale);
  put_f(s.dmu, s.mu); put_f(s.dsc, s.sc); put_f(s.dbe, s.be); put_f(s.drstd, s.rstd);
  put_f(s.dmdz, s.mdz); put_f(s.dmdzx, s.mdzx);
  put_f(s.dmu2, s.mu2); put_f(s.dsc2, s.sc2); put_f(s.dbe2, s.be2); put_f(s.drstd2, s.rstd2);
}

// storage variant of the case: 1 forward on bf16 activations (A, C), 2 gradient view on a bf16 y
static int storage(const Case& c) { return !c.bf16 ? 0 : (c.route == DGRAD ? 2 : 1); }

static void make_member(const Case& c, uint64_t seed, int M, int Pexp, Member& m) {
  const int st = storage(c);
  m.M = M;
  m.Pexp = Pexp;
  m.A.resize((size_t)M * c.K);
  gck::fill_uni(m.A, seed + 21);
  if (st == 1) put_bf(m.dA, m.A);
  else put_f(m.dA, m.A);
  if (c.mode == 3) {
    m.Y.resize((size_t)M * c.K);
    gck::fill_uni(m.Y, seed + 22);
    if (st == 2) put_bf(m.dY, m.Y);
    else put_f(m.dY, m.Y);
  }
  const bool cbf = st == 1;
  const size_t mn = (size_t)M * c.N;
  m.C.alloc(mn * (cbf ? 2 : 4));
  if (c.acc) {
    // (bf16 C: a fill an eighth of the products' scale, see DESIGN.md on the 2^-9 |C| term)
    m.Cprev.resize(mn);
    gck::fill_uni(m.Cprev, seed + 23, cbf ? 0.125f : 1.0f);
    if (cbf) {
      for (size_t i = 0; i < mn; ++i) {
        const uint16_t h = gck::f2bf(m.Cprev[i]);
        m.Cprev[i] = gck::bf2f(h);
        std::memcpy(m.C.fill() + 2 * i, &h, 2);
      }
    } else {
      std::memcpy(m.C.fill(), m.Cprev.data(), mn * 4);
    }
  } else if (cbf) {
    m.C.fill16(0x7fc0);
  } else {
    m.C.fill32(0x7fc00000u);
  }
  if (c.sink == GRAD) {
    m.Y2.resize(mn);
    gck::fill_uni(m.Y2, seed + 24);
    if (st == 2) put_bf(m.dY2, m.Y2);
    else put_f(m.dY2, m.Y2);
  }
  if (c.sink) {
    m.part.alloc((size_t)c.N * Pexp * 8);
    m.part.fill32(gck::kUnwritten);
    m.cnt.alloc((size_t)Pexp * 4);
    m.cnt.fill32(gck::kUnwritten);
  }
}

static gck::Problem problem(const Case& c, const Shared& s, const Member& m) {
  gck::Problem p;
  p.M = m.M; p.N = c.N; p.K = c.K; p.mode = c.mode; p.act = c.act;
  p.bf16 = c.bf16; p.cbf = storage(c) == 1; p.acc = c.acc; p.rpi = c.rpi;
  p.A = m.A.data(); p.Y = m.Y.data(); p.Bt = s.Bt.data();
  p.bias = c.bias ? s.bias.data() : nullptr;
  p.Cprev = m.Cprev.data(); p.rowscale = s.rowscale.data();
  p.mu = s.mu.data(); p.sc = s.sc.data(); p.be = s.be.data();
  p.rstd = s.rstd.data(); p.mdz = s.mdz.data(); p.mdzx = s.mdzx.data();
  return p;
}

static std::vector<float> c_floats(const Case& c, const Member& m) {
  const size_t mn = (size_t)m.M * c.N;
  std::vector<float> out(mn);
  if (storage(c) == 1) {
    for (size_t i = 0; i < mn; ++i) {
      uint16_t h;
      std::memcpy(&h, m.C.out() + 2 * i, 2);
      out[i] = gck::bf2f(h);
    }
  } else {
    std::memcpy(out.data(), m.C.out(), mn * 4);
  }
  return out;
}

static InX view_in(const Case& c, const Shared& s, const Member& m) {
  const bool v = c.mode == 1 || c.mode == 2;
  return InX{m.dA.f(), v ? s.dmu.f() : nullptr, v ? s.dsc.f() : nullptr, v ? s.dbe.f() : nullptr, v ? c.act : 0,
             storage(c) == 1 ? 1 : 0};
}
static GradX view_grad(const Case& c, const Shared& s, const Member& m) {
  if (c.mode != 3) return GradX{m.dA.f(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  return GradX{m.dA.f(), m.dY.f(), s.dmu.f(), s.drstd.f(), s.dsc.f(), s.dbe.f(), s.dmdz.f(), s.dmdzx.f(), c.act,
               storage(c) == 2 ? 1 : 0};
}
static StatSink stat_sink(const Case& c, const Member& m) {
  if (c.sink != STAT) return StatSink{};
  return StatSink{reinterpret_cast<float2*>(m.part.ptr()), m.cnt.ptr(), c.N, 0};
}
static GradSink grad_sink(const Case& c, const Shared& s, const Member& m) {
  if (c.sink != GRAD) return GradSink{};
  return GradSink{reinterpret_cast<float2*>(m.part.ptr()), c.N, 0, m.dY2.f(), s.dmu2.f(), s.drstd2.f(), s.dsc2.f(),
                  s.dbe2.f(), c.act, storage(c) == 2 ? 1 : 0};
}

// checks of one member after a launch that returned P partial rows
static void check_member(const Case& c, const Shared& s, Member& m, int P, Verdict& v) {
  m.C.download();
  v.canary_ok &= m.C.intact();
  const std::vector<float> C = c_floats(c, m);
  const gck::Reference ref = gck::reference(problem(c, s, m));
  const gck::CCheck cc = gck::check_c(ref, C.data(), (long)m.M * c.N);
  gck::SinkCheck sc;
  if (c.sink) {
    m.part.download();
    m.cnt.download();
    v.canary_ok &= m.part.intact() && m.cnt.intact();
    if (P != m.Pexp) {
      v.P_ok = false;  // the partials are laid out with another pitch: not read
    } else if (c.sink == STAT) {
      sc = gck::check_statsink(C.data(), m.M, c.N, reinterpret_cast<const float*>(m.part.out()),
                               reinterpret_cast<const float*>(m.cnt.out()), P);
    } else {
      sc = gck::check_gradsink(C.data(), m.M, c.N, m.Y2.data(), s.mu2.data(), s.rstd2.data(), s.sc2.data(),
                               s.be2.data(), c.act, reinterpret_cast<const float*>(m.part.out()), P);
    }
  }
  merge(v, cc, sc);
}

static Verdict run_case(const Case& c, uint64_t seed, hipStream_t st) {
  Verdict v;
  v.has_sink = c.sink != NONE;
  const int wgs = gemm2_target_wgs();
  const int n = c.nseg ? c.nseg : 1;
  int max_rows = c.M;
  for (int i = 0; i < c.nseg; ++i) max_rows = std::max(max_rows, c.Ms[i]);
  Shared s;
  make_shared(c, seed, max_rows, s);
  if (c.force_wsk) gemm2_force_wsk(c.force_wsk / 10, c.force_wsk % 10);
  std::vector<Member> ms(n);
  for (int i = 0; i < n; ++i) {
    int Pexp = 0;
    if (c.sink) {
      if (c.nseg) {
        Pexp = group_rows(c, i);
      } else if (c.route == SPLIT) {
        const Gemm2Plan p = plan_gemm2(c.M, c.N, c.K, wgs, c.bf16, true, false);
        Pexp = p.splits > 1 ? gemm_splitk_stats_partials(c.M, c.N) : p.P;
      } else if (c.sink == STAT) {
        Pexp = gemm_stat_partials(c.M, c.N, c.K, c.bf16);
      } else {
        Pexp = gemm_dgrad_gsink_partials(c.M, c.N, c.K, c.bf16);
      }
    }
    make_member(c, seed + 100 * i, c.nseg ? c.Ms[i] : c.M, Pexp, ms[i]);
  }
  v.Pexp = ms[0].Pexp;
  Guarded partial;
  partial.alloc(split_floats(c) * 4);
  partial.fill32(0x7fc00000u);

  std::vector<int> Pout(n, 0);
  auto launch = [&]() {
    for (auto& m : ms) {
      m.C.upload();
      if (c.sink) {
        m.part.upload();
        m.cnt.upload();
      }
    }
    partial.upload();
    const float* bias = c.bias ? s.dbias.f() : nullptr;
    if (c.nseg) {
      std::vector<GemmSeg> segs(n);
      int Pmax = 0;
      for (int i = 0; i < n; ++i) {
        segs[i] = GemmSeg{view_in(c, s, ms[i]), view_grad(c, s, ms[i]), bias, ms[i].C.ptr(), ms[i].M, c.acc,
                          stat_sink(c, ms[i]), grad_sink(c, s, ms[i])};
        Pmax = std::max(Pmax, ms[i].Pexp);
      }
      // max_part_rows = the rows the regions hold: the launcher throws before launching if a member
      // would write more
      gemm_group_run(c.mode, segs.data(), n, s.dBt.f(), c.N, c.K, st, c.bf16, Pout.data(), Pmax);
    } else if (c.route == FWD) {
      Pout[0] = launch_gemm(view_in(c, s, ms[0]), s.dBt.f(), bias, ms[0].C.ptr(), c.M, c.N, c.K, c.acc,
                            c.mode == 2 ? s.drs.f() : nullptr, c.rpi, st, partial.ptr(), stat_sink(c, ms[0]), c.bf16);
    } else if (c.route == DGRAD) {
      Pout[0] = launch_gemm_dgrad(view_grad(c, s, ms[0]), s.dBt.f(), ms[0].C.ptr(), c.M, c.N, c.K, c.acc, st,
                                  partial.ptr(), grad_sink(c, s, ms[0]), c.bf16);
    } else {
      Pout[0] = gemm2_run(c.mode, view_in(c, s, ms[0]), GradX{}, s.dBt.f(), bias, ms[0].C.ptr(), c.M, c.N, c.K, c.acc,
                          c.mode == 2 ? s.drs.f() : nullptr, c.rpi, st, partial.ptr(), stat_sink(c, ms[0]), wgs,
                          GradSink{}, c.bf16, false);
    }
    CK(hipStreamSynchronize(st));
    CK(hipGetLastError());
  };
  try {
    launch();
  } catch (const HipError& e) {
    fatal(e.what(), c.name);
  } catch (const std::exception& e) {
    v.threw = true;
    v.what = e.what();
    if (c.force_wsk) gemm2_force_wsk(0, 0);
    return v;
  }
  v.P = Pout[0];
  for (int i = 0; i < n; ++i) check_member(c, s, ms[i], Pout[i], v);
  partial.download();
  v.canary_ok &= partial.intact();
  // repeatability: a second launch from the same initial state leaves the same bits
  std::vector<std::vector<uint8_t>> keep;
  for (auto& m : ms) {
    keep.push_back(m.C.got);
    keep.push_back(m.part.got);
    keep.push_back(m.cnt.got);
  }
  try {
    launch();
  } catch (const HipError& e) {
    fatal(e.what(), c.name);
  } catch (const std::exception& e) {
    v.repeat_ok = false;
  }
  size_t q = 0;
  for (auto& m : ms) {
    m.C.download();
    v.repeat_ok &= m.C.got == keep[q++];
    if (c.sink) {
      m.part.download();
      m.cnt.download();
      v.repeat_ok &= m.part.got == keep[q] && m.cnt.got == keep[q + 1];
    }
    q += 2;
  }
  if (c.force_wsk) gemm2_force_wsk(0, 0);
  return v;
}

// an argument refusal: the launcher throws (not a HIP error) and C stays as it was
static Verdict run_refusal(const Case& c, uint64_t seed, hipStream_t st) {
  Verdict v;
  Shared s;
  make_shared(c, seed, c.M, s);
  const int n = c.nseg ? c.nseg : 1;
  std::vector<Member> ms(n);
  for (int i = 0; i < n; ++i)
    make_member(c, seed + 100 * i, c.nseg ? c.Ms[i] : c.M, c.nseg ? group_rows(c, i) : 8, ms[i]);
  for (auto& m : ms) {
    m.C.upload();
    if (c.sink) {
      m.part.upload();
      m.cnt.upload();
    }
  }
  Guarded partial;
  partial.alloc(16);
  partial.upload();
  const int wgs = gemm2_target_wgs();
  try {
    Member& m = ms[0];
    switch (c.refuse) {
      case R_K4:
      case R_STATS_ACC:
      case R_STATS_N3:
        launch_gemm(view_in(c, s, m), s.dBt.f(), nullptr, m.C.ptr(), c.M, c.N, c.K, c.acc, nullptr, 1, st,
                    partial.ptr(), stat_sink(c, m), false);
        break;
      case R_GSINK_MODE1:
        gemm2_run(1, view_in(c, s, m), GradX{}, s.dBt.f(), nullptr, m.C.ptr(), c.M, c.N, c.K, false, nullptr, 1, st,
                  partial.ptr(), StatSink{}, wgs, grad_sink(c, s, m), false, false);
        break;
      case R_NULL_VIEW: {
        InX a = view_in(c, s, m);
        a.p = nullptr;
        launch_gemm(a, s.dBt.f(), nullptr, m.C.ptr(), c.M, c.N, c.K, false, nullptr, 1, st, partial.ptr(), StatSink{},
                    false);
        break;
      }
      case R_GROUP_ROWS: {
        std::vector<GemmSeg> segs(n);
        int Pmax = 0;
        for (int i = 0; i < n; ++i) {
          segs[i] = GemmSeg{view_in(c, s, ms[i]), view_grad(c, s, ms[i]), s.dbias.f(), ms[i].C.ptr(), ms[i].M, false,
                            stat_sink(c, ms[i]), grad_sink(c, s, ms[i])};
          Pmax = std::max(Pmax, ms[i].Pexp);
        }
        gemm_group_run(c.mode, segs.data(), n, s.dBt.f(), c.N, c.K, st, false, nullptr, Pmax - 1);
        break;
      }
    }
  } catch (const HipError& e) {
    fatal(e.what(), c.name);
  } catch (const std::exception& e) {
    v.threw = true;
    v.what = e.what();
  }
  CK(hipStreamSynchronize(st));
  CK(hipGetLastError());
  // nothing was launched: every output still holds its fill
  for (auto& m : ms) {
    m.C.download();
    v.repeat_ok &= m.C.got == m.C.init;
    if (c.sink) {
      m.part.download();
      m.cnt.download();
      v.repeat_ok &= m.part.got == m.part.init && m.cnt.got == m.cnt.init;
    }
  }
  return v;
}

int main(int argc, char** argv) {
  const std::vector<Case> t = table();
  if (argc > 1 && std::string(argv[1]) == "--plan") {
    for (const Case& c : t) print_plan(c, stdout);
    printf("{\"done\":true,\"cases\":%zu}\n", t.size());
    return 0;
  }
  if (argc > 4 && std::string(argv[1]) == "--shape") {
    const bool bf = argc > 5 && atoi(argv[5]);
    for (Route r : {FWD, SPLIT}) {
      Case c{"shape", "", r, atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0, 0, false, false, NONE, bf};
      print_plan(c, stdout);
    }
    return 0;
  }
  if (argc > 1) {
    fprintf(stderr, "usage: gemm_parity [--plan | --shape M N K [bf16]]\n");
    return 2;
  }
  hipStream_t st;
  CK(hipStreamCreate(&st));
  size_t ran = 0, passed = 0;
  for (size_t i = 0; i < t.size(); ++i) {
    const Case& c = t[i];
    g_case = c.name;
    const Path p = path_of(c);
    const bool refuse = c.route == REFUSE;
    const Verdict v = refuse ? run_refusal(c, 1000 + 50 * i, st) : run_case(c, 1000 + 50 * i, st);
    bool ok;
    std::string line = std::string("{\"case\":\"") + c.name + "\",\"path\":\"" + p.path + "\"";
    if (refuse) {
      ok = v.threw && v.repeat_ok;
      line += std::string(",\"threw\":") + (v.threw ? "true" : "false") + ",\"untouched\":" +
              (v.repeat_ok ? "true" : "false") + ",\"what\":\"" + esc(v.what) + "\"";
    } else {
      ok = !v.threw && v.c.ratio <= 1.0 && v.c.nonfinite == 0 && v.canary_ok && v.repeat_ok;
      if (v.has_sink)
        ok = ok && v.P_ok && v.s.rows_written && v.s.sum_ratio <= 1.0 && v.s.m2_ratio <= 1.0 &&
             (c.sink != STAT || (v.s.cnt_ok && v.s.cnt_sum_ok));
      line += std::string(",\"threw\":") + (v.threw ? "true" : "false");
      if (v.threw) line += ",\"what\":\"" + esc(v.what) + "\"";
      line += ",\"c_ratio\":" + num(v.c.ratio) + ",\"c_nonfinite\":" + std::to_string(v.c.nonfinite) +
              ",\"c_worst\":" + std::to_string(v.c.worst) + ",\"c_worst_err\":" + num(v.c.worst_err) +
              ",\"c_worst_bound\":" + num(v.c.worst_bound) + ",\"canary_ok\":" + (v.canary_ok ? "true" : "false") +
              ",\"repeat_ok\":" + (v.repeat_ok ? "true" : "false") + ",\"sink\":" + std::to_string(c.sink);
      if (v.has_sink)
        line += ",\"P\":" + std::to_string(v.P) + ",\"P_expected\":" + std::to_string(v.Pexp) +
                ",\"P_ok\":" + (v.P_ok ? "true" : "false") + ",\"rows_written\":" + (v.s.rows_written ? "true" : "false") +
                ",\"cnt_ok\":" + (v.s.cnt_ok ? "true" : "false") + ",\"cnt_sum_ok\":" +
                (v.s.cnt_sum_ok ? "true" : "false") + ",\"sum_ratio\":" + num(v.s.sum_ratio) +
                ",\"m2_ratio\":" + num(v.s.m2_ratio);
    }
    line += std::string(",\"pass\":") + (ok ? "true" : "false") + "}";
    puts(line.c_str());
    fflush(stdout);
    ++ran;
    passed += ok;
  }
  CK(hipStreamDestroy(st));
  printf("{\"done\":true,\"cases\":%zu,\"ran\":%zu,\"passed\":%zu}\n", t.size(), ran, passed);
  fflush(stdout);
  return 0;
}
