// norm_parity — kernel-level parity of kernels_norm.hip (BN statistics and finalizes, BN backward
// reductions, the bn=sync sum halves, squeeze-excite, residual add / gradient copy with their GradSink,
// max-pool and nearest upsample) against an fp64 host reference.
//
//   norm_parity --plan   the case table with each case's reduction geometry (red_plan_info), SE plan
//                        (se_plan_info), expected partial count, tensor bytes and the share of elements
//                        under a kink / tie allowance (host code only: runs without a GPU)
//   norm_parity          run the table on the GPU: one flushed JSON line per case, then a `done` line
//
// Only the launchers of kernels.hpp are called, on one stream.  The PHX_RED_* knobs are read once per
// process by the library; the table is chosen for their defaults and the first line says whether they
// are unset.  The exit status is 0 when every case ran (the verdicts are in the lines); a HIP error ends
// the process at once with a `fatal` line and status 3.  Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "norm_check.hpp"
#include "parity_dev.hpp"

using namespace phx;
using gck::kEps24;
using nck::Field;

// ---- the case table ----------------------------------------------------------------------------
enum Op { STATS, STATS_SUMS, BRED, BRED_SUMS, BN_BWD, FIN, BFIN, FOLD, SE_FWD, SE_BWD, POOL, UPS, ADD, COPYG, GSUMS, APPLY, APPLY2, BF2F, DROPK, CKSUM, MOVAPPLY, FROZEN, FUSE_F, FUSE_B, REFUSE };
static const char* kOpName[] = {"bn_stats", "bn_stats_sums", "bn_bwd_reduce", "bn_bwd_reduce_sums", "bn_bwd",
                                "bn_finalize", "bn_bwd_finalize", "bn_fold_from_sums", "se_fwd", "se_bwd", "maxpool",
                                "upsample", "add", "copy_grad", "grad_sums", "bn_apply", "bn_bwd_apply2", "bf16_to_f32",
                                "drop_keep", "cksum", "bn_moving_apply", "bn_frozen_stats", "fuse_fwd", "fuse_bwd", "refuse"};
enum Refuse {
  R_NONE = 0, R_STATS_C4, R_SUMS_C4, R_BRED_C4, R_APPLY_C4, R_BWD_C4, R_APPLY2_C4, R_GRP0, R_GRP6, R_BGRP6, R_FOLD0,
  R_SE_N, R_SEB_N, R_ADD_MIXED, R_ADD_C4, R_COPY_C4, R_COPY_TAIL, R_GSUMS_C4, R_LAST
};

struct Case {
  const char* name = "";
  Op op = STATS;
  int B = 1;     // images (SE, resampling, drop connect); members of a finalize group
  long M = 1;    // rows (per image for SE / elementwise)
  int C = 8, N = 0;
  int bf = 0, act = 0, flav = 0, view = 0;
  int P = 0;
  int H = 0, W = 0, Ho = 0, Wo = 0, k = 3, s = 2;
  bool acc = false;
  int sink = 0;  // 2: GradSink
  int drop = 0;  // 0 off, 1 p = 1, 2 p = 0.8, 3 p = 2^-6 + 2^-9
  int refuse = R_NONE;
};

static std::vector<Case> table() {
  std::vector<Case> t;
  // column reductions over [M][C].  flav (bn_stats): 0 no moving statistics, 1 moving, 2 deferred side
  // pairs; (bn_bwd): 1 frozen.  Every bn_stats input has a channel at 1e3 x its spread and a constant one.
  auto red = [&](const char* name, Op op, long M, int C, int bf, int act, int flav, bool acc = false) {
    Case c;
    c.name = name; c.op = op; c.M = M; c.C = C; c.bf = bf; c.act = act; c.flav = flav; c.acc = acc;
    t.push_back(c);
  };
  // finalizes from synthetic partials: B members (1: the plain launcher), P partials for the first
  // (member i: P - 37 i, at least 1).  flav & 1: partials with cnt == 0 holding NaN; flav & 2: side pairs
  auto fin = [&](const char* name, Op op, int P, int flav, int members = 1, int C = 8) {
    Case c;
    c.name = name; c.op = op; c.P = P; c.flav = flav; c.B = members; c.C = C;
    t.push_back(c);
  };
  // squeeze-excite.  view: 0 raw x, 1 BN + swish view, 2 BN + relu6 view
  auto se = [&](const char* name, Op op, int B, int HW, int C, int N, int view, int bf, bool acc = false, int sink = 0) {
    Case c;
    c.name = name; c.op = op; c.B = B; c.M = HW; c.C = C; c.N = N; c.view = view; c.bf = bf; c.acc = acc; c.sink = sink;
    c.act = 1;
    t.push_back(c);
  };
  // max-pool forward + backward.  flav: 0 raw, 1 raw in eighths (exact ties), 2 relu6 view saturated
  // beyond -1 and 7 (exact ties whatever the rounding), 3 swish view
  auto pool = [&](const char* name, int B, int H, int W, int C, int k, int s, int flav, int bf, bool acc) {
    Case c;
    c.name = name; c.op = POOL; c.B = B; c.H = H; c.W = W; c.C = C; c.k = k; c.s = s; c.flav = flav; c.bf = bf; c.acc = acc;
    t.push_back(c);
  };
  auto ups = [&](const char* name, int B, int H, int Ho, int C, int view, int bf, bool acc, int W = 0, int Wo = 0) {
    Case c;
    c.name = name; c.op = UPS; c.B = B; c.H = H; c.W = W ? W : H; c.Ho = Ho; c.Wo = Wo ? Wo : Ho; c.C = C; c.view = view;
    c.bf = bf; c.acc = acc;
    t.push_back(c);
  };
  // residual add / gradient copy / gradient sums over B images of M rows
  auto ew = [&](const char* name, Op op, int B, long rows, int C, int view, int bf, bool acc, int sink, int drop) {
    Case c;
    c.name = name; c.op = op; c.B = B; c.M = rows; c.C = C; c.view = view; c.bf = bf; c.acc = acc; c.sink = sink;
    c.drop = drop; c.act = view == 2 ? 2 : 1;
    t.push_back(c);
  };
  // the remaining elementwise launchers over [M][C]
  auto misc = [&](const char* name, Op op, long M, int C, int act, int bf, int flav = 0) {
    Case c;
    c.name = name; c.op = op; c.M = M; c.C = C; c.act = act; c.bf = bf; c.flav = flav;
    t.push_back(c);
  };
  // BiFPN fuse over [M][C]: N inputs, method k (0 fastattn, 1 sum).  flav: 0 positive weights, 1 the second
  // negative, 2 the first zero, 3 all zero (the denominator is 1e-4); backward: P = bit mask of the inputs
  // that take a gradient, s = bit mask of those that accumulate
  auto fuse = [&](const char* name, Op op, long M, int C, int nin, int method, int act, int flav, int bf, int take = 7,
                  int accm = 0) {
    Case c;
    c.name = name; c.op = op; c.M = M; c.C = C; c.N = nin; c.k = method; c.act = act; c.flav = flav; c.bf = bf; c.P = take;
    c.s = accm;
    t.push_back(c);
  };
  auto ref = [&](const char* name, int refuse) {
    Case c;
    c.name = name; c.op = REFUSE; c.refuse = refuse;
    t.push_back(c);
  };

  // a. launch_bn_stats: C 4 .. 2688 (tpr 1, 2, 10, 36, 60, 168, 256 + 32, 256 + 256 + 160), M at the lane
  // and chunk edges of each geometry (--plan prints them)
  red("st_c4_m1", STATS, 1, 4, 0, 0, 1);
  red("st_c4_m255", STATS, 255, 4, 0, 0, 0);
  red("st_c4_m257_side", STATS, 257, 4, 0, 0, 2);
  red("st_c4_m2049", STATS, 2049, 4, 0, 0, 1);
  red("st_c4_m34817", STATS, 34817, 4, 0, 0, 1);
  red("st_c8_m127", STATS, 127, 8, 0, 0, 1);
  red("st_c8_m129_bf", STATS, 129, 8, 1, 0, 1);
  red("st_c8_m1025_side", STATS, 1025, 8, 0, 0, 2);
  red("st_c40_m24", STATS, 24, 40, 0, 0, 1);
  red("st_c40_m26", STATS, 26, 40, 0, 0, 0);
  red("st_c40_m199_bf", STATS, 199, 40, 1, 0, 1);
  red("st_c40_m201", STATS, 201, 40, 0, 0, 1);
  red("st_c40_m3201", STATS, 3201, 40, 0, 0, 1);
  red("st_c144_m6", STATS, 6, 144, 0, 0, 1);
  red("st_c144_m8", STATS, 8, 144, 0, 0, 2);
  red("st_c144_m55_bf", STATS, 55, 144, 1, 0, 1);
  red("st_c144_m57", STATS, 57, 144, 0, 0, 1);
  red("st_c144_m953", STATS, 953, 144, 0, 0, 1);
  red("st_c240_m3", STATS, 3, 240, 0, 0, 1);
  red("st_c240_m5", STATS, 5, 240, 0, 0, 0);
  red("st_c240_m33", STATS, 33, 240, 0, 0, 1);
  red("st_c240_m545_bf", STATS, 545, 240, 1, 0, 2);
  red("st_c672_m1", STATS, 1, 672, 0, 0, 1);
  red("st_c672_m8", STATS, 8, 672, 0, 0, 1);
  red("st_c672_m9", STATS, 9, 672, 0, 0, 0);
  red("st_c672_m128", STATS, 128, 672, 0, 0, 1);
  red("st_c672_m129_bf", STATS, 129, 672, 1, 0, 1);
  red("st_c672_m385", STATS, 385, 672, 0, 0, 2);
  red("st_c672_m392", STATS, 392, 672, 0, 0, 1);
  red("st_c672_m521", STATS, 521, 672, 0, 0, 1);
  red("st_c1152_m1", STATS, 1, 1152, 0, 0, 1);
  red("st_c1152_m9", STATS, 9, 1152, 0, 0, 1);
  red("st_c1152_m131_bf", STATS, 131, 1152, 1, 0, 2);
  red("st_c2688_m1", STATS, 1, 2688, 0, 0, 1);
  red("st_c2688_m7", STATS, 7, 2688, 0, 0, 0);
  red("st_c2688_m137", STATS, 137, 2688, 0, 0, 1);
  // b. launch_bn_stats_sums: the un-shifting, at the same geometries
  red("ss_c4_m257", STATS_SUMS, 257, 4, 0, 0, 0);
  red("ss_c8_m1025_bf", STATS_SUMS, 1025, 8, 1, 0, 0);
  red("ss_c40_m201", STATS_SUMS, 201, 40, 0, 0, 0);
  red("ss_c144_m57", STATS_SUMS, 57, 144, 0, 0, 0);
  red("ss_c240_m33_bf", STATS_SUMS, 33, 240, 1, 0, 0);
  red("ss_c672_m521", STATS_SUMS, 521, 672, 0, 0, 0);
  red("ss_c1152_m131", STATS_SUMS, 131, 1152, 0, 0, 0);
  red("ss_c2688_m7", STATS_SUMS, 7, 2688, 0, 0, 0);
  // c. launch_bn_bwd_reduce (two operands per row), activations none / swish / relu6
  red("br_c4_m1_swish", BRED, 1, 4, 0, 1, 0);
  red("br_c4_m257_relu6", BRED, 257, 4, 0, 2, 0);
  red("br_c4_m2049_none", BRED, 2049, 4, 0, 0, 0);
  red("br_c8_m129_swish_bf", BRED, 129, 8, 1, 1, 0);
  red("br_c40_m26_relu6", BRED, 26, 40, 0, 2, 0);
  red("br_c40_m201_swish", BRED, 201, 40, 0, 1, 0);
  red("br_c144_m6_none", BRED, 6, 144, 0, 0, 0);
  red("br_c144_m57_swish_bf", BRED, 57, 144, 1, 1, 0);
  red("br_c144_m953_relu6", BRED, 953, 144, 0, 2, 0);
  red("br_c240_m5_swish", BRED, 5, 240, 0, 1, 0);
  red("br_c240_m545_relu6_bf", BRED, 545, 240, 1, 2, 0);
  red("br_c672_m9_swish", BRED, 9, 672, 0, 1, 0);
  red("br_c672_m128_swish", BRED, 128, 672, 0, 1, 0);
  red("br_c672_m129_relu6", BRED, 129, 672, 0, 2, 0);
  red("br_c672_m392_swish", BRED, 392, 672, 0, 1, 0);
  red("br_c672_m521_none", BRED, 521, 672, 0, 0, 0);
  red("br_c1152_m9_swish", BRED, 9, 1152, 0, 1, 0);
  red("br_c1152_m131_relu6", BRED, 131, 1152, 0, 2, 0);
  red("br_c2688_m7_swish", BRED, 7, 2688, 0, 1, 0);
  red("br_c2688_m137_relu6_bf", BRED, 137, 2688, 1, 2, 0);
  // d. launch_bn_bwd_reduce_sums
  red("bs_c8_m129_swish", BRED_SUMS, 129, 8, 0, 1, 0);
  red("bs_c144_m57_relu6_bf", BRED_SUMS, 57, 144, 1, 2, 0);
  red("bs_c672_m521_swish", BRED_SUMS, 521, 672, 0, 1, 0);
  red("bs_c1152_m131_none", BRED_SUMS, 131, 1152, 0, 0, 0);
  // e. launch_bn_bwd: the unfused reduce + apply (and its frozen form)
  red("bb_c4_m257_swish", BN_BWD, 257, 4, 0, 1, 0);
  red("bb_c40_m201_relu6_acc", BN_BWD, 201, 40, 0, 2, 0, true);
  red("bb_c144_m57_none", BN_BWD, 57, 144, 0, 0, 0);
  red("bb_c672_m129_swish_acc", BN_BWD, 129, 672, 0, 1, 0, true);
  red("bb_c1152_m9_relu6", BN_BWD, 9, 1152, 0, 2, 0);
  red("bb_c40_m201_swish_frozen", BN_BWD, 201, 40, 0, 1, 1);
  red("bb_c144_m8_relu6_frozen_acc", BN_BWD, 8, 144, 0, 2, 1, true);

  // f. k_bn_finalize from synthetic partials: P at the 1024-stride body's and the remainders' edges
  fin("fin_p1", FIN, 1, 0);
  fin("fin_p2", FIN, 2, 0);
  fin("fin_p255", FIN, 255, 0);
  fin("fin_p256", FIN, 256, 2);
  fin("fin_p257", FIN, 257, 1);
  fin("fin_p768", FIN, 768, 0);
  fin("fin_p769", FIN, 769, 1);
  fin("fin_p1024", FIN, 1024, 0);
  fin("fin_p1025", FIN, 1025, 1);
  fin("fin_p1800_zero_side", FIN, 1800, 3);
  fin("fin_p2049_c40", FIN, 2049, 1, 1, 40);
  fin("fin_group2", FIN, 300, 1, 2);
  fin("fin_group5", FIN, 1100, 1, 5);
  fin("fin_group5_side", FIN, 160, 3, 5);
  fin("bfin_p1", BFIN, 1, 0);
  fin("bfin_p2", BFIN, 2, 0);
  fin("bfin_p255", BFIN, 255, 0);
  fin("bfin_p256", BFIN, 256, 0);
  fin("bfin_p257", BFIN, 257, 0);
  fin("bfin_p768", BFIN, 768, 0);
  fin("bfin_p769", BFIN, 769, 0);
  fin("bfin_p1024", BFIN, 1024, 0);
  fin("bfin_p1025", BFIN, 1025, 0);
  fin("bfin_p1800", BFIN, 1800, 0);
  fin("bfin_group2", BFIN, 300, 0, 2);
  fin("bfin_group5", BFIN, 1100, 0, 5);
  // g. from_sums(fold_sums(x)) == finalize(x), bit for bit (one world)
  fin("fold_p1", FOLD, 1, 0);
  fin("fold_p257_zero", FOLD, 257, 1);
  fin("fold_p1025_zero", FOLD, 1025, 1);
  fin("fold_p1800_c40", FOLD, 1800, 0, 1, 40);

  // h. launch_se_fwd: D0's (C, Cse) pairs and one D4 pair; B 1, 2, 3, 16 and 300 (s1 = 1); HW 1, 4, 49,
  // 288 (one row past the 8-deep body) and enough chunks for both fold bodies
  se("sef_c32_n8_b2_hw49", SE_FWD, 2, 49, 32, 8, 1, 0);
  se("sef_c32_n8_b1_hw1_raw", SE_FWD, 1, 1, 32, 8, 0, 0);
  se("sef_c32_n8_b16_hw288", SE_FWD, 16, 288, 32, 8, 1, 0);
  se("sef_c32_n8_b300_hw4", SE_FWD, 300, 4, 32, 8, 1, 0);
  se("sef_c96_n4_b1_hw9121", SE_FWD, 1, 9121, 96, 4, 0, 0);
  se("sef_c96_n4_b3_hw49_relu6", SE_FWD, 3, 49, 96, 4, 2, 0);
  se("sef_c96_n4_b1_hw4_bf", SE_FWD, 1, 4, 96, 4, 1, 1);
  se("sef_c144_n6_b2_hw49", SE_FWD, 2, 49, 144, 6, 1, 0);
  se("sef_c144_n6_b1_hw1700", SE_FWD, 1, 1700, 144, 6, 1, 0);
  se("sef_c240_n10_b3_hw49_bf", SE_FWD, 3, 49, 240, 10, 1, 1);
  se("sef_c240_n10_b16_hw4", SE_FWD, 16, 4, 240, 10, 0, 0);
  se("sef_c480_n20_b2_hw49", SE_FWD, 2, 49, 480, 20, 1, 0);
  se("sef_c480_n20_b1_hw300", SE_FWD, 1, 300, 480, 20, 1, 0);
  se("sef_c672_n28_b1_hw49", SE_FWD, 1, 49, 672, 28, 1, 0);
  se("sef_c672_n28_b3_hw1", SE_FWD, 3, 1, 672, 28, 1, 0);
  se("sef_c672_n28_b1_hw700", SE_FWD, 1, 700, 672, 28, 0, 0);
  se("sef_c1152_n48_b2_hw49", SE_FWD, 2, 49, 1152, 48, 1, 0);
  se("sef_c1152_n48_b1_hw4_relu6", SE_FWD, 1, 4, 1152, 48, 2, 0);
  se("sef_c1152_n48_b16_hw1", SE_FWD, 16, 1, 1152, 48, 1, 0);
  se("sef_c2688_n112_b4_hw49", SE_FWD, 4, 49, 2688, 112, 1, 0);
  se("sef_c2688_n112_b4_hw4_bf", SE_FWD, 4, 4, 2688, 112, 1, 1);
  se("sef_c1152_n48_b64_hw4", SE_FWD, 64, 4, 1152, 48, 1, 0);
  se("sef_c1152_n48_b64_hw49_bf", SE_FWD, 64, 49, 1152, 48, 0, 1);
  se("sef_c2688_n112_b128_hw1", SE_FWD, 128, 1, 2688, 112, 1, 0);
  // i. launch_se_bwd, with and without GradSink and accumulation
  se("seb_c32_n8_b2_hw49_gs", SE_BWD, 2, 49, 32, 8, 1, 0, false, 2);
  se("seb_c32_n8_b1_hw1_raw", SE_BWD, 1, 1, 32, 8, 0, 0);
  se("seb_c32_n8_b16_hw288_gs_acc", SE_BWD, 16, 288, 32, 8, 1, 0, true, 2);
  se("seb_c32_n8_b300_hw4", SE_BWD, 300, 4, 32, 8, 1, 0);
  se("seb_c96_n4_b1_hw9121", SE_BWD, 1, 9121, 96, 4, 0, 0);
  se("seb_c96_n4_b3_hw49_relu6_gs", SE_BWD, 3, 49, 96, 4, 2, 0, false, 2);
  se("seb_c144_n6_b2_hw49_acc", SE_BWD, 2, 49, 144, 6, 1, 0, true);
  se("seb_c144_n6_b1_hw1700_gs", SE_BWD, 1, 1700, 144, 6, 1, 0, false, 2);
  se("seb_c240_n10_b3_hw49_bf_gs", SE_BWD, 3, 49, 240, 10, 1, 1, false, 2);
  se("seb_c480_n20_b2_hw49_gs_acc", SE_BWD, 2, 49, 480, 20, 1, 0, true, 2);
  se("seb_c672_n28_b1_hw49_gs", SE_BWD, 1, 49, 672, 28, 1, 0, false, 2);
  se("seb_c672_n28_b1_hw700", SE_BWD, 1, 700, 672, 28, 0, 0);
  se("seb_c1152_n48_b2_hw49_gs", SE_BWD, 2, 49, 1152, 48, 1, 0, false, 2);
  se("seb_c1152_n48_b16_hw1", SE_BWD, 16, 1, 1152, 48, 1, 0);
  se("seb_c2688_n112_b4_hw49_gs_acc", SE_BWD, 4, 49, 2688, 112, 1, 0, true, 2);
  se("seb_c2688_n112_b4_hw4_bf", SE_BWD, 4, 4, 2688, 112, 1, 1);
  se("seb_c1152_n48_b64_hw4_gs", SE_BWD, 64, 4, 1152, 48, 1, 0, false, 2);
  se("seb_c2688_n112_b128_hw1", SE_BWD, 128, 1, 2688, 112, 1, 0);

  // j. max-pool, quad (C % 4 == 0) and scalar forms
  pool("mp_3s2_1x1_c4", 2, 1, 1, 4, 3, 2, 0, 0, false);
  pool("mp_3s2_2x2_c64_eighths", 2, 2, 2, 64, 3, 2, 1, 0, false);
  pool("mp_3s2_8x8_c64_eighths_acc", 2, 8, 8, 64, 3, 2, 1, 0, true);
  pool("mp_3s2_9x7_c4_raw", 2, 9, 7, 4, 3, 2, 0, 0, false);
  pool("mp_3s2_9x7_c64_relu6_sat", 2, 9, 7, 64, 3, 2, 2, 0, true);
  pool("mp_3s2_8x8_c64_swish", 2, 8, 8, 64, 3, 2, 3, 0, false);
  pool("mp_3s2_9x7_c64_bf_eighths", 2, 9, 7, 64, 3, 2, 1, 1, false);
  pool("mp_3s2_8x8_c64_bf_swish", 2, 8, 8, 64, 3, 2, 3, 1, false);
  pool("mp_2s2_8x8_c64_eighths", 2, 8, 8, 64, 2, 2, 1, 0, false);
  pool("mp_2s2_9x7_c4_raw_acc", 2, 9, 7, 4, 2, 2, 0, 0, true);
  pool("mp_3s2_1x1_c3", 2, 1, 1, 3, 3, 2, 0, 0, false);
  pool("mp_3s2_2x2_c6_eighths", 2, 2, 2, 6, 3, 2, 1, 0, false);
  pool("mp_3s2_9x7_c3_eighths_acc", 2, 9, 7, 3, 3, 2, 1, 0, true);
  pool("mp_3s2_8x8_c6_relu6_sat", 2, 8, 8, 6, 3, 2, 2, 0, false);
  pool("mp_3s2_9x7_c6_swish", 2, 9, 7, 6, 3, 2, 3, 0, false);
  pool("mp_3s2_9x7_c3_bf_eighths", 2, 9, 7, 3, 3, 2, 1, 1, false);
  pool("mp_2s2_8x8_c6_raw", 2, 8, 8, 6, 2, 2, 0, 0, false);
  // k. nearest upsample, integer and non-integer ratios and the identity
  ups("up_1to2_c64", 2, 1, 2, 64, 0, 0, false);
  ups("up_5to10_c64_swish", 2, 5, 10, 64, 1, 0, false);
  ups("up_3to5_c64_acc", 2, 3, 5, 64, 0, 0, true);
  ups("up_3to5_c4_bf", 2, 3, 5, 4, 0, 1, false);
  ups("up_2to3_c64_relu6", 2, 2, 3, 64, 2, 0, false);
  ups("up_7to10_c64", 2, 7, 10, 64, 0, 0, false);
  ups("up_7to10_c4_acc", 2, 7, 10, 4, 0, 0, true);
  ups("up_id_8_c64", 2, 8, 8, 64, 0, 0, false);
  ups("up_3x7_to_5x10_c64", 2, 3, 5, 64, 0, 0, false, 7, 10);
  ups("up_1to2_c3", 2, 1, 2, 3, 0, 0, false);
  ups("up_5to10_c6_swish", 2, 5, 10, 6, 1, 0, false);
  ups("up_3to5_c3_acc", 2, 3, 5, 3, 0, 0, true);
  ups("up_3to5_c6_bf", 2, 3, 5, 6, 0, 1, false);
  ups("up_2to3_c6", 2, 2, 3, 6, 0, 0, false);
  ups("up_7to10_c3_acc", 2, 7, 10, 3, 0, 0, true);
  ups("up_id_8_c6", 2, 8, 8, 6, 0, 0, false);

  // l. residual add (view: 0 raw + raw, 1 BN swish + raw, 2 BN relu6 + BN)
  ew("add_c4_r37_raw", ADD, 3, 37, 4, 0, 0, false, 0, 0);
  ew("add_c40_r37_swish_drop08", ADD, 3, 37, 40, 1, 0, false, 0, 2);
  ew("add_c144_r7_relu6_drop1", ADD, 4, 7, 144, 2, 0, false, 0, 1);
  ew("add_c672_r5_bf_swish_dropsmall", ADD, 3, 5, 672, 1, 1, false, 0, 3);
  ew("add_c8_r1_bf_raw", ADD, 1, 1, 8, 0, 1, false, 0, 0);
  ew("add_c2688_r3_swish_drop08", ADD, 2, 3, 2688, 1, 0, false, 0, 2);
  // m. gradient copy: the plain kernel, and ew_gstats (D = 4 body + tail) with the GradSink
  ew("cg_c4_r37", COPYG, 3, 37, 4, 0, 0, false, 0, 0);
  ew("cg_c40_r37_acc_drop08", COPYG, 3, 37, 40, 0, 0, true, 0, 2);
  ew("cg_c144_r7_dropsmall", COPYG, 4, 7, 144, 0, 0, false, 0, 3);
  ew("cg_c4_r427_gs_swish", COPYG, 3, 427, 4, 1, 0, false, 2, 0);
  ew("cg_c8_r213_gs_relu6_acc_drop08", COPYG, 3, 213, 8, 2, 0, true, 2, 2);
  ew("cg_c40_r42_gs_swish_drop1", COPYG, 3, 42, 40, 1, 0, false, 2, 1);
  ew("cg_c144_r12_gs_swish_bf_drop08", COPYG, 3, 12, 144, 1, 1, false, 2, 2);
  ew("cg_c240_r7_gs_relu6_acc", COPYG, 3, 7, 240, 2, 0, true, 2, 0);
  ew("cg_c672_r43_gs_swish_dropsmall", COPYG, 3, 43, 672, 1, 0, false, 2, 3);
  ew("cg_c1152_r3_gs_swish_drop08", COPYG, 3, 3, 1152, 1, 0, false, 2, 2);
  ew("cg_c2688_r5_gs_relu6", COPYG, 3, 5, 2688, 2, 0, false, 2, 0);
  ew("gsum_c8_r213_swish", GSUMS, 3, 213, 8, 1, 0, false, 2, 0);
  ew("gsum_c144_r12_relu6_bf", GSUMS, 3, 12, 144, 2, 1, false, 2, 0);
  ew("gsum_c672_r43_swish", GSUMS, 3, 43, 672, 1, 0, false, 2, 0);

  // n. bn_apply, the materialised gradient view, the widening copy, keep flags, checksum, moving
  // statistics, frozen statistics
  misc("ap_c4_m37_swish", APPLY, 37, 4, 1, 0);
  misc("ap_c144_m9_relu6", APPLY, 9, 144, 2, 0);
  misc("ap_c672_m3_none", APPLY, 3, 672, 0, 0);
  misc("ap2_c4_m37_swish", APPLY2, 37, 4, 1, 0);
  misc("ap2_c40_m65_relu6", APPLY2, 65, 40, 2, 0);
  misc("ap2_c144_m9_swish_ybf", APPLY2, 9, 144, 1, 1);
  misc("ap2_c672_m3_relu6_ybf", APPLY2, 3, 672, 2, 1);
  misc("ap2_c40_m7_passthrough", APPLY2, 7, 40, 0, 0, 1);
  misc("b2f_n1", BF2F, 1, 1, 0, 1);
  misc("b2f_n257", BF2F, 257, 1, 0, 1);
  misc("b2f_n100003", BF2F, 100003, 1, 0, 1);
  misc("dropk_golden", DROPK, 1, 1, 0, 0);
  misc("ck_n3", CKSUM, 3, 1, 0, 0);
  misc("ck_n70001", CKSUM, 70001, 1, 0, 0);
  misc("ck_n600001_grid_capped", CKSUM, 600001, 1, 0, 0);
  misc("mov_one_pass", MOVAPPLY, 1, 300, 0, 0, 0);
  misc("mov_two_pass", MOVAPPLY, 1, 300, 0, 0, 1);
  misc("frozen_c4", FROZEN, 1, 4, 0, 0);
  misc("frozen_c300", FROZEN, 1, 300, 0, 0);
  // o. BiFPN fuse
  fuse("ff_c64_n2_m0_swish", FUSE_F, 37, 64, 2, 0, 1, 0, 0);
  fuse("ff_c64_n3_m0_relu6_neg", FUSE_F, 37, 64, 3, 0, 2, 1, 0);
  fuse("ff_c64_n3_m1_swish", FUSE_F, 37, 64, 3, 1, 1, 0, 0);
  fuse("ff_c64_n2_m1_relu6_bf", FUSE_F, 37, 64, 2, 1, 2, 0, 1);
  fuse("ff_c6_n3_m0_swish_zero", FUSE_F, 37, 6, 3, 0, 1, 2, 0);
  fuse("ff_c6_n2_m0_relu6_allzero", FUSE_F, 37, 6, 2, 0, 2, 3, 0);
  fuse("ff_c3_n3_m0_swish_bf", FUSE_F, 37, 3, 3, 0, 1, 0, 1);
  fuse("fb_c64_n2_m0_swish", FUSE_B, 37, 64, 2, 0, 1, 0, 0, 3, 0);
  fuse("fb_c64_n3_m0_relu6_neg_acc", FUSE_B, 37, 64, 3, 0, 2, 1, 0, 7, 5);
  fuse("fb_c64_n3_m1_swish_null", FUSE_B, 37, 64, 3, 1, 1, 0, 0, 5, 4);
  fuse("fb_c64_n2_m1_relu6_bf", FUSE_B, 37, 64, 2, 1, 2, 0, 1, 3, 1);
  fuse("fb_c64_n3_m0_swish_allzero", FUSE_B, 37, 64, 3, 0, 1, 3, 0, 7, 2);
  fuse("fb_c6_n3_m0_swish_zero_acc", FUSE_B, 37, 6, 3, 0, 1, 2, 0, 7, 3);
  fuse("fb_c6_n2_m0_relu6_null", FUSE_B, 37, 6, 2, 0, 2, 0, 0, 2, 0);
  fuse("fb_c3_n3_m1_relu6_bf_acc", FUSE_B, 37, 3, 3, 1, 2, 0, 1, 7, 7);

  // p. argument refusals: the launcher throws, nothing is launched, every buffer keeps its fill
  ref("refuse_stats_c_mod4", R_STATS_C4);
  ref("refuse_stats_sums_c_mod4", R_SUMS_C4);
  ref("refuse_bwd_reduce_c_mod4", R_BRED_C4);
  ref("refuse_bn_apply_c_mod4", R_APPLY_C4);
  ref("refuse_bn_bwd_c_mod4", R_BWD_C4);
  ref("refuse_bn_bwd_apply2_c_mod4", R_APPLY2_C4);
  ref("refuse_finalize_group_0", R_GRP0);
  ref("refuse_finalize_group_6", R_GRP6);
  ref("refuse_bwd_finalize_group_6", R_BGRP6);
  ref("refuse_fold_sums_0", R_FOLD0);
  ref("refuse_se_fwd_cse_257", R_SE_N);
  ref("refuse_se_bwd_cse_257", R_SEB_N);
  ref("refuse_add_mixed_storage", R_ADD_MIXED);
  ref("refuse_add_c_mod4", R_ADD_C4);
  ref("refuse_copy_grad_c_mod4", R_COPY_C4);
  ref("refuse_copy_grad_tail", R_COPY_TAIL);
  ref("refuse_grad_sums_c_mod4", R_GSUMS_C4);
  return t;
}
// ---- end of the table --------------------------------------------------------------------------

// ---- verdict and the launch rig ----------------------------------------------------------------
struct Verdict {
  bool threw = false;
  std::string what;
  Field f;
  bool exact_ok = true, canary_ok = true, repeat_ok = true, inputs_ok = true, untouched = true;
  long kinks = 0, kink_of = 0;
  bool sink = false, P_ok = true;
  int P = 0, Pexp = 0;
  gck::SinkCheck s;
  std::string detail;  // "name":ratio pairs of the case's fields
  double bytes = 0;    // the tensors of the case
  std::string plan;    // --plan: the geometry
  void field(const char* name, const Field& x) {
    f.merge(x);
    detail += std::string(detail.empty() ? "" : ",") + "\"" + name + "\":" + num(x.ratio);
  }
};

struct In : Dev {  // an input buffer that must come back unchanged
  std::vector<uint8_t> h;
  void raw(const void* p, size_t bytes) {
    h.assign(static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(p) + bytes);
    put(h.data(), bytes);
  }
  void f32(const std::vector<float>& v) { raw(v.data(), v.size() * 4); }
  void bf(std::vector<float>& v) {  // rounds v in place to the stored values
    std::vector<uint16_t> w(v.size());
    for (size_t i = 0; i < v.size(); ++i) {
      w[i] = gck::f2bf(v[i]);
      v[i] = gck::bf2f(w[i]);
    }
    raw(w.data(), w.size() * 2);
  }
  void st(std::vector<float>& v, bool asbf) {
    if (asbf) bf(v);
    else f32(v);
  }
  bool same() const {
    std::vector<uint8_t> g(h.size());
    if (!h.empty()) CK(hipMemcpy(g.data(), d, g.size(), hipMemcpyDeviceToHost));
    return g == h;
  }
};

struct Rig {
  hipStream_t st;
  Verdict& v;
  std::vector<Guarded*> outs;
  std::vector<In*> ins;
  // NaN-filled (or prev-filled) float output
  void outf(Guarded& g, size_t n, const std::vector<float>* prev = nullptr) {
    g.alloc(n * 4);
    if (prev) std::memcpy(g.fill(), prev->data(), n * 4);
    else g.fill32(0x7fc00000u);
    outs.push_back(&g);
    v.bytes += n * 4.0;
  }
  void outd(Guarded& g, size_t n) {  // doubles: both words of 0x7ff80000 7ff80000 make a NaN
    g.alloc(n * 8);
    g.fill32(0x7ff80000u);
    outs.push_back(&g);
  }
  void outb(Guarded& g, size_t bytes, uint8_t fill) {
    g.alloc(bytes);
    std::memset(g.fill(), fill, g.n);
    outs.push_back(&g);
  }
  void in(In& i, std::vector<float>& h, bool asbf = false) {
    i.st(h, asbf);
    ins.push_back(&i);
    v.bytes += h.size() * (asbf ? 2.0 : 4.0);
  }
  // two launches from the same initial state; false when the launcher refused
  template <class L>
  bool go(L&& launch) {
    std::vector<std::vector<uint8_t>> first;
    for (int rep = 0; rep < 2; ++rep) {
      for (Guarded* o : outs) o->upload();
      try {
        launch();
      } catch (const HipError& e) {
        fatal(e.what(), g_case);
      } catch (const std::exception& e) {
        v.threw = true;
        v.what = e.what();
      }
      CK(hipStreamSynchronize(st));
      CK(hipGetLastError());
      for (size_t i = 0; i < outs.size(); ++i) {
        outs[i]->download();
        if (v.threw) v.untouched &= outs[i]->got == outs[i]->init;
        v.canary_ok &= outs[i]->intact();
        if (rep == 0) first.push_back(outs[i]->got);
        else v.repeat_ok &= outs[i]->got == first[i];
      }
      if (v.threw) break;
    }
    for (In* i : ins) v.inputs_ok &= i->same();
    return !v.threw;
  }
};

static const float* F(const Guarded& g) { return reinterpret_cast<const float*>(g.out()); }
static const double* D(const Guarded& g) { return reinterpret_cast<const double*>(g.out()); }
static std::vector<float> widen(const Guarded& g, size_t n, bool bf) {
  std::vector<float> o(n);
  if (bf) {
    for (size_t i = 0; i < n; ++i) {
      uint16_t h;
      std::memcpy(&h, g.out() + 2 * i, 2);
      o[i] = gck::bf2f(h);
    }
  } else {
    std::memcpy(o.data(), g.out(), n * 4);
  }
  return o;
}
static bool bytes_equal(const Guarded& g, const void* want, size_t bytes) { return std::memcmp(g.out(), want, bytes) == 0; }

// per-channel BN parameters, all distinct; relu6 views reach z < 0 and z > 6 (conv_parity's recipe)
struct Bn {
  std::vector<float> mu, rstd, sc, be, gamma;
  In dmu, drstd, dsc, dbe, dgamma;
  void gen(int n, int act, uint64_t seed) {
    mu.resize(n); rstd.resize(n); sc.resize(n); be.resize(n); gamma.resize(n);
    gck::fill_uni(mu, seed, 0.3f);
    gck::fill_uni(rstd, seed + 3, 0.5f, 1.0f);
    gck::fill_uni(gamma, seed + 1, act == 2 ? 3.5f : 0.5f, act == 2 ? 4.5f : 1.0f);
    for (int k = 0; k < n; ++k) {
      if (k % 3 == 1) gamma[k] = -gamma[k];
      sc[k] = gamma[k] * rstd[k];
    }
    gck::fill_uni(be, seed + 2, act == 2 ? 3.0f : 0.5f, act == 2 ? 2.0f : 0.0f);
  }
  void up(Rig& r) {
    r.in(dmu, mu); r.in(drstd, rstd); r.in(dsc, sc); r.in(dbe, be); r.in(dgamma, gamma);
  }
  cck::BnView view(const float* x, int act) const { return cck::BnView{x, mu.data(), sc.data(), be.data(), act}; }
  InX inx(const In& x, int act, int bf) const { return InX{x.f(), dmu.f(), dsc.f(), dbe.f(), act, bf}; }
};
static InX raw_inx(const In& x, int bf) { return InX{x.f(), nullptr, nullptr, nullptr, 0, bf}; }

// the GradSink of a case: its BN input y2 [rows][C], partial buffer and the comparison
struct Sink {
  Bn bn;
  std::vector<float> y2;
  In dy2;
  Guarded part;
  int act = 0, bf = 0, C = 0;
  long rows = 0;
  void gen(long rows_, int C_, int act_, int bf_, uint64_t seed) {
    rows = rows_; C = C_; act = act_; bf = bf_;
    bn.gen(C, act, seed);
    y2.resize((size_t)rows * C);
    gck::fill_uni(y2, seed + 9);
    if (bf) for (auto& x : y2) x = gck::round_bf(x);
  }
  long kinks() const { return cck::gradsink_kinks(y2.data(), rows, C, bn.mu.data(), bn.sc.data(), bn.be.data(), act); }
  void up(Rig& r, int Pexp) {
    bn.up(r);
    r.in(dy2, y2, bf != 0);
    part.alloc((size_t)C * Pexp * 8);
    part.fill32(gck::kUnwritten);
    r.outs.push_back(&part);
    r.v.sink = true;
    r.v.Pexp = Pexp;
  }
  GradSink gs() const {
    return GradSink{reinterpret_cast<float2*>(part.ptr()), C, 0, dy2.f(), bn.dmu.f(), bn.drstd.f(), bn.dsc.f(), bn.dbe.f(),
                    act, bf};
  }
  // stored: the gradient the device wrote (or read, for grad_sums)
  void check(Verdict& v, const float* stored, int P) {
    v.P = P;
    v.P_ok = P == v.Pexp;
    if (!v.P_ok) return;  // the partials are laid out with another pitch: not read
    v.s = gck::check_gradsink(stored, rows, C, y2.data(), bn.mu.data(), bn.rstd.data(), bn.sc.data(), bn.be.data(), act,
                              reinterpret_cast<const float*>(part.out()), P, true);
    v.kinks += kinks();
    v.kink_of += (long)y2.size();
  }
};

static std::string red_geo(long rows, int C, int nseg) {
  const RedPlanInfo p = red_plan_info(rows, C, nseg);
  const long last = rows - (long)(p.chunks - 1) * p.rpc;         // rows of the last chunk
  const long full = std::min<long>(p.rpc, rows);                 // rows of the first
  const long lane_max = (full + p.rpi - 1) / p.rpi;              // rows lane 0 of a row group sees there
  const long lane_last = last >= p.rpi ? (last - (p.rpi - 1) + p.rpi - 1) / p.rpi : 0;  // rows the last lane sees in the last chunk
  char b[400];
  snprintf(b, sizeof b,
           "\"red\":{\"rows\":%ld,\"nseg\":%d,\"tpr\":%d,\"rpi\":%d,\"idle\":%d,\"cgroups\":%d,\"tpr_last\":%d,\"rpc\":%ld,"
           "\"chunks\":%d,\"last_chunk_rows\":%ld,\"lane_rows\":%ld,\"lane0_rows_last\":%ld,\"lastlane_rows_last\":%ld,"
           "\"depth\":%d,\"scratch_doubles\":%zu}",
           rows, nseg, p.tpr, p.rpi, 256 - p.tpr * p.rpi, p.cgroups, p.tpr_last, p.rpc, p.chunks, last, lane_max,
           (last + p.rpi - 1) / p.rpi, lane_last, p.depth, colred_scratch_doubles(rows, C, nseg));
  return b;
}

// ---- column reductions -------------------------------------------------------------------------
static void run_red(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  const long M = c.M;
  const int C = c.C;
  const size_t n = (size_t)M * C;
  v.plan = red_geo(M, C, 1);
  const bool stats = c.op == STATS || c.op == STATS_SUMS;
  std::vector<float> y(n), da, gamma(C), mm0(C), mv0(C), prev;
  gck::fill_uni(y, seed);
  if (stats)
    for (long m = 0; m < M; ++m) {
      y[m * C + 0] += 1000.f;                       // mean 1e3 x the spread: the shift
      y[m * C + 1] = 0.75f;                         // constant: var = 0, rstd = 1 / sqrt(eps)
      y[m * C + 2] *= 1.0f / 1024.f;                // a small channel
    }
  if (c.bf) for (auto& x : y) x = gck::round_bf(x);
  gck::fill_uni(gamma, seed + 1, 0.5f, 1.0f);
  gck::fill_uni(mm0, seed + 2);
  gck::fill_uni(mv0, seed + 3, 0.5f, 1.0f);
  Bn bn;
  bn.gen(C, c.act, seed + 10);
  const nck::BnPar par{bn.mu.data(), bn.rstd.data(), bn.gamma.data(), bn.be.data(), c.act};
  if (!stats) {
    da.resize(n);
    gck::fill_uni(da, seed + 4);
    if (c.act == 2) {  // the reference alone stays under the kink cap
      for (int ch = 0; ch < C; ++ch) v.kinks += nck::bwd_sums(da.data(), y.data(), M, C, ch, par).kinks;
      v.kink_of = (long)n;
    }
  }
  if (c.acc) {
    prev.resize(n);
    gck::fill_uni(prev, seed + 5);
  }
  v.bytes = n * (c.bf ? 2.0 : 4.0) + da.size() * 4.0;
  if (plan) return;

  In dy, dda, dgamma;
  Guarded scratch, mean, rstd, sc, mmean, mvar, side, sums, mdz, mdzx, coef, out;
  r.in(dy, y, c.bf != 0);
  r.outd(scratch, colred_scratch_doubles(M, C, 1));
  const float eps = 1e-3f;
  const bool frozen = c.op == BN_BWD && c.flav == 1;
  if (stats) r.in(dgamma, gamma);
  else {
    r.in(dda, da);
    bn.up(r);
  }
  switch (c.op) {
    case STATS:
      r.outf(mean, C); r.outf(rstd, C); r.outf(sc, C);
      r.outf(mmean, C, &mm0); r.outf(mvar, C, &mv0);
      if (c.flav == 2) r.outd(side, 2 * (size_t)C);
      break;
    case STATS_SUMS: case BRED_SUMS: r.outd(sums, 3 * (size_t)C); break;
    case BRED: r.outf(mdz, C); r.outf(mdzx, C); break;
    case BN_BWD: r.outf(coef, 3 * (size_t)C); r.outf(out, n, c.acc ? &prev : nullptr); break;
    default: break;
  }
  const bool ran = r.go([&] {
    double* sp = reinterpret_cast<double*>(scratch.ptr());
    switch (c.op) {
      case STATS:
        launch_bn_stats(dy.f(), M, C, sp, mean.ptr(), rstd.ptr(), dgamma.f(), sc.ptr(), c.flav ? mmean.ptr() : nullptr,
                        c.flav ? mvar.ptr() : nullptr, eps, r.st, c.bf != 0,
                        c.flav == 2 ? reinterpret_cast<double*>(side.ptr()) : nullptr);
        break;
      case STATS_SUMS: launch_bn_stats_sums(dy.f(), M, C, sp, reinterpret_cast<double*>(sums.ptr()), r.st, c.bf != 0); break;
      case BRED:
        launch_bn_bwd_reduce(dda.f(), dy.f(), bn.dmu.f(), bn.drstd.f(), bn.dgamma.f(), bn.dbe.f(), M, C, c.act, sp, mdz.ptr(),
                             mdzx.ptr(), r.st, c.bf != 0);
        break;
      case BRED_SUMS:
        launch_bn_bwd_reduce_sums(dda.f(), dy.f(), bn.dmu.f(), bn.drstd.f(), bn.dgamma.f(), bn.dbe.f(), M, C, c.act, sp,
                                  reinterpret_cast<double*>(sums.ptr()), r.st, c.bf != 0);
        break;
      case BN_BWD:
        launch_bn_bwd(dda.f(), dy.f(), bn.dmu.f(), bn.drstd.f(), bn.dgamma.f(), bn.dbe.f(), out.ptr(), M, C, c.act, frozen,
                      c.acc, sp, coef.ptr(), r.st);
        break;
      default: break;
    }
  });
  if (!ran) return;
  if (c.op == STATS) {
    nck::StatOut o;
    o.mean = F(mean); o.rstd = F(rstd); o.sc = F(sc);
    if (c.flav == 1) { o.mmean = F(mmean); o.mvar = F(mvar); }
    if (c.flav == 2) o.side = D(side);
    const nck::StatCheck k = nck::check_stats(y.data(), M, C, gamma.data(), eps, mm0.data(), mv0.data(), o);
    v.field("mean", k.mean); v.field("rstd", k.rstd); v.field("sc", k.sc);
    if (c.flav == 1) v.field("moving", k.moving);
    if (c.flav == 2) v.field("side", k.side);
    // without moving statistics, or with the deferred pairs, the moving buffers keep their bytes
    if (c.flav != 1) v.exact_ok &= bytes_equal(mmean, mm0.data(), C * 4) && bytes_equal(mvar, mv0.data(), C * 4);
  } else if (c.op == STATS_SUMS) {
    v.field("sums", nck::check_stats_sums(y.data(), M, C, D(sums)));
  } else {
    Field f1, f2, f0;
    for (int ch = 0; ch < C; ++ch) {
      if (frozen) break;
      const nck::BwdSums s = nck::bwd_sums(da.data(), y.data(), M, C, ch, par);
      if (c.op == BRED_SUMS) {
        f0.add(D(sums)[3 * ch], (double)M, 0.0, ch);
        f1.add(D(sums)[3 * ch + 1], s.s1, s.e1, ch);
        f2.add(D(sums)[3 * ch + 2], s.s2, s.e2, ch);
      } else {
        const float* a = c.op == BRED ? F(mdz) + ch : F(coef) + 3 * ch + 1;
        const float* b = c.op == BRED ? F(mdzx) + ch : F(coef) + 3 * ch + 2;
        f1.add(*a, s.s1 / M, nck::fstore(s.s1 / M, s.e1 / M), ch);
        f2.add(*b, s.s2 / M, nck::fstore(s.s2 / M, s.e2 / M), ch);
        if (c.op == BN_BWD) {
          const double g = (double)bn.gamma[ch] * (double)bn.rstd[ch];
          f0.add(F(coef)[3 * ch], g, nck::fstore(g, 0.0), ch);
        }
      }
    }
    if (!frozen) {
      v.field("sum_dz", f1);
      v.field("sum_dzx", f2);
      if (c.op != BRED) v.field(c.op == BN_BWD ? "coef0" : "rows", f0);
    }
    if (c.op == BN_BWD) {
      long kk = 0;
      const gck::Reference ref = nck::bwd_apply_ref(da.data(), y.data(), M, C, par, F(coef), frozen,
                                                    c.acc ? prev.data() : nullptr, &kk);
      v.field("dy", nck::check_arr(ref, F(out)));
      if (frozen) v.exact_ok &= coef.got == coef.init;  // the frozen form writes no coefficients
    }
  }
}

// ---- finalizes ---------------------------------------------------------------------------------
struct FinMember {
  int P = 0;
  long M = 0;
  std::vector<float> part, cnt, gamma, mm0, mv0;
  In dpart, dcnt, dgamma;
  Guarded mean, rstd, sc, mmean, mvar, side, mdz, mdzx;
  Guarded mean2, rstd2, sc2, mmean2, mvar2;  // FOLD: the fold_sums + from_sums path
};
static void run_fin(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  const int C = c.C, n = c.B;
  const bool bwd = c.op == BFIN;
  std::vector<FinMember> ms(n);
  std::string pl = "\"members\":[";
  for (int i = 0; i < n; ++i) {
    FinMember& m = ms[i];
    m.P = std::max(1, c.P - 37 * i);
    long zeros = 0;
    nck::gen_partials(C, m.P, (c.flav & 1) != 0, bwd, seed + 100 * i, m.part, m.cnt, &m.M, &zeros);
    if (bwd) m.M = 1000 + 17 * i;
    m.gamma.resize(C); m.mm0.resize(C); m.mv0.resize(C);
    gck::fill_uni(m.gamma, seed + 100 * i + 1, 0.5f, 1.0f);
    gck::fill_uni(m.mm0, seed + 100 * i + 2);
    gck::fill_uni(m.mv0, seed + 100 * i + 3, 0.5f, 1.0f);
    v.bytes += m.part.size() * 4.0;
    pl += std::string(i ? "," : "") + "{\"P\":" + std::to_string(m.P) + ",\"M\":" + std::to_string(m.M) +
          ",\"zero_cnt\":" + std::to_string(zeros) + "}";
  }
  v.plan = pl + "]";
  if (plan) return;
  const float eps = 1e-3f;
  const bool side = (c.flav & 2) != 0;
  Guarded sums;
  for (FinMember& m : ms) {
    r.in(m.dpart, m.part);
    r.in(m.dcnt, m.cnt);
    r.in(m.dgamma, m.gamma);
    if (bwd) {
      r.outf(m.mdz, C); r.outf(m.mdzx, C);
    } else {
      r.outf(m.mean, C); r.outf(m.rstd, C); r.outf(m.sc, C); r.outf(m.mmean, C, &m.mm0); r.outf(m.mvar, C, &m.mv0);
      if (side) r.outd(m.side, 2 * (size_t)C);
    }
    if (c.op == FOLD) {
      r.outf(m.mean2, C); r.outf(m.rstd2, C); r.outf(m.sc2, C); r.outf(m.mmean2, C, &m.mm0); r.outf(m.mvar2, C, &m.mv0);
    }
  }
  if (c.op == FOLD) r.outd(sums, (size_t)n * C * 3);
  auto seg = [&](FinMember& m, bool second) {
    BnFinSeg s{};
    s.part = reinterpret_cast<const float2*>(m.dpart.d);
    s.cnt = bwd ? nullptr : m.dcnt.f();
    s.P = m.P;
    s.M = m.M;
    s.gamma = m.dgamma.f();
    if (bwd) {
      s.mdz = m.mdz.ptr(); s.mdzx = m.mdzx.ptr();
    } else if (second) {
      s.mean = m.mean2.ptr(); s.rstd = m.rstd2.ptr(); s.sc = m.sc2.ptr(); s.mmean = m.mmean2.ptr(); s.mvar = m.mvar2.ptr();
    } else {
      s.mean = m.mean.ptr(); s.rstd = m.rstd.ptr(); s.sc = m.sc.ptr(); s.mmean = m.mmean.ptr(); s.mvar = m.mvar.ptr();
      s.side = side ? reinterpret_cast<double*>(m.side.ptr()) : nullptr;
    }
    return s;
  };
  const bool ran = r.go([&] {
    std::vector<BnFinSeg> segs;
    for (FinMember& m : ms) segs.push_back(seg(m, false));
    if (n == 1 && bwd) {
      launch_bn_bwd_finalize(segs[0].part, segs[0].P, segs[0].M, C, segs[0].mdz, segs[0].mdzx, r.st);
    } else if (n == 1) {
      launch_bn_finalize(segs[0].part, segs[0].cnt, segs[0].P, segs[0].M, C, segs[0].mean, segs[0].rstd, segs[0].gamma,
                         segs[0].sc, segs[0].mmean, segs[0].mvar, eps, r.st, segs[0].side);
    } else if (bwd) {
      launch_bn_bwd_finalize_group(segs.data(), n, C, r.st);
    } else {
      launch_bn_finalize_group(segs.data(), n, C, eps, r.st);
    }
    if (c.op == FOLD) {
      std::vector<BnFinSeg> s2;
      for (FinMember& m : ms) s2.push_back(seg(m, true));
      launch_bn_fold_sums(s2.data(), n, C, false, reinterpret_cast<double*>(sums.ptr()), r.st);
      launch_bn_from_sums(s2.data(), n, C, false, reinterpret_cast<const double*>(sums.ptr()), eps, r.st);
    }
  });
  if (!ran) return;
  nck::StatCheck k;
  Field f1, f2;
  for (FinMember& m : ms)
    for (int ch = 0; ch < C; ++ch) {
      const nck::Sums s = nck::fold_partials(m.part.data(), m.cnt.data(), m.P, ch, bwd);
      if (bwd) {
        f1.add(F(m.mdz)[ch], s.s0 / m.M, nck::fstore(s.s0 / m.M, s.e0 / m.M), ch);
        f2.add(F(m.mdzx)[ch], s.s1 / m.M, nck::fstore(s.s1 / m.M, s.e1 / m.M), ch);
        continue;
      }
      nck::StatOut o;
      o.mean = F(m.mean); o.rstd = F(m.rstd); o.sc = F(m.sc);
      if (side) o.side = D(m.side);
      else { o.mmean = F(m.mmean); o.mvar = F(m.mvar); }
      nck::check_stat_chan(nck::stats_from(s, m.M, m.gamma[ch], (double)eps, m.mm0[ch], m.mv0[ch]), o, ch, k);
    }
  if (bwd) {
    v.field("mdz", f1);
    v.field("mdzx", f2);
    return;
  }
  v.field("mean", k.mean); v.field("rstd", k.rstd); v.field("sc", k.sc);
  if (side) v.field("side", k.side);
  else v.field("moving", k.moving);
  for (FinMember& m : ms) {
    if (side) v.exact_ok &= bytes_equal(m.mmean, m.mm0.data(), C * 4) && bytes_equal(m.mvar, m.mv0.data(), C * 4);
    if (c.op == FOLD)
      v.exact_ok &= m.mean.got == m.mean2.got && m.rstd.got == m.rstd2.got && m.sc.got == m.sc2.got &&
                    m.mmean.got == m.mmean2.got && m.mvar.got == m.mvar2.got;
  }
  if (c.op == FOLD) {  // sums[i][c] = (rows, S1, S2)
    Field fs;
    for (int i = 0; i < n; ++i)
      for (int ch = 0; ch < C; ++ch) {
        const nck::Sums s = nck::fold_partials(ms[i].part.data(), ms[i].cnt.data(), ms[i].P, ch, false);
        const double* q = D(sums) + ((size_t)i * C + ch) * 3;
        fs.add(q[0], (double)ms[i].M, 0.0, ch);
        fs.add(q[1], s.s0, s.e0, ch);
        fs.add(q[2], s.s1, s.e1, ch);
      }
    v.field("sums", fs);
  }
}

// ---- squeeze-excite ----------------------------------------------------------------------------
static void run_se(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  const int B = c.B, HW = (int)c.M, C = c.C, N = c.N;
  const size_t n = (size_t)B * HW * C;
  const RedPlanInfo rp = red_plan_info(HW, C, B);
  const SePlanInfo sp = se_plan_info(B, C, N, rp.chunks);
  const bool bwd = c.op == SE_BWD;
  const int Pexp = c.sink ? ew_gstats_partials(HW, C, B) : 0;
  char b[300];
  snprintf(b, sizeof b,
           ",\"se\":{\"s1\":%d,\"cs1\":%d,\"s2\":%d,\"cs2\":%d,\"fold_small\":%d,\"kg\":%d,\"jg\":%d,\"fold_deep\":%d,"
           "\"shares_floats\":%ld,\"tail_floats\":%ld},\"P_expected\":%d",
           sp.s1, sp.cs1, sp.s2, sp.cs2, sp.fold_small, sp.kg, sp.jg,
           sp.fold_small ? (rp.chunks > 7 * sp.kg) : (rp.chunks > 3), (long)B * sp.s1 * N, (long)B * C * 4, Pexp);
  v.plan = red_geo(HW, C, B) + b;
  std::vector<float> x(n), w1((size_t)C * N), b1(N), w2((size_t)N * C), b2(C), dy, scale, hidden, prev;
  gck::fill_uni(x, seed);
  if (c.bf) for (auto& q : x) q = gck::round_bf(q);
  gck::fill_uni(w1, seed + 1, 2.0f / std::sqrt((float)C));
  gck::fill_uni(b1, seed + 2, 0.5f);
  gck::fill_uni(w2, seed + 3, 2.0f / std::sqrt((float)N));  // fwd: [N][C]; bwd: the transposed kernel [C][N]
  gck::fill_uni(b2, seed + 4, 0.5f);
  const int xact = c.view == 2 ? 2 : 1;
  Bn bn;
  bn.gen(C, xact, seed + 10);
  Sink sk;
  if (bwd) {
    dy.resize(n); scale.resize((size_t)B * C); hidden.resize((size_t)B * N);
    gck::fill_uni(dy, seed + 5);
    gck::fill_uni(scale, seed + 6, 0.45f, 0.5f);
    gck::fill_uni(hidden, seed + 7, 3.0f);
    if (c.acc) {
      prev.resize(n);
      gck::fill_uni(prev, seed + 8);
    }
    if (c.sink) {
      sk.gen((long)B * HW, C, xact, c.bf, seed + 20);
      v.kinks = sk.kinks();
      v.kink_of = (long)n;
    }
  }
  v.bytes = n * (c.bf ? 2.0 : 4.0) + dy.size() * 4.0 + prev.size() * 4.0;
  if (plan) return;

  In dx, dw1, db1, dw2, db2, ddy, dscale, dhidden;
  Guarded scratch, pool, hid, sc, gsum, out;
  r.in(dx, x, c.bf != 0);
  r.in(dw1, w1); r.in(db1, b1); r.in(dw2, w2); r.in(db2, b2);
  if (c.view) bn.up(r);
  r.outd(scratch, colred_scratch_doubles(HW, C, B));
  const InX xin = c.view ? bn.inx(dx, xact, c.bf) : raw_inx(dx, c.bf);
  int P = 0;
  if (!bwd) {
    r.outf(pool, (size_t)B * C); r.outf(hid, (size_t)B * N); r.outf(sc, (size_t)B * C);
  } else {
    r.in(ddy, dy); r.in(dscale, scale); r.in(dhidden, hidden);
    r.outf(gsum, (size_t)B * C);
    r.outf(out, n, c.acc ? &prev : nullptr);
    if (c.sink) sk.up(r, Pexp);
  }
  const bool ran = r.go([&] {
    double* spd = reinterpret_cast<double*>(scratch.ptr());
    if (!bwd)
      launch_se_fwd(xin, nullptr, B, HW, C, N, dw1.f(), db1.f(), dw2.f(), db2.f(), c.act, pool.ptr(), hid.ptr(), sc.ptr(),
                    r.st, spd);
    else
      P = launch_se_bwd(ddy.f(), xin, out.ptr(), B, HW, C, N, dw1.f(), db1.f(), dw2.f(), db2.f(), c.act, nullptr,
                        dhidden.f(), dscale.f(), gsum.ptr(), c.acc, r.st, spd, c.sink ? sk.gs() : GradSink{});
  });
  if (!ran) return;
  const cck::BnView bv = c.view ? bn.view(x.data(), xact) : cck::BnView{x.data()};
  const cck::Val xv = cck::view_inx(bv, (long)B * HW, C);
  const nck::SeShape sh{B, HW, C, N, c.act, sp.s1, sp.cs1, sp.jg};
  if (!bwd) {
    const nck::SeFwdRef ref = nck::se_fwd_ref(sh, xv, w1.data(), b1.data(), w2.data(), b2.data());
    v.field("pool", nck::check_arr(ref.pool, F(pool)));
    v.field("hidden", nck::check_arr(ref.hidden, F(hid)));
    v.field("scale", nck::check_arr(ref.scale, F(sc)));
  } else {
    const nck::SeBwdRef ref = nck::se_bwd_ref(sh, dy.data(), xv, scale.data(), hidden.data(), w2.data(), w1.data(),
                                              c.acc ? prev.data() : nullptr);
    v.field("gsum", nck::check_arr(ref.gsum, F(gsum)));
    v.field("dx", nck::check_arr(ref.dx, F(out)));
    if (c.sink) sk.check(v, F(out), P);
  }
}

// ---- max-pool ----------------------------------------------------------------------------------
// the forward on the host in float, for --plan's tie share (and norm_teeth)
static void pool_inputs(const Case& c, uint64_t seed, std::vector<float>& x, Bn& bn, int* act) {
  const size_t n = (size_t)c.B * c.H * c.W * c.C;
  x.resize(n);
  gck::fill_uni(x, seed);
  *act = c.flav == 2 ? 2 : c.flav == 3 ? 1 : 0;
  if (c.flav == 1)
    for (auto& q : x) q = std::floor(q * 8.f) / 8.f;  // eighths: exact ties are frequent
  if (c.flav == 2) {
    // |x| in [2, 9) below zero, [8, 15) above: with sc in +-[1, 1.25], mu and be within 0.3 every
    // pre-activation lies beyond -1 or 7
    for (auto& q : x) q = q < 0.f ? -2.f + 7.f * q : 8.f + 7.f * q;
    bn.mu.resize(c.C); bn.sc.resize(c.C); bn.be.resize(c.C); bn.rstd.assign(c.C, 1.f); bn.gamma.resize(c.C);
    gck::fill_uni(bn.mu, seed + 1, 0.3f);
    gck::fill_uni(bn.sc, seed + 2, 0.125f, 1.125f);
    for (int k = 0; k < c.C; ++k) if (k % 3 == 1) bn.sc[k] = -bn.sc[k];
    bn.gamma = bn.sc;
    gck::fill_uni(bn.be, seed + 3, 0.3f);
  } else {
    bn.gen(c.C, *act, seed + 1);
  }
  if (c.bf) for (auto& q : x) q = gck::round_bf(q);
}
static void run_pool(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  const nck::PoolGeo g = nck::pool_geo(c.B, c.H, c.W, c.C, c.k, c.s);
  const size_t nin = (size_t)g.B * g.H * g.W * g.C, nout = (size_t)g.B * g.Ho * g.Wo * g.C;
  char b[200];
  snprintf(b, sizeof b, "\"pool\":{\"Ho\":%d,\"Wo\":%d,\"pt\":%d,\"pl\":%d,\"quad\":%d}", g.Ho, g.Wo, g.pt, g.pl, c.C % 4 == 0);
  v.plan = b;
  std::vector<float> x, dyv(nout), prev;
  Bn bn;
  int act;
  pool_inputs(c, seed, x, bn, &act);
  const bool view = c.flav >= 2;
  const cck::BnView bv = view ? bn.view(x.data(), act) : cck::BnView{x.data()};
  gck::fill_uni(dyv, seed + 5);
  if (c.acc) {
    prev.resize(nin);
    gck::fill_uni(prev, seed + 6);
  }
  v.bytes = nin * (c.bf ? 2.0 : 4.0) + nout * 5.0;
  v.kink_of = (long)nout;
  if (plan) {
    std::vector<float> hy;
    std::vector<uint8_t> ha;
    nck::maxpool_fwd_cpu(g, bv, false, hy, ha);
    if (c.bf) for (auto& q : hy) q = gck::round_bf(q);
    v.kinks = nck::check_maxpool_fwd(g, bv, c.bf != 0, hy.data(), ha.data()).ties;
    return;
  }
  In dx, ddy;
  Guarded y, amax, out;
  r.in(dx, x, c.bf != 0);
  if (view) bn.up(r);
  r.in(ddy, dyv);
  if (c.bf) { y.alloc(nout * 2); y.fill16(0x7fc0); r.outs.push_back(&y); }
  else r.outf(y, nout);
  r.outb(amax, (nout + 3) / 4 * 4, 0xEE);
  r.outf(out, nin, c.acc ? &prev : nullptr);
  const InX xin = view ? bn.inx(dx, act, c.bf) : raw_inx(dx, c.bf);
  const bool ran = r.go([&] {
    uint8_t* am = reinterpret_cast<uint8_t*>(amax.ptr());
    launch_maxpool_fwd(xin, y.ptr(), am, g.B, g.H, g.W, g.C, g.Ho, g.Wo, g.k, g.s, g.pt, g.pl, r.st);
    launch_maxpool_bwd(am, ddy.f(), out.ptr(), g.B, g.H, g.W, g.C, g.Ho, g.Wo, g.k, g.s, g.pt, g.pl, c.acc, r.st);
  });
  if (!ran) return;
  const std::vector<float> ys = widen(y, nout, c.bf != 0);
  const nck::PoolCheck k = nck::check_maxpool_fwd(g, bv, c.bf != 0, ys.data(), amax.out());
  v.field("y", k.y);
  v.kinks = k.ties;
  v.exact_ok &= k.amax_bad == 0;
  // the gather replayed from the taps the device recorded, in its own order: exact
  const std::vector<float> want = nck::maxpool_bwd_replay(g, amax.out(), dyv.data(), c.acc ? prev.data() : nullptr);
  const bool dx_ok = bytes_equal(out, want.data(), nin * 4);
  v.exact_ok &= dx_ok;
  v.detail += std::string(",\"amax_bad\":") + std::to_string(k.amax_bad) + ",\"dx_exact\":" + (dx_ok ? "1" : "0");
}

// ---- nearest upsample --------------------------------------------------------------------------
static void run_ups(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  const int B = c.B, H = c.H, W = c.W, Ho = c.Ho, Wo = c.Wo, C = c.C;
  const size_t nin = (size_t)B * H * W * C, nout = (size_t)B * Ho * Wo * C;
  // the float source map against the exact rational one floor(d in / out)
  int differs = 0, maxfan = 0;
  for (int iy = 0; iy < H; ++iy) {
    int fan = 0;
    for (int oy = 0; oy < Ho; ++oy) fan += nck::nn_src(oy, H, Ho) == iy;
    maxfan = std::max(maxfan, fan);
  }
  for (int oy = 0; oy < Ho; ++oy) differs += nck::nn_src(oy, H, Ho) != std::min((int)((long)oy * H / Ho), H - 1);
  char b[200];
  snprintf(b, sizeof b, "\"ups\":{\"quad\":%d,\"max_fan\":%d,\"float_map_differs\":%d}", C % 4 == 0, maxfan, differs);
  v.plan = b;
  std::vector<float> x(nin), dyv(nout), prev;
  gck::fill_uni(x, seed);
  if (c.bf) for (auto& q : x) q = gck::round_bf(q);
  gck::fill_uni(dyv, seed + 5);
  const int act = c.view == 2 ? 2 : 1;
  Bn bn;
  bn.gen(C, act, seed + 1);
  if (c.acc) {
    prev.resize(nin);
    gck::fill_uni(prev, seed + 6);
  }
  v.bytes = nin * 4.0 + nout * 8.0;
  if (plan) return;
  In dx, ddy;
  Guarded y, out;
  r.in(dx, x, c.bf != 0);
  if (c.view) bn.up(r);
  r.in(ddy, dyv);
  if (c.bf) { y.alloc(nout * 2); y.fill16(0x7fc0); r.outs.push_back(&y); }
  else r.outf(y, nout);
  r.outf(out, nin, c.acc ? &prev : nullptr);
  const InX xin = c.view ? bn.inx(dx, act, c.bf) : raw_inx(dx, c.bf);
  const bool ran = r.go([&] {
    launch_upsample_fwd(xin, y.ptr(), B, H, W, C, Ho, Wo, r.st);
    launch_upsample_bwd(ddy.f(), out.ptr(), B, H, W, C, Ho, Wo, c.acc, r.st);
  });
  if (!ran) return;
  const std::vector<float> ys = widen(y, nout, c.bf != 0);
  const cck::BnView bv = c.view ? bn.view(x.data(), act) : cck::BnView{x.data()};
  Field f;
  for (int bb = 0; bb < B; ++bb)
    for (int oy = 0; oy < Ho; ++oy)
      for (int ox = 0; ox < Wo; ++ox)
        for (int ch = 0; ch < C; ++ch) {
          const long e = (((long)bb * H + nck::nn_src(oy, H, Ho)) * W + nck::nn_src(ox, W, Wo)) * C + ch;
          double a, ea;
          cck::inx_one(bv, e, ch, &a, &ea);
          if (c.bf) {
            const double m = std::fabs(a) + ea;
            a = (double)gck::round_bf((float)a);
            if (ea > 0.0 && m > 0.0) ea += std::ldexp(1.0, std::ilogb(m) - 7);
          }
          const long o = (((long)bb * Ho + oy) * Wo + ox) * C + ch;
          f.add(ys[o], a, ea, o);  // a raw view: bound 0, the value itself
        }
  v.field("y", f);
  const std::vector<float> want = nck::upsample_bwd_replay(B, H, W, C, Ho, Wo, dyv.data(), c.acc ? prev.data() : nullptr);
  const bool dx_ok = bytes_equal(out, want.data(), nin * 4);
  v.exact_ok &= dx_ok;
  v.detail += std::string(",\"dx_exact\":") + (dx_ok ? "1" : "0");
}

// ---- residual add, gradient copy, gradient sums ------------------------------------------------
static float drop_p(int drop) { return drop == 2 ? 0.8f : drop == 3 ? 0.015625f + 0.001953125f : 1.0f; }
static void run_ew(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  const int B = c.B, C = c.C;
  const long rows = (long)B * c.M;
  const size_t n = (size_t)rows * C;
  const int Pexp = c.sink ? ew_gstats_partials(rows, C, 1) : 0;
  v.plan = (c.sink ? red_geo(rows, C, 1) + "," : std::string()) + "\"P_expected\":" + std::to_string(Pexp) +
           ",\"rows_per_image\":" + std::to_string(c.M);
  std::vector<float> a(n), bb(n), prev, keep(B);
  gck::fill_uni(a, seed);
  gck::fill_uni(bb, seed + 1);
  for (int i = 0; i < B; ++i) keep[i] = (i % 2 == 0) ? 1.f : 0.f;  // kept / dropped images alternate
  if (c.bf && c.op == ADD) {
    for (auto& q : a) q = gck::round_bf(q);
    for (auto& q : bb) q = gck::round_bf(q);
  }
  if (c.acc) {
    prev.resize(n);
    gck::fill_uni(prev, seed + 2);
  }
  Bn bna, bnb;
  bna.gen(C, c.act, seed + 10);
  bnb.gen(C, 0, seed + 20);
  Sink sk;
  if (c.sink) {
    sk.gen(rows, C, c.act, c.bf, seed + 30);
    v.kinks = sk.kinks();
    v.kink_of = (long)n;
  }
  v.bytes = n * 12.0;
  if (plan) return;
  In da, db, dkeep;
  Guarded out;
  const float p = drop_p(c.drop);
  r.in(dkeep, keep);
  const DropView dv = c.drop ? DropView{dkeep.f(), p, c.M} : DropView{};
  int P = 0;
  bool ran;
  if (c.op == ADD) {
    r.in(da, a, c.bf != 0);
    r.in(db, bb, c.bf != 0);
    if (c.view) { bna.up(r); bnb.up(r); }
    if (c.bf) { out.alloc(n * 2); out.fill16(0x7fc0); r.outs.push_back(&out); }
    else r.outf(out, n);
    const InX xa = c.view ? bna.inx(da, c.act, c.bf) : raw_inx(da, c.bf);
    const InX xb = c.view == 2 ? bnb.inx(db, 0, c.bf) : raw_inx(db, c.bf);
    ran = r.go([&] { launch_add(xa, xb, out.ptr(), (long)n, C, r.st, dv); });
    if (!ran) return;
    const cck::Val va = cck::view_inx(c.view ? bna.view(a.data(), c.act) : cck::BnView{a.data()}, rows, C);
    const cck::Val vb = cck::view_inx(c.view == 2 ? bnb.view(bb.data(), 0) : cck::BnView{bb.data()}, rows, C);
    gck::Reference ref = nck::add_ref(va, vb, rows, C, c.drop ? keep.data() : nullptr, p, c.M);
    if (c.bf) cck::bf_store(ref);
    const std::vector<float> ys = widen(out, n, c.bf != 0);
    v.field("y", nck::check_arr(ref, ys.data()));
    return;
  }
  r.in(da, a);
  if (c.sink) sk.up(r, Pexp);
  if (c.op == COPYG) {
    r.outf(out, n, c.acc ? &prev : nullptr);
    ran = r.go([&] {
      P = launch_copy_grad(da.f(), out.ptr(), (long)n, c.acc, r.st, C, c.sink ? sk.gs() : GradSink{}, dv);
    });
    if (!ran) return;
    const std::vector<float> want =
        nck::copy_grad_replay(a.data(), rows, C, c.drop ? keep.data() : nullptr, p, c.M, c.acc ? prev.data() : nullptr);
    const bool ok = bytes_equal(out, want.data(), n * 4);
    v.exact_ok &= ok;
    v.detail += std::string("\"dst_exact\":") + (ok ? "1" : "0");
    for (size_t i = 0; i < n; ++i) v.f.nonfinite += !std::isfinite(F(out)[i]);
    if (c.sink) sk.check(v, F(out), P);
  } else {
    ran = r.go([&] { P = launch_grad_sums(da.f(), (long)n, C, sk.gs(), r.st); });
    if (!ran) return;
    sk.check(v, a.data(), P);
  }
}

// ---- the remaining elementwise launchers -------------------------------------------------------
static std::string g_golden;  // tests/golden/norm, beside the binary's directory
static void run_misc(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  const long M = c.M;
  const int C = c.C;
  const size_t n = (size_t)M * C;
  v.bytes = n * 8.0;
  if (c.op == APPLY || c.op == APPLY2) {
    std::vector<float> y(n), da(n), mdz(C), mdzx(C);
    gck::fill_uni(y, seed);
    gck::fill_uni(da, seed + 1);
    gck::fill_uni(mdz, seed + 2, 0.1f);
    gck::fill_uni(mdzx, seed + 3, 0.1f);
    if (c.bf) for (auto& q : y) q = gck::round_bf(q);
    Bn bn;
    bn.gen(C, c.act, seed + 10);
    const bool pass = c.op == APPLY2 && c.flav == 1;
    cck::GradRef gr;
    gr.da = da.data(); gr.act = c.act;
    if (!pass) {
      gr.y = y.data(); gr.mu = bn.mu.data(); gr.rstd = bn.rstd.data(); gr.sc = bn.sc.data(); gr.be = bn.be.data();
      gr.mdz = mdz.data(); gr.mdzx = mdzx.data();
    }
    cck::Val ref;
    if (c.op == APPLY2) {
      ref = cck::view_grad(gr, M, C);
      v.kinks = ref.kinks;
      v.kink_of = (long)n;
    }
    if (plan) return;
    In dy, dda, dmdz, dmdzx;
    Guarded out;
    r.in(dy, y, c.bf != 0); r.in(dda, da); r.in(dmdz, mdz); r.in(dmdzx, mdzx);
    bn.up(r);
    r.outf(out, n);
    const bool ran = r.go([&] {
      if (c.op == APPLY)
        launch_bn_apply(dy.f(), bn.dmu.f(), bn.drstd.f(), bn.dgamma.f(), bn.dbe.f(), out.ptr(), M, C, c.act, r.st);
      else
        launch_bn_bwd_apply2(GradX{dda.f(), pass ? nullptr : dy.f(), bn.dmu.f(), bn.drstd.f(), bn.dsc.f(), bn.dbe.f(),
                                   dmdz.f(), dmdzx.f(), c.act, c.bf},
                             out.ptr(), M, C, r.st);
    });
    if (!ran) return;
    if (c.op == APPLY2) {
      if (pass) v.exact_ok &= bytes_equal(out, da.data(), n * 4);  // the gradient itself
      gck::Reference rr;
      rr.c = ref.v; rr.bound = ref.e;
      v.field("gx", nck::check_arr(rr, F(out)));
      return;
    }
    // z = ((y - mean) rstd) gamma + beta: four roundings, |z_dev - z| <= 2^-24 (3 |t| + |z|)
    Field f;
    for (long m = 0; m < M; ++m)
      for (int ch = 0; ch < C; ++ch) {
        const double t = ((double)y[m * C + ch] - (double)bn.mu[ch]) * (double)bn.rstd[ch] * (double)bn.gamma[ch];
        const double z = t + (double)bn.be[ch];
        double a, ea;
        cck::act_val(z, kEps24 * (3.0 * std::fabs(t) + std::fabs(z)), c.act, &a, &ea);
        f.add(F(out)[m * C + ch], a, ea, m * C + ch);
      }
    v.field("a", f);
    return;
  }
  if (c.op == BF2F) {
    std::vector<float> x(n);
    gck::fill_uni(x, seed, 100.f);
    if (plan) return;
    In dx;
    Guarded out;
    r.in(dx, x, true);
    r.outf(out, n);
    if (!r.go([&] { launch_bf16_to_f32(dx.f(), out.ptr(), (long)n, r.st); })) return;
    v.exact_ok &= bytes_equal(out, x.data(), n * 4);
    return;
  }
  if (c.op == DROPK) {
    // vectors drawn by oracle/philox.py (tests/test_norm_parity_host.py holds the file to the oracle)
    FILE* fp = fopen((g_golden + "/drop_keep.txt").c_str(), "r");
    unsigned long long sd = 0;
    long step = 0;
    int gimg0 = 0, pass = 0, nd = 0, B = 0;
    if (!fp || fscanf(fp, "%llx %ld %d %d %d %d", &sd, &step, &gimg0, &pass, &nd, &B) != 6 || nd < 1 || nd > 64 || B < 1 ||
        B > 1024) {
      v.exact_ok = false;
      v.detail = "\"golden_read\":0";
      if (fp) fclose(fp);
      return;
    }
    std::vector<int> block(nd);
    std::vector<float> p(nd), keep((size_t)nd * B);
    bool ok = true;
    for (int i = 0; i < nd; ++i) ok &= fscanf(fp, "%d", &block[i]) == 1;
    for (int i = 0; i < nd; ++i) {
      unsigned u = 0;
      ok &= fscanf(fp, "%x", &u) == 1;
      p[i] = gck::u2f(u);
    }
    for (auto& k : keep) {
      int q = 0;
      ok &= fscanf(fp, "%d", &q) == 1;
      k = (float)q;
    }
    fclose(fp);
    v.exact_ok &= ok;
    if (plan || !ok) return;
    In dblock, dp;
    Guarded out;
    dblock.raw(block.data(), nd * 4);
    r.ins.push_back(&dblock);
    r.in(dp, p);
    r.outf(out, keep.size());
    if (!r.go([&] {
          launch_drop_keep(reinterpret_cast<const int*>(dblock.d), dp.f(), nd, B, sd, step, gimg0, pass, out.ptr(), r.st);
        }))
      return;
    v.exact_ok &= bytes_equal(out, keep.data(), keep.size() * 4);
    return;
  }
  if (c.op == CKSUM) {
    // the hash restated: sum over i of mix((i << 16) ^ word_i ^ golden ratio), 64-bit wrapping.  Three sizes
    // give a grid of 1 workgroup, of many, and the capped grid whose lanes stride; one flipped bit must
    // change the value.
    std::vector<uint16_t> w(n);
    v.bytes = n * 4.0;  // two buffers of 16-bit words
    gck::Rng rng(seed);
    for (auto& q : w) q = (uint16_t)rng.next();
    auto mix = [](unsigned long long x) {
      x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
      return x;
    };
    auto hash = [&](const std::vector<uint16_t>& q) {
      unsigned long long h = 0;
      for (size_t i = 0; i < q.size(); ++i) h += mix(((unsigned long long)i << 16) ^ q[i] ^ 0x9e3779b97f4a7c15ull);
      return h;
    };
    std::vector<uint16_t> w2 = w;
    w2[n / 2] ^= 0x0100;
    const unsigned long long want[2] = {hash(w), hash(w2)};
    v.exact_ok &= want[0] != want[1];
    if (plan) return;
    In d1, d2;
    Guarded out;
    d1.raw(w.data(), n * 2); d2.raw(w2.data(), n * 2);
    r.ins.push_back(&d1); r.ins.push_back(&d2);
    r.outb(out, 16, 0);  // the caller zeroes the sums
    if (!r.go([&] {
          unsigned long long* o = reinterpret_cast<unsigned long long*>(out.ptr());
          launch_cksum(d1.d, n * 2, o, r.st);
          launch_cksum(d2.d, n * 2, o + 1, r.st);
        }))
      return;
    v.exact_ok &= bytes_equal(out, want, 16);
    return;
  }
  if (c.op == MOVAPPLY) {
    // a table of three entries with different C, offsets into W and into the side pairs
    const int Cs[3] = {C, 8, 257};
    std::vector<MovEntry> tab(3);
    long woff = 0;
    int soff = 0, cmax = 0;
    for (int i = 0; i < 3; ++i) {
      tab[i] = MovEntry{woff, woff + Cs[i], Cs[i], soff};
      woff += 2 * Cs[i];
      soff += Cs[i];
      cmax = std::max(cmax, Cs[i]);
    }
    std::vector<float> W(woff);
    gck::fill_uni(W, seed, 0.5f, 1.0f);
    std::vector<double> s0(2 * (size_t)soff), s1(2 * (size_t)soff);
    gck::Rng rng(seed + 1);
    for (auto& q : s0) q = (double)rng.uni() + 1e-9 * (double)rng.uni();
    for (auto& q : s1) q = (double)rng.uni() * 3.0 + 1e-9 * (double)rng.uni();
    // m <- fl(m - (m - batch) 0.01) per pass, in pass order
    std::vector<float> want = W;
    auto upd = nck::moving_update;
    for (int i = 0; i < 3; ++i)
      for (int ch = 0; ch < Cs[i]; ++ch) {
        const long o = 2L * (tab[i].off + ch);
        float& mm = want[tab[i].mm + ch];
        float& mv = want[tab[i].mv + ch];
        mm = upd(mm, s0[o]); mv = upd(mv, s0[o + 1]);
        if (c.flav) { mm = upd(mm, s1[o]); mv = upd(mv, s1[o + 1]); }
      }
    if (plan) return;
    In dtab, ds0, ds1;
    Guarded out;
    dtab.raw(tab.data(), tab.size() * sizeof(MovEntry));
    ds0.raw(s0.data(), s0.size() * 8); ds1.raw(s1.data(), s1.size() * 8);
    r.ins.push_back(&dtab); r.ins.push_back(&ds0); r.ins.push_back(&ds1);
    r.outf(out, W.size(), &W);
    if (!r.go([&] {
          launch_bn_moving_apply(reinterpret_cast<const MovEntry*>(dtab.d), 3, cmax, out.ptr(),
                                 reinterpret_cast<const double*>(ds0.d),
                                 c.flav ? reinterpret_cast<const double*>(ds1.d) : nullptr, r.st);
        }))
      return;
    v.exact_ok &= bytes_equal(out, want.data(), W.size() * 4);
    return;
  }
  if (c.op == FROZEN) {
    std::vector<float> mm(C), mv(C), gamma(C);
    gck::fill_uni(mm, seed);
    gck::fill_uni(mv, seed + 1, 0.5f, 0.5f);  // [0, 1)
    mv[1] = 0.f;
    gck::fill_uni(gamma, seed + 2, 0.5f, 1.0f);
    if (plan) return;
    In dmm, dmv, dg;
    Guarded mean, rstd, sc;
    r.in(dmm, mm); r.in(dmv, mv); r.in(dg, gamma);
    r.outf(mean, C); r.outf(rstd, C); r.outf(sc, C);
    const float eps = 1e-3f;
    if (!r.go([&] { launch_bn_frozen_stats(dmm.f(), dmv.f(), mean.ptr(), rstd.ptr(), dg.f(), sc.ptr(), C, eps, r.st); })) return;
    v.exact_ok &= bytes_equal(mean, mm.data(), C * 4);
    Field f1, f2;
    for (int ch = 0; ch < C; ++ch) {  // fp64 sqrt, division, product: 4 2^-53 at the most, then the float store
      const double rs = 1.0 / std::sqrt((double)mv[ch] + (double)eps), s = rs * (double)gamma[ch];
      f1.add(F(rstd)[ch], rs, nck::fstore(rs, 4.0 * nck::kEps53 * rs), ch);
      f2.add(F(sc)[ch], s, nck::fstore(s, 6.0 * nck::kEps53 * std::fabs(s)), ch);
    }
    v.field("rstd", f1);
    v.field("sc", f2);
    return;
  }
  // BiFPN fuse
  const int nin = c.N, method = c.k;
  std::vector<float> x[3], dyv(n), prev[3], fw = {0.7f, 0.9f, 1.1f};
  if (c.flav == 1) fw[1] = -0.4f;
  if (c.flav == 2) fw[0] = 0.f;
  if (c.flav == 3) fw = {0.f, -0.5f, 0.f};
  Bn bn[3];
  cck::FuseRef fr;
  fr.nin = nin; fr.method = method; fr.act = c.act;
  for (int i = 0; i < nin; ++i) {
    x[i].resize(n);
    gck::fill_uni(x[i], seed + i);
    if (c.bf) for (auto& q : x[i]) q = gck::round_bf(q);
    bn[i].gen(C, c.act, seed + 10 + 3 * i);
    fr.w[i] = fw[i];
    fr.x[i] = i < 2 ? bn[i].view(x[i].data(), 0) : cck::BnView{x[i].data()};
  }
  gck::fill_uni(dyv, seed + 5);
  const cck::Val fv = cck::view_fuse(fr, M, C);
  gck::Reference gref[3];
  if (c.op == FUSE_B) {
    for (int k = 0; k < nin; ++k)
      if ((c.s >> k) & 1) {
        prev[k].resize(n);
        gck::fill_uni(prev[k], seed + 20 + k);
      }
    v.kink_of = (long)n;
    v.kinks = nck::fuse_bwd_ref(fr, M, C, dyv.data(), prev, gref);
  }
  if (plan) return;
  In dx[3], dfw, ddy;
  Guarded out[3];
  r.in(dfw, fw);
  InX xs[3];
  for (int i = 0; i < nin; ++i) {
    r.in(dx[i], x[i], c.bf != 0);
    if (i < 2) bn[i].up(r);
    xs[i] = i < 2 ? bn[i].inx(dx[i], 0, c.bf) : raw_inx(dx[i], c.bf);
  }
  if (c.op == FUSE_F) {
    if (c.bf) { out[0].alloc(n * 2); out[0].fill16(0x7fc0); r.outs.push_back(&out[0]); }
    else r.outf(out[0], n);
    if (!r.go([&] {
          launch_fuse_fwd(xs, nin, dfw.f(), dfw.f() + 1, dfw.f() + 2, method, c.act, out[0].ptr(), (long)n, C, r.st);
        }))
      return;
    gck::Reference ref;
    ref.c = fv.v; ref.bound = fv.e;
    if (c.bf) cck::bf_store(ref);
    const std::vector<float> ys = widen(out[0], n, c.bf != 0);
    v.field("y", nck::check_arr(ref, ys.data()));
    return;
  }
  r.in(ddy, dyv);
  float* dxs[3] = {nullptr, nullptr, nullptr};
  bool acc[3] = {false, false, false};
  for (int k = 0; k < nin; ++k) {
    acc[k] = (c.s >> k) & 1;
    r.outf(out[k], n, acc[k] ? &prev[k] : nullptr);  // an input that takes no gradient keeps its NaN fill
    if ((c.P >> k) & 1) dxs[k] = out[k].ptr();
  }
  if (!r.go([&] {
        launch_fuse_bwd(xs, nin, dfw.f(), dfw.f() + 1, dfw.f() + 2, method, c.act, ddy.f(), dxs, acc, (long)n, C, r.st);
      }))
    return;
  for (int k = 0; k < nin; ++k) {
    if ((c.P >> k) & 1) v.field(k == 0 ? "dx0" : k == 1 ? "dx1" : "dx2", nck::check_arr(gref[k], F(out[k])));
    else v.exact_ok &= out[k].got == out[k].init;
  }
}

// ---- refusals ----------------------------------------------------------------------------------
static void run_refuse(const Case& c, uint64_t seed, Rig& r, bool plan) {
  Verdict& v = r.v;
  if (plan) return;
  const int C = 8, M = 16;
  std::vector<float> h((size_t)M * 2688);
  gck::fill_uni(h, seed);
  In a, b;
  Guarded o1, o2, o3, o4, scratch;
  r.in(a, h);
  r.in(b, h);
  r.outf(o1, h.size()); r.outf(o2, 4096); r.outf(o3, 4096); r.outf(o4, 4096);
  r.outd(scratch, 65536);
  r.go([&] {
    double* sp = reinterpret_cast<double*>(scratch.ptr());
    const float* x = a.f();
    const InX xa = raw_inx(a, 0);
    InX xb = raw_inx(b, 0);
    std::vector<BnFinSeg> segs(kMaxSeg + 1);
    for (auto& s : segs) {
      s = BnFinSeg{};
      s.part = reinterpret_cast<const float2*>(a.d); s.cnt = b.f(); s.P = 4; s.M = 64;
      s.mean = o2.ptr(); s.rstd = o3.ptr(); s.gamma = x; s.sc = o4.ptr(); s.mdz = o2.ptr(); s.mdzx = o3.ptr();
    }
    const GradSink gs{reinterpret_cast<float2*>(o2.ptr()), 6, 0, x, x, x, x, x, 1, 0};
    switch (c.refuse) {
      case R_STATS_C4: launch_bn_stats(x, M, 6, sp, o2.ptr(), o3.ptr(), x, o4.ptr(), nullptr, nullptr, 1e-3f, r.st); break;
      case R_SUMS_C4: launch_bn_stats_sums(x, M, 6, sp, reinterpret_cast<double*>(o2.ptr()), r.st, false); break;
      case R_BRED_C4: launch_bn_bwd_reduce(x, x, x, x, x, x, M, 6, 1, sp, o2.ptr(), o3.ptr(), r.st); break;
      case R_APPLY_C4: launch_bn_apply(x, x, x, x, x, o1.ptr(), M, 6, 1, r.st); break;
      case R_BWD_C4: launch_bn_bwd(x, x, x, x, x, x, o1.ptr(), M, 6, 1, false, false, sp, o2.ptr(), r.st); break;
      case R_APPLY2_C4: launch_bn_bwd_apply2(GradX{x, x, x, x, x, x, x, x, 1, 0}, o1.ptr(), M, 6, r.st); break;
      case R_GRP0: launch_bn_finalize_group(segs.data(), 0, C, 1e-3f, r.st); break;
      case R_GRP6: launch_bn_finalize_group(segs.data(), kMaxSeg + 1, C, 1e-3f, r.st); break;
      case R_BGRP6: launch_bn_bwd_finalize_group(segs.data(), kMaxSeg + 1, C, r.st); break;
      case R_FOLD0: launch_bn_fold_sums(segs.data(), 0, C, false, sp, r.st); break;
      case R_SE_N: launch_se_fwd(xa, nullptr, 2, 4, 2048, 257, x, x, x, x, 1, o2.ptr(), o3.ptr(), o4.ptr(), r.st, sp); break;
      case R_SEB_N:
        launch_se_bwd(x, xa, o1.ptr(), 2, 4, 2048, 257, x, x, x, x, 1, nullptr, x, x, o2.ptr(), false, r.st, sp);
        break;
      case R_ADD_MIXED: xb.bf = 1; launch_add(xa, xb, o1.ptr(), (long)M * C, C, r.st); break;
      case R_ADD_C4: launch_add(xa, xb, o1.ptr(), (long)M * 6, 6, r.st); break;
      case R_COPY_C4: launch_copy_grad(x, o1.ptr(), (long)M * 6, false, r.st, 6); break;
      case R_COPY_TAIL: launch_copy_grad(x, o1.ptr(), (long)M * C + 2, false, r.st, C); break;
      case R_GSUMS_C4: launch_grad_sums(x, (long)M * 6, 6, gs, r.st); break;
      default: break;
    }
  });
}

static void run_case(const Case& c, uint64_t seed, hipStream_t st, bool plan, Verdict& v) {
  Rig r{st, v, {}, {}};
  switch (c.op) {
    case STATS: case STATS_SUMS: case BRED: case BRED_SUMS: case BN_BWD: run_red(c, seed, r, plan); break;
    case FIN: case BFIN: case FOLD: run_fin(c, seed, r, plan); break;
    case SE_FWD: case SE_BWD: run_se(c, seed, r, plan); break;
    case POOL: run_pool(c, seed, r, plan); break;
    case UPS: run_ups(c, seed, r, plan); break;
    case ADD: case COPYG: case GSUMS: run_ew(c, seed, r, plan); break;
    case APPLY: case APPLY2: case BF2F: case DROPK: case CKSUM: case MOVAPPLY: case FROZEN: case FUSE_F: case FUSE_B:
      run_misc(c, seed, r, plan);
      break;
    case REFUSE: run_refuse(c, seed, r, plan); break;
  }
}

static const char* tf(bool b) { return b ? "true" : "false"; }
static bool knobs_unset() {
  return !std::getenv("PHX_RED_BLOCKS") && !std::getenv("PHX_RED_DEPTH") && !std::getenv("PHX_RED_MINROWS") &&
         !std::getenv("PHX_RED_MINROWS1");
}
static std::string head(const Case& c) {
  char b[400];
  snprintf(b, sizeof b,
           "{\"case\":\"%s\",\"op\":\"%s\",\"B\":%d,\"M\":%ld,\"C\":%d,\"N\":%d,\"bf\":%d,\"act\":%d,\"flav\":%d,\"view\":%d,"
           "\"P\":%d,\"H\":%d,\"W\":%d,\"Ho\":%d,\"Wo\":%d,\"k\":%d,\"s\":%d,\"acc\":%d,\"sink\":%d,\"drop\":%d,\"refuse\":%d",
           c.name, kOpName[c.op], c.B, c.M, c.C, c.N, c.bf, c.act, c.flav, c.view, c.P, c.H, c.W, c.Ho, c.Wo, c.k, c.s,
           (int)c.acc, c.sink, c.drop, c.refuse);
  return b;
}

int main(int argc, char** argv) {
  const std::vector<Case> t = table();
  const bool plan = argc > 1 && std::string(argv[1]) == "--plan";
  if (argc > 1 && !plan) {
    fprintf(stderr, "usage: norm_parity [--plan]\n");
    return 2;
  }
  {
    std::string self = argv[0];
    const size_t sl = self.rfind('/');
    g_golden = (sl == std::string::npos ? std::string(".") : self.substr(0, sl)) + "/../golden/norm";
  }
  printf("{\"knobs_unset\":%s,\"red_depth\":%d}\n", tf(knobs_unset()), red_plan_info(1, 4, 1).depth);
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t st = nullptr;
  if (!plan) CK(hipStreamCreate(&st));
  size_t ran = 0, passed = 0;
  for (size_t i = 0; i < t.size(); ++i) {
    const Case& c = t[i];
    g_case = c.name;
    Verdict v;
    run_case(c, 1000 + 50 * i, st, plan, v);
    const double share = v.kink_of ? (double)v.kinks / (double)v.kink_of : 0.0;
    std::string line = head(c);
    if (plan) {
      line += ",\"bytes\":" + num(v.bytes) + ",\"kink_share\":" + num(share);
      if (!v.plan.empty()) line += "," + v.plan;
      line += "}";
      puts(line.c_str());
      continue;
    }
    bool ok;
    line += std::string(",\"threw\":") + tf(v.threw);
    if (v.threw) line += ",\"what\":\"" + esc(v.what) + "\"";
    if (c.refuse) {
      ok = v.threw && v.untouched && v.canary_ok && v.inputs_ok;
      line += std::string(",\"untouched\":") + tf(v.untouched);
    } else {
      ok = !v.threw && v.f.ratio <= 1.0 && v.f.nonfinite == 0 && v.exact_ok && v.canary_ok && v.repeat_ok &&
           v.inputs_ok && share <= 0.01;
      if (v.sink) ok = ok && v.P_ok && v.s.rows_written && v.s.sum_ratio <= 1.0 && v.s.m2_ratio <= 1.0;
      line += ",\"ratio\":" + num(v.f.ratio) + ",\"nonfinite\":" + std::to_string(v.f.nonfinite) + ",\"exact_ok\":" +
              tf(v.exact_ok) + ",\"canary_ok\":" + tf(v.canary_ok) + ",\"repeat_ok\":" + tf(v.repeat_ok) +
              ",\"inputs_ok\":" + tf(v.inputs_ok) + ",\"kink_share\":" + num(share) + ",\"has_sink\":" + tf(v.sink);
      if (v.sink)
        line += ",\"P_got\":" + std::to_string(v.P) + ",\"P_expected\":" + std::to_string(v.Pexp) + ",\"P_ok\":" +
                tf(v.P_ok) + ",\"rows_written\":" + tf(v.s.rows_written) + ",\"sum_ratio\":" + num(v.s.sum_ratio) +
                ",\"m2_ratio\":" + num(v.s.m2_ratio);
      std::string det = v.detail;
      if (!det.empty() && det[0] == ',') det.erase(0, 1);
      line += ",\"fields\":{" + det + "}";
    }
    line += std::string(",\"pass\":") + tf(ok) + "}";
    puts(line.c_str());
    fflush(stdout);
    ++ran;
    passed += ok;
  }
  if (!plan) CK(hipStreamDestroy(st));
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (plan) printf("{\"done\":true,\"cases\":%zu}\n", t.size());
  else printf("{\"done\":true,\"cases\":%zu,\"ran\":%zu,\"passed\":%zu,\"seconds\":%.2f}\n", t.size(), ran, passed, secs);
  fflush(stdout);
  return 0;
}
