// conv_parity — kernel-level parity of the depthwise convs (kernels_dw.hip: k_dw_fwd, k_dw_bwd, grouped
// and with the BiFPN fuse view) and the fused separable conv (kernels_sep.hip: k_sep_fwd, k_sep_bwd)
// against an fp64 host reference.
//
//   conv_parity --plan   the case table with each case's TF-SAME geometry, the tile plan the launchers
//                        choose and the sinks' partial counts, plus the share of elements under the relu6
//                        kink allowance (host code only: runs without a GPU)
//   conv_parity          run the table on the GPU: one flushed JSON line per case, then a `done` line
//
// Only the launchers of kernels.hpp are called.  The exit status is 0 when every case ran (the verdicts
// are in the lines); a HIP error ends the process at once with a `fatal` line and status 3.
// Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "conv_check.hpp"
#include "kernels.hpp"
#include "parity_dev.hpp"

using namespace phx;

// ---- the case table ----------------------------------------------------------------------------
enum Op { DW_FWD, DW_BWD, DW_FUSED, DW_FWD_GRP, DW_BWD_GRP, SEP_FWD, SEP_BWD };
enum Sink { NONE = 0, STAT = 1, GRAD = 2 };
enum ViewK { RAW = 0, BN = 1, FUSE = 2, GRADX = 3 };
enum Refuse {
  R_NONE = 0, R_C4, R_K7, R_S3, R_GRP_SINKS, R_GRP_N, R_FUSED_K5, R_SEP_C, R_SEP_N, R_SEP_GRP_FUSE, R_SEP_EMPTY,
  R_SEPB_N
};
static const char* kOpName[] = {"dw_fwd", "dw_bwd", "dw_fused", "dw_fwd_group", "dw_bwd_group", "sep_fwd", "sep_bwd"};

struct HW {
  int H, W;
};
struct Case {
  const char* name = "";
  Op op = DW_FWD;
  int B = 2, C = 64, N = 0, k = 3, s = 1;
  int view = RAW, act = 0, sink = NONE;
  int st = 0;  // storage: 1 forward on bf16 activations (x and y), 2 backward with the BN inputs y in bf16
  bool bias = false;
  int nin = 0, method = 0, neg = -1;  // fuse view: inputs, method, which weight is negative
  int small = -1;                     // dw_fused: the side of the few-workgroups switch the case was chosen for
  int n = 1;
  HW hw[kMaxSeg] = {};
  bool acc[kMaxSeg] = {false, false, false, false, false};
  int refuse = R_NONE;
};

static bool is_fwd(Op op) { return op == DW_FWD || op == DW_FUSED || op == DW_FWD_GRP || op == SEP_FWD; }
static bool is_sep(Op op) { return op == SEP_FWD || op == SEP_BWD; }

static std::vector<Case> table() {
  std::vector<Case> t;
  // depthwise forward: view RAW / BN, sink NONE / STAT
  auto fwd = [&](const char* name, int k, int s, int H, int W, int C, int view, int act, int sink, int st = 0) {
    Case c;
    c.name = name; c.op = DW_FWD; c.k = k; c.s = s; c.C = C; c.view = view; c.act = act; c.sink = sink; c.st = st;
    c.hw[0] = {H, W};
    t.push_back(c);
  };
  // depthwise data gradient: view RAW / GRADX, sink NONE / GRAD (act is also the GradSink BN's)
  auto bwd = [&](const char* name, int k, int s, int H, int W, int C, int view, int act, int sink, bool acc,
                 int st = 0) {
    Case c;
    c.name = name; c.op = DW_BWD; c.k = k; c.s = s; c.C = C; c.view = view; c.act = act; c.sink = sink; c.st = st;
    c.hw[0] = {H, W};
    c.acc[0] = acc;
    t.push_back(c);
  };
  auto fus = [&](const char* name, int B, int H, int W, int C, int nin, int method, int neg, int act, int small) {
    Case c;
    c.name = name; c.op = DW_FUSED; c.B = B; c.C = C; c.view = FUSE; c.act = act; c.nin = nin; c.method = method;
    c.neg = neg; c.small = small;
    c.hw[0] = {H, W};
    t.push_back(c);
  };
  auto grp = [&](const char* name, Op op, std::initializer_list<HW> hw, int view, int act, int sink,
                 std::initializer_list<int> acc = {}) {
    Case c;
    c.name = name; c.op = op; c.view = view; c.act = act; c.sink = sink;
    c.N = is_sep(op) ? 64 : 0;
    c.n = 0;
    for (HW x : hw) c.hw[c.n++] = x;
    int i = 0;
    for (int a : acc) c.acc[i++] = a != 0;
    t.push_back(c);
    return &t.back();
  };
  auto sepf = [&](const char* name, int H, int W, int N, int view, int act, bool bias, int sink, int nin = 0,
                  int method = 0, int neg = -1) {
    Case c;
    c.name = name; c.op = SEP_FWD; c.N = N; c.view = view; c.act = act; c.bias = bias; c.sink = sink; c.nin = nin;
    c.method = method; c.neg = neg;
    c.hw[0] = {H, W};
    t.push_back(c);
  };
  auto sepb = [&](const char* name, int H, int W, int view, int act, int sink, bool acc, int st = 0) {
    Case c;
    c.name = name; c.op = SEP_BWD; c.N = 64; c.view = view; c.act = act; c.sink = sink; c.st = st;
    c.hw[0] = {H, W};
    c.acc[0] = acc;
    t.push_back(c);
  };

  // a. k_dw_fwd 3x3 stride 1 (lcg capped at 2)
  fwd("f31_1x1_c20_raw", 3, 1, 1, 1, 20, RAW, 0, NONE);
  fwd("f31_2x2_c24_swish_stat", 3, 1, 2, 2, 24, BN, 1, STAT);
  fwd("f31_3x3_c16_relu6_stat", 3, 1, 3, 3, 16, BN, 2, STAT);
  fwd("f31_4x4_c96_bn", 3, 1, 4, 4, 96, BN, 0, NONE);
  fwd("f31_5x7_c48_raw_stat", 3, 1, 5, 7, 48, RAW, 0, STAT);
  fwd("f31_15x15_c24_swish_stat", 3, 1, 15, 15, 24, BN, 1, STAT);
  fwd("f31_16x16_c20_relu6_stat", 3, 1, 16, 16, 20, BN, 2, STAT);
  fwd("f31_30x30_c96_swish_stat", 3, 1, 30, 30, 96, BN, 1, STAT);
  fwd("f31_33x17_c48_swish_stat", 3, 1, 33, 17, 48, BN, 1, STAT);
  fwd("f31_33x17_c20_relu6", 3, 1, 33, 17, 20, BN, 2, NONE);
  fwd("f31_1x70_c48_raw_stat", 3, 1, 1, 70, 48, RAW, 0, STAT);
  fwd("f31_9x70_c48_swish_stat", 3, 1, 9, 70, 48, BN, 1, STAT);  // column tiles x row tiles
  fwd("f31_3x70_c96_swish_stat", 3, 1, 3, 70, 96, BN, 1, STAT);
  fwd("f31_8x8_c672_swish_stat", 3, 1, 8, 8, 672, BN, 1, STAT);
  fwd("f31_15x15_c24_bf_swish_stat", 3, 1, 15, 15, 24, BN, 1, STAT, 1);
  fwd("f31_33x17_c48_bf_raw", 3, 1, 33, 17, 48, RAW, 0, NONE, 1);
  // b. k_dw_fwd 3x3 stride 2 (pt = 1 on odd input, 0 on even)
  fwd("f32_1x1_c20_raw", 3, 2, 1, 1, 20, RAW, 0, NONE);
  fwd("f32_2x2_c24_swish_stat", 3, 2, 2, 2, 24, BN, 1, STAT);
  fwd("f32_3x3_c16_relu6_stat", 3, 2, 3, 3, 16, BN, 2, STAT);
  fwd("f32_4x4_c96_bn", 3, 2, 4, 4, 96, BN, 0, NONE);
  fwd("f32_5x7_c48_raw_stat", 3, 2, 5, 7, 48, RAW, 0, STAT);
  fwd("f32_15x15_c24_swish_stat", 3, 2, 15, 15, 24, BN, 1, STAT);
  fwd("f32_16x16_c20_relu6_stat", 3, 2, 16, 16, 20, BN, 2, STAT);
  fwd("f32_30x30_c96_swish_stat", 3, 2, 30, 30, 96, BN, 1, STAT);
  fwd("f32_33x17_c48_swish_stat", 3, 2, 33, 17, 48, BN, 1, STAT);
  fwd("f32_33x17_c20_relu6", 3, 2, 33, 17, 20, BN, 2, NONE);
  fwd("f32_1x140_c48_raw_stat", 3, 2, 1, 140, 48, RAW, 0, STAT);
  fwd("f32_5x67_c96_swish_stat", 3, 2, 5, 67, 96, BN, 1, STAT);
  fwd("f32_8x8_c672_swish_stat", 3, 2, 8, 8, 672, BN, 1, STAT);
  fwd("f32_15x15_c24_bf_swish_stat", 3, 2, 15, 15, 24, BN, 1, STAT, 1);
  fwd("f32_16x16_c96_bf_raw", 3, 2, 16, 16, 96, RAW, 0, NONE, 1);
  // c. k_dw_fwd 5x5 stride 1
  fwd("f51_1x1_c20_raw", 5, 1, 1, 1, 20, RAW, 0, NONE);
  fwd("f51_2x2_c24_swish_stat", 5, 1, 2, 2, 24, BN, 1, STAT);
  fwd("f51_3x3_c16_relu6_stat", 5, 1, 3, 3, 16, BN, 2, STAT);
  fwd("f51_4x4_c96_bn", 5, 1, 4, 4, 96, BN, 0, NONE);
  fwd("f51_5x7_c48_raw_stat", 5, 1, 5, 7, 48, RAW, 0, STAT);
  fwd("f51_15x15_c24_swish_stat", 5, 1, 15, 15, 24, BN, 1, STAT);
  fwd("f51_16x16_c20_relu6_stat", 5, 1, 16, 16, 20, BN, 2, STAT);
  fwd("f51_30x30_c96_swish_stat", 5, 1, 30, 30, 96, BN, 1, STAT);
  fwd("f51_33x17_c48_swish_stat", 5, 1, 33, 17, 48, BN, 1, STAT);
  fwd("f51_33x17_c20_relu6", 5, 1, 33, 17, 20, BN, 2, NONE);
  fwd("f51_1x70_c48_raw_stat", 5, 1, 1, 70, 48, RAW, 0, STAT);
  fwd("f51_9x70_c48_relu6_stat", 5, 1, 9, 70, 48, BN, 2, STAT);
  fwd("f51_8x8_c672_swish_stat", 5, 1, 8, 8, 672, BN, 1, STAT);
  fwd("f51_16x16_c24_bf_swish_stat", 5, 1, 16, 16, 24, BN, 1, STAT, 1);
  fwd("f51_33x17_c48_bf_raw", 5, 1, 33, 17, 48, RAW, 0, NONE, 1);
  // d. k_dw_fwd 5x5 stride 2 (pt = 2 on odd input, 1 on even)
  fwd("f52_1x1_c20_raw", 5, 2, 1, 1, 20, RAW, 0, NONE);
  fwd("f52_2x2_c24_swish_stat", 5, 2, 2, 2, 24, BN, 1, STAT);
  fwd("f52_3x3_c16_relu6_stat", 5, 2, 3, 3, 16, BN, 2, STAT);
  fwd("f52_4x4_c96_bn", 5, 2, 4, 4, 96, BN, 0, NONE);
  fwd("f52_5x7_c48_raw_stat", 5, 2, 5, 7, 48, RAW, 0, STAT);
  fwd("f52_15x15_c24_swish_stat", 5, 2, 15, 15, 24, BN, 1, STAT);
  fwd("f52_16x16_c20_relu6_stat", 5, 2, 16, 16, 20, BN, 2, STAT);
  fwd("f52_30x30_c96_swish_stat", 5, 2, 30, 30, 96, BN, 1, STAT);
  fwd("f52_33x17_c48_swish_stat", 5, 2, 33, 17, 48, BN, 1, STAT);
  fwd("f52_33x17_c20_relu6", 5, 2, 33, 17, 20, BN, 2, NONE);
  fwd("f52_1x140_c48_raw_stat", 5, 2, 1, 140, 48, RAW, 0, STAT);
  fwd("f52_5x67_c96_swish_stat", 5, 2, 5, 67, 96, BN, 1, STAT);
  fwd("f52_8x8_c672_swish_stat", 5, 2, 8, 8, 672, BN, 1, STAT);
  fwd("f52_15x15_c24_bf_swish_stat", 5, 2, 15, 15, 24, BN, 1, STAT, 1);
  fwd("f52_16x16_c96_bf_raw", 5, 2, 16, 16, 96, RAW, 0, NONE, 1);

  // e. k_dw_bwd 3x3 stride 1 (H, W: the conv input = the gradient written; lcg up to 3)
  bwd("b31_1x1_c20_raw", 3, 1, 1, 1, 20, RAW, 0, NONE, false);
  bwd("b31_2x2_c24_gx_swish_gs", 3, 1, 2, 2, 24, GRADX, 1, GRAD, false);
  bwd("b31_3x3_c16_gx_relu6_gs_acc", 3, 1, 3, 3, 16, GRADX, 2, GRAD, true);
  bwd("b31_4x4_c96_gx_acc", 3, 1, 4, 4, 96, GRADX, 0, NONE, true);
  bwd("b31_5x7_c48_raw_gs", 3, 1, 5, 7, 48, RAW, 1, GRAD, false);
  bwd("b31_15x15_c24_gx_swish_gs", 3, 1, 15, 15, 24, GRADX, 1, GRAD, false);
  bwd("b31_16x16_c20_gx_relu6", 3, 1, 16, 16, 20, GRADX, 2, NONE, false);
  bwd("b31_30x30_c96_gx_swish_gs_acc", 3, 1, 30, 30, 96, GRADX, 1, GRAD, true);
  bwd("b31_33x17_c48_gx_swish_gs", 3, 1, 33, 17, 48, GRADX, 1, GRAD, false);
  bwd("b31_33x17_c20_gx_relu6_acc", 3, 1, 33, 17, 20, GRADX, 2, NONE, true);
  bwd("b31_1x70_c48_raw_gs", 3, 1, 1, 70, 48, RAW, 0, GRAD, false);
  bwd("b31_9x70_c48_gx_swish_gs", 3, 1, 9, 70, 48, GRADX, 1, GRAD, false);
  bwd("b31_3x70_c96_gx_swish_gs", 3, 1, 3, 70, 96, GRADX, 1, GRAD, false);
  bwd("b31_8x8_c672_gx_swish_gs", 3, 1, 8, 8, 672, GRADX, 1, GRAD, false);
  bwd("b31_15x15_c24_ybf_gx_swish_gs", 3, 1, 15, 15, 24, GRADX, 1, GRAD, false, 2);
  bwd("b31_33x17_c48_ybf_gx_relu6_acc", 3, 1, 33, 17, 48, GRADX, 2, NONE, true, 2);
  // f. k_dw_bwd 3x3 stride 2: (H parity, k) -> pt, both branches of the window origin's floor
  bwd("b32_1x1_c20_raw", 3, 2, 1, 1, 20, RAW, 0, NONE, false);
  bwd("b32_2x2_c24_gx_swish_gs", 3, 2, 2, 2, 24, GRADX, 1, GRAD, false);
  bwd("b32_3x3_c16_gx_relu6_gs_acc", 3, 2, 3, 3, 16, GRADX, 2, GRAD, true);
  bwd("b32_4x4_c96_gx_acc", 3, 2, 4, 4, 96, GRADX, 0, NONE, true);
  bwd("b32_5x7_c48_raw_gs", 3, 2, 5, 7, 48, RAW, 1, GRAD, false);
  bwd("b32_15x15_c24_gx_swish_gs", 3, 2, 15, 15, 24, GRADX, 1, GRAD, false);
  bwd("b32_16x16_c20_gx_relu6", 3, 2, 16, 16, 20, GRADX, 2, NONE, false);
  bwd("b32_30x30_c96_gx_swish_gs_acc", 3, 2, 30, 30, 96, GRADX, 1, GRAD, true);
  bwd("b32_33x17_c48_gx_swish_gs", 3, 2, 33, 17, 48, GRADX, 1, GRAD, false);
  bwd("b32_33x17_c20_gx_relu6_acc", 3, 2, 33, 17, 20, GRADX, 2, NONE, true);
  bwd("b32_1x70_c48_raw_gs", 3, 2, 1, 70, 48, RAW, 0, GRAD, false);
  bwd("b32_6x35_c96_gx_swish_gs", 3, 2, 6, 35, 96, GRADX, 1, GRAD, false);
  bwd("b32_8x8_c672_gx_swish_gs", 3, 2, 8, 8, 672, GRADX, 1, GRAD, false);
  bwd("b32_15x15_c24_ybf_gx_swish_gs", 3, 2, 15, 15, 24, GRADX, 1, GRAD, false, 2);
  bwd("b32_16x16_c96_ybf_gx_relu6_acc", 3, 2, 16, 16, 96, GRADX, 2, NONE, true, 2);
  // g. k_dw_bwd 5x5 stride 1 (lcg capped at 2)
  bwd("b51_1x1_c20_raw", 5, 1, 1, 1, 20, RAW, 0, NONE, false);
  bwd("b51_2x2_c24_gx_swish_gs", 5, 1, 2, 2, 24, GRADX, 1, GRAD, false);
  bwd("b51_3x3_c16_gx_relu6_gs_acc", 5, 1, 3, 3, 16, GRADX, 2, GRAD, true);
  bwd("b51_4x4_c96_gx_acc", 5, 1, 4, 4, 96, GRADX, 0, NONE, true);
  bwd("b51_5x7_c48_raw_gs", 5, 1, 5, 7, 48, RAW, 1, GRAD, false);
  bwd("b51_15x15_c24_gx_swish_gs", 5, 1, 15, 15, 24, GRADX, 1, GRAD, false);
  bwd("b51_16x16_c20_gx_relu6", 5, 1, 16, 16, 20, GRADX, 2, NONE, false);
  bwd("b51_30x30_c96_gx_swish_gs_acc", 5, 1, 30, 30, 96, GRADX, 1, GRAD, true);
  bwd("b51_33x17_c48_gx_swish_gs", 5, 1, 33, 17, 48, GRADX, 1, GRAD, false);
  bwd("b51_33x17_c20_gx_relu6_acc", 5, 1, 33, 17, 20, GRADX, 2, NONE, true);
  bwd("b51_1x70_c48_raw_gs", 5, 1, 1, 70, 48, RAW, 0, GRAD, false);
  bwd("b51_9x70_c48_gx_relu6_gs_acc", 5, 1, 9, 70, 48, GRADX, 2, GRAD, true);
  bwd("b51_8x8_c672_gx_swish_gs", 5, 1, 8, 8, 672, GRADX, 1, GRAD, false);
  bwd("b51_16x16_c24_ybf_gx_swish_gs", 5, 1, 16, 16, 24, GRADX, 1, GRAD, false, 2);
  bwd("b51_33x17_c48_ybf_gx_relu6_acc", 5, 1, 33, 17, 48, GRADX, 2, NONE, true, 2);
  // h. k_dw_bwd 5x5 stride 2
  bwd("b52_1x1_c20_raw", 5, 2, 1, 1, 20, RAW, 0, NONE, false);
  bwd("b52_2x2_c24_gx_swish_gs", 5, 2, 2, 2, 24, GRADX, 1, GRAD, false);
  bwd("b52_3x3_c16_gx_relu6_gs_acc", 5, 2, 3, 3, 16, GRADX, 2, GRAD, true);
  bwd("b52_4x4_c96_gx_acc", 5, 2, 4, 4, 96, GRADX, 0, NONE, true);
  bwd("b52_5x7_c48_raw_gs", 5, 2, 5, 7, 48, RAW, 1, GRAD, false);
  bwd("b52_15x15_c24_gx_swish_gs", 5, 2, 15, 15, 24, GRADX, 1, GRAD, false);
  bwd("b52_16x16_c20_gx_relu6", 5, 2, 16, 16, 20, GRADX, 2, NONE, false);
  bwd("b52_30x30_c96_gx_swish_gs_acc", 5, 2, 30, 30, 96, GRADX, 1, GRAD, true);
  bwd("b52_33x17_c48_gx_swish_gs", 5, 2, 33, 17, 48, GRADX, 1, GRAD, false);
  bwd("b52_33x17_c20_gx_relu6_acc", 5, 2, 33, 17, 20, GRADX, 2, NONE, true);
  bwd("b52_1x70_c48_raw_gs", 5, 2, 1, 70, 48, RAW, 0, GRAD, false);
  bwd("b52_9x70_c48_gx_swish_gs", 5, 2, 9, 70, 48, GRADX, 1, GRAD, false);
  bwd("b52_8x8_c672_gx_swish_gs", 5, 2, 8, 8, 672, GRADX, 1, GRAD, false);
  bwd("b52_15x15_c24_ybf_gx_swish_gs", 5, 2, 15, 15, 24, GRADX, 1, GRAD, false, 2);
  bwd("b52_16x16_c96_ybf_gx_relu6_acc", 5, 2, 16, 16, 96, GRADX, 2, NONE, true, 2);

  // i. launch_dw_fwd_fused: both sides of the few-workgroups switch (the large side needs 512
  // workgroups of at least 33 x 4 pixels x 16 channels: B 4 here, the one case above the size cap)
  fus("fused_4x4_n2_m0_swish", 2, 4, 4, 64, 2, 0, 0, 1, 1);
  fus("fused_4x4_n3_m1_relu6", 2, 4, 4, 64, 3, 1, -1, 2, 1);
  fus("fused_8x8_n3_m0_swish", 2, 8, 8, 64, 3, 0, 1, 1, 1);
  fus("fused_8x8_n2_m1_swish", 2, 8, 8, 64, 2, 1, -1, 1, 1);
  fus("fused_8x8_n3_m0_relu6", 2, 8, 8, 64, 3, 0, 2, 2, 1);
  fus("fused_9x5_c20_n2_m0_relu6", 2, 9, 5, 20, 2, 0, 1, 2, 1);
  fus("fused_125x33_n3_m0_swish_large", 4, 125, 33, 64, 3, 0, 1, 1, 0);
  fus("fused_124x33_n2_m0_relu6_below", 4, 124, 33, 64, 2, 0, -1, 2, 1);

  // j. grouped depthwise (C 64, 3x3 stride 1): the head's levels of a 128^2 image, non-zero everywhere
  grp("gf5_swish_stat", DW_FWD_GRP, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, BN, 1, STAT);
  grp("gf5_raw", DW_FWD_GRP, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, RAW, 0, NONE);
  grp("gf3_relu6_stat", DW_FWD_GRP, {{20, 12}, {5, 3}, {1, 1}}, BN, 2, STAT);
  // (the levels of a 320^2 image: members with different tile counts, so nps[i] differ)
  grp("gf5_40_bn_stat", DW_FWD_GRP, {{40, 40}, {20, 20}, {10, 10}, {5, 5}, {3, 3}}, BN, 0, STAT);
  grp("gb5_40_gx_swish_gs_acc", DW_BWD_GRP, {{40, 40}, {20, 20}, {10, 10}, {5, 5}, {3, 3}}, GRADX, 1, GRAD, {0, 1, 0, 1, 1});
  grp("gb5_gx_swish_gs_acc", DW_BWD_GRP, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, GRADX, 1, GRAD, {1, 0, 1, 0, 1});
  grp("gb5_gx_relu6_acc", DW_BWD_GRP, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, GRADX, 2, NONE, {0, 1, 0, 1, 0});
  grp("gb3_gx_swish_gs_acc", DW_BWD_GRP, {{20, 12}, {5, 3}, {1, 1}}, GRADX, 1, GRAD, {0, 1, 1});
  grp("gb3_raw_gs", DW_BWD_GRP, {{20, 12}, {5, 3}, {1, 1}}, RAW, 0, GRAD);

  // k. k_sep_fwd (C 64): tiles 16 x 8 (W > 8), 8 x 16 (W 5..8), 4 x 16 (W <= 4); N 64, 36, 8, 1
  sepf("sf_1x1_n64_raw_bias_stat", 1, 1, 64, RAW, 0, true, STAT);
  sepf("sf_4x4_n36_swish_bias_stat", 4, 4, 36, BN, 1, true, STAT);
  sepf("sf_4x4_n1_bn_stat", 4, 4, 1, BN, 0, false, STAT);
  sepf("sf_5x8_n8_relu6_stat", 5, 8, 8, BN, 2, false, STAT);
  sepf("sf_8x8_n1_bn_bias", 8, 8, 1, BN, 0, true, NONE);
  sepf("sf_8x8_n64_fuse2_m1_relu6", 8, 8, 64, FUSE, 2, false, NONE, 2, 1, -1);
  sepf("sf_9x9_n64_swish_stat", 9, 9, 64, BN, 1, false, STAT);
  sepf("sf_9x9_n8_relu6_bias_stat", 9, 9, 8, BN, 2, true, STAT);
  sepf("sf_16x8_n36_raw_bias", 16, 8, 36, RAW, 0, true, NONE);
  sepf("sf_17x8_n64_swish_stat", 17, 8, 64, BN, 1, false, STAT);
  sepf("sf_17x3_n64_swish_bias_stat", 17, 3, 64, BN, 1, true, STAT);
  sepf("sf_17x33_n64_swish_bias_stat", 17, 33, 64, BN, 1, true, STAT);
  sepf("sf_17x33_n36_fuse3_m0_swish_bias_stat", 17, 33, 36, FUSE, 1, true, STAT, 3, 0, 1);
  sepf("sf_33x17_n8_fuse2_m0_swish", 33, 17, 8, FUSE, 1, false, NONE, 2, 0, 0);
  grp("sf_g5_n64_swish_bias_stat", SEP_FWD, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, BN, 1, STAT)->bias = true;
  {
    Case* c = grp("sf_g5_n36_relu6", SEP_FWD, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, BN, 2, NONE);
    c->N = 36;
  }
  grp("sf_g3_n64_raw_stat", SEP_FWD, {{20, 12}, {5, 3}, {1, 1}}, RAW, 0, STAT);

  // l. k_sep_bwd (C = N = 64)
  sepb("sb_1x1_gx_swish_gs", 1, 1, GRADX, 1, GRAD, false);
  sepb("sb_4x4_gx_relu6_gs_acc", 4, 4, GRADX, 2, GRAD, true);
  sepb("sb_5x8_raw_acc", 5, 8, RAW, 0, NONE, true);
  sepb("sb_8x8_gx_swish_gs", 8, 8, GRADX, 1, GRAD, false);
  sepb("sb_9x9_gx_relu6", 9, 9, GRADX, 2, NONE, false);
  sepb("sb_9x8_gx_swish_gs_acc", 9, 8, GRADX, 1, GRAD, true);
  sepb("sb_16x8_raw_gs", 16, 8, RAW, 1, GRAD, false);
  sepb("sb_17x7_gx_swish_gs", 17, 7, GRADX, 1, GRAD, false);
  sepb("sb_17x3_gx_bn_gs", 17, 3, GRADX, 0, GRAD, false);
  sepb("sb_17x33_gx_swish_gs_acc", 17, 33, GRADX, 1, GRAD, true);
  sepb("sb_17x33_gx_relu6", 17, 33, GRADX, 2, NONE, false);
  sepb("sb_9x9_ybf_gx_swish_gs", 9, 9, GRADX, 1, GRAD, false, 2);
  grp("sb_g5_gx_swish_gs_acc", SEP_BWD, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, GRADX, 1, GRAD, {1, 0, 1, 0, 1});
  grp("sb_g5_gx_relu6", SEP_BWD, {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}}, GRADX, 2, NONE, {0, 1, 0, 1, 0});
  grp("sb_g3_raw_gs", SEP_BWD, {{20, 12}, {5, 3}, {1, 1}}, RAW, 0, GRAD);

  // m. argument refusals: the launcher throws, nothing is launched, every output keeps its fill
  auto ref = [&](const char* name, Op op, int refuse, int n = 1) {
    Case c;
    c.name = name; c.op = op; c.refuse = refuse; c.n = n;
    c.C = refuse == R_C4 ? 20 : 64;
    c.N = is_sep(op) ? 64 : 0;
    c.view = op == DW_FUSED ? FUSE : RAW;
    c.nin = op == DW_FUSED ? 2 : 0;
    c.sink = (refuse == R_GRP_SINKS) ? STAT : NONE;
    for (int i = 0; i < n; ++i) c.hw[i] = {std::max(8 >> i, 1), std::max(8 >> i, 1)};
    t.push_back(c);
  };
  ref("refuse_c_mod4", DW_FWD, R_C4);
  ref("refuse_k7", DW_FWD, R_K7);
  ref("refuse_stride3", DW_BWD, R_S3);
  ref("refuse_group_sinks_differ", DW_FWD_GRP, R_GRP_SINKS, 3);
  ref("refuse_group_six_members", DW_BWD_GRP, R_GRP_N, 5);
  ref("refuse_fused_k5", DW_FUSED, R_FUSED_K5);
  ref("refuse_sep_c32", SEP_FWD, R_SEP_C);
  ref("refuse_sep_n96", SEP_FWD, R_SEP_N);
  ref("refuse_sep_grouped_fuse", SEP_FWD, R_SEP_GRP_FUSE, 2);
  ref("refuse_sep_empty_member", SEP_FWD, R_SEP_EMPTY, 2);
  ref("refuse_sep_bwd_n32", SEP_BWD, R_SEPB_N);
  return t;
}
// ---- end of the table --------------------------------------------------------------------------

static cck::Geo geo_of(const Case& c, int i) {
  return cck::make_geo(c.B, c.hw[i].H, c.hw[i].W, c.C, c.k, c.s);
}
// the partial rows the host-side planners promise member i's sink
static int partials_of(const Case& c, int i) {
  const cck::Geo g = geo_of(c, i);
  if (is_sep(c.op)) return sep_stat_partials(c.B, g.H, g.W);
  if (is_fwd(c.op)) return dw_stat_partials(c.B, g.H, g.W, g.C, g.Ho, g.Wo, g.k, g.s, g.pt, g.pl);
  return dw_bwd_partials(c.B, g.H, g.W, g.C, g.Ho, g.Wo, g.k, g.s, g.pt, g.pl);
}

// ---- inputs (host) -----------------------------------------------------------------------------
struct Mem {
  cck::Geo g;
  bool acc = false;
  int Pexp = 0;
  std::vector<float> x[3];               // forward: the view's inputs [B][H][W][C]
  std::vector<float> da, yv, prev, y2;   // backward: gradient and BN input [B][Ho][Wo][Cg], old dx, GradSink y
  Dev dx[3], dda, dyv, dy2;
  Guarded out, part, cnt;
};
struct Shared {
  std::vector<float> w, bt, wp, bias, fw;
  std::vector<float> mu[3], sc[3], be[3];                  // forward views
  std::vector<float> gmu, grstd, gsc, gbe, gmdz, gmdzx;    // gradient view
  std::vector<float> smu, srstd, ssc, sbe;                 // GradSink's BN
  Dev dw_, dbt, dwp, dbias, dfw, dmu[3], dsc[3], dbe[3], dgmu, dgrstd, dgsc, dgbe, dgmdz, dgmdzx, dsmu, dsrstd, dssc,
      dsbe;
};
static int out_ch(const Case& c) { return c.op == SEP_FWD ? c.N : c.C; }   // channels of the tensor written
static int grad_ch(const Case& c) { return c.op == SEP_BWD ? c.N : c.C; }  // channels of the gradient read

// per-channel BN parameters, all distinct; sc of both signs; relu6 views reach z < 0 and z > 6, swish
// views both sides of 0 (gemm_parity's recipe)
static void bn_params(int n, int act, uint64_t seed, std::vector<float>& mu, std::vector<float>& sc,
                      std::vector<float>& be, int flip) {
  mu.resize(n); sc.resize(n); be.resize(n);
  gck::fill_uni(mu, seed, 0.3f);
  gck::fill_uni(sc, seed + 1, act == 2 ? 3.5f : 0.5f, act == 2 ? 4.5f : 1.0f);
  for (int k = 0; k < n; ++k) if (k % 3 == flip) sc[k] = -sc[k];
  gck::fill_uni(be, seed + 2, act == 2 ? 3.0f : 0.5f, act == 2 ? 2.0f : 0.0f);
}

static void gen_shared(const Case& c, uint64_t seed, Shared& s) {
  const int C = c.C, N = std::max(c.N, 1), G = grad_ch(c);
  s.w.resize((size_t)c.k * c.k * C);
  gck::fill_uni(s.w, seed + 1);
  s.bt.resize((size_t)N * C);
  gck::fill_uni(s.bt, seed + 2);
  s.wp.resize((size_t)C * N);
  gck::fill_uni(s.wp, seed + 3);
  s.bias.resize(N);
  gck::fill_uni(s.bias, seed + 4);
  // (a fuse's inputs are BN outputs without activation — the fuse applies it — scaled as the activation
  // needs; its third input is a raw tensor)
  for (int i = 0; i < 3; ++i) bn_params(C, c.act, seed + 10 + 3 * i, s.mu[i], s.sc[i], s.be[i], i);
  s.fw = {0.7f, 0.9f, 1.1f};
  if (c.neg >= 0) s.fw[c.neg] = -0.4f;
  bn_params(G, c.act, seed + 20, s.gmu, s.gsc, s.gbe, 1);
  s.grstd.resize(G); s.gmdz.resize(G); s.gmdzx.resize(G);
  gck::fill_uni(s.grstd, seed + 23, 0.5f, 1.0f);
  gck::fill_uni(s.gmdz, seed + 24, 0.1f);
  gck::fill_uni(s.gmdzx, seed + 25, 0.1f);
  bn_params(C, c.act, seed + 30, s.smu, s.ssc, s.sbe, 2);
  s.srstd.resize(C);
  gck::fill_uni(s.srstd, seed + 33, 0.5f, 1.0f);
}

static void round_bf_all(std::vector<float>& v) {
  for (auto& x : v) x = gck::round_bf(x);
}

static void gen_member(const Case& c, int i, uint64_t seed, Mem& m) {
  m.g = geo_of(c, i);
  m.acc = c.acc[i];
  const cck::Geo& g = m.g;
  if (is_fwd(c.op)) {
    const int nx = c.view == FUSE ? c.nin : 1;
    for (int j = 0; j < nx; ++j) {
      m.x[j].resize((size_t)g.in_px() * g.C);
      gck::fill_uni(m.x[j], seed + 1 + j);
      if (c.st == 1) round_bf_all(m.x[j]);
    }
  } else {
    const size_t ng = (size_t)g.out_px() * grad_ch(c);
    m.da.resize(ng);
    gck::fill_uni(m.da, seed + 5);
    if (c.view == GRADX) {
      m.yv.resize(ng);
      gck::fill_uni(m.yv, seed + 6);
      if (c.st == 2) round_bf_all(m.yv);
    }
    if (m.acc) {
      m.prev.resize((size_t)g.in_px() * g.C);
      gck::fill_uni(m.prev, seed + 7);
    }
    if (c.sink == GRAD) {
      m.y2.resize((size_t)g.in_px() * g.C);
      gck::fill_uni(m.y2, seed + 8);
      if (c.st == 2) round_bf_all(m.y2);
    }
  }
}

// ---- the fp64 reference of one member ----------------------------------------------------------
struct RefOut {
  gck::Reference r;
  long kinks = 0, kink_of = 0;  // elements under the relu6 kink allowance, of how many
};
static RefOut reference(const Case& c, const Shared& s, const Mem& m) {
  RefOut o;
  const cck::Geo& g = m.g;
  if (is_fwd(c.op)) {
    cck::Val a;
    if (c.view == FUSE) {
      cck::FuseRef f;
      f.nin = c.nin; f.method = c.method; f.act = c.act;
      for (int i = 0; i < c.nin; ++i) {
        f.w[i] = s.fw[i];
        f.x[i].x = m.x[i].data();
        f.x[i].act = 0;
        if (i < 2) { f.x[i].mu = s.mu[i].data(); f.x[i].sc = s.sc[i].data(); f.x[i].be = s.be[i].data(); }
      }
      a = cck::view_fuse(f, g.in_px(), g.C);
    } else {
      cck::BnView b;
      b.x = m.x[0].data();
      b.act = c.act;
      if (c.view == BN) { b.mu = s.mu[0].data(); b.sc = s.sc[0].data(); b.be = s.be[0].data(); }
      a = cck::view_inx(b, g.in_px(), g.C);
    }
    o.r = cck::dw_fwd_ref(g, a, s.w.data());
    if (c.op == SEP_FWD) o.r = cck::pw_fwd_ref(o.r, g.out_px(), g.C, c.N, s.bt.data(), c.bias ? s.bias.data() : nullptr);
    if (c.st == 1) cck::bf_store(o.r);
    return o;
  }
  cck::GradRef gr;
  gr.da = m.da.data();
  gr.act = c.act;
  if (c.view == GRADX) {
    gr.y = m.yv.data(); gr.mu = s.gmu.data(); gr.rstd = s.grstd.data(); gr.sc = s.gsc.data(); gr.be = s.gbe.data();
    gr.mdz = s.gmdz.data(); gr.mdzx = s.gmdzx.data();
  }
  cck::Val gy = cck::view_grad(gr, g.out_px(), grad_ch(c));
  o.kinks = gy.kinks;
  o.kink_of = (long)gy.v.size();
  if (c.op == SEP_BWD) gy = cck::pw_bwd_ref(gy, g.out_px(), c.N, g.C, s.wp.data());
  o.r = cck::dw_bwd_ref(g, gy, s.w.data(), m.acc ? m.prev.data() : nullptr);
  if (c.sink == GRAD) {
    o.kinks += cck::gradsink_kinks(m.y2.data(), g.in_px(), g.C, s.smu.data(), s.ssc.data(), s.sbe.data(), c.act);
    o.kink_of += (long)m.y2.size();
  }
  return o;
}

// ---- --plan ------------------------------------------------------------------------------------
static void print_plan(const Case& c, uint64_t seed, FILE* f) {
  std::string mem;
  double elems = 0;
  long kinks = 0, kink_of = 0;
  Shared s;
  gen_shared(c, seed, s);
  for (int i = 0; i < c.n; ++i) {
    const cck::Geo g = geo_of(c, i);
    elems += (double)g.in_px() * g.C;
    char b[512];
    int len = snprintf(b, sizeof b, "%s{\"H\":%d,\"W\":%d,\"Ho\":%d,\"Wo\":%d,\"pt\":%d,\"pl\":%d,\"acc\":%d,\"P\":%d",
                       i ? "," : "", g.H, g.W, g.Ho, g.Wo, g.pt, g.pl, (int)c.acc[i], partials_of(c, i));
    if (is_sep(c.op)) {
      const SepTileInfo t = sep_tile_info(g.H, g.W);
      len += snprintf(b + len, sizeof b - len, ",\"tw\":%d,\"th\":%d,\"tiles_x\":%d,\"ntiles\":%d", t.tw, t.th, t.tiles_x,
                      t.ntiles);
    } else {
      const DwTileInfo t = c.op == DW_FUSED ? dw_fused_tile_info(c.B, g.H, g.W, g.C, g.Ho, g.Wo, g.pt, g.pl)
                                            : dw_tile_info(g.H, g.W, g.C, g.Ho, g.Wo, g.pt, g.pl, g.k, g.s, !is_fwd(c.op));
      len += snprintf(b + len, sizeof b - len,
                      ",\"lcg\":%d,\"rpt\":%d,\"otw\":%d,\"oth\":%d,\"nrg\":%d,\"rin\":%d,\"cin\":%d,\"tiles_x\":%d,"
                      "\"ntiles\":%d,\"ncg\":%d,\"small\":%d,\"wgs\":%ld",
                      t.lcg, t.rpt, t.otw, t.oth, t.nrg, t.rin, t.cin, t.tiles_x, t.ntiles, t.ncg, t.small, t.wgs);
    }
    snprintf(b + len, sizeof b - len, "}");
    mem += b;
    if (!c.refuse && !is_fwd(c.op) && c.act == 2) {  // the reference alone stays inside the kink allowance's share
      Mem m;
      gen_member(c, i, seed + 100 * (i + 1), m);
      const RefOut o = reference(c, s, m);
      kinks += o.kinks;
      kink_of += o.kink_of;
    }
  }
  fprintf(f,
          "{\"case\":\"%s\",\"op\":\"%s\",\"B\":%d,\"C\":%d,\"N\":%d,\"k\":%d,\"s\":%d,\"view\":%d,\"act\":%d,\"sink\":%d,"
          "\"st\":%d,\"bias\":%d,\"nin\":%d,\"method\":%d,\"neg\":%d,\"expect_small\":%d,\"n\":%d,\"refuse\":%d,"
          "\"elems\":%.0f,\"kink_share\":%.3g,\"members\":[%s]}\n",
          c.name, kOpName[c.op], c.B, c.C, c.N, c.k, c.s, c.view, c.act, c.sink, c.st, (int)c.bias, c.nin, c.method, c.neg,
          c.small, c.n, c.refuse, elems, kink_of ? (double)kinks / (double)kink_of : 0.0, mem.c_str());
  fflush(f);
}

// ---- device side -------------------------------------------------------------------------------
static void upload_shared(Shared& s) {
  put_f(s.dw_, s.w); put_f(s.dbt, s.bt); put_f(s.dwp, s.wp); put_f(s.dbias, s.bias); put_f(s.dfw, s.fw);
  for (int i = 0; i < 3; ++i) { put_f(s.dmu[i], s.mu[i]); put_f(s.dsc[i], s.sc[i]); put_f(s.dbe[i], s.be[i]); }
  put_f(s.dgmu, s.gmu); put_f(s.dgrstd, s.grstd); put_f(s.dgsc, s.gsc); put_f(s.dgbe, s.gbe);
  put_f(s.dgmdz, s.gmdz); put_f(s.dgmdzx, s.gmdzx);
  put_f(s.dsmu, s.smu); put_f(s.dsrstd, s.srstd); put_f(s.dssc, s.ssc); put_f(s.dsbe, s.sbe);
}

static void put_st(Dev& d, std::vector<float>& v, bool bf) {
  if (bf) put_bf(d, v);  // (already rounded: exact)
  else put_f(d, v);
}

static void upload_member(const Case& c, Mem& m, int Pexp) {
  const cck::Geo& g = m.g;
  m.Pexp = Pexp;
  const bool obf = is_fwd(c.op) && c.st == 1;
  const size_t on = (size_t)(is_fwd(c.op) ? g.out_px() : g.in_px()) * out_ch(c);
  m.out.alloc(on * (obf ? 2 : 4));
  if (is_fwd(c.op)) {
    for (int j = 0; j < 3; ++j)
      if (!m.x[j].empty()) put_st(m.dx[j], m.x[j], c.st == 1);
    if (obf) m.out.fill16(0x7fc0);
    else m.out.fill32(0x7fc00000u);
  } else {
    put_f(m.dda, m.da);
    if (!m.yv.empty()) put_st(m.dyv, m.yv, c.st == 2);
    if (!m.y2.empty()) put_st(m.dy2, m.y2, c.st == 2);
    if (m.acc) std::memcpy(m.out.fill(), m.prev.data(), on * 4);
    else m.out.fill32(0x7fc00000u);
  }
  if (c.sink) {
    m.part.alloc((size_t)out_ch(c) * Pexp * 8);
    m.part.fill32(gck::kUnwritten);
    m.cnt.alloc((size_t)Pexp * 4);
    m.cnt.fill32(gck::kUnwritten);
  }
}

static InX view_in(const Case& c, const Shared& s, const Mem& m, int j) {
  const bool v = c.view == BN || (c.view == FUSE && j < 2);
  return InX{m.dx[j].f(), v ? s.dmu[j].f() : nullptr, v ? s.dsc[j].f() : nullptr, v ? s.dbe[j].f() : nullptr,
             c.view == FUSE ? 0 : c.act, c.st == 1 ? 1 : 0};
}
static FuseView view_fuse(const Case& c, const Shared& s, const Mem& m) {
  FuseView f{};
  for (int j = 0; j < 3; ++j) {
    f.x[j] = j < c.nin ? view_in(c, s, m, j) : view_in(c, s, m, 0);  // (an unused slot holds a valid view)
    f.w[j] = s.dfw.f() + j;
  }
  f.nin = c.nin;
  f.method = c.method;
  f.act = c.act;
  return f;
}
static GradX view_grad(const Case& c, const Shared& s, const Mem& m) {
  if (c.view != GRADX) return GradX{m.dda.f(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  return GradX{m.dda.f(), m.dyv.f(), s.dgmu.f(), s.dgrstd.f(), s.dgsc.f(), s.dgbe.f(), s.dgmdz.f(), s.dgmdzx.f(), c.act,
               c.st == 2 ? 1 : 0};
}
static StatSink stat_sink(const Case& c, const Mem& m) {
  if (c.sink != STAT) return StatSink{};
  return StatSink{reinterpret_cast<float2*>(m.part.ptr()), m.cnt.ptr(), out_ch(c), 0};
}
static GradSink grad_sink(const Case& c, const Shared& s, const Mem& m) {
  if (c.sink != GRAD) return GradSink{};
  return GradSink{reinterpret_cast<float2*>(m.part.ptr()), c.C, 0, m.dy2.f(), s.dsmu.f(), s.dsrstd.f(), s.dssc.f(),
                  s.dsbe.f(), c.act, c.st == 2 ? 1 : 0};
}

struct Verdict {
  bool threw = false;
  std::string what;
  bool P_ok = true, canary_ok = true, repeat_ok = true, untouched = true;
  int P = 0, Pexp = 0;
  gck::CCheck c;
  gck::SinkCheck s;
  long kinks = 0, kink_of = 0;
  double ref_ms = 0;
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

// what the device stored, widened to float
static std::vector<float> out_floats(const Case& c, const Mem& m) {
  const bool obf = is_fwd(c.op) && c.st == 1;
  const size_t n = m.out.n / (obf ? 2 : 4);
  std::vector<float> out(n);
  if (obf) {
    for (size_t i = 0; i < n; ++i) {
      uint16_t h;
      std::memcpy(&h, m.out.out() + 2 * i, 2);
      out[i] = gck::bf2f(h);
    }
  } else {
    std::memcpy(out.data(), m.out.out(), n * 4);
  }
  return out;
}

static void check_member(const Case& c, const Shared& s, Mem& m, int P, Verdict& v) {
  m.out.download();
  v.canary_ok &= m.out.intact();
  const std::vector<float> out = out_floats(c, m);
  const auto t0 = std::chrono::steady_clock::now();
  const RefOut ref = reference(c, s, m);
  v.ref_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  v.kinks += ref.kinks;
  v.kink_of += ref.kink_of;
  const gck::CCheck cc = gck::check_c(ref.r, out.data(), (long)out.size());
  gck::SinkCheck sc;
  if (c.sink) {
    m.part.download();
    m.cnt.download();
    v.canary_ok &= m.part.intact() && m.cnt.intact();
    const long rows = is_fwd(c.op) ? m.g.out_px() : m.g.in_px();
    if (P != m.Pexp) {
      v.P_ok = false;  // the partials are laid out with another pitch: not read
    } else if (c.sink == STAT) {
      sc = gck::check_statsink(out.data(), rows, out_ch(c), reinterpret_cast<const float*>(m.part.out()),
                               reinterpret_cast<const float*>(m.cnt.out()), P);
    } else {
      sc = gck::check_gradsink(out.data(), rows, c.C, m.y2.data(), s.smu.data(), s.srstd.data(), s.ssc.data(),
                               s.sbe.data(), c.act, reinterpret_cast<const float*>(m.part.out()), P, true);
    }
  }
  merge(v, cc, sc);
}

static Verdict run_case(const Case& c, uint64_t seed, hipStream_t st) {
  Verdict v;
  const int n = c.n;
  Shared s;
  gen_shared(c, seed, s);
  upload_shared(s);
  std::vector<Mem> ms(n);
  for (int i = 0; i < n; ++i) {
    gen_member(c, i, seed + 100 * (i + 1), ms[i]);
    upload_member(c, ms[i], partials_of(c, i));
  }
  v.Pexp = ms[0].Pexp;
  std::vector<int> Pout(kMaxSeg + 1, 0);

  auto launch = [&]() {
    for (auto& m : ms) {
      m.out.upload();
      if (c.sink) {
        m.part.upload();
        m.cnt.upload();
      }
    }
    const cck::Geo& g = ms[0].g;
    int C = c.C, N = c.N, k = c.k, stride = c.s;
    if (c.refuse == R_C4) C = 18;
    if (c.refuse == R_K7) k = 7;
    if (c.refuse == R_S3) stride = 3;
    if (c.refuse == R_FUSED_K5) k = 5;
    if (c.refuse == R_SEP_C) C = 32;
    if (c.refuse == R_SEP_N) N = 96;
    if (c.refuse == R_SEPB_N) N = 32;
    switch (c.op) {
      case DW_FWD:
        Pout[0] = launch_dw_fwd(view_in(c, s, ms[0], 0), s.dw_.f(), ms[0].out.ptr(), c.B, g.H, g.W, C, g.Ho, g.Wo, k,
                                stride, g.pt, g.pl, st, stat_sink(c, ms[0]));
        break;
      case DW_BWD:
        Pout[0] = launch_dw_bwd(view_grad(c, s, ms[0]), s.dw_.f(), ms[0].out.ptr(), c.B, g.H, g.W, C, g.Ho, g.Wo, k,
                                stride, g.pt, g.pl, ms[0].acc, st, grad_sink(c, s, ms[0]));
        break;
      case DW_FUSED:
        launch_dw_fwd_fused(view_fuse(c, s, ms[0]), s.dw_.f(), ms[0].out.ptr(), c.B, g.H, g.W, C, g.Ho, g.Wo, k, stride,
                            g.pt, g.pl, st);
        break;
      case DW_FWD_GRP:
      case DW_BWD_GRP: {
        std::vector<DwSeg> segs(kMaxSeg + 1);
        for (int i = 0; i <= kMaxSeg; ++i) {
          const Mem& m = ms[std::min(i, n - 1)];
          segs[i] = DwSeg{c.op == DW_FWD_GRP ? view_in(c, s, m, 0) : InX{}, c.op == DW_BWD_GRP ? view_grad(c, s, m) : GradX{},
                          m.out.ptr(), m.g.H, m.g.W, m.g.Ho, m.g.Wo, m.g.pt, m.g.pl, m.acc, stat_sink(c, m),
                          grad_sink(c, s, m)};
        }
        if (c.refuse == R_GRP_SINKS) segs[1].sink = StatSink{};
        const int nn = c.refuse == R_GRP_N ? kMaxSeg + 1 : n;
        if (c.op == DW_FWD_GRP) launch_dw_fwd_group(segs.data(), nn, c.B, C, s.dw_.f(), k, stride, st, Pout.data());
        else launch_dw_bwd_group(segs.data(), nn, c.B, C, s.dw_.f(), k, stride, st, Pout.data());
        break;
      }
      case SEP_FWD: {
        std::vector<SepMember> mem(n);
        for (int i = 0; i < n; ++i) {
          const Mem& m = ms[i];
          const bool fuse = c.view == FUSE || c.refuse == R_SEP_GRP_FUSE;
          mem[i] = SepMember{view_in(c, s, m, 0), c.view == FUSE ? view_fuse(c, s, m) : FuseView{}, fuse, m.out.ptr(),
                             m.g.H, m.g.W, stat_sink(c, m)};
        }
        if (c.refuse == R_SEP_EMPTY) mem[1].H = 0;
        launch_sep_fwd(mem.data(), n, c.B, C, N, s.dw_.f(), s.dbt.f(), c.bias ? s.dbias.f() : nullptr, st, Pout.data());
        break;
      }
      case SEP_BWD: {
        std::vector<SepBwdMember> mem(n);
        for (int i = 0; i < n; ++i)
          mem[i] = SepBwdMember{view_grad(c, s, ms[i]), ms[i].out.ptr(), ms[i].g.H, ms[i].g.W, ms[i].acc,
                                grad_sink(c, s, ms[i])};
        launch_sep_bwd(mem.data(), n, c.B, C, N, s.dw_.f(), s.dwp.f(), st, Pout.data());
        break;
      }
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
  }
  if (v.threw || c.refuse) {
    // an argument refusal launches nothing: every output still holds its fill
    CK(hipStreamSynchronize(st));
    CK(hipGetLastError());
    for (auto& m : ms) {
      m.out.download();
      v.untouched &= m.out.got == m.out.init;
      if (c.sink) {
        m.part.download();
        m.cnt.download();
        v.untouched &= m.part.got == m.part.init && m.cnt.got == m.cnt.init;
      }
    }
    return v;
  }
  v.P = Pout[0];
  for (int i = 0; i < n; ++i) check_member(c, s, ms[i], c.sink ? Pout[i] : 0, v);
  // repeatability: a second launch from the same initial state leaves the same bits
  std::vector<std::vector<uint8_t>> keep;
  for (auto& m : ms) {
    keep.push_back(m.out.got);
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
    m.out.download();
    v.repeat_ok &= m.out.got == keep[q++];
    if (c.sink) {
      m.part.download();
      m.cnt.download();
      v.repeat_ok &= m.part.got == keep[q] && m.cnt.got == keep[q + 1];
    }
    q += 2;
  }
  return v;
}

static const char* tf(bool b) { return b ? "true" : "false"; }

int main(int argc, char** argv) {
  const std::vector<Case> t = table();
  if (argc > 1 && std::string(argv[1]) == "--plan") {
    for (size_t i = 0; i < t.size(); ++i) print_plan(t[i], 1000 + 50 * i, stdout);
    printf("{\"done\":true,\"cases\":%zu}\n", t.size());
    return 0;
  }
  if (argc > 1) {
    fprintf(stderr, "usage: conv_parity [--plan]\n");
    return 2;
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t st;
  CK(hipStreamCreate(&st));
  size_t ran = 0, passed = 0;
  for (size_t i = 0; i < t.size(); ++i) {
    const Case& c = t[i];
    g_case = c.name;
    const Verdict v = run_case(c, 1000 + 50 * i, st);
    bool ok;
    std::string line = std::string("{\"case\":\"") + c.name + "\",\"op\":\"" + kOpName[c.op] + "\",\"refuse\":" +
                       std::to_string(c.refuse) + ",\"threw\":" + tf(v.threw);
    if (v.threw) line += ",\"what\":\"" + esc(v.what) + "\"";
    if (c.refuse) {
      ok = v.threw && v.untouched;
      line += std::string(",\"untouched\":") + tf(v.untouched);
    } else {
      const double share = v.kink_of ? (double)v.kinks / (double)v.kink_of : 0.0;
      ok = !v.threw && v.c.ratio <= 1.0 && v.c.nonfinite == 0 && v.canary_ok && v.repeat_ok && share <= 0.01;
      if (c.sink)
        ok = ok && v.P_ok && v.s.rows_written && v.s.sum_ratio <= 1.0 && v.s.m2_ratio <= 1.0 &&
             (c.sink != STAT || (v.s.cnt_ok && v.s.cnt_sum_ok));
      line += ",\"c_ratio\":" + num(v.c.ratio) + ",\"c_nonfinite\":" + std::to_string(v.c.nonfinite) +
              ",\"c_worst\":" + std::to_string(v.c.worst) + ",\"c_worst_err\":" + num(v.c.worst_err) +
              ",\"c_worst_bound\":" + num(v.c.worst_bound) + ",\"canary_ok\":" + tf(v.canary_ok) +
              ",\"repeat_ok\":" + tf(v.repeat_ok) + ",\"kink_share\":" + num(share) + ",\"sink\":" +
              std::to_string(c.sink) + ",\"ref_ms\":" + num(v.ref_ms);
      if (c.sink)
        line += ",\"P\":" + std::to_string(v.P) + ",\"P_expected\":" + std::to_string(v.Pexp) + ",\"P_ok\":" +
                tf(v.P_ok) + ",\"rows_written\":" + tf(v.s.rows_written) + ",\"cnt_ok\":" + tf(v.s.cnt_ok) +
                ",\"cnt_sum_ok\":" + tf(v.s.cnt_sum_ok) + ",\"sum_ratio\":" + num(v.s.sum_ratio) +
                ",\"m2_ratio\":" + num(v.s.m2_ratio);
    }
    line += std::string(",\"pass\":") + tf(ok) + "}";
    puts(line.c_str());
    fflush(stdout);
    ++ran;
    passed += ok;
  }
  CK(hipStreamDestroy(st));
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("{\"done\":true,\"cases\":%zu,\"ran\":%zu,\"passed\":%zu,\"seconds\":%.2f}\n", t.size(), ran, passed, secs);
  fflush(stdout);
  return 0;
}
