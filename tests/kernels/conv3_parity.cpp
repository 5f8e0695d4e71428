// conv3_parity — kernel-level parity of the dense 3x3 convolutions against an fp64 host reference: the
// stem (kernels_conv.hip: k_stem_fwd, k_stem_bwd, k_stem_bwd_gx), the GEMM over an implicitly gathered
// column matrix (launch_gemm_gather, k_gemm2 MODE 4) and the U-Net's conv kernels (kernels_unet.hip:
// un_im2col, un_wprep, un_conv3_small, un_wgrad).
//
//   conv3_parity --plan   the case table with each case's geometry and what the host planners return (the
//                         stem's blocks and tiles, k_conv3_small's grid and XCD ranges, the weight gradient's
//                         slices, the gather GEMM's plans), plus the share of elements under the relu6 kink
//                         allowance (host code only: runs without a GPU)
//   conv3_parity          run the table on the GPU: one flushed JSON line per case, then a `done` line
//
// Only the launchers of kernels.hpp and unet.hpp are called.  The exit status is 0 when every case ran
// (the verdicts are in the lines); a HIP error ends the process at once with a `fatal` line and status 3.
// Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "conv3_check.hpp"
#include "kernels.hpp"
#include "parity_dev.hpp"
#include "unet.hpp"

using namespace phx;
using c3k::pad4;

// ---- the case table ----------------------------------------------------------------------------
enum Op { STEM_FWD, STEM_BWD, STEM_GX, IM2COL, WPREP, CONV3, GATHER, WGRAD };
static const char* kOpName[] = {"stem_fwd", "stem_bwd", "stem_gx", "im2col", "wprep", "conv3", "gather", "wgrad"};
enum Refuse {
  R_NONE = 0, R_STEM_ODD_H, R_STEM_ODD_W, R_STEM_PT, R_STEM_CO36, R_GX_CO56, R_GX_CO64, R_CV_N33, R_CV_KP292,
  R_CV_KP_SHORT, R_CV_KP_MOD4, R_GG_W15, R_GG_C3, R_GG_K, R_GG_ALIGN, R_WG_ODD_H, R_WG_M
};
enum Own { OWN_NULL = 0, OWN_NONE, OWN_LAST_ELEM, OWN_EDGE_QUAD, OWN_ALL };

struct Case {
  const char* name = "";
  Op op = STEM_FWD;
  int B = 1, H = 2, W = 2, C = 3, N = 32;  // N: output channels (the stem's Co, the weight gradient's Co)
  int gk = 0;                              // c3k::make_gather's kind
  bool sink = false, ybf = false, acc = false, bias = false, mis = false, tconv = false;
  int act = 0, own = OWN_NULL;
  int kind = 0, src = 0, ldy = 0;
  int refuse = R_NONE;
};

static std::vector<Case> table() {
  std::vector<Case> t;
  auto sf = [&](const char* name, int B, int H, int W, int Co, bool sink, bool ybf) {
    Case c;
    c.name = name; c.op = STEM_FWD; c.B = B; c.H = H; c.W = W; c.N = Co; c.sink = sink; c.ybf = ybf;
    t.push_back(c);
  };
  auto sb = [&](const char* name, int B, int H, int W, int Co, bool acc) {
    Case c;
    c.name = name; c.op = STEM_BWD; c.B = B; c.H = H; c.W = W; c.N = Co; c.acc = acc;
    t.push_back(c);
  };
  auto gx = [&](const char* name, int H, int W, int Co, int act, bool ybf, int own) {
    Case c;
    c.name = name; c.op = STEM_GX; c.B = 2; c.H = H; c.W = W; c.N = Co; c.act = act; c.ybf = ybf; c.own = own;
    t.push_back(c);
  };
  auto ic = [&](const char* name, int gk, int B, int H, int W, int C) {
    Case c;
    c.name = name; c.op = IM2COL; c.gk = gk; c.B = B; c.H = H; c.W = W; c.C = C;
    t.push_back(c);
  };
  auto wp = [&](const char* name, int kind, int ci, int co) {
    Case c;
    c.name = name; c.op = WPREP; c.kind = kind; c.C = ci; c.N = co;
    t.push_back(c);
  };
  // a forward (conv: gather 0; tconv: gather 2) over x [B][H][W][C] to N channels, and its data gradient
  auto cv = [&](const char* name, bool tconv, int B, int H, int W, int C, int N, bool bias, bool mis = false) {
    Case c;
    c.name = name; c.op = CONV3; c.tconv = tconv; c.gk = tconv ? 2 : 0; c.B = B; c.H = H; c.W = W; c.C = C; c.N = N;
    c.bias = bias; c.mis = mis;
    t.push_back(c);
  };
  auto gg = [&](const char* name, int gk, int B, int H, int W, int C, int N) {
    Case c;
    c.name = name; c.op = GATHER; c.gk = gk; c.B = B; c.H = H; c.W = W; c.C = C; c.N = N; c.bias = true;
    t.push_back(c);
  };
  // rows = the B H W pixels; src 0: x [rows][C] (a 1x1 conv's input), kind 4; src 1: kind 0; src 2: kind 2
  auto wg = [&](const char* name, int src, int B, int H, int W, int C, int Co, int ldy = 0, bool mis = false) {
    Case c;
    c.name = name; c.op = WGRAD; c.src = src; c.kind = src == 0 ? 4 : src == 1 ? 0 : 2; c.B = B; c.H = H; c.W = W;
    c.C = C; c.N = Co; c.ldy = ldy ? ldy : Co; c.mis = mis;
    t.push_back(c);
  };
  auto ref = [&](const char* name, Op op, int refuse) {
    Case c;
    c.name = name; c.op = op; c.refuse = refuse;
    c.B = 1; c.H = 8; c.W = 8; c.C = 4; c.N = 32;
    if (op == STEM_FWD || op == STEM_BWD || op == STEM_GX) { c.H = 6; c.W = 10; c.C = 3; c.sink = op == STEM_FWD; }
    if (op == GATHER) c.N = 40;
    if (op == WGRAD) { c.src = 2; c.kind = 2; c.C = 6; c.N = 8; c.ldy = 8; c.H = 6; c.W = 6; }
    if (op == CONV3) c.bias = true;
    t.push_back(c);
  };

  // a. k_stem_fwd: every Co at (1,2,2) one pixel, (1,2,514) 257 rows (the last block holds one), (3,6,10) one
  // partial block, (2,34,30) two blocks with 254 rows in the last; with / without the sink, fp32 / bf16 storage
  sf("sf_c32_1x2x2_stat", 1, 2, 2, 32, true, false);
  sf("sf_c32_1x2x514_stat", 1, 2, 514, 32, true, false);
  sf("sf_c32_3x6x10", 3, 6, 10, 32, false, false);
  sf("sf_c32_2x34x30_bf_stat", 2, 34, 30, 32, true, true);
  sf("sf_c32_3x6x10_bf", 3, 6, 10, 32, false, true);
  sf("sf_c40_1x2x2", 1, 2, 2, 40, false, false);
  sf("sf_c40_1x2x514_bf_stat", 1, 2, 514, 40, true, true);
  sf("sf_c40_3x6x10_stat", 3, 6, 10, 40, true, false);
  sf("sf_c40_2x34x30_stat", 2, 34, 30, 40, true, false);
  sf("sf_c40_2x34x30_bf", 2, 34, 30, 40, false, true);
  sf("sf_c48_1x2x2_bf_stat", 1, 2, 2, 48, true, true);
  sf("sf_c48_1x2x514_stat", 1, 2, 514, 48, true, false);
  sf("sf_c48_3x6x10_bf_stat", 3, 6, 10, 48, true, true);
  sf("sf_c48_2x34x30", 2, 34, 30, 48, false, false);
  sf("sf_c48_1x2x514_bf", 1, 2, 514, 48, false, true);
  sf("sf_c56_1x2x2_stat", 1, 2, 2, 56, true, false);
  sf("sf_c56_1x2x514_stat", 1, 2, 514, 56, true, false);
  sf("sf_c56_3x6x10_bf", 3, 6, 10, 56, false, true);
  sf("sf_c56_2x34x30_bf_stat", 2, 34, 30, 56, true, true);
  sf("sf_c56_2x34x30", 2, 34, 30, 56, false, false);
  sf("sf_c64_1x2x2_bf", 1, 2, 2, 64, false, true);
  sf("sf_c64_1x2x514_bf_stat", 1, 2, 514, 64, true, true);
  sf("sf_c64_3x6x10_stat", 3, 6, 10, 64, true, false);
  sf("sf_c64_2x34x30_stat", 2, 34, 30, 64, true, false);
  sf("sf_c64_1x2x514", 1, 2, 514, 64, false, false);
  // b. k_stem_bwd (materialised dy): (1,2,2) has all three neighbour dy pixels out of range
  sb("sb_c32_1x2x2", 1, 2, 2, 32, false);
  sb("sb_c32_2x34x30_acc", 2, 34, 30, 32, true);
  sb("sb_c32_3x6x10", 3, 6, 10, 32, false);
  sb("sb_c40_1x2x2_acc", 1, 2, 2, 40, true);
  sb("sb_c40_2x34x30", 2, 34, 30, 40, false);
  sb("sb_c40_3x6x10_acc", 3, 6, 10, 40, true);
  sb("sb_c48_1x2x2", 1, 2, 2, 48, false);
  sb("sb_c48_2x34x30_acc", 2, 34, 30, 48, true);
  sb("sb_c48_3x6x10", 3, 6, 10, 48, false);
  sb("sb_c56_1x2x2_acc", 1, 2, 2, 56, true);
  sb("sb_c56_2x34x30", 2, 34, 30, 56, false);
  sb("sb_c56_3x6x10_acc", 3, 6, 10, 56, true);
  sb("sb_c64_1x2x2", 1, 2, 2, 64, false);
  sb("sb_c64_2x34x30_acc", 2, 34, 30, 64, true);
  sb("sb_c64_3x6x10", 3, 6, 10, 64, false);
  // c. k_stem_bwd_gx: 34 x 34 = 2 x 2 tiles, the last of one quad row / column; 66 x 34 = 3 x 2 tiles.
  // The contract is per 32 x 32-pixel tile: a tile with no owned element is +0.0 everywhere (its dy / y NaN
  // here wherever no live tile reads them), a tile with any owned element holds the full gradient
  gx("gx_c32_34_swish_null", 34, 34, 32, 1, false, OWN_NULL);
  gx("gx_c32_34_relu6_none", 34, 34, 32, 2, false, OWN_NONE);
  gx("gx_c32_34_swish_last_elem", 34, 34, 32, 1, false, OWN_LAST_ELEM);
  gx("gx_c32_34_relu6_edge_quad", 34, 34, 32, 2, false, OWN_EDGE_QUAD);
  gx("gx_c32_66x34_raw_all", 66, 34, 32, 0, false, OWN_ALL);
  gx("gx_c32_66x34_swish_ybf_edge_quad", 66, 34, 32, 1, true, OWN_EDGE_QUAD);
  gx("gx_c40_34_raw_null", 34, 34, 40, 0, false, OWN_NULL);
  gx("gx_c40_34_swish_ybf_none", 34, 34, 40, 1, true, OWN_NONE);
  gx("gx_c40_34_relu6_ybf_last_elem", 34, 34, 40, 2, true, OWN_LAST_ELEM);
  gx("gx_c40_66x34_swish_edge_quad", 66, 34, 40, 1, false, OWN_EDGE_QUAD);
  gx("gx_c40_66x34_relu6_all", 66, 34, 40, 2, false, OWN_ALL);
  gx("gx_c48_34_relu6_ybf_null", 34, 34, 48, 2, true, OWN_NULL);
  gx("gx_c48_34_raw_none", 34, 34, 48, 0, false, OWN_NONE);
  gx("gx_c48_34_raw_last_elem", 34, 34, 48, 0, false, OWN_LAST_ELEM);
  gx("gx_c48_66x34_relu6_edge_quad", 66, 34, 48, 2, false, OWN_EDGE_QUAD);
  gx("gx_c48_66x34_swish_ybf_all", 66, 34, 48, 1, true, OWN_ALL);
  // d. un_im2col: C 1 / 3 / 6 / 8 (Kp 12 / 28 / 56 / 72), odd and non-square, the three gathers
  ic("ic_s1_c1_7x5", 0, 2, 7, 5, 1);
  ic("ic_s1_c3_5x9", 0, 1, 5, 9, 3);
  ic("ic_s1_c6_7x5", 0, 2, 7, 5, 6);
  ic("ic_s1_c8_3x11", 0, 1, 3, 11, 8);
  ic("ic_s2_c1_10x6", 1, 1, 10, 6, 1);
  ic("ic_s2_c3_6x14", 1, 2, 6, 14, 3);
  ic("ic_s2_c6_7x5", 1, 1, 7, 5, 6);
  ic("ic_s2_c8_10x6", 1, 2, 10, 6, 8);
  ic("ic_t_c1_3x5", 2, 2, 3, 5, 1);
  ic("ic_t_c3_7x5", 2, 1, 7, 5, 3);
  ic("ic_t_c6_5x3", 2, 2, 5, 3, 6);
  ic("ic_t_c8_3x7", 2, 1, 3, 7, 8);
  ic("ic_s1_c64_2x48x48_gridstride", 0, 2, 48, 48, 64);  // > 8192 * 256 column elements
  // e. un_wprep: every kind, ci != co, Kp padded
  wp("wp_k0_3_5", 0, 3, 5);
  wp("wp_k1_3_5", 1, 3, 5);
  wp("wp_k2_3_5", 2, 3, 5);
  wp("wp_k3_3_5", 3, 3, 5);
  wp("wp_k4_3_5", 4, 3, 5);
  wp("wp_k5_3_5", 5, 3, 5);
  wp("wp_k0_6_17", 0, 6, 17);
  wp("wp_k1_6_17", 1, 6, 17);
  wp("wp_k2_17_6", 2, 17, 6);
  wp("wp_k3_17_6", 3, 17, 6);
  wp("wp_k4_6_17", 4, 6, 17);
  wp("wp_k5_17_6", 5, 17, 6);
  // f. un_conv3_small: a forward and its wprep'd data gradient.  Rows M = 48 (one workgroup, one idle wave),
  // 448 (G 7: no XCD ranges), 520 (G 9, XCD 7's range empty), 675 (G 11, ragged last tile, second sweeps)
  cv("cv_c3_n3_1x6x8_bias", false, 1, 6, 8, 3, 3, true);
  cv("cv_c4_n16_1x6x8", false, 1, 6, 8, 4, 16, false);
  cv("cv_c6_n17_1x16x28_bias", false, 1, 16, 28, 6, 17, true);
  cv("cv_c8_n32_2x14x16", false, 2, 14, 16, 8, 32, false);
  cv("cv_c32_n16_1x20x26_bias", false, 1, 20, 26, 32, 16, true);
  cv("cv_c3_n32_1x20x26", false, 1, 20, 26, 3, 32, false);
  cv("cv_c8_n3_3x15x15_bias", false, 3, 15, 15, 8, 3, true);
  cv("cv_c32_n32_3x15x15_bias", false, 3, 15, 15, 32, 32, true);
  cv("cv_c6_n16_3x15x15", false, 3, 15, 15, 6, 16, false);
  cv("cv_c4_n17_3x15x15_bias", false, 3, 15, 15, 4, 17, true);
  cv("cv_c8_n16_1x20x26_misaligned", false, 1, 20, 26, 8, 16, true, true);
  cv("cvt_c3_n3_1x3x4_bias", true, 1, 3, 4, 3, 3, true);
  cv("cvt_c4_n16_1x8x14", true, 1, 8, 14, 4, 16, false);
  cv("cvt_c6_n17_1x10x13_bias", true, 1, 10, 13, 6, 17, true);
  cv("cvt_c8_n32_1x10x13", true, 1, 10, 13, 8, 32, false);
  cv("cvt_c32_n16_1x8x14_bias", true, 1, 8, 14, 32, 16, true);
  cv("cvt_c32_n32_3x5x9_bias", true, 3, 5, 9, 32, 32, true);
  cv("cvt_c3_n17_3x5x9", true, 3, 5, 9, 3, 17, false);
  cv("cvt_c4_n32_1x10x13_misaligned", true, 1, 10, 13, 4, 32, false, true);
  // g. launch_gemm_gather against un_im2col + the plain GEMM, bit for bit (H, W: the gather's input)
  gg("gg_s1_c4_n40_4x16x16", 0, 4, 16, 16, 4, 40);
  gg("gg_s1_c64_n64_4x16x16", 0, 4, 16, 16, 64, 64);
  gg("gg_s1_c128_n128_4x16x16", 0, 4, 16, 16, 128, 128);
  gg("gg_s1_c64_n128_2x8x32", 0, 2, 8, 32, 64, 128);
  gg("gg_s1_c4_n64_2x32x8", 0, 2, 32, 8, 4, 64);
  gg("gg_s2_c4_n128_4x32x32", 1, 4, 32, 32, 4, 128);
  gg("gg_s2_c64_n40_4x16x64", 1, 4, 16, 64, 64, 40);
  gg("gg_s2_c128_n64_2x64x16", 1, 2, 64, 16, 128, 64);
  gg("gg_t_c4_n40_2x16x4", 2, 2, 16, 4, 4, 40);
  gg("gg_t_c64_n128_4x8x8", 2, 4, 8, 8, 64, 128);
  gg("gg_t_c128_n64_2x4x16", 2, 2, 4, 16, 128, 64);
  gg("gg_t_c64_n64_8x8x8", 2, 8, 8, 8, 64, 64);
  // h. un_wgrad.  src 0: the 1x1 convs (Co 1 with ldy 1: the attention gate; Co 3: the output layer)
  wg("wg0_c8_co1_ldy1_3x15x15", 0, 3, 15, 15, 8, 1, 1);
  wg("wg0_c16_co3_3x15x15", 0, 3, 15, 15, 16, 3);
  wg("wg0_c8_co16_1x3x3", 0, 1, 3, 3, 8, 16);
  wg("wg0_c6_co16_scalar_2x22x24", 0, 2, 22, 24, 6, 16);
  wg("wg0_c8_co3_misaligned_3x15x15", 0, 3, 15, 15, 8, 3, 0, true);
  wg("wg0_c16_co12_ldy20_2x22x24", 0, 2, 22, 24, 16, 12, 20);
  wg("wg1_c3_co16_1x3x3", 1, 1, 3, 3, 3, 16);
  wg("wg1_c3_co17_3x15x15", 1, 3, 15, 15, 3, 17);
  wg("wg1_c8_co17_3x15x15", 1, 3, 15, 15, 8, 17);
  wg("wg1_c16_co40_2x22x24", 1, 2, 22, 24, 16, 40);
  wg("wg1_c64_co40_3x15x15", 1, 3, 15, 15, 64, 40);
  wg("wg1_c64_co3_1x3x3", 1, 1, 3, 3, 64, 3);
  wg("wg1_c8_co16_2x48x48_fold65", 1, 2, 48, 48, 8, 16);  // 72 slices: k_wgrad_fold's unrolled loop
  wg("wg1_c16_co17_misaligned_2x22x24", 1, 2, 22, 24, 16, 17, 0, true);
  wg("wg2_c6_co16_2x22x24", 2, 2, 22, 24, 6, 16);
  wg("wg2_c16_co3_1x2x4", 2, 1, 2, 4, 16, 3);
  wg("wg2_c16_co17_3x14x16", 2, 3, 14, 16, 16, 17);
  wg("wg2_c6_co40_1x26x26", 2, 1, 26, 26, 6, 40);
  // i. refusals: the launcher throws or returns false, nothing is launched, every output keeps its fill
  ref("refuse_stem_odd_h", STEM_FWD, R_STEM_ODD_H);
  ref("refuse_stem_odd_w", STEM_BWD, R_STEM_ODD_W);
  ref("refuse_stem_pt1", STEM_FWD, R_STEM_PT);
  ref("refuse_stem_co36", STEM_FWD, R_STEM_CO36);
  ref("refuse_gx_co56", STEM_GX, R_GX_CO56);
  ref("refuse_gx_co64", STEM_GX, R_GX_CO64);
  ref("refuse_cv_n33", CONV3, R_CV_N33);
  ref("refuse_cv_kp292", CONV3, R_CV_KP292);
  ref("refuse_cv_kp_below_9c", CONV3, R_CV_KP_SHORT);
  ref("refuse_cv_kp_mod4", CONV3, R_CV_KP_MOD4);
  ref("refuse_gg_w15", GATHER, R_GG_W15);
  ref("refuse_gg_c3", GATHER, R_GG_C3);
  ref("refuse_gg_k_not_9c", GATHER, R_GG_K);
  ref("refuse_gg_misaligned", GATHER, R_GG_ALIGN);
  ref("refuse_wg_src2_odd_h", WGRAD, R_WG_ODD_H);
  ref("refuse_wg_rows", WGRAD, R_WG_M);
  return t;
}
// ---- end of the table --------------------------------------------------------------------------

// ---- device buffers ----------------------------------------------------------------------------
struct In {  // an input: what was uploaded is kept, to show the launch left it alone
  uint8_t* d = nullptr;
  size_t off = 0;
  std::vector<uint8_t> h;
  In() = default;
  In(const In&) = delete;
  In& operator=(const In&) = delete;
  ~In() { if (d) (void)hipFree(d); }
  void put(const void* p, size_t bytes, size_t offset = 0) {
    off = offset;
    h.assign((const uint8_t*)p, (const uint8_t*)p + bytes);
    CK(hipMalloc(reinterpret_cast<void**>(&d), std::max<size_t>(bytes, 16) + 16));
    if (bytes) CK(hipMemcpy(d + off, p, bytes, hipMemcpyHostToDevice));
  }
  const float* f() const { return reinterpret_cast<const float*>(d + off); }
  bool same() const {
    std::vector<uint8_t> g(h.size());
    if (!g.empty()) CK(hipMemcpy(g.data(), d + off, g.size(), hipMemcpyDeviceToHost));
    return g == h;
  }
};

struct Verdict {
  bool threw = false, refused = false, untouched = true;
  std::string what;
  double ratio = 0.0;
  long nonfinite = 0;
  std::vector<std::pair<std::string, double>> fields;
  bool exact_ok = true, canary_ok = true, repeat_ok = true, inputs_ok = true, agree_ok = true;
  long kinks = 0, kink_of = 0;
  bool has_sink = false, P_ok = true;
  int P = 0, Pexp = 0;
  gck::SinkCheck s;
  double ref_ms = 0;
  void take(const char* name, const gck::CCheck& c) {
    ratio = std::max(ratio, c.ratio);
    nonfinite += c.nonfinite;
    fields.emplace_back(name, c.ratio);
  }
};

struct Job {
  std::vector<std::unique_ptr<In>> ins;
  std::vector<std::unique_ptr<Guarded>> outs;
  std::function<bool()> launch;          // false: the launcher returned false (refused)
  std::function<void(Verdict&)> check;   // after the outputs were downloaded
  In* in(const std::vector<float>& v, bool mis = false) {
    ins.emplace_back(new In);
    ins.back()->put(v.data(), v.size() * 4, mis ? 4 : 0);
    return ins.back().get();
  }
  In* in_bf(std::vector<float>& v) {  // rounds v in place to the stored values
    std::vector<uint16_t> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) {
      h[i] = gck::f2bf(v[i]);
      v[i] = gck::bf2f(h[i]);
    }
    ins.emplace_back(new In);
    ins.back()->put(h.data(), h.size() * 2);
    return ins.back().get();
  }
  Guarded* out(size_t bytes, uint32_t fill = 0x7fc00000u) {
    outs.emplace_back(new Guarded);
    outs.back()->alloc(bytes);
    outs.back()->fill32(fill);
    return outs.back().get();
  }
};
static const float* of(const Guarded* g) { return reinterpret_cast<const float*>(g->out()); }

static std::vector<float> uni(size_t n, uint64_t seed, float scale = 1.f, float shift = 0.f) {
  std::vector<float> v(n);
  gck::fill_uni(v, seed, scale, shift);
  return v;
}
// per-channel BN parameters, all distinct; sc of both signs; relu6 views reach z < 0 and z > 6, swish views
// both sides of 0 (gemm_parity's recipe)
static void bn_params(int n, int act, uint64_t seed, std::vector<float>& mu, std::vector<float>& sc,
                      std::vector<float>& be) {
  mu = uni(n, seed, 0.3f);
  sc = uni(n, seed + 1, act == 2 ? 3.5f : 0.5f, act == 2 ? 4.5f : 1.0f);
  for (int k = 0; k < n; ++k) if (k % 3 == 1) sc[k] = -sc[k];
  be = uni(n, seed + 2, act == 2 ? 3.0f : 0.5f, act == 2 ? 2.0f : 0.0f);
}

// ---- host inputs of the stem's gradient-view cases (shared with --plan) ---------------------------
struct GxHost {
  std::vector<float> da, y, mu, rstd, sc, be, mdz, mdzx, w;
  std::vector<int16_t> owner;
  bool has_owner = false;
};
static GxHost gen_gx(const Case& c, uint64_t seed) {
  GxHost h;
  const int Co = c.N, Ho = c.H / 2, Wo = c.W / 2;
  const size_t n = (size_t)c.B * Ho * Wo * Co;
  h.da = uni(n, seed + 1);
  h.y = uni(n, seed + 2);
  if (c.ybf) for (auto& v : h.y) v = gck::round_bf(v);
  bn_params(Co, c.act, seed + 3, h.mu, h.sc, h.be);
  h.rstd = uni(Co, seed + 6, 0.5f, 1.0f);
  h.mdz = uni(Co, seed + 7, 0.1f);
  h.mdzx = uni(Co, seed + 8, 0.1f);
  h.w = uni((size_t)27 * Co, seed + 9, 0.3f);
  h.has_owner = c.own != OWN_NULL;
  if (h.has_owner) {
    h.owner.assign((size_t)c.B * c.H * c.W * 3, c.own == OWN_ALL ? 0 : -1);
    auto at = [&](int b, int iy, int ix, int ch) -> int16_t& { return h.owner[(((size_t)b * c.H + iy) * c.W + ix) * 3 + ch]; };
    // the last of the six elements a quad's scan of its second row reads, in the corner tile of the last image
    if (c.own == OWN_LAST_ELEM) at(c.B - 1, c.H - 1, c.W - 1, 2) = 7;
    // one whole quad in the ragged right-edge tile of the first tile row (quad row 5, the last quad column)
    if (c.own == OWN_EDGE_QUAD)
      for (int a = 0; a < 2; ++a)
        for (int e = 0; e < 2; ++e)
          for (int ch = 0; ch < 3; ++ch) at(0, 10 + a, c.W - 2 + e, ch) = 3;
  }
  return h;
}
static cck::Val gx_view(const Case& c, const GxHost& h) {
  cck::GradRef gr;
  gr.da = h.da.data();
  gr.act = c.act;
  if (c.act) {
    gr.y = h.y.data(); gr.mu = h.mu.data(); gr.rstd = h.rstd.data(); gr.sc = h.sc.data(); gr.be = h.be.data();
    gr.mdz = h.mdz.data(); gr.mdzx = h.mdzx.data();
  }
  return cck::view_grad(gr, (long)c.B * (c.H / 2) * (c.W / 2), c.N);
}

// the weight gradient's geometry
static c3k::WgradGeo wgrad_geo(const Case& c) {
  c3k::WgradGeo q;
  q.src = c.src; q.B = c.B; q.H = c.H; q.W = c.W; q.C = c.C;
  q.M = (long)c.B * c.H * c.W;
  q.Co = c.N; q.Kin = c.C; q.taps = c.src == 0 ? 1 : 9; q.kind = c.kind;
  q.ldx = c.C; q.ldy = c.ldy;
  return q;
}
static int wgrad_kp(const Case& c) { return c.src == 0 ? c.C : pad4(9 * c.C); }

// the conv pair's two gathers: the forward over x, the data gradient over dy
static c3k::Gather cv_fwd(const Case& c) { return c3k::make_gather(c.tconv ? 2 : 0, c.B, c.H, c.W, c.C); }
static c3k::Gather cv_bwd(const Case& c) {
  const c3k::Gather f = cv_fwd(c);
  return c3k::make_gather(c.tconv ? 1 : 0, c.B, f.Ho, f.Wo, c.N);
}

static int wprep_kp(const Case& c) {
  const int K = (c.kind >= 4 ? 1 : 9) * ((c.kind & 1) ? c.N : c.C);
  return pad4(K) == K ? K + 4 : pad4(K);  // always padded
}

// ---- --plan ------------------------------------------------------------------------------------
static std::string j(const char* k, long v, bool first = false) {
  return std::string(first ? "\"" : ",\"") + k + "\":" + std::to_string(v);
}
static std::string plan_conv3(const char* key, long M) {
  const Conv3PlanInfo p = conv3_small_plan_info(M);
  std::string s = std::string(",\"") + key + "\":{" + j("M", M, true) + j("G", p.G) + j("xr", p.xr) + j("tiles", p.tiles) +
                  j("tper", p.tper) + j("sweeps", p.sweeps) + ",\"xcd_tiles\":[";
  for (int x = 0; x < 8; ++x) s += (x ? "," : "") + std::to_string(p.xcd_tiles[x]);
  s += "],\"xcd_wgs\":[";
  for (int x = 0; x < 8; ++x) s += (x ? "," : "") + std::to_string(p.xcd_wgs[x]);
  return s + "]}";
}
static std::string plan_g2(const char* key, const Gemm2Plan& p) {
  return std::string(",\"") + key + "\":{" + j("wm", p.wm, true) + j("tm", p.tm) + j("tn", p.tn) + j("mtiles", p.mtiles) +
         j("gx", p.gx) + j("gy", p.gy) + j("splits", p.splits) + j("kslice", p.kslice) + j("res", p.res_lds > 0) +
         j("wsk", p.wsk) + "}";
}
static void print_plan(const Case& c, uint64_t seed, FILE* f) {
  std::string s = std::string("{\"case\":\"") + c.name + "\",\"op\":\"" + kOpName[c.op] + "\"" + j("refuse", c.refuse) +
                  j("B", c.B) + j("H", c.H) + j("W", c.W) + j("C", c.C) + j("N", c.N) + j("gk", c.gk) + j("sink", c.sink) +
                  j("ybf", c.ybf) + j("acc", c.acc) + j("bias", c.bias) + j("mis", c.mis) + j("tconv", c.tconv) +
                  j("act", c.act) + j("own", c.own) + j("kind", c.kind) + j("src", c.src) + j("ldy", c.ldy);
  double elems = 0, kink_share = 0;
  switch (c.op) {
    case STEM_FWD:
    case STEM_BWD:
    case STEM_GX: {
      const StemPlanInfo p = stem_plan_info(c.B, c.H, c.W);
      s += j("Ho", c.H / 2) + j("Wo", c.W / 2) + j("blocks", p.blocks) + j("last_valid", p.last_valid) +
           j("tiles_x", p.tiles_x) + j("tiles_y", p.tiles_y) + j("last_qx", p.last_qx) + j("last_qy", p.last_qy) +
           j("gx_supported", stem_bwd_gx_supported(c.N));
      elems = (double)c.B * (c.H / 2) * (c.W / 2) * c.N;
      if (c.op == STEM_GX && !c.refuse) {
        const GxHost h = gen_gx(c, seed);
        const cck::Val v = gx_view(c, h);
        kink_share = (double)v.kinks / (double)v.v.size();
        const c3k::TileMap t = c3k::stem_tiles(c.B, c.H, c.W, h.has_owner ? h.owner.data() : nullptr);
        long live = 0;
        for (uint8_t x : t.live) live += x;
        long poisoned = 0;
        if (c.own == OWN_NONE || c.own == OWN_LAST_ELEM || c.own == OWN_EDGE_QUAD)
          for (uint8_t x : c3k::stem_dy_read(c.B, c.H, c.W, t)) poisoned += !x;
        s += j("live_tiles", live) + j("tiles", (long)t.live.size()) + j("poisoned_px", poisoned);
      }
      break;
    }
    case IM2COL: {
      const c3k::Gather g = c3k::make_gather(c.gk, c.B, c.H, c.W, c.C);
      const int Kp = pad4(9 * c.C);
      elems = (double)g.out_px() * Kp;
      s += j("Ho", g.Ho) + j("Wo", g.Wo) + j("Kp", Kp) + j("mode", g.mode) + j("s", g.s) + j("pt", g.pt) +
           j("grid_strides", (long)((elems + 8192.0 * 256 - 1) / (8192.0 * 256)));
      break;
    }
    case WPREP: {
      const bool dg = c.kind & 1;
      const int Kin = dg ? c.N : c.C, taps = c.kind >= 4 ? 1 : 9;
      s += j("Kin", Kin) + j("taps", taps) + j("Kp", wprep_kp(c));
      break;
    }
    case CONV3: {
      const c3k::Gather gf = cv_fwd(c), gb = cv_bwd(c);
      const int Kf = pad4(9 * c.C), Kb = pad4(9 * c.N);
      elems = std::max((double)gf.out_px() * c.N, (double)gf.in_px() * c.C);
      s += j("Kp_f", Kf) + j("Kp_d", Kb) + j("KpR_f", (Kf + 63) / 64 * 64) + j("KpR_d", (Kb + 63) / 64 * 64) +
           j("vec_f", c.C % 4 == 0 && !c.mis) + j("vec_d", c.N % 4 == 0) + j("mode_f", gf.mode) + j("s_f", gf.s) +
           j("mode_d", gb.mode) + j("s_d", gb.s) + j("pt_d", gb.pt) + j("H_d", gb.H) + j("Ho_d", gb.Ho);
      s += plan_conv3("fwd", gf.out_px()) + plan_conv3("dgrad", gb.out_px());
      break;
    }
    case GATHER: {
      const c3k::Gather g = c3k::make_gather(c.gk, c.B, c.H, c.W, c.C);
      const int K = 9 * c.C, M = (int)g.out_px();
      elems = (double)M * K;
      const Gemm2Plan pg = plan_gemm2(M, c.N, K, gemm2_target_wgs(), false, false, true);
      const Gemm2Plan pe = plan_gemm2(M, c.N, K, gemm2_target_wgs(), false, true, false);
      s += j("Ho", g.Ho) + j("Wo", g.Wo) + j("M", M) + j("K", K) + j("mode", g.mode) + j("s", g.s) +
           j("gather_ok", gemm_gather_ok(c.B, c.H, c.W, c.C, g.Ho, g.Wo, K, g.mode, g.s, g.pt, g.pl)) +
           j("xcd_ranges", pg.gx >= 8 && pg.gx % 8 == 0) + j("impl", gemm_impl_for(c.N)) +
           j("partial_floats", (long)gemm_partial_floats(M, c.N, K));
      s += plan_g2("plan_gather", pg) + plan_g2("plan_explicit", pe);
      break;
    }
    case WGRAD: {
      const c3k::WgradGeo q = wgrad_geo(c);
      const int Kp = wgrad_kp(c);
      const long rps = un_wgrad_rows_per_slice(q.M, q.Co, Kp);
      const int ns = un_wgrad_slices(q.M, q.Co, Kp);
      elems = std::max((double)q.M * std::max(c.C, c.ldy), (double)ns * q.Co * Kp);
      s += j("M", q.M) + j("Kp", Kp) + j("rps", rps) + j("slices", ns) + j("last_rows", q.M - (ns - 1) * rps) +
           j("depth", c3k::wgrad_depth(rps, ns)) + j("vec", !c.mis && c.C % 4 == 0);
      break;
    }
  }
  char b[96];
  snprintf(b, sizeof b, ",\"elems\":%.0f,\"kink_share\":%.3g}", elems, kink_share);
  fprintf(f, "%s%s\n", s.c_str(), b);
  fflush(f);
}

// ---- the jobs ----------------------------------------------------------------------------------
static std::vector<float> widen(const Guarded* g, bool bf) {
  const size_t n = g->n / (bf ? 2 : 4);
  std::vector<float> out(n);
  if (bf) {
    for (size_t i = 0; i < n; ++i) {
      uint16_t h;
      std::memcpy(&h, g->out() + 2 * i, 2);
      out[i] = gck::bf2f(h);
    }
  } else {
    std::memcpy(out.data(), g->out(), n * 4);
  }
  return out;
}

static void job_stem_fwd(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const int Co = c.N, Ho = c.H / 2, Wo = c.W / 2;
  const long rows = (long)c.B * Ho * Wo;
  auto x = std::make_shared<std::vector<float>>(uni((size_t)c.B * c.H * c.W * 3, seed + 1));
  auto w = std::make_shared<std::vector<float>>(uni((size_t)27 * Co, seed + 2, 0.3f));
  In* dx = jb.in(*x);
  In* dw = jb.in(*w);
  Guarded* y = jb.out((size_t)rows * Co * (c.ybf ? 2 : 4), c.ybf ? 0x7fc07fc0u : 0x7fc00000u);
  const int Pexp = (int)((rows + 255) / 256);
  Guarded *part = nullptr, *cnt = nullptr;
  if (c.sink) {
    part = jb.out((size_t)Co * Pexp * 8, gck::kUnwritten);
    cnt = jb.out((size_t)Pexp * 4, gck::kUnwritten);
  }
  auto P = std::make_shared<int>(0);
  jb.launch = [=]() {
    int H = c.H, W = c.W, pt = 0, co = Co;
    if (c.refuse == R_STEM_ODD_H) H -= 1;
    if (c.refuse == R_STEM_PT) pt = 1;
    if (c.refuse == R_STEM_CO36) co = 36;
    const StatSink sk = c.sink ? StatSink{reinterpret_cast<float2*>(part->ptr()), cnt->ptr(), Co, 0} : StatSink{};
    *P = launch_stem_fwd(dx->f(), dw->f(), y->ptr(), c.B, H, W, Ho, Wo, co, pt, 0, st, sk, c.ybf);
    return true;
  };
  jb.check = [=](Verdict& v) {
    gck::Reference r = c3k::stem_fwd_ref(c.B, c.H, c.W, Co, x->data(), w->data());
    if (c.ybf) cck::bf_store(r);
    const std::vector<float> out = widen(y, c.ybf);
    v.take("y", gck::check_c(r, out.data(), (long)out.size()));
    v.P = *P;
    v.Pexp = Pexp;
    v.P_ok = *P == Pexp;
    if (c.sink) {
      v.has_sink = true;
      if (v.P_ok)
        v.s = gck::check_statsink(out.data(), rows, Co, of(part), of(cnt), Pexp);
    }
  };
}

static void job_stem_bwd(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const int Co = c.N, Ho = c.H / 2, Wo = c.W / 2;
  const size_t n = (size_t)c.B * c.H * c.W * 3;
  auto dy = std::make_shared<std::vector<float>>(uni((size_t)c.B * Ho * Wo * Co, seed + 1));
  auto w = std::make_shared<std::vector<float>>(uni((size_t)27 * Co, seed + 2, 0.3f));
  auto prev = std::make_shared<std::vector<float>>(uni(n, seed + 3));
  In* ddy = jb.in(*dy);
  In* dw = jb.in(*w);
  Guarded* dx = jb.out(n * 4);
  if (c.acc) std::memcpy(dx->fill(), prev->data(), n * 4);
  jb.launch = [=]() {
    launch_stem_bwd(ddy->f(), dw->f(), dx->ptr(), c.B, c.H, c.refuse == R_STEM_ODD_W ? c.W - 1 : c.W, Ho, Wo, Co, 0, 0,
                    c.acc, st);
    return true;
  };
  jb.check = [=](Verdict& v) {
    cck::Val g;
    g.v.assign(dy->begin(), dy->end());
    g.e.assign(dy->size(), 0.0);
    const gck::Reference r = c3k::stem_bwd_ref(c.B, c.H, c.W, Co, g, w->data(), c.acc ? prev->data() : nullptr);
    v.take("dx", gck::check_c(r, of(dx), (long)n));
  };
}

static void job_stem_gx(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const int Co = c.N, Ho = c.H / 2, Wo = c.W / 2;
  const size_t n = (size_t)c.B * c.H * c.W * 3;
  auto h = std::make_shared<GxHost>(gen_gx(c, seed));
  const c3k::TileMap tiles = c3k::stem_tiles(c.B, c.H, c.W, h->has_owner ? h->owner.data() : nullptr);
  // what the device reads: dy and y are NaN wherever no live tile's window reaches
  std::vector<float> da = h->da, y = h->y;
  if (c.own == OWN_NONE || c.own == OWN_LAST_ELEM || c.own == OWN_EDGE_QUAD) {
    const std::vector<uint8_t> rd = c3k::stem_dy_read(c.B, c.H, c.W, tiles);
    for (size_t p = 0; p < rd.size(); ++p)
      if (!rd[p])
        for (int k = 0; k < Co; ++k) da[p * Co + k] = y[p * Co + k] = gck::u2f(0x7fc00000u);
  }
  In* dda = jb.in(da);
  In* dyv = c.ybf ? jb.in_bf(y) : jb.in(y);
  In *dmu = jb.in(h->mu), *drs = jb.in(h->rstd), *dsc = jb.in(h->sc), *dbe = jb.in(h->be), *dm1 = jb.in(h->mdz),
     *dm2 = jb.in(h->mdzx), *dw = jb.in(h->w);
  In* down = nullptr;
  if (h->has_owner) {
    jb.ins.emplace_back(new In);
    down = jb.ins.back().get();
    down->put(h->owner.data(), h->owner.size() * 2);
  }
  Guarded* dx = jb.out(n * 4);
  jb.launch = [=]() {
    const int co = c.refuse == R_GX_CO56 ? 56 : c.refuse == R_GX_CO64 ? 64 : Co;
    const GradX g{dda->f(), c.act ? dyv->f() : nullptr, dmu->f(), drs->f(), dsc->f(), dbe->f(), dm1->f(), dm2->f(), c.act,
                  c.ybf ? 1 : 0};
    launch_stem_bwd_gx(g, dw->f(), down ? reinterpret_cast<const int16_t*>(down->d) : nullptr, dx->ptr(), c.B, c.H, c.W,
                       Ho, Wo, co, 0, 0, st);
    return true;
  };
  jb.check = [=](Verdict& v) {
    const cck::Val g = gx_view(c, *h);  // the clean tensors: a live tile reads none of the poisoned pixels
    v.kinks = g.kinks;
    v.kink_of = (long)g.v.size();
    gck::Reference r = c3k::stem_bwd_ref(c.B, c.H, c.W, Co, g, h->w.data(), nullptr);
    const c3k::TileCheck tc = c3k::apply_tiles(c.B, c.H, c.W, tiles, r, of(dx));
    v.take("dx", gck::check_c(r, of(dx), (long)n));
    v.fields.emplace_back("dead_bad", (double)tc.dead_bad);
    v.exact_ok = tc.dead_bad == 0;
    v.agree_ok = stem_bwd_gx_supported(Co);
  };
}

static void job_im2col(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const c3k::Gather g = c3k::make_gather(c.gk, c.B, c.H, c.W, c.C);
  const int Kp = pad4(9 * c.C);
  auto x = std::make_shared<std::vector<float>>(uni((size_t)g.in_px() * c.C, seed + 1));
  In* dx = jb.in(*x);
  Guarded* col = jb.out((size_t)g.out_px() * Kp * 4);
  jb.launch = [=]() {
    un_im2col(dx->f(), col->ptr(), g.B, g.H, g.W, g.C, g.Ho, g.Wo, Kp, g.mode, g.s, g.pt, g.pl, st);
    return true;
  };
  jb.check = [=](Verdict& v) {
    const std::vector<float> r = c3k::im2col_ref(g, x->data(), Kp);
    const long d = c3k::count_diff_bits(r.data(), of(col), (long)r.size());
    v.fields.emplace_back("col_bad", (double)d);
    v.exact_ok = d == 0;
  };
}

static void job_wprep(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const int ci = c.C, co = c.N, Kp = wprep_kp(c), N = (c.kind & 1) ? ci : co;
  auto w = std::make_shared<std::vector<float>>(uni((size_t)(c.kind >= 4 ? 1 : 9) * ci * co, seed + 1));
  In* dw = jb.in(*w);
  Guarded* bt = jb.out((size_t)N * Kp * 4);
  jb.launch = [=]() {
    un_wprep(dw->f(), bt->ptr(), c.kind, ci, co, Kp, st);
    return true;
  };
  jb.check = [=](Verdict& v) {
    const std::vector<float> r = c3k::wprep_ref(w->data(), c.kind, ci, co, Kp);
    const long d = c3k::count_diff_bits(r.data(), of(bt), (long)r.size());
    v.fields.emplace_back("bt_bad", (double)d);
    v.exact_ok = d == 0;
  };
}

static void job_conv3(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const c3k::Gather gf = cv_fwd(c), gb = cv_bwd(c);
  const int ci = c.C, co = c.N, Kf = pad4(9 * ci), Kb = pad4(9 * co);
  auto x = std::make_shared<std::vector<float>>(uni((size_t)gf.in_px() * ci, seed + 1));
  auto w = std::make_shared<std::vector<float>>(uni((size_t)9 * ci * co, seed + 2, 0.5f));
  auto bias = std::make_shared<std::vector<float>>(uni(co, seed + 3));
  auto dy = std::make_shared<std::vector<float>>(uni((size_t)gf.out_px() * co, seed + 4));
  In* dx = jb.in(*x, c.mis);
  In* dxa = c.mis ? jb.in(*x) : nullptr;  // the same data, aligned: the VEC instantiation
  In *dw = jb.in(*w), *db = jb.in(*bias), *ddy = jb.in(*dy);
  Guarded* btf = jb.out((size_t)co * Kf * 4);
  Guarded* btd = jb.out((size_t)ci * Kb * 4);
  Guarded* y = jb.out((size_t)gf.out_px() * co * 4);
  Guarded* gxo = jb.out((size_t)gf.in_px() * ci * 4);
  Guarded* y2 = c.mis ? jb.out((size_t)gf.out_px() * co * 4) : nullptr;
  if (c.refuse) {
    jb.launch = [=]() {
      int N = 32, C = 4, Kp = 36;
      if (c.refuse == R_CV_N33) N = 33;
      if (c.refuse == R_CV_KP292) { C = 32; Kp = 292; }
      if (c.refuse == R_CV_KP_SHORT) Kp = 32;
      if (c.refuse == R_CV_KP_MOD4) { C = 3; Kp = 30; }
      return un_conv3_small(dx->f(), btf->ptr(), db->f(), y->ptr(), 1, 4, 4, C, 4, 4, N, Kp, 0, 1, 1, 1, st);
    };
    return;
  }
  jb.launch = [=]() {
    bool ok = true;
    un_wprep(dw->f(), btf->ptr(), c.tconv ? 2 : 0, ci, co, Kf, st);
    un_wprep(dw->f(), btd->ptr(), c.tconv ? 3 : 1, ci, co, Kb, st);
    ok &= un_conv3_small(dx->f(), btf->ptr(), c.bias ? db->f() : nullptr, y->ptr(), gf.B, gf.H, gf.W, ci, gf.Ho, gf.Wo, co,
                         Kf, gf.mode, gf.s, gf.pt, gf.pl, st);
    ok &= un_conv3_small(ddy->f(), btd->ptr(), nullptr, gxo->ptr(), gb.B, gb.H, gb.W, co, gb.Ho, gb.Wo, ci, Kb, gb.mode,
                         gb.s, gb.pt, gb.pl, st);
    if (y2)
      ok &= un_conv3_small(dxa->f(), btf->ptr(), c.bias ? db->f() : nullptr, y2->ptr(), gf.B, gf.H, gf.W, ci, gf.Ho, gf.Wo,
                           co, Kf, gf.mode, gf.s, gf.pt, gf.pl, st);
    return ok;
  };
  jb.check = [=](Verdict& v) {
    c3k::Weights wt;
    wt.w = w->data(); wt.tconv = c.tconv; wt.ci = ci; wt.co = co;
    const gck::Reference rf = c3k::conv_fwd_ref(gf, x->data(), wt, co, c.bias ? bias->data() : nullptr, Kf);
    v.take("y", gck::check_c(rf, of(y), (long)rf.c.size()));
    const gck::Reference rb = c3k::conv_adj_ref(gf, dy->data(), wt, co, Kb);
    v.take("dx", gck::check_c(rb, of(gxo), (long)rb.c.size()));
    const std::vector<float> bf = c3k::wprep_ref(w->data(), c.tconv ? 2 : 0, ci, co, Kf);
    const std::vector<float> bd = c3k::wprep_ref(w->data(), c.tconv ? 3 : 1, ci, co, Kb);
    const long d = c3k::count_diff_bits(bf.data(), of(btf), (long)bf.size()) +
                   c3k::count_diff_bits(bd.data(), of(btd), (long)bd.size());
    v.fields.emplace_back("bt_bad", (double)d);
    v.exact_ok = d == 0;
    if (y2) {
      v.take("y_vec", gck::check_c(rf, of(y2), (long)rf.c.size()));
      v.fields.emplace_back("vec_pair", c3k::pair_ratio(rf, of(y), of(y2), (long)rf.c.size()));
    }
  };
}

static void job_gather(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const c3k::Gather g = c3k::make_gather(c.gk, c.B, c.H, c.W, c.C);
  const int K = 9 * c.C, N = c.N, M = (int)g.out_px();
  auto x = std::make_shared<std::vector<float>>(uni((size_t)g.in_px() * c.C, seed + 1));
  auto bt = std::make_shared<std::vector<float>>(uni((size_t)N * K, seed + 2, 0.2f));
  auto bias = std::make_shared<std::vector<float>>(uni(N, seed + 3));
  In* dx = jb.in(*x, c.refuse == R_GG_ALIGN);
  In *dbt = jb.in(*bt), *db = jb.in(*bias);
  const size_t pf = gemm_partial_floats(M, N, K);
  Guarded* o1 = jb.out((size_t)M * N * 4);
  Guarded* p1 = jb.out(pf * 4);
  if (c.refuse) {
    jb.launch = [=]() {
      int W = c.W, C = c.C, Kx = K;
      if (c.refuse == R_GG_W15) W = 15;
      if (c.refuse == R_GG_C3) { C = 3; Kx = 27; }  // (27 % 4 != 0 as well; the geometry check comes first)
      if (c.refuse == R_GG_K) Kx = K + 4;
      launch_gemm_gather(dx->f(), c.B, c.H, W, C, g.Ho, W, g.mode, g.s, g.pt, g.pl, dbt->f(), db->f(), o1->ptr(), N, Kx, st,
                         p1->ptr());
      return true;
    };
    jb.check = [=](Verdict& v) {
      int W = c.W, C = c.C, Kx = K;
      if (c.refuse == R_GG_W15) W = 15;
      if (c.refuse == R_GG_C3) { C = 3; Kx = 27; }
      if (c.refuse == R_GG_K) Kx = K + 4;
      // gemm_gather_ok agrees where it applies (alignment is the launcher's own check)
      v.agree_ok = gemm_gather_ok(c.B, c.H, W, C, g.Ho, W, Kx, g.mode, g.s, g.pt, g.pl) == (c.refuse == R_GG_ALIGN);
    };
    return;
  }
  Guarded* col = jb.out((size_t)M * K * 4);
  Guarded* o2 = jb.out((size_t)M * N * 4);
  Guarded* p2 = jb.out(pf * 4);
  jb.launch = [=]() {
    launch_gemm_gather(dx->f(), g.B, g.H, g.W, g.C, g.Ho, g.Wo, g.mode, g.s, g.pt, g.pl, dbt->f(), db->f(), o1->ptr(), N, K,
                       st, p1->ptr());
    un_im2col(dx->f(), col->ptr(), g.B, g.H, g.W, g.C, g.Ho, g.Wo, K, g.mode, g.s, g.pt, g.pl, st);
    gemm2_run(0, InX{col->ptr(), nullptr, nullptr, nullptr, 0}, GradX{}, dbt->f(), db->f(), o2->ptr(), M, N, K, false,
              nullptr, 1, st, p2->ptr(), StatSink{}, gemm2_target_wgs(), GradSink{}, false, false);
    return true;
  };
  jb.check = [=](Verdict& v) {
    c3k::Weights wt;
    wt.bt = bt->data(); wt.ldb = K; wt.ci = c.C;
    const gck::Reference r = c3k::conv_fwd_ref(g, x->data(), wt, N, bias->data(), K);
    v.take("gather", gck::check_c(r, of(o1), (long)r.c.size()));
    v.take("explicit", gck::check_c(r, of(o2), (long)r.c.size()));
    const std::vector<float> cr = c3k::im2col_ref(g, x->data(), K);
    const long dc = c3k::count_diff_bits(cr.data(), of(col), (long)cr.size());
    const long dg = c3k::count_diff_bits(of(o1), of(o2), (long)r.c.size());
    v.fields.emplace_back("col_bad", (double)dc);
    v.fields.emplace_back("gather_bad", (double)dg);
    v.exact_ok = dc == 0 && dg == 0;
    v.agree_ok = gemm_gather_ok(g.B, g.H, g.W, g.C, g.Ho, g.Wo, K, g.mode, g.s, g.pt, g.pl) && gemm_impl_for(N) == 2;
  };
}

static void job_wgrad(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  const c3k::WgradGeo q = wgrad_geo(c);
  const int Kp = wgrad_kp(c);
  const long xin = c.src == 0 ? q.M * q.ldx : c.src == 1 ? q.M * c.C : (long)c.B * (c.H / 2) * (c.W / 2) * c.C;
  auto dy = std::make_shared<std::vector<float>>(uni((size_t)q.M * q.ldy, seed + 1));
  auto x = std::make_shared<std::vector<float>>(uni((size_t)xin, seed + 2));
  In* ddy = jb.in(*dy);
  In* dx = jb.in(*x, c.mis);
  const int ns = un_wgrad_slices(q.M, q.Co, Kp);
  const long rps = un_wgrad_rows_per_slice(q.M, q.Co, Kp);
  Guarded* part = jb.out((size_t)ns * q.Co * Kp * 4);
  Guarded* g = jb.out((size_t)q.g_elems() * 4);
  jb.launch = [=]() {
    un_wgrad(ddy->f(), q.ldy, dx->f(), q.ldx, c.src, c.B, c.refuse == R_WG_ODD_H ? c.H - 1 : c.H, c.W, c.C,
             c.refuse == R_WG_M ? q.M - 1 : c.refuse == R_WG_ODD_H ? (long)c.B * (c.H - 1) * c.W : q.M, q.Co, Kp, q.Kin,
             q.taps, c.kind, part->ptr(), g->ptr(), st);
    return true;
  };
  jb.check = [=](Verdict& v) {
    const gck::Reference r = c3k::wgrad_ref(q, dy->data(), x->data(), c3k::wgrad_depth(rps, ns));
    v.take("g", gck::check_c(r, of(g), (long)r.c.size()));
  };
}

static void make_job(const Case& c, uint64_t seed, hipStream_t st, Job& jb) {
  switch (c.op) {
    case STEM_FWD: job_stem_fwd(c, seed, st, jb); break;
    case STEM_BWD: job_stem_bwd(c, seed, st, jb); break;
    case STEM_GX: job_stem_gx(c, seed, st, jb); break;
    case IM2COL: job_im2col(c, seed, st, jb); break;
    case WPREP: job_wprep(c, seed, st, jb); break;
    case CONV3: job_conv3(c, seed, st, jb); break;
    case GATHER: job_gather(c, seed, st, jb); break;
    case WGRAD: job_wgrad(c, seed, st, jb); break;
  }
}

static Verdict run_case(const Case& c, uint64_t seed, hipStream_t st) {
  Verdict v;
  Job jb;
  make_job(c, seed, st, jb);
  auto launch = [&]() {
    for (auto& o : jb.outs) o->upload();
    const bool ok = jb.launch();
    CK(hipStreamSynchronize(st));
    CK(hipGetLastError());
    return ok;
  };
  try {
    v.refused = !launch();
  } catch (const HipError& e) {
    fatal(e.what(), c.name);
  } catch (const std::exception& e) {
    v.threw = v.refused = true;
    v.what = e.what();
  }
  if (v.refused || c.refuse) {
    // a refusal launches nothing: every output still holds its fill
    CK(hipStreamSynchronize(st));
    CK(hipGetLastError());
    for (auto& o : jb.outs) {
      o->download();
      v.untouched &= o->got == o->init;
    }
    for (auto& i : jb.ins) v.inputs_ok &= i->same();
    if (jb.check && c.op == GATHER) jb.check(v);
    if (c.op == STEM_GX) v.agree_ok = !stem_bwd_gx_supported(c.refuse == R_GX_CO56 ? 56 : 64);
    return v;
  }
  for (auto& o : jb.outs) {
    o->download();
    v.canary_ok &= o->intact();
  }
  const auto t0 = std::chrono::steady_clock::now();
  jb.check(v);
  v.ref_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // repeatability: a second launch from the same initial state leaves the same bits
  std::vector<std::vector<uint8_t>> keep;
  for (auto& o : jb.outs) keep.push_back(o->got);
  try {
    if (!launch()) v.repeat_ok = false;
  } catch (const HipError& e) {
    fatal(e.what(), c.name);
  } catch (const std::exception& e) {
    v.repeat_ok = false;
  }
  for (size_t i = 0; i < jb.outs.size(); ++i) {
    jb.outs[i]->download();
    v.repeat_ok &= jb.outs[i]->got == keep[i];
  }
  for (auto& i : jb.ins) v.inputs_ok &= i->same();
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
    fprintf(stderr, "usage: conv3_parity [--plan]\n");
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
                       std::to_string(c.refuse) + ",\"threw\":" + tf(v.threw) + ",\"refused\":" + tf(v.refused);
    if (v.threw) line += ",\"what\":\"" + esc(v.what) + "\"";
    if (c.refuse) {
      ok = v.refused && v.untouched && v.inputs_ok && v.agree_ok;
      line += std::string(",\"untouched\":") + tf(v.untouched) + ",\"inputs_ok\":" + tf(v.inputs_ok) + ",\"agree_ok\":" +
              tf(v.agree_ok);
    } else {
      const double share = v.kink_of ? (double)v.kinks / (double)v.kink_of : 0.0;
      ok = !v.refused && v.ratio <= 1.0 && v.nonfinite == 0 && v.exact_ok && v.canary_ok && v.repeat_ok && v.inputs_ok &&
           v.agree_ok && share <= 0.01;
      std::string fields;
      for (auto& f : v.fields) {
        const bool count = f.first.size() > 4 && f.first.compare(f.first.size() - 4, 4, "_bad") == 0;
        if (!count) ok = ok && f.second <= 1.0;
        fields += (fields.empty() ? "\"" : ",\"") + f.first + "\":" + num(f.second);
      }
      if (v.has_sink)
        ok = ok && v.P_ok && v.s.rows_written && v.s.cnt_ok && v.s.cnt_sum_ok && v.s.sum_ratio <= 1.0 &&
             v.s.m2_ratio <= 1.0;
      else if (c.op == STEM_FWD)
        ok = ok && v.P_ok;
      line += ",\"ratio\":" + num(v.ratio) + ",\"nonfinite\":" + std::to_string(v.nonfinite) + ",\"fields\":{" + fields +
              "},\"exact_ok\":" + tf(v.exact_ok) + ",\"canary_ok\":" + tf(v.canary_ok) + ",\"repeat_ok\":" +
              tf(v.repeat_ok) + ",\"inputs_ok\":" + tf(v.inputs_ok) + ",\"agree_ok\":" + tf(v.agree_ok) +
              ",\"kink_share\":" + num(share) + ",\"ref_ms\":" + num(v.ref_ms) + ",\"has_sink\":" + tf(v.has_sink) +
              ",\"P_got\":" + std::to_string(v.P) + ",\"P_expected\":" + std::to_string(v.Pexp) + ",\"P_ok\":" + tf(v.P_ok);
      if (v.has_sink)
        line += std::string(",\"rows_written\":") + tf(v.s.rows_written) + ",\"cnt_ok\":" + tf(v.s.cnt_ok) +
                ",\"cnt_sum_ok\":" + tf(v.s.cnt_sum_ok) + ",\"sum_ratio\":" + num(v.s.sum_ratio) + ",\"m2_ratio\":" +
                num(v.s.m2_ratio);
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
