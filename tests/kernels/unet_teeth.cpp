// unet_teeth — the teeth of unet_check.hpp's references and bounds: its CPU stand-in (Sim: the kernels restated in
// fp32, the fp64 reduction with k_colred64's block / lane-group geometry and the finals' wave fold) runs clean
// through the same check functions the device's results take, then once per seeded fault.  One JSON line per run
// ({"run", "fields", "flags"}), then a `done` line; tests/test_unet_parity_host.py asserts that every clean run
// passes every bound and that each fault trips its own fields and no other.  Host only.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "unet_check.hpp"

using namespace uck;

static int g_runs = 0;
static void run(const std::string& name, Fault f, int op, const std::function<void(Case&)>& more) {
  Case c;
  c.name = name; c.op = op; c.seed = 900 + (uint32_t)op;
  more(c);
  Sim sim(f);
  Verdict v;
  run_case(c, sim, v);
  v.flags["no_nonfinite"] = v.nonfinite == 0;
  v.flags["no_throw"] = !v.threw;
  printf("{\"run\":\"%s\",%s}\n", name.c_str(), verdict_json(v).c_str());
  ++g_runs;
}

int main(int argc, char** argv) {
  {
    const std::string self = argv[0];
    const size_t sl = self.rfind('/');
    g_golden.load((sl == std::string::npos ? std::string(".") : self.substr(0, sl)) + "/../golden/unet");
  }
  // the host's expf / tanhf stand in for the device's: the same measurement sets the allowance
  {
    VF xe = exp_args(), xt = tanh_args();
    double we = 0, wt = 0;
    for (float x : xe) we = std::max(we, ulp_err(expf(x), std::exp((double)x)));
    for (float x : xt) wt = std::max(wt, ulp_err(tanhf(x), std::tanh((double)x)));
    set_ulps(we, wt);
  }
  const auto colsum3 = [](Case& c) { c.C = 24; c.M = 700; c.data = 1; };                 // 3 blocks, 16 idle threads
  const auto colsum65 = [](Case& c) { c.C = 256; c.M = 2049; c.data = 1; };              // 65 blocks
  const auto stats = [](Case& c) { c.C = 8; c.M = 257; c.data = 1; c.flav = 0; };
  const auto stats_mv = [](Case& c) { c.C = 3; c.M = 5; c.flav = 1; };
  const auto bnbwd = [](Case& c) { c.C = 24; c.M = 700; c.data = 1; };
  const auto pool = [](Case& c) { c.B = 2; c.H = 4; c.W = 6; c.C = 3; c.layer = 0; c.gimg0 = 3; c.seed = 502; };
  const auto cat = [](Case& c) { c.C = 8; c.B = 1; c.HW = 5; c.layer = 7; };
  const auto out = [](Case& c) { c.C = 8; c.B = 3; c.HW = 257; c.M = 3 * 257; };
  const auto flt = [](Case& c) { c.B = 65; c.maxo = 100; c.sets = 0; c.flav = 1; };
  struct R { const char* name; Fault f; int op; std::function<void(Case&)> more; };
  const std::vector<R> runs = {
      {"clean_colsum", F_NONE, COLSUM, colsum3},
      {"clean_colsum_blk65", F_NONE, COLSUM, colsum65},
      {"clean_stats", F_NONE, STATS, stats},
      {"clean_stats_moving", F_NONE, STATS, stats_mv},
      {"clean_bn_bwd", F_NONE, BNBWD, bnbwd},
      {"clean_bnact", F_NONE, BNACT, [](Case& c) { c.M = 85; c.C = 3; }},
      {"clean_att_s", F_NONE, ATT_S, [](Case& c) { c.M = 85; c.C = 3; }},
      {"clean_att_s_bwd", F_NONE, ATT_S_BWD, [](Case& c) { c.M = 85; c.C = 3; }},
      {"clean_att_t", F_NONE, ATT_T, [](Case& c) { c.M = 257; c.C = 8; }},
      {"clean_small_dgrad", F_NONE, SMALL_DGRAD, [](Case& c) { c.M = 85; c.C = 3; c.O = 3; c.acc = 1; }},
      {"clean_add", F_NONE, ADD, [](Case& c) { c.M = 257; }},
      {"clean_pool", F_NONE, POOL, pool},
      {"clean_att_cat", F_NONE, ATT_CAT, cat},
      {"clean_att_cat_saturated", F_NONE, ATT_CAT, [](Case& c) { c.C = 8; c.B = 1; c.HW = 40; c.layer = 5; c.flav = 1; }},
      {"clean_out", F_NONE, OUT, out},
      {"clean_out_target_is_output", F_NONE, OUT, [](Case& c) { c.C = 8; c.B = 3; c.HW = 257; c.M = 3 * 257; c.flav = 1; }},
      {"clean_perm", F_NONE, PERM, [](Case& c) { c.B = 5; c.H = 7; c.W = 4; c.P = 3; c.gimg0 = 7; c.step = 2; }},
      {"clean_filter", F_NONE, FILTER, flt},
      {"block_last_row_dropped", F_BLOCK_LAST_ROW, COLSUM, colsum3},
      {"idle_threads_rows_added", F_IDLE_ROWS, COLSUM, colsum3},
      {"block_64_skipped", F_SKIP_BLOCK64, COLSUM, colsum65},
      {"shift_not_added_back", F_NO_SHIFT, STATS, stats},
      {"bessel_missing", F_NO_BESSEL, STATS, stats_mv},
      {"last_maximum", F_LAST_MAX, POOL, pool},
      {"pool_bwd_scale_missing", F_BWD_NO_SCALE, POOL, pool},
      {"element_index_not_restarted", F_NO_RESTART, POOL, pool},
      {"xor_tree_one_step_short", F_XOR_SHORT, ATT_CAT, cat},
      {"clamped_lane_stores", F_CLAMP_STORES, ATT_CAT, cat},
      {"sigmoid_derivative_missing", F_NO_DSIG, ATT_CAT, cat},
      {"loss_divided_by_m", F_LOSS_M, OUT, out},
      {"un_out_other_order", F_OUT_ORDER, OUT, out},
      {"filter_area_ge", F_AREA_GE, FILTER, flt},
      {"filter_tail_rows_unzeroed", F_TAIL_ROWS, FILTER, flt},
  };
  for (const R& r : runs) run(r.name, r.f, r.op, r.more);
  printf("{\"done\":true,\"runs\":%d,\"golden_read\":%s}\n", g_runs, g_golden.read ? "true" : "false");
  return 0;
}
