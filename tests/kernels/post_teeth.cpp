// post_teeth — the teeth of the post-processing kernel parity checker's references, bounds and compare functions
// (post_check.hpp), without a GPU: the CPU fp32 stand-in (the kernels' own structure: tiles and levels, the two
// class halves, the chunked per-image max, the lazy soft-NMS queue) runs clean and with one seeded fault at a time
// through the same stage-by-stage checks post_parity applies to the device's output.  One JSON line per run, then
// a `done` line; tests/test_post_parity_host.py asserts that every clean run passes and every fault trips its own
// fields and no other.
// Build: make -C tests/kernels.
#include <cstdio>
#include <string>
#include <vector>

#include "post_check.hpp"

using namespace pck;

static void run(const char* name, Case c, Fault f) {
  c.name = name;
  Sim sim;
  sim.f = f;
  Verdict V;
  run_case(c, sim, V);
  printf("{\"run\":\"%s\",%s,\"pass\":%s}\n", name, verdict_json(V).c_str(), V.pass() ? "true" : "false");
  fflush(stdout);
}

int main() {
  const std::vector<float> x = exp_args();
  std::vector<float> y(x.size());
  for (size_t i = 0; i < x.size(); ++i) y[i] = expf(x[i]);
  set_exp_ulp(exp_max_ulp(x, y));
  Case chain;
  chain.kind = K_CHAIN; chain.seed = 7; chain.B = 3; chain.K = 65; chain.nseg = 8;
  Case bf = chain;
  bf.bf = 1; bf.cand_mask = 1; bf.cand_thresh = 0.5f; bf.max_out = 7;
  Case half = chain;  // a list threshold of 0.5 with every anchor eligible: the planted score of exactly 0.5 decides
  half.cand_mask = -1; half.cand_thresh = 0.5f;
  Case nms;
  nms.kind = K_NMS; nms.seed = 320; nms.B = 2; nms.N = 4096; nms.plant = 1;
  Case imax;
  imax.kind = K_IMAX; imax.seed = 318; imax.B = 4; imax.N = 846;
  Case loss;
  loss.kind = K_LOSS;
  Case adam;
  adam.kind = K_ADAM; adam.n = kNPatch + 1; adam.t = 1; adam.clip = 1;
  run("clean_chain_f32", chain, F_NONE);
  run("clean_chain_bf16_mask1", bf, F_NONE);
  run("clean_nms_ties_dups", nms, F_NONE);
  run("clean_imax_loss", imax, F_NONE);
  run("clean_adam_clip", adam, F_NONE);
  // one fault each
  run("second_half_wins_ties", chain, F_HALF_GE);
  run("ragged_last_anchor_dropped", chain, F_RAGGED_LAST);
  run("level_lookup_off_by_one", chain, F_LEVEL_OFF1);
  run("area_ge_100", chain, F_AREA_GE);
  run("person_bit_after_filter", chain, F_PERSON_AFTER);
  run("candidate_gate_ge", half, F_CAND_GE);
  run("candidate_appended_twice", chain, F_CAND_TWICE);
  run("imax_tie_counts_not_added", imax, F_IMAX_NOADD);
  run("imax_first_index_not_smallest", imax, F_IMAX_FIRST);
  run("loss_grad_zero_at_raw_zero", loss, F_LOSS_GRAD0);
  run("tied_classes_not_divided", chain, F_TIE_NODIV);
  run("only_first_tied_class", chain, F_TIE_FIRST);
  run("dx_overwritten", chain, F_DX_OVERWRITE);
  run("nms_ties_higher_index", nms, F_NMS_TIE_HI);
  run("nms_clip_omitted", nms, F_NO_CLIP);
  run("cand_count_not_reset", chain, F_COUNT_KEEP);
  run("adam_scale_clipped_pm1", adam, F_ADAM_SCALE_CLIP);
  printf("{\"done\":true}\n");
  return 0;
}
