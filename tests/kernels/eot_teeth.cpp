// eot_teeth — the teeth of the EOT kernel parity checker's references, bounds and compare functions
// (eot_check.hpp), without a GPU: the CPU fp32 stand-in (the kernels' own operation order: placement and
// lists, the banded resize in row tiles, the per-pixel fold, the two-stage adjoint behind adj_range) runs
// clean and with one seeded fault at a time through the same stage-by-stage checks eot_parity applies to the
// device's output.  One JSON line per run, then a `done` line; tests/test_eot_parity_host.py asserts that
// every clean run passes and every fault trips its own fields and no other.
// Build: make -C tests/kernels.
#include <cstdio>
#include <string>
#include <vector>

#include "eot_check.hpp"

using namespace eck;

static Case base(const char* name) {
  Case c;
  c.name = name;
  c.B = 2; c.H = 56; c.W = 48; c.maxb = 4; c.P = 37;
  c.counts = {3, 2};
  c.ps = {30, 9, 14, 22, 41};
  c.seed = 11;
  return c;
}

static void run(const char* name, Case c, Fault f) {
  c.name = name;
  const Inputs in = make_inputs(c);
  Sim sim;
  sim.f = f;
  StageOut so;
  const Verdict V = run_case(in, sim, so);
  printf("{\"run\":\"%s\",%s,\"margin\":%s,\"pass\":%s}\n", name, verdict_json(V).c_str(), jnum(in.margin).c_str(),
         V.pass() ? "true" : "false");
  fflush(stdout);
}

int main() {
  // clean: every operation, under both placement rules, both matcher launches, planted gate values, an image
  // without boxes, the upscale, TV on and off
  Case a = base("");
  Case planted = a;
  planted.plant = 1;
  planted.layout = L_CLUSTER;
  Case def = a;
  def.defender = 1; def.batch = 1; def.clipw = 1; def.counts = {0, 4}; def.add_tv = 0; def.add_loss = 0; def.amp = 0.f;
  def.ps = {12, 17, 9, 23};
  Case noprint = a;
  noprint.apply_print = 0; noprint.P = 5; noprint.ps = {7, 3, 5}; noprint.img_amp = 1.3f;
  run("clean_attacker_p37", a, F_NONE);
  run("clean_planted_cluster", planted, F_NONE);
  run("clean_defender_batch_clipw", def, F_NONE);
  run("clean_noprint_p5_upscale", noprint, F_NONE);
  // one fault each
  run("adj_range_narrow_high", a, F_ADJ_NARROW);
  run("owner_first_kept", planted, F_OWNER_FIRST);
  run("fill_test_le", planted, F_FILL_LE);
  run("ragged_tile_dropped", a, F_RAGGED_TILE);
  run("band_skipped", a, F_BAND_SKIP);
  run("inv_transposed", a, F_INV_TRANSPOSED);
  run("noise_omitted", a, F_NO_NOISE);
  run("delta_before_noise", a, F_DELTA_FIRST);
  run("pre_clip_gate_strict", planted, F_GATE_STRICT);
  run("tv_last_row_dropped", a, F_TV_LAST_ROW);
  run("mean_dyc_omitted", a, F_NO_MEAN_DYC);
  Case empty_first = a;
  empty_first.B = 3; empty_first.counts = {2, 0, 2};
  run("img_first_after_empty_image", empty_first, F_IMG_FIRST);
  printf("{\"done\":true}\n");
  return 0;
}
