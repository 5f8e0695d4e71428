// exec_plan — prints the executor plan (csrc/exec_plan.hpp) of each configuration given on the command
// line as one JSON line.  Host only: plan_exec makes no HIP call, so this runs without a GPU.
//   exec_plan [--full] MODEL:SIZE:B:TAG:BN:DTYPE ...
// SIZE 0 is the model's default image size; BN is local | frozen | sync; DTYPE is f32 | bf16.  The
// planner's environment knobs (PHX_SEP, PHX_SEP_MINROWS, PHX_SEPB, PHX_GROUP, PHX_FOLD) apply as in
// the library.  tests/test_exec_plan_host.py compares the lines with tests/golden/exec_plan/plans.json.
//   exec_plan --guard
// plans hand-built programs (two 1x1 convs -> BiFPN fuse -> 3x3 stride-1 depthwise -> 1x1 conv) whose
// depthwise op is SAME, VALID, SAME-sized with no top/left pad, or depth multiplier 2, and prints
// whether the fuse was folded and the separable conv fused: only SAME may be.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "exec_plan.hpp"
#include "exec_plan_json.hpp"
#include "phx.h"

using namespace phx;

// input -> pw, pw -> fuse -> dw (pad, Ho x Wo x Co) -> pw
static Program guard_program(int B, int H, int pad, int Ho, int Co) {
  Program P;
  auto tensor = [&](int h, int c) {
    Tensor t;
    t.n = B, t.h = h, t.w = h, t.c = c;
    t.off = P.act_floats;
    P.act_floats += t.numel();
    P.tensors.push_back(t);
    return (int)P.tensors.size() - 1;
  };
  auto op = [&](OpT t, std::vector<int> in, int out, int k = 1, int p = 0) {
    Op o;
    o.t = t;
    o.nin = (int)in.size();
    for (int j = 0; j < o.nin; ++j) o.in[j] = in[j];
    o.out = out;
    o.k = k, o.pad_t = p, o.pad_l = p;
    o.w = 64L * 64 * (long)P.ops.size();
    o.name = "op" + std::to_string(P.ops.size());
    P.ops.push_back(o);
  };
  P.input = tensor(H, 64);
  const int a = tensor(H, 64), b = tensor(H, 64), f = tensor(H, 64), d = tensor(Ho, Co), y = tensor(Ho, 64);
  op(OP_PW, {P.input}, a);
  op(OP_PW, {P.input}, b);
  op(OP_FUSE, {a, b}, f);
  op(OP_DW, {f}, d, 3, pad);
  op(OP_PW, {d}, y);
  P.batch = B;
  return P;
}

static int guard() {
  setenv("PHX_SEP_MINROWS", "0", 1);
  struct C { const char* name; int pad, Ho, Co; };
  const int H = 16;
  const C cases[] = {{"same", 1, H, 64}, {"valid", 0, H - 2, 64}, {"same_size_no_pad", 0, H, 64}, {"multiplier_2", 1, H, 128}};
  for (const C& c : cases) {
    const ExecPlan E = plan_program(guard_program(2, H, c.pad, c.Ho, c.Co), 2, 0, PHX_BN_FROZEN, false, 64, 9, 0);
    printf("{\"case\":\"%s\",\"fuse_folded\":%d,\"sep\":%d}\n", c.name, (int)E.fuse_folded[2], (int)E.sep[3]);
  }
  printf("{\"done\":true}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--guard") return guard();
  bool full = false;
  std::vector<std::string> specs;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--full") full = true;
    else specs.push_back(argv[i]);
  }
  if (specs.empty()) {
    fprintf(stderr, "usage: exec_plan [--full] MODEL:SIZE:B:TAG:BN:DTYPE ...\n");
    return 2;
  }
  for (const std::string& spec : specs) {
    std::vector<std::string> f;
    std::stringstream ss(spec);
    for (std::string t; std::getline(ss, t, ':');) f.push_back(t);
    ModelConfig mc;
    if (f.size() != 6 || !get_model_config(f[0], &mc)) {
      fprintf(stderr, "exec_plan: bad configuration '%s'\n", spec.c_str());
      return 2;
    }
    if (std::atoi(f[1].c_str()) > 0) mc.image_size = std::atoi(f[1].c_str());
    const int B = std::atoi(f[2].c_str()), tag = std::atoi(f[3].c_str());
    const int bn = f[4] == "local" ? PHX_BN_LOCAL : f[4] == "frozen" ? PHX_BN_FROZEN : f[4] == "sync" ? PHX_BN_SYNC : -1;
    if (B <= 0 || tag < 0 || tag > 2 || bn < 0 || (f[5] != "f32" && f[5] != "bf16")) {
      fprintf(stderr, "exec_plan: bad configuration '%s'\n", spec.c_str());
      return 2;
    }
    // the context's anchor count (phx_create)
    int fs = mc.image_size, A = 0;
    for (int l = 1; l <= mc.max_level; ++l) {
      fs = (fs - 1) / 2 + 1;
      if (l >= mc.min_level) A += fs * fs * mc.num_anchors();
    }
    const ExecPlan E = plan_exec(mc, B, tag, bn, f[5] == "bf16", A);
    PlanDump d;
    plan_dump_fields(E, d);
    d.s("red_need", (long long)E.red_need);
    d.s("coef_need", (long long)E.coef_need);
    d.s("seg_need", (long long)E.seg_need);
    d.s("gp_need", (long long)E.gp_need);
    d.s("nreg", (long long)E.nreg);
    d.s("side_need", (long long)E.side_need);
    d.s("sync_need", (long long)E.sync_need);
    std::vector<long long> mov;
    for (const MovEntry& m : E.mov) {
      const long long v[4] = {m.mm, m.mv, m.C, m.off};
      mov.insert(mov.end(), v, v + 4);
    }
    d.v("mov", mov);
    d.v("drop_blocks", E.drop_blocks);
    d.vf("drop_surv", E.drop_surv);
    printf("%s\n", plan_json(spec, d, full).c_str());
  }
  printf("{\"done\":true}\n");
  return 0;
}
