// exec.cpp — the program executor: an executor's buffers (allocated from its plan, exec_plan.hpp), the
// victim's forward and data-gradient interpreters with their grouped and fused-separable launches,
// pre-NMS / NMS, the checksum and guard-band diagnostics and the profiler's launch-group hooks.
#include "ctx.hpp"

// ------------------------------------------------------------------------------------------
// executor
// ------------------------------------------------------------------------------------------
// One executor per (batch size, tag) (the program and its arenas are shaped by B; tag 1 is the
// concurrent first pass's forward-only executor, §12 of DESIGN.md; tag 2 is phx_serve's forward-only
// executor in a context whose BN mode is not frozen, planned for inference BN exactly as a
// bn=frozen context's tag 0, so that serving computes the same bits whatever the context's mode).
// At most kMaxExecs stay
// alive, two per batch size for two batch sizes, so a driver that mixes batch sizes (a last
// partial batch, validation) keeps both sizes' step and side executors without evicting at every
// switch.  A third batch size evicts (after the device has drained, so no queued kernel still
// reads its memory) a forward-only executor first — the smaller, cheaper one to rebuild — and
// the least recently used among those.
constexpr size_t kMaxExecs = 4;

namespace {

// The buffers of a planned executor: every size comes from the plan (A: the context's anchor count).
void alloc_exec(Exec& E, int A) {
  const Program& P = E.prog;
  const int B = E.B;
  E.act = E.alloc<float>(E.abf ? (P.act_floats + 1) / 2 : P.act_floats);
  // the concurrent first pass's executor (tag 1) runs forwards only: no gradient arena
  E.grad = E.alloc<float>(E.tag != 0 ? 1 : P.grad_floats);
  // statistics slots
  E.slot_a.assign(P.n_slots, nullptr);
  E.slot_b.assign(P.n_slots, nullptr);
  E.slot_c.assign(P.n_slots, nullptr);
  E.slot_d.assign(P.n_slots, nullptr);
  E.slot_e.assign(P.n_slots, nullptr);
  for (const Op& op : P.ops) {
    const Tensor& ti = P.tensors[op.in[0]];
    if (op.t == OP_BN) {
      E.slot_a[op.slot] = E.alloc<float>(ti.c);
      E.slot_b[op.slot] = E.alloc<float>(ti.c);
      E.slot_c[op.slot] = E.alloc<float>(ti.c);
      E.slot_d[op.slot] = E.alloc<float>(ti.c);
      E.slot_e[op.slot] = E.alloc<float>(ti.c);
      PHX_HIP(hipMemset(E.slot_d[op.slot], 0, ti.c * sizeof(float)));
      PHX_HIP(hipMemset(E.slot_e[op.slot], 0, ti.c * sizeof(float)));
    } else if (op.t == OP_SE) {
      E.slot_a[op.slot] = E.alloc<float>((size_t)B * ti.c * 2);
      E.slot_b[op.slot] = E.alloc<float>((size_t)B * op.cse);
      E.slot_c[op.slot] = E.alloc<float>((size_t)B * ti.c);
    }
  }
  E.side = E.alloc<double>(E.side_need);
  E.mov_tab = E.alloc<MovEntry>(std::max<size_t>(E.mov.size(), 1));
  if (!E.mov.empty())
    PHX_HIP(hipMemcpy(E.mov_tab, E.mov.data(), sizeof(MovEntry) * E.mov.size(), hipMemcpyHostToDevice));
  if (E.sync_need) E.sync_sums = E.alloc<double>(E.sync_need);
  E.spart = E.alloc<float2>(E.sp_region * E.nreg);
  E.scnt = E.alloc<float>(E.sc_region * E.nreg);
  E.stat_P.assign(P.tensors.size(), 0);
  E.stat_region.assign(P.tensors.size(), 0);
  E.gstat_region.assign(P.ops.size(), 0);
  E.pool_amax.assign(P.ops.size(), nullptr);
  for (size_t i = 0; i < P.ops.size(); ++i)
    if (P.ops[i].t == OP_MAXPOOL) E.pool_amax[i] = E.alloc<uint8_t>(P.tensors[P.ops[i].out].numel());
  E.gpart = E.alloc<float>(E.gp_need);
  E.red = E.alloc<double>(E.red_need);
  E.coef = E.alloc<float>(E.coef_need);
  E.se_g = E.alloc<float>(E.seg_need);
  // level tables (class / box outputs)
  const int nlev = (int)E.lev.size();
  E.lev_dev = E.alloc<LevelDesc>(nlev);
  PHX_HIP(hipMemcpy(E.lev_dev, E.lev.data(), nlev * sizeof(LevelDesc), hipMemcpyHostToDevice));
  E.dxoff_dev = E.alloc<long>(nlev);
  PHX_HIP(hipMemcpy(E.dxoff_dev, E.dxoff.data(), nlev * sizeof(long), hipMemcpyHostToDevice));
  // post-processing buffers
  const long BA = (long)B * A;
  E.scores = E.alloc<float>(BA);
  E.classes = E.alloc<int>(BA);
  E.boxes = E.alloc<float>(BA * 4);
  E.keep = E.alloc<uint8_t>(BA);
  E.cand_list = E.alloc<int>(BA);
  E.cand_count = E.alloc<int>(B);
  PHX_HIP(hipMemset(E.cand_count, 0, (size_t)B * sizeof(int)));
  E.nms_ws = E.alloc<float>(soft_nms_work_floats(B, A));
  E.nms1_boxes = E.alloc<float>((size_t)B * PHX_MAX_OUT * 4);
  E.nms1_scores = E.alloc<float>((size_t)B * PHX_MAX_OUT);
  E.nms1_count = E.alloc<int>(B);
  E.nms2_boxes = E.alloc<float>((size_t)B * PHX_MAX_OUT * 4);
  E.nms2_scores = E.alloc<float>((size_t)B * PHX_MAX_OUT);
  E.nms2_count = E.alloc<int>(B);
  E.mraw = E.alloc<float>(B);
  E.dm = E.alloc<float>(B);
  E.argm = E.alloc<int>(B);
  E.nties = E.alloc<int>(B);
  E.imax_scratch = E.alloc<int>(image_max_scratch_ints(B));
  if (P.box_grad) {
    const size_t ng = (size_t)B * kIdiouMaxGt;
    E.bl_max = E.alloc<float>(ng);
    E.bl_anchor = E.alloc<int>(ng);
    E.bl_nties = E.alloc<int>(ng);
    E.bl_img = E.alloc<float>(B);
    E.bl_batch = E.alloc<float>(1);
    E.bl_scratch = E.alloc<int>(idiou_scratch_ints(B, A));
    E.dxoff_box_dev = E.alloc<long>(nlev);
    if ((int)E.dxoff_box.size() != nlev) throw std::logic_error("box loss: no box-predict gradient offsets in the plan");
    PHX_HIP(hipMemcpy(E.dxoff_box_dev, E.dxoff_box.data(), nlev * sizeof(long), hipMemcpyHostToDevice));
  }
  // EOT
  const int S = E.ed.H;
  const long nslot = (long)B * PHX_MAX_OUT;
  E.img = E.alloc<ImgParams>(B);
  E.place = reinterpret_cast<BoxPlace*>(E.alloc<char>(eot_place_bytes(B, PHX_MAX_OUT)));
  E.spans = E.alloc<SpanEntry>(nslot * S);
  E.ysum = E.alloc<double>((size_t)B * 2 * 64);
  E.ymean = E.alloc<float>((size_t)B * 2);
  // the resized patches; reused by the resize adjoint's row buffer once the rotation backward
  // has consumed them
  // (the concurrent first pass's and the serving executor run no EOT: their patch stores stay one element)
  const bool eot = E.tag == 0;
  E.rstore = E.alloc<float>(eot ? std::max(E.ed.rcap, eot_resize_scratch_floats(E.ed)) : 1);
  E.dstore = E.alloc<float>(eot ? E.ed.rcap : 1);
  const size_t np = (size_t)PHX_PATCH_SIZE * PHX_PATCH_SIZE * 3;
  E.matched = E.alloc<float>(eot ? np * B : 1);
  E.dmatched = E.alloc<float>(eot ? np * B : 1);
  // the histogram matcher's chunk counts (128 KB per image) and tables, held whichever matcher is
  // selected so that no step allocates
  E.hpart = E.alloc<int>(eot ? eot_hist_part_ints(B) : 1);
  E.hlut = E.alloc<float>(eot ? (size_t)B * 256 : 1);
  E.dsum = E.alloc<double>((size_t)B * 64);
  E.tvs = E.alloc<double>(256);
  E.err = E.alloc<int>(1);
  E.patched = E.alloc<float>(eot ? (size_t)B * S * S * 3 : 1);
  E.owner = E.alloc<int16_t>(eot ? (size_t)B * S * S * 3 : 1);
  if (E.ndrop) {
    E.drop_block = E.alloc<int>(E.ndrop);
    E.drop_p = E.alloc<float>(E.ndrop);
    E.drop_keep = E.alloc<float>((size_t)E.ndrop * B);
    PHX_HIP(hipMemcpy(E.drop_block, E.drop_blocks.data(), E.ndrop * sizeof(int), hipMemcpyHostToDevice));
    PHX_HIP(hipMemcpy(E.drop_p, E.drop_surv.data(), E.ndrop * sizeof(float), hipMemcpyHostToDevice));
  }
  E.inj_boxes = E.alloc<float>((size_t)B * PHX_MAX_OUT * 4);
  E.inj_count = E.alloc<int>(B);
  E.dscale_scratch = E.alloc<float>(1);
}

}  // namespace

Exec& phx_ctx::exec_for(int B, int tag) {
  ++clock;
  for (auto& e : execs)
    if (e->B == B && e->tag == tag) {
      e->used = clock;
      return *e;
    }
  if (execs.size() >= kMaxExecs) {
    size_t lru = 0;
    auto older = [&](size_t i, size_t j) {
      if (execs[i]->tag != execs[j]->tag) return execs[i]->tag > execs[j]->tag;
      return execs[i]->used < execs[j]->used;
    };
    for (size_t i = 1; i < execs.size(); ++i)
      if (older(i, lru)) lru = i;
    PHX_HIP(hipDeviceSynchronize());
    if (last == execs[lru].get()) last = nullptr;
    if (execs[lru]->tag == 1) pre = Pre{};  // a prefetched first pass lives in the side executor
    sum_clobber(*execs[lru]);
    execs.erase(execs.begin() + (long)lru);
  }
  // (the box-regression term changes the step executor's backward plan only: tags 1 and 2 run forwards)
  auto ex = std::make_unique<Exec>(plan_exec(mc, B, tag, bn_mode, bf16, A, tag == 0 && box_loss != PHX_BOX_LOSS_NONE));
  alloc_exec(*ex, A);
  ex->used = clock;
  execs.push_back(std::move(ex));
  return *execs.back();
}

namespace phx {

// How consumers see tensor t: BN outputs are virtual (BN input + per-channel transform).
static InX view(phx_ctx* ctx, const Exec& E, int t, const float* input) {
  int bi = E.bn_of_tensor[t];
  if (bi < 0) return InX{E.tptr(t, input), nullptr, nullptr, nullptr, 0, E.tbf(t)};
  const Op& op = E.prog.ops[bi];
  return InX{E.tptr(op.in[0], input), E.slot_a[op.slot], E.slot_c[op.slot], ctx->w() + op.beta, op.act,
             E.tbf(op.in[0])};
}

// The gradient w.r.t. tensor t as its producer's dgrad sees it: for a BN input the BN backward
// is applied on load (GradX); otherwise the materialised gradient.
static GradX gview(phx_ctx* ctx, const Exec& E, int t, const float* input) {
  int bi = E.bn_consumer[t];
  if (bi >= 0 && E.prog.ops[bi].bwd) {
    const Op& op = E.prog.ops[bi];
    return GradX{E.gptr(op.out), E.tptr(t, input), E.slot_a[op.slot], E.slot_b[op.slot],
                 E.slot_c[op.slot], ctx->w() + op.beta, E.slot_d[op.slot], E.slot_e[op.slot], op.act, E.tbf(t)};
  }
  return GradX{E.gptr(t), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
}

// Work-skipping timing diagnostics (wrong results), compiled in only with -DPHX_DEBUG_KNOBS=1 (make
// DEBUG_KNOBS=1): the shipped library ignores PHX_SKIP_TIMING / PHX_SKIP_KINDS / PHX_NO_DROP, so no
// environment can make a measured step skip work (bench.py also refuses to run with them set).
#if defined(PHX_DEBUG_KNOBS) && PHX_DEBUG_KNOBS
// PHX_SKIP_TIMING=f,b,s (timing experiments only: wrong results): skip the forward BN finalizes (f),
// the backward ones (b), the SE MLP launches (s) — what removing them would be worth at most
static bool skip_timing(char k) {
  static const std::string v = [] {
    const char* e = std::getenv("PHX_SKIP_TIMING");
    return std::string(e ? e : "");
  }();
  return v.find(k) != std::string::npos;
}

// PHX_SKIP_KINDS=f:gemm,b:dw_bwd,...|name1,name2 (timing experiments only: wrong results): skip the
// ungrouped launches of those kinds (f: forward, b: backward), or of ops whose name contains one of
// the names after '|'
static bool skip_kind(const std::string& kind, const std::string& name) {
  static const std::pair<std::vector<std::string>, std::vector<std::string>> v = [] {
    std::pair<std::vector<std::string>, std::vector<std::string>> r;
    const char* e = std::getenv("PHX_SKIP_KINDS");
    std::string t = e ? e : "";
    const size_t bar = t.find('|');
    auto split = [](const std::string& x, std::vector<std::string>& out) {
      size_t a = 0;
      while (a < x.size()) {
        size_t b = x.find(',', a);
        if (b == std::string::npos) b = x.size();
        if (b > a) out.push_back(x.substr(a, b - a));
        a = b + 1;
      }
    };
    split(t.substr(0, bar), r.first);
    if (bar != std::string::npos) split(t.substr(bar + 1), r.second);
    return r;
  }();
  if (v.first.empty() && v.second.empty()) return false;
  for (const auto& k : v.first)
    if (k == kind) return true;
  for (const auto& n : v.second)
    if (name.find(n) != std::string::npos) return true;
  return false;
}
#else
static bool skip_timing(char) { return false; }
static bool skip_kind(const std::string&, const std::string&) { return false; }
#endif

// ---- PHX_CKSUM diagnostics -----------------------------------------------------------------
// Read per call, so one process can compare a one-stream step with concurrent ones op by op: the
// first checksum that differs between two steps on the same inputs names the launch whose inputs
// still agreed and whose output did not.
static bool cksum_env() {
  return env_flag("PHX_CKSUM");
}

void ck_begin(Exec& E, hipStream_t s) {
  E.ck_on = cksum_env();
  E.ck_names.clear();
  if (!E.ck_on) return;
  if (!E.ck) {
    E.ck_cap = 8 * E.prog.ops.size() + 256;
    E.ck = E.alloc<unsigned long long>(E.ck_cap);
  }
  PHX_HIP(hipMemsetAsync(E.ck, 0, E.ck_cap * sizeof(unsigned long long), s));
}

void ck_note(Exec& E, const std::string& name, const void* p, size_t bytes, hipStream_t s) {
  if (!E.ck_on || !p || E.ck_names.size() >= E.ck_cap) return;
  launch_cksum(p, bytes, E.ck + E.ck_names.size(), s);
  E.ck_names.push_back(name);
}

// what forward op i wrote (every member, for a grouped launch)
static void ck_fwd(Exec& E, int i, int pass, hipStream_t s) {
  if (!E.ck_on) return;
  const Program& P = E.prog;
  const Op& op = P.ops[i];
  if (E.fuse_folded[i] || E.sep[i]) return;  // (never stored)
  const std::string nm = "p" + std::to_string(pass) + " f " + std::to_string(i) + " " + op.name;
  const Tensor& ti = P.tensors[op.in[0]];
  if (op.t == OP_BN) {
    ck_note(E, nm + " mean", E.slot_a[op.slot], ti.c * 4, s);
    ck_note(E, nm + " rstd", E.slot_b[op.slot], ti.c * 4, s);
    ck_note(E, nm + " scale", E.slot_c[op.slot], ti.c * 4, s);
  } else if (op.t == OP_SE) {
    ck_note(E, nm + " excite", E.slot_c[op.slot], (size_t)E.B * ti.c * 4, s);
  } else {
    const Tensor& to = P.tensors[op.out];
    ck_note(E, nm + " out", E.tptr(op.out, nullptr), to.numel() * (E.tbf(op.out) ? 2 : 4), s);
  }
}

// the forward outputs of pass `pass` once more, as "post <name>" (after the step's join)
void ck_post(Exec& E, int pass, hipStream_t s) {
  const size_t n0 = E.ck_names.size();
  for (size_t i = 0; i < E.prog.ops.size(); ++i) ck_fwd(E, (int)i, pass, s);
  for (size_t k = n0; k < E.ck_names.size(); ++k) E.ck_names[k] = "post " + E.ck_names[k];
}

// what backward op i wrote: its inputs' gradients (BN: the backward means)
static void ck_bwd(Exec& E, int i, hipStream_t s) {
  if (!E.ck_on) return;
  const Program& P = E.prog;
  const Op& op = P.ops[i];
  const std::string nm = "b " + std::to_string(i) + " " + op.name;
  if (op.t == OP_SE && E.sefold[i]) {
    // its input's gradient is never stored: the head of that slot holds dpool [B][C]
    const Tensor& ti = P.tensors[op.in[0]];
    ck_note(E, nm + " dpool", E.gptr(op.in[0]), (size_t)ti.n * ti.c * 4, s);
    return;
  }
  if (op.t == OP_BN) {
    const int C = P.tensors[op.in[0]].c;
    ck_note(E, nm + " mdz", E.slot_d[op.slot], C * 4, s);
    ck_note(E, nm + " mdzx", E.slot_e[op.slot], C * 4, s);
    return;
  }
  for (int k = 0; k < op.nin; ++k)
    if (const float* g = E.gptr(op.in[k])) ck_note(E, nm + " d" + std::to_string(k), g, P.tensors[op.in[k]].numel() * 4, s);
}

// PHX_FROZEN_REUSE=0: every inference pass recomputes its BN statistics (A/B; read per call)
static bool frozen_reuse_off() {
  return !env_on("PHX_FROZEN_REUSE");
}


// bn=sync: the BN sums of `segs` (fold -> the caller's all-reduce -> statistics from the global sums)
// bn=sync: all-reduce the sums of `n` members already in E.sync_sums, then their statistics
static void sync_reduce_apply(phx_ctx* ctx, Exec& E, const BnFinSeg* segs, int n, int C, bool bwd, hipStream_t s) {
  if (!ctx->ar_fn) throw std::logic_error("bn=sync: no collective registered (phx_set_allreduce)");
  if (ctx->ar_fn(ctx->ar_user, E.sync_sums, (size_t)n * C * 3, s) != 0)
    throw std::runtime_error("bn=sync: the all-reduce callback failed");
  launch_bn_from_sums(segs, n, C, bwd, E.sync_sums, kBnEps, s);
}

static void sync_finalize(phx_ctx* ctx, Exec& E, const BnFinSeg* segs, int n, int C, bool bwd, hipStream_t s) {
  if (!ctx->ar_fn) throw std::logic_error("bn=sync: no collective registered (phx_set_allreduce)");
  launch_bn_fold_sums(segs, n, C, bwd, E.sync_sums, s);
  sync_reduce_apply(ctx, E, segs, n, C, bwd, s);
}

static void run_group_fwd(phx_ctx* ctx, Exec& E, int gid, const float* input, hipStream_t s, bool frozen) {
  const Program& P = E.prog;
  const std::vector<int>& g = E.groups[gid];
  const int n = (int)g.size();
  const Op& o0 = P.ops[g[0]];
  const Tensor& ti0 = P.tensors[o0.in[0]];
  const Tensor& to0 = P.tensors[o0.out];
  float* W = ctx->w();
  const bool sink_on = !frozen && g[0] + 1 < (int)P.ops.size() && E.fused_bn[g[0] + 1];
  auto sink_of = [&](int r) {
    return sink_on ? StatSink{E.spart + (size_t)r * E.sp_region, E.scnt + (size_t)r * E.sc_region, to0.c, 0}
                   : StatSink{};
  };
  double fl = 0, by = 0;
  for (int i : g) {
    const Tensor& ti = P.tensors[P.ops[i].in[0]];
    const Tensor& to = P.tensors[P.ops[i].out];
    if (o0.t == OP_PW) fl += 2.0 * ti.rows() * ti.c * to.c;
    if (o0.t == OP_DW) fl += 2.0 * to.numel() * o0.k * o0.k;
    by += o0.t == OP_BN ? 8.0 * (double)E.stat_P[P.ops[i].in[0]] * ti.c : 4.0 * (double)(ti.numel() + to.numel());
  }
  if (o0.t == OP_PW) by += 4.0 * ti0.c * to0.c;
  Scope scope(ctx, o0.t == OP_PW ? "gemm" : o0.t == OP_DW ? "dw_fwd" : "bn_stats", fl, by, s,
              prof_detail() ? " group" + op_tag(P, o0, false) : std::string());
  switch (o0.t) {
    case OP_DW: {
      DwSeg segs[kMaxSeg];
      int nps[kMaxSeg];
      for (int r = 0; r < n; ++r) {
        const Op& op = P.ops[g[r]];
        const Tensor& ti = P.tensors[op.in[0]];
        const Tensor& to = P.tensors[op.out];
        segs[r] = DwSeg{view(ctx, E, op.in[0], input), GradX{}, E.tptr(op.out, input), ti.h, ti.w, to.h, to.w,
                        op.pad_t, op.pad_l, false, sink_of(r), GradSink{}};
      }
      launch_dw_fwd_group(segs, n, ti0.n, ti0.c, W + o0.w, o0.k, o0.stride, s, nps);
      if (sink_on)
        for (int r = 0; r < n; ++r) {
          E.stat_P[P.ops[g[r]].out] = nps[r];
          E.stat_region[P.ops[g[r]].out] = r;
        }
      break;
    }
    case OP_PW: {
      GemmSeg segs[kMaxSeg];
      const int mode = view(ctx, E, o0.in[0], input).mu ? 1 : 0;
      for (int r = 0; r < n; ++r) {
        const Op& op = P.ops[g[r]];
        segs[r] = GemmSeg{view(ctx, E, op.in[0], input), GradX{}, op.b >= 0 ? W + op.b : nullptr,
                          E.tptr(op.out, input), (int)P.tensors[op.in[0]].rows(), false, sink_of(r), GradSink{}};
      }
      int np[kMaxSeg];  // each member's statistics partial rows
      gemm_group_run(mode, segs, n, ctx->wt_of(o0.w), to0.c, ti0.c, s, E.bf16, np,
                     std::min<long>((long)(E.sp_region / to0.c), (long)E.sc_region));
      if (sink_on)
        for (int r = 0; r < n; ++r) {
          E.stat_P[P.ops[g[r]].out] = np[r];
          E.stat_region[P.ops[g[r]].out] = r;
        }
      break;
    }
    case OP_BN: {
      if (frozen) {  // inference BN (test_step): statistics from the moving averages
        if (E.frozen_ver == ctx->w_ver && !frozen_reuse_off()) break;  // (kept from the last inference pass)
        for (int r = 0; r < n; ++r) {
          const Op& op = P.ops[g[r]];
          launch_bn_frozen_stats(W + op.mmean, W + op.mvar, E.slot_a[op.slot], E.slot_b[op.slot],
                                 W + op.gamma, E.slot_c[op.slot], ti0.c, kBnEps, s);
        }
        break;
      }
      BnFinSeg segs[kMaxSeg];
      for (int r = 0; r < n; ++r) {
        const Op& op = P.ops[g[r]];
        const int reg = E.stat_region[op.in[0]];
        segs[r] = BnFinSeg{E.spart + (size_t)reg * E.sp_region, E.scnt + (size_t)reg * E.sc_region,
                           E.stat_P[op.in[0]], (long)P.tensors[op.in[0]].rows(), E.slot_a[op.slot],
                           E.slot_b[op.slot], W + op.gamma, E.slot_c[op.slot], W + op.mmean, W + op.mvar,
                           nullptr, nullptr, E.side_for(op.slot)};
      }
      if (ctx->bn_mode == PHX_BN_SYNC) sync_finalize(ctx, E, segs, n, ti0.c, false, s);
      else if (!skip_timing('f')) launch_bn_finalize_group(segs, n, ti0.c, kBnEps, s);
      break;
    }
    default:
      throw std::logic_error("grouped launch of an unsupported op");
  }
}

static void run_group_bwd(phx_ctx* ctx, Exec& E, int gid, const float* input, hipStream_t s) {
  const Program& P = E.prog;
  const std::vector<int>& g = E.groups[gid];
  const int n = (int)g.size();
  const Op& o0 = P.ops[g[0]];
  const Tensor& ti0 = P.tensors[o0.in[0]];
  const Tensor& to0 = P.tensors[o0.out];
  float* W = ctx->w();
  const bool gs_on = g[0] > 0 && E.gfused_bn[g[0] - 1];
  auto gsk_of = [&](int r) {
    if (!gs_on) return GradSink{};
    const Op& bn = P.ops[g[r] - 1];
    return GradSink{E.spart + (size_t)r * E.sp_region, P.tensors[bn.out].c, 0, E.tptr(bn.in[0], input),
                    E.slot_a[bn.slot], E.slot_b[bn.slot], E.slot_c[bn.slot], W + bn.beta, bn.act, E.tbf(bn.in[0])};
  };
  double fl = 0, by = 0;
  for (int i : g) {
    const Tensor& ti = P.tensors[P.ops[i].in[0]];
    const Tensor& to = P.tensors[P.ops[i].out];
    if (o0.t == OP_PW) fl += 2.0 * ti.rows() * ti.c * to.c;
    if (o0.t == OP_DW) fl += 2.0 * to.numel() * o0.k * o0.k;
    by += o0.t == OP_BN ? 8.0 * (double)E.gstat_P[i] * ti.c : 4.0 * (double)(ti.numel() + to.numel());
    if (o0.t != OP_BN) {
      const int bi = E.bn_consumer[P.ops[i].out];
      if (bi >= 0 && P.ops[bi].bwd) by += 4.0 * (double)to.numel();
      if (P.ops[i].acc[0]) by += 4.0 * (double)ti.numel();
    }
  }
  if (o0.t == OP_PW) by += 4.0 * ti0.c * to0.c;
  Scope scope(ctx, o0.t == OP_PW ? "gemm" : o0.t == OP_DW ? "dw_bwd" : "bn_bwd_reduce", fl, by, s,
              prof_detail() ? " group" + op_tag(P, o0, true) : std::string());
  switch (o0.t) {
    case OP_DW: {
      DwSeg segs[kMaxSeg];
      int nps[kMaxSeg];
      for (int r = 0; r < n; ++r) {
        const Op& op = P.ops[g[r]];
        const Tensor& ti = P.tensors[op.in[0]];
        const Tensor& to = P.tensors[op.out];
        segs[r] = DwSeg{InX{}, gview(ctx, E, op.out, input), E.gptr(op.in[0]), ti.h, ti.w, to.h, to.w, op.pad_t,
                        op.pad_l, op.acc[0], StatSink{}, gsk_of(r)};
      }
      launch_dw_bwd_group(segs, n, ti0.n, ti0.c, W + o0.w, o0.k, o0.stride, s, nps);
      if (gs_on)
        for (int r = 0; r < n; ++r) {
          E.gstat_P[g[r] - 1] = nps[r];
          E.gstat_region[g[r] - 1] = r;
        }
      break;
    }
    case OP_PW: {
      GemmSeg segs[kMaxSeg];
      const GradX gx0 = gview(ctx, E, o0.out, input);
      const int mode = gx0.y ? 3 : 0;
      for (int r = 0; r < n; ++r) {
        const Op& op = P.ops[g[r]];
        const GradX gv = gview(ctx, E, op.out, input);
        segs[r] = GemmSeg{InX{gv.da, nullptr, nullptr, nullptr, 0}, gv, nullptr, E.gptr(op.in[0]),
                          (int)P.tensors[op.in[0]].rows(), op.acc[0], StatSink{}, gsk_of(r)};
      }
      // dX[M,Cin] = dY[M,Cout] * W^T : Bt = W in HWIO layout [Cin][Cout]
      int np[kMaxSeg];  // each member's BN-backward-sum partial rows
      gemm_group_run(mode, segs, n, W + o0.w, ti0.c, to0.c, s, E.bf16, np, (long)(E.sp_region / ti0.c));
      if (gs_on)
        for (int r = 0; r < n; ++r) {
          E.gstat_P[g[r] - 1] = np[r];
          E.gstat_region[g[r] - 1] = r;
        }
      break;
    }
    case OP_BN: {
      if (ctx->bn_mode == PHX_BN_FROZEN) break;
      BnFinSeg segs[kMaxSeg];
      for (int r = 0; r < n; ++r) {
        const int i = g[r];
        const Op& op = P.ops[i];
        segs[r] = BnFinSeg{E.spart + (size_t)E.gstat_region[i] * E.sp_region, nullptr, E.gstat_P[i],
                           (long)P.tensors[op.in[0]].rows(), nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, E.slot_d[op.slot], E.slot_e[op.slot]};
      }
      if (ctx->bn_mode == PHX_BN_SYNC) sync_finalize(ctx, E, segs, n, ti0.c, true, s);
      else if (!skip_timing('b')) launch_bn_bwd_finalize_group(segs, n, ti0.c, s);
      break;
    }
    default:
      throw std::logic_error("grouped launch of an unsupported op");
  }
}

// the fused separable conv whose depthwise op is i (its group's members when grouped): the depthwise
// op's input view — the BiFPN node fuse computed on load when that fuse is folded — the pointwise op's
// weights and output, and the BN after it takes its statistics from this launch
static void run_sep(phx_ctx* ctx, Exec& E, int i, const float* input, hipStream_t s, bool frozen) {
  const Program& P = E.prog;
  float* W = ctx->w();
  const int gd = E.grp_of[i];
  const std::vector<int> mem = gd >= 0 ? E.groups[gd] : std::vector<int>{i};
  const int n = (int)mem.size();
  const Op& d0 = P.ops[mem[0]];
  const Op& p0 = P.ops[mem[0] + 1];
  const int C = P.tensors[d0.in[0]].c, N = P.tensors[p0.out].c;
  const bool sink_on = !frozen && mem[0] + 2 < (int)P.ops.size() && E.fused_bn[mem[0] + 2];
  SepMember m[kMaxSeg];
  double fl = 0, by = 4.0 * (9.0 * C + (double)N * C + N);
  for (int r = 0; r < n; ++r) {
    const int di = mem[r];
    const Op& d = P.ops[di];
    const Op& pw = P.ops[di + 1];
    const Tensor& ti = P.tensors[d.in[0]];
    SepMember& mm = m[r];
    mm = SepMember{};
    if (di > 0 && E.fuse_folded[di - 1]) {
      const Op& f = P.ops[di - 1];
      mm.fuse = true;
      mm.f.nin = f.nin;
      for (int k = 0; k < f.nin; ++k) {
        mm.f.x[k] = view(ctx, E, f.in[k], input);
        mm.f.w[k] = f.wsm[k] >= 0 ? W + f.wsm[k] : nullptr;
      }
      mm.f.method = f.fuse_method;
      mm.f.act = f.act;
      by += 4.0 * (double)ti.numel() * (f.nin - 1);
    } else {
      mm.x = view(ctx, E, d.in[0], input);
    }
    mm.y = E.tptr(pw.out, input);
    mm.H = ti.h;
    mm.W = ti.w;
    if (sink_on)
      mm.sink = StatSink{E.spart + (size_t)r * E.sp_region, E.scnt + (size_t)r * E.sc_region, N, 0};
    fl += 2.0 * ti.numel() * 9.0 + 2.0 * (double)ti.rows() * C * N;
    by += 4.0 * ((double)ti.numel() + (double)ti.rows() * N);
  }
  Scope scope(ctx, "sep_fwd", fl, by, s,
              prof_detail() ? std::string(n > 1 ? " group" : "") + op_tag(P, p0, false) : std::string());
  int nps[kMaxSeg];
  launch_sep_fwd(m, n, E.B, C, N, W + d0.w, ctx->wt_of(p0.w), p0.b >= 0 ? W + p0.b : nullptr, s, nps);
  if (sink_on)
    for (int r = 0; r < n; ++r) {
      E.stat_P[P.ops[mem[r] + 1].out] = nps[r];
      E.stat_region[P.ops[mem[r] + 1].out] = r;
    }
}

// victim forward over the program (EfficientDetNet.call, efficientdet_keras.py:884-906)
// pass: 0 first (clean) pass, 1 second (patched) pass, 2 standalone detect — with `step` and the
// global index of the first image it keys the drop-connect draws
static DropView drop_view(const Exec& E, int op) {
  const int d = E.drop_slot.empty() ? -1 : E.drop_slot[op];
  if (d < 0) return DropView{};
  const Tensor& t = E.prog.tensors[E.prog.ops[op].out];
  return DropView{E.drop_keep + (long)d * E.B, E.prog.ops[op].survival, (long)t.h * t.w};
}

// train = false: Keras training=False (test_step, attacker.py:325) — inference BN from the moving
// statistics (not updated) and no drop connect, whatever the context's BN mode
// force_frozen: inference BN in a training pass (a victim whose layers are not trainable, as the
// defender's protege, attack_detection.py:46-47); drop connect still follows `train`
void run_forward(phx_ctx* ctx, Exec& E, const float* input, hipStream_t s, int pass, int64_t step,
                 int gimg0, bool train, bool force_frozen) {
  const Program& P = E.prog;
  float* W = ctx->w();
  struct PlanImages {
    int& n = gemm_plan_images();
    explicit PlanImages(int v) { n = v; }
    ~PlanImages() { n = 0; }
  } plan_images(E.infer_plan ? E.B : 0);
  const bool frozen = ctx->bn_mode == PHX_BN_FROZEN || !train || force_frozen;
  // inference BN: the statistics from the moving averages are a function of the weights, so the
  // slots keep them from the last inference pass at the same weights version (the frozen protege of
  // the defender: 108 launches per step saved); a training pass overwrites the slots and may move
  // the moving statistics
  const bool frozen_reuse = frozen && E.frozen_ver == ctx->w_ver && !frozen_reuse_off();
  if (!frozen) {
    E.frozen_ver = 0;
    ++ctx->w_ver;
  }
  if (E.ndrop && train)
    launch_drop_keep(E.drop_block, E.drop_p, E.ndrop, E.B, ctx->seed, step, gimg0, pass, E.drop_keep, s);
  if (E.ndrop && train) ck_note(E, "p" + std::to_string(pass) + " drop keep", E.drop_keep, (size_t)E.ndrop * E.B * 4, s);
  for (size_t i = 0; i < P.ops.size(); ++i) {
    if (ctx->fwd_hook && i == ctx->fwd_hook_at) {
      auto h = std::move(ctx->fwd_hook);
      ctx->fwd_hook = nullptr;
      h();
    }
    if (E.grp_of[i] >= 0) {
      if (E.groups[E.grp_of[i]].front() == (int)i) {
        if (E.sep[i]) {
          run_sep(ctx, E, (int)i, input, s, frozen);
          for (int m : E.groups[E.grp_of[i]]) ck_fwd(E, m + 1, pass, s);
        } else if (!(i > 0 && E.sep[i - 1])) {  // (a fused sepconv's pointwise group: done above)
          run_group_fwd(ctx, E, E.grp_of[i], input, s, frozen);
          for (int m : E.groups[E.grp_of[i]]) ck_fwd(E, m, pass, s);
        }
      }
      continue;
    }
    if (E.fuse_folded[i]) continue;  // computed by the depthwise conv that follows
    if (E.sep[i]) {  // depthwise + pointwise in one launch
      run_sep(ctx, E, (int)i, input, s, frozen);
      ck_fwd(E, (int)i + 1, pass, s);
      continue;
    }
    if (i > 0 && E.sep[i - 1]) continue;  // (the pointwise half of the fused sepconv above)
    const Op& op = P.ops[i];
    const Tensor& ti = P.tensors[op.in[0]];
    const Tensor& to = P.tensors[op.out];
    float* x = E.tptr(op.in[0], input);
    float* y = E.tptr(op.out, input);
    double fl = 0, by = 4.0 * (double)(ti.numel() + to.numel());
    const char* kind = "fwd_other";
    switch (op.t) {
      case OP_STEM: kind = "stem_fwd"; fl = 2.0 * to.numel() * 27; break;
      case OP_PW: kind = "gemm"; fl = 2.0 * ti.rows() * ti.c * to.c; by += 4.0 * ti.c * to.c; break;
      case OP_DW: kind = "dw_fwd"; fl = 2.0 * to.numel() * op.k * op.k; break;
      case OP_BN: kind = "bn_stats"; by = 4.0 * ti.numel(); break;
      case OP_SE: kind = "se_fwd"; by = 4.0 * ti.numel(); break;
      default: break;
    }
    // the BN right after this op takes its statistics from this launch (StatSink)
    const bool sink_on = !frozen && i + 1 < P.ops.size() && E.fused_bn[i + 1];
    const StatSink sink = sink_on ? StatSink{E.spart, E.scnt, to.c, 0}
                                  : StatSink{};
    if (op.t == OP_BN && E.fused_bn[i]) by = 8.0 * (double)E.stat_P[op.in[0]] * ti.c;
    if (skip_kind(std::string("f:") + kind, op.name)) continue;
    Scope scope(ctx, kind, fl, by, s, (prof_detail() || debug_sync()) ? op_tag(P, op, false) : std::string());
    int np = 0;
    switch (op.t) {
      case OP_STEM:
        np = launch_stem_fwd(x, W + op.w, y, ti.n, ti.h, ti.w, to.h, to.w, to.c, op.pad_t, op.pad_l, s, sink,
                             E.tbf(op.out) != 0);
        break;
      case OP_PW: {
        InX A = view(ctx, E, op.in[0], input);
        const float* rs = nullptr;
        int rpi = 1;
        int se = E.se_of_tensor[op.in[0]];
        if (se >= 0) {  // SE excitation folded into the GEMM's A load
          const Op& sop = P.ops[se];
          A = view(ctx, E, sop.in[0], input);
          rs = E.slot_c[sop.slot];
          rpi = ti.h * ti.w;
        }
        np = launch_gemm(A, ctx->wt_of(op.w), op.b >= 0 ? W + op.b : nullptr, y, (int)ti.rows(), to.c,
                         ti.c, false, rs, rpi, s, E.gpart, sink, E.bf16);
        break;
      }
      case OP_DW:
        if (i > 0 && E.fuse_folded[i - 1]) {
          const Op& f = P.ops[i - 1];
          FuseView fv{};
          fv.nin = f.nin;
          for (int k = 0; k < f.nin; ++k) {
            fv.x[k] = view(ctx, E, f.in[k], input);
            fv.w[k] = f.wsm[k] >= 0 ? W + f.wsm[k] : nullptr;
          }
          fv.method = f.fuse_method;
          fv.act = f.act;
          launch_dw_fwd_fused(fv, W + op.w, y, ti.n, ti.h, ti.w, ti.c, to.h, to.w, op.k, op.stride, op.pad_t,
                              op.pad_l, s);
          break;
        }
        np = launch_dw_fwd(view(ctx, E, op.in[0], input), W + op.w, y, ti.n, ti.h, ti.w, ti.c, to.h, to.w, op.k,
                           op.stride, op.pad_t, op.pad_l, s, sink);
        break;
      case OP_BN: {
        float* mean = E.slot_a[op.slot];
        float* rstd = E.slot_b[op.slot];
        // statistics only: the normalised output is applied by every consumer on load (InX)
        if (frozen && frozen_reuse) {
        } else if (frozen)
          launch_bn_frozen_stats(W + op.mmean, W + op.mvar, mean, rstd, W + op.gamma,
                                 E.slot_c[op.slot], ti.c, kBnEps, s);
        else if (E.fused_bn[i] && ctx->bn_mode == PHX_BN_SYNC) {
          const BnFinSeg sg{E.spart + E.stat_region[op.in[0]] * E.sp_region,
                            E.scnt + E.stat_region[op.in[0]] * E.sc_region, E.stat_P[op.in[0]], (long)ti.rows(),
                            mean, rstd, W + op.gamma, E.slot_c[op.slot], W + op.mmean, W + op.mvar, nullptr, nullptr,
                            E.side_for(op.slot)};
          sync_finalize(ctx, E, &sg, 1, ti.c, false, s);
        } else if (E.fused_bn[i] && skip_timing('f')) {  // (timing diagnostics)
        } else if (E.fused_bn[i])
          launch_bn_finalize(E.spart + E.stat_region[op.in[0]] * E.sp_region,
                             E.scnt + E.stat_region[op.in[0]] * E.sc_region, E.stat_P[op.in[0]],
                             (long)ti.rows(), ti.c, mean, rstd,
                             W + op.gamma, E.slot_c[op.slot], W + op.mmean, W + op.mvar, kBnEps, s,
                             E.side_for(op.slot));
        else if (ctx->bn_mode == PHX_BN_SYNC) {
          launch_bn_stats_sums(x, (long)ti.rows(), ti.c, E.red, E.sync_sums, s, E.tbf(op.in[0]) != 0);
          const BnFinSeg sg{nullptr, nullptr, 0, (long)ti.rows(), mean, rstd, W + op.gamma, E.slot_c[op.slot],
                            W + op.mmean, W + op.mvar, nullptr, nullptr, E.side_for(op.slot)};
          sync_reduce_apply(ctx, E, &sg, 1, ti.c, false, s);
        }
        else
          launch_bn_stats(x, (long)ti.rows(), ti.c, E.red, mean, rstd, W + op.gamma,
                          E.slot_c[op.slot], W + op.mmean, W + op.mvar, kBnEps, s, E.tbf(op.in[0]) != 0,
                          E.side_for(op.slot));
        (void)y;
        break;
      }
      case OP_SE:
        if (skip_timing('s')) break;
        launch_se_fwd(view(ctx, E, op.in[0], input), nullptr, ti.n, ti.h * ti.w, ti.c, op.cse, W + op.w1, W + op.b1, W + op.w2,
                      W + op.b2, op.act, E.slot_a[op.slot], E.slot_b[op.slot], E.slot_c[op.slot], s,
                      E.red);
        break;
      case OP_ADD: {
#if defined(PHX_DEBUG_KNOBS) && PHX_DEBUG_KNOBS
        static const bool no_drop = env_flag("PHX_NO_DROP");  // PHX_NO_DROP=1: diagnostics only (not the reference's step)
#else
        constexpr bool no_drop = false;
#endif
        const DropView dv = (train && !no_drop) ? drop_view(E, (int)i) : DropView{};
        if (E.ck_on) {  // what the add is about to read (PHX_CKSUM)
          const std::string nm = "p" + std::to_string(pass) + " f " + std::to_string(i) + " add in ";
          for (int k = 0; k < 2; ++k) {
            const Tensor& tk = P.tensors[op.in[k]];
            ck_note(E, nm + std::to_string(k), E.tptr(op.in[k], input), tk.numel() * (E.tbf(op.in[k]) ? 2 : 4), s);
          }
          if (dv.keep) ck_note(E, nm + "keep", dv.keep, (size_t)E.B * 4, s);
        }
        launch_add(view(ctx, E, op.in[0], input), view(ctx, E, op.in[1], input), y,
                   (long)to.numel(), to.c, s, dv);
        break;
      }
      case OP_MAXPOOL:
        launch_maxpool_fwd(view(ctx, E, op.in[0], input), y, E.pool_amax[i], ti.n, ti.h, ti.w, ti.c, to.h, to.w, op.k, op.stride, op.pad_t,
                           op.pad_l, s);
        break;
      case OP_UPSAMPLE:
        launch_upsample_fwd(view(ctx, E, op.in[0], input), y, ti.n, ti.h, ti.w, ti.c, to.h, to.w, s);
        break;
      case OP_FUSE: {
        InX xs[3] = {};
        for (int k = 0; k < op.nin; ++k) xs[k] = view(ctx, E, op.in[k], input);
        launch_fuse_fwd(xs, op.nin, op.wsm[0] >= 0 ? W + op.wsm[0] : nullptr,
                        op.wsm[1] >= 0 ? W + op.wsm[1] : nullptr,
                        op.wsm[2] >= 0 ? W + op.wsm[2] : nullptr, op.fuse_method, op.act, y,
                        (long)to.numel(), to.c, s);
        break;
      }
    }
    if (sink_on) {
      E.stat_P[op.out] = np;
      E.stat_region[op.out] = 0;
    }
    ck_fwd(E, (int)i, pass, s);
  }
  if (frozen) E.frozen_ver = ctx->w_ver;
}

// the fused backward of the sepconv whose depthwise op is i (its group's members when grouped): dx of
// the depthwise input from the pointwise output's gradient view, and the BN-backward sums of the BN
// the depthwise conv reads
static void run_sep_bwd(phx_ctx* ctx, Exec& E, int i, const float* input, hipStream_t s) {
  const Program& P = E.prog;
  float* W = ctx->w();
  const int gd = E.grp_of[i];
  const std::vector<int> mem = gd >= 0 ? E.groups[gd] : std::vector<int>{i};
  const int n = (int)mem.size();
  const Op& d0 = P.ops[mem[0]];
  const Op& p0 = P.ops[mem[0] + 1];
  const int C = P.tensors[d0.in[0]].c, N = P.tensors[p0.out].c;
  const bool gs_on = mem[0] > 0 && E.gfused_bn[mem[0] - 1];
  SepBwdMember m[kMaxSeg];
  double fl = 0, by = 4.0 * (9.0 * C + (double)N * C);
  for (int r = 0; r < n; ++r) {
    const int di = mem[r];
    const Op& d = P.ops[di];
    const Op& pw = P.ops[di + 1];
    const Tensor& ti = P.tensors[d.in[0]];
    SepBwdMember& mm = m[r];
    mm = SepBwdMember{};
    mm.gv = gview(ctx, E, pw.out, input);
    mm.dx = E.gptr(d.in[0]);
    mm.H = ti.h;
    mm.W = ti.w;
    mm.acc = d.acc[0];
    if (gs_on) {
      const Op& bn = P.ops[di - 1];
      mm.gs = GradSink{E.spart + (size_t)r * E.sp_region, P.tensors[bn.out].c, 0, E.tptr(bn.in[0], input),
                       E.slot_a[bn.slot], E.slot_b[bn.slot], E.slot_c[bn.slot], W + bn.beta, bn.act, E.tbf(bn.in[0])};
    }
    fl += 2.0 * (double)ti.rows() * C * N + 2.0 * ti.numel() * 9.0;
    by += 4.0 * (3.0 * (double)ti.rows() * N + (d.acc[0] ? 2.0 : 1.0) * ti.numel() + (gs_on ? ti.numel() : 0.0));
  }
  Scope scope(ctx, "sep_bwd", fl, by, s,
              prof_detail() ? std::string(n > 1 ? " group" : "") + op_tag(P, p0, true) : std::string());
  int nps[kMaxSeg];
  launch_sep_bwd(m, n, E.B, C, N, W + d0.w, W + p0.w, s, nps);
  if (gs_on)
    for (int r = 0; r < n; ++r) {
      if (nps[r] != E.gstat_P[mem[r] - 1]) throw std::logic_error("sep bwd: planned and launched partial counts differ");
      E.gstat_region[mem[r] - 1] = r;
    }
}

// data-gradient of the victim from the sparse class-logit gradient (attacker.py:217)
void run_backward(phx_ctx* ctx, Exec& E, const float* input, hipStream_t s) {
  const Program& P = E.prog;
  float* W = ctx->w();
  const bool frozen = ctx->bn_mode == PHX_BN_FROZEN;
  const int na = ctx->mc.num_anchors();
  // 1. sparse class-head gradient into the inputs of the class-predict pointwise convs
  int K = 0;
  long wpred = -1;
  std::vector<std::pair<char*, size_t>> zero;  // the levels' gradient buffers, merged where adjacent
  int Kb = 0;
  long wbox = -1;
  for (int l = 0; l < (int)P.cls_out.size(); ++l) {
    for (const Op& op : P.ops) {
      const bool box = P.box_grad && op.out == P.box_out[l];
      if (op.out != P.cls_out[l] && !box) continue;
      const Tensor& ti = P.tensors[op.in[0]];
      zero.emplace_back(reinterpret_cast<char*>(E.gptr(op.in[0])), ti.numel() * sizeof(float));
      if (box) {
        Kb = ti.c;
        wbox = op.w;
      } else {
        K = ti.c;
        wpred = op.w;
      }
    }
  }
  std::sort(zero.begin(), zero.end());
  std::vector<char*> zp;
  std::vector<size_t> zb;
  for (size_t i = 0; i < zero.size();) {
    char* p0 = zero[i].first;
    char* p1 = p0 + zero[i].second;
    size_t j = i + 1;
    for (; j < zero.size() && zero[j].first <= p1; ++j) p1 = std::max(p1, zero[j].first + zero[j].second);
    zp.push_back(p0);
    zb.push_back((size_t)(p1 - p0));
    i = j;
  }
  // one launch for all of them (was one memset packet per level)
  bool aligned = zp.size() <= (size_t)kZeroSegs;
  for (size_t k = 0; k < zp.size(); ++k) aligned = aligned && ((reinterpret_cast<uintptr_t>(zp[k]) | zb[k]) & 15) == 0;
  if (aligned) launch_zero_segs(zp.data(), zb.data(), (int)zp.size(), s);
  else
    for (size_t k = 0; k < zp.size(); ++k) PHX_HIP(hipMemsetAsync(zp[k], 0, zb[k], s));
  launch_cls_scatter(E.scores, E.keep, E.mraw, E.nties, E.dm, E.tptr(P.cls_out[0], input),
                     E.lev_dev, (int)E.lev.size(), ctx->A, E.B, ctx->mc.num_classes, na,
                     W + wpred, K, E.grad, E.dxoff_dev, s, E.tbf(P.cls_out[0]));
  // 1b. the box-regression term's sparse gradient into the inputs of the box-predict pointwise convs
  if (P.box_grad) {
    if (!E.bl_valid || ctx->box_loss == PHX_BOX_LOSS_NONE) throw std::logic_error("box loss: backward without its forward");
    Scope scope(ctx, "box_scatter", 0.0, (double)E.B * (ctx->A / na) * 4.0, s);
    launch_box_scatter(E.boxes, E.keep, E.bl_gt, E.bl_gcount, E.bl_max, E.bl_anchor, E.bl_nties,
                       E.tptr(P.box_out[0], input), reinterpret_cast<const float*>(ctx->d_anchors.get()), E.lev_dev,
                       (int)E.lev.size(), ctx->A, E.B, na, W + wbox, Kb, ctx->box_w, E.grad, E.dxoff_box_dev, s);
  }
  // 2. reverse sweep
  for (int i = (int)P.ops.size() - 1; i >= 0; --i) {
    const Op& op = P.ops[i];
    if (!op.bwd) continue;
    if (op.t == OP_PW && is_scatter_out(P, op.out)) continue;  // handled by the scatters
    if (i > 0 && E.sepb[i - 1]) continue;  // (the pointwise half of a fused sepconv: with its depthwise op)
    if (E.grp_of[i] >= 0) {
      if (E.groups[E.grp_of[i]].back() == i) {
        if (E.sepb[i]) run_sep_bwd(ctx, E, i, input, s);
        else run_group_bwd(ctx, E, E.grp_of[i], input, s);
        for (int m : E.groups[E.grp_of[i]]) ck_bwd(E, m, s);
      }
      continue;
    }
    if (E.sepb[i]) {
      run_sep_bwd(ctx, E, i, input, s);
      ck_bwd(E, i, s);
      continue;
    }
    const bool se_fold = op.t == OP_SE && E.sefold[i];
    const bool dw_fold = op.t == OP_DW && i + 2 < (int)P.ops.size() && E.sefold[i + 2];
    const Tensor& ti = P.tensors[op.in[0]];
    const Tensor& to = P.tensors[op.out];
    const float* dy = E.gptr(op.out);
    float* dx = E.gptr(op.in[0]);
    double fl = 0, by = 4.0 * (double)(ti.numel() + to.numel());
    const char* kind = "bwd_other";
    switch (op.t) {
      case OP_STEM: kind = "stem_bwd"; fl = 2.0 * to.numel() * 27; break;
      case OP_PW: kind = "gemm"; fl = 2.0 * ti.rows() * ti.c * to.c; by += 4.0 * ti.c * to.c; break;
      case OP_DW: kind = "dw_bwd"; fl = 2.0 * to.numel() * op.k * op.k; break;
      case OP_BN: kind = "bn_bwd_reduce"; by = 4.0 * 2.0 * ti.numel(); break;
      case OP_SE: kind = "se_bwd"; by = 4.0 * (se_fold ? 2.0 : 3.0) * ti.numel(); break;
      default: break;
    }
    // algorithmic bytes of a dgrad: a gradient view also reads the BN input; accumulation
    // re-reads the destination
    if (op.t == OP_PW || op.t == OP_DW) {
      const int bi = E.bn_consumer[op.out];
      if (bi >= 0 && P.ops[bi].bwd) by += 4.0 * (double)to.numel();
      if (op.acc[0]) by += 4.0 * (double)ti.numel();
    }
    // the BN right before this op takes its backward sums from this op's dgrad (GradSink)
    GradSink gsk{};
    int gsk_in = -1;  // which input's gradient carries them
    if (i > 0 && E.gfused_bn[i - 1]) {
      const Op& bn = P.ops[i - 1];
      gsk = GradSink{E.spart, P.tensors[bn.out].c, 0, E.tptr(bn.in[0], input), E.slot_a[bn.slot],
                     E.slot_b[bn.slot], E.slot_c[bn.slot], W + bn.beta, bn.act, E.tbf(bn.in[0])};
      gsk_in = op.in[0] == bn.out ? 0 : 1;
    }
    if (op.t == OP_BN && E.gfused_bn[i]) by = 8.0 * (double)E.gstat_P[i] * ti.c;
    if (skip_kind(std::string("b:") + kind, op.name)) continue;
    Scope scope(ctx, kind, fl, by, s, (prof_detail() || debug_sync()) ? op_tag(P, op, true) : std::string());
    int np = -1;
    switch (op.t) {
      case OP_STEM: {
        GradX g = gview(ctx, E, op.out, input);
        // the image gradient feeds only the EOT backward, which reads it at owned pixels
        if (!op.acc[0] && stem_bwd_gx_supported(to.c)) {
          launch_stem_bwd_gx(g, W + op.w, E.owner, dx, ti.n, ti.h, ti.w, to.h, to.w, to.c, op.pad_t,
                             op.pad_l, s);
          break;
        }
        // the stem dgrad reads each dy element up to 4x: materialise the BN-backward output once
        float* gy = E.gptr(op.out);
        if (g.y) launch_bn_bwd_apply2(g, gy, (long)to.rows(), to.c, s);
        launch_stem_bwd(g.y ? gy : g.da, W + op.w, dx, ti.n, ti.h, ti.w, to.h, to.w, to.c, op.pad_t, op.pad_l,
                        op.acc[0], s);
        break;
      }
      case OP_PW:
        // dX[M,Cin] = dY[M,Cout] * W^T : Bt = W in HWIO layout [Cin][Cout]
        np = launch_gemm_dgrad(gview(ctx, E, op.out, input), W + op.w, dx, (int)ti.rows(), ti.c, to.c,
                               op.acc[0], s, E.gpart, gsk, E.bf16);
        break;
      case OP_DW:
        if (dw_fold) {
          // the BN output's gradient is formed on load from the SE output's gradient, s and dpool
          const Op& se = P.ops[i + 2];
          const Tensor& tb = P.tensors[se.in[0]];
          GradX g = gview(ctx, E, op.out, input);
          g.da = E.gptr(se.out);
          np = launch_dw_bwd_se(g, E.slot_c[se.slot], E.gptr(se.in[0]), 1.0f / (float)(tb.h * tb.w), W + op.w, dx, ti.n, ti.h, ti.w, ti.c, to.h, to.w, op.k, op.stride, op.pad_t, op.pad_l,
                                op.acc[0], s, gsk);
          break;
        }
        np = launch_dw_bwd(gview(ctx, E, op.out, input), W + op.w, dx, ti.n, ti.h, ti.w, ti.c, to.h, to.w, op.k,
                           op.stride, op.pad_t, op.pad_l, op.acc[0], s, gsk);
        break;
      case OP_BN:
        // reduction only; the apply half runs in the producer's dgrad (gview)
        if (op.acc[0]) throw std::runtime_error("BN input with several consumers");
        if (!frozen && E.gfused_bn[i] && ctx->bn_mode == PHX_BN_SYNC) {
          const BnFinSeg sg{E.spart + E.gstat_region[i] * E.sp_region, nullptr, E.gstat_P[i], (long)ti.rows(),
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, E.slot_d[op.slot], E.slot_e[op.slot]};
          sync_finalize(ctx, E, &sg, 1, ti.c, true, s);
        } else if (!frozen && E.gfused_bn[i] && skip_timing('b')) {  // (timing diagnostics)
        } else if (!frozen && E.gfused_bn[i])
          launch_bn_bwd_finalize(E.spart + E.gstat_region[i] * E.sp_region, E.gstat_P[i], (long)ti.rows(),
                                 ti.c, E.slot_d[op.slot],
                                 E.slot_e[op.slot], s);
        else if (!frozen && ctx->bn_mode == PHX_BN_SYNC) {
          launch_bn_bwd_reduce_sums(dy, E.tptr(op.in[0], input), E.slot_a[op.slot], E.slot_b[op.slot], W + op.gamma,
                                    W + op.beta, (long)ti.rows(), ti.c, op.act, E.red, E.sync_sums, s,
                                    E.tbf(op.in[0]) != 0);
          const BnFinSeg sg{nullptr, nullptr, 0, (long)ti.rows(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            E.slot_d[op.slot], E.slot_e[op.slot]};
          sync_reduce_apply(ctx, E, &sg, 1, ti.c, true, s);
        }
        else if (!frozen)
          launch_bn_bwd_reduce(dy, E.tptr(op.in[0], input), E.slot_a[op.slot], E.slot_b[op.slot],
                               W + op.gamma, W + op.beta, (long)ti.rows(), ti.c, op.act, E.red,
                               E.slot_d[op.slot], E.slot_e[op.slot], s, E.tbf(op.in[0]) != 0);
        (void)dx;
        break;
      case OP_SE:
        if (se_fold) {
          // dpool goes to the head of the slot of the gradient that is no longer stored
          np = launch_se_bwd_sums(dy, view(ctx, E, op.in[0], input), ti.n, ti.h * ti.w, ti.c, op.cse, W + op.w1,
                                  ctx->wt_of(op.w2), op.act, E.slot_b[op.slot], E.slot_c[op.slot], dx, s, E.red, gsk);
          break;
        }
        np = launch_se_bwd(dy, view(ctx, E, op.in[0], input), dx, ti.n, ti.h * ti.w, ti.c, op.cse, W + op.w1,
                           W + op.b1, ctx->wt_of(op.w2), W + op.b2, op.act, E.slot_a[op.slot],
                           E.slot_b[op.slot], E.slot_c[op.slot], E.se_g, op.acc[0], s, E.red, gsk);
        break;
      case OP_ADD: {
        // inputs whose gradient buffer aliases the output's (model.cpp: plan_backward) need no
        // copy, only the BN-backward sums when they are a BN output
        int n0 = 0, n1 = 0;
        if (dx == dy) {
          if (gsk_in == 0) n0 = launch_grad_sums(dy, (long)to.numel(), to.c, gsk, s);
        } else {
          n0 = launch_copy_grad(dy, dx, (long)to.numel(), op.acc[0], s, to.c,
                                gsk_in == 0 ? gsk : GradSink{}, drop_view(E, i));
        }
        if (E.gptr(op.in[1]) == dy) {
          if (gsk_in == 1) n1 = launch_grad_sums(dy, (long)to.numel(), to.c, gsk, s);
        } else {
          n1 = launch_copy_grad(dy, E.gptr(op.in[1]), (long)to.numel(), op.acc[1], s, to.c,
                                gsk_in == 1 ? gsk : GradSink{});
        }
        np = gsk_in == 0 ? n0 : n1;
        break;
      }
      case OP_MAXPOOL:
        launch_maxpool_bwd(E.pool_amax[i], dy, dx, ti.n, ti.h, ti.w, ti.c, to.h, to.w,
                           op.k, op.stride, op.pad_t, op.pad_l, op.acc[0], s);
        break;
      case OP_UPSAMPLE:
        launch_upsample_bwd(dy, dx, ti.n, ti.h, ti.w, ti.c, to.h, to.w, op.acc[0], s);
        break;
      case OP_FUSE: {
        InX xs[3] = {};
        float* dxs[3] = {nullptr, nullptr, nullptr};
        bool acc[3] = {false, false, false};
        for (int k = 0; k < op.nin; ++k) {
          xs[k] = view(ctx, E, op.in[k], input);
          dxs[k] = E.gptr(op.in[k]);
          acc[k] = op.acc[k];
        }
        launch_fuse_bwd(xs, op.nin, op.wsm[0] >= 0 ? W + op.wsm[0] : nullptr,
                        op.wsm[1] >= 0 ? W + op.wsm[1] : nullptr,
                        op.wsm[2] >= 0 ? W + op.wsm[2] : nullptr, op.fuse_method, op.act, dy, dxs,
                        acc, (long)to.numel(), to.c, s);
        break;
      }
    }
    if (gsk.part && np != E.gstat_P[i - 1])
      throw std::logic_error("BN backward sums: planned and launched partial counts differ");
    if (gsk.part) E.gstat_region[i - 1] = 0;
    ck_bwd(E, i, s);
  }
}

// InverseDIOULoss (regression_loss.py:27-68) of the second pass's kept anchors against the gts
void run_box_loss(phx_ctx* ctx, Exec& E, const float* gt, const int* gcount, float* metrics, hipStream_t s) {
  if (!E.prog.box_grad) throw std::logic_error("box loss: the executor was planned without it");
  // algorithmic bytes: every decoded box and keep flag once, the gts, the chunk partials written and read
  Scope scope(ctx, "idiou", 0.0,
              (double)E.B * ctx->A * 17.0 + (double)E.B * kIdiouMaxGt * (16.0 + 24.0 * idiou_chunks(ctx->A)), s);
  launch_idiou(E.boxes, E.keep, gt, gcount, E.B, ctx->A, E.bl_max, E.bl_anchor, E.bl_nties, E.bl_img, E.bl_batch,
               E.bl_scratch, ctx->box_w, metrics, s);
  E.bl_gt = gt;
  E.bl_gcount = gcount;
  E.bl_valid = true;
}

// cand_mask: the keep bits whose anchors (above the NMS threshold) pre_nms appends to the
// soft-NMS candidate list (2: the first pass's person/valid/>=thresh, 1: the second pass's
// person/valid for the ASR metric, 4: person, -1: every anchor (serving, postprocess_global), 0: no
// list); the run_nms that follows consumes it
// nms_t: the NMS score threshold of the candidate list (kNmsCtxThresh: the context's)
void run_pre_nms(phx_ctx* ctx, Exec& E, hipStream_t s, int cand_mask, float nms_t) {
  const Program& P = E.prog;
  Scope scope(ctx, "pre_nms", 0.0,
              (double)E.B * ctx->A * (ctx->mc.num_classes + 4 + 4 + 6) * 4.0, s);
  const float S = (float)ctx->mc.image_size;
  // every list starts empty: a step that failed between a pre_nms and its run_nms (which
  // normally resets the counts) must not leave stale candidates for the next soft-NMS
  if (cand_mask) PHX_HIP(hipMemsetAsync(E.cand_count, 0, (size_t)E.B * sizeof(int), s));
  launch_pre_nms(E.tptr(P.cls_out[0], nullptr), E.tptr(P.box_out[0], nullptr),
                 E.lev_dev, (int)E.lev.size(), reinterpret_cast<const float*>(ctx->d_anchors.get()),
                 ctx->A, E.B, ctx->mc.num_classes, ctx->mc.num_anchors(), S, S, ctx->filter_thresh,
                 E.scores, E.classes, E.boxes, E.keep, E.ntiles, s,
                 cand_mask ? NmsCand{E.cand_list, E.cand_count, cand_mask, std::isnan(nms_t) ? ctx->nms_thresh : nms_t}
                           : NmsCand{},
                 E.tbf(P.cls_out[0]) != 0);
}

// postprocess.nms under the context's nms_configs (phx_set_nms_config).  gaussian (sigma 0.5 -> soft_nms_sigma
// 0.25 by default): k_soft_nms, run to 100 selections and cut to max_output_size; hard: the segmented kernel, one
// segment per image
void run_nms(phx_ctx* ctx, Exec& E, int keep_mask, float* ob, float* os, int* oc, hipStream_t s,
             float nms_t, int* sel) {
  Scope scope(ctx, "soft_nms", 0.0, (double)E.B * ctx->A * 5.0, s);
  const float t = std::isnan(nms_t) ? ctx->nms_thresh : nms_t;
  const NmsSegParams q = ctx->nms_params(t);
  if (!ctx->nms_hard()) {
    launch_soft_nms(E.boxes, E.scores, E.keep, keep_mask, nullptr, E.B, ctx->A, t,
                    q.soft_sigma, PHX_MAX_OUT, (float)ctx->mc.image_size, ob, os, oc, E.nms_ws, s,
                    NmsCand{E.cand_list, E.cand_count, keep_mask, t}, sel);
    launch_nms_truncate(ob, os, oc, sel, E.B, q.max_out, s);
    return;
  }
  seg_scratch(ctx, E);
  launch_nms_seg_global(E.boxes, E.scores, E.keep, keep_mask, nullptr, E.B, ctx->A, q, (float)ctx->mc.image_size, ob,
                        os, oc, E.seg_ws, s, NmsCand{E.cand_list, E.cand_count, keep_mask, t}, sel);
}

// the executor's scratch of the segmented NMS (one segment per image, or one per class), reserved at its first use
float* seg_scratch(phx_ctx* ctx, Exec& E) {
  if (!E.seg_ws) E.seg_ws = E.alloc<float>(nms_seg_work_floats(E.B, ctx->A, std::max(1, ctx->mc.num_classes)));
  return E.seg_ws;
}

// postprocess.nms(padded=True) + clip_boxes over caller-provided candidates (phx_soft_nms, phx_nms_global) under
// the context's nms_configs; the context's scratch grows on demand (synchronising s)
void run_nms_candidates(phx_ctx* ctx, const float* boxes, const float* scores, const int* count, int B, int N,
                        float* ob, float* os, int* oc, int* sel, hipStream_t s) {
  const NmsSegParams q = ctx->nms_params(ctx->nms_thresh);
  if (!ctx->nms_hard()) {
    const size_t need = soft_nms_work_floats(B, N);
    if (need > ctx->sn_cap) {
      PHX_HIP(hipStreamSynchronize(s));
      ctx->sn_ws.reset(dalloc<float>(need));
      ctx->sn_cap = need;
    }
    launch_soft_nms(boxes, scores, nullptr, 0, count, B, N, q.score_thresh, q.soft_sigma, PHX_MAX_OUT,
                    (float)ctx->mc.image_size, ob, os, oc, (float*)ctx->sn_ws.get(), s, NmsCand{}, sel);
    launch_nms_truncate(ob, os, oc, sel, B, q.max_out, s);
    return;
  }
  launch_nms_seg_global(boxes, scores, nullptr, 0, count, B, N, q, (float)ctx->mc.image_size, ob, os, oc,
                        seg_scratch(ctx, B, N, 1, s), s, NmsCand{}, sel);
}

float* seg_scratch(phx_ctx* ctx, int B, int N, int C, hipStream_t s) {
  if (!nms_seg_accepts(N)) throw std::runtime_error("nms: too many candidates");
  const size_t need = nms_seg_work_floats(B, N, C);
  if (need > ctx->seg_cap) {
    PHX_HIP(hipStreamSynchronize(s));
    ctx->seg_ws.reset(dalloc<float>(need));
    ctx->seg_cap = need;
  }
  return static_cast<float*>(ctx->seg_ws.get());
}

// PHX_GUARD_BYTES: after a step, every executor allocation's guard band must still be 0xA5
void check_guards(phx_ctx* ctx, hipStream_t s) {
  PHX_HIP(hipStreamSynchronize(s));
  if (ctx->s1) PHX_HIP(hipStreamSynchronize(ctx->s1));
  const size_t gb = guard_bytes();
  std::vector<unsigned char> h(gb);
  for (auto& ep : ctx->execs) {
    for (size_t i = 0; i < ep->guards.size(); ++i) {
      const Guard& g = ep->guards[i];
      for (int side = 0; side < 2; ++side) {
        const char* band = side ? g.base + g.size : g.base - gb;
        PHX_HIP(hipMemcpy(h.data(), band, gb, hipMemcpyDeviceToHost));
        size_t first = gb, last = 0;
        for (size_t k = 0; k < gb; ++k)
          if (h[k] != 0xA5) {
            first = std::min(first, k);
            last = k;
          }
        if (first < gb) {
          if (side)
            fprintf(stderr, "phx guard: exec B=%d tag=%d allocation %zu (%zu bytes) overwritten at +%zu..+%zu past its end\n",
                    ep->B, ep->tag, i, g.size, first, last);
          else
            fprintf(stderr, "phx guard: exec B=%d tag=%d allocation %zu (%zu bytes) overwritten at -%zu..-%zu before its start\n",
                    ep->B, ep->tag, i, g.size, gb - last, gb - first);
          PHX_HIP(hipMemset(const_cast<char*>(band), 0xA5, gb));
        }
      }
    }
  }
}

}  // namespace phx

phx::ExtTiming*& phx::ext_timing() {
  static ExtTiming* t = nullptr;
  return t;
}

phx::ProfScope phx::prof_begin(phx_ctx* ctx, const char* kind, double flops, double bytes, hipStream_t s) {
  ProfScope r{nullptr, 0, s};
  if (!ctx || !ctx->prof.on) return r;
  Prof* p = &ctx->prof;
  Prof::Rec rec{kind, p->ev(), p->ev(), flops, bytes, 157.3};
  PHX_HIP(hipEventRecord(rec.a, s));
  p->recs.push_back(rec);
  r.p = p;
  r.idx = p->recs.size() - 1;
  return r;
}

void phx::prof_end(const ProfScope& r) {
  if (r.p) PHX_HIP(hipEventRecord(static_cast<Prof*>(r.p)->recs[r.idx].b, r.s));
}
