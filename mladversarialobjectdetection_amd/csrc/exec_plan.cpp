// exec_plan.cpp — the executor's planner (exec_plan.hpp).  The decisions run in a fixed order, each
// reading the earlier ones: fused statistics, gradient sinks, groups, fold, sep, sepb, sefold.
#include "exec_plan.hpp"

#include <algorithm>
#include <map>
#include <stdexcept>

#include "env.hpp"
#include "phx.h"

namespace phx {

bool is_cls_out(const Program& P, int t) {
  return std::find(P.cls_out.begin(), P.cls_out.end(), t) != P.cls_out.end();
}

bool is_scatter_out(const Program& P, int t) {
  if (is_cls_out(P, t)) return true;
  return P.box_grad && std::find(P.box_out.begin(), P.box_out.end(), t) != P.box_out.end();
}

namespace {

// ---- level-batched heads -----------------------------------------------------------------
bool grouping_enabled() {
  static const bool on = env_on("PHX_GROUP");
  return on;
}

// Members of a candidate group must be interchangeable launches: same op kind and geometry, same
// statistics / gradient-sink wiring, no SE row scale; grouped GEMMs must not need split-K.
bool group_uniform(const ExecPlan& E, const std::vector<int>& v) {
  const Program& P = E.prog;
  const Op& a = P.ops[v[0]];
  const int n = (int)P.ops.size();
  auto fused_next = [&](int i) { return i + 1 < n && E.fused_bn[i + 1]; };
  auto gfused_prev = [&](int i) { return i > 0 && E.gfused_bn[i - 1]; };
  auto has_gx = [&](int i) {
    const int bi = E.bn_consumer[P.ops[i].out];
    return bi >= 0 && P.ops[bi].bwd;
  };
  std::vector<int> M;
  for (int i : v) {
    const Op& b = P.ops[i];
    const Tensor& ti = P.tensors[b.in[0]];
    const Tensor& to = P.tensors[b.out];
    const Tensor& ta = P.tensors[a.in[0]];
    const Tensor& tb = P.tensors[a.out];
    if (b.t != a.t || b.k != a.k || b.stride != a.stride || b.nin != 1 || ti.c != ta.c || to.c != tb.c ||
        ti.n != ta.n)
      return false;
    if (b.bwd != a.bwd || b.acc[0] != a.acc[0] || fused_next(i) != fused_next(v[0]) ||
        gfused_prev(i) != gfused_prev(v[0]) || has_gx(i) != has_gx(v[0]))
      return false;
    if ((E.bn_of_tensor[b.in[0]] >= 0) != (E.bn_of_tensor[a.in[0]] >= 0)) return false;
    if (E.se_of_tensor[b.in[0]] >= 0 || b.in[0] == P.input) return false;
    if (gfused_prev(i) && P.ops[i - 1].out != b.in[0]) return false;
    M.push_back((int)ti.rows());
  }
  if (a.t == OP_PW) {
    const Tensor& ta = P.tensors[a.in[0]];
    const Tensor& tb = P.tensors[a.out];
    if (!gemm_group_ok(M.data(), (int)M.size(), tb.c, ta.c, E.bf16)) return false;  // forward
    if (a.bwd && !gemm_group_ok(M.data(), (int)M.size(), ta.c, tb.c, E.bf16)) return false;  // dgrad
  }
  return true;
}

// Groups: convs sharing a weight tensor (the per-level copies of a head conv) and the BNs right
// after them.  The schedule is then checked; any violation disables grouping for this executor.
void plan_groups(ExecPlan& E, bool local_bn) {
  const Program& P = E.prog;
  const int n = (int)P.ops.size();
  E.grp_of.assign(n, -1);
  E.groups.clear();
  if (!grouping_enabled() || !local_bn) return;
  std::map<long, std::vector<int>> byw;
  for (int i = 0; i < n; ++i)
    if ((P.ops[i].t == OP_DW || P.ops[i].t == OP_PW) && P.ops[i].w >= 0) byw[P.ops[i].w].push_back(i);
  for (auto& kv : byw) {
    const std::vector<int>& v = kv.second;
    if (v.size() < 2 || v.size() > (size_t)kMaxSeg || !group_uniform(E, v)) continue;
    const int g = (int)E.groups.size();
    E.groups.push_back(v);
    for (int i : v) E.grp_of[i] = g;
    std::vector<int> bn;
    for (int i : v)
      if (i + 1 < n && P.ops[i + 1].t == OP_BN && P.ops[i + 1].in[0] == P.ops[i].out && E.fused_bn[i + 1] &&
          !P.ops[i + 1].acc[0])
        bn.push_back(i + 1);
    if (bn.size() != v.size()) continue;
    bool ok = true;
    for (int b : bn)
      ok = ok && P.ops[b].bwd == P.ops[bn[0]].bwd && E.gfused_bn[b] == E.gfused_bn[bn[0]] &&
           P.ops[b].act == P.ops[bn[0]].act;
    if (!ok || (P.ops[bn[0]].bwd && !E.gfused_bn[bn[0]])) continue;
    const int gb = (int)E.groups.size();
    E.groups.push_back(bn);
    for (int b : bn) E.grp_of[b] = gb;
  }
  if (E.groups.empty()) return;
  // schedule checks: forward position = first member, reverse position = last member
  auto fpos = [&](int i) { return E.grp_of[i] >= 0 ? E.groups[E.grp_of[i]].front() : i; };
  auto bpos = [&](int i) { return E.grp_of[i] >= 0 ? E.groups[E.grp_of[i]].back() : i; };
  std::vector<int> producer(P.tensors.size(), -1);
  for (int i = 0; i < n; ++i) producer[P.ops[i].out] = i;
  bool ok = true;
  for (int i = 0; i < n && ok; ++i) {
    const Op& op = P.ops[i];
    for (int j = 0; j < op.nin; ++j) {
      const int p = producer[op.in[j]];
      if (p >= 0 && (fpos(p) >= fpos(i) || (E.grp_of[i] >= 0 && E.grp_of[p] == E.grp_of[i]))) ok = false;
    }
    // statistics partials: producer launch immediately before its BN's finalize
    if (op.t == OP_BN && E.fused_bn[i] && fpos(i) != fpos(i - 1) + 1) ok = false;
    if (op.t == OP_BN && E.gfused_bn[i] && op.bwd && bpos(i + 1) != bpos(i) + 1) ok = false;
  }
  // reverse sweep: every consumer's backward before its producer's; writers of one gradient keep
  // their program order and never share a launch
  for (int i = 0; i < n && ok; ++i) {
    if (!P.ops[i].bwd) continue;
    for (int c = i + 1; c < n && ok; ++c) {
      const Op& oc = P.ops[c];
      if (!oc.bwd || (oc.t == OP_PW && is_scatter_out(P, oc.out))) continue;
      for (int j = 0; j < oc.nin; ++j) {
        if (oc.in[j] == P.ops[i].out && bpos(c) <= bpos(i)) ok = false;
        for (int k = 0; k < P.ops[i].nin; ++k)
          if (oc.in[j] == P.ops[i].in[k] && (bpos(c) <= bpos(i))) ok = false;
      }
    }
  }
  if (!ok) {
    E.grp_of.assign(n, -1);
    E.groups.clear();
  }
}

// what k_sep_fwd / k_sep_bwd and the folded fuse's depthwise kernel assume of a depthwise op beyond
// k = 3, stride 1: SAME padding (one row on top, one column on the left, output as large as the
// input) and depth multiplier 1
bool dw_same_3x3(const Program& P, const Op& d) {
  const Tensor& ti = P.tensors[d.in[0]];
  const Tensor& to = P.tensors[d.out];
  return d.k == 3 && d.stride == 1 && d.pad_t == 1 && d.pad_l == 1 && to.h == ti.h && to.w == ti.w && to.c == ti.c;
}

}  // namespace

// the serving executor (tag 2) is planned as a bn=frozen context plans: inference BN only
static bool batch_bn(int tag, int bn_mode) { return tag == 2 ? false : bn_mode != PHX_BN_FROZEN; }

ExecPlan plan_exec(const ModelConfig& mc, int B, int tag, int bn_mode, bool bf16, int num_anchors, bool box_grad) {
  NetBuilder nb(mc, B, batch_bn(tag, bn_mode));
  nb.set_box_grad(box_grad);
  nb.build();
  return plan_program(nb.program(), B, tag, bn_mode, bf16, mc.image_size, mc.num_anchors(), num_anchors);
}

ExecPlan plan_program(const Program& prog, int B, int tag, int bn_mode, bool bf16, int image_size, int na,
                      int num_anchors) {
  ExecPlan E;
  E.B = B;
  E.tag = tag;
  E.bf16 = bf16;
  E.abf = bf16;
  const bool bbn = batch_bn(tag, bn_mode);
  E.infer_plan = !bbn;
  E.prog = prog;
  const Program& P = E.prog;
  // tensor -> op maps; statistics scratch
  E.se_of_tensor.assign(P.tensors.size(), -1);
  E.bn_of_tensor.assign(P.tensors.size(), -1);
  E.bn_consumer.assign(P.tensors.size(), -1);
  for (size_t i = 0; i < P.ops.size(); ++i) {
    const Op& op = P.ops[i];
    const Tensor& ti = P.tensors[op.in[0]];
    if (op.t == OP_BN) {
      E.bn_of_tensor[op.out] = (int)i;
      E.bn_consumer[op.in[0]] = (int)i;
      E.red_need = std::max(E.red_need, bn_stats_scratch_doubles((long)ti.rows(), ti.c));
      E.coef_need = std::max(E.coef_need, (size_t)ti.c * 3);
    } else if (op.t == OP_SE) {
      E.seg_need = std::max(E.seg_need, (size_t)B * ti.c * 2);
      E.red_need = std::max(E.red_need, colred_scratch_doubles((long)ti.h * ti.w, ti.c, B));
      E.se_of_tensor[op.out] = (int)i;
    }
  }
  // moving statistics: one table entry per BN, its deferred (batch mean, variance) at side_off
  {
    int off = 0;
    E.side_off.assign(P.n_slots, 0);
    for (const Op& op : P.ops)
      if (op.t == OP_BN) {
        const int C = P.tensors[op.in[0]].c;
        E.side_off[op.slot] = off;
        E.mov.push_back(MovEntry{op.mmean, op.mvar, C, off});
        off += C;
        E.mov_cmax = std::max(E.mov_cmax, C);
      }
    E.side_need = 2 * (size_t)std::max(off, 1);
    E.n_mov = (int)E.mov.size();
  }
  // fused statistics: a BN whose input is produced by the op right before it (stem, 1x1 conv,
  // depthwise conv) gets its batch statistics from that producer's epilogue
  E.fused_bn.assign(P.ops.size(), 0);
  size_t sp_need = 1, sc_need = 1;
  if (bbn) {
    for (size_t i = 1; i < P.ops.size(); ++i) {
      const Op& op = P.ops[i];
      const Op& pr = P.ops[i - 1];
      if (op.t != OP_BN || pr.out != op.in[0]) continue;
      const Tensor& ti = P.tensors[pr.in[0]];
      const Tensor& to = P.tensors[pr.out];
      int np = 0;
      if (pr.t == OP_STEM) np = cdiv((long)to.rows(), 256);
      else if (pr.t == OP_PW && to.c % 4 == 0) np = gemm_stat_partials((int)ti.rows(), to.c, ti.c, bf16);
      else if (pr.t == OP_DW) np = dw_stat_partials(ti.n, ti.h, ti.w, ti.c, to.h, to.w, pr.k, pr.stride, pr.pad_t, pr.pad_l);
      if (np <= 0) continue;
      E.fused_bn[i] = 1;
      sp_need = std::max(sp_need, (size_t)np * to.c);
      sc_need = std::max(sc_need, (size_t)np);
    }
  }
  E.gfused_bn.assign(P.ops.size(), 0);
  E.gstat_P.assign(P.ops.size(), 0);
  if (bbn) {
    for (size_t i = 0; i + 1 < P.ops.size(); ++i) {
      const Op& bn = P.ops[i];
      const Op& L = P.ops[i + 1];
      if (bn.t != OP_BN || !bn.bwd || !L.bwd) continue;
      const Tensor& tz = P.tensors[bn.out];
      int np = 0;
      const Tensor& li = P.tensors[L.in[0]];
      const Tensor& lo = P.tensors[L.out];
      if (L.t == OP_DW && L.in[0] == bn.out)
        np = dw_bwd_partials(li.n, li.h, li.w, li.c, lo.h, lo.w, L.k, L.stride, L.pad_t, L.pad_l);
      else if (L.t == OP_SE && L.in[0] == bn.out)
        np = ew_gstats_partials((long)li.h * li.w, li.c, li.n);
      else if (L.t == OP_PW && L.in[0] == bn.out && !is_scatter_out(P, L.out))
        np = gemm_dgrad_gsink_partials((int)li.rows(), li.c, lo.c, bf16);
      else if (L.t == OP_ADD && (L.in[0] == bn.out || L.in[1] == bn.out) && L.in[0] != L.in[1])
        np = ew_gstats_partials((long)tz.rows(), tz.c, 1);
      if (np <= 0 || tz.c % 4) continue;
      E.gfused_bn[i] = 1;
      E.gstat_P[i] = np;
      sp_need = std::max(sp_need, (size_t)np * tz.c);
    }
  }
  plan_groups(E, bbn);
  if (bn_mode == PHX_BN_SYNC && tag != 2) {
    int cmax = 1;
    for (const Tensor& t : P.tensors) cmax = std::max(cmax, t.c);
    E.sync_need = (size_t)kMaxSeg * cmax * 3;
  }
  std::vector<int> nuse(P.tensors.size(), 0);  // readers of each tensor
  for (const Op& op : P.ops)
    for (int j = 0; j < op.nin; ++j) ++nuse[op.in[j]];
  E.fuse_folded.assign(P.ops.size(), 0);
  {
    static const bool fold = env_on("PHX_FOLD");
    for (size_t i = 0; fold && i + 1 < P.ops.size(); ++i) {
      const Op& f = P.ops[i];
      const Op& d = P.ops[i + 1];
      if (f.t != OP_FUSE || d.t != OP_DW || d.in[0] != f.out || nuse[f.out] != 1) continue;
      if (!dw_same_3x3(P, d) || E.grp_of[i + 1] >= 0 || P.tensors[f.out].c % 4) continue;
      if (i + 2 < P.ops.size() && E.fused_bn[i + 2]) continue;
      E.fuse_folded[i] = 1;
    }
  }
  // fused separable convs: a 3x3 stride-1 SAME depthwise op whose output feeds only the next op's
  // pointwise conv (keras SeparableConv2D of the BiFPN nodes and both heads, model.cpp sepconv), fp32,
  // both ungrouped or grouped member for member (the heads' per-level copies).  PHX_SEP=0 keeps the
  // two launches (A/B; read per executor).
  E.sep.assign(P.ops.size(), 0);
  {
    const bool on = env_on("PHX_SEP");
    const long sep_min_rows = env_long("PHX_SEP_MINROWS", 32768);
    for (size_t i = 0; on && i + 1 < P.ops.size(); ++i) {
      const Op& d = P.ops[i];
      const Op& pw = P.ops[i + 1];
      if (d.t != OP_DW || pw.t != OP_PW || pw.in[0] != d.out || pw.nin != 1 || nuse[d.out] != 1) continue;
      if (!dw_same_3x3(P, d) || d.in[0] == P.input) continue;
      const Tensor& ti = P.tensors[d.in[0]];
      const Tensor& to = P.tensors[pw.out];
      if (!sep_supported(ti.c, to.c, E.bf16 || E.abf) || E.se_of_tensor[d.out] >= 0) continue;
      // the fused launch is a latency chain per 8 x 16 tile (window, depthwise, MFMAs, stores): it wins
      // where there are enough tiles to fill the chip (the P3 level; a head group, whose P3 member
      // dominates) and loses to the two launches on the small levels (tools/sep_probe: 4 x 4 to
      // 32 x 32 levels of 16 images 1-5 us slower fused)
      if ((long)ti.rows() < sep_min_rows) continue;
      const int gd = E.grp_of[i], gp = E.grp_of[i + 1];
      if ((gd >= 0) != (gp >= 0)) continue;
      if (gd >= 0) {
        // the pointwise members: the depthwise group's, member for member
        const std::vector<int>& a = E.groups[gd];
        bool ok = a[0] == (int)i && E.groups[gp].size() == a.size();
        for (size_t r = 0; ok && r < a.size(); ++r) {
          const Op& pr = P.ops[a[r] + 1];
          ok = pr.t == OP_PW && pr.in[0] == P.ops[a[r]].out && pr.w == pw.w && pr.b == pw.b &&
               E.grp_of[a[r] + 1] == gp && E.groups[gp][r] == a[r] + 1;
        }
        if (!ok) continue;
      }
      if (i > 0 && E.fuse_folded[i - 1] && gd >= 0) continue;  // (a fuse view is never grouped)
      const std::vector<int> mem = gd >= 0 ? E.groups[gd] : std::vector<int>{(int)i};
      for (int di : mem) {
        E.sep[di] = 1;
        const Tensor& tm = P.tensors[P.ops[di].in[0]];
        if (di + 2 < (int)P.ops.size() && E.fused_bn[di + 2] && P.ops[di + 2].in[0] == P.ops[di + 1].out) {
          const int np = sep_stat_partials(tm.n, tm.h, tm.w);
          sp_need = std::max(sp_need, (size_t)np * to.c);
          sc_need = std::max(sc_need, (size_t)np);
        }
      }
    }
  }
  // the fused sepconvs' backward: pointwise dgrad through the consumer BN's gradient view and the
  // depthwise transpose in one launch (not the class-predict conv: its input gradient is the sparse
  // scatter's).  PHX_SEPB=0 keeps the two launches.
  E.sepb.assign(P.ops.size(), 0);
  {
    const bool on = env_on("PHX_SEPB") && bbn;
    for (size_t i = 0; on && i + 1 < P.ops.size(); ++i) {
      if (!E.sep[i]) continue;
      const int gd = E.grp_of[i];
      if (gd >= 0 && E.groups[gd][0] != (int)i) continue;  // (decided per group, at its first member)
      const std::vector<int> mem = gd >= 0 ? E.groups[gd] : std::vector<int>{(int)i};
      bool ok = true;
      for (int di : mem) {
        const Op& d = P.ops[di];
        const Op& pw = P.ops[di + 1];
        const int bi = E.bn_consumer[pw.out];
        ok = ok && d.bwd && pw.bwd && !is_scatter_out(P, pw.out) && bi >= 0 && P.ops[bi].bwd &&
             sep_bwd_supported(P.tensors[d.in[0]].c, P.tensors[pw.out].c, E.bf16 || E.abf);
        ok = ok && (di > 0 && E.gfused_bn[di - 1]) == (mem[0] > 0 && E.gfused_bn[mem[0] - 1]);
      }
      if (!ok) continue;
      for (int di : mem) {
        E.sepb[di] = 1;
        if (di > 0 && E.gfused_bn[di - 1]) {
          const Tensor& tm = P.tensors[P.ops[di].in[0]];
          const int np = sep_stat_partials(tm.n, tm.h, tm.w);
          E.gstat_P[di - 1] = np;
          sp_need = std::max(sp_need, (size_t)np * tm.c);
        }
      }
    }
  }
  // SE backward without the dx tensor: an SE over a batch-statistics BN (bn=local) whose backward sums it
  // produces (gfused_bn), fed by an ungrouped depthwise conv that runs its own backward launch, with the SE
  // the only writer of the BN output's gradient: that gradient is formed on load by the depthwise dgrad and
  // its slot keeps the SE's dpool.  PHX_SEFOLD=0 keeps the apply pass's store (A/B; read per executor).
  // No other plan field depends on the flag, and every result keeps its bits.
  E.sefold.assign(P.ops.size(), 0);
  {
    const bool on = env_on("PHX_SEFOLD") && bbn && bn_mode == PHX_BN_LOCAL;
    for (size_t i = 2; on && i < P.ops.size(); ++i) {
      const Op& se = P.ops[i];
      const Op& bn = P.ops[i - 1];
      const Op& dw = P.ops[i - 2];
      if (se.t != OP_SE || !se.bwd || se.acc[0]) continue;
      if (bn.t != OP_BN || !bn.bwd || bn.out != se.in[0] || !E.gfused_bn[i - 1] || E.grp_of[i - 1] >= 0) continue;
      if (dw.t != OP_DW || !dw.bwd || dw.out != bn.in[0] || E.grp_of[i - 2] >= 0 || E.sepb[i - 2]) continue;
      if (P.tensors[se.in[0]].c % 4 || P.tensors[se.in[0]].goff < 0) continue;
      E.sefold[i] = 1;
    }
  }
  E.nreg = E.groups.empty() ? 1 : kMaxSeg;
  E.sp_region = sp_need;
  E.sc_region = sc_need;
  for (const Op& op : P.ops) {
    if (op.t != OP_PW) continue;
    const Tensor& ti = P.tensors[op.in[0]];
    const Tensor& to = P.tensors[op.out];
    E.gp_need = std::max(E.gp_need, gemm_partial_floats((int)ti.rows(), to.c, ti.c, bf16));  // forward
    E.gp_need = std::max(E.gp_need, gemm_partial_floats((int)ti.rows(), ti.c, to.c, bf16));  // dgrad
  }
  // level tables (class / box outputs)
  const int nlev = (int)P.cls_out.size();
  int a0 = 0;
  for (int l = 0; l < nlev; ++l) {
    const Tensor& tc = P.tensors[P.cls_out[l]];
    const Tensor& tb = P.tensors[P.box_out[l]];
    LevelDesc d;
    d.cls_off = (long)tc.off - (long)P.tensors[P.cls_out[0]].off;
    d.box_off = (long)tb.off - (long)P.tensors[P.box_out[0]].off;
    d.h = tc.h;
    d.w = tc.w;
    d.anchor0 = a0;
    d.tile0 = E.ntiles;
    E.ntiles += pre_nms_tiles(tc.h, tc.w, na);
    a0 += tc.h * tc.w * na;
    E.lev.push_back(d);
    // input of the class-predict pointwise conv
    for (const Op& op : P.ops)
      if (op.out == P.cls_out[l]) E.dxoff.push_back(P.tensors[op.in[0]].goff);
    // ... and of the box-predict pointwise conv, where the box head runs backward
    if (P.box_grad)
      for (const Op& op : P.ops)
        if (op.out == P.box_out[l]) E.dxoff_box.push_back(P.tensors[op.in[0]].goff);
  }
  if (a0 != num_anchors) throw std::runtime_error("anchor count mismatch");
  // EOT
  const int S = image_size;
  E.ed.B = B;
  E.ed.H = S;
  E.ed.W = S;
  E.ed.maxb = PHX_MAX_OUT;
  E.ed.P = PHX_PATCH_SIZE;
  E.ed.span_stride = S;
  // worst case: every slot holds a full-image patch
  E.ed.rcap = (long)B * PHX_MAX_OUT * S * S * 3;
  // drop connect
  E.drop_slot.assign(P.ops.size(), -1);
  for (size_t i = 0; i < P.ops.size(); ++i)
    if (P.ops[i].t == OP_ADD && P.ops[i].survival > 0.f) {
      E.drop_slot[i] = (int)E.drop_blocks.size();
      E.drop_blocks.push_back(P.ops[i].drop_block);
      E.drop_surv.push_back(P.ops[i].survival);
    }
  E.ndrop = (int)E.drop_blocks.size();
  return E;
}

}  // namespace phx
