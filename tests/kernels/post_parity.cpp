// post_parity — kernel-level parity of the post-processing and attack-loss kernels (kernels_post.hip, and k_adam
// of kernels_eot.hip) against an exact or fp64 host reference, stage by stage: pre_nms with its validity filter
// and candidate lists, soft-NMS, count_ge, the per-image max, the loss, zero_segs, the sparse class-head backward
// and Adam.
//
//   post_parity --plan   the case table with each case's geometry and coverage by the reference alone (tiles per
//                        staging branch, planted argmax ties and validity edges, candidate counts, soft-NMS pops,
//                        ties, margins, nms_plan's numbers, tie chunks of the per-image max), the share of anchors
//                        under the decision allowance, and the CPU stand-in's verdict (no GPU is touched)
//   post_parity          run the table on the GPU: one flushed JSON line per case, then a `done` line
//
// Only the launchers of kernels.hpp and post.hpp are called, on one stream.  A chain case runs pre_nms, soft-NMS
// (list path), count_ge, image_max, loss, zero_segs and cls_scatter in that order, every stage on what the device
// wrote in the stages before, read back.  Soft-NMS also runs with out_index null, with PHX_NMS_FAST=0 (read per
// call) and, on the list path, over a shuffled list: bit-equal.  The exit status is 0 when every case ran (the
// verdicts are in the lines); a HIP error ends the process at once with a `fatal` line and status 3.
// Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "post.hpp"
#include "post_check.hpp"
#include "parity_dev.hpp"

using namespace pck;
using namespace phx;

static_assert(sizeof(Lev) == sizeof(LevelDesc) && offsetof(Lev, tile0) == offsetof(LevelDesc, tile0) &&
              offsetof(Lev, h) == offsetof(LevelDesc, h) && offsetof(Lev, box_off) == offsetof(LevelDesc, box_off),
              "post_check.hpp's Lev is LevelDesc");
static_assert(kMaxOutDev == PHX_MAX_OUT_DEV && kNPatch == PHX_NPATCH_DEV && kNMetric == PHX_NMETRIC, "post.hpp's constants");
static_assert(M_LOSS == PHX_M_LOSS && M_SCALE_LOSS == PHX_M_SCALE_LOSS && M_SUM_M == PHX_M_SUM_M && M_SUM_M2 == PHX_M_SUM_M2 &&
              M_NIMG == PHX_M_NIMG, "phx.h's metric slots");

// ---- the case table ----------------------------------------------------------------------------
static std::vector<Case> table() {
  std::vector<Case> t;
  auto pc = [&](const char* name, int kind, std::function<void(Case&)> more) {
    Case c;
    c.name = name; c.kind = kind; c.seed = 300 + (uint32_t)t.size();
    more(c);
    t.push_back(c);
  };
  // a. the chain on the 846-anchor pyramid (na 9): fp32 and bf16 storage of the same logits (same seed), every
  // nclass and na path, every cand.mask and no list, both list thresholds, K around the 64-column rounds
  pc("chain_f32_b3_c90", K_CHAIN, [](Case& c) { c.seed = 7; c.B = 3; c.K = 64; c.nseg = 8; });
  pc("chain_bf16_b3_c90", K_CHAIN, [](Case& c) { c.seed = 7; c.B = 3; c.bf = 1; c.cand_mask = 1; c.cand_thresh = 0.5f; c.K = 160; c.max_out = 7; });
  pc("chain_c1_b1_all_candidates", K_CHAIN, [](Case& c) { c.B = 1; c.nclass = 1; c.cand_mask = -1; c.K = 1; });
  pc("chain_c2_b2_mask4", K_CHAIN, [](Case& c) { c.nclass = 2; c.cand_mask = 4; c.K = 63; c.max_out = 1; });
  pc("chain_c3_b2_bf16", K_CHAIN, [](Case& c) { c.nclass = 3; c.bf = 1; c.K = 65; });
  pc("chain_c91_b2_no_list", K_CHAIN, [](Case& c) { c.nclass = 91; c.cand_list = 0; c.K = 64; });
  pc("chain_c100_b2_general_classes", K_CHAIN, [](Case& c) { c.nclass = 100; c.K = 65; });
  pc("chain_c100_b2_bf16", K_CHAIN, [](Case& c) { c.nclass = 100; c.bf = 1; c.cand_mask = -1; c.cand_thresh = 0.5f; c.K = 63; });
  pc("chain_na1_b2", K_CHAIN, [](Case& c) { c.na = 1; c.K = 64; });
  pc("chain_na17_b2_general_anchors", K_CHAIN, [](Case& c) { c.na = 17; c.K = 64; c.max_out = 7; });
  // b. soft-NMS driven directly: keep mask without a list and count null; a count prefix clamped to N and 0;
  // N no multiple of 64; max_out 1, 7, 100; ties, duplicates and a candidate over 30 selections; chunk factor 2
  pc("nms_mask_n1", K_NMS, [](Case& c) { c.B = 1; c.N = 1; });
  pc("nms_mask_n77_b2_mo7", K_NMS, [](Case& c) { c.B = 2; c.N = 77; c.max_out = 7; });
  pc("nms_prefix_n1000_b3_clamped", K_NMS, [](Case& c) { c.B = 3; c.N = 1000; c.nms_mode = NM_PREFIX; c.counts = {1500, 0, 600}; });
  pc("nms_mask_n77_b1_mo1", K_NMS, [](Case& c) { c.B = 1; c.N = 77; c.max_out = 1; });
  pc("nms_mask_n4096_b2_ties_dups", K_NMS, [](Case& c) { c.seed = 320; c.B = 2; c.N = 4096; c.plant = 1; });
  pc("nms_m2_n262208", K_NMS, [](Case& c) { c.B = 1; c.N = 262208; c.nms_mode = NM_M2; });
  // c. the per-image max (and the loss on its output): fewer anchors than chunks, one per chunk, the pyramid's
  // count, a lane stride with the merge kernel's second workgroup
  pc("imax_a47_b1", K_IMAX, [](Case& c) { c.B = 1; c.N = 47; });
  pc("imax_a48_b3", K_IMAX, [](Case& c) { c.B = 3; c.N = 48; });
  pc("imax_a846_b4", K_IMAX, [](Case& c) { c.B = 4; c.N = 846; });
  pc("imax_a12301_b65", K_IMAX, [](Case& c) { c.B = 65; c.N = 12301; });
  // d. loss: raw maxima > 0, 0, -0.0, < 0, -FLT_MAX
  pc("loss_raw_edges", K_LOSS, [](Case& c) { c.scale = 0.3f; });
  pc("loss_raw_edges_scale1", K_LOSS, [](Case& c) { c.scale = 1.0f; });
  // e. zero_segs and count_ge
  pc("zero_1_seg", K_ZERO, [](Case& c) { c.nseg = 1; });
  pc("zero_8_segs", K_ZERO, [](Case& c) { c.nseg = 8; });
  pc("count_ge_mo100", K_COUNT, [](Case& c) { c.max_out = 100; });
  pc("count_ge_mo7", K_COUNT, [](Case& c) { c.max_out = 7; });
  // f. Adam
  pc("adam_n1_t1", K_ADAM, [](Case& c) { c.n = 1; c.t = 1; });
  pc("adam_n257_t2", K_ADAM, [](Case& c) { c.n = 257; c.t = 2; });
  pc("adam_n1000_t1000", K_ADAM, [](Case& c) { c.n = 1000; c.t = 1000; });
  pc("adam_clip_npatch_plus_1", K_ADAM, [](Case& c) { c.n = kNPatch + 1; c.t = 1; c.clip = 1; });
  // g. refusals: nothing is launched, every output keeps its fill
  pc("refuse_nms_max_out_101", K_REFUSE, [](Case& c) { c.refuse = R_NMS_MAXOUT101; c.B = 2; c.N = 77; c.max_out = 101; });
  pc("refuse_zero_9_segs", K_REFUSE, [](Case& c) { c.refuse = R_ZERO_9; c.nseg = 9; });
  pc("refuse_zero_misaligned", K_REFUSE, [](Case& c) { c.refuse = R_ZERO_MISALIGNED; c.nseg = 2; });
  pc("refuse_scatter_na33", K_REFUSE, [](Case& c) { c.refuse = R_SCATTER_NA33; c.na = 33; c.nclass = 3; c.K = 8; });
  pc("refuse_scatter_a_mod_na", K_REFUSE, [](Case& c) { c.refuse = R_SCATTER_AMODNA; c.nclass = 3; c.K = 8; });
  return t;
}
// ---- end of the table --------------------------------------------------------------------------

// ---- device buffers ----------------------------------------------------------------------------
struct In {  // an input: what was uploaded is kept, to show the launch left it alone
  uint8_t* d = nullptr;
  std::vector<uint8_t> h;
  In() = default;
  In(const In&) = delete;
  In& operator=(const In&) = delete;
  ~In() { if (d) (void)hipFree(d); }
  void put(const void* p, size_t bytes) {
    h.assign((const uint8_t*)p, (const uint8_t*)p + bytes);
    CK(hipMalloc(reinterpret_cast<void**>(&d), std::max<size_t>(bytes, 16)));
    if (bytes) CK(hipMemcpy(d, p, bytes, hipMemcpyHostToDevice));
  }
  template <class T> const T* as() const { return reinterpret_cast<const T*>(d); }
  bool same() const {
    std::vector<uint8_t> g(h.size());
    if (!g.empty()) CK(hipMemcpy(g.data(), d, g.size(), hipMemcpyDeviceToHost));
    return g == h;
  }
};
struct Flags {
  bool canary_ok = true, inputs_ok = true, repeat_ok = true;
  long variant_bad = 0;
  bool variants_run = false;
};
struct Job {
  std::vector<std::unique_ptr<In>> ins;
  std::vector<std::unique_ptr<Guarded>> outs;
  std::vector<char> free_order;  // outputs whose content is a set or scratch: left out of the repeat comparison
  template <class T> In* in(const std::vector<T>& v) {
    ins.emplace_back(new In);
    ins.back()->put(v.data(), v.size() * sizeof(T));
    return ins.back().get();
  }
  // bf16 storage of fp32 values that are bf16 numbers already
  In* in_bf(const std::vector<float>& v) {
    std::vector<uint16_t> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = gck::f2bf(v[i]);
    return in(h);
  }
  Guarded* out(size_t bytes, bool any_order = false) {
    outs.emplace_back(new Guarded);
    outs.back()->alloc(bytes);
    outs.back()->fill32(kFillWord);
    free_order.push_back(any_order);
    return outs.back().get();
  }
  // an in-out buffer: the payload starts as `v`
  template <class T> Guarded* inout(const std::vector<T>& v, bool any_order = false) {
    Guarded* g = out(v.size() * sizeof(T), any_order);
    std::memcpy(g->fill(), v.data(), v.size() * sizeof(T));
    return g;
  }
  // launch, read back, check guards and inputs; launch again over fresh fills: bit-equal
  void run(const std::function<void()>& launch, Flags& F) {
    for (auto& o : outs) o->upload();
    launch();
    CK(hipDeviceSynchronize());
    std::vector<std::vector<uint8_t>> first;
    for (auto& o : outs) {
      o->download();
      F.canary_ok &= o->intact();
      first.push_back(o->got);
    }
    for (auto& o : outs) o->upload();
    launch();
    CK(hipDeviceSynchronize());
    for (size_t i = 0; i < outs.size(); ++i) {
      outs[i]->download();
      F.canary_ok &= outs[i]->intact();
      if (!free_order[i]) F.repeat_ok &= outs[i]->got == first[i];
    }
    for (auto& i : ins) F.inputs_ok &= i->same();
  }
  // launch again (a variant of the same stage) and count the outputs picked by `which` that differ from `want`
  long again(const std::function<void()>& launch, const std::vector<int>& which, const std::vector<std::vector<uint8_t>>& want, Flags& F) {
    for (auto& o : outs) o->upload();
    launch();
    CK(hipDeviceSynchronize());
    long bad = 0;
    for (size_t i = 0; i < outs.size(); ++i) {
      outs[i]->download();
      F.canary_ok &= outs[i]->intact();
    }
    for (size_t k = 0; k < which.size(); ++k) bad += outs[which[k]]->got != want[k];
    return bad;
  }
};
template <class T> static std::vector<T> take(const Guarded* g, size_t n) {
  std::vector<T> v(n);
  if (n) std::memcpy(v.data(), g->out(), n * sizeof(T));
  return v;
}

static float* g_params = nullptr;  // [PHX_NPATCH_DEV + 1]: the loss reads only the scale at [PHX_NPATCH_DEV]
static void set_scale(float s) {
  if (!g_params) {
    CK(hipMalloc(reinterpret_cast<void**>(&g_params), ((size_t)PHX_NPATCH_DEV + 1) * 4));
    CK(hipMemset(g_params, 0, ((size_t)PHX_NPATCH_DEV + 1) * 4));
  }
  CK(hipMemcpy(g_params + PHX_NPATCH_DEV, &s, 4, hipMemcpyHostToDevice));
}
struct NoFast {  // PHX_NMS_FAST=0 for the launches in scope (the library reads it per call)
  NoFast() { setenv("PHX_NMS_FAST", "0", 1); }
  ~NoFast() { unsetenv("PHX_NMS_FAST"); }
};

// the library's expf on the device, for the expf figure (not a kernel under test)
__global__ void k_expf(const float* __restrict__ x, float* __restrict__ y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = expf(x[i]);
}
static double measure_device_expf() {
  const std::vector<float> x = exp_args();
  Job j;
  In* xi = j.in(x);
  Guarded* yo = j.out(x.size() * 4);
  yo->upload();
  hipLaunchKernelGGL(k_expf, dim3((unsigned)((x.size() + 255) / 256)), dim3(256), 0, nullptr, xi->as<float>(), yo->ptr(), (int)x.size());
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  yo->download();
  return exp_max_ulp(x, take<float>(yo, x.size()));
}

// ---- the device backend --------------------------------------------------------------------------
struct Gpu {
  Flags F;
  hipStream_t s = nullptr;
  std::vector<LevelDesc> levels(const Chain& ch) {
    std::vector<LevelDesc> lv(ch.lev.size());
    std::memcpy(lv.data(), ch.lev.data(), lv.size() * sizeof(LevelDesc));
    return lv;
  }
  void pre_nms(const Chain& ch, PreOut& o) {
    const Case& c = ch.c;
    const size_t BA = (size_t)c.B * ch.A;
    Job j;
    In* cls = c.bf ? j.in_bf(ch.cls) : j.in(ch.cls);
    In* box = c.bf ? j.in_bf(ch.box) : j.in(ch.box);
    In* lev = j.in(levels(ch));
    In* an = j.in(ch.anchors);
    Guarded* sc = j.out(BA * 4);
    Guarded* cl = j.out(BA * 4);
    Guarded* bx = j.out(BA * 16);
    Guarded* kp = j.out(BA);
    Guarded* li = j.out(BA * 4, true);  // a set per image: any order
    Guarded* cn = j.inout(std::vector<int>(c.B, 0));
    NmsCand cand;
    if (c.cand_list) { cand.list = reinterpret_cast<int*>(li->ptr()); cand.count = reinterpret_cast<int*>(cn->ptr()); }
    cand.mask = c.cand_mask; cand.thresh = c.cand_thresh;
    std::vector<std::vector<int>> first_sets;
    auto sets = [&] {
      std::vector<std::vector<int>> v;
      const std::vector<int> cnt = take<int>(cn, c.B), lst = take<int>(li, BA);
      for (int b = 0; b < c.B; ++b) {
        const int n = std::min(std::max(cnt[b], 0), ch.A);
        v.emplace_back(lst.begin() + (size_t)b * ch.A, lst.begin() + (size_t)b * ch.A + n);
        std::sort(v.back().begin(), v.back().end());
      }
      return v;
    };
    int pass = 0;
    j.run([&] {
      if (pass++ == 1) first_sets = sets();  // (the first launch's outputs are downloaded by now)
      launch_pre_nms(cls->as<float>(), box->as<float>(), lev->as<LevelDesc>(), ch.nlev, an->as<float>(), ch.A, c.B, c.nclass, c.na,
                     ch.img, ch.img, c.thresh, sc->ptr(), reinterpret_cast<int*>(cl->ptr()), bx->ptr(),
                     reinterpret_cast<uint8_t*>(kp->ptr()), ch.ntiles, s, cand, c.bf != 0);
    }, F);
    if (c.cand_list) F.repeat_ok &= sets() == first_sets;
    o.scores = take<float>(sc, BA);
    o.classes = take<int>(cl, BA);
    o.boxes = take<float>(bx, BA * 4);
    o.keep = take<uint8_t>(kp, BA);
    o.list = c.cand_list ? take<int>(li, BA) : std::vector<int>();
    o.count = c.cand_list ? take<int>(cn, c.B) : std::vector<int>();
    if (!c.cand_list) {  // no list: the list and count buffers keep their fills
      F.canary_ok &= li->got == li->init && cn->got == cn->init;
    }
  }
  void soft_nms(const NmsIn& in, const std::vector<uint8_t>* keep, int keep_mask, const std::vector<int>* count, const PreOut* lists,
                NmsOut& o) {
    const size_t rows = (size_t)in.B * in.max_out;
    Job j;
    In* bx = j.in(in.boxes);
    In* sc = j.in(in.scores);
    In* kp = keep ? j.in(*keep) : nullptr;
    In* cn = count ? j.in(*count) : nullptr;
    Guarded* ob = j.out(rows * 16);
    Guarded* os = j.out(rows * 4);
    Guarded* oc = j.out((size_t)in.B * 4);
    Guarded* oi = j.out(rows * 4);
    Guarded* wk = j.out(soft_nms_work_floats(in.B, in.N) * 4, true);  // scratch
    Guarded* li = lists ? j.inout(lists->list) : nullptr;
    Guarded* lc = lists ? j.inout(lists->count) : nullptr;
    auto go = [&](bool with_index) {
      return [&, with_index] {
        NmsCand cand;
        if (lists) { cand.list = reinterpret_cast<int*>(li->ptr()); cand.count = reinterpret_cast<int*>(lc->ptr()); }
        launch_soft_nms(bx->as<float>(), sc->as<float>(), kp ? kp->as<uint8_t>() : nullptr, keep_mask, cn ? cn->as<int>() : nullptr,
                        in.B, in.N, in.thresh, in.sigma, in.max_out, in.clip, ob->ptr(), os->ptr(), reinterpret_cast<int*>(oc->ptr()),
                        wk->ptr(), s, cand, with_index ? reinterpret_cast<int*>(oi->ptr()) : nullptr);
      };
    };
    j.run(go(true), F);
    o.boxes = take<float>(ob, rows * 4);
    o.scores = take<float>(os, rows);
    o.count = take<int>(oc, in.B);
    o.index = take<int>(oi, rows);
    o.cand_count = lists ? take<int>(lc, in.B) : std::vector<int>();
    const std::vector<uint8_t> g_b = ob->got, g_s = os->got, g_c = oc->got, g_i = oi->got;
    F.variants_run = true;
    // out_index null: the same other outputs, the index buffer keeps its fill
    F.variant_bad += j.again(go(false), {0, 1, 2, 3}, {g_b, g_s, g_c, oi->init}, F);
    {
      NoFast nf;
      F.variant_bad += j.again(go(true), {0, 1, 2, 3}, {g_b, g_s, g_c, g_i}, F);
    }
    if (lists) {
      // the same candidates in another order: reversed, then odd positions before even ones
      std::vector<int> sh = lists->list;
      for (int b = 0; b < in.B; ++b) {
        int* l = sh.data() + (size_t)b * in.N;
        const int n = lists->count[b];
        std::vector<int> r;
        for (int par = 1; par >= 0; --par)
          for (int i = n - 1; i >= 0; --i)
            if (((n - 1 - i) & 1) == par) r.push_back(l[i]);
        std::copy(r.begin(), r.end(), l);
      }
      std::memcpy(li->fill(), sh.data(), sh.size() * 4);
      F.variant_bad += j.again(go(true), {0, 1, 2, 3}, {g_b, g_s, g_c, g_i}, F);
      NoFast nf;
      F.variant_bad += j.again(go(true), {0, 1, 2, 3}, {g_b, g_s, g_c, g_i}, F);
    }
    for (auto& i : j.ins) F.inputs_ok &= i->same();
  }
  void image_max(const std::vector<float>& sc, const std::vector<uint8_t>& keep, int B, int A, ImaxOut& o) {
    Job j;
    In* s_ = j.in(sc);
    In* k_ = j.in(keep);
    Guarded* m = j.out((size_t)B * 4);
    Guarded* am = j.out((size_t)B * 4);
    Guarded* nt = j.out((size_t)B * 4);
    Guarded* scr = j.out(image_max_scratch_ints(B) * 4);
    j.run([&] {
      launch_image_max(s_->as<float>(), k_->as<uint8_t>(), B, A, m->ptr(), reinterpret_cast<int*>(am->ptr()), reinterpret_cast<int*>(nt->ptr()),
                       reinterpret_cast<int*>(scr->ptr()), s);
    }, F);
    o.m = take<float>(m, B);
    o.argm = take<int>(am, B);
    o.nties = take<int>(nt, B);
  }
  void loss(const std::vector<float>& mraw, float sv, LossOut& o) {
    const int B = (int)mraw.size();
    Job j;
    In* mr = j.in(mraw);
    Guarded* dm = j.out((size_t)B * 4);
    Guarded* ds = j.out(4);
    Guarded* me = j.inout(metrics0());
    set_scale(sv);
    j.run([&] { launch_loss(mr->as<float>(), B, g_params, dm->ptr(), ds->ptr(), me->ptr(), s); }, F);
    o.dm = take<float>(dm, B);
    o.dscale = take<float>(ds, 1)[0];
    o.metrics = take<float>(me, PHX_NMETRIC);
  }
  float count_ge(const std::vector<float>& sc, const std::vector<int>& cnt, int maxo, float th) {
    Job j;
    In* s_ = j.in(sc);
    In* c_ = j.in(cnt);
    Guarded* o = j.out(4);
    j.run([&] { launch_count_ge(s_->as<float>(), c_->as<int>(), (int)cnt.size(), maxo, th, o->ptr(), s); }, F);
    return take<float>(o, 1)[0];
  }
  void zero_segs(const Segs& sg, std::vector<uint8_t>& fill, std::vector<uint8_t>& got) {
    Job j;
    Guarded* buf = j.out(sg.total);
    std::vector<char*> ptr;
    for (size_t off : sg.off) ptr.push_back(reinterpret_cast<char*>(buf->ptr()) + off);
    j.run([&] { launch_zero_segs(ptr.data(), sg.bytes.data(), (int)ptr.size(), s); }, F);
    fill.assign(buf->fill(), buf->fill() + sg.total);
    got.assign(buf->out(), buf->out() + sg.total);
  }
  void cls_scatter(const ScatterIn& si, std::vector<float>& dx) {
    const Chain& ch = *si.ch;
    const Case& c = ch.c;
    const size_t BA = (size_t)c.B * ch.A;
    Job j;
    In* sc = j.in(std::vector<float>(si.scores, si.scores + BA));
    In* kp = j.in(std::vector<uint8_t>(si.keep, si.keep + BA));
    In* mr = j.in(std::vector<float>(si.mraw, si.mraw + c.B));
    In* nt = j.in(std::vector<int>(si.nties, si.nties + c.B));
    In* dm = j.in(std::vector<float>(si.dm, si.dm + c.B));
    In* cls = c.bf ? j.in_bf(ch.cls) : j.in(ch.cls);
    In* lev = j.in(levels(ch));
    In* wp = j.in(ch.wpred);
    In* off = j.in(ch.dx_off);
    Guarded* d = j.inout(ch.dx0);
    j.run([&] {
      launch_cls_scatter(sc->as<float>(), kp->as<uint8_t>(), mr->as<float>(), nt->as<int>(), dm->as<float>(), cls->as<float>(),
                         lev->as<LevelDesc>(), ch.nlev, ch.A, c.B, c.nclass, c.na, wp->as<float>(), c.K, d->ptr(), off->as<long>(), s,
                         c.bf != 0);
    }, F);
    dx = take<float>(d, ch.dx0.size());
  }
  void adam(const AdamIO& in, float lr, int t, bool clip, AdamIO& o) {
    const size_t n = in.p.size();
    Job j;
    In* g = j.in(in.g);
    Guarded* p = j.inout(in.p);
    Guarded* m = j.inout(in.m);
    Guarded* v = j.inout(in.v);
    j.run([&] {
      if (clip) launch_adam_clip(p->ptr(), g->as<float>(), m->ptr(), v->ptr(), (long)n, lr, t, s);
      else launch_adam(p->ptr(), g->as<float>(), m->ptr(), v->ptr(), (long)n, lr, t, s);
    }, F);
    o.p = take<float>(p, n); o.m = take<float>(m, n); o.v = take<float>(v, n);
  }
};

// ---- refusals ------------------------------------------------------------------------------------
struct Refusal {
  bool threw = false, untouched = true, inputs_ok = true;
  std::string what;
};
static Refusal run_refusal(const Case& c) {
  Refusal r;
  Job j;
  auto attempt = [&](const std::function<void()>& launch) {
    for (auto& o : j.outs) o->upload();
    try {
      launch();
    } catch (const phx::HipError&) {
      throw;
    } catch (const std::exception& e) {
      r.threw = true;
      r.what = e.what();
    }
    CK(hipDeviceSynchronize());
    for (auto& o : j.outs) {
      o->download();
      r.untouched &= o->got == o->init;
    }
    for (auto& i : j.ins) r.inputs_ok &= i->same();
  };
  if (c.refuse == R_NMS_MAXOUT101) {
    std::vector<uint8_t> keep;
    std::vector<int> count;
    const NmsIn in = make_nms(c, keep, count);
    const size_t rows = (size_t)in.B * in.max_out;
    In* bx = j.in(in.boxes);
    In* sc = j.in(in.scores);
    In* kp = j.in(keep);
    Guarded* ob = j.out(rows * 16);
    Guarded* os = j.out(rows * 4);
    Guarded* oc = j.out((size_t)in.B * 4);
    Guarded* oi = j.out(rows * 4);
    Guarded* wk = j.out(soft_nms_work_floats(in.B, in.N) * 4);
    attempt([&] {
      launch_soft_nms(bx->as<float>(), sc->as<float>(), kp->as<uint8_t>(), 1, nullptr, in.B, in.N, in.thresh, in.sigma, in.max_out, in.clip,
                      ob->ptr(), os->ptr(), reinterpret_cast<int*>(oc->ptr()), wk->ptr(), nullptr, NmsCand{}, reinterpret_cast<int*>(oi->ptr()));
    });
  } else if (c.refuse == R_ZERO_9 || c.refuse == R_ZERO_MISALIGNED) {
    const Segs sg = make_segs(c.nseg);
    Guarded* buf = j.out(sg.total);
    std::vector<char*> ptr;
    for (size_t off : sg.off) ptr.push_back(reinterpret_cast<char*>(buf->ptr()) + off);
    if (c.refuse == R_ZERO_MISALIGNED) ptr[1] += 4;  // (its 16-byte gap keeps the segment inside the buffer)
    attempt([&] { launch_zero_segs(ptr.data(), sg.bytes.data(), (int)ptr.size(), nullptr); });
  } else {
    // valid, properly sized inputs by the stand-in; A % na != 0: one anchor fewer than the buffers hold
    const Chain ch = make_chain(c);
    Sim sim;
    PreOut po;
    sim.pre_nms(ch, po);
    ImaxOut io;
    sim.image_max(po.scores, po.keep, c.B, ch.A, io);
    LossOut lo;
    sim.loss(io.m, c.scale, lo);
    In* sc = j.in(po.scores);
    In* kp = j.in(po.keep);
    In* mr = j.in(io.m);
    In* nt = j.in(io.nties);
    In* dm = j.in(lo.dm);
    In* cls = j.in(ch.cls);
    std::vector<LevelDesc> lv(ch.lev.size());
    std::memcpy(lv.data(), ch.lev.data(), lv.size() * sizeof(LevelDesc));
    In* lev = j.in(lv);
    In* wp = j.in(ch.wpred);
    In* off = j.in(ch.dx_off);
    Guarded* d = j.inout(ch.dx0);
    const int A = c.refuse == R_SCATTER_AMODNA ? ch.A - 1 : ch.A;
    attempt([&] {
      launch_cls_scatter(sc->as<float>(), kp->as<uint8_t>(), mr->as<float>(), nt->as<int>(), dm->as<float>(), cls->as<float>(),
                         lev->as<LevelDesc>(), ch.nlev, A, c.B, c.nclass, c.na, wp->as<float>(), c.K, d->ptr(), off->as<long>(), nullptr);
    });
  }
  return r;
}

// ---- JSON ------------------------------------------------------------------------------------------
static std::string j(const char* k, long v, bool first = false) {
  return std::string(first ? "\"" : ",\"") + k + "\":" + std::to_string(v);
}
static std::string jd(const char* k, double v) { return std::string(",\"") + k + "\":" + jnum(v); }
static std::string jl(const char* k, const std::vector<long>& v) {
  std::string s = std::string(",\"") + k + "\":[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
  return s + "]";
}
static const char* kind_name(int k) {
  static const char* n[] = {"chain", "nms", "imax", "loss", "zero", "count", "adam", "refuse"};
  return n[k];
}
static std::string case_head(const Case& c) {
  return std::string("{\"case\":\"") + c.name + "\",\"kind\":\"" + kind_name(c.kind) + "\"" + j("refuse", c.refuse) + j("B", c.B) +
         j("nclass", c.nclass) + j("na", c.na) + j("bf", c.bf) + j("cand_mask", c.cand_mask) + j("cand_list", c.cand_list) +
         jd("cand_thresh", c.cand_thresh) + j("K", c.K) + j("max_out", c.max_out) + j("nseg", c.nseg) + j("N", c.N) +
         j("nms_mode", c.nms_mode) + j("n", c.n) + j("t", c.t) + j("clip", c.clip);
}
static void print_plan(const Case& c, FILE* f) {
  std::string s = case_head(c);
  if (c.kind != K_REFUSE) {
    Sim sim;
    Verdict V;
    CaseStats st;
    run_case(c, sim, V, &st);
    s += "," + verdict_json(V) + ",\"standin_pass\":" + (V.pass() ? "true" : "false") + j("elems", st.elems);
    if (c.kind == K_CHAIN) {
      const Chain ch = make_chain(c);
      const PreStats& p = st.pre;
      s += j("A", ch.A) + j("ntiles", ch.ntiles) + j("aligned_tiles", st.aligned_tiles) + j("unaligned_tiles", st.unaligned_tiles) +
           j("ragged_tiles", st.ragged_tiles) + j("short_tiles", st.short_tiles) + j("lds_bytes", (long)kPreTile * c.nclass * 4) +
           j("tie_first_half", p.tie_first_half) + j("tie_both_halves", p.tie_both_halves) + j("second_greater", p.second_greater) +
           j("all_equal", p.all_equal) + j("max_last", p.max_last) + jl("keep_hist", std::vector<long>(p.keep_hist, p.keep_hist + 8)) +
           j("cls_nonzero", p.cls_nonzero) + j("sc_eq_thresh", p.sc_eq_thresh) + j("sc_ge", p.sc_ge) + j("sc_lt", p.sc_lt) +
           j("bw_eq_1", p.bw_eq_1) + j("area_eq_100", p.area_eq_100) + j("area_just_above", p.area_just_above) + jl("cand", p.cand);
      std::string pl = ",\"plants\":[";
      for (size_t i = 0; i < ch.plants.size(); ++i)
        pl += std::string(i ? "," : "") + "[\"" + ch.plants[i].what + "\"," + std::to_string(ch.plants[i].b) + "," + std::to_string(ch.plants[i].a) + "]";
      s += pl + "]";
      const ScatterStats& q = st.sc;
      s += j("sc_rows_written", q.rows_written) + j("sc_win_anchors", q.win_anchors) + j("sc_max_class_ties", q.max_class_ties) +
           j("sc_pixels_2_winners", q.pixels_2_winners) + j("sc_levels_hit", q.levels_hit) + j("sc_images_dm0", q.images_dm0);
    }
    if (c.kind == K_CHAIN || c.kind == K_NMS) {
      const NmsStats& n = st.nms;
      const int N = c.kind == K_CHAIN ? make_chain(c).A : c.N;
      const PostPlanInfo pi = post_plan_info(N);
      s += j("nms_candidates", n.candidates) + j("nms_pops", n.pops) + j("nms_requeues", n.requeues) + j("nms_tie_pops", n.tie_pops) +
           j("nms_dup_visits", n.dup_visits) + j("nms_max_first_overlaps", n.max_first_overlaps) + j("nms_selected", n.selected) +
           jd("nms_min_margin", n.min_margin) + jd("nms_min_arg", n.min_arg) + j("nms_m", pi.nms_m) + j("nms_cap", pi.nms_cap) +
           j("nms_lp", pi.nms_lp) + j("nms_qrows", pi.nms_qrows) + j("nms_lds", pi.nms_lds) + j("nms_top_want", pi.nms_top_want);
    }
    if (c.kind == K_CHAIN || c.kind == K_IMAX) {
      const ImaxStats& m = st.imax;
      s += j("imax_empty_images", m.empty_images) + j("imax_ties_in_chunk", m.ties_in_chunk) + j("imax_ties_2_chunks", m.ties_2_chunks) +
           j("imax_ties_3_chunks", m.ties_3_chunks) + j("imax_empty_chunks", m.empty_chunks) + j("imax_max_zero", m.max_zero) +
           j("imax_max_neg", m.max_neg) + j("imax_bits_without_1", m.bits_without_1);
    }
  }
  fprintf(f, "%s}\n", s.c_str());
  fflush(f);
}

// ---- main ----------------------------------------------------------------------------------------
int main(int argc, char** argv) {
  const std::vector<Case> t = table();
  if (argc > 1 && std::string(argv[1]) == "--plan") {
    // the host's expf through the same measurement, for the stand-in's bounds
    const std::vector<float> x = exp_args();
    std::vector<float> y(x.size());
    for (size_t i = 0; i < x.size(); ++i) y[i] = expf(x[i]);
    const double host_ulp = exp_max_ulp(x, y);
    set_exp_ulp(host_ulp);
    for (const Case& c : t) print_plan(c, stdout);
    const PostPlanInfo pi = post_plan_info(846);
    printf("{\"done\":true,\"cases\":%d,\"host_exp_ulp\":%s,\"pre_tile\":%d,\"check_pre_tile\":%d,\"imax_chunks\":%d,\"check_imax_chunks\":%d,"
           "\"nms_fl\":%d,\"check_nms_fl\":%d}\n", (int)t.size(), jnum(host_ulp).c_str(), pi.pre_tile, kPreTile, pi.imax_chunks, kImaxChunks,
           pi.nms_fl, kNmsFl);
    return 0;
  }
  const char* only = argc > 1 ? argv[1] : nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  g_case = "expf";
  const double dev_ulp = measure_device_expf();
  set_exp_ulp(dev_ulp);
  int ran = 0;
  for (const Case& c : t) {
    if (only && c.name != only) continue;
    g_case = c.name.c_str();
    const auto c0 = std::chrono::steady_clock::now();
    std::string s = case_head(c);
    bool pass = false;
    auto b = [](bool x) { return x ? "true" : "false"; };
    try {
      if (c.refuse) {
        const Refusal r = run_refusal(c);
        pass = r.threw && r.untouched && r.inputs_ok;
        s += std::string(",\"threw\":") + b(r.threw) + ",\"untouched\":" + b(r.untouched) + ",\"inputs_ok\":" + b(r.inputs_ok) +
             ",\"what\":\"" + esc(r.what) + "\"";
      } else {
        Gpu gpu;
        Verdict V;
        run_case(c, gpu, V);
        const Flags& F = gpu.F;
        if (F.variants_run) V.fields["nms_variant_bad"] = (double)F.variant_bad;
        pass = V.pass() && F.canary_ok && F.repeat_ok && F.inputs_ok;
        s += std::string(",\"threw\":false,") + verdict_json(V) + ",\"canary_ok\":" + b(F.canary_ok) + ",\"repeat_ok\":" + b(F.repeat_ok) +
             ",\"inputs_ok\":" + b(F.inputs_ok);
      }
    } catch (const phx::HipError& e) {
      fatal(e.what(), g_case);
    } catch (const std::exception& e) {
      s += std::string(",\"threw\":true,\"unexpected\":\"") + esc(e.what()) + "\"";
      pass = false;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    printf("%s,\"ms\":%s,\"pass\":%s}\n", s.c_str(), jnum(ms).c_str(), pass ? "true" : "false");
    fflush(stdout);
    ++ran;
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("{\"done\":true,\"cases\":%d,\"seconds\":%s,\"exp_ulp_measured\":%s,\"exp_ulp_used\":%s}\n", ran, jnum(sec).c_str(),
         jnum(dev_ulp).c_str(), jnum(g_exp_ulp).c_str());
  return 0;
}
