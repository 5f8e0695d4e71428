// eot_parity — kernel-level parity of the EOT patch pipeline (kernels_eot.hip) against an fp64 host reference,
// stage by stage: placement and its compact lists (k_eot_place, k_eot_spans, k_eot_bands), the brightness
// matcher, the banded resize, the compositor with its owner map and mask, the rotation gradient, the two-stage
// resize adjoint, the patch gradient and TV.
//
//   eot_parity --plan   the case table with each case's geometry by the reference alone (the placement's lists,
//                       row tiles per XCD band, workgroups that straddle two images, ballot rounds, chunks), the
//                       share of elements under the decision allowance, the placement's truncation margin, and
//                       the CPU stand-in's verdict (host code only: runs without a GPU)
//   eot_parity          run the table on the GPU: one flushed JSON line per case, then a `done` line
//
// Only the launchers of post.hpp are called.  Every stage after placement takes its BoxPlace, lists, spans and
// tensors from what the device wrote in the stages before, read back to the host.  Composite and resize_bwd run
// a second time with PHX_EOT_V1=1 (read per call): bit-equal.  The exit status is 0 when every case ran (the
// verdicts are in the lines); a HIP error ends the process at once with a `fatal` line and status 3.
// Build: make -C tests/kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "eot_check.hpp"
#include "parity_dev.hpp"

using namespace eck;

// ---- the case table ----------------------------------------------------------------------------
static std::vector<Case> table() {
  std::vector<Case> t;
  auto ec = [&](const char* name, int B, int H, int W, int maxb, int P, std::vector<int> counts, std::vector<int> ps,
                std::function<void(Case&)> more = nullptr) {
    Case c;
    c.name = name; c.B = B; c.H = H; c.W = W; c.maxb = maxb; c.P = P; c.counts = counts; c.ps = ps;
    c.seed = 100 + t.size();
    if (more) more(c);
    t.push_back(c);
  };
  // a. placement and its lists.  B maxb <= 256, == 256, > 256 (two passes of the 256-slot scan); images without
  // boxes first, in the middle and last; no valid box at all; boxes invalid by ps <= 2 and by ps > span_stride
  ec("small_b2_p24", 2, 64, 48, 4, 24, {3, 2}, {10, 17, 6, 24, 30});
  ec("scan_256_b4_m64", 4, 48, 40, 64, 24, {5, 64, 0, 9}, {5, 8, 3, 11, 16, 7});
  ec("place_maxb128_place_only", 2, 48, 40, 128, 24, {128, 3}, {5, 8, 3, 11}, [](Case& c) { c.step = 5; c.gimg0 = 6; c.place_only = 1; });
  ec("scan_300_chunks_p37", 3, 72, 64, 100, 37, {100, 100, 100}, {44, 43, 42}, [](Case& c) { c.amp = 0.01f; });
  ec("empty_images_b5", 5, 48, 40, 4, 24, {0, 2, 0, 3, 0}, {9, 14, 20, 5, 12});
  ec("no_valid_box", 2, 40, 36, 3, 24, {2, 1}, {2, 1, 2}, [](Case& c) { c.img_amp = 1.3f; });
  ec("invalid_small_and_big", 1, 64, 56, 4, 24, {4}, {2, 40, 12, 9}, [](Case& c) { c.span_stride = 16; });
  ec("defender_rule_b3", 3, 64, 56, 5, 37, {2, 5, 1}, {12, 30, 7, 19}, [](Case& c) { c.defender = 1; c.batch = 1; c.add_tv = 0; c.add_loss = 0; c.gimg0 = 9; });
  // b. the resize ladder at P 64: ps 3, P/4 and below (vertical spans >= 8 taps: the unrolled loop), between,
  // P - 1, P, above P; ps % 4 != 0 (ragged last row tile); nt < 8 (empty bands), nt 8, nt 9; ps^2 <= 256 and just
  // above (a partial second chunk)
  ec("ladder_p64", 1, 128, 112, 10, 64, {10}, {3, 16, 13, 33, 63, 64, 70, 31, 17, 47});
  ec("ladder_p64_noise_off", 1, 128, 112, 6, 64, {6}, {16, 33, 63, 64, 70, 9}, [](Case& c) { c.amp = 0.f; c.apply_print = 0; });
  ec("p160_b2", 2, 96, 88, 3, 160, {3, 2}, {40, 159, 160, 37, 200}, [](Case& c) { c.clipw = 1; });
  ec("p5_b1_mostly_empty_sum_chunks", 1, 40, 36, 3, 5, {3}, {7, 3, 5}, [](Case& c) { c.apply_print = 0; c.img_amp = 1.3f; });
  ec("p37_b3_odd_nx", 3, 56, 48, 4, 37, {3, 2, 4}, {30, 9, 14, 22, 41, 37, 36}, [](Case& c) { c.clipw = 1; c.plant = 1; });
  // c. the production ratios at P 640 (one or a few boxes: the adjoint's row buffer stays under the element cap)
  ec("p640_quarter_and_below", 1, 96, 80, 4, 640, {4}, {160, 150, 97, 3});
  ec("p640_ps639", 1, 96, 80, 1, 640, {1}, {639}, [](Case& c) { c.add_tv = 0; });
  ec("p640_ps640", 1, 96, 80, 1, 640, {1}, {640}, [](Case& c) { c.apply_print = 0; c.add_loss = 0; });
  ec("p640_ps700_upscale", 1, 96, 80, 1, 640, {1}, {700}, [](Case& c) { c.amp = 0.f; });
  // d. the compositor: H W no multiple of 256 with B >= 2 (workgroups that straddle two images: the unstaged
  // path) and a multiple; W < 256 (a workgroup spans rows) and W >= 256 (inside one row); more than 64 valid
  // boxes on one image (a second ballot round); overlapping boxes with planted fill; images beyond [-1, 1];
  // boxes pressed into each corner
  ec("unstaged_b2_50x47_cluster", 2, 50, 47, 4, 24, {4, 3}, {14, 11, 17, 9}, [](Case& c) { c.layout = L_CLUSTER; c.img_amp = 1.3f; c.plant = 1; });
  ec("unstaged_b2_301x300", 2, 301, 300, 3, 24, {3, 2}, {40, 25, 90}, [](Case& c) { c.img_amp = 1.2f; });
  ec("row_wg_w256_80_boxes", 1, 264, 256, 80, 24, {80}, {3, 4, 5}, [](Case& c) { c.layout = L_GRID; });
  ec("corners_b2", 2, 64, 64, 4, 24, {4, 4}, {20, 13, 30, 8}, [](Case& c) { c.layout = L_CORNERS; c.img_amp = 1.3f; });
  ec("cluster_overlap_noprint", 1, 80, 64, 6, 37, {6}, {30, 21, 26, 17, 35, 12}, [](Case& c) { c.layout = L_CLUSTER; c.apply_print = 0; c.plant = 1; });
  ec("defender_cluster_clipw", 2, 64, 64, 4, 24, {3, 4}, {15, 22, 10}, [](Case& c) { c.layout = L_CLUSTER; c.defender = 1; c.batch = 1; c.clipw = 1; c.img_amp = 1.1f; });
  // e. refusals: nothing is launched, every output keeps its fill
  ec("refuse_place_maxb129", 1, 48, 40, 129, 24, {2}, {9, 12}, [](Case& c) { c.refuse = R_PLACE_129; });
  ec("refuse_composite_maxb101", 1, 48, 40, 101, 24, {2}, {9, 12}, [](Case& c) { c.refuse = R_COMPOSITE_101; });
  ec("refuse_resize_bwd_maxb101", 1, 48, 40, 101, 24, {2}, {9, 12}, [](Case& c) { c.refuse = R_RESIZE_BWD_101; });
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
  bool canary_ok = true, inputs_ok = true, repeat_ok = true, v1_ok = true, variants_ok = true;
};
struct Job {
  std::vector<std::unique_ptr<In>> ins;
  std::vector<std::unique_ptr<Guarded>> outs;
  template <class T> In* in(const std::vector<T>& v) {
    ins.emplace_back(new In);
    ins.back()->put(v.data(), v.size() * sizeof(T));
    return ins.back().get();
  }
  In* in_bytes(const void* p, size_t n) {
    ins.emplace_back(new In);
    ins.back()->put(p, n);
    return ins.back().get();
  }
  // fill: a 32-bit word, or 0 for the guard byte throughout
  Guarded* out(size_t bytes, uint32_t fill = kFillWord) {
    outs.emplace_back(new Guarded);
    outs.back()->alloc(bytes);
    if (fill) outs.back()->fill32(fill);
    return outs.back().get();
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
      F.repeat_ok &= outs[i]->got == first[i];
    }
    for (auto& i : ins) F.inputs_ok &= i->same();
  }
  // launch again (another variant of the same stage) and compare the outputs picked by `which` with `want`
  bool again(const std::function<void()>& launch, const std::vector<int>& which, const std::vector<std::vector<uint8_t>>& want, Flags& F) {
    for (auto& o : outs) o->upload();
    launch();
    CK(hipDeviceSynchronize());
    bool eq = true;
    for (size_t i = 0; i < outs.size(); ++i) {
      outs[i]->download();
      F.canary_ok &= outs[i]->intact();
    }
    for (size_t k = 0; k < which.size(); ++k) eq &= outs[which[k]]->got == want[k];
    return eq;
  }
};
template <class T> static std::vector<T> take(const Guarded* g, size_t n) {
  std::vector<T> v(n);
  std::memcpy(v.data(), g->out(), n * sizeof(T));
  return v;
}

static float* g_params = nullptr;  // [PHX_NPATCH_DEV + 1]: only the scale at [PHX_NPATCH_DEV] is read
static void set_scale(float s) {
  if (!g_params) {
    CK(hipMalloc(reinterpret_cast<void**>(&g_params), ((size_t)PHX_NPATCH_DEV + 1) * 4));
    CK(hipMemset(g_params, 0, ((size_t)PHX_NPATCH_DEV + 1) * 4));
  }
  CK(hipMemcpy(g_params + PHX_NPATCH_DEV, &s, 4, hipMemcpyHostToDevice));
}
struct V1 {  // PHX_EOT_V1 for the launches in scope (the library reads it per call)
  V1() { setenv("PHX_EOT_V1", "1", 1); }
  ~V1() { unsetenv("PHX_EOT_V1"); }
};

// ---- the device backend --------------------------------------------------------------------------
struct Gpu {
  Flags F;
  hipStream_t s = nullptr;
  void place(const Inputs& in, PlaceOut& po) {
    const EotDims& d = in.d;
    Job j;
    In* boxes = j.in(in.boxes);
    In* count = j.in(in.count);
    const size_t nslot = (size_t)d.B * d.maxb;
    Guarded* img = j.out(d.B * sizeof(ImgParams));
    Guarded* pb = j.out(eot_place_bytes(d.B, d.maxb), 0);
    Guarded* sp = j.out(nslot * d.span_stride * sizeof(SpanEntry), 0);
    Guarded* err = j.out(4);
    set_scale(in.c.scale);
    j.run([&] {
      launch_eot_place(d, boxes->as<float>(), count->as<int>(), g_params, in.c.seed, in.c.step, in.c.gimg0,
                       reinterpret_cast<ImgParams*>(img->ptr()), reinterpret_cast<BoxPlace*>(pb->ptr()),
                       reinterpret_cast<SpanEntry*>(sp->ptr()), reinterpret_cast<int*>(err->ptr()), s, in.rule);
    }, F);
    po.img = take<ImgParams>(img, d.B);
    po.pb.init(d.B, d.maxb);
    std::memcpy(po.pb.bytes.data(), pb->out(), po.pb.bytes.size());
    po.spans = take<SpanEntry>(sp, nslot * d.span_stride);
    F.variants_ok &= take<int>(err, 1)[0] == 0;
  }
  void match(const Inputs& in, const MatchIn& m, std::vector<float>& ymean, std::vector<float>& matched) {
    const EotDims& d = in.d;
    Job j;
    const size_t pp = (size_t)d.P * d.P * 3;
    In* src = j.in_bytes(m.src, (m.stride ? pp * d.B : pp) * 4);
    In* img = j.in_bytes(m.img, d.B * sizeof(ImgParams));
    In* tgt = j.in(in.imgs);
    Guarded* om = j.out(pp * d.B * 4);
    Guarded* ys = j.out((size_t)d.B * 2 * 64 * 8);
    Guarded* ym = j.out((size_t)d.B * 2 * 4);
    j.run([&] {
      if (in.c.batch)
        launch_eot_match_batch(d, src->as<float>(), img->as<ImgParams>(), tgt->as<float>(), om->ptr(),
                               reinterpret_cast<double*>(ys->ptr()), ym->ptr(), s);
      else
        launch_eot_match(d, src->as<float>(), img->as<ImgParams>(), tgt->as<float>(), om->ptr(),
                         reinterpret_cast<double*>(ys->ptr()), ym->ptr(), in.c.apply_print != 0, s);
    }, F);
    ymean = take<float>(ym, (size_t)d.B * 2);
    matched = take<float>(om, pp * d.B);
  }
  void resize(const Inputs& in, const PlaceOut& po, const std::vector<float>& matched, std::vector<float>& rstore) {
    Job j;
    In* m = j.in(matched);
    In* pb = j.in(po.pb.bytes);
    In* sp = j.in(po.spans);
    const size_t n = (size_t)std::max(r_total(in.d, po.pb), 4L);
    Guarded* r = j.out(n * 4);
    j.run([&] {
      launch_eot_resize(in.d, m->as<float>(), pb->as<BoxPlace>(), sp->as<SpanEntry>(), in.c.seed, in.c.step, in.c.gimg0,
                        r->ptr(), s, in.c.amp);
    }, F);
    rstore = take<float>(r, n);
  }
  void composite(const Inputs& in, const PlaceOut& po, const std::vector<float>& R, std::vector<float>& out,
                 std::vector<int16_t>& owner, std::vector<float>& mask) {
    const EotDims& d = in.d;
    Job j;
    In* im = j.in(in.imgs);
    In* pb = j.in(po.pb.bytes);
    In* r = j.in(R);
    const size_t n = (size_t)d.B * d.H * d.W * 3;
    Guarded* o = j.out(n * 4);
    Guarded* ow = j.out(n * 2, 0x7f7f7f7fu);
    Guarded* mk = j.out(n * 4);
    auto go = [&](bool with_owner, bool with_mask) {
      return [&, with_owner, with_mask] {
        launch_eot_composite(d, im->as<float>(), pb->as<BoxPlace>(), r->as<float>(), o->ptr(),
                             with_owner ? reinterpret_cast<int16_t*>(ow->ptr()) : nullptr, s, with_mask ? mk->ptr() : nullptr);
      };
    };
    j.run(go(true, true), F);
    out = take<float>(o, n);
    owner = take<int16_t>(ow, n);
    mask = take<float>(mk, n);
    const std::vector<uint8_t> g_o = o->got, g_ow = ow->got, g_mk = mk->got;
    // owner null / mask null: the same image, and the absent output keeps its fill
    std::vector<uint8_t> fill_ow = ow->init, fill_mk = mk->init;
    F.variants_ok &= j.again(go(false, false), {0, 1, 2}, {g_o, fill_ow, fill_mk}, F);
    F.variants_ok &= j.again(go(true, false), {0, 1, 2}, {g_o, g_ow, fill_mk}, F);
    F.variants_ok &= j.again(go(false, true), {0, 1, 2}, {g_o, fill_ow, g_mk}, F);
    {
      V1 v1;
      F.v1_ok &= j.again(go(true, true), {0, 1, 2}, {g_o, g_ow, g_mk}, F);
    }
    for (auto& i : j.ins) F.inputs_ok &= i->same();
  }
  void rot_bwd(const Inputs& in, const PlaceOut& po, const std::vector<float>& R, const std::vector<int16_t>& owner,
               std::vector<float>& dstore) {
    Job j;
    In* dg = j.in(in.dimg);
    In* ow = j.in(owner);
    In* pb = j.in(po.pb.bytes);
    In* r = j.in(R);
    const size_t n = (size_t)std::max(r_total(in.d, po.pb), 4L);
    Guarded* o = j.out(n * 4);
    j.run([&] { launch_eot_rot_bwd(in.d, dg->as<float>(), ow->as<int16_t>(), pb->as<BoxPlace>(), r->as<float>(), o->ptr(), s); }, F);
    dstore = take<float>(o, n);
  }
  void resize_bwd(const Inputs& in, const PlaceOut& po, const std::vector<float>& dstore, std::vector<float>& tstore,
                  std::vector<float>& dmatched) {
    const EotDims& d = in.d;
    Job j;
    In* pb = j.in(po.pb.bytes);
    In* sp = j.in(po.spans);
    In* dr = j.in(dstore);
    const size_t nt = (size_t)std::max(t_total(d, po.pb), 4L), nm = (size_t)d.B * d.P * d.P * 3;
    Guarded* t = j.out(nt * 4);
    Guarded* m = j.out(nm * 4);
    auto go = [&] { launch_eot_resize_bwd(d, pb->as<BoxPlace>(), sp->as<SpanEntry>(), dr->as<float>(), t->ptr(), m->ptr(), s); };
    j.run(go, F);
    tstore = take<float>(t, nt);
    dmatched = take<float>(m, nm);
    const std::vector<uint8_t> g_t = t->got, g_m = m->got;
    {
      V1 v1;
      F.v1_ok &= j.again(go, {0, 1}, {g_t, g_m}, F);
    }
    for (auto& i : j.ins) F.inputs_ok &= i->same();
  }
  void patch_bwd(const Inputs& in, const PatchBwdIn& pi, std::vector<float>& grad) {
    const EotDims& d = in.d;
    Job j;
    const size_t pp = (size_t)d.P * d.P * 3;
    In* p = j.in(in.patch);
    In* img = j.in_bytes(pi.img, d.B * sizeof(ImgParams));
    In* ym = j.in_bytes(pi.ymean, (size_t)d.B * 2 * 4);
    In* dm = j.in_bytes(pi.dmatched, pp * d.B * 4);
    Guarded* ds = j.out((size_t)d.B * 64 * 8);
    Guarded* g = j.out(pp * 4);
    j.run([&] {
      launch_eot_patch_bwd(d, p->as<float>(), img->as<ImgParams>(), ym->as<float>(), dm->as<float>(),
                           reinterpret_cast<double*>(ds->ptr()), g->ptr(), pi.add_tv, s);
    }, F);
    grad = take<float>(g, pp);
  }
  void tv(const Inputs& in, std::vector<float>& metrics) {
    Job j;
    In* p = j.in(in.patch);
    Guarded* sc = j.out(256 * 8);
    Guarded* m = j.out(PHX_NMETRIC * 4);
    const std::vector<float> m0 = metrics0();
    std::memcpy(m->fill(), m0.data(), m0.size() * 4);
    j.run([&] { launch_tv(p->as<float>(), in.d.P, reinterpret_cast<double*>(sc->ptr()), m->ptr(), in.c.add_loss != 0, s); }, F);
    metrics = take<float>(m, PHX_NMETRIC);
  }
};

// a backend that stops after the placement (maxb beyond what composite and resize_bwd take)
template <class Backend> static Verdict run_place_only(const Inputs& in, Backend& be, StageOut& so) {
  Verdict V;
  be.place(in, so.po);
  check_place(in, so.po, V);
  return V;
}

// ---- refusals ------------------------------------------------------------------------------------
struct Refusal {
  bool threw = false, untouched = true, inputs_ok = true;
  std::string what;
};
static Refusal run_refusal(const Inputs& in) {
  Refusal r;
  const EotDims& d = in.d;
  Job j;
  auto attempt = [&](const std::function<void()>& launch) {
    for (auto& o : j.outs) o->upload();
    try {
      launch();
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
  const size_t nslot = (size_t)d.B * d.maxb;
  if (in.c.refuse == R_PLACE_129) {
    In* boxes = j.in(in.boxes);
    In* count = j.in(in.count);
    Guarded* img = j.out(d.B * sizeof(ImgParams));
    Guarded* pb = j.out(eot_place_bytes(d.B, d.maxb), 0);
    Guarded* sp = j.out(nslot * d.span_stride * sizeof(SpanEntry), 0);
    Guarded* err = j.out(4);
    set_scale(in.c.scale);
    attempt([&] {
      launch_eot_place(d, boxes->as<float>(), count->as<int>(), g_params, in.c.seed, in.c.step, in.c.gimg0,
                       reinterpret_cast<ImgParams*>(img->ptr()), reinterpret_cast<BoxPlace*>(pb->ptr()),
                       reinterpret_cast<SpanEntry*>(sp->ptr()), reinterpret_cast<int*>(err->ptr()), nullptr, in.rule);
    });
    return r;
  }
  // the placement and R by the stand-in: properly sized, valid inputs
  Sim sim;
  StageOut so;
  sim.place(in, so.po);
  so.img_used = so.po.img;
  const MatchIn m = match_in(in, so.img_used);
  sim.match(in, m, so.ymean, so.matched);
  sim.resize(in, so.po, so.matched, so.rstore);
  In* pb = j.in(so.po.pb.bytes);
  if (in.c.refuse == R_COMPOSITE_101) {
    In* im = j.in(in.imgs);
    In* R = j.in(so.rstore);
    const size_t n = (size_t)d.B * d.H * d.W * 3;
    Guarded* o = j.out(n * 4);
    Guarded* ow = j.out(n * 2);
    Guarded* mk = j.out(n * 4);
    attempt([&] {
      launch_eot_composite(d, im->as<float>(), pb->as<BoxPlace>(), R->as<float>(), o->ptr(), reinterpret_cast<int16_t*>(ow->ptr()),
                           nullptr, mk->ptr());
    });
  } else {
    In* sp = j.in(so.po.spans);
    std::vector<float> dz(so.rstore.size(), 0.25f);
    In* dr = j.in(dz);
    Guarded* t = j.out((size_t)std::max(t_total(d, so.po.pb), 4L) * 4);
    Guarded* dm = j.out((size_t)d.B * d.P * d.P * 3 * 4);
    attempt([&] { launch_eot_resize_bwd(d, pb->as<BoxPlace>(), sp->as<SpanEntry>(), dr->as<float>(), t->ptr(), dm->ptr(), nullptr); });
  }
  return r;
}

// ---- --plan --------------------------------------------------------------------------------------
static std::string j(const char* k, long v, bool first = false) {
  return std::string(first ? "\"" : ",\"") + k + "\":" + std::to_string(v);
}
static std::string jd(const char* k, double v) { return std::string(",\"") + k + "\":" + jnum(v); }
static std::string jl(const char* k, const std::vector<long>& v) {
  std::string s = std::string(",\"") + k + "\":[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
  return s + "]";
}
static std::string case_head(const Case& c, const Inputs& in) {
  return std::string("{\"case\":\"") + c.name + "\"" + j("refuse", c.refuse) + j("place_only", c.place_only) + j("B", c.B) + j("H", c.H) +
         j("W", c.W) + j("maxb", c.maxb) + j("P", c.P) + j("span_stride", in.d.span_stride) + j("defender", c.defender) +
         j("apply_print", c.apply_print) + j("batch", c.batch) + j("clipw", c.clipw) + jd("amp", c.amp) + jd("img_amp", c.img_amp) +
         j("add_tv", c.add_tv) + j("add_loss", c.add_loss) + j("plant", c.plant) + j("layout", c.layout);
}
static void print_plan(const Case& c, FILE* f) {
  const Inputs in = make_inputs(c);
  const EotDims& d = in.d;
  const EotPlanInfo pi = eot_plan_info();
  const PlaceOut po = sim_place(d, in.boxes, in.count, c.scale, c.seed, c.step, c.gimg0, in.rule);
  const BoxPlace* place = po.pb.place();
  const Lists L = po.pb.lists();
  const long nslot = po.pb.nslot();
  std::string s = case_head(c, in);
  s += j("nslot", nslot) + j("scan_passes", (nslot + 255) / 256) + j("nvalid", *L.nvalid) + j("total_chunks", *L.total_chunks) +
       j("row_tiles", L.tprefix[*L.nvalid]) + j("rows_per_tile", pi.rows_per_tile) + j("resize_grid", pi.resize_grid) +
       j("box_grid", pi.box_grid) + j("band_max_boxes", pi.band_max_boxes);
  std::vector<long> counts, img_n, band_items(8, 0);
  for (int b = 0; b < d.B; ++b) { counts.push_back(in.count[b]); img_n.push_back(L.img_n[b]); }
  long inv_small = 0, inv_big = 0, odd_nx = 0, empty_band_boxes = 0, vspan_max = 0, sq_le256 = 0, partial_chunk = 0, corners = 0,
       overlaps = 0, adj_slack_min = 1 << 20, over_p = 0;
  std::set<long> ps_set, nt_set;
  for (long sl = 0; sl < nslot; ++sl) {
    const BoxPlace& P = place[sl];
    const bool drawn = (sl % d.maxb) < in.count[sl / d.maxb];
    if (drawn && !P.valid) { inv_small += P.ps <= 2; inv_big += P.ps > d.span_stride; }
    if (!P.valid) continue;
    ps_set.insert(P.ps);
    const int nt = (P.ps + pi.rows_per_tile - 1) / pi.rows_per_tile;
    nt_set.insert(nt);
    bool any_empty = false;
    for (int x = 0; x < 8; ++x) {
      const int k = EotPlanInfo::band_tiles(P.ps, x, pi.rows_per_tile);
      band_items[x] += k;
      any_empty |= k == 0;
    }
    empty_band_boxes += any_empty;
    const SpanEntry* sp = &po.spans[sl * d.span_stride];
    odd_nx += (sp[P.ps - 1].end - sp[0].start) & 1;
    for (int i = 0; i < P.ps; ++i) vspan_max = std::max<long>(vspan_max, sp[i].end - sp[i].start);
    sq_le256 += P.ps * P.ps <= 256;
    partial_chunk += (P.ps * P.ps) % 256 != 0;
    over_p += P.ps > d.P;
    corners += (P.ymin == 0 || P.ymin + P.diag >= d.H - 1) && (P.xmin == 0 || P.xmin + P.diag >= d.W - 1);
    adj_slack_min = std::min<long>(adj_slack_min, adj_slack(sp, P.ps, d.P));
    for (long s2 = sl + 1; s2 < (sl / d.maxb + 1) * d.maxb; ++s2) {
      const BoxPlace& Q = place[s2];
      if (Q.valid && P.ymin < Q.ymin + Q.diag && Q.ymin < P.ymin + P.diag && P.xmin < Q.xmin + Q.diag && Q.xmin < P.xmin + P.diag) overlaps++;
    }
  }
  long band_wg_rounds = 0;
  for (int x = 0; x < 8; ++x) band_wg_rounds = std::max(band_wg_rounds, (band_items[x] + pi.resize_grid / 8 - 1) / (pi.resize_grid / 8));
  const long npx = (long)d.H * d.W, nwg = ((long)d.B * npx + 255) / 256;
  long unstaged = 0;
  for (long w = 0; w < nwg; ++w) {
    const long first = w * 256, last = std::min(first + 256, (long)d.B * npx) - 1;
    unstaged += first / npx != last / npx;
  }
  const long max_img_n = img_n.empty() ? 0 : *std::max_element(img_n.begin(), img_n.end());
  const long r_elems = r_total(d, po.pb), t_elems = t_total(d, po.pb);
  const long elems_rest = std::max({(long)d.B * npx * 3, (long)d.B * d.P * d.P * 3, t_elems, nslot * d.span_stride, nslot * 22});
  s += jl("counts", counts) + jl("img_n", img_n) + jl("band_items", band_items) + j("band_wg_rounds", band_wg_rounds) +
       jl("ps_set", std::vector<long>(ps_set.begin(), ps_set.end())) + jl("nt_set", std::vector<long>(nt_set.begin(), nt_set.end())) +
       j("invalid_small", inv_small) + j("invalid_big", inv_big) + j("odd_nx", odd_nx) + j("empty_band_boxes", empty_band_boxes) +
       j("vspan_max", vspan_max) + j("sq_le256", sq_le256) + j("partial_chunk", partial_chunk) + j("over_p", over_p) +
       j("corners", corners) + j("overlaps", overlaps) + j("adj_slack_min", *L.nvalid ? adj_slack_min : 0) + j("hw_mod256", npx % 256) +
       j("unstaged_wgs", unstaged) + j("max_img_n", max_img_n) + j("ballot_rounds", (max_img_n + 63) / 64) + j("r_elems", r_elems) +
       j("t_elems", t_elems) + j("elems_rest", elems_rest) + jd("margin", in.margin);
  {
    const TvTies tt = tv_ties(in.patch.data(), d.P);
    s += jl("tv_ties_v", std::vector<long>(tt.v, tt.v + 5)) + jl("tv_ties_h", std::vector<long>(tt.h, tt.h + 5)) +
         j("tv_zero_term_elems", tt.zero_term_elems) + j("check_rows_per_tile", kRowsPerTile);
  }
  // the stand-in through the same checks: the allowance share and the share of pre outside [-1, 1] by the
  // reference alone
  if (!c.refuse) {
    Sim sim;
    StageOut so;
    const Verdict V = c.place_only ? run_place_only(in, sim, so) : run_case(in, sim, so);
    s += "," + verdict_json(V) + ",\"standin_pass\":" + (V.pass() ? "true" : "false");
    if (!c.place_only) {
      // the fold's branches by the fp32 restatement: a later box's fill over a pixel an earlier box owns; covered
      // pixels beyond [-1, 1] that no box owns (clipped) and uncovered ones (not clipped)
      FoldStats fs;
      long covered_fill_over1 = 0, uncovered_over1 = 0;
      for (int b = 0; b < d.B; ++b)
        for (int y = 0; y < d.H; ++y)
          for (int x = 0; x < d.W; ++x)
            for (int ch = 0; ch < 3; ++ch) {
              const float inp = in.imgs[((((size_t)b * d.H + y) * d.W) + x) * 3 + ch];
              Gates g;
              const Px<float> p = composite_px<float>(d, so.po.pb, so.rin.data(), b, y, x, ch, inp, g, F_NONE, &fs);
              if (std::fabs(inp) > 1.0f) {
                covered_fill_over1 += p.covered && p.own < 0 && std::fabs(p.v) == 1.0f;
                uncovered_over1 += !p.covered && p.v == inp;
              }
            }
      s += j("fill_over_owned", fs.fill_over_owned) + j("covered_fill_over1", covered_fill_over1) + j("uncovered_over1", uncovered_over1);
    }
  }
  fprintf(f, "%s}\n", s.c_str());
  fflush(f);
}

// ---- main ----------------------------------------------------------------------------------------
int main(int argc, char** argv) {
  const std::vector<Case> t = table();
  if (argc > 1 && std::string(argv[1]) == "--plan") {
    for (const Case& c : t) print_plan(c, stdout);
    printf("{\"done\":true}\n");
    return 0;
  }
  const char* only = argc > 1 ? argv[1] : nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  int ran = 0;
  for (const Case& c : t) {
    if (only && c.name != only) continue;
    g_case = c.name.c_str();
    const auto c0 = std::chrono::steady_clock::now();
    const Inputs in = make_inputs(c);
    std::string s = case_head(c, in);
    bool pass = false;
    try {
      if (c.refuse) {
        const Refusal r = run_refusal(in);
        pass = r.threw && r.untouched && r.inputs_ok;
        s += std::string(",\"threw\":") + (r.threw ? "true" : "false") + ",\"untouched\":" + (r.untouched ? "true" : "false") +
             ",\"inputs_ok\":" + (r.inputs_ok ? "true" : "false") + ",\"what\":\"" + esc(r.what) + "\"";
      } else {
        Gpu gpu;
        StageOut so;
        const Verdict V = c.place_only ? run_place_only(in, gpu, so) : run_case(in, gpu, so);
        const Flags& F = gpu.F;
        const bool exact_ok = V.place_ok && F.v1_ok && F.variants_ok;
        pass = V.pass() && exact_ok && F.canary_ok && F.repeat_ok && F.inputs_ok;
        auto b = [](bool x) { return x ? "true" : "false"; };
        s += std::string(",\"threw\":false,") + verdict_json(V) + ",\"exact_ok\":" + b(exact_ok) + ",\"v1_ok\":" + b(F.v1_ok) +
             ",\"variants_ok\":" + b(F.variants_ok) + ",\"canary_ok\":" + b(F.canary_ok) + ",\"repeat_ok\":" + b(F.repeat_ok) +
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
  printf("{\"done\":true,\"cases\":%d,\"seconds\":%s}\n", ran, jnum(sec).c_str());
  return 0;
}
