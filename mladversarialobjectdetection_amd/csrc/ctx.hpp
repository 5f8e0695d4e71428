// ctx.hpp — internal to the library's host side (api.cpp, api_data.cpp, api_vis.cpp, exec.cpp): the context behind
// the C ABI's phx_ctx, its executors (plan + buffers), the profiler's records and launch-group scope,
// the error mapping of the C entry points, and the executor's interpreters (exec.cpp).  The defender
// does not include this: it keeps its narrow window onto the victim (unet.hpp, "victim side").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <functional>
#include <limits>
#include <vector>

#include "common.hpp"
#include "env.hpp"
#include "exec_plan.hpp"
#include "kernels.hpp"
#include "model.hpp"
#include "phx.h"
#include "boxloss.hpp"
#include "post.hpp"
#include "unet.hpp"

using namespace phx;  // (only the host files above include this header)

constexpr float kBnEps = 1e-3f;  // efficientnet_builder.py:179, util_keras.py:35

template <typename T>
T* dalloc(size_t n) {
  if (n == 0) n = 1;
  void* p = nullptr;
  PHX_HIP(hipMalloc(&p, n * sizeof(T)));
  static const bool log = env_flag("PHX_ALLOC_LOG");
  if (log) fprintf(stderr, "phx alloc %p %zu\n", p, n * sizeof(T));
  return reinterpret_cast<T*>(p);
}

// PHX_GUARD_BYTES=n (diagnostics): every executor allocation gets n guard bytes of 0xA5 after its
// end, and phx_step_grad checks them after the step (synchronising), reporting any overwrite on
// stderr — an out-of-bounds write past a buffer shows up even when it corrupts nothing visible.
// (rounded up to a multiple of 256 so every buffer keeps the 256-B alignment its 16-B vector loads
// and the GEMM planner assume; counted in Exec::bytes)
inline size_t guard_bytes() {
  static const size_t g = [] {
    const long v = env_long("PHX_GUARD_BYTES", 0);
    const size_t r = v > 0 ? ((size_t)v + 255) / 256 * 256 : 0;
    if (r) fprintf(stderr, "phx: PHX_GUARD_BYTES: %zu-byte guard bands around every executor buffer\n", r);
    return r;
  }();
  return g;
}
struct Guard {
  const char* base;
  size_t size;  // the buffer's own bytes (the guard follows)
};

struct DevFree {
  void operator()(void* p) const {
    if (p) (void)hipFree(p);
  }
};
using DPtr = std::unique_ptr<void, DevFree>;

// Per-batch-size executable state: the plan (program, fusion decisions, host tables, buffer sizes:
// exec_plan.hpp) + arenas + step buffers.
struct Exec : ExecPlan {
  explicit Exec(ExecPlan&& p) : ExecPlan(std::move(p)) {}
  std::vector<DPtr> owned;
  float* act = nullptr;
  float* grad = nullptr;
  std::vector<float*> slot_a, slot_b, slot_c;  // BN: mean,rstd ; SE: pool(+part),hidden,scale
  double* red = nullptr;                       // BN partial sums
  float* coef = nullptr;                       // BN backward coefficients
  float* se_g = nullptr;                       // SE backward scratch
  float* gpart = nullptr;                      // split-K GEMM partial slabs
  std::vector<float*> slot_d, slot_e;          // BN backward: mean(dz), mean(dz*xhat)
  // BN statistics fused into the producing kernel (StatSink): channel-major partials and their
  // row counts
  float2* spart = nullptr;
  float* scnt = nullptr;
  // written while a pass runs (state, not plan)
  std::vector<int> stat_P;                     // tensor id -> partial rows written by its producer
  std::vector<int> stat_region;                // tensor id -> region of its producer's partials
  std::vector<int> gstat_region;               // BN op id -> region of its backward partials
  std::vector<uint8_t*> pool_amax;             // op id -> max-pool argmax taps (MAXPOOL ops)
  LevelDesc* lev_dev = nullptr;
  long* dxoff_dev = nullptr;
  // pre_nms / nms / loss
  float *scores = nullptr, *boxes = nullptr;
  int* classes = nullptr;
  uint8_t* keep = nullptr;
  int* cand_list = nullptr;   // soft-NMS candidates appended by pre_nms [B][A] + counts [B]
  int* cand_count = nullptr;
  float* nms_ws = nullptr;
  float *nms1_boxes = nullptr, *nms1_scores = nullptr;
  int* nms1_count = nullptr;
  float *nms2_boxes = nullptr, *nms2_scores = nullptr;
  int* nms2_count = nullptr;
  float *mraw = nullptr, *dm = nullptr;
  int *argm = nullptr, *nties = nullptr;
  int* imax_scratch = nullptr;
  // box-regression term (phx_set_box_loss; reserved only by an executor planned with it): per (image, gt)
  // maximum, its lowest anchor and tie count [B,100], the per-image and batch values, the chunk scratch
  // and the box-predict convs' input-gradient offsets
  float *bl_max = nullptr, *bl_img = nullptr, *bl_batch = nullptr;
  int *bl_anchor = nullptr, *bl_nties = nullptr, *bl_scratch = nullptr;
  long* dxoff_box_dev = nullptr;
  const float* bl_gt = nullptr;   // the gts of the last step with the term (an executor's or a label slot's)
  const int* bl_gcount = nullptr;
  bool bl_valid = false;          // a step with the term has filled the buffers above
  // EOT
  ImgParams* img = nullptr;
  BoxPlace* place = nullptr;  // followed by the int lists
  SpanEntry* spans = nullptr;
  double* ysum = nullptr;
  float* ymean = nullptr;
  int* hpart = nullptr;  // histogram matcher: per-workgroup counts and the lookup tables [B,256]
  float* hlut = nullptr;
  float *rstore = nullptr, *dstore = nullptr;
  float *matched = nullptr, *dmatched = nullptr;
  double* dsum = nullptr;
  double* tvs = nullptr;
  int* err = nullptr;
  float* patched = nullptr;
  int16_t* owner = nullptr;
  // drop connect (non-b0 backbones, training): per drop op its block id and survival, and the
  // per-image keep flags of the current pass [ndrop][B]
  int* drop_block = nullptr;
  float* drop_p = nullptr;
  float* drop_keep = nullptr;
  // caller-injected placement boxes ([B,100,4] slot layout + counts)
  float* inj_boxes = nullptr;
  int* inj_count = nullptr;
  float* dscale_scratch = nullptr;  // dL/dscale of a gradient-free (eval) step
  // serving (phx_serve): the preprocessed batch [B,S,S,3], image_scale_to_original [B] and the
  // soft-NMS's selected anchors [B,100]; reserved by the first phx_serve of this batch size
  float *srv_images = nullptr, *srv_scales = nullptr;
  int* srv_sel = nullptr;
  // hard / per-class NMS (kernels_nms_seg.hip): reserved by the first such NMS of this batch size
  float* seg_ws = nullptr;
  double* sync_sums = nullptr;      // bn=sync: [member][C][3] per-channel sums to all-reduce

  // deferred moving statistics (a step whose first pass runs beside the second): while defer_mov
  // the BN finalizes leave the moving statistics alone and write (batch mean, variance) of their
  // slot to side + 2 * side_off[slot]; launch_bn_moving_apply then applies both passes in order
  bool defer_mov = false;
  double* side = nullptr;
  MovEntry* mov_tab = nullptr;
  double* side_for(int slot) const { return defer_mov ? side + 2 * (size_t)side_off[slot] : nullptr; }
  uint64_t frozen_ver = 0;  // ctx->w_ver whose inference-BN statistics the BN slots hold (0: none)
  size_t bytes = 0;  // device bytes owned by this executor
  uint64_t used = 0;  // phx_ctx::clock at the last use
  std::vector<Guard> guards;  // PHX_GUARD_BYTES
  // PHX_CKSUM=1 (diagnostics): a hash of every tensor / statistics slot an op writes, taken on the
  // op's stream right after it, in launch order (phx_debug_checksums)
  unsigned long long* ck = nullptr;
  size_t ck_cap = 0;
  bool ck_on = false;
  std::vector<std::string> ck_names;
  template <typename T>
  T* alloc(size_t n) {
    const size_t gb = guard_bytes();
    if (n == 0) n = 1;
    // [gb guard][buffer][gb guard] (gb a multiple of 256 keeps the buffer's alignment)
    char* q = dalloc<char>(n * sizeof(T) + 2 * gb);
    owned.emplace_back(q);
    if (gb) {
      PHX_HIP(hipMemset(q, 0xA5, gb));
      PHX_HIP(hipMemset(q + gb + n * sizeof(T), 0xA5, gb));
      guards.push_back(Guard{q + gb, n * sizeof(T)});
    }
    bytes += n * sizeof(T) + 2 * gb;
    return reinterpret_cast<T*>(q + gb);
  }
  // base pointer of tensor t (bf16 elements when tbf(t): kernels index it as such)
  float* tptr(int t, const float* input) const {
    if (t == prog.input) return const_cast<float*>(input);
    if (abf) return reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(act) + prog.tensors[t].off);
    return act + prog.tensors[t].off;
  }
  int tbf(int t) const { return abf && t != prog.input ? 1 : 0; }
  float* gptr(int t) const {
    long g = prog.tensors[t].goff;
    return g < 0 ? nullptr : grad + g;
  }
};


// Per-launch-group timing with HIP events on the launch stream (phx_profile): used by bench.py
// to time the dominant kernel live; off by default (no events on the timed path).
struct Prof {
  struct Rec {
    std::string kind;
    hipEvent_t a, b;
    double flops, bytes;
    double peak_tflops;  // the matrix-core peak the launch's FLOPs run at
  };
  bool on = false;
  std::vector<Rec> recs;
  std::string report;  // the report a size query (buf == NULL) built: the copy call returns it verbatim
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t ev() {
    if (used == pool.size()) {
      hipEvent_t e;
      PHX_HIP(hipEventCreate(&e));
      pool.push_back(e);
    }
    return pool[used++];
  }
  ~Prof() {
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

struct phx_ctx {
  Prof prof;
  ModelConfig mc;
  int device = 0;
  int max_batch = 0;
  int bn_mode = PHX_BN_LOCAL;
  // bn=sync: the caller's SUM all-reduce of the BN sums (phx_set_allreduce)
  phx_allreduce_fn ar_fn = nullptr;
  void* ar_user = nullptr;
  bool batch_bn() const { return bn_mode != PHX_BN_FROZEN; }  // training-mode batch statistics
  bool bf16 = false;  // PHX_DTYPE_BF16: bf16 matrix cores for the 1x1 convs
  // nms_configs.score_thresh: the first pass keeps scores >= filter_thresh (attacker.py:83-84);
  // gaussian soft-NMS keeps scores > nms_thresh = score_thresh or 0.001 (postprocess.py:186-188)
  float score_thresh = 0.f;
  float filter_thresh = 0.f, nms_thresh = 0.001f;
  // nms_configs' method, iou_thresh, sigma and max_output_size (phx_set_nms_config) and the post mode of
  // phx_serve (phx_set_post_mode).  postprocess.nms (postprocess.py:179-188): hard = IoU threshold
  // "iou_thresh or 0.5", score threshold "score_thresh or -inf", no decay; gaussian = IoU threshold 1,
  // "score_thresh or 0.001", soft_nms_sigma = sigma / 2
  phx_nms_config nms{PHX_NMS_GAUSSIAN, 0.f, 0.5f, PHX_MAX_OUT};
  int post_mode = PHX_POST_GLOBAL;
  bool nms_hard() const { return nms.method == PHX_NMS_HARD; }
  // the NMS score threshold of nms_configs.score_thresh == t under the method in force
  float nms_thresh_of(float t) const {
    if (t != 0.f) return t;
    return nms_hard() ? -std::numeric_limits<float>::infinity() : 0.001f;
  }
  // NonMaxSuppressionV5's parameters at NMS score threshold t
  NmsSegParams nms_params(float t) const {
    if (nms_hard()) return NmsSegParams{t, nms.iou_thresh != 0.f ? nms.iou_thresh : 0.5f, 0.f, nms.max_output_size};
    return NmsSegParams{t, 1.0f, nms.sigma * 0.5f, nms.max_output_size};
  }
  // scratch of the caller-candidate entry points under hard or per-class NMS (phx_soft_nms, phx_nms_global,
  // phx_nms_per_class), grown on demand
  DPtr seg_ws;
  size_t seg_cap = 0;
  uint64_t seed = 0;
  int matcher = PHX_MATCH_MEAN;  // phx_set_matcher: the attack's patch-to-scene matcher
  // phx_set_box_loss: loss += box_w * InverseDIOULoss()(second-pass boxes, placement boxes); kind NONE:
  // every plan, buffer and result is what it was before the term existed
  int box_loss = PHX_BOX_LOSS_NONE;
  float box_w = 1.0f;
  std::vector<WeightEntry> weights;
  size_t wfloats = 0;
  std::string manifest_json;
  DPtr d_w, d_wt;
  // version of the weights and moving statistics: bumped by every load and every training-mode
  // forward (it may update the moving statistics); an executor's inference-BN statistics computed
  // at this version are reused (Exec::frozen_ver)
  uint64_t w_ver = 1;
  std::vector<long> wt_map;  // weight offset -> offset in d_wt (dense map over kernel entries)
  std::vector<std::pair<long, long>> wt_pairs;
  bool weights_loaded = false;
  DPtr d_anchors;
  int A = 0;
  std::vector<std::unique_ptr<Exec>> execs;
  Exec* last = nullptr;
  std::string err;
  // scratch for phx_soft_nms standalone
  DPtr sn_ws;
  size_t sn_cap = 0;
  // scratch for phx_augment (per-image channel-sum partials)
  DPtr aug_ws;
  size_t aug_cap = 0;
  DPtr ap_ws;          // inference compositor scratch (phx_adv_patch)
  size_t ap_cap = 0;
  // scratch for phx_brightness_match (Y-mean partials) and phx_histogram_match / phx_histogram_lut
  // (chunk counts, lookup tables), grown on demand
  DPtr bm_ws;
  size_t bm_cap = 0;
  // serving: frame tables of the preprocess (phx_serve_preprocess / phx_serve take host offsets and
  // dims).  kSrvRing slots of max_batch frames, pinned on the host and mirrored on the device; a
  // call fills the next slot, copies it on its stream and records the slot's event after its
  // kernel, so the host waits only when kSrvRing calls are still in flight.  Reserved at the first
  // serving call; srv_sel_ws: phx_nms_global's selected indices [max_batch,100].
  static constexpr int kSrvRing = 8;
  ServeFrame* srv_host = nullptr;
  DPtr srv_dev;
  hipEvent_t srv_ev[kSrvRing] = {};
  bool srv_busy[kSrvRing] = {};
  int srv_next = 0;
  DPtr srv_sel_ws;
  size_t srv_sel_cap = 0;
  size_t srv_bytes = 0;
  // executor use clock (least-recently-used eviction, see exec_for)
  uint64_t clock = 0;

  void set_score_thresh(float t) {
    score_thresh = t;
    filter_thresh = t;
    nms_thresh = nms_thresh_of(t);
  }
  void set_nms_config(const phx_nms_config& c) {
    nms = c;
    nms_thresh = nms_thresh_of(score_thresh);
  }

  float* w() const { return reinterpret_cast<float*>(d_w.get()); }
  const float* wt_of(long off) const {
    for (auto& p : wt_pairs)
      if (p.first == off) return reinterpret_cast<const float*>(d_wt.get()) + p.second;
    throw std::runtime_error("no transposed kernel for weight offset");
  }
  Exec& exec_for(int B, int tag = 0);
  std::string model_info() const;
  // issued by run_forward once it has issued op fwd_hook_at (the second pass starts the concurrent
  // first pass part-way through its own forward, §12 of DESIGN.md)
  std::function<void()> fwd_hook;
  size_t fwd_hook_at = 0;
  // concurrent first pass (injected placement): its own stream and fork / join events
  hipStream_t s1 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // cross-step first-pass prefetch (phx_set_next, first-pass placement): the next batch's first pass
  // on s2 and the side executor (tag 1), beside the current step's second pass and backward
  hipStream_t s2 = nullptr;
  hipEvent_t ev_pfork = nullptr, ev_pdone = nullptr;
  struct Next {
    const float* images = nullptr;
    int B = 0, gimg0 = 0;
  } next;
  struct Pre {
    const float* images = nullptr;
    int B = 0, gimg0 = 0;
    int64_t step = -1;
    bool pending = false;
    int slot = 0;  // which of pre_lab's two label slots holds its detections
  } pre;
  // A prefetched first pass runs in the side executor, but its soft-NMS output (the labels the consuming
  // step places its patches by) goes to one of two label slots of the context, which no other entry
  // point writes: a step that consumes a prefetch issues the next one into the other slot, so its own
  // labels outlive the step (phx_step_summary), and a validation pass or a defender between a prefetch
  // and its consumer cannot touch them.  [max_batch,100,4] boxes + [max_batch,100] scores +
  // [max_batch] counts per slot, reserved by the first phx_set_next and counted by phx_workspace_bytes
  // from then on.
  struct Labels {
    float* boxes = nullptr;
    float* scores = nullptr;
    int* count = nullptr;
  };
  DPtr pre_lab_mem;
  Labels pre_lab[2];
  size_t pre_lab_bytes = 0;
  // phx_step_summary: the executor of the last phx_step_grad / phx_eval_step (patched batch, second-pass
  // soft-NMS output) and its first-pass detections where the step read them — a label slot, or the
  // nms1_* of det_exec; cleared by whatever overwrites that state (another victim call on an executor,
  // its eviction)
  struct Sum {
    Exec* E = nullptr;
    Labels det;
    const Exec* det_exec = nullptr;
  } sum;
  void sum_clobber(const Exec& e) {
    if (sum.E == &e || sum.det_exec == &e) sum = Sum{};
  }
  // `s` waits for a prefetch in flight (it holds the side executor and its deferred statistics)
  void pre_join(hipStream_t s) {
    if (pre.pending) PHX_HIP(hipStreamWaitEvent(s, ev_pdone, 0));
  }
  // new weights or thresholds: a prefetched first pass no longer matches what the step would compute
  void pre_drop() {
    if (pre.pending) PHX_HIP(hipStreamSynchronize(s2));
    pre = Pre{};
  }
  ~phx_ctx() {
    for (hipEvent_t e : srv_ev)
      if (e) (void)hipEventDestroy(e);
    if (srv_host) (void)hipHostFree(srv_host);
    if (s2) (void)hipStreamSynchronize(s2);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (s1) (void)hipStreamDestroy(s1);
    if (ev_pfork) (void)hipEventDestroy(ev_pfork);
    if (ev_pdone) (void)hipEventDestroy(ev_pdone);
    if (s2) (void)hipStreamDestroy(s2);
  }
};


inline int fail(phx_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}
// the same for a call without a context: the message phx_last_error(NULL) returns (api.cpp)
int fail_global(int code, const std::string& msg);

// PHX_PROF_DETAIL=1: launch groups are split by shape ("gemm fwd M=.. N=.. K=..") for tuning
inline bool prof_detail() {
  static const bool on = env_flag("PHX_PROF_DETAIL");
  return on;
}

inline std::string op_tag(const Program& P, const Op& op, bool bwd) {
  const Tensor& ti = P.tensors[op.in[0]];
  const Tensor& to = P.tensors[op.out];
  char b[160];
  if (op.t == OP_PW)
    snprintf(b, sizeof b, " %s M=%zu N=%d K=%d", bwd ? "dgrad" : "fwd", ti.rows(), bwd ? ti.c : to.c,
             bwd ? to.c : ti.c);
  else if (op.t == OP_DW)
    snprintf(b, sizeof b, " %dx%dx%d k%d s%d", ti.h, ti.w, ti.c, op.k, op.stride);
  else
    snprintf(b, sizeof b, " %dx%dx%dx%d", ti.n, ti.h, ti.w, ti.c);
  return b;
}

// PHX_DEBUG_SYNC=1: synchronise and check for a device error after every launch group, naming it
// in the exception (fault localisation; never on the timed path)
inline bool debug_sync() {
  static const bool on = env_flag("PHX_DEBUG_SYNC");
  return on;
}

struct Scope {
  Prof* p;
  size_t idx;
  hipStream_t s;
  std::string dbg;
  ExtTiming ext;  // GEMM groups: timed by the kernels' own dispatch timestamps (PHX_TLAUNCH)
  Scope(phx_ctx* ctx, const char* kind, double flops, double bytes, hipStream_t st, const std::string& tag = "")
      : p(ctx->prof.on ? &ctx->prof : nullptr), s(st) {
    if (debug_sync()) {
      dbg = std::string(kind) + tag;
      PHX_HIP(hipStreamSynchronize(s));
    }
    if (!p) return;
    // GEMMs of a bf16 context run on the bf16 matrix cores; everything else at the fp32 rate
    const double peak = (ctx->bf16 && std::string(kind) == "gemm") ? 2500.0 : 157.3;
    Prof::Rec r{std::string(kind) + (prof_detail() ? tag : std::string()), p->ev(), p->ev(), flops, bytes, peak};
    PHX_HIP(hipEventRecord(r.a, s));  // (re-recorded by the group's first timed kernel)
    p->recs.push_back(r);
    idx = p->recs.size() - 1;
    if (std::string(kind) == "gemm") {
      ext = ExtTiming{r.a, r.b, false};
      ext_timing() = &ext;
    }
  }
  ~Scope() noexcept(false) {
    if (p) {
      if (ext_timing() == &ext) ext_timing() = nullptr;
      if (!ext.used) (void)hipEventRecord(p->recs[idx].b, s);
    }
    if (!dbg.empty() && std::uncaught_exceptions() == 0) {
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) throw HipError(std::string("device error after ") + dbg + ": " + hipGetErrorString(e));
    }
  }
};

inline void check_ready(phx_ctx* ctx, int B) {
  if (!ctx->weights_loaded) throw std::logic_error("weights not loaded");
  if (B <= 0 || B > ctx->max_batch) throw std::out_of_range("batch exceeds max_batch");
}

// the C entry points map exceptions to the ABI's error codes
#define PHX_TRY(ctx)                                                           \
  try {
#define PHX_CATCH(ctx)                                                         \
  }                                                                            \
  catch (const std::out_of_range& e) { return fail(ctx, PHX_ECAP, e.what()); } \
  catch (const std::invalid_argument& e) { return fail(ctx, PHX_EINVAL, e.what()); } \
  catch (const std::logic_error& e) { return fail(ctx, PHX_ESTATE, e.what()); } \
  catch (const HipError& e) { return fail(ctx, PHX_EHIP, e.what()); }          \
  catch (const std::exception& e) { return fail(ctx, PHX_EINVAL, e.what()); }

// ---- exec.cpp: the interpreters over an executor's program ----------------------------------
namespace phx {
// victim forward over the program; pass: 0 first (clean) pass, 1 second (patched) pass, 2 standalone
// detect; train = false: inference BN and no drop connect; force_frozen: inference BN in a training pass
void run_forward(phx_ctx* ctx, Exec& E, const float* input, hipStream_t s, int pass, int64_t step, int gimg0,
                 bool train = true, bool force_frozen = false);
// data-gradient of the victim from the sparse class-logit gradient (and, in an executor planned with the
// box-regression term, the sparse box-logit gradient of the last run_box_loss)
void run_backward(phx_ctx* ctx, Exec& E, const float* input, hipStream_t s);
// the box-regression term over E's second-pass pre_nms outputs and the gts (gt [B,100,4], gcount [B]):
// values into E.bl_*, box_w * batch value added to metrics[PHX_M_LOSS]
void run_box_loss(phx_ctx* ctx, Exec& E, const float* gt, const int* gcount, float* metrics, hipStream_t s);
// nms_t of run_pre_nms / run_nms: the context's NMS score threshold (a hard NMS's may be -inf, so no
// real value can stand for it)
constexpr float kNmsCtxThresh = std::numeric_limits<float>::quiet_NaN();
void run_pre_nms(phx_ctx* ctx, Exec& E, hipStream_t s, int cand_mask = 0, float nms_t = kNmsCtxThresh);
void run_nms(phx_ctx* ctx, Exec& E, int keep_mask, float* ob, float* os, int* oc, hipStream_t s, float nms_t = kNmsCtxThresh,
             int* sel = nullptr);
float* seg_scratch(phx_ctx* ctx, Exec& E);
float* seg_scratch(phx_ctx* ctx, int B, int N, int C, hipStream_t s);
void run_nms_candidates(phx_ctx* ctx, const float* boxes, const float* scores, const int* count, int B, int N,
                        float* ob, float* os, int* oc, int* sel, hipStream_t s);
void check_guards(phx_ctx* ctx, hipStream_t s);
// PHX_CKSUM diagnostics
void ck_begin(Exec& E, hipStream_t s);
void ck_note(Exec& E, const std::string& name, const void* p, size_t bytes, hipStream_t s);
void ck_post(Exec& E, int pass, hipStream_t s);
// api.cpp: the EOT forward and the staging of caller boxes, shared by the step and phx_patch_images
void eot_forward(phx_ctx* ctx, Exec& E, const float* images, int B, const float* boxes, const int32_t* count,
                 const float* params, int64_t step, int gimg0, hipStream_t s);
void stage_boxes(Exec& E, const float* boxes, const int32_t* count, int B, int maxb, hipStream_t s);
}  // namespace phx
