// api.cpp — libphx C ABI: context lifecycle, weight management, detection and the attack step that
// strings the kernels together; the profile and debug entry points.  The executor is exec.cpp, the
// serving and data entry points are api_data.cpp.
#include "ctx.hpp"

namespace {

std::string json_escape(const std::string& s) {
  std::string o;
  for (char c : s) {
    if (c == '"' || c == '\\') o.push_back('\\');
    o.push_back(c);
  }
  return o;
}

// anchors.py:83-165 in float64, cast to float32
std::vector<float> make_anchors(const ModelConfig& mc) {
  std::vector<int> fs{mc.image_size};
  int f = mc.image_size;
  for (int l = 1; l <= mc.max_level; ++l) {
    f = (f - 1) / 2 + 1;
    fs.push_back(f);
  }
  std::vector<float> out;
  for (int level = mc.min_level; level <= mc.max_level; ++level) {
    const double stride = (double)fs[0] / (double)fs[level];
    struct C { double base_x, base_y, ax, ay; };
    std::vector<C> cs;
    for (int o = 0; o < mc.num_scales; ++o) {
      for (float ar : mc.aspect_ratios) {
        double octave = (double)o / (double)mc.num_scales;
        double base = (double)mc.anchor_scale * stride * std::pow(2.0, octave);
        double ax = std::sqrt((double)ar);
        double ay = 1.0 / ax;
        cs.push_back({base, base, ax, ay});
      }
    }
    std::vector<double> xs, ys;
    // numpy arange: start + i*step
    for (int i = 0;; ++i) {
      double v = stride / 2 + i * stride;
      if (v >= mc.image_size) break;
      xs.push_back(v);
    }
    ys = xs;
    for (double yv : ys) {
      for (double xv : xs) {
        for (const C& c : cs) {
          double sx2 = c.base_x * c.ax / 2.0, sy2 = c.base_y * c.ay / 2.0;
          out.push_back((float)(yv - sy2));
          out.push_back((float)(xv - sx2));
          out.push_back((float)(yv + sy2));
          out.push_back((float)(xv + sx2));
        }
      }
    }
  }
  return out;
}

// phx_last_error(NULL): the last failed phx_create or context-free call (phx_ingest_dims)
thread_local std::string g_create_err;

}  // namespace

int fail_global(int code, const std::string& msg) {
  g_create_err = msg;
  return code;
}

// phx_model_info: the configuration the program builder used (model.cpp get_model_config) in
// hparams_config's key names, plus the BiFPN node list (fpn_configs.py:24-72)
std::string phx_ctx::model_info() const {
  const ModelConfig& c = mc;
  std::ostringstream js;
  js.precision(9);
  auto arr3 = [&](const float* v) {
    std::ostringstream o;
    o.precision(9);
    o << "[" << v[0] << "," << v[1] << "," << v[2] << "]";
    return o.str();
  };
  js << "{\"name\":\"" << json_escape(c.name) << "\",\"backbone_name\":\"" << json_escape(c.backbone)
     << "\",\"image_size\":" << c.image_size << ",\"fpn_num_filters\":" << c.fpn_num_filters
     << ",\"fpn_cell_repeats\":" << c.fpn_cell_repeats << ",\"box_class_repeats\":" << c.box_class_repeats
     << ",\"anchor_scale\":" << c.anchor_scale << ",\"num_scales\":" << c.num_scales << ",\"aspect_ratios\":[";
  for (size_t i = 0; i < c.aspect_ratios.size(); ++i) js << (i ? "," : "") << c.aspect_ratios[i];
  js << "],\"min_level\":" << c.min_level << ",\"max_level\":" << c.max_level << ",\"act_type\":\""
     << (c.act == ACT_RELU6 ? "relu6" : c.act == ACT_SWISH ? "swish" : "none") << "\",\"fpn_weight_method\":\""
     << (c.fpn_weight_method == 1 ? "sum" : "fastattn") << "\",\"mean_rgb\":" << arr3(c.mean_rgb)
     << ",\"stddev_rgb\":" << arr3(c.stddev_rgb) << ",\"num_classes\":" << c.num_classes
     << ",\"survival_prob\":" << c.survival_prob << ",\"width_coefficient\":" << c.width_coefficient
     << ",\"depth_coefficient\":" << c.depth_coefficient << ",\"score_thresh\":" << filter_thresh
     << ",\"nms_score_thresh\":";
  // a hard NMS without a score threshold keeps everything ("score_thresh or -inf"): no JSON number
  if (std::isinf(nms_thresh)) js << "null"; else js << nms_thresh;
  js << ",\"nms_method\":\"" << (nms_hard() ? "hard" : "gaussian") << "\",\"nms_iou_thresh\":"
     << nms_params(nms_thresh).iou_thresh << ",\"nms_sigma\":" << nms.sigma << ",\"nms_max_output_size\":"
     << nms.max_output_size << ",\"post_mode\":\"" << (post_mode == PHX_POST_PER_CLASS ? "per_class" : "global")
     << "\",\"compute_dtype\":\"" << (bf16 ? "bf16" : "f32") << "\",\"fpn_nodes\":[";
  const int nlev = c.max_level - c.min_level + 1;
  std::map<int, std::vector<int>> ids;
  for (int i = 0; i < nlev; ++i) ids[c.min_level + i] = {i};
  int cnt = nlev;
  bool first = true;
  auto node = [&](int level, const std::vector<int>& in) {
    js << (first ? "" : ",") << "{\"feat_level\":" << level << ",\"inputs_offsets\":[";
    for (size_t k = 0; k < in.size(); ++k) js << (k ? "," : "") << in[k];
    js << "]}";
    first = false;
  };
  for (int i = c.max_level - 1; i >= c.min_level; --i) {
    node(i, {ids[i].back(), ids[i + 1].back()});
    ids[i].push_back(cnt++);
  }
  for (int i = c.min_level + 1; i <= c.max_level; ++i) {
    std::vector<int> in = ids[i];
    in.push_back(ids[i - 1].back());
    node(i, in);
    ids[i].push_back(cnt++);
  }
  js << "]}";
  return js.str();
}

int phx::ctx_image_size(const phx_ctx* ctx) { return ctx->mc.image_size; }
bool phx::ctx_profiling(const phx_ctx* ctx) { return ctx->prof.on; }
uint64_t phx::ctx_seed(const phx_ctx* ctx) { return ctx->seed; }
int phx::ctx_device(const phx_ctx* ctx) { return ctx->device; }
uint64_t phx::ctx_generation(const phx_ctx* ctx) {
  uint32_t f, n;
  std::memcpy(&f, &ctx->filter_thresh, 4);
  std::memcpy(&n, &ctx->nms_thresh, 4);
  // every NMS setting moves it: what a holder of first-pass results keyed on it computed is stale
  uint32_t iou, sg;
  std::memcpy(&iou, &ctx->nms.iou_thresh, 4);
  std::memcpy(&sg, &ctx->nms.sigma, 4);
  const uint64_t cfg = ((uint64_t)iou << 32 | sg) ^ ((uint64_t)ctx->nms.method << 40) ^
                       ((uint64_t)ctx->nms.max_output_size << 48);
  const uint64_t dflt = ((uint64_t)0x3f000000u) ^ ((uint64_t)PHX_NMS_GAUSSIAN << 40) ^ ((uint64_t)PHX_MAX_OUT << 48);
  return (ctx->w_ver * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)f << 32 | n) ^ ((cfg ^ dflt) * 0xD6E8FEB86659FD93ull);
}

void phx::def_first_pass(phx_ctx* ctx, const float* images, int B, int64_t step, int gimg0, float* boxes, int* count,
                    hipStream_t s, bool train, int pass, float score_thresh, float* scores, DefKeep keep) {
  if (!ctx->weights_loaded) throw std::logic_error("weights not loaded");
  if (B <= 0 || B > ctx->max_batch) throw std::out_of_range("batch exceeds max_batch");
  Exec& E = ctx->exec_for(B);
  ctx->sum_clobber(E);
  // the protege's layers are frozen (inference BN); the call's training flag still reaches its
  // drop connect (attack_detection.py:46-47, 183)
  run_forward(ctx, E, images, s, pass, step, gimg0, train, true);
  // odet_model(images, score_thresh) (attack_detection.py:96-127): an explicit threshold replaces
  // the config's for the soft-NMS only ("score_thresh or 0.001", postprocess.py:186-188), while
  // filter_valid_boxes keeps reading self.config's (:79-94)
  // (hard NMS: "score_thresh or -inf", :183)
  const float nt = score_thresh < 0.f ? ctx->nms_thresh : ctx->nms_thresh_of(score_thresh);
  run_pre_nms(ctx, E, s, 4, nt);  // person anchors only (attack_detection.py:116-121)
  run_nms(ctx, E, 4, E.nms1_boxes, E.nms1_scores, E.nms1_count, s, nt);
  const float S = (float)ctx->mc.image_size;
  def_filter(E.nms1_boxes, E.nms1_scores, E.nms1_count, B, PHX_MAX_OUT, S, S, ctx->filter_thresh, boxes, count, s,
             scores, keep);
}

// the EOT forward and the staging of caller boxes: the step's, and phx_patch_images' (api_data.cpp)
namespace phx {
void eot_forward(phx_ctx* ctx, Exec& E, const float* images, int B, const float* boxes,
                 const int32_t* count, const float* params, int64_t step, int gimg0,
                 hipStream_t s) {
  EotDims d = E.ed;
  d.B = B;
  Scope scope(ctx, "eot_fwd", 0.0, (double)B * (2.0 * PHX_NPATCH + 3.0 * d.H * d.W * 3) * 4.0, s);
  launch_eot_place(d, boxes, count, params, ctx->seed, step, gimg0, E.img, E.place, E.spans, E.err,
                   s);
  if (ctx->matcher == PHX_MATCH_HISTOGRAM)
    launch_eot_hist_match(d, params, E.img, images, E.matched, E.hpart, E.hlut, true, s);
  else
    launch_eot_match(d, params, E.img, images, E.matched, E.ysum, E.ymean, true, s);
  launch_eot_resize(d, E.matched, E.place, E.spans, ctx->seed, step, gimg0, E.rstore, s);
  launch_eot_composite(d, images, E.place, E.rstore, E.patched, E.owner, s);
}

// copy caller boxes [B,maxb,4] into the [B,100,4] slot layout of the injected-box buffers
void stage_boxes(Exec& E, const float* boxes, const int32_t* count, int B, int maxb,
                 hipStream_t s) {
  if (maxb > PHX_MAX_OUT) throw std::out_of_range("maxb > 100");
  if (maxb < PHX_MAX_OUT) PHX_HIP(hipMemsetAsync(E.inj_boxes, 0, (size_t)B * PHX_MAX_OUT * 16, s));
  PHX_HIP(hipMemcpy2DAsync(E.inj_boxes, PHX_MAX_OUT * 16, boxes, (size_t)maxb * 16,
                           (size_t)maxb * 16, B, hipMemcpyDeviceToDevice, s));
  PHX_HIP(hipMemcpyAsync(E.inj_count, count, B * sizeof(int), hipMemcpyDeviceToDevice, s));
}

}  // namespace phx

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int phx_abi_version(void) { return PHX_ABI_VERSION; }

int phx_create(const phx_config* cfg, int device, phx_ctx** out) {
  g_create_err.clear();
  if (!cfg || !out || !cfg->model_name) {
    g_create_err = "phx_create: null config, model name or output pointer";
    return PHX_EINVAL;
  }
  *out = nullptr;
  auto ctx = std::make_unique<phx_ctx>();
  try {
    if (!get_model_config(cfg->model_name, &ctx->mc)) {
      g_create_err = std::string("unknown model '") + cfg->model_name +
                     "' (efficientdet-d0..d7, efficientdet-lite0..lite4)";
      return PHX_EINVAL;
    }
    if (cfg->image_size < 0 || cfg->max_batch < 0) throw std::invalid_argument("negative image_size / max_batch");
    if (cfg->bn_mode != PHX_BN_LOCAL && cfg->bn_mode != PHX_BN_FROZEN && cfg->bn_mode != PHX_BN_SYNC)
      throw std::invalid_argument("unknown bn_mode");
    if (!(cfg->score_thresh >= 0.f && cfg->score_thresh <= 1.f)) throw std::invalid_argument("score_thresh outside [0, 1]");
    if (cfg->image_size > 0) ctx->mc.image_size = cfg->image_size;
    ctx->device = device;
    ctx->max_batch = cfg->max_batch > 0 ? cfg->max_batch : 1;
    ctx->bn_mode = cfg->bn_mode;
    if (cfg->compute_dtype != PHX_DTYPE_F32 && cfg->compute_dtype != PHX_DTYPE_BF16)
      throw std::invalid_argument("unknown compute_dtype");
    ctx->bf16 = cfg->compute_dtype == PHX_DTYPE_BF16;
    ctx->set_score_thresh(cfg->score_thresh);
    ctx->seed = cfg->seed;
    NetBuilder nb(ctx->mc, 0);
    nb.build();
    ctx->weights = nb.weights();
    ctx->wfloats = nb.weight_floats();
    std::ostringstream js;
    js << "[";
    for (size_t i = 0; i < ctx->weights.size(); ++i) {
      const WeightEntry& w = ctx->weights[i];
      js << (i ? "," : "") << "{\"name\":\"" << json_escape(w.name) << "\",\"shape\":[";
      for (size_t k = 0; k < w.shape.size(); ++k) js << (k ? "," : "") << w.shape[k];
      js << "],\"offset\":" << w.offset << ",\"kind\":\"" << w.kind << "\"}";
    }
    js << "]";
    ctx->manifest_json = js.str();
    // anchors
    int f = ctx->mc.image_size, a = 0;
    for (int l = 1; l <= ctx->mc.max_level; ++l) {
      f = (f - 1) / 2 + 1;
      if (l >= ctx->mc.min_level) a += f * f * ctx->mc.num_anchors();
    }
    ctx->A = a;
  } catch (const std::exception& e) {
    g_create_err = std::string("phx_create(") + cfg->model_name + "): " + e.what();
    return PHX_EINVAL;
  }
  *out = ctx.release();
  return PHX_OK;
}

int phx_set_allreduce(phx_ctx* ctx, phx_allreduce_fn fn, void* user) {
  if (!ctx) return PHX_EINVAL;
  ctx->ar_fn = fn;
  ctx->ar_user = user;
  return PHX_OK;
}

int phx_set_score_thresh(phx_ctx* ctx, float t) {
  if (!ctx) return PHX_EINVAL;
  if (!(t >= 0.f && t <= 1.f)) return fail(ctx, PHX_EINVAL, "score_thresh outside [0, 1]");
  PHX_TRY(ctx)
  ctx->pre_drop();
  ctx->set_score_thresh(t);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_set_nms_config(phx_ctx* ctx, const phx_nms_config* cfg) {
  if (!ctx) return PHX_EINVAL;
  if (!cfg) return fail(ctx, PHX_EINVAL, "nms_config: null config");
  if (cfg->method != PHX_NMS_GAUSSIAN && cfg->method != PHX_NMS_HARD)
    return fail(ctx, PHX_EINVAL, "nms_config: unknown method (PHX_NMS_GAUSSIAN or PHX_NMS_HARD)");
  if (cfg->max_output_size > PHX_MAX_OUT)
    return fail(ctx, PHX_EINVAL, "nms_config: max_output_size > 100 (every output array is [B,100]: its shape is part of the ABI)");
  if (cfg->max_output_size < 1) return fail(ctx, PHX_EINVAL, "nms_config: max_output_size < 1");
  if (!(cfg->iou_thresh >= 0.f && cfg->iou_thresh <= 1.f)) return fail(ctx, PHX_EINVAL, "nms_config: iou_thresh outside [0, 1]");
  if (!(cfg->sigma > 0.f) || std::isinf(cfg->sigma)) return fail(ctx, PHX_EINVAL, "nms_config: sigma must be positive and finite");
  PHX_TRY(ctx)
  ctx->pre_drop();
  ctx->set_nms_config(*cfg);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_get_nms_config(const phx_ctx* ctx, phx_nms_config* cfg) {
  if (!ctx || !cfg) return PHX_EINVAL;
  *cfg = ctx->nms;
  return PHX_OK;
}

int phx_set_box_loss(phx_ctx* ctx, int kind, float weight) {
  if (!ctx) return PHX_EINVAL;
  if (kind != PHX_BOX_LOSS_NONE && kind != PHX_BOX_LOSS_INV_DIOU)
    return fail(ctx, PHX_EINVAL, "box_loss: unknown kind (PHX_BOX_LOSS_NONE or PHX_BOX_LOSS_INV_DIOU)");
  if (!std::isfinite(weight)) return fail(ctx, PHX_EINVAL, "box_loss: the weight must be finite");
  if (kind != PHX_BOX_LOSS_NONE && ctx->bf16)
    return fail(ctx, PHX_EINVAL, "box_loss: the box-regression term runs in PHX_DTYPE_F32 contexts only");
  if (ctx->pre.pending || ctx->next.images)
    return fail(ctx, PHX_ESTATE, "box_loss: a phx_set_next prefetch is pending (run its step or withdraw it first)");
  PHX_TRY(ctx)
  if (kind != ctx->box_loss && !ctx->execs.empty()) {
    // the backward plan and the gradient arena change: drop every planned executor (after the device has
    // drained, so no queued kernel still reads its memory)
    PHX_HIP(hipSetDevice(ctx->device));
    PHX_HIP(hipDeviceSynchronize());
    ctx->last = nullptr;
    ctx->sum = phx_ctx::Sum{};
    ctx->execs.clear();
  }
  ctx->box_loss = kind;
  ctx->box_w = weight;
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_get_box_loss(const phx_ctx* ctx, int* kind, float* weight) {
  if (!ctx) return PHX_EINVAL;
  if (kind) *kind = ctx->box_loss;
  if (weight) *weight = ctx->box_w;
  return PHX_OK;
}

int phx_set_post_mode(phx_ctx* ctx, int mode) {
  if (!ctx) return PHX_EINVAL;
  if (mode != PHX_POST_GLOBAL && mode != PHX_POST_PER_CLASS)
    return fail(ctx, PHX_EINVAL, "post_mode: PHX_POST_GLOBAL or PHX_POST_PER_CLASS");
  ctx->post_mode = mode;
  return PHX_OK;
}

int phx_get_post_mode(const phx_ctx* ctx) { return ctx ? ctx->post_mode : PHX_EINVAL; }

int phx_model_info(const phx_ctx* ctx, char* buf, size_t cap, size_t* needed) {
  if (!ctx) return PHX_EINVAL;
  const std::string js = ctx->model_info();
  if (needed) *needed = js.size() + 1;
  if (buf && cap > 0) {
    size_t c = std::min(cap - 1, js.size());
    memcpy(buf, js.data(), c);
    buf[c] = 0;
  }
  return PHX_OK;
}

void phx_destroy(phx_ctx* ctx) { delete ctx; }

const char* phx_last_error(const phx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int phx_weight_manifest(const phx_ctx* ctx, char* buf, size_t cap, size_t* needed) {
  if (!ctx) return PHX_EINVAL;
  size_t n = ctx->manifest_json.size() + 1;
  if (needed) *needed = n;
  if (buf && cap > 0) {
    size_t c = std::min(cap - 1, ctx->manifest_json.size());
    memcpy(buf, ctx->manifest_json.data(), c);
    buf[c] = 0;
  }
  return PHX_OK;
}

size_t phx_weight_count(const phx_ctx* ctx) { return ctx ? ctx->wfloats : 0; }
int phx_num_anchors(const phx_ctx* ctx) { return ctx ? ctx->A : 0; }
int phx_image_size(const phx_ctx* ctx) { return ctx ? ctx->mc.image_size : 0; }

int phx_workspace_bytes(phx_ctx* ctx, int B, size_t* bytes) {
  if (!ctx || !bytes || B <= 0) return PHX_EINVAL;
  if (B > ctx->max_batch) return fail(ctx, PHX_ECAP, "batch exceeds max_batch");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  size_t tot = ctx->exec_for(B).bytes;
  for (const auto& e : ctx->execs)  // + the concurrent first pass's executor, once a step made it
    if (e->B == B && e->tag != 0) tot += e->bytes;
  // + the serving frame tables, once a serving call made them, and the prefetch's label slots, once a
  // phx_set_next made them
  *bytes = tot + ctx->srv_bytes + ctx->pre_lab_bytes;
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_load_weights(phx_ctx* ctx, const float* blob, size_t nfloats) {
  if (!ctx || !blob) return PHX_EINVAL;
  if (nfloats != ctx->wfloats) return fail(ctx, PHX_EINVAL, "weight blob size mismatch");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  ctx->pre_drop();
  if (!ctx->d_w) ctx->d_w.reset(dalloc<float>(ctx->wfloats));
  PHX_HIP(hipMemcpy(ctx->d_w.get(), blob, nfloats * sizeof(float), hipMemcpyHostToDevice));
  ++ctx->w_ver;
  // transposed copies of every 1x1 kernel: [Cout][Cin] for the forward GEMM
  std::vector<float> wt;
  ctx->wt_pairs.clear();
  for (const WeightEntry& w : ctx->weights) {
    if (w.kind != "kernel" || w.shape.size() != 4 || w.shape[0] != 1 || w.shape[1] != 1) continue;
    const int ci = w.shape[2], co = w.shape[3];
    ctx->wt_pairs.push_back({(long)w.offset, (long)wt.size()});
    size_t base = wt.size();
    wt.resize(base + (size_t)ci * co);
    for (int i = 0; i < ci; ++i)
      for (int o = 0; o < co; ++o) wt[base + (size_t)o * ci + i] = blob[w.offset + (size_t)i * co + o];
  }
  ctx->d_wt.reset(dalloc<float>(wt.size()));
  PHX_HIP(hipMemcpy(ctx->d_wt.get(), wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!ctx->d_anchors) {
    std::vector<float> an = make_anchors(ctx->mc);
    if ((int)an.size() != ctx->A * 4) throw std::runtime_error("anchor generation mismatch");
    ctx->d_anchors.reset(dalloc<float>(an.size()));
    PHX_HIP(hipMemcpy(ctx->d_anchors.get(), an.data(), an.size() * sizeof(float),
                      hipMemcpyHostToDevice));
  }
  ctx->weights_loaded = true;
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_read_weights(phx_ctx* ctx, float* blob, size_t nfloats) {
  if (!ctx || !blob || nfloats != ctx->wfloats) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->weights_loaded) throw std::logic_error("weights not loaded");
  PHX_HIP(hipDeviceSynchronize());
  PHX_HIP(hipMemcpy(blob, ctx->d_w.get(), nfloats * sizeof(float), hipMemcpyDeviceToHost));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_detect(phx_ctx* ctx, const float* images, int B, float* scores, int32_t* classes,
               float* boxes, void* stream) {
  if (!ctx || !images) return PHX_EINVAL;
  PHX_TRY(ctx)
  check_ready(ctx, B);
  hipStream_t s = (hipStream_t)stream;
  Exec& E = ctx->exec_for(B);
  ctx->sum_clobber(E);
  run_forward(ctx, E, images, s, 2, 0, 0);
  run_pre_nms(ctx, E, s);
  const long BA = (long)B * ctx->A;
  if (scores) PHX_HIP(hipMemcpyAsync(scores, E.scores, BA * 4, hipMemcpyDeviceToDevice, s));
  if (classes) PHX_HIP(hipMemcpyAsync(classes, E.classes, BA * 4, hipMemcpyDeviceToDevice, s));
  if (boxes) PHX_HIP(hipMemcpyAsync(boxes, E.boxes, BA * 16, hipMemcpyDeviceToDevice, s));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_first_pass(phx_ctx* ctx, const float* images, int B, float* ob, float* os, int32_t* oc,
                   void* stream) {
  if (!ctx || !images || !ob || !os || !oc) return PHX_EINVAL;
  PHX_TRY(ctx)
  check_ready(ctx, B);
  hipStream_t s = (hipStream_t)stream;
  Exec& E = ctx->exec_for(B);
  ctx->sum_clobber(E);
  run_forward(ctx, E, images, s, 0, 0, 0);
  run_pre_nms(ctx, E, s, 2);
  run_nms(ctx, E, 2, ob, os, oc, s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_soft_nms(phx_ctx* ctx, const float* boxes, const float* scores, const int32_t* count,
                 int B, int N, float* ob, float* os, int32_t* oc, void* stream) {
  if (!ctx || !boxes || !scores || B <= 0 || N <= 0) return PHX_EINVAL;
  PHX_TRY(ctx)
  hipStream_t s = (hipStream_t)stream;
  run_nms_candidates(ctx, boxes, scores, count, B, N, ob, os, oc, nullptr, s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

// the concurrent first pass of phx_step_grad (on unless PHX_CONC=0; read per call so a test can
// compare both orders in one process)
static bool concurrent_first_pass() {
  return env_on("PHX_CONC");
}

// the cross-step first-pass prefetch runs where a second stream is allowed: bn=local (bn=sync issues
// collectives that every rank must order alike; bn=frozen has no deferred statistics to carry), not
// in a profiled step (one stream), not under the checksum / guard diagnostics, not with PHX_CONC=0
static bool prefetch_ok(phx_ctx* ctx, const Exec& E) {
  return ctx->s2 && concurrent_first_pass() && ctx->bn_mode == PHX_BN_LOCAL && !ctx->prof.on && !E.ck_on &&
         !guard_bytes();
}

int phx_set_next(phx_ctx* ctx, const float* next_images, int B, int32_t global_image_offset) {
  if (!ctx) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (next_images) check_ready(ctx, B);
  PHX_HIP(hipSetDevice(ctx->device));
  if (next_images && !ctx->s2) {
    PHX_HIP(hipStreamCreateWithFlags(&ctx->s2, hipStreamNonBlocking));
    PHX_HIP(hipEventCreateWithFlags(&ctx->ev_pfork, hipEventDisableTiming));
    PHX_HIP(hipEventCreateWithFlags(&ctx->ev_pdone, hipEventDisableTiming));
  }
  if (next_images && !ctx->pre_lab_mem) {  // the two label slots (ctx.hpp), 2.4 KB per image each
    // (a slot is a multiple of 256 B, so every array in it keeps 16-B alignment)
    const size_t mb = (size_t)ctx->max_batch, per = (mb * PHX_MAX_OUT * 5 + mb + 63) / 64 * 64;
    float* p = dalloc<float>(2 * per);
    ctx->pre_lab_mem.reset(p);
    ctx->pre_lab_bytes = 2 * per * sizeof(float);
    for (int k = 0; k < 2; ++k, p += per)
      ctx->pre_lab[k] = phx_ctx::Labels{p, p + mb * PHX_MAX_OUT * 4, reinterpret_cast<int*>(p + mb * PHX_MAX_OUT * 5)};
  }
  ctx->next = next_images ? phx_ctx::Next{next_images, B, global_image_offset} : phx_ctx::Next{};
  // NULL also withdraws a first pass already prefetched for the next step (the caller refilled that
  // batch's buffer in place: the prefetch saw the old contents); the step then runs its own
  if (!next_images) ctx->pre_drop();
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_sync(phx_ctx* ctx, void* stream) {
  if (!ctx) return PHX_EINVAL;
  PHX_TRY(ctx)
  ctx->pre_join((hipStream_t)stream);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_step_grad(phx_ctx* ctx, const float* images, int B, const float* boxes,
                  const int32_t* count, int maxb, const float* params, int64_t step, int gimg0,
                  int add_tv, float* grad, float* metrics, void* stream) {
  if (!ctx || !images || !params || !grad || !metrics) return PHX_EINVAL;
  PHX_TRY(ctx)
  check_ready(ctx, B);
  hipStream_t s = (hipStream_t)stream;
  Exec& E = ctx->exec_for(B);
  ctx->last = &E;
  ctx->sum = phx_ctx::Sum{};
  const bool inject = boxes != nullptr;
  // a first pass the previous step prefetched for exactly this batch (phx_set_next)
  const bool use_pre = !inject && ctx->pre.pending && ctx->pre.images == images && ctx->pre.B == B &&
                       ctx->pre.step == step && ctx->pre.gimg0 == gimg0;
  ctx->pre_join(s);
  ctx->pre.pending = false;
  if (inject && !count) throw std::invalid_argument("boxes without count");
  if (inject && maxb > PHX_MAX_OUT) throw std::out_of_range("maxb > 100");
  // the metric row zeroed and the caller's boxes staged in one launch (16-B aligned boxes)
  const bool inject_k = inject && (reinterpret_cast<uintptr_t>(boxes) & 15) == 0;
  launch_step_prologue(metrics, PHX_NMETRIC, inject_k ? boxes : nullptr, count, B, maxb, E.inj_boxes,
                       E.inj_count, s);
  ck_begin(E, s);
  // Injected placement: the first pass only feeds the ASR denominator (and the moving statistics),
  // so it runs on a second stream beside the second pass and the backward, on its own executor
  // (its own activation arena).  Both passes defer their moving-statistics updates, applied in
  // pass order after the join, so every result equals the one-stream order bit for bit.  Not with
  // bn=sync: every rank must issue its collectives in one order.  PHX_CONC=0 turns it off.
  Exec* E1p = nullptr;
  if (concurrent_first_pass() && ctx->bn_mode != PHX_BN_SYNC && !ctx->s1) {
    PHX_HIP(hipStreamCreateWithFlags(&ctx->s1, hipStreamNonBlocking));
    PHX_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    PHX_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  }
  // (a profiled step runs on one stream: its per-launch-group events time each kernel alone)
  if (inject && concurrent_first_pass() && ctx->bn_mode == PHX_BN_LOCAL && !ctx->prof.on) {
    E1p = &ctx->exec_for(B, 1);
    ctx->last = &E;
  }
  const bool fork = E1p != nullptr;
  // (an error part-way leaves neither executor deferring)
  struct DeferReset {
    phx_ctx* c;
    Exec *a, *b;
    ~DeferReset() {
      c->fwd_hook = nullptr;  // never left armed (it refers to this call's frame)
      a->defer_mov = false;
      if (b) b->defer_mov = false;
    }
  } defer_reset{ctx, &E, E1p};
  // Where the side stream starts: when the second pass's forward reaches the backbone's stage 6
  // (the first op at 1/32 of the image side), so the first pass's HBM-bound early layers run beside
  // the second pass's latency-bound deep layers, BiFPN and heads rather than beside its own early
  // layers (C2 12.06 -> 11.89 ms).  PHX_FORK_FRAC: 0 = at the step start, 0 < f < 1 = after that
  // fraction of the ops (experiments).
  static const double fork_frac = [] {
    const char* e = std::getenv("PHX_FORK_FRAC");
    return e ? atof(e) : -1.0;
  }();
  auto side = [&]() {
    Exec& E1 = *E1p;
    hipStream_t s1 = ctx->s1;
    E1.defer_mov = true;
    PHX_HIP(hipEventRecord(ctx->ev_fork, s));
    PHX_HIP(hipStreamWaitEvent(s1, ctx->ev_fork, 0));
    ck_begin(E1, s1);
    run_forward(ctx, E1, images, s1, 0, step, gimg0);
    E1.defer_mov = false;
    run_pre_nms(ctx, E1, s1, 2);
    ck_note(E1, "p0 scores", E1.scores, (size_t)B * ctx->A * 4, s1);
    run_nms(ctx, E1, 2, E1.nms1_boxes, E1.nms1_scores, E1.nms1_count, s1);
    launch_count_ge(E1.nms1_scores, E1.nms1_count, B, PHX_MAX_OUT, 0.5f, metrics + PHX_M_ASR_DEN, s1);
    PHX_HIP(hipEventRecord(ctx->ev_join, s1));
  };
  if (fork) {
    E.defer_mov = true;
    if (fork_frac == 0.0) {
      side();
    } else {
      ctx->fwd_hook = side;
      if (fork_frac > 0.0) {
        ctx->fwd_hook_at = (size_t)(fork_frac * (double)E.prog.ops.size());
      } else {
        // the first op at 1/32 of the image side (the backbone's stage 6)
        ctx->fwd_hook_at = E.prog.ops.size();
        for (size_t i = 0; i < E.prog.ops.size(); ++i)
          if (E.prog.tensors[E.prog.ops[i].out].h * 32 <= ctx->mc.image_size) {
            ctx->fwd_hook_at = i;
            break;
          }
      }
    }
  }
  // the first-pass detections that place the patches: this executor's, or a prefetch's label slot
  phx_ctx::Labels lab{E.nms1_boxes, E.nms1_scores, E.nms1_count};
  int lab_slot = -1;
  if (!fork && use_pre) {
    // 1'. the prefetched first pass (side executor): its moving-statistics updates, deferred, go in
    // now — after the previous step's second pass, before this step's — and its ASR denominator
    // (the pass ran in the side executor; its detections are in a label slot of the context)
    Exec& Es = ctx->exec_for(B, 1);
    ctx->last = &E;
    lab_slot = ctx->pre.slot;
    lab = ctx->pre_lab[lab_slot];
    launch_bn_moving_apply(E.mov_tab, E.n_mov, E.mov_cmax, ctx->w(), Es.side, nullptr, s);
    launch_count_ge(lab.scores, lab.count, B, PHX_MAX_OUT, 0.5f, metrics + PHX_M_ASR_DEN, s);
  } else if (!fork) {
    // 1. first pass: clean forward, pre_nms, person/valid/threshold filter, soft-NMS
    run_forward(ctx, E, images, s, 0, step, gimg0);
    run_pre_nms(ctx, E, s, 2);
    run_nms(ctx, E, 2, E.nms1_boxes, E.nms1_scores, E.nms1_count, s);
    launch_count_ge(E.nms1_scores, E.nms1_count, B, PHX_MAX_OUT, 0.5f, metrics + PHX_M_ASR_DEN, s);
  }
  if (inject && !inject_k) stage_boxes(E, boxes, count, B, maxb, s);  // (unaligned caller boxes)
  // 2. EOT paste
  eot_forward(ctx, E, images, B, inject ? E.inj_boxes : lab.boxes, inject ? E.inj_count : lab.count, params, step,
              gimg0, s);
  launch_eot_count(E.ed, E.place, metrics, s);
  // the next batch's first pass (phx_set_next) on s2 beside this step's second pass and backward:
  // it starts once this step's own first pass and paste are done with the side executor's
  // detections, and defers its moving-statistics updates to the step that uses it
  // (consumed by this call either way: a step with caller boxes drops it)
  const phx_ctx::Next nx = ctx->next;
  ctx->next = phx_ctx::Next{};
  auto prefetch = [&]() {
      Exec& E1 = ctx->exec_for(B, 1);
      ctx->last = &E;
      // its detections go to the label slot this step did not read, so this step's stay readable after
      // it (phx_step_summary); no other entry point writes the slots
      const int slot = lab_slot == 0 ? 1 : 0;
      const phx_ctx::Labels det = ctx->pre_lab[slot];
      PHX_HIP(hipEventRecord(ctx->ev_pfork, s));
      PHX_HIP(hipStreamWaitEvent(ctx->s2, ctx->ev_pfork, 0));
      struct Defer {
        Exec& e;
        ~Defer() { e.defer_mov = false; }
      } defer{E1};
      try {
        E1.defer_mov = true;
        run_forward(ctx, E1, nx.images, ctx->s2, 0, step + 1, nx.gimg0);
        E1.defer_mov = false;
        run_pre_nms(ctx, E1, ctx->s2, 2);
        run_nms(ctx, E1, 2, det.boxes, det.scores, det.count, ctx->s2);
        PHX_HIP(hipEventRecord(ctx->ev_pdone, ctx->s2));
      } catch (...) {
        // a part-way enqueued prefetch: drain it (its side executor is shared with the injected flow's
        // concurrent pass on s1) and leave nothing pending
        (void)hipStreamSynchronize(ctx->s2);
        ctx->pre = phx_ctx::Pre{};
        throw;
      }
      ctx->pre = phx_ctx::Pre{nx.images, B, nx.gimg0, step + 1, true, slot};
  };
  if (!inject && nx.images && nx.B == B && prefetch_ok(ctx, E)) {
    // forked, like the injected flow's concurrent pass, when the second pass reaches the backbone's
    // stage 6, so its HBM-bound early layers run beside the second pass's deep layers and the
    // backward rather than beside the second pass's own early layers (PHX_PF_FORK=0: right here)
    if (!env_on("PHX_PF_FORK")) {
      prefetch();
    } else {
      ctx->fwd_hook = prefetch;
      ctx->fwd_hook_at = E.prog.ops.size();
      for (size_t i = 0; i < E.prog.ops.size(); ++i)
        if (E.prog.tensors[E.prog.ops[i].out].h * 32 <= ctx->mc.image_size) {
          ctx->fwd_hook_at = i;
          break;
        }
    }
  }
  ck_note(E, "eot patched", E.patched, (size_t)B * ctx->mc.image_size * ctx->mc.image_size * 12, s);
  // 3. second pass + loss
  run_forward(ctx, E, E.patched, s, 1, step, gimg0);
  if (ctx->fwd_hook) {
    auto h = std::move(ctx->fwd_hook);
    ctx->fwd_hook = nullptr;
    h();
  }
  E.defer_mov = false;
  run_pre_nms(ctx, E, s, 1);
  ck_note(E, "p1 scores", E.scores, (size_t)B * ctx->A * 4, s);
  ck_note(E, "p1 keep", E.keep, (size_t)B * ctx->A, s);
  // 5. ASR metric: soft-NMS over second-pass person boxes (attacker.py:203-205).  It reads the
  // pre_nms outputs only (the backward reads them too, nothing writes them until the next step),
  // so it runs on the side stream beside the backward and joins at the end of the step
  const bool side_nms = ctx->s1 != nullptr && concurrent_first_pass() && ctx->bn_mode != PHX_BN_SYNC && !ctx->prof.on;
  if (side_nms) {
    PHX_HIP(hipEventRecord(ctx->ev_fork, s));
    PHX_HIP(hipStreamWaitEvent(ctx->s1, ctx->ev_fork, 0));
    run_nms(ctx, E, 1, E.nms2_boxes, E.nms2_scores, E.nms2_count, ctx->s1);
    launch_count_ge(E.nms2_scores, E.nms2_count, B, PHX_MAX_OUT, 0.5f, metrics + PHX_M_ASR_NUM, ctx->s1);
    PHX_HIP(hipEventRecord(ctx->ev_join, ctx->s1));
  }
  launch_image_max(E.scores, E.keep, B, ctx->A, E.mraw, E.argm, E.nties, E.imax_scratch, s);
  launch_loss(E.mraw, B, params, E.dm, grad + PHX_NPATCH, metrics, s);
  ck_note(E, "image max", E.mraw, (size_t)B * 4, s);
  // the box-regression term: the kept second-pass boxes against the boxes the patches were placed by
  if (ctx->box_loss != PHX_BOX_LOSS_NONE)
    run_box_loss(ctx, E, inject ? E.inj_boxes : lab.boxes, inject ? E.inj_count : lab.count, metrics, s);
  // 4. victim data-gradient -> d(patched images)
  run_backward(ctx, E, E.patched, s);
  if (!side_nms) {
    run_nms(ctx, E, 1, E.nms2_boxes, E.nms2_scores, E.nms2_count, s);
    launch_count_ge(E.nms2_scores, E.nms2_count, B, PHX_MAX_OUT, 0.5f, metrics + PHX_M_ASR_NUM, s);
  }
  // 6. EOT backward -> d patch (+ TV)
  EotDims d = E.ed;
  d.B = B;
  const float* dimg = E.gptr(E.prog.input);
  Scope scope(ctx, "eot_bwd", 0.0, (double)B * (3.0 * PHX_NPATCH + 2.0 * d.H * d.W * 3) * 4.0, s);
  launch_eot_rot_bwd(d, dimg, E.owner, E.place, E.rstore, E.dstore, s);
  launch_eot_resize_bwd(d, E.place, E.spans, E.dstore, E.rstore, E.dmatched, s);
  if (ctx->matcher == PHX_MATCH_HISTOGRAM)
    launch_eot_hist_patch_bwd(d, params, E.img, E.hlut, E.dmatched, grad, add_tv != 0, s);
  else
    launch_eot_patch_bwd(d, params, E.img, E.ymean, E.dmatched, E.dsum, grad, add_tv != 0, s);
  launch_tv(params, PHX_PATCH_SIZE, E.tvs, metrics, add_tv != 0, s);
  ck_note(E, "grad", grad, (size_t)(PHX_NPATCH + 1) * 4, s);
  if (fork || side_nms) PHX_HIP(hipStreamWaitEvent(s, ctx->ev_join, 0));
  if (fork) launch_bn_moving_apply(E.mov_tab, E.n_mov, E.mov_cmax, ctx->w(), E1p->side, E.side, s);
  if (E.ck_on) {
    // every forward tensor once more after the join: a tensor whose hash changed after its producer
    // was overwritten later in the step (PHX_CKSUM)
    ck_post(E, 1, s);
    if (fork) ck_post(*E1p, 0, s);
  }
  if (guard_bytes()) check_guards(ctx, s);
  if (fork) ctx->sum = phx_ctx::Sum{&E, phx_ctx::Labels{E1p->nms1_boxes, E1p->nms1_scores, E1p->nms1_count}, E1p};
  else ctx->sum = phx_ctx::Sum{&E, lab, lab_slot < 0 ? &E : nullptr};
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_eval_step(phx_ctx* ctx, const float* images, int B, const float* boxes, const int32_t* count,
                  int maxb, const float* params, int64_t step, int gimg0, int add_tv, float* metrics,
                  float* out_boxes, float* out_scores, int32_t* out_count, void* stream) {
  if (!ctx || !images || !params || !metrics) return PHX_EINVAL;
  PHX_TRY(ctx)
  check_ready(ctx, B);
  hipStream_t s = (hipStream_t)stream;
  Exec& E = ctx->exec_for(B);
  ctx->last = &E;
  ctx->sum = phx_ctx::Sum{};
  PHX_HIP(hipMemsetAsync(metrics, 0, PHX_NMETRIC * sizeof(float), s));
  run_forward(ctx, E, images, s, 0, step, gimg0, false);
  run_pre_nms(ctx, E, s, 2);
  run_nms(ctx, E, 2, E.nms1_boxes, E.nms1_scores, E.nms1_count, s);
  launch_count_ge(E.nms1_scores, E.nms1_count, B, PHX_MAX_OUT, 0.5f, metrics + PHX_M_ASR_DEN, s);
  const bool inject = boxes != nullptr;
  if (inject) {
    if (!count) throw std::invalid_argument("boxes without count");
    stage_boxes(E, boxes, count, B, maxb, s);
  }
  eot_forward(ctx, E, images, B, inject ? E.inj_boxes : E.nms1_boxes, inject ? E.inj_count : E.nms1_count,
              params, step, gimg0, s);
  launch_eot_count(E.ed, E.place, metrics, s);
  run_forward(ctx, E, E.patched, s, 1, step, gimg0, false);
  run_pre_nms(ctx, E, s, 1);
  launch_image_max(E.scores, E.keep, B, ctx->A, E.mraw, E.argm, E.nties, E.imax_scratch, s);
  launch_loss(E.mraw, B, params, E.dm, E.dscale_scratch, metrics, s);
  if (ctx->box_loss != PHX_BOX_LOSS_NONE)
    run_box_loss(ctx, E, inject ? E.inj_boxes : E.nms1_boxes, inject ? E.inj_count : E.nms1_count, metrics, s);
  run_nms(ctx, E, 1, E.nms2_boxes, E.nms2_scores, E.nms2_count, s);
  launch_count_ge(E.nms2_scores, E.nms2_count, B, PHX_MAX_OUT, 0.5f, metrics + PHX_M_ASR_NUM, s);
  launch_tv(params, PHX_PATCH_SIZE, E.tvs, metrics, add_tv != 0, s);
  if (out_boxes) PHX_HIP(hipMemcpyAsync(out_boxes, E.nms2_boxes, (size_t)B * PHX_MAX_OUT * 16, hipMemcpyDeviceToDevice, s));
  if (out_scores) PHX_HIP(hipMemcpyAsync(out_scores, E.nms2_scores, (size_t)B * PHX_MAX_OUT * 4, hipMemcpyDeviceToDevice, s));
  if (out_count) PHX_HIP(hipMemcpyAsync(out_count, E.nms2_count, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  ctx->sum = phx_ctx::Sum{&E, phx_ctx::Labels{E.nms1_boxes, E.nms1_scores, E.nms1_count}, &E};
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_profile(phx_ctx* ctx, int enable) {
  if (!ctx) return PHX_EINVAL;
  ctx->prof.on = enable != 0;
  ctx->prof.recs.clear();
  ctx->prof.used = 0;
  return PHX_OK;
}

int phx_profile_report(phx_ctx* ctx, char* buf, size_t cap, size_t* needed) {
  if (!ctx) return PHX_EINVAL;
  PHX_TRY(ctx)
  // the copy call after a size query returns the string that query measured (rebuilding it could
  // print a timing differently and no longer fit the caller's buffer)
  if (buf && cap && !ctx->prof.report.empty()) {
    const std::string out = std::move(ctx->prof.report);
    ctx->prof.report.clear();
    if (needed) *needed = out.size() + 1;
    const size_t c = std::min(cap - 1, out.size());
    memcpy(buf, out.data(), c);
    buf[c] = 0;
    return PHX_OK;
  }
  // per launch group: measured time and the roofline time of its algorithmic work at the MI355X
  // peaks (HBM 8 TB/s; fp32 MFMA 157.3 TFLOP/s, bf16 2.5 PFLOP/s for bf16 GEMMs); roof = sum over
  // launches of max(hbm, mfma)
  struct Agg { long n = 0; double ms = 0, flops = 0, bytes = 0, hbm_ms = 0, mfma_ms = 0, roof_ms = 0; };
  std::map<std::string, Agg> agg;
  for (auto& r : ctx->prof.recs) {
    PHX_HIP(hipEventSynchronize(r.b));
    float ms = 0.f;
    PHX_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    Agg& a = agg[r.kind];
    a.n++;
    a.ms += ms;
    a.flops += r.flops;
    a.bytes += r.bytes;
    const double th = r.bytes / 8.0e12 * 1e3, tm = r.flops / (r.peak_tflops * 1e12) * 1e3;
    a.hbm_ms += th;
    a.mfma_ms += tm;
    a.roof_ms += std::max(th, tm);
  }
  std::ostringstream js;
  js << "{";
  bool first = true;
  for (auto& kv : agg) {
    js << (first ? "" : ",") << "\"" << kv.first << "\":{\"count\":" << kv.second.n
       << ",\"ms\":" << kv.second.ms << ",\"flops\":" << kv.second.flops
       << ",\"bytes\":" << kv.second.bytes << ",\"hbm_ms\":" << kv.second.hbm_ms
       << ",\"mfma_ms\":" << kv.second.mfma_ms << ",\"roof_ms\":" << kv.second.roof_ms << "}";
    first = false;
  }
  js << "}";
  std::string out = js.str();
  if (needed) *needed = out.size() + 1;
  if (!buf) ctx->prof.report = out;
  if (buf && cap) {
    size_t c = std::min(cap - 1, out.size());
    memcpy(buf, out.data(), c);
    buf[c] = 0;
  }
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_adam_clip(phx_ctx* ctx, float* params, const float* grad, float* m, float* v, float lr,
                  int64_t t, void* stream) {
  if (!params || !grad || !m || !v || t < 1) return PHX_EINVAL;
  PHX_TRY(ctx)
  launch_adam_clip(params, grad, m, v, PHX_NPARAM, lr, t, (hipStream_t)stream);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_debug_last_patched(phx_ctx* ctx, float* out, void* stream) {
  if (!ctx || !out || ctx->execs.empty()) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last) throw std::logic_error("no step has run");
  Exec& E = *ctx->last;
  const int S = ctx->mc.image_size;
  PHX_HIP(hipMemcpyAsync(out, E.patched, (size_t)E.B * S * S * 12, hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_debug_last_image_grad(phx_ctx* ctx, float* out, void* stream) {
  if (!ctx || !out || ctx->execs.empty()) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last) throw std::logic_error("no step has run");
  Exec& E = *ctx->last;
  const int S = ctx->mc.image_size;
  PHX_HIP(hipMemcpyAsync(out, E.gptr(E.prog.input), (size_t)E.B * S * S * 12, hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_debug_tap(phx_ctx* ctx, const char* op_name, int which, float* out, size_t nfloats, void* stream) {
  if (!ctx || !op_name || !out || ctx->execs.empty()) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last) throw std::logic_error("no step has run");
  Exec& E = *ctx->last;
  for (size_t i = 0; i < E.prog.ops.size(); ++i) {
    const Op& op = E.prog.ops[i];
    if (op.name != op_name) continue;
    const int t = (op.t == OP_BN && which == 0) ? op.in[0] : op.out;
    if (nfloats != E.prog.tensors[t].numel())
      throw std::invalid_argument("tap: size mismatch (the tensor has " + std::to_string(E.prog.tensors[t].numel()) +
                                  " elements)");
    if (which == 0 && op.t == OP_FUSE && E.fuse_folded[i])
      throw std::invalid_argument("tap: this fuse is computed on load by its depthwise conv, never stored");
    if (which == 1 && op.t == OP_DW && E.sepb[i])
      throw std::invalid_argument("tap: this depthwise output's gradient is formed in LDS by the fused "
                                  "separable-conv backward, never stored (PHX_SEPB=0 keeps it)");
    if (which == 0 && op.t == OP_DW && E.sep[i])
      throw std::invalid_argument("tap: this depthwise output feeds the fused separable conv's registers only, "
                                  "never stored (PHX_SEP=0 at victim creation keeps it)");
    if (which == 1 && op.t == OP_BN && i + 1 < E.prog.ops.size() && E.sefold[i + 1]) {
      // the BN below such an SE: its output's gradient fma(dy, s, dpool / HW) is never stored (the head of
      // its slot holds dpool); dy, s and dpool are intact after the step
      const Op& se = E.prog.ops[i + 1];
      const Tensor& tb = E.prog.tensors[op.out];
      if (!E.gptr(se.out)) throw std::invalid_argument("tap: no gradient for this tensor");
      launch_se_da(E.gptr(se.out), E.slot_c[se.slot], E.gptr(op.out), out, tb.n, tb.h * tb.w, tb.c,
                   (hipStream_t)stream);
      return PHX_OK;
    }
    const float* src = which == 0 ? E.tptr(t, nullptr) : E.gptr(op.out);
    if (!src) throw std::invalid_argument("tap: no gradient for this tensor");
    if (which == 0 && E.tbf(t)) launch_bf16_to_f32(src, out, (long)nfloats, (hipStream_t)stream);
    else PHX_HIP(hipMemcpyAsync(out, src, nfloats * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PHX_OK;
  }
  throw std::invalid_argument(std::string("tap: no op named ") + op_name);
  PHX_CATCH(ctx)
}

int phx_debug_tensor(phx_ctx* ctx, int tag, int op_index, int which, void* out, size_t nbytes, void* stream) {
  if (!ctx || !out || ctx->execs.empty()) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last) throw std::logic_error("no step has run");
  Exec* E = nullptr;
  for (auto& e : ctx->execs)
    if (e->B == ctx->last->B && e->tag == tag) E = e.get();
  if (!E) throw std::invalid_argument("tensor: no executor with this tag");
  if (op_index < 0 || op_index >= (int)E->prog.ops.size() || which < 0 || which > 2)
    throw std::invalid_argument("tensor: bad op index / which");
  const Op& op = E->prog.ops[op_index];
  const int t = which == 0 ? op.out : op.in[which - 1];
  if (t < 0 || t == E->prog.input) throw std::invalid_argument("tensor: no such arena tensor");
  const size_t nb = E->prog.tensors[t].numel() * (E->tbf(t) ? 2 : 4);
  if (nb != nbytes) throw std::invalid_argument("tensor: size mismatch (" + std::to_string(nb) + " bytes)");
  PHX_HIP(hipMemcpyAsync(out, E->tptr(t, nullptr), nb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_debug_checksums(phx_ctx* ctx, int tag, char* buf, size_t cap, size_t* needed) {
  if (!ctx || ctx->execs.empty()) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last) throw std::logic_error("no step has run");
  Exec* E = nullptr;
  for (auto& e : ctx->execs)
    if (e->B == ctx->last->B && e->tag == tag) E = e.get();
  if (!E) throw std::invalid_argument("checksums: no executor with this tag");
  std::string out;
  if (E->ck && !E->ck_names.empty()) {
    PHX_HIP(hipDeviceSynchronize());
    std::vector<unsigned long long> h(E->ck_names.size());
    PHX_HIP(hipMemcpy(h.data(), E->ck, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    char v[32];
    for (size_t i = 0; i < h.size(); ++i) {
      snprintf(v, sizeof v, "%016llx", h[i]);
      out += E->ck_names[i] + "\t" + v + "\n";
    }
  }
  if (needed) *needed = out.size() + 1;
  if (buf && cap) {
    const size_t n = std::min(cap - 1, out.size());
    memcpy(buf, out.data(), n);
    buf[n] = 0;
  }
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_debug_last_detections(phx_ctx* ctx, float* scores, int32_t* classes, float* boxes, void* stream) {
  if (!ctx || ctx->execs.empty()) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last) throw std::logic_error("no step has run");
  Exec& E = *ctx->last;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)E.B * ctx->A;
  if (scores) PHX_HIP(hipMemcpyAsync(scores, E.scores, n * 4, hipMemcpyDeviceToDevice, s));
  if (classes) PHX_HIP(hipMemcpyAsync(classes, E.classes, n * 4, hipMemcpyDeviceToDevice, s));
  if (boxes) PHX_HIP(hipMemcpyAsync(boxes, E.boxes, n * 16, hipMemcpyDeviceToDevice, s));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_debug_last_box_loss(phx_ctx* ctx, float* per_image, float* gt_max, int32_t* gt_anchor, int32_t* gt_nties,
                            void* stream) {
  if (!ctx) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last || !ctx->last->bl_valid) throw std::logic_error("no step with the box-regression term has run");
  Exec& E = *ctx->last;
  hipStream_t s = (hipStream_t)stream;
  const size_t ng = (size_t)E.B * PHX_MAX_OUT * 4;
  if (per_image) PHX_HIP(hipMemcpyAsync(per_image, E.bl_img, E.B * 4, hipMemcpyDeviceToDevice, s));
  if (gt_max) PHX_HIP(hipMemcpyAsync(gt_max, E.bl_max, ng, hipMemcpyDeviceToDevice, s));
  if (gt_anchor) PHX_HIP(hipMemcpyAsync(gt_anchor, E.bl_anchor, ng, hipMemcpyDeviceToDevice, s));
  if (gt_nties) PHX_HIP(hipMemcpyAsync(gt_nties, E.bl_nties, ng, hipMemcpyDeviceToDevice, s));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_debug_last_maxscores(phx_ctx* ctx, float* m, int32_t* anchor, void* stream) {
  if (!ctx || ctx->execs.empty()) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (!ctx->last) throw std::logic_error("no step has run");
  Exec& E = *ctx->last;
  hipStream_t s = (hipStream_t)stream;
  if (m) PHX_HIP(hipMemcpyAsync(m, E.mraw, E.B * 4, hipMemcpyDeviceToDevice, s));
  if (anchor) PHX_HIP(hipMemcpyAsync(anchor, E.argm, E.B * 4, hipMemcpyDeviceToDevice, s));
  return PHX_OK;
  PHX_CATCH(ctx)
}

}  // extern "C"
