// api_data.cpp — libphx C ABI, the serving and data entry points: phx_serve*, phx_ingest*, phx_nms_global, the
// patch-to-scene matchers, phx_persons, phx_letterbox, phx_augment, phx_adv_patch(_dev), phx_patch_images.
#include "ctx.hpp"

namespace {

// The frame table of a serving call, sized as DetectionInputProcessor does in fp32
// (dataloader.py:115-127: image_scale = min(S / h, S / w), scaled = int(side * image_scale)), and
// every argument check of phx_serve_preprocess / phx_serve.  Host arithmetic only: a refused call
// has launched nothing.  Returns the message of the first bad argument ("" = fine).
std::string serve_frames(const phx_ctx* ctx, const char* fn, const void* src, const int64_t* offsets,
                         const int32_t* dims, int B, std::vector<ServeFrame>* out) {
  const std::string who = std::string(fn) + ": ";
  if (B < 1 || B > ctx->max_batch)
    return who + "B = " + std::to_string(B) + " outside [1, max_batch = " + std::to_string(ctx->max_batch) + "]";
  if (!src) return who + "src is null";
  if (!offsets) return who + "offsets is null";
  if (!dims) return who + "dims is null";
  const int S = ctx->mc.image_size;
  if (S % 4) return who + "image_size " + std::to_string(S) + " is not a multiple of 4";
  out->resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    const int h = dims[2 * b], w = dims[2 * b + 1];
    const std::string at = who + "dims[" + std::to_string(b) + "] = " + std::to_string(h) + "x" + std::to_string(w);
    if (h < 1 || w < 1) return at + ": h and w must be >= 1";
    if (offsets[b] < 0) return who + "offsets[" + std::to_string(b) + "] is negative";
    const float sy = (float)S / (float)h, sx = (float)S / (float)w;
    const float sc = std::fmin(sy, sx);
    const int sh = (int)((float)h * sc), sw = (int)((float)w * sc);  // truncating fp32 products
    // tf.image.resize raises on an empty size
    if (sh < 1) return at + ": scaled height int(h * image_scale) is 0 at image_size " + std::to_string(S);
    if (sw < 1) return at + ": scaled width int(w * image_scale) is 0 at image_size " + std::to_string(S);
    if (sh > S || sw > S) return at + ": scaled size exceeds image_size";
    const float inv = 1.0f / sc;
    (*out)[b] = ServeFrame{offsets[b], h, w, sh, sw, inv, 0};
  }
  return "";
}

// the next slot of the frame-table ring (max_batch ServeFrame-sized rows), filled with `bytes` of rows
// and copied on `s`; the caller records srv_ev[slot] on `s` after the kernel that reads the table
const void* stage_rows(phx_ctx* ctx, const void* rows, size_t bytes, hipStream_t s, int* slot_out) {
  const size_t slot_frames = (size_t)ctx->max_batch;
  if (!ctx->srv_host) {
    const size_t n = slot_frames * phx_ctx::kSrvRing;
    void* hp = nullptr;
    PHX_HIP(hipHostMalloc(&hp, n * sizeof(ServeFrame), hipHostMallocDefault));
    ctx->srv_host = static_cast<ServeFrame*>(hp);
    ctx->srv_dev.reset(dalloc<ServeFrame>(n));
    for (hipEvent_t& e : ctx->srv_ev) PHX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->srv_bytes += n * sizeof(ServeFrame);
  }
  const int slot = ctx->srv_next;
  ctx->srv_next = (slot + 1) % phx_ctx::kSrvRing;
  if (ctx->srv_busy[slot]) PHX_HIP(hipEventSynchronize(ctx->srv_ev[slot]));  // kSrvRing calls in flight
  ctx->srv_busy[slot] = false;
  ServeFrame* h = ctx->srv_host + slot * slot_frames;
  ServeFrame* d = static_cast<ServeFrame*>(ctx->srv_dev.get()) + slot * slot_frames;
  std::memcpy(h, rows, bytes);
  PHX_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
  *slot_out = slot;
  return d;
}

const ServeFrame* serve_stage(phx_ctx* ctx, const std::vector<ServeFrame>& fr, hipStream_t s, int* slot_out) {
  return static_cast<const ServeFrame*>(stage_rows(ctx, fr.data(), fr.size() * sizeof(ServeFrame), s, slot_out));
}

// streaming.Stream.change_frame_size's destination size (streaming.py:59-62): scale = set_width / w and
// h * scale in float64, truncated; set_width 0 = no rescaling.  Returns the refusal's reason ("" = fine).
std::string ingest_size(int set_width, int h, int w, int* dh, int* dw) {
  if (h < 1 || w < 1) return "h and w must be >= 1";
  if (set_width == 0) {
    *dh = h;
    *dw = w;
    return "";
  }
  const double scale = (double)set_width / (double)w;
  const double hs = (double)h * scale;
  if (hs >= 2147483648.0) return "height int(h * (set_width / w)) exceeds the int range";
  if ((int)hs < 1) return "height int(h * (set_width / w)) is 0 (cv2.resize raises on an empty size)";
  *dh = (int)hs;
  *dw = set_width;
  return "";
}

void serve_preprocess(phx_ctx* ctx, const uint8_t* src, const std::vector<ServeFrame>& fr, float* images,
                      float* scales, hipStream_t s) {
  const int B = (int)fr.size(), S = ctx->mc.image_size;
  double bytes = 0;
  for (const ServeFrame& f : fr) bytes += (double)f.h * f.w * 3 + 12.0 * S * S;
  Scope scope(ctx, "preprocess", 0.0, bytes, s);
  int slot = 0;
  const ServeFrame* d = serve_stage(ctx, fr, s, &slot);
  launch_serve_preprocess(src, d, B, S, ctx->mc.mean_rgb, ctx->mc.stddev_rgb, images, scales, s);
  PHX_HIP(hipEventRecord(ctx->srv_ev[slot], s));
  ctx->srv_busy[slot] = true;
}

}  // namespace

// the defender's frame recovery (defender.cpp) preprocesses as phx_serve does
std::string phx::def_serve_frames(const phx_ctx* ctx, const char* fn, const void* src, const int64_t* offsets,
                                  const int32_t* dims, int B, std::vector<ServeFrame>* out) {
  return serve_frames(ctx, fn, src, offsets, dims, B, out);
}

void phx::def_serve_preprocess(phx_ctx* ctx, const uint8_t* src, const std::vector<ServeFrame>& fr, float* images,
                               float* scales, hipStream_t s) {
  serve_preprocess(ctx, src, fr, images, scales, s);
}

void phx::ctx_mean_std(const phx_ctx* ctx, float mean[3], float stdv[3]) {
  for (int c = 0; c < 3; ++c) {
    mean[c] = ctx->mc.mean_rgb[c];
    stdv[c] = ctx->mc.stddev_rgb[c];
  }
}

extern "C" {

int phx_serve_preprocess(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B,
                         float* images, float* scales, void* stream) {
  if (!ctx) return PHX_EINVAL;
  std::vector<ServeFrame> fr;
  const std::string bad = serve_frames(ctx, "serve_preprocess", src, offsets, dims, B, &fr);
  if (!bad.empty()) return fail(ctx, PHX_EINVAL, bad);
  if (!images) return fail(ctx, PHX_EINVAL, "serve_preprocess: images is null");
  if (!scales) return fail(ctx, PHX_EINVAL, "serve_preprocess: scales is null");
  if (reinterpret_cast<uintptr_t>(images) & 15)
    return fail(ctx, PHX_EINVAL, "serve_preprocess: images is not 16-byte aligned");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  serve_preprocess(ctx, src, fr, images, scales, (hipStream_t)stream);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_ingest_dims(int set_width, const int32_t* dims, int B, int32_t* out_dims) {
  if (!dims) return fail_global(PHX_EINVAL, "ingest_dims: dims is null");
  if (!out_dims) return fail_global(PHX_EINVAL, "ingest_dims: out_dims is null");
  if (B < 1) return fail_global(PHX_EINVAL, "ingest_dims: B = " + std::to_string(B) + " must be >= 1");
  if (set_width < 0)
    return fail_global(PHX_EINVAL, "ingest_dims: set_width = " + std::to_string(set_width) + " is negative");
  for (int b = 0; b < B; ++b) {
    int dh = 0, dw = 0;
    const int h = dims[2 * b], w = dims[2 * b + 1];
    const std::string why = ingest_size(set_width, h, w, &dh, &dw);
    if (!why.empty())
      return fail_global(PHX_EINVAL, "ingest_dims: dims[" + std::to_string(b) + "] = " + std::to_string(h) + "x" +
                                         std::to_string(w) + ": " + why);
    out_dims[2 * b] = dh;
    out_dims[2 * b + 1] = dw;
  }
  return PHX_OK;
}

int phx_ingest(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B, int set_width,
               int flags, uint8_t* out, const int64_t* out_offsets, void* stream) {
  if (!ctx) return PHX_EINVAL;
  // every check is host arithmetic: a refused call has launched nothing
  auto refuse = [&](int code, const std::string& msg) { return fail(ctx, code, "ingest: " + msg); };
  if (B < 1) return refuse(PHX_EINVAL, "B = " + std::to_string(B) + " must be >= 1");
  if (B > ctx->max_batch)
    return refuse(PHX_ECAP, "B = " + std::to_string(B) + " exceeds max_batch = " + std::to_string(ctx->max_batch));
  if (!src) return refuse(PHX_EINVAL, "src is null");
  if (!offsets) return refuse(PHX_EINVAL, "offsets is null");
  if (!dims) return refuse(PHX_EINVAL, "dims is null");
  if (!out) return refuse(PHX_EINVAL, "out is null");
  if (!out_offsets) return refuse(PHX_EINVAL, "out_offsets is null");
  if (set_width < 0) return refuse(PHX_EINVAL, "set_width = " + std::to_string(set_width) + " is negative");
  if (flags & ~PHX_INGEST_BGR) return refuse(PHX_EINVAL, "flags = " + std::to_string(flags) + " has an unknown bit");
  std::vector<IngestFrame> fr((size_t)B);
  struct Range {
    uintptr_t lo, hi;
  };
  std::vector<Range> rs((size_t)B), ro((size_t)B);
  long max_lanes = 0;
  double bytes = 0;
  for (int b = 0; b < B; ++b) {
    const int h = dims[2 * b], w = dims[2 * b + 1];
    const std::string at = "dims[" + std::to_string(b) + "] = " + std::to_string(h) + "x" + std::to_string(w);
    int dh = 0, dw = 0;
    const std::string why = ingest_size(set_width, h, w, &dh, &dw);
    if (!why.empty()) return refuse(PHX_EINVAL, at + ": " + why);
    if (offsets[b] < 0) return refuse(PHX_EINVAL, "offsets[" + std::to_string(b) + "] is negative");
    if (out_offsets[b] < 0) return refuse(PHX_EINVAL, "out_offsets[" + std::to_string(b) + "] is negative");
    const int64_t lanes = (int64_t)dh * ((dw + 3) / 4);
    if (lanes > (int64_t)INT32_MAX - 256) return refuse(PHX_EINVAL, at + ": the resized frame exceeds 2^31 lanes");
    // byte ranges in the address space (h * w and dh * dw are below 2^62)
    const int64_t spx = (int64_t)h * w, opx = (int64_t)dh * dw;
    const uintptr_t slo = reinterpret_cast<uintptr_t>(src) + (uintptr_t)offsets[b];
    const uintptr_t olo = reinterpret_cast<uintptr_t>(out) + (uintptr_t)out_offsets[b];
    if (spx > INT64_MAX / 3 || (uintptr_t)(spx * 3) > UINTPTR_MAX - slo || slo < (uintptr_t)offsets[b])
      return refuse(PHX_EINVAL, at + ": the frame exceeds the address range");
    if ((uintptr_t)(opx * 3) > UINTPTR_MAX - olo || olo < (uintptr_t)out_offsets[b])
      return refuse(PHX_EINVAL, at + ": the resized frame exceeds the address range");
    rs[b] = Range{slo, slo + (uintptr_t)(spx * 3)};
    ro[b] = Range{olo, olo + (uintptr_t)(opx * 3)};
    fr[b] = IngestFrame{offsets[b], out_offsets[b], h, w, dh, dw};
    max_lanes = std::max<long>(max_lanes, lanes);
    bytes += std::min((double)spx * 3, 12.0 * (double)opx) + 3.0 * (double)opx;
  }
  // the kernel reads and writes without an order between lanes: no output frame may touch a source
  // frame or another output frame
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < B; ++k) {
      if (ro[b].lo < rs[k].hi && rs[k].lo < ro[b].hi)
        return refuse(PHX_EINVAL, "out_offsets[" + std::to_string(b) + "]: the output frame overlaps source frame " +
                                      std::to_string(k));
      if (k < b && ro[b].lo < ro[k].hi && ro[k].lo < ro[b].hi)
        return refuse(PHX_EINVAL, "out_offsets[" + std::to_string(b) + "]: the output frame overlaps output frame " +
                                      std::to_string(k));
    }
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  Scope scope(ctx, "ingest", 0.0, bytes, s);
  int slot = 0;
  const void* d = stage_rows(ctx, fr.data(), fr.size() * sizeof(IngestFrame), s, &slot);
  launch_ingest(src, out, static_cast<const IngestFrame*>(d), B, max_lanes, (flags & PHX_INGEST_BGR) != 0, s);
  PHX_HIP(hipEventRecord(ctx->srv_ev[slot], s));
  ctx->srv_busy[slot] = true;
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_nms_global(phx_ctx* ctx, const float* boxes, const float* scores, const int32_t* classes,
                   const int32_t* count, int B, int N, const float* scales, float* ob, float* os, float* ocl,
                   int32_t* oc, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (B < 1 || N < 1) return fail(ctx, PHX_EINVAL, "nms_global: B and N must be >= 1");
  if (!boxes || !scores || !classes || !ob || !os || !ocl || !oc)
    return fail(ctx, PHX_EINVAL, "nms_global: null boxes, scores, classes or output pointer");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t nsel = (size_t)B * PHX_MAX_OUT;
  if (nsel > ctx->srv_sel_cap) {
    PHX_HIP(hipStreamSynchronize(s));
    ctx->srv_sel_ws.reset(dalloc<int>(nsel));
    ctx->srv_sel_cap = nsel;
  }
  int* sel = static_cast<int*>(ctx->srv_sel_ws.get());
  // nms(padded=True) on every candidate above the threshold, boxes clipped to [0, S] by the kernel
  run_nms_candidates(ctx, boxes, scores, count, B, N, ob, os, oc, sel, s);
  launch_nms_global_epilogue(sel, oc, classes, scales, B, N, PHX_MAX_OUT, ob, ocl, s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_nms_per_class(phx_ctx* ctx, const float* boxes, const float* scores, const int32_t* classes,
                      const int32_t* count, int B, int N, const float* scales, float* ob, float* os, float* ocl,
                      int32_t* oc, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (B < 1 || N < 1) return fail(ctx, PHX_EINVAL, "nms_per_class: B and N must be >= 1");
  if (!boxes || !scores || !classes || !ob || !os || !ocl || !oc)
    return fail(ctx, PHX_EINVAL, "nms_per_class: null boxes, scores, classes or output pointer");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int C = ctx->mc.num_classes;
  launch_nms_seg_per_class(boxes, scores, classes, count, B, N, C, ctx->nms_params(ctx->nms_thresh), scales, ob, os,
                           ocl, oc, seg_scratch(ctx, B, N, C, s), s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_serve(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B, float* ob,
              float* os, float* ocl, int32_t* oc, float* out_scales, void* stream) {
  if (!ctx) return PHX_EINVAL;
  std::vector<ServeFrame> fr;
  const std::string bad = serve_frames(ctx, "serve", src, offsets, dims, B, &fr);
  if (!bad.empty()) return fail(ctx, PHX_EINVAL, bad);
  if (!ob || !os || !ocl || !oc)
    return fail(ctx, PHX_EINVAL, "serve: null out_boxes, out_scores, out_classes or out_count");
  if (ctx->bf16)
    return fail(ctx, PHX_EINVAL, "serve: a PHX_DTYPE_BF16 context does not serve (fp32 contexts only)");
  PHX_TRY(ctx)
  check_ready(ctx, B);
  // a prefetched first pass (phx_set_next) holds the side executor and its deferred statistics; an
  // executor built here could evict it, and a training pass in flight on the side stream moves the
  // moving statistics this forward reads
  if (ctx->pre.pending)
    throw std::logic_error("serve: a phx_set_next prefetch is pending (run or withdraw it first)");
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  // a bn=frozen context's own executor is already planned for inference BN; the others serve from
  // one planned the same way (tag 2), so the result does not depend on bn_mode
  Exec& E = ctx->exec_for(B, ctx->batch_bn() ? 2 : 0);
  ctx->sum_clobber(E);
  const int S = ctx->mc.image_size;
  if (!E.srv_images) {  // the first serving call of this batch size reserves its buffers
    E.srv_images = E.alloc<float>((size_t)B * S * S * 3);
    E.srv_scales = E.alloc<float>(B);
    E.srv_sel = E.alloc<int>((size_t)B * PHX_MAX_OUT);
  }
  serve_preprocess(ctx, src, fr, E.srv_images, E.srv_scales, s);
  // KerasDriver builds the model with is_training_bn=False (infer_lib.py:171) and calls it with
  // training=False: inference BN, no drop connect, moving statistics untouched
  run_forward(ctx, E, E.srv_images, s, 2, 0, 0, false);
  // postprocess_global (postprocess.py:375-406): pre_nms over all classes, nms(padded=True) on every
  // anchor above the threshold, clip to [0, S], x image_scale_to_original, classes + CLASS_OFFSET
  if (ctx->post_mode == PHX_POST_PER_CLASS) {
    // postprocess_per_class (postprocess.py:470-493): pre_nms, then per_class_nms over every anchor's argmax
    // class with the frames' image_scale_to_original; no clip_boxes on this path
    run_pre_nms(ctx, E, s);
    Scope scope(ctx, "nms_per_class", 0.0, (double)E.B * ctx->A * 5.0, s);
    launch_nms_seg_per_class(E.boxes, E.scores, E.classes, nullptr, B, ctx->A, ctx->mc.num_classes,
                             ctx->nms_params(ctx->nms_thresh), E.srv_scales, ob, os, ocl, oc, seg_scratch(ctx, E), s);
  } else {
    run_pre_nms(ctx, E, s, -1);
    run_nms(ctx, E, -1, ob, os, oc, s, kNmsCtxThresh, E.srv_sel);
    launch_nms_global_epilogue(E.srv_sel, oc, E.classes, E.srv_scales, B, ctx->A, PHX_MAX_OUT, ob, ocl, s);
  }
  if (out_scales) PHX_HIP(hipMemcpyAsync(out_scales, E.srv_scales, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_persons(phx_ctx* ctx, const float* boxes, const float* scores, const float* classes, const int32_t* valid,
                int B, double min_score_thresh, float* pboxes, int32_t* pcount, float* best, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (B < 1) return fail(ctx, PHX_EINVAL, "persons: B must be >= 1");
  if (!boxes || !scores || !classes || !valid || !pboxes || !pcount || !best)
    return fail(ctx, PHX_EINVAL, "persons: null boxes, scores, classes, valid or output pointer");
  if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(pboxes)) & 15)
    return fail(ctx, PHX_EINVAL, "persons: boxes and pboxes must be 16-byte aligned");
  if (boxes == pboxes) return fail(ctx, PHX_EINVAL, "persons: boxes and pboxes alias");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  launch_persons(boxes, scores, classes, valid, B, (float)min_score_thresh, PHX_MAX_OUT, pboxes, pcount, best,
                 (hipStream_t)stream);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_brightness_match(phx_ctx* ctx, const float* src, int P, const float* tgt, int H, int W,
                         int B, float* out, void* stream) {
  if (!ctx || !src || !tgt || !out || B <= 0 || B > ctx->max_batch) return PHX_EINVAL;
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  // its own small scratch (per-image Y partial sums + means), not an executor
  const size_t need = (size_t)B * 2 * 64 * sizeof(double) + (size_t)B * 2 * sizeof(float);
  if (need > ctx->bm_cap) {
    PHX_HIP(hipStreamSynchronize(s));
    ctx->bm_ws.reset(dalloc<char>(need));
    ctx->bm_cap = need;
  }
  double* ysum = reinterpret_cast<double*>(ctx->bm_ws.get());
  float* ymean = reinterpret_cast<float*>(ysum + (size_t)B * 2 * 64);
  EotDims d{};
  d.B = B;
  d.P = P;
  d.H = H;
  d.W = W;
  d.maxb = PHX_MAX_OUT;
  d.span_stride = std::max(H, W);
  launch_eot_match(d, src, nullptr, tgt, out, ysum, ymean, false, s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_set_matcher(phx_ctx* ctx, int matcher) {
  if (!ctx) return PHX_EINVAL;
  if (matcher != PHX_MATCH_MEAN && matcher != PHX_MATCH_HISTOGRAM)
    return fail(ctx, PHX_EINVAL, "matcher must be PHX_MATCH_MEAN (0) or PHX_MATCH_HISTOGRAM (1)");
  ctx->matcher = matcher;
  return PHX_OK;
}

namespace {
// scratch of the stand-alone histogram matcher (chunk counts + lookup tables), shared with
// phx_brightness_match's
void hist_scratch(phx_ctx* ctx, int B, hipStream_t s, int** hpart, float** lut) {
  const size_t need = eot_hist_part_ints(B) * sizeof(int) + (size_t)B * 256 * sizeof(float);
  if (need > ctx->bm_cap) {
    PHX_HIP(hipStreamSynchronize(s));
    ctx->bm_ws.reset(dalloc<char>(need));
    ctx->bm_cap = need;
  }
  *hpart = reinterpret_cast<int*>(ctx->bm_ws.get());
  *lut = reinterpret_cast<float*>(*hpart + eot_hist_part_ints(B));
}
EotDims match_dims(int B, int P, int H, int W) {
  EotDims d{};
  d.B = B;
  d.P = P;
  d.H = H;
  d.W = W;
  d.maxb = PHX_MAX_OUT;
  d.span_stride = std::max(H, W);
  return d;
}
}  // namespace

int phx_histogram_match(phx_ctx* ctx, const float* src, int P, const float* tgt, int H, int W,
                        int B, float* out, void* stream) {
  if (!ctx || !src || !tgt || !out || B <= 0 || B > ctx->max_batch || P < 2 || H <= 0 || W <= 0 ||
      (long)H * W < 2)
    return PHX_EINVAL;
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  int* hpart;
  float* lut;
  hist_scratch(ctx, B, s, &hpart, &lut);
  launch_eot_hist_match(match_dims(B, P, H, W), src, nullptr, tgt, out, hpart, lut, false, s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_histogram_lut(phx_ctx* ctx, const float* src, int P, const float* tgt, int H, int W, int B,
                      int32_t* hist, float* lut, void* stream) {
  if (!ctx || !src || !tgt || !lut || B <= 0 || B > ctx->max_batch || P < 2 || H <= 0 || W <= 0 ||
      (long)H * W < 2)
    return PHX_EINVAL;
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  int* hpart;
  float* own;
  hist_scratch(ctx, B, s, &hpart, &own);
  launch_eot_hist_lut(match_dims(B, P, H, W), src, nullptr, tgt, hpart, hist, lut, false, s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_letterbox(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B,
                  const float* mean_rgb, const float* stddev_rgb, int out_h, int out_w, float* out,
                  void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (!src || !offsets || !dims || !mean_rgb || !stddev_rgb || !out || B <= 0 || out_h <= 0 || out_w <= 0)
    return fail(ctx, PHX_EINVAL, "letterbox: null pointer or empty shape");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  launch_letterbox(src, offsets, dims, B, mean_rgb, stddev_rgb, out_h, out_w, out, (hipStream_t)stream);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_augment(phx_ctx* ctx, const float* in, int B, int H, int W, int64_t step, int global_image_offset,
                float* out, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (!in || !out || B <= 0 || H <= 0 || W <= 0) return fail(ctx, PHX_EINVAL, "augment: null pointer or empty shape");
  if (in == out) return fail(ctx, PHX_EINVAL, "augment: in and out alias (the mirror reads other pixels)");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  const size_t need = augment_scratch_doubles(B) * sizeof(double);
  if (need > ctx->aug_cap) {  // first call for this batch size allocates (synchronous)
    ctx->aug_ws.reset(dalloc<char>(need));
    ctx->aug_cap = need;
  }
  launch_augment(in, out, B, H, W, ctx->seed, step, global_image_offset,
                 reinterpret_cast<double*>(ctx->aug_ws.get()), (hipStream_t)stream);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_adv_patch(phx_ctx* ctx, uint8_t* images, int B, int H, int W, const float* boxes, const int32_t* count,
                  int max_boxes, const uint8_t* patch, int patch_size, double scale, int out_h, int out_w,
                  int64_t step, int global_image_offset, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (!images || !boxes || !count || !patch || B <= 0 || H <= 0 || W <= 0 || max_boxes < 0 || patch_size <= 0 ||
      out_h <= 0 || out_w <= 0)
    return fail(ctx, PHX_EINVAL, "adv_patch: null pointer or empty shape");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int P = patch_size;
  // placements (AdversarialPatch._create, adv_patch.py:60-91), in double as Python computes them
  int rounds = 0;
  std::vector<ApBox> tab;
  for (int b = 0; b < B; ++b) {
    if (count[b] < 0 || count[b] > max_boxes) throw std::invalid_argument("adv_patch: box count out of range");
    rounds = std::max(rounds, (int)count[b]);
  }
  tab.assign((size_t)std::max(rounds, 1) * B, ApBox{0, 0, 0, 0, 0});
  std::vector<int> round_pix(std::max(rounds, 1), 0);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < count[b]; ++k) {
      const float* q = boxes + ((size_t)b * max_boxes + k) * 4;
      // float32 boxes (the detector's dtype) under numpy's promotion: h, w in float32, then float64
      const double ymin = q[0], xmin = q[1];
      const double h = (float)(q[2] - q[0]), w = (float)(q[3] - q[1]);
      const double long_side = std::max(h, w);
      const int pw = (int)(long_side * scale), ph = pw;
      if (ph < 1) throw std::invalid_argument("adv_patch: patch side below 1 pixel (cv2.resize to an empty size)");
      if (ph > H || pw > W) throw std::invalid_argument("adv_patch: patch larger than the image");
      double ymp = std::max((ymin + h / 2.0) - ph / 2.0, 0.0), xmp = std::max((xmin + w / 2.0) - pw / 2.0, 0.0);
      if (ymp + ph > H) ymp = H - ph;
      if (xmp + pw > W) xmp = W - pw;
      tab[(size_t)k * B + b] = ApBox{1, (int)ymp, (int)xmp, ph, pw};
      round_pix[k] = std::max(round_pix[k], ph * pw);
    }
  // the rescale of AdversarialPatch.rescale (adv_patch.py:93-108)
  const double sc = std::min((double)out_w / W, (double)out_h / H);
  const int sh = (int)(H * sc), sw = (int)(W * sc);
  if (sh < 1 || sw < 1) throw std::invalid_argument("adv_patch: the rescaled image is empty");
  const size_t need = (size_t)P * P * 3 + sizeof(unsigned long long) * (1 + (size_t)B) + sizeof(ApBox) * tab.size() + 64;
  if (need > ctx->ap_cap) {
    ctx->ap_ws.reset(dalloc<char>(need));
    ctx->ap_cap = need;
  }
  char* ws = static_cast<char*>(ctx->ap_ws.get());
  auto* ysum = reinterpret_cast<unsigned long long*>(ws);
  auto* ysrc = ysum + B;
  auto* dtab = reinterpret_cast<ApBox*>(ysrc + 1);
  uint8_t* printed = reinterpret_cast<uint8_t*>(dtab + tab.size());
  PHX_HIP(hipMemcpyAsync(dtab, tab.data(), sizeof(ApBox) * tab.size(), hipMemcpyHostToDevice, s));
  launch_ap_print(patch, printed, P, ysrc, s);
  for (int k = 0; k < rounds; ++k) {
    launch_ap_ysum(images, B, H, W, out_h, out_w, sh, sw, ysum, s);
    launch_ap_paste(images, B, H, W, printed, P, dtab + (size_t)k * B, round_pix[k], k, ysum, ysrc, out_h, out_w,
                    ctx->seed, step, global_image_offset, s);
  }
  // the host table must outlive its (pageable, staged) copy
  PHX_HIP(hipStreamSynchronize(s));
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_adv_patch_dev(phx_ctx* ctx, uint8_t* images, int B, int H, int W, const float* boxes, const int32_t* count,
                      int max_boxes, int rounds, const uint8_t* patch, int patch_size, double scale, int out_h,
                      int out_w, int64_t step, int global_image_offset, int32_t* status, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (!images || !boxes || !count || !patch || !status || B <= 0 || H <= 0 || W <= 0 || max_boxes < 0 ||
      patch_size <= 0 || out_h <= 0 || out_w <= 0)
    return fail(ctx, PHX_EINVAL, "adv_patch_dev: null pointer or empty shape");
  if (rounds < 0) return fail(ctx, PHX_EINVAL, "adv_patch_dev: rounds is negative");
  if ((long)B * std::max(max_boxes, rounds) > (1L << 30))
    return fail(ctx, PHX_EINVAL, "adv_patch_dev: B * max(max_boxes, rounds) exceeds 2^30");
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int P = patch_size;
  // the rescale of AdversarialPatch.rescale (adv_patch.py:93-108)
  const double sc = std::min((double)out_w / W, (double)out_h / H);
  const int sh = (int)(H * sc), sw = (int)(W * sc);
  if (sh < 1 || sw < 1) throw std::invalid_argument("adv_patch_dev: the rescaled image is empty");
  // phx_adv_patch's scratch and layout: [ysum B | ysrc 1 | table rounds x B | printed P x P x 3]
  const size_t ntab = (size_t)std::max(rounds, 1) * B;
  const size_t need = (size_t)P * P * 3 + sizeof(unsigned long long) * (1 + (size_t)B) + sizeof(ApBox) * ntab + 64;
  if (need > ctx->ap_cap) {
    PHX_HIP(hipStreamSynchronize(s));
    ctx->ap_ws.reset(dalloc<char>(need));
    ctx->ap_cap = need;
  }
  char* ws = static_cast<char*>(ctx->ap_ws.get());
  auto* ysum = reinterpret_cast<unsigned long long*>(ws);
  auto* ysrc = ysum + B;
  auto* dtab = reinterpret_cast<ApBox*>(ysrc + 1);
  uint8_t* printed = reinterpret_cast<uint8_t*>(dtab + ntab);
  PHX_HIP(hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), s));
  launch_ap_place(boxes, count, B, max_boxes, rounds, H, W, scale, dtab, status, s);
  launch_ap_print(patch, printed, P, ysrc, s);
  // a patch is square and fits the frame: no round has more than min(H, W)^2 pixels; the paste grid is
  // sized for that and a workgroup beyond its frame's ph * pw (or of a frame without a box) exits at once
  const int side = std::min(H, W);
  const int max_pix = (int)std::min<long>((long)side * side, 1L << 30);
  for (int k = 0; k < rounds; ++k) {
    launch_ap_ysum(images, B, H, W, out_h, out_w, sh, sw, ysum, s, dtab + (size_t)k * B);
    launch_ap_paste(images, B, H, W, printed, P, dtab + (size_t)k * B, max_pix, k, ysum, ysrc, out_h, out_w,
                    ctx->seed, step, global_image_offset, s);
  }
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_patch_images(phx_ctx* ctx, const float* images, int B, const float* boxes,
                     const int32_t* count, int maxb, const float* params, int64_t step,
                     int gimg0, float* out_images, float* placements, void* stream) {
  if (!ctx || !images || !boxes || !count || !params || !out_images) return PHX_EINVAL;
  PHX_TRY(ctx)
  if (B <= 0 || B > ctx->max_batch) throw std::out_of_range("batch exceeds max_batch");
  hipStream_t s = (hipStream_t)stream;
  Exec& E = ctx->exec_for(B);
  ctx->last = &E;
  ctx->sum_clobber(E);
  stage_boxes(E, boxes, count, B, maxb, s);
  eot_forward(ctx, E, images, B, E.inj_boxes, E.inj_count, params, step, gimg0, s);
  const int S = ctx->mc.image_size;
  PHX_HIP(hipMemcpyAsync(out_images, E.patched, (size_t)B * S * S * 12, hipMemcpyDeviceToDevice, s));
  if (placements) {
    std::vector<BoxPlace> hp((size_t)B * PHX_MAX_OUT);
    PHX_HIP(hipStreamSynchronize(s));
    PHX_HIP(hipMemcpy(hp.data(), E.place, hp.size() * sizeof(BoxPlace), hipMemcpyDeviceToHost));
    std::vector<float> pl((size_t)B * maxb * 8, 0.f);
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < maxb; ++k) {
        const BoxPlace& P = hp[(size_t)b * PHX_MAX_OUT + k];
        float* o = &pl[((size_t)b * maxb + k) * 8];
        o[0] = (float)P.ymin; o[1] = (float)P.xmin; o[2] = (float)P.ps; o[3] = (float)P.diag;
        o[4] = P.angle; o[5] = P.delta; o[6] = (float)P.valid; o[7] = 0.f;
      }
    PHX_HIP(hipMemcpy(placements, pl.data(), pl.size() * 4, hipMemcpyHostToDevice));
  }
  return PHX_OK;
  PHX_CATCH(ctx)
}

}  // extern "C"
