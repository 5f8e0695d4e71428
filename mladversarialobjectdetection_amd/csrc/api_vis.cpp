// api_vis.cpp — libphx C ABI: the training summaries (attacker.py:257-305): the box-drawn uint8 sample
// and the ASR-versus-threshold counts, stand-alone over caller tensors and for the last attack step.
// The defender's summary is in defender.cpp; the kernels are kernels_vis.hip.
#include "ctx.hpp"

namespace {

// "" or what is wrong with one box set of a sample call
std::string bad_box_set(const char* which, const float* boxes, const int32_t* count, int n) {
  if (!boxes) return "";
  if (!count) return std::string("count_") + which + " is null while boxes_" + which + " is given";
  if (n < 1 || n >= kVisMaxBoxes)
    return std::string("n_") + which + " = " + std::to_string(n) + " outside [1, " + std::to_string(kVisMaxBoxes - 1) + "]";
  return "";
}

std::string bad_thresholds(const float* thresholds, int T) {
  if (!thresholds) return "thresholds is null";
  if (T < 1 || T > kCurveMaxT) return "T = " + std::to_string(T) + " outside [1, " + std::to_string(kCurveMaxT) + "]";
  return "";
}

}  // namespace

extern "C" {

int phx_vis_sample(phx_ctx* ctx, const float* images, int B, int H, int W, const float* boxes_a,
                   const int32_t* count_a, int n_a, const float* boxes_b, const int32_t* count_b, int n_b,
                   uint8_t* out_u8, int64_t out_stride, int64_t out_offset, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (!images) return fail(ctx, PHX_EINVAL, "vis_sample: images is null");
  if (!out_u8) return fail(ctx, PHX_EINVAL, "vis_sample: out_u8 is null");
  if (B < 1 || H < 1 || W < 1) return fail(ctx, PHX_EINVAL, "vis_sample: B, H and W must be at least 1");
  const int64_t n = (int64_t)H * W * 3;
  if (out_offset < 0) return fail(ctx, PHX_EINVAL, "vis_sample: out_offset is negative");
  if (B > 1 && out_stride < n) return fail(ctx, PHX_EINVAL, "vis_sample: out_stride is smaller than one image (H * W * 3 bytes)");
  std::string bad = bad_box_set("a", boxes_a, count_a, n_a);
  if (bad.empty()) bad = bad_box_set("b", boxes_b, count_b, n_b);
  if (!bad.empty()) return fail(ctx, PHX_EINVAL, "vis_sample: " + bad);
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  Scope scope(ctx, "vis_sample", 0.0, (double)B * (double)n * 5.0, s);
  launch_vis_sample(images, B, H, W, boxes_a, count_a, n_a, boxes_b, count_b, n_b, ctx->mc.mean_rgb, ctx->mc.stddev_rgb,
                    out_u8, (long)out_stride, (long)out_offset, s);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_score_curve(phx_ctx* ctx, const float* scores, const int32_t* count, int B, int N, const float* thresholds,
                    int T, int32_t* out_counts, void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (!scores) return fail(ctx, PHX_EINVAL, "score_curve: scores is null");
  if (!out_counts) return fail(ctx, PHX_EINVAL, "score_curve: out_counts is null");
  if (B < 1 || N < 1) return fail(ctx, PHX_EINVAL, "score_curve: B and N must be at least 1");
  const std::string bad = bad_thresholds(thresholds, T);
  if (!bad.empty()) return fail(ctx, PHX_EINVAL, "score_curve: " + bad);
  PHX_TRY(ctx)
  PHX_HIP(hipSetDevice(ctx->device));
  launch_score_curve(scores, count, nullptr, nullptr, B, N, thresholds, T, out_counts, (hipStream_t)stream);
  return PHX_OK;
  PHX_CATCH(ctx)
}

int phx_step_summary(phx_ctx* ctx, const float* thresholds, int T, int32_t* curve_counts, uint8_t* sample_u8,
                     void* stream) {
  if (!ctx) return PHX_EINVAL;
  if (curve_counts) {
    const std::string bad = bad_thresholds(thresholds, T);
    if (!bad.empty()) return fail(ctx, PHX_EINVAL, "step_summary: " + bad);
  }
  PHX_TRY(ctx)
  if (!ctx->sum.E || !ctx->sum.det.boxes)
    throw std::logic_error("step_summary: no phx_step_grad / phx_eval_step has run on this context, or its "
                           "executor was rebuilt or reused by another call since");
  PHX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const Exec& E = *ctx->sum.E;
  const phx_ctx::Labels D = ctx->sum.det;  // where the step read its first-pass detections
  const int B = E.B, S = ctx->mc.image_size;
  if (curve_counts) {
    Scope scope(ctx, "score_curve", 0.0, 2.0 * B * PHX_MAX_OUT * 4.0, s);
    launch_score_curve(D.scores, D.count, E.nms2_scores, E.nms2_count, B, PHX_MAX_OUT, thresholds, T,
                       curve_counts, s);
  }
  if (sample_u8) {
    const long n = (long)S * S * 3;
    Scope scope(ctx, "vis_sample", 0.0, (double)B * (double)n * 5.0, s);
    launch_vis_sample(E.patched, B, S, S, D.boxes, D.count, PHX_MAX_OUT, E.nms2_boxes, E.nms2_count,
                      PHX_MAX_OUT, ctx->mc.mean_rgb, ctx->mc.stddev_rgb, sample_u8, n, 0, s);
  }
  return PHX_OK;
  PHX_CATCH(ctx)
}

}  // extern "C"
