// span.hpp — the per-axis span arithmetic of tf.image.resize(antialias=True) (TF's ScaleAndTranslate),
// shared by the EOT patch resize (kernels_eot.hip) and the serving preprocess (kernels_serve.hip).
// Restated in oracle/eot.py: resize_matrix.  Both users compile with FP contraction off.
#pragma once
#include "common.hpp"
#include "post.hpp"

namespace phx {

// TF ScaleAndTranslate span computation (ComputeSpansCore, triangle kernel, antialias=True,
// translate=0) for output index i of a resize input_size -> ps.
__device__ __forceinline__ void tf_span(int i, int ps, int in_size, SpanEntry* out) {
  const float scale = (float)ps / (float)in_size;
  const float inv_scale = (float)(1.0 / (double)scale);
  const float kscale = fmaxf(inv_scale, 1.0f);
  const float one_over_k = 1.0f / kscale;
  const float radius = 1.0f;
  const float sample_f = ((float)i + 0.5f) * inv_scale + (-inv_scale * 0.0f);
  long start = (long)ceilf(sample_f - radius * kscale - 0.5f);
  long end = (long)floorf(sample_f + radius * kscale - 0.5f);
  start = start < 0 ? 0 : (start > in_size - 1 ? in_size - 1 : start);
  end = (end < 0 ? 0 : (end > in_size - 1 ? in_size - 1 : end)) + 1;
  float total = 0.0f;
  for (long src = start; src < end; ++src) {
    float pos = (float)src + 0.5f - sample_f;
    float x = fabsf(pos * one_over_k);
    total += x < 1.0f ? 1.0f - x : 0.0f;
  }
  out->start = (int)start;
  out->end = (int)end;
  out->inv_total = fabsf(total) >= 1000.0f * 1.17549435e-38f ? 1.0f / total : 0.0f;
  out->sample_f = sample_f;
}

__device__ __forceinline__ float span_weight(const SpanEntry& sp, int src, float one_over_k) {
  float pos = (float)src + 0.5f - sp.sample_f;
  float x = fabsf(pos * one_over_k);
  float w = x < 1.0f ? 1.0f - x : 0.0f;
  return w * sp.inv_total;
}

// 1 / max(in_size / ps, 1) as tf_span computes it: the argument scale of span_weight
__device__ __forceinline__ float span_one_over_k(int ps, int in_size) {
  const float scale = (float)ps / (float)in_size;
  const float inv_scale = (float)(1.0 / (double)scale);
  return 1.0f / fmaxf(inv_scale, 1.0f);
}

}  // namespace phx
