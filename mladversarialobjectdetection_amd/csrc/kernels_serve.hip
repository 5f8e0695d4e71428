// kernels_serve.hip — the serving path around the detector forward (Detector.infer):
//   preprocess   EfficientDetModel._preprocessing(mode='infer') -> DetectionInputProcessor
//                (automl/efficientdet/dataloader.py:59-65 normalize_image, :115-127
//                set_scale_factors_to_output_size, :129-142 resize_and_crop_image with
//                tf.image.resize(antialias=True) + pad_to_bounding_box, :199-201 image_scale_to_original)
//   epilogue     postprocess_global's class gather and rescale (postprocess.py:375-406) after the
//                soft-NMS kernel, which has clipped the boxes to [0, S] (clip_boxes, :61-64)
//   recovery     RecoveryDemo.serve after the U-Net (demo_v2.py:159-168): add, clip, denormalise,
//                cv2.resize back to frame scale and crop (k_def_recover, below the serving kernels)
//
// k_serve_pre: one launch for a packed batch of uint8 frames of any sizes, no intermediate tensor in
// HBM.  A workgroup owns kServeRows canvas rows x 1024 consecutive canvas floats (256 lanes x one
// 16-B store per row).  It walks the source rows its canvas rows' vertical spans cover; each source
// row's bytes under the workgroup's horizontal spans are staged into LDS as normalised floats (one
// table lookup per byte, dword loads where the dword lies inside the frame), in chunks of
// kServeChunk pixels, and every lane runs the horizontal taps of its four canvas elements from LDS
// (the resized source row: a row buffer of one element per lane, kept in registers since the lane
// that produces an element is the one that consumes it), then adds the row into its canvas rows
// with the vertical weights.  Spans and weights are TF's ScaleAndTranslate (span.hpp), each axis
// with its own scaled/in ratio; tap counts are unbounded (loops, no tap arrays).  Canvas elements
// outside [scaled_h, scaled_w] are stored as 0: the kernel pads, there is no memset.
// Algorithmic bytes per frame: h*w*3 read + 12*S*S written.
#include <stdexcept>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

#include "span.hpp"

namespace phx {

constexpr int kServeRows = 4;      // canvas rows per workgroup
constexpr int kServeChunk = 1024;  // source pixels staged per pass (12 KB of floats)

struct ServePreArgs {
  const uint8_t* src;
  const ServeFrame* frames;
  float mean[3], std[3];
  int S;
  float* images;
  float* scales;
};

__global__ __launch_bounds__(256) void k_serve_pre(ServePreArgs a) {
  __shared__ float tab[3 * 256];                               // (byte - mean[c]) / std[c]
  __shared__ __attribute__((aligned(16))) float row[kServeChunk * 3 + 8];  // a staged chunk, dword-aligned
  const int t = threadIdx.x;
  const int b = blockIdx.z;
  const ServeFrame f = a.frames[b];
  const int S = a.S, h = f.h, w = f.w, sh = f.sh, sw = f.sw;
  const int i0 = blockIdx.y * kServeRows;
  if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) a.scales[b] = f.scale_to_original;
  for (int k = t; k < 3 * 256; k += 256) {
    const int c = k >> 8;
    tab[k] = ((float)(k & 255) - a.mean[c]) / a.std[c];
  }
  // this lane's four canvas elements of each row: floats e0 .. e0 + 3 of the row's S * 3
  const int e0 = (blockIdx.x * 256 + t) * 4;
  const bool lane_on = e0 < S * 3;
  SpanEntry spx[4];
  int cx[4];
  bool onx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int px = (e0 + j) / 3;
    cx[j] = (e0 + j) - px * 3;
    onx[j] = lane_on && px < sw;
    spx[j] = SpanEntry{0, 0, 0.f, 0.f};
    if (onx[j]) tf_span(px, sw, w, &spx[j]);
  }
  // the workgroup's canvas pixels [p_lo, p_hi] inside the resized image and their source columns
  const int p_lo = blockIdx.x * 1024 / 3;
  const int p_hi = min(sw - 1, (blockIdx.x * 1024 + 1023) / 3);
  // its canvas rows inside the resized image and their source rows
  const int nrow = min(kServeRows, sh - i0);  // <= 0: padding rows only
  SpanEntry spy[kServeRows];
#pragma unroll
  for (int r = 0; r < kServeRows; ++r) {
    spy[r] = SpanEntry{0, 0, 0.f, 0.f};
    if (r < nrow) tf_span(i0 + r, sh, h, &spy[r]);
  }
  float acc[kServeRows][4];
#pragma unroll
  for (int r = 0; r < kServeRows; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[r][j] = 0.f;
  __syncthreads();  // tab
  if (nrow > 0 && p_lo <= p_hi) {
    SpanEntry s0, s1;
    tf_span(p_lo, sw, w, &s0);
    tf_span(p_hi, sw, w, &s1);
    const int x_lo = s0.start, x_hi = s1.end;
    const int y_lo = spy[0].start;
    int y_hi = spy[0].end;
#pragma unroll
    for (int r = 1; r < kServeRows; ++r)
      if (r < nrow) y_hi = max(y_hi, spy[r].end);
    const float okx = span_one_over_k(sw, w), oky = span_one_over_k(sh, h);
    const uintptr_t F0 = reinterpret_cast<uintptr_t>(a.src) + (uintptr_t)f.offset;
    const uintptr_t F1 = F0 + (uintptr_t)h * w * 3;
    for (int y = y_lo; y < y_hi; ++y) {
      float hrow[4] = {0.f, 0.f, 0.f, 0.f};  // the resized source row at this lane's elements
      for (int x0 = x_lo; x0 < x_hi; x0 += kServeChunk) {
        const int n = min(kServeChunk, x_hi - x0);
        // bytes [A, A + 3n) of the frame, staged from the dword boundary A4 <= A
        const uintptr_t A = F0 + ((uintptr_t)y * w + x0) * 3;
        const uintptr_t A4 = A & ~(uintptr_t)3;
        const int lead = (int)(A - A4);
        const int nwords = (lead + 3 * n + 3) >> 2;
        __syncthreads();  // the previous chunk has been read
        for (int k = t; k < nwords; k += 256) {
          const uintptr_t W = A4 + 4 * (uintptr_t)k;
          // element q of the staged run is byte W + m; its channel is (q - lead) mod 3
          int c = (4 * k - lead) % 3;
          if (c < 0) c += 3;
          float v[4];
          if (W >= F0 && W + 4 <= F1) {
            const uint32_t word = *reinterpret_cast<const uint32_t*>(W);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              v[m] = tab[c * 256 + ((word >> (8 * m)) & 255u)];
              c = c == 2 ? 0 : c + 1;
            }
          } else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              const uintptr_t p = W + m;
              v[m] = (p >= F0 && p < F1) ? tab[c * 256 + *reinterpret_cast<const uint8_t*>(p)] : 0.f;
              c = c == 2 ? 0 : c + 1;
            }
          }
          *reinterpret_cast<float4*>(&row[4 * k]) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!onx[j]) continue;
          const int xa = max(spx[j].start, x0), xb = min(spx[j].end, x0 + n);
          for (int x = xa; x < xb; ++x)
            hrow[j] += span_weight(spx[j], x, okx) * row[lead + (x - x0) * 3 + cx[j]];
        }
      }
#pragma unroll
      for (int r = 0; r < kServeRows; ++r) {
        if (r < nrow && y >= spy[r].start && y < spy[r].end) {
          const float wy = span_weight(spy[r], y, oky);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[r][j] += wy * hrow[j];
        }
      }
    }
  }
  if (!lane_on) return;
#pragma unroll
  for (int r = 0; r < kServeRows; ++r) {
    const int i = i0 + r;
    if (i < S)
      *reinterpret_cast<float4*>(a.images + ((long)b * S + i) * S * 3 + e0) =
          make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
  }
}

void launch_serve_preprocess(const uint8_t* src, const ServeFrame* frames_dev, int B, int S, const float* mean,
                             const float* stdv, float* images, float* scales, hipStream_t s) {
  if ((S * 3) % 4) throw std::invalid_argument("serve_preprocess: image_size must be a multiple of 4");
  ServePreArgs a;
  a.src = src;
  a.frames = frames_dev;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean[c];
    a.std[c] = stdv[c];
  }
  a.S = S;
  a.images = images;
  a.scales = scales;
  const dim3 grid((S * 3 + 1023) / 1024, (S + kServeRows - 1) / kServeRows, B);
  hipLaunchKernelGGL(k_serve_pre, grid, dim3(256), 0, s, a);
  PHX_LAUNCH_CHECK();
}

// classes = argmax + CLASS_OFFSET as float32 (postprocess.py:30, :402), boxes x image_scale_to_original
// after the soft-NMS kernel's clip (:396-400); rows at and beyond the count are zero
__global__ __launch_bounds__(128) void k_nms_global_epilogue(const int* __restrict__ sel, const int* __restrict__ count,
                                                             const int* __restrict__ classes,
                                                             const float* __restrict__ scales, int N, int max_out,
                                                             float* __restrict__ boxes, float* __restrict__ out_classes) {
  const int b = blockIdx.x;
  const int n = count[b];
  const float sc = scales ? scales[b] : 1.0f;
  for (int k = threadIdx.x; k < max_out; k += blockDim.x) {
    const long o = (long)b * max_out + k;
    if (k < n) {
      const int a = min(max(sel[o], 0), N - 1);
      out_classes[o] = (float)(classes[(long)b * N + a] + 1);
      if (scales) {
#pragma unroll
        for (int q = 0; q < 4; ++q) boxes[o * 4 + q] = boxes[o * 4 + q] * sc;
      }
    } else {
      out_classes[o] = 0.f;
    }
  }
}

void launch_nms_global_epilogue(const int* sel, const int* count, const int* classes, const float* scales, int B,
                                int N, int max_out, float* boxes, float* out_classes, hipStream_t s) {
  hipLaunchKernelGGL(k_nms_global_epilogue, dim3(B), dim3(128), 0, s, sel, count, classes, scales, N, max_out, boxes,
                     out_classes);
  PHX_LAUNCH_CHECK();
}

// ---- person selector (detector.py:48-57, util.py:163-174, demo.py:81) --------------------------------
// k_persons: one wave per frame over phx_serve's 100 rows, in two passes of 64.  A row is a person when
// it lies below valid[b] and its class is 1; it is kept when its score >= thresh (fp32).  The kept
// rows' output slot is the number of kept rows before it: the popcount of the ballot's lower lanes plus
// the first pass's total, so the order is the NMS order and nothing depends on timing (no atomics).
// best[b] = the maximum score of every person row, kept or not (a butterfly max), 0 without one.
// Rows of pboxes at and beyond the count are zeroed by the same wave.  Latency-trivial: 2.4 KB per frame.
__global__ __launch_bounds__(64) void k_persons(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                const float* __restrict__ classes, const int* __restrict__ valid,
                                                float thresh, int max_out, float* __restrict__ pboxes,
                                                int* __restrict__ pcount, float* __restrict__ best) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(valid[b], 0), max_out);
  const long row0 = (long)b * max_out;
  const float4* in = reinterpret_cast<const float4*>(boxes) + row0;
  float4* out = reinterpret_cast<float4*>(pboxes) + row0;
  int base = 0;
  bool any = false;
  float mx = -INFINITY;
  for (int i0 = 0; i0 < max_out; i0 += 64) {
    const int i = i0 + lane;
    const bool person = i < n && classes[row0 + i] == 1.0f;
    const float sc = person ? scores[row0 + i] : -INFINITY;
    mx = fmaxf(mx, sc);
    const bool keep = person && sc >= thresh;
    const unsigned long long kept = __ballot(keep);
    any |= __ballot(person) != 0ull;
    if (keep) out[base + __popcll(kept & ((1ull << lane) - 1ull))] = in[i];
    base += __popcll(kept);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  for (int i = base + lane; i < max_out; i += 64) out[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (lane == 0) {
    pcount[b] = base;
    best[b] = any ? mx : 0.f;
  }
}

void launch_persons(const float* boxes, const float* scores, const float* classes, const int* valid, int B,
                    float thresh, int max_out, float* pboxes, int* pcount, float* best, hipStream_t s) {
  hipLaunchKernelGGL(k_persons, dim3(B), dim3(64), 0, s, boxes, scores, classes, valid, thresh, max_out, pboxes,
                     pcount, best);
  PHX_LAUNCH_CHECK();
}

// ---- recovery epilogue (demo_v2.py:159-168) ----------------------------------------------------------
// k_def_recover: one launch for a batch of differently sized frames, no [S,S,3] or [d,d,3] intermediate
// in HBM.  A frame's cropped output [oh,ow,3] is one contiguous run of oh * ow * 3 elements; a lane owns
// four consecutive ones, cut so that its uint8 store is one aligned dword (its float store one aligned
// 16-B word when that address allows, else four dwords), a wave's stores are contiguous.  Every element
// takes its four taps from the canvas and `updates` (1.5 MB each per image at S = 512: they stay in
// L2), applies add, clip and denormalise per tap in fp32 (each multiply and add rounds on its own, as
// numpy's), then interpolates as cv2's CV_32F resize does: horizontal pass first, fp32 weights (1 - f, f)
// with f from the double expression, taps clamped.  S == 2 d is cv2's INTER_AREA shortcut, the 2x2
// box sum times 0.25.  Algorithmic bytes per frame: 24 * S * S read + (4 and / or 1) * oh * ow * 3 written.
struct RecoverArgs {
  const float* canvas;
  const float* upd;
  const RecFrame* frames;
  float mean[3], std[3];
  int S;
  uint8_t* out_u8;
  float* out_f32;
};

struct RecAxis {
  int i0, i1;
  float w0, w1;
};

// cv2's resize tables for destination index o (resize.cpp: fx = (float)((dx + 0.5) * scale_x - 0.5);
// sx = cvFloor(fx); fx -= sx): the horizontal table resets the weight where it clamps, the vertical
// pass clamps the rows and keeps the weights
__device__ __forceinline__ RecAxis rec_axis(int o, double scale, int S, bool horizontal) {
  float f = (float)(((double)o + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  RecAxis a;
  if (horizontal) {
    if (s < 0) {
      s = 0;
      f = 0.f;
    }
    if (s >= S - 1) {
      s = S - 1;
      f = 0.f;
    }
    a.i0 = s;
    a.i1 = min(s + 1, S - 1);
  } else {
    a.i0 = min(max(s, 0), S - 1);
    a.i1 = min(max(s + 1, 0), S - 1);
  }
  a.w0 = 1.0f - f;
  a.w1 = f;
  return a;
}

// clip(2 * PatchNeutralizer(x) + x, -1, 1) * stddev_rgb + mean_rgb at one canvas element
__device__ __forceinline__ float rec_tap(const float* __restrict__ cv, const float* __restrict__ up, long i, float sd,
                                         float mn) {
  const float y = fminf(fmaxf(up[i] + cv[i], -1.0f), 1.0f);
  return y * sd + mn;
}

__global__ __launch_bounds__(256) void k_def_recover(RecoverArgs a) {
  const int b = blockIdx.y;
  const RecFrame f = a.frames[b];
  const int S = a.S;
  const long row = (long)f.ow * 3, n = row * f.oh;
  // lane groups start `pad` elements before the frame so that group stores are aligned words
  const int pad = a.out_u8 ? (int)(reinterpret_cast<uintptr_t>(a.out_u8 + f.out_off) & 3)
                           : (int)((reinterpret_cast<uintptr_t>(a.out_f32 + f.out_off) >> 2) & 3);
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4 - pad;
  if (e0 >= n) return;
  const long ef = e0 < 0 ? 0 : e0;
  int oy = (int)(ef / row);
  const int r = (int)(ef - (long)oy * row);
  int ox = r / 3, c = r - ox * 3;
  const float* __restrict__ cv = a.canvas + (long)b * S * S * 3;
  const float* __restrict__ up = a.upd + (long)b * S * S * 3;
  const bool box = 2 * f.d == S;
  RecAxis ay = rec_axis(oy, f.scale, S, false), ax = rec_axis(ox, f.scale, S, true);
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long e = e0 + j;
    v[j] = 0.f;
    if (e < 0 || e >= n) continue;
    const float sd = c == 0 ? a.std[0] : c == 1 ? a.std[1] : a.std[2];
    const float mn = c == 0 ? a.mean[0] : c == 1 ? a.mean[1] : a.mean[2];
    const long r0 = (long)ay.i0 * S * 3 + c, r1 = (long)ay.i1 * S * 3 + c;
    const float t00 = rec_tap(cv, up, r0 + ax.i0 * 3, sd, mn), t01 = rec_tap(cv, up, r0 + ax.i1 * 3, sd, mn);
    const float t10 = rec_tap(cv, up, r1 + ax.i0 * 3, sd, mn), t11 = rec_tap(cv, up, r1 + ax.i1 * 3, sd, mn);
    if (box) {
      v[j] = (((t00 + t01) + t10) + t11) * 0.25f;
    } else {
      const float h0 = t00 * ax.w0 + t01 * ax.w1, h1 = t10 * ax.w0 + t11 * ax.w1;
      v[j] = h0 * ay.w0 + h1 * ay.w1;
    }
    if (++c == 3) {
      c = 0;
      if (++ox == f.ow) {
        ox = 0;
        ay = rec_axis(++oy, f.scale, S, false);
      }
      ax = rec_axis(ox, f.scale, S, true);
    }
  }
  const bool full = e0 >= 0 && e0 + 4 <= n;
  if (a.out_f32) {
    float* p = a.out_f32 + f.out_off + e0;
    if (full && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j >= 0 && e0 + j < n) p[j] = v[j];
    }
  }
  if (a.out_u8) {
    // np.clip(., 0, 255).astype('uint8') (demo_v2.py:134): the cast truncates
    uint32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = (uint32_t)(int)fminf(fmaxf(v[j], 0.f), 255.f);
    uint8_t* p = a.out_u8 + f.out_off + e0;
    if (full) {  // (dword aligned by the choice of pad)
      *reinterpret_cast<uint32_t*>(p) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j >= 0 && e0 + j < n) p[j] = (uint8_t)q[j];
    }
  }
}

void launch_def_recover(const float* canvas, const float* updates, const RecFrame* frames_dev, int B, int S,
                        const float* mean, const float* stdv, uint8_t* out_u8, float* out_f32, long max_elems,
                        hipStream_t s) {
  if (!out_u8 && !out_f32) throw std::invalid_argument("def_recover: no output");
  if (B < 1 || S < 2 || max_elems < 1) throw std::invalid_argument("def_recover: empty batch or frame");
  RecoverArgs a;
  a.canvas = canvas;
  a.upd = updates;
  a.frames = frames_dev;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean[c];
    a.std[c] = stdv[c];
  }
  a.S = S;
  a.out_u8 = out_u8;
  a.out_f32 = out_f32;
  const long groups = (max_elems + 3 + 3) / 4;  // up to 3 elements of lead-in per frame
  const dim3 grid((unsigned)((groups + 255) / 256), B);
  hipLaunchKernelGGL(k_def_recover, grid, dim3(256), 0, s, a);
  PHX_LAUNCH_CHECK();
}

}  // namespace phx
