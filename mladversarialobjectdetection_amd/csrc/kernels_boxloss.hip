// kernels_boxloss.hip — the box-regression attack term: the reference's InverseDIOULoss
// (regression_loss.py:16-142), taken as written, over the second pass's kept anchors (attacker.py:118-141)
// and the boxes the patches were placed by.
//   value     per (gt g, pred p): 1 - diou_loss(b1 = g, b2 = p) (:71-84, :101-142); per image
//             sum_g max_p (+ Keras epsilon 1e-7, :49-59); the batch value is the sum over images (:61)
//   gradient  [TF-recall] reduce_max splits among exact ties; tf.maximum(x, y) / tf.minimum(x, y) send a
//             tie to x, so a pred coordinate (always y here) gets gradient only where it wins strictly and
//             maximum(0., v) passes only v > 0; divide_no_nan has zero gradient where the denominator is 0
// One maximum per (image, gt): k_idiou_part reduces a chunk of anchors to (max, lowest anchor, tie
// count) per gt, k_idiou_merge folds the chunks in chunk order (k_image_max_part / _merge with a gt
// axis).  No float atomics: every sum and every merge runs in a fixed order.
// The arithmetic that decides the argmax and the ties is kept in the reference's operation order with
// FMA contraction disabled; the scatter re-evaluates it with the same function, so its equality tests
// against the merged maximum are exact.
#include <cfloat>
#include <stdexcept>

#include "boxloss.hpp"
#include "common.hpp"
#include "phx.h"

#pragma clang fp contract(off)

namespace phx {

namespace {

constexpr int kNone = 0x7fffffff;

__device__ __forceinline__ float div_no_nan(float x, float y) { return y == 0.0f ? 0.0f : x / y; }

// 1. - diou_loss(b1 = g, b2 = p): regression_loss.py:84, :101-142.  The gt's height, width and area
// are not clamped (:45-47), the pred's are (:115-117); the "centres" are (ymin + height, xmin + width)
// as written (:130-131).
__device__ __forceinline__ float idiou_value(const float4 g, const float4 p) {
  const float gh = g.z - g.x, gw = g.w - g.y;
  const float ga = gh * gw;
  const float pw = fmaxf(0.0f, p.w - p.y), ph = fmaxf(0.0f, p.z - p.x);
  const float pa = pw * ph;
  const float iy0 = fmaxf(g.x, p.x), ix0 = fmaxf(g.y, p.y), iy1 = fminf(g.z, p.z), ix1 = fminf(g.w, p.w);
  const float iw = fmaxf(0.0f, ix1 - ix0), ih = fmaxf(0.0f, iy1 - iy0);
  const float ia = iw * ih;
  const float ua = ga + pa - ia;
  const float iou = div_no_nan(ia, ua);
  const float dy = (g.x + gh) - (p.x + ph), dx = (g.y + gw) - (p.y + pw);
  const float cd = dy * dy + dx * dx;
  const float ey0 = fminf(g.x, p.x), ex0 = fminf(g.y, p.y), ey1 = fmaxf(g.z, p.z), ex1 = fmaxf(g.w, p.w);
  const float ew = fmaxf(0.0f, ex1 - ex0), eh = fmaxf(0.0f, ey1 - ey0);
  const float diag = eh * eh + ew * ew;
  const float diou = iou - div_no_nan(cd, diag);
  return 1.0f - (1.0f - diou);
}

// d value / d (p.ymin, p.xmin, p.ymax, p.xmax) under the rules in the header
__device__ __forceinline__ float4 idiou_grad(const float4 g, const float4 p) {
  const float gh = g.z - g.x, gw = g.w - g.y;
  const float ga = gh * gw;
  const float rw = p.w - p.y, rh = p.z - p.x;
  const float pw = fmaxf(0.0f, rw), ph = fmaxf(0.0f, rh);
  const float pa = pw * ph;
  const float iy0 = fmaxf(g.x, p.x), ix0 = fmaxf(g.y, p.y), iy1 = fminf(g.z, p.z), ix1 = fminf(g.w, p.w);
  const float riw = ix1 - ix0, rih = iy1 - iy0;
  const float iw = fmaxf(0.0f, riw), ih = fmaxf(0.0f, rih);
  const float ia = iw * ih;
  const float ua = ga + pa - ia;
  const float dy = (g.x + gh) - (p.x + ph), dx = (g.y + gw) - (p.y + pw);
  const float cd = dy * dy + dx * dx;
  const float ey0 = fminf(g.x, p.x), ex0 = fminf(g.y, p.y), ey1 = fmaxf(g.z, p.z), ex1 = fmaxf(g.w, p.w);
  const float rew = ex1 - ex0, reh = ey1 - ey0;
  const float ew = fmaxf(0.0f, rew), eh = fmaxf(0.0f, reh);
  const float diag = eh * eh + ew * ew;
  float gy0 = 0.f, gx0 = 0.f, gy1 = 0.f, gx1 = 0.f;  // d / d p.ymin, p.xmin, p.ymax, p.xmax
  float gph = 0.f, gpw = 0.f;                        // d / d (clamped) pred height, width
  // iou = ia / ua, ua = ga + pa - ia
  if (ua != 0.0f) {
    const float dia = 1.0f / ua + ia / (ua * ua);  // through the numerator and through -ia in ua
    const float dpa = -ia / (ua * ua);
    gph += dpa * pw;
    gpw += dpa * ph;
    const float dih = dia * iw, diw = dia * ih;
    if (rih > 0.0f) {
      if (p.z < g.z) gy1 += dih;  // iy1 = min(g.ymax, p.ymax): the pred wins strictly
      if (p.x > g.x) gy0 -= dih;  // iy0 = max(g.ymin, p.ymin)
    }
    if (riw > 0.0f) {
      if (p.w < g.w) gx1 += diw;
      if (p.y > g.y) gx0 -= diw;
    }
  }
  // - cd / diag
  if (diag != 0.0f) {
    const float dcd = -1.0f / diag;
    const float ddiag = cd / (diag * diag);
    // cd = dy^2 + dx^2, dy = c1y - (p.ymin + ph)
    const float dc2y = dcd * 2.0f * dy * -1.0f, dc2x = dcd * 2.0f * dx * -1.0f;
    gy0 += dc2y;
    gph += dc2y;
    gx0 += dc2x;
    gpw += dc2x;
    const float deh = ddiag * 2.0f * eh, dew = ddiag * 2.0f * ew;
    if (reh > 0.0f) {
      if (p.z > g.z) gy1 += deh;  // ey1 = max(g.ymax, p.ymax)
      if (p.x < g.x) gy0 -= deh;  // ey0 = min(g.ymin, p.ymin)
    }
    if (rew > 0.0f) {
      if (p.w > g.w) gx1 += dew;
      if (p.y < g.y) gx0 -= dew;
    }
  }
  if (rh > 0.0f) {
    gy1 += gph;
    gy0 -= gph;
  }
  if (rw > 0.0f) {
    gx1 += gpw;
    gx0 -= gpw;
  }
  return make_float4(gy0, gx0, gy1, gx1);
}

// (max, lowest anchor, tie count) of two disjoint anchor sets; kNone marks an empty set
__device__ __forceinline__ void idiou_fold(float& m, int& a, int& c, float om, int oa, int oc) {
  if (oa == kNone) return;
  if (a == kNone || om > m) {
    m = om;
    a = oa;
    c = oc;
  } else if (om == m) {
    a = min(a, oa);
    c += oc;
  }
}

__device__ __forceinline__ int gt_count(const int* __restrict__ gcount, int b) {
  return min(max(gcount[b], 0), kIdiouMaxGt);
}

// grid (chunks, B), 256 lanes: lane t holds anchors chunk * 1024 + t + 256 u (u < 4) in registers and
// evaluates its kept ones against every gt (staged in LDS); per gt a wave butterfly, then the four
// waves merge in wave order.  pm / pi / pc: [B][chunks][100]
__global__ __launch_bounds__(256) void k_idiou_part(const float* __restrict__ boxes,
                                                    const uint8_t* __restrict__ keep,
                                                    const float* __restrict__ gt,
                                                    const int* __restrict__ gcount, int A,
                                                    float* __restrict__ pm, int* __restrict__ pi,
                                                    int* __restrict__ pc) {
  const int b = blockIdx.y, ch = blockIdx.x, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  __shared__ float4 s_g[kIdiouMaxGt];
  __shared__ float s_m[4][kIdiouMaxGt];
  __shared__ int s_a[4][kIdiouMaxGt];
  __shared__ int s_c[4][kIdiouMaxGt];
  const int G = gt_count(gcount, b);
  for (int g = t; g < G; g += 256) s_g[g] = reinterpret_cast<const float4*>(gt)[(long)b * kIdiouMaxGt + g];
  float4 bx[4];
  bool kp[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int a = ch * kIdiouChunk + u * 256 + t;
    kp[u] = a < A && (keep[(long)b * A + min(a, A - 1)] & 1);
    bx[u] = kp[u] ? reinterpret_cast<const float4*>(boxes)[(long)b * A + a] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const bool any_wave = __ballot(kp[0] || kp[1] || kp[2] || kp[3]) != 0ull;
  for (int g = 0; g < G; ++g) {
    float m = -FLT_MAX;
    int am = kNone, c = 0;
    if (any_wave) {  // (wave-uniform)
      const float4 gb = s_g[g];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!kp[u]) continue;
        const float v = idiou_value(gb, bx[u]);
        idiou_fold(m, am, c, v, ch * kIdiouChunk + u * 256 + t, 1);
      }
      for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(m, off);
        const int oa = __shfl_xor(am, off);
        const int oc = __shfl_xor(c, off);
        idiou_fold(m, am, c, om, oa, oc);
      }
    }
    if (lane == 0) {
      s_m[wave][g] = m;
      s_a[wave][g] = am;
      s_c[wave][g] = c;
    }
  }
  __syncthreads();
  for (int g = t; g < G; g += 256) {
    float m = s_m[0][g];
    int am = s_a[0][g], c = s_c[0][g];
    for (int w = 1; w < 4; ++w) idiou_fold(m, am, c, s_m[w][g], s_a[w][g], s_c[w][g]);
    const long o = ((long)b * gridDim.x + ch) * kIdiouMaxGt + g;
    pm[o] = m;
    pi[o] = am;
    pc[o] = c;
  }
}

// grid B, 128 lanes: lane g folds gt g's chunks in chunk order; lane 0 then sums the image's maxima in
// gt order and adds the epsilon
__global__ __launch_bounds__(128) void k_idiou_merge(const float* __restrict__ pm, const int* __restrict__ pi,
                                                     const int* __restrict__ pc, int S,
                                                     const int* __restrict__ gcount,
                                                     float* __restrict__ gt_max, int* __restrict__ gt_anchor,
                                                     int* __restrict__ gt_nties,
                                                     float* __restrict__ per_image) {
  const int b = blockIdx.x, g = threadIdx.x;
  __shared__ float s_v[kIdiouMaxGt];
  const int G = gt_count(gcount, b);
  if (g < kIdiouMaxGt) {
    float m = -FLT_MAX;
    int am = kNone, c = 0;
    if (g < G)
      for (int k = 0; k < S; ++k) {
        const long o = ((long)b * S + k) * kIdiouMaxGt + g;
        idiou_fold(m, am, c, pm[o], pi[o], pc[o]);
      }
    const bool none = am == kNone;
    const long o = (long)b * kIdiouMaxGt + g;
    gt_max[o] = none ? 0.0f : m;
    gt_anchor[o] = none ? -1 : am;
    gt_nties[o] = none ? 0 : c;
    s_v[g] = none ? 0.0f : m;
  }
  __syncthreads();
  if (g == 0) {
    float v = 0.0f;
    for (int k = 0; k < G; ++k) v += s_v[k];
    per_image[b] = v + 1e-7f;  // keras.backend.epsilon() (regression_loss.py:59)
  }
}

// the batch value (the images in order) and the weighted term into the loss metric.  One lane.
__global__ void k_idiou_batch(const float* __restrict__ per_image, int B, float weight,
                              float* __restrict__ batch, float* __restrict__ metrics) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float v = 0.0f;
  for (int b = 0; b < B; ++b) v += per_image[b];
  *batch = v;
  if (metrics) metrics[PHX_M_LOSS] += weight * v;
}

// grid (pixel blocks, B), 256 lanes, one lane per (image, pixel).  The image's gts and their (max,
// anchor, tie count) are staged in LDS; the lane walks them in gt order and, for a gt whose winner is one
// of its pixel's anchors (a tied gt: every anchor of the pixel is re-evaluated), adds that anchor's four
// box-logit gradients times the box-predict kernel's columns into its own dx row, in (gt, anchor) order.
__global__ __launch_bounds__(256) void k_box_scatter(
    const float* __restrict__ boxes, const uint8_t* __restrict__ keep, const float* __restrict__ gt,
    const int* __restrict__ gcount, const float* __restrict__ gt_max, const int* __restrict__ gt_anchor,
    const int* __restrict__ gt_nties, const float* __restrict__ box_base, const float* __restrict__ anchors,
    const LevelDesc* __restrict__ lev, int nlev, int A, int na, const float* __restrict__ wpred /*[K][na*4]*/,
    int K, float weight, float* __restrict__ dx_base, const long* __restrict__ dx_off) {
  const int b = blockIdx.y, t = threadIdx.x;
  const int PT = A / na;
  const int p = blockIdx.x * 256 + t;
  __shared__ float4 s_g[kIdiouMaxGt];
  __shared__ float s_m[kIdiouMaxGt];
  __shared__ int s_a[kIdiouMaxGt];
  __shared__ int s_c[kIdiouMaxGt];
  const int G = gt_count(gcount, b);
  for (int g = t; g < G; g += 256) {
    const long o = (long)b * kIdiouMaxGt + g;
    s_g[g] = reinterpret_cast<const float4*>(gt)[o];
    s_m[g] = gt_max[o];
    s_a[g] = gt_anchor[o];
    s_c[g] = gt_nties[o];
  }
  __syncthreads();
  if (p >= PT) return;
  int l = 0;
  while (l + 1 < nlev && p * na >= lev[l + 1].anchor0) ++l;
  const LevelDesc L = lev[l];
  const int pix = p - L.anchor0 / na;
  const long prow = (long)b * L.h * L.w + pix;
  float* dx = dx_base + dx_off[l] + prow * K;
  const int N = na * 4;
  for (int g = 0; g < G; ++g) {
    const int nt = s_c[g];
    if (nt <= 0) continue;
    uint32_t win = 0;
    if (nt == 1) {
      const int a = s_a[g];
      if (a / na != p) continue;
      win = 1u << (a - p * na);
    } else {
      const float mx = s_m[g];
      for (int k = 0; k < na; ++k) {
        const long e = (long)b * A + (long)p * na + k;
        if ((keep[e] & 1) && idiou_value(s_g[g], reinterpret_cast<const float4*>(boxes)[e]) == mx) win |= 1u << k;
      }
      if (!win) continue;
    }
    const float coef = weight / (float)nt;
    for (int k = 0; k < na; ++k) {
      if (!(win >> k & 1)) continue;
      const int a = p * na + k;
      const float4 d = idiou_grad(s_g[g], reinterpret_cast<const float4*>(boxes)[(long)b * A + a]);
      // decode_box_outputs (anchors.py:30-58): ymin = yc - h / 2, ymax = yc + h / 2, yc = ty ha + yca,
      // h = exp(th) ha (and the same in x)
      const float4 an = reinterpret_cast<const float4*>(anchors)[a];
      const float ha = an.z - an.x, wa = an.w - an.y;
      const float4 lg = *reinterpret_cast<const float4*>(box_base + L.box_off + (prow * na + k) * 4);
      const float h = expf(lg.z) * ha, w = expf(lg.w) * wa;
      const float dt0 = coef * ((d.x + d.z) * ha);
      const float dt1 = coef * ((d.y + d.w) * wa);
      const float dt2 = coef * ((d.z - d.x) * 0.5f * h);
      const float dt3 = coef * ((d.w - d.y) * 0.5f * w);
      const float* wc = wpred + k * 4;
#pragma unroll 8
      for (int j = 0; j < K; ++j) {
        const float* wj = wc + (long)j * N;  // (a kernel's offset in the weight blob is not 16-B aligned)
        dx[j] = dx[j] + (((wj[0] * dt0 + wj[1] * dt1) + wj[2] * dt2) + wj[3] * dt3);
      }
    }
  }
}

}  // namespace

void launch_idiou(const float* boxes, const uint8_t* keep, const float* gt, const int* gcount, int B, int A,
                  float* gt_max, int* gt_anchor, int* gt_nties, float* per_image, float* batch, int* scratch,
                  float weight, float* metrics, hipStream_t s) {
  if (B < 1 || A < 1) throw std::invalid_argument("idiou: empty batch or anchor set");
  const int S = idiou_chunks(A);
  const size_t n = (size_t)B * S * kIdiouMaxGt;
  float* pm = reinterpret_cast<float*>(scratch);
  int* pi = scratch + n;
  int* pc = pi + n;
  hipLaunchKernelGGL(k_idiou_part, dim3(S, B), dim3(256), 0, s, boxes, keep, gt, gcount, A, pm, pi, pc);
  PHX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_idiou_merge, dim3(B), dim3(128), 0, s, pm, pi, pc, S, gcount, gt_max, gt_anchor, gt_nties,
                     per_image);
  PHX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_idiou_batch, dim3(1), dim3(64), 0, s, per_image, B, weight, batch, metrics);
  PHX_LAUNCH_CHECK();
}

void launch_box_scatter(const float* boxes, const uint8_t* keep, const float* gt, const int* gcount,
                        const float* gt_max, const int* gt_anchor, const int* gt_nties, const float* box_base,
                        const float* anchors, const LevelDesc* lev, int nlev, int A, int B, int na,
                        const float* wpred, int K, float weight, float* dx_base, const long* dx_off,
                        hipStream_t s) {
  if (na < 1 || A % na) throw std::runtime_error("box_scatter: anchors not a multiple of anchors per pixel");
  if (na > 32) throw std::runtime_error("box_scatter: more than 32 anchors per pixel");
  hipLaunchKernelGGL(k_box_scatter, dim3(cdiv(A / na, 256), B), dim3(256), 0, s, boxes, keep, gt, gcount, gt_max,
                     gt_anchor, gt_nties, box_base, anchors, lev, nlev, A, na, wpred, K, weight, dx_base, dx_off);
  PHX_LAUNCH_CHECK();
}

}  // namespace phx
