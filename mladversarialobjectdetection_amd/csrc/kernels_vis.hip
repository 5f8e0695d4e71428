// kernels_vis.hip — the training summaries of PatchAttacker.vis_images / PatchAttackDefender.vis_images
// (attacker.py:257-305, attack_detection.py:239-288) on the device:
//   k_vis_sample   tf.image.draw_bounding_boxes twice + clip(x * stddev_rgb + mean_rgb, 0, 255) -> uint8
//   k_score_curve  #scores >= threshold for every bin of the ASR curve (calc_asr, attacker.py:238-255)
//   k_add_clip     clip(images + updates, -1, 1), the recovered batch the detector reads
// Built with -ffp-contract=off (Makefile): every multiply and add rounds on its own, as TF's do.
//
// draw_bounding_boxes, restated ([TF-recall], parity unpinned).  A box
// (ymin, xmin, ymax, xmax) in pixels is normalised by convert_format in fp32 (ymin / h, xmin / w, ...)
// and the op takes min_row = trunc((ymin / h) * (H - 1)) in fp32 (max_row, min_col, max_col likewise).
// An inverted box (min > max on either axis) or one wholly outside the image draws nothing; otherwise
// its top line is drawn if min_row >= 0, its bottom line if max_row < H, the left if min_col >= 0, the
// right if max_col < W, each over the clamped range of the other axis, one pixel thick.  Taken together
// a box paints exactly the pixels of the image that lie on the border of the integer rectangle
// [min_row, max_row] x [min_col, max_col] — the test this kernel applies per pixel (tests/vis_oracle.py
// draws the four lines).  All boxes of one call share one colour, so only the order of the two calls
// matters: set B paints over set A.  box.to_tensor() pads every image's list with zero boxes up to the
// batch's longest; a zero box paints pixel (0, 0).
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"

namespace phx {

namespace {

constexpr int kVisGroups = 8;  // 1024-byte lane groups a workgroup walks (8 KB of output, 32 KB read)

struct VisArgs {
  const float* img;
  const float* box[2];
  const int* cnt[2];
  int n[2];
  int B, H, W;
  uint8_t* out;
  long stride, off;
  float mean[3], std[3];
};

// trunc((v / d) * m) in fp32 (v / d correctly rounded: div_exact is n / d bit for bit), clamped so the
// conversion is defined for any finite input
__device__ __forceinline__ int vis_extent(float v, float d, float m) {
  const float f = div_exact(v, d) * m;
  return (int)fminf(fmaxf(f, -1.0e9f), 1.0e9f);
}

__device__ __forceinline__ bool vis_hit(int4 e, int r, int c) {
  return r >= e.x && r <= e.z && c >= e.y && c <= e.w && (r == e.x || r == e.z || c == e.y || c == e.w);
}

// A workgroup owns kVisGroups * 1024 consecutive output bytes of one image (a few rows).  It stages the
// integer extents of the boxes that reach its rows in LDS once (set A in the lower half, set B in the
// upper), so a pixel is tested against those only.  A lane owns four consecutive output bytes, cut so
// that its store is one aligned dword: one 16-B load (three per four pixels) where the input address
// allows it, four dword loads otherwise; the image's first and last lanes store bytes.
__global__ __launch_bounds__(256) void k_vis_sample(VisArgs a) {
  __shared__ int4 sbox[2 * kVisMaxBoxes];
  __shared__ int s_n[2], s_max[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const long row = (long)W * 3, n = row * H;
  uint8_t* out = a.out + (long)b * a.stride + a.off;
  const int pad = (int)(reinterpret_cast<uintptr_t>(out) & 3);
  const long g0 = (long)blockIdx.x * kVisGroups * 1024 - pad;
  if (g0 >= n) return;
  if (tid < 2) {
    s_n[tid] = 0;
    s_max[tid] = 0;
  }
  __syncthreads();
  // the batch's longest list per set (to_tensor's padded width)
  for (int k = 0; k < 2; ++k)
    if (a.box[k])
      for (int i = tid; i < a.B; i += 256) atomicMax(&s_max[k], min(max(a.cnt[k][i], 0), a.n[k]));
  __syncthreads();
  const int r0 = (int)(max(g0, 0L) / row), r1 = (int)((min(g0 + (long)kVisGroups * 1024, n) - 1) / row);
  const float fh = (float)H, fw = (float)W, mh = (float)(H - 1), mw = (float)(W - 1);
  for (int k = 0; k < 2; ++k) {
    if (!a.box[k]) continue;
    const int cnt = min(max(a.cnt[k][b], 0), a.n[k]);
    const int total = cnt + (cnt < s_max[k] ? 1 : 0);  // + one zero box standing for all the padding
    const float* bx = a.box[k] + (long)b * a.n[k] * 4;
    for (int i = tid; i < total; i += 256) {
      int4 e = make_int4(0, 0, 0, 0);
      if (i < cnt) {
        e.x = vis_extent(bx[i * 4 + 0], fh, mh);
        e.y = vis_extent(bx[i * 4 + 1], fw, mw);
        e.z = vis_extent(bx[i * 4 + 2], fh, mh);
        e.w = vis_extent(bx[i * 4 + 3], fw, mw);
      }
      const bool drawn = e.x <= e.z && e.y <= e.w && e.x < H && e.z >= 0 && e.y < W && e.w >= 0;
      if (drawn && max(e.x, 0) <= r1 && min(e.z, H - 1) >= r0) sbox[k * kVisMaxBoxes + atomicAdd(&s_n[k], 1)] = e;
    }
  }
  __syncthreads();
  const int na = s_n[0], nb = s_n[1];
  const float* __restrict__ src = a.img + (long)b * n;
  for (int g = 0; g < kVisGroups; ++g) {
    const long e0 = g0 + ((long)g * 256 + tid) * 4;
    if (e0 >= n) break;
    const long ef = e0 < 0 ? 0 : e0;
    // the lane's bytes lie in at most two pixels
    const long p0 = ef / 3;
    int ch = (int)(ef - p0 * 3);
    const int ra = (int)(p0 / W), ca = (int)(p0 - (long)ra * W);
    const int rb = ca + 1 == W ? ra + 1 : ra, cb = ca + 1 == W ? 0 : ca + 1;
    int qa = 0, qb = 0;  // 0: the image, 1: set A's colour, 2: set B's
    for (int i = 0; i < na; ++i) {
      const int4 e = sbox[i];
      if (vis_hit(e, ra, ca)) qa = 1;
      if (vis_hit(e, rb, cb)) qb = 1;
    }
    for (int i = 0; i < nb; ++i) {
      const int4 e = sbox[kVisMaxBoxes + i];
      if (vis_hit(e, ra, ca)) qa = 2;
      if (vis_hit(e, rb, cb)) qb = 2;
    }
    const bool full = e0 >= 0 && e0 + 4 <= n;
    float x[4];
    if (full && (reinterpret_cast<uintptr_t>(src + e0) & 15) == 0) {
      const float4 v = *reinterpret_cast<const float4*>(src + e0);
      x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = (e0 + j >= 0 && e0 + j < n) ? src[e0 + j] : 0.f;
    }
    uint32_t q[4];
    int code = qa;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e0 + j >= 0) {
        // tf.constant([[0., 1., 0.]]) / [[0., 0., 1.]] written into the normalised image
        const float v = code == 0 ? x[j] : (ch == code ? 1.f : 0.f);
        const float sd = ch == 0 ? a.std[0] : ch == 1 ? a.std[1] : a.std[2];
        const float mn = ch == 0 ? a.mean[0] : ch == 1 ? a.mean[1] : a.mean[2];
        q[j] = (uint32_t)(int)fminf(fmaxf(v * sd + mn, 0.f), 255.f);  // tf.cast(., uint8) truncates
        if (++ch == 3) {
          ch = 0;
          code = qb;
        }
      } else {
        q[j] = 0;
      }
    }
    uint8_t* p = out + e0;
    if (full) {  // (dword aligned by the choice of pad)
      *reinterpret_cast<uint32_t*>(p) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j >= 0 && e0 + j < n) p[j] = (uint8_t)q[j];
    }
  }
}

struct CurveArgs {
  const float* sc[2];
  const int* cnt[2];
  int B, N, T;
  int* out;
  float th[kCurveMaxT];
};

constexpr int kCurveChunk = 4096;

// One workgroup per score set.  The valid scores are staged in LDS a chunk at a time (a slot beyond
// count[b] holds NaN, which no threshold admits); threshold t belongs to a group of L = 256 / T' lanes
// (T' = T rounded up to a power of two, at least 4: the group lies in one wave), which strides over the
// chunk and adds its integer counts with shuffles.  Integer counts only; no atomics.
__global__ __launch_bounds__(256) void k_score_curve(CurveArgs a) {
  __shared__ float s[kCurveChunk];
  const int k = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ sc = a.sc[k];
  const int* __restrict__ cnt = a.cnt[k];
  int tp = 4;
  while (tp < a.T) tp <<= 1;
  const int L = 256 / tp, t = tid / L, l = tid - t * L;
  const float th = t < a.T ? a.th[t] : 0.f;
  const long total = (long)a.B * a.N;
  int acc = 0;
  for (long base = 0; base < total; base += kCurveChunk) {
    const int m = (int)min((long)kCurveChunk, total - base);
    __syncthreads();
    for (int i = tid; i < m; i += 256) {
      const long e = base + i;
      const int bb = (int)(e / a.N), j = (int)(e - (long)bb * a.N);
      const int c = cnt ? min(max(cnt[bb], 0), a.N) : a.N;
      s[i] = j < c ? sc[e] : __uint_as_float(0x7fc00000u);
    }
    __syncthreads();
    if (t < a.T)
      for (int i = l; i < m; i += L) acc += s[i] >= th ? 1 : 0;
  }
  for (int w = L >> 1; w > 0; w >>= 1) acc += __shfl_xor(acc, w);
  if (t < a.T && l == 0) a.out[k * a.T + t] = acc;
}

__global__ __launch_bounds__(256) void k_add_clip(const float* __restrict__ x, const float* __restrict__ u,
                                                  float* __restrict__ y, long n4, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) {
    const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(u)[i];
    reinterpret_cast<float4*>(y)[i] =
        make_float4(fminf(fmaxf(a.x + b.x, -1.f), 1.f), fminf(fmaxf(a.y + b.y, -1.f), 1.f),
                    fminf(fmaxf(a.z + b.z, -1.f), 1.f), fminf(fmaxf(a.w + b.w, -1.f), 1.f));
  } else {
    const long e = n4 * 4 + (i - n4);
    if (e < n) y[e] = fminf(fmaxf(x[e] + u[e], -1.f), 1.f);
  }
}

}  // namespace

void launch_vis_sample(const float* images, int B, int H, int W, const float* boxes_a, const int* count_a, int na,
                       const float* boxes_b, const int* count_b, int nb, const float* mean, const float* stdv,
                       uint8_t* out, long out_stride, long out_offset, hipStream_t s) {
  if (!images || !out) throw std::invalid_argument("vis_sample: null images or output");
  if (B < 1 || H < 1 || W < 1) throw std::invalid_argument("vis_sample: empty batch or image");
  if ((boxes_a && (!count_a || na < 0 || na >= kVisMaxBoxes)) || (boxes_b && (!count_b || nb < 0 || nb >= kVisMaxBoxes)))
    throw std::invalid_argument("vis_sample: a box set needs its counts and fewer than 512 slots");
  VisArgs a;
  a.img = images;
  a.box[0] = boxes_a;
  a.box[1] = boxes_b;
  a.cnt[0] = count_a;
  a.cnt[1] = count_b;
  a.n[0] = na;
  a.n[1] = nb;
  a.B = B, a.H = H, a.W = W;
  a.out = out;
  a.stride = out_stride;
  a.off = out_offset;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean[c];
    a.std[c] = stdv[c];
  }
  const long n = (long)H * W * 3, per = (long)kVisGroups * 1024;
  const dim3 grid((unsigned)((n + 3 + per - 1) / per), B);  // up to 3 bytes of lead-in per image
  hipLaunchKernelGGL(k_vis_sample, grid, dim3(256), 0, s, a);
  PHX_LAUNCH_CHECK();
}

void launch_score_curve(const float* scores0, const int* count0, const float* scores1, const int* count1, int B, int N,
                        const float* thresholds, int T, int* out, hipStream_t s) {
  if (!scores0 || !thresholds || !out) throw std::invalid_argument("score_curve: null scores, thresholds or output");
  if (B < 1 || N < 1) throw std::invalid_argument("score_curve: empty score set");
  if (T < 1 || T > kCurveMaxT) throw std::invalid_argument("score_curve: T outside [1, 128]");
  CurveArgs a;
  a.sc[0] = scores0, a.sc[1] = scores1;
  a.cnt[0] = count0, a.cnt[1] = count1;
  a.B = B, a.N = N, a.T = T;
  a.out = out;
  for (int t = 0; t < kCurveMaxT; ++t) a.th[t] = t < T ? thresholds[t] : 0.f;
  hipLaunchKernelGGL(k_score_curve, dim3(scores1 ? 2 : 1), dim3(256), 0, s, a);
  PHX_LAUNCH_CHECK();
}

void launch_add_clip(const float* x, const float* u, float* y, long n, hipStream_t s) {
  if (n < 1) return;
  const bool al = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const long n4 = al ? n / 4 : 0, threads = n4 + (n - n4 * 4);
  hipLaunchKernelGGL(k_add_clip, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, x, u, y, n4, n);
  PHX_LAUNCH_CHECK();
}

}  // namespace phx
