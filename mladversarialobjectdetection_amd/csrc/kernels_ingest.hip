// kernels_ingest.hip — the reference's streaming.Stream.change_frame_size (streaming.py:53-62) for a
// packed batch of HWC uint8 frames of mixed sizes: cv2.resize(frame, (set_width, int(h * scale))) with
// the default INTER_LINEAR on an 8UC3 frame, restated as oracle/adv_patch.py::resize_linear_u8 does:
//   equal size             a copy
//   W == 2 dw, H == 2 dh   resize() runs INTER_AREA: the 2x2 box mean (sum + 2) >> 2
//   anything else          11-bit fixed-point bilinear taps (lin_tap), horizontal pass into int rows,
//                          vertical pass ((b0 * (S0 >> 4)) >> 16 + (b1 * (S1 >> 4)) >> 16 + 2) >> 2
// with the video path's BGR -> RGB swap (streaming.py:75) folded into the read.  One launch, frames on
// blockIdx.y; a frame's mode comes from its own dims (sized on the host, IngestFrame).
//
// Output-stationary: a lane owns 4 consecutive output pixels of one row (12 bytes).  They leave as
// three dword stores when the 12 bytes start 4-byte aligned (always at set_width 640 / 1280 with an
// aligned frame offset), byte stores otherwise; the box mode reads its 2 x 24 source bytes as dwords
// under the same condition on the source.  The bilinear mode reads a pixel's two adjacent horizontal
// taps of a row as a dword and a halfword at any alignment (16 loads per lane, all issued before the
// arithmetic; as 48 byte loads the 1080p -> 640 batch took 1.4 times as long).  Bounds: a downscale reads at most
// min(source, 12 B per output pixel) and writes 3 B per output pixel — HBM-trivial next to the detector
// that follows; the per-pixel work is integer ALU plus five fp64 tap positions per lane.
#include <cstdint>

#include "common.hpp"
#include "cv_resize.hpp"
#include "kernels.hpp"

namespace phx {

__global__ __launch_bounds__(256) void k_ingest(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                const IngestFrame* __restrict__ frames, int swap) {
  const IngestFrame f = frames[blockIdx.y];
  const int H = f.h, W = f.w, dh = f.dh, dw = f.dw;
  const int gpr = (dw + 3) >> 2;  // lanes per output row
  const unsigned g = blockIdx.x * 256u + threadIdx.x;  // (the host refuses a frame of 2^31 lanes)
  if ((long)g >= (long)dh * gpr) return;
  const int oy = (int)(g / (unsigned)gpr), ox0 = (int)(g - (unsigned)oy * (unsigned)gpr) * 4;
  const int n = min(4, dw - ox0);  // pixels of this lane
  const uint8_t* im = src + f.src_off;
  uint8_t* dst = out + f.out_off + ((long)oy * dw + ox0) * 3;
  int v[12];
  if (dh == H && dw == W) {  // copy
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const long q = ((long)oy * W + min(ox0 + p, W - 1)) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) v[3 * p + k] = im[q + k];
    }
  } else if (W == 2 * dw && H == 2 * dh) {  // exact 2x decimation
    const uint8_t* r0 = im + ((long)(2 * oy) * W + 2 * ox0) * 3;
    const uint8_t* r1 = r0 + (long)W * 3;
    // W * 3 = 6 dw and 6 ox0 = 24 * (lane in row): both rows start 4-byte aligned when the frame does
    if (n == 4 && (reinterpret_cast<uintptr_t>(r0) & 3) == 0 && ((W * 3L) & 3) == 0) {
      uint32_t a[6], b[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        a[i] = reinterpret_cast<const uint32_t*>(r0)[i];
        b[i] = reinterpret_cast<const uint32_t*>(r1)[i];
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int j0 = 6 * p + k, j1 = j0 + 3;  // byte indices of the two source pixels in a row
          const int s = (int)((a[j0 >> 2] >> (8 * (j0 & 3))) & 255u) + (int)((a[j1 >> 2] >> (8 * (j1 & 3))) & 255u) +
                        (int)((b[j0 >> 2] >> (8 * (j0 & 3))) & 255u) + (int)((b[j1 >> 2] >> (8 * (j1 & 3))) & 255u);
          v[3 * p + k] = (s + 2) >> 2;
        }
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const long q = 6L * (min(ox0 + p, dw - 1) - ox0);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[3 * p + k] = (r0[q + k] + r0[q + 3 + k] + r1[q + k] + r1[q + 3 + k] + 2) >> 2;
      }
    }
  } else {  // INTER_LINEAR, fixed point
    const double sy = 1.0 / ((double)dh / (double)H), sx = 1.0 / ((double)dw / (double)W);
    int ys, yw0, yw1;
    lin_tap(oy, sy, H, false, &ys, &yw0, &yw1);
    const uint8_t* r0 = im + (long)min(max(ys, 0), H - 1) * W * 3;
    const uint8_t* r1 = im + (long)min(max(ys + 1, 0), H - 1) * W * 3;
    int xw0[4], xw1[4];
    if (W >= 2) {
      // a pixel's two horizontal taps are adjacent: 6 bytes per row, read as a dword and a halfword at
      // any alignment (2 loads instead of 6).  A tap clamped to the last column (xs = W - 1, weight
      // 2048 / 0) reads from W - 2 and takes the second pixel, so nothing beyond the row is touched.
      uint32_t lo[4][2];
      uint16_t hi[4][2];
      bool last[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        int xs;
        lin_tap(min(ox0 + p, dw - 1), sx, W, true, &xs, &xw0[p], &xw1[p]);
        const int xb = min(xs, W - 2);
        last[p] = xb != xs;
        __builtin_memcpy(&lo[p][0], r0 + 3L * xb, 4);
        __builtin_memcpy(&hi[p][0], r0 + 3L * xb + 4, 2);
        __builtin_memcpy(&lo[p][1], r1 + 3L * xb, 4);
        __builtin_memcpy(&hi[p][1], r1 + 3L * xb + 4, 2);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          int t[2][2];  // [row][tap]
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const uint32_t l = lo[p][r], h = hi[p][r];
            t[r][0] = (int)((l >> (8 * k)) & 255u);
            t[r][1] = k == 0 ? (int)(l >> 24) : (int)((h >> (8 * (k - 1))) & 255u);
            if (last[p]) t[r][0] = t[r][1];
          }
          v[3 * p + k] = lin_vert(t[0][0] * xw0[p] + t[0][1] * xw1[p], t[1][0] * xw0[p] + t[1][1] * xw1[p], yw0, yw1);
        }
    } else {  // one source column: every tap is pixel 0 with the weights 2048 / 0
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[3 * p + k] = lin_vert(r0[k] * 2048, r1[k] * 2048, yw0, yw1);
    }
  }
  if (swap) {  // PHX_INGEST_BGR: channel c is read from 2 - c (every mode works per channel)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int r = v[3 * p];
      v[3 * p] = v[3 * p + 2];
      v[3 * p + 2] = r;
    }
  }
  if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) |
                                            ((uint32_t)v[4 * i + 2] << 16) | ((uint32_t)v[4 * i + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < 3 * n) dst[j] = (uint8_t)v[j];
  }
}

void launch_ingest(const uint8_t* src, uint8_t* out, const IngestFrame* frames_dev, int B, long max_lanes, bool bgr,
                   hipStream_t s) {
  if (max_lanes <= 0) return;
  hipLaunchKernelGGL(k_ingest, dim3((unsigned)cdiv(max_lanes, 256L), B), dim3(256), 0, s, src, out, frames_dev,
                     bgr ? 1 : 0);
  PHX_LAUNCH_CHECK();
}

}  // namespace phx
