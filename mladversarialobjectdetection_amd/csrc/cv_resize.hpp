// cv_resize.hpp — cv2.resize's 8-bit INTER_LINEAR tap (oracle/adv_patch.py::_linear_tabs / _linear_vtabs),
// shared by the inference compositor's Y sum (kernels_advpatch.hip) and the stream ingest
// (kernels_ingest.hip).  Every multiply and add rounds on its own: a translation unit that includes
// this is compiled with -ffp-contract=off (csrc/Makefile).
#pragma once

#include <hip/hip_runtime.h>

namespace phx {

// saturate_cast<short>(float): round half to even
__device__ __forceinline__ int round_short(float x) { return (int)rintf(x); }

// INTER_LINEAR tap of destination index d (resize(): fx in float32 from a double expression); scale =
// 1 / (dsize / ssize) in double.  -> source index s and the 11-bit weights of s and s + 1; clamp: the
// horizontal table's clamping of s to [0, ssize - 1] with the weight moved onto it (the vertical pass
// clamps its rows, not its weights)
__device__ __forceinline__ void lin_tap(int d, double scale, int ssize, bool clamp, int* s, int* w0, int* w1) {
  const float f0 = (float)__dadd_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), -0.5);
  int sx = (int)floorf(f0);
  float f = __fadd_rn(f0, -(float)sx);
  if (clamp) {
    if (sx < 0) { f = 0.f; sx = 0; }
    if (sx >= ssize - 1) { f = 0.f; sx = ssize - 1; }
  }
  *s = sx;
  *w0 = round_short(__fmul_rn(__fadd_rn(1.f, -f), 2048.f));
  *w1 = round_short(__fmul_rn(f, 2048.f));
}

// the vertical pass over two horizontally interpolated int rows (VResizeLinear's 8-bit form)
__device__ __forceinline__ int lin_vert(int s0, int s1, int b0, int b1) {
  return (((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2;
}

}  // namespace phx
