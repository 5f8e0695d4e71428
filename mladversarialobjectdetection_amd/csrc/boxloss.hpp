// boxloss.hpp — launchers of the box-regression attack term (kernels_boxloss.hip): the reference's
// InverseDIOULoss (regression_loss.py:16-142) over the second pass's kept anchors and the boxes the
// patches were placed by, and its sparse gradient into the box head.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

namespace phx {

// anchors per workgroup of k_idiou_part (four per lane) and the chunk count for A anchors
constexpr int kIdiouChunk = 1024;
constexpr int kIdiouMaxGt = 100;  // PHX_MAX_OUT: gt slots per image
inline int idiou_chunks(int A) { return (A + kIdiouChunk - 1) / kIdiouChunk; }
// ints of scratch: per (image, chunk, gt) a maximum, its lowest anchor and its tie count
inline size_t idiou_scratch_ints(int B, int A) { return (size_t)B * idiou_chunks(A) * kIdiouMaxGt * 3; }

// boxes [B,A,4] decoded (ymin,xmin,ymax,xmax), keep [B,A] (bit 0: in the predicted set), gt [B,100,4],
// gcount [B].  Outputs: gt_max / gt_anchor / gt_nties [B,100] (slots at or past gcount[b], and every slot
// of an image without a kept anchor: 0, -1, 0), per_image [B] (sum over gts + 1e-7), batch [1].
// metrics (optional): metrics[PHX_M_LOSS] += weight * batch.
void launch_idiou(const float* boxes, const uint8_t* keep, const float* gt, const int* gcount, int B, int A,
                  float* gt_max, int* gt_anchor, int* gt_nties, float* per_image, float* batch, int* scratch,
                  float weight, float* metrics, hipStream_t s);

// For every (image, gt) winner (every tied anchor, each with 1 / nties): weight * d diou / d box through
// decode_box_outputs into the four box logits, and from there dx[pixel, :] += W[:, k*4 + j] * dt_j, the
// input gradient of the box-predict pointwise conv (wpred [K][na*4]; dx_off[l]: level l's offset in dx_base).
// box_base + lev[l].box_off: level l's box logits [B,h,w,na*4] (fp32).
void launch_box_scatter(const float* boxes, const uint8_t* keep, const float* gt, const int* gcount,
                        const float* gt_max, const int* gt_anchor, const int* gt_nties, const float* box_base,
                        const float* anchors, const LevelDesc* lev, int nlev, int A, int B, int na,
                        const float* wpred, int K, float weight, float* dx_base, const long* dx_off,
                        hipStream_t s);

}  // namespace phx
