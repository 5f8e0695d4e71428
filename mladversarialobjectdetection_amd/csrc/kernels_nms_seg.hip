// kernels_nms_seg.hip — segmented NonMaxSuppressionV5: the NMS settings k_soft_nms (kernels_post.hip) does not
// serve.  postprocess.nms (automl/efficientdet/tf2/postprocess.py:159-205) with method 'hard' (IoU threshold
// below 1, no decay) and per_class_nms (:409-467), one NMS per (image, class).
//
// A segment is a list of candidate indices into one image's boxes [N,4] and scores [N].  Per segment the op is
// TF's lazy priority queue [TF-recall], in fp32 with every operation rounded on its own:
//   * candidates: score > score_threshold;
//   * pop order: score descending, then index ascending (the queue key carries the candidate's index, so the
//     order of a segment's list does not matter);
//   * a popped candidate visits the selections made since its last visit, newest first: sim = IoU (tf_iou), the
//     score is multiplied by (sim <= iou_threshold ? exp(scale * sim * sim) : 0), scale = -0.5 / soft_nms_sigma;
//     with soft_nms_sigma == 0 the score is left alone and sim > iou_threshold drops the candidate outright;
//   * an unchanged score selects the candidate, a changed one still above the threshold re-queues it; the loop
//     stops at max_output_size selections.
// TF stops a visit at the first product <= score_threshold.  The full product decides the same: a candidate's
// score lies above the threshold, every factor lies in [0, 1], so a positive score only falls (once at or below
// the threshold it stays there) and a negative one only rises towards 0 (it never reaches a threshold below it).
//
// Kernels: k_seg_bucket (an image's candidates grouped by class, or one group per image), k_nms_seg (one
// workgroup per segment, the queue in wave 0, selections and queue keys in LDS), k_seg_gather (global: padded
// outputs, boxes clipped) and k_seg_merge (per class: the max_output_size best of an image's classes).
#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "common.hpp"
#include "kernels.hpp"
#include "post.hpp"

#pragma clang fp contract(off)

namespace phx {

namespace {

constexpr int kSegThreads = 256;
constexpr int kSegLdsBytes = 160 * 1024;
constexpr int kSegGroups = 64;  // group maxima (<= 64 groups of 64 chunks)
constexpr int kSegStride = PHX_MAX_OUT_DEV;  // a segment's rows in the selection scratch
constexpr int kSegFixed = kSegGroups * 8 + kSegStride * (16 + 4 + 4) + 64;
constexpr int kBucketThreads = 1024;
constexpr int kMergeThreads = 1024;
constexpr int kSegMaxClasses = 1024;

static_assert(kSegFixed % 16 == 0, "the key array after the fixed region stays 16-byte aligned");

// IoU exactly as k_soft_nms' tf_iou (and oracle/postprocess.py _iou): corners min/max-normalised, an area <= 0
// gives 0
__device__ __forceinline__ float seg_iou(float4 bi, float4 bj) {
  const float ymin_i = fminf(bi.x, bi.z), xmin_i = fminf(bi.y, bi.w);
  const float ymax_i = fmaxf(bi.x, bi.z), xmax_i = fmaxf(bi.y, bi.w);
  const float ymin_j = fminf(bj.x, bj.z), xmin_j = fminf(bj.y, bj.w);
  const float ymax_j = fmaxf(bj.x, bj.z), xmax_j = fmaxf(bj.y, bj.w);
  const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
  const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
  if (area_i <= 0.f || area_j <= 0.f) return 0.f;
  const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
  const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
  const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
  return inter / (area_i + area_j - inter);
}

// wave-wide maximum by DPP within 16-lane rows and readlane across them (as kernels_post.hip's)
__device__ __forceinline__ uint32_t seg_wave_max_u32(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, false));  // row_half_mirror
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, false));  // row_mirror
  const uint32_t a = max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16));
  const uint32_t c = max((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48));
  return max(a, c);
}

__device__ __forceinline__ uint64_t seg_wave_max_u64(uint64_t v) {
  const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
  const uint32_t mh = seg_wave_max_u32(hi);
  const uint32_t ml = seg_wave_max_u32(hi == mh ? lo : 0u);
  return ((uint64_t)mh << 32) | ml;
}

// a float as an unsigned integer of the same order (any sign; -0.0 counts as +0.0, which the float compares
// of TF's queue and of tf.math.top_k cannot tell apart)
__device__ __forceinline__ uint32_t seg_ord(float v) {
  const uint32_t b = __float_as_uint(v + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float seg_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// queue key: the higher score wins, then the lower index; 0 = not queued (no score > a threshold maps to 0)
__device__ __forceinline__ uint64_t seg_key(float score, int idx) {
  return ((uint64_t)seg_ord(score) << 32) | (uint32_t)~(uint32_t)idx;
}

// sc = orig * f(newest) * f(next) * ... (lane l holds the factor of selection nsel-1-l in f0 and of nsel-65-l in
// f1; lanes past the visit hold 1).  A factor of exactly 1 leaves the product as it is and is skipped.
__device__ __forceinline__ float seg_decay_chain(float orig, float f0, float f1) {
  float sc = orig;
  unsigned long long m0 = __ballot(f0 != 1.f), m1 = __ballot(f1 != 1.f);
  while (m0) {
    const int l = __ffsll(m0) - 1;
    m0 &= m0 - 1ull;
    sc *= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(f0), l));
  }
  while (m1) {
    const int l = __ffsll(m1) - 1;
    m1 &= m1 - 1ull;
    sc *= __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(f1), l));
  }
  return sc;
}

struct SegPlan {
  int m;         // chunk = 64*m positions
  int nchunk;    // chunks for N positions
  int ck_bytes;  // chunk-maxima region
  int cap;       // positions whose key / visit count live in LDS (the rest in global memory)
  int lds;       // dynamic LDS bytes
};

SegPlan seg_plan(int N) {
  SegPlan p;
  p.m = std::max(1, cdiv(N, 64L * 64 * kSegGroups));
  p.nchunk = cdiv(N, 64L * p.m);
  p.ck_bytes = (p.nchunk * 8 + 15) / 16 * 16;
  const int cap = (kSegLdsBytes - kSegFixed - p.ck_bytes) / 9 / 64 * 64;
  p.cap = std::max(0, std::min(cap, (N + 63) / 64 * 64));
  p.lds = (kSegFixed + p.ck_bytes + p.cap * 9 + 15) / 16 * 16;
  return p;
}

// ------------------------------------------------------------------------------------------
// One workgroup per image: the candidates (i < count[b], keep & mask, score > thresh) grouped by class into the
// image's list [N] — class c's group at seg_off[b*C+c], seg_cnt[b*C+c] entries.  classes == nullptr: one group.
// A class outside [0, C) belongs to no group (tf.equal(classes, cid) matches no cid).  Entries of a group land
// in any order: k_nms_seg's queue key carries the index.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBucketThreads) void k_seg_bucket(const float* __restrict__ scores,
                                                               const int* __restrict__ classes,
                                                               const int* __restrict__ count,
                                                               const uint8_t* __restrict__ keep, int keep_mask, int N,
                                                               int C, float thresh, int* __restrict__ list,
                                                               int* __restrict__ seg_off, int* __restrict__ seg_cnt) {
  extern __shared__ int bk_smem[];  // [C] counts, then [C] cursors
  int* s_cnt = bk_smem;
  int* s_cur = bk_smem + C;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* sb = scores + (long)b * N;
  const int* cb = classes ? classes + (long)b * N : nullptr;
  const uint8_t* kb = keep ? keep + (long)b * N : nullptr;
  const int n_in = count ? min(max(count[b], 0), N) : N;
  for (int c = t; c < C; c += kBucketThreads) s_cnt[c] = 0;
  __syncthreads();
  auto group_of = [&](int i) -> int {
    if (!(sb[i] > thresh)) return -1;
    if (kb && (kb[i] & keep_mask) == 0) return -1;
    if (!cb) return 0;
    const int c = cb[i];
    return c >= 0 && c < C ? c : -1;
  };
  for (int i = t; i < n_in; i += kBucketThreads) {
    const int g = group_of(i);
    if (g >= 0) atomicAdd(&s_cnt[g], 1);
  }
  __syncthreads();
  if (t == 0) {
    int off = 0;
    for (int c = 0; c < C; ++c) {
      s_cur[c] = off;
      seg_off[(long)b * C + c] = off;
      seg_cnt[(long)b * C + c] = s_cnt[c];
      off += s_cnt[c];  // <= n_in <= N: every position written below is inside the image's list
    }
  }
  __syncthreads();
  int* lst = list + (long)b * N;
  for (int i = t; i < n_in; i += kBucketThreads) {
    const int g = group_of(i);
    if (g >= 0) lst[atomicAdd(&s_cur[g], 1)] = i;
  }
}

// ------------------------------------------------------------------------------------------
// One workgroup per segment.  Queue keys (u64) and last-visit counts (u8) of the first `cap` positions live in
// LDS, of the rest in global memory; per-chunk maxima (chunks of 64*m positions) and per-group maxima (groups
// of 64 chunks) in LDS: a pop is one group scan, and its update one chunk and one group rescan.  The pop loop
// runs in wave 0 alone (no workgroup barriers); its state is wave-uniform.  An empty segment writes its count
// and returns.
// ------------------------------------------------------------------------------------------
template <bool HARD>
__global__ __launch_bounds__(kSegThreads) void k_nms_seg(const float* __restrict__ boxes,
                                                         const float* __restrict__ scores,
                                                         const int* __restrict__ list,
                                                         const int* __restrict__ seg_off, int* __restrict__ seg_cnt,
                                                         int C, int N, float thresh, float iou_t, float scale,
                                                         int max_out, int reset_cnt, uint64_t* __restrict__ gkey_all,
                                                         uint8_t* __restrict__ gwb_all, SegPlan pl,
                                                         int* __restrict__ out_idx, float* __restrict__ out_score,
                                                         int* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sg_smem[];
  const int seg = blockIdx.x, b = seg / C;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  uint64_t* s_ck = reinterpret_cast<uint64_t*>(sg_smem);
  uint64_t* s_gk = reinterpret_cast<uint64_t*>(sg_smem + pl.ck_bytes);
  float4* s_sel = reinterpret_cast<float4*>(s_gk + kSegGroups);
  float* s_sels = reinterpret_cast<float*>(s_sel + kSegStride);
  int* s_seli = reinterpret_cast<int*>(s_sels + kSegStride);
  int* s_misc = s_seli + kSegStride;
  uint64_t* s_key = reinterpret_cast<uint64_t*>(s_misc + 16);
  uint8_t* s_wb = reinterpret_cast<uint8_t*>(s_key + pl.cap);
  const int cap = pl.cap;

  if (t == 0) {
    const int off = seg_off ? min(max(seg_off[seg], 0), N) : 0;
    s_misc[0] = min(max(seg_cnt[seg], 0), N - off);
    s_misc[2] = off;
    s_misc[1] = 0;
  }
  __syncthreads();
  const int n = __builtin_amdgcn_readfirstlane(s_misc[0]);
  const int off = __builtin_amdgcn_readfirstlane(s_misc[2]);
  if (n == 0) {
    if (t == 0) out_cnt[seg] = 0;
    return;
  }
  if (reset_cnt && t == 0) seg_cnt[seg] = 0;  // a pre_nms candidate list is consumed: the next one appends from 0
  const float4* bb = reinterpret_cast<const float4*>(boxes) + (long)b * N;
  const float* sb = scores + (long)b * N;
  const int* lst = list + (long)b * N + off;
  uint64_t* gkey = gkey_all + (long)b * N + off;
  uint8_t* gwb = gwb_all + (long)b * N + off;

  // 1. queue keys
  for (int p = t; p < n; p += kSegThreads) {
    const int i = lst[p];
    uint64_t k = 0ull;
    if (i >= 0 && i < N) {
      const float sc = sb[i];
      if (sc > thresh) k = seg_key(sc, i);
    }
    if (p < cap) {
      s_key[p] = k;
      s_wb[p] = 0;
    } else {
      gkey[p] = k;
      gwb[p] = 0;
    }
  }
  __syncthreads();

  // 2. chunk and group maxima
  const int CH = 64 * pl.m;
  const int nch = (n + CH - 1) / CH;
  const int ngr = (nch + 63) / 64;
  // spilled keys / visit counts are re-read after wave 0 rewrote them: volatile (L1-bypassing) loads
  volatile const uint64_t* vgkey = gkey;
  volatile const uint8_t* vgwb = gwb;
  auto key_at = [&](int p) -> uint64_t { return p < cap ? s_key[p] : vgkey[p]; };
  for (int ch = wave; ch < nch; ch += kSegThreads / 64) {
    uint64_t v = 0;
    for (int j = 0; j < pl.m; ++j) {
      const int p = ch * CH + j * 64 + lane;
      if (p < n) {
        const uint64_t k = key_at(p);
        v = k > v ? k : v;
      }
    }
    v = seg_wave_max_u64(v);
    if (lane == 0) s_ck[ch] = v;
  }
  __syncthreads();
  for (int g = wave; g < ngr; g += kSegThreads / 64) {
    const int ch = g * 64 + lane;
    const uint64_t v = seg_wave_max_u64(ch < nch ? s_ck[ch] : 0ull);
    if (lane == 0) s_gk[g] = v;
  }
  __syncthreads();

  // 3. the lazy priority queue, wave 0 only
  if (wave == 0) {
    int nsel = 0;
    while (nsel < max_out) {
      const uint64_t gv0 = lane < ngr ? s_gk[lane] : 0ull;
      const uint64_t top = seg_wave_max_u64(gv0);
      if (top == 0ull) break;
      // the key is unique (it carries the index): its group, chunk and position by ballot
      const int g = __ffsll(__ballot(gv0 == top)) - 1;
      const int chl = g * 64 + lane;
      const uint64_t cv0 = chl < nch ? s_ck[chl] : 0ull;
      const int ch = g * 64 + __ffsll(__ballot(cv0 == top)) - 1;
      int c = -1;
      for (int j = 0; j < pl.m && c < 0; ++j) {
        const int p = ch * CH + j * 64 + lane;
        const unsigned long long hit = __ballot(p < n && key_at(p) == top);
        if (hit) c = ch * CH + j * 64 + __ffsll(hit) - 1;
      }
      if (c < 0) break;  // unreachable: the maxima are maxima of the keys
      const int idx = (int)~(uint32_t)top;
      const float orig = seg_unord((uint32_t)(top >> 32));
      const int from = c < cap ? (int)s_wb[c] : (int)vgwb[c];
      const float4 cb4 = bb[idx];
      // the selections since the last visit, newest first: lane l takes selection nsel-1-l (and nsel-65-l)
      const int nf = nsel - from;
      float f0 = 1.f, f1 = 1.f;
      bool over = false;
      if (lane < nf) {
        const float sim = seg_iou(cb4, s_sel[nsel - 1 - lane]);
        if constexpr (HARD) over = sim > iou_t;
        else f0 = sim <= iou_t ? expf(scale * sim * sim) : 0.f;
      }
      if (lane + 64 < nf) {
        const float sim = seg_iou(cb4, s_sel[nsel - 65 - lane]);
        if constexpr (HARD) over = over || sim > iou_t;
        else f1 = sim <= iou_t ? expf(scale * sim * sim) : 0.f;
      }
      float sc = orig;
      bool dropped = false;
      if constexpr (HARD) dropped = __ballot(over) != 0ull;
      else sc = seg_decay_chain(orig, f0, f1);
      uint64_t nk = 0ull;
      int wbnew = nsel;
      if (!dropped) {
        if (sc == orig) {
          if (lane == 0) {
            s_sel[nsel] = cb4;
            s_sels[nsel] = sc;
            s_seli[nsel] = idx;
          }
          ++nsel;
        } else if (sc > thresh) {
          nk = seg_key(sc, idx);
        }
      }
      if (lane == 0) {
        if (c < cap) {
          s_key[c] = nk;
          s_wb[c] = (uint8_t)wbnew;
        } else {
          gkey[c] = nk;
          gwb[c] = (uint8_t)wbnew;
        }
      }
      // rescan c's chunk (c's own key from registers) and its group
      uint64_t v = 0;
      for (int j = 0; j < pl.m; ++j) {
        const int p = ch * CH + j * 64 + lane;
        if (p < n) {
          const uint64_t k = p == c ? nk : key_at(p);
          v = k > v ? k : v;
        }
      }
      const uint64_t cmax = seg_wave_max_u64(v);
      uint64_t gv = chl == ch ? cmax : cv0;
      gv = seg_wave_max_u64(gv);
      if (lane == 0) {
        s_ck[ch] = cmax;
        s_gk[g] = gv;
      }
    }
    if (lane == 0) s_misc[1] = nsel;
  }
  __syncthreads();
  const int nsel = s_misc[1];
  for (int k = t; k < nsel; k += kSegThreads) {
    out_idx[(long)seg * kSegStride + k] = s_seli[k];
    out_score[(long)seg * kSegStride + k] = s_sels[k];
  }
  if (t == 0) out_cnt[seg] = nsel;
}

// ------------------------------------------------------------------------------------------
// global: nms(padded=True) + clip_boxes (postprocess.py:61-64, 402) of one segment per image, in the layout of
// k_soft_nms' outputs with rows of kSegStride: rows >= count are zero, their index -1
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_seg_gather(const float* __restrict__ boxes, const int* __restrict__ sel_idx,
                                                    const float* __restrict__ sel_score,
                                                    const int* __restrict__ sel_cnt, int N, float clip_hi,
                                                    float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                    int* __restrict__ out_count, int* __restrict__ out_index) {
  const int b = blockIdx.x, k = threadIdx.x;
  const int n = min(max(sel_cnt[b], 0), kSegStride);
  if (k == 0) out_count[b] = n;
  if (k >= kSegStride) return;
  const long o = (long)b * kSegStride + k;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float sc = 0.f;
  int idx = -1;
  if (k < n) {
    idx = min(max(sel_idx[o], 0), N - 1);
    const float4 s4 = reinterpret_cast<const float4*>(boxes)[(long)b * N + idx];
    v = make_float4(fminf(fmaxf(s4.x, 0.0f), clip_hi), fminf(fmaxf(s4.y, 0.0f), clip_hi),
                    fminf(fmaxf(s4.z, 0.0f), clip_hi), fminf(fmaxf(s4.w, 0.0f), clip_hi));
    sc = sel_score[o];
  }
  float* ob = out_boxes + o * 4;
  ob[0] = v.x; ob[1] = v.y; ob[2] = v.z; ob[3] = v.w;
  out_scores[o] = sc;
  if (out_index) out_index[o] = idx;
}

// rows at and beyond max_out of k_soft_nms' [B,100] outputs cleared, the count capped: the selections of the
// lazy queue are made one after another, so the first max_out of a run to 100 are the run to max_out
__global__ __launch_bounds__(128) void k_seg_truncate(float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                      int* __restrict__ out_count, int* __restrict__ out_index,
                                                      int max_out) {
  const int b = blockIdx.x, k = threadIdx.x;
  const int n = out_count[b];
  __syncthreads();
  if (k == 0 && n > max_out) out_count[b] = max_out;
  if (k >= max_out && k < kSegStride) {
    const long o = (long)b * kSegStride + k;
    float* ob = out_boxes + o * 4;
    ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
    out_scores[o] = 0.f;
    if (out_index) out_index[o] = -1;
  }
}

// ------------------------------------------------------------------------------------------
// per class: per_class_nms' merge (postprocess.py:443-467) of one image.  The classes' selections concatenated
// in class order and padded with max_out zero rows; tf.math.top_k(k = max_out) = score descending, ties to the
// lower position (a bitonic sort of (score, ~position) keys in LDS); valid_len = min(max_out, total).  Boxes x
// image_scale, not clipped; classes cid + 1 as float; rows at and beyond valid_len zero.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMergeThreads) void k_seg_merge(const float* __restrict__ boxes,
                                                             const int* __restrict__ sel_idx,
                                                             const float* __restrict__ sel_score,
                                                             const int* __restrict__ sel_cnt, int C, int N,
                                                             int max_out, int P, const float* __restrict__ scales,
                                                             float* __restrict__ out_boxes,
                                                             float* __restrict__ out_scores,
                                                             float* __restrict__ out_classes,
                                                             int* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mg_smem[];
  uint64_t* s_k = reinterpret_cast<uint64_t*>(mg_smem);  // [P]
  int* s_pre = reinterpret_cast<int*>(s_k + P);           // [C + 1]
  const int b = blockIdx.x, t = threadIdx.x;
  if (t == 0) {
    int tot = 0;
    for (int c = 0; c < C; ++c) {
      s_pre[c] = tot;
      tot += min(max(sel_cnt[(long)b * C + c], 0), max_out);
    }
    s_pre[C] = tot;
  }
  __syncthreads();
  const int total = s_pre[C];
  int Pk = 2;
  while (Pk < total + max_out) Pk <<= 1;  // <= P: total <= C * max_out (launcher)
  auto class_of = [&](int e) -> int {  // the class whose rows hold position e < total
    int lo = 0, hi = C;                // s_pre[lo] <= e < s_pre[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_pre[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
  };
  for (int e = t; e < Pk; e += kMergeThreads) {
    uint64_t k = 0ull;
    if (e < total) {
      const int c = class_of(e);
      k = seg_key(sel_score[((long)b * C + c) * kSegStride + (e - s_pre[c])], e);
    } else if (e < total + max_out) {
      k = seg_key(0.0f, e);  // tf.pad's rows
    }
    s_k[e] = k;
  }
  __syncthreads();
  for (int k = 2; k <= Pk; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < Pk; i += kMergeThreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = s_k[i], c = s_k[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? a < c : a > c) {
            s_k[i] = c;
            s_k[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  const int valid = min(max_out, total);
  if (t == 0) out_count[b] = valid;
  const float scale = scales ? scales[b] : 1.0f;
  for (int r = t; r < kSegStride; r += kMergeThreads) {
    const long o = (long)b * kSegStride + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    float sc = 0.f, cl = 0.f;
    if (r < valid) {
      const int e = (int)~(uint32_t)s_k[r];
      if (e < total) {  // else one of the pad rows (it outranks a negative score): zeros
        const int c = class_of(e);
        const long q = ((long)b * C + c) * kSegStride + (e - s_pre[c]);
        const int idx = min(max(sel_idx[q], 0), N - 1);
        v = reinterpret_cast<const float4*>(boxes)[(long)b * N + idx];
        if (scales) v = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
        sc = sel_score[q];
        cl = (float)(c + 1);
      }
    }
    float* ob = out_boxes + o * 4;
    ob[0] = v.x; ob[1] = v.y; ob[2] = v.z; ob[3] = v.w;
    out_scores[o] = sc;
    out_classes[o] = cl;
  }
}

int merge_sort_size(int C, int max_out) {
  int P = 2;
  while (P < C * max_out + max_out) P <<= 1;
  return P;
}

// the scratch of one call carved from `work` (nms_seg_work_floats): spilled keys [B][N] u64 | image lists
// [B][N] | segment offsets, counts [B*C] | selections [B*C][kSegStride] index, score | counts [B*C] |
// visit counts [B][N] bytes
struct SegWork {
  uint64_t* gkey;
  int *list, *off, *cnt, *sel_idx;
  float* sel_score;
  int* sel_cnt;
  uint8_t* gwb;
};
SegWork seg_work(float* work, int B, int N, int C) {
  const size_t BN = (size_t)B * N, S = (size_t)B * C;
  SegWork w;
  w.gkey = reinterpret_cast<uint64_t*>(work);
  float* p = work + 2 * BN;
  w.list = reinterpret_cast<int*>(p); p += BN;
  w.off = reinterpret_cast<int*>(p); p += S;
  w.cnt = reinterpret_cast<int*>(p); p += S;
  w.sel_idx = reinterpret_cast<int*>(p); p += S * kSegStride;
  w.sel_score = p; p += S * kSegStride;
  w.sel_cnt = reinterpret_cast<int*>(p); p += S;
  w.gwb = reinterpret_cast<uint8_t*>(p);
  return w;
}

void check_params(const NmsSegParams& q, int B, int N, int C) {
  if (B < 1 || C < 1 || C > kSegMaxClasses) throw std::invalid_argument("nms_seg: B < 1 or classes outside [1, 1024]");
  if (!nms_seg_accepts(N)) throw std::runtime_error("nms_seg: too many candidates");
  if (q.max_out < 1 || q.max_out > PHX_MAX_OUT_DEV) throw std::runtime_error("nms_seg: max_out outside [1, 100]");
  if (!(q.soft_sigma >= 0.f)) throw std::invalid_argument("nms_seg: soft_nms_sigma < 0");
  if (std::isnan(q.iou_thresh) || std::isnan(q.score_thresh)) throw std::invalid_argument("nms_seg: NaN threshold");
}

void launch_seg_kernel(const float* boxes, const float* scores, const int* list, const int* seg_off, int* seg_cnt,
                       int nseg, int C, int N, const NmsSegParams& q, int reset_cnt, uint64_t* gkey, uint8_t* gwb,
                       int* sel_idx, float* sel_score, int* sel_cnt, hipStream_t s) {
  const SegPlan pl = seg_plan(N);
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nms_seg<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kSegLdsBytes) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nms_seg<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kSegLdsBytes) == hipSuccess;
  }();
  (void)attr;
  // TF: is_soft_nms = soft_nms_sigma > 0, scale = -0.5 / soft_nms_sigma
  if (q.soft_sigma > 0.f) {
    const float scale = -0.5f / q.soft_sigma;
    hipLaunchKernelGGL(k_nms_seg<false>, dim3(nseg), dim3(kSegThreads), pl.lds, s, boxes, scores, list, seg_off,
                       seg_cnt, C, N, q.score_thresh, q.iou_thresh, scale, q.max_out, reset_cnt, gkey, gwb, pl,
                       sel_idx, sel_score, sel_cnt);
  } else {
    hipLaunchKernelGGL(k_nms_seg<true>, dim3(nseg), dim3(kSegThreads), pl.lds, s, boxes, scores, list, seg_off,
                       seg_cnt, C, N, q.score_thresh, q.iou_thresh, 0.f, q.max_out, reset_cnt, gkey, gwb, pl,
                       sel_idx, sel_score, sel_cnt);
  }
  PHX_LAUNCH_CHECK();
}

}  // namespace

bool nms_seg_accepts(int N) { return N >= 1 && soft_nms_accepts(N); }

size_t nms_seg_work_floats(int B, int N, int C) {
  const size_t BN = (size_t)B * N, S = (size_t)B * C;
  return 3 * BN + 3 * S + 2 * S * kSegStride + (BN + 3) / 4 + 4;
}

NmsSegPlanInfo nms_seg_plan_info(int N) {
  const SegPlan p = seg_plan(N);
  return NmsSegPlanInfo{p.m, p.nchunk, p.cap, p.lds, kSegThreads};
}

void launch_nms_seg_raw(const float* boxes, const float* scores, const int* list, const int* seg_off,
                        const int* seg_cnt, int B, int C, int N, const NmsSegParams& q, int* sel_idx,
                        float* sel_score, int* sel_cnt, float* work, hipStream_t s) {
  check_params(q, B, N, C);
  const SegWork w = seg_work(work, B, N, C);
  launch_seg_kernel(boxes, scores, list, seg_off, const_cast<int*>(seg_cnt), B * C, C, N, q, 0, w.gkey, w.gwb,
                    sel_idx, sel_score, sel_cnt, s);
}

void launch_nms_seg_global(const float* boxes, const float* scores, const uint8_t* keep, int keep_mask,
                           const int* count, int B, int N, const NmsSegParams& q, float clip_hi, float* out_boxes,
                           float* out_scores, int* out_count, float* work, hipStream_t s, NmsCand cand,
                           int* out_index) {
  check_params(q, B, N, 1);
  const SegWork w = seg_work(work, B, N, 1);
  if (cand.list) {
    // pre_nms appended the candidates (keep & mask and score > thresh applied); the kernel resets the counts
    launch_seg_kernel(boxes, scores, cand.list, nullptr, cand.count, B, 1, N, q, 1, w.gkey, w.gwb, w.sel_idx,
                      w.sel_score, w.sel_cnt, s);
  } else {
    hipLaunchKernelGGL(k_seg_bucket, dim3(B), dim3(kBucketThreads), 2 * sizeof(int), s, scores, nullptr, count, keep,
                       keep_mask, N, 1, q.score_thresh, w.list, w.off, w.cnt);
    PHX_LAUNCH_CHECK();
    launch_seg_kernel(boxes, scores, w.list, w.off, w.cnt, B, 1, N, q, 0, w.gkey, w.gwb, w.sel_idx, w.sel_score,
                      w.sel_cnt, s);
  }
  hipLaunchKernelGGL(k_seg_gather, dim3(B), dim3(128), 0, s, boxes, w.sel_idx, w.sel_score, w.sel_cnt, N, clip_hi,
                     out_boxes, out_scores, out_count, out_index);
  PHX_LAUNCH_CHECK();
}

void launch_nms_seg_per_class(const float* boxes, const float* scores, const int* classes, const int* count, int B,
                              int N, int C, const NmsSegParams& q, const float* scales, float* out_boxes,
                              float* out_scores, float* out_classes, int* out_count, float* work, hipStream_t s) {
  check_params(q, B, N, C);
  if (!classes) throw std::invalid_argument("nms_seg: per-class needs classes");
  const int P = merge_sort_size(C, q.max_out);
  const size_t merge_lds = (size_t)P * 8 + (size_t)(C + 1) * 4;
  if (merge_lds > (size_t)kSegLdsBytes) throw std::runtime_error("nms_seg: too many classes for the merge");
  const SegWork w = seg_work(work, B, N, C);
  hipLaunchKernelGGL(k_seg_bucket, dim3(B), dim3(kBucketThreads), 2 * C * sizeof(int), s, scores, classes, count,
                     nullptr, 0, N, C, q.score_thresh, w.list, w.off, w.cnt);
  PHX_LAUNCH_CHECK();
  launch_seg_kernel(boxes, scores, w.list, w.off, w.cnt, B * C, C, N, q, 0, w.gkey, w.gwb, w.sel_idx, w.sel_score,
                    w.sel_cnt, s);
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_seg_merge),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kSegLdsBytes) == hipSuccess;
  }();
  (void)attr;
  hipLaunchKernelGGL(k_seg_merge, dim3(B), dim3(kMergeThreads), merge_lds, s, boxes, w.sel_idx, w.sel_score,
                     w.sel_cnt, C, N, q.max_out, P, scales, out_boxes, out_scores, out_classes, out_count);
  PHX_LAUNCH_CHECK();
}

void launch_nms_truncate(float* out_boxes, float* out_scores, int* out_count, int* out_index, int B, int max_out,
                         hipStream_t s) {
  if (max_out < 1 || max_out > PHX_MAX_OUT_DEV) throw std::runtime_error("nms_truncate: max_out outside [1, 100]");
  if (max_out == PHX_MAX_OUT_DEV) return;
  hipLaunchKernelGGL(k_seg_truncate, dim3(B), dim3(128), 0, s, out_boxes, out_scores, out_count, out_index, max_out);
  PHX_LAUNCH_CHECK();
}

}  // namespace phx
