// nms_seg_check.hpp — host reference, case table and seeded faults of the segmented-NMS parity checker
// (kernels_nms_seg.hip).  Everything here is host code: nms_seg_parity compares the device against it, and
// nms_seg_teeth shows that each seeded fault changes the reference's answer on at least one case of the table.
//
// The reference restates NonMaxSuppressionV5 [TF-recall] with a std::priority_queue (score descending, index
// ascending), per_class_nms' merge (postprocess.py:443-467) with a stable sort, and the global path's padded,
// clipped outputs.  IoU and the decay argument are made of basic fp32 operations (contraction off: build with
// -ffp-contract=off), so they are the same numbers on the host and on the device; expf is the one library
// function (g_expf), and the host's and the device's differ by an ulp on some arguments.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <limits>
#include <queue>
#include <string>
#include <vector>

namespace nsk {

constexpr int kRows = 100;  // rows of every output
constexpr float kNegInf = -std::numeric_limits<float>::infinity();

enum Fault {
  F_NONE,
  F_IOU_GE,            // sim >= iou_threshold suppresses (for >)
  F_TIE_HI,            // score ties popped by the higher index
  F_VISIT_OLDEST,      // a visit runs oldest selection first
  F_PC_CLIP,           // per-class boxes clipped to [0, image_size]
  F_MERGE_CLASS_DESC,  // merge ties go to the higher class
  F_VALID_UNCAPPED,    // valid_len = the classes' total, not capped at max_out
  F_COUNT
};
inline const char* fault_name(int f) {
  static const char* n[] = {"none", "iou_ge", "tie_hi", "visit_oldest", "pc_clip", "merge_class_desc", "valid_uncapped"};
  return n[f];
}

struct Params {
  float thresh, iou, sigma;
  int max_out;
};

inline float iou(const float* bi, const float* bj) {
  const float ymin_i = fminf(bi[0], bi[2]), xmin_i = fminf(bi[1], bi[3]);
  const float ymax_i = fmaxf(bi[0], bi[2]), xmax_i = fmaxf(bi[1], bi[3]);
  const float ymin_j = fminf(bj[0], bj[2]), xmin_j = fminf(bj[1], bj[3]);
  const float ymax_j = fmaxf(bj[0], bj[2]), xmax_j = fmaxf(bj[1], bj[3]);
  const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
  const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
  if (area_i <= 0.f || area_j <= 0.f) return 0.f;
  const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
  const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
  const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
  return inter / (area_i + area_j - inter);
}

// expf, the one library function of the decay: the parity checker replaces it with the device's own values (see
// nms_seg_parity.cpp), so that everything else is compared exactly
inline std::function<float(float)> g_expf = [](float x) { return expf(x); };

struct Sel {
  std::vector<int> idx;
  std::vector<float> sc;
  long pops = 0, requeues = 0, drops = 0;
};

// one segment: boxes [N,4], scores [N] of the image, cand = the segment's indices (any order)
inline Sel nms_v5(const float* boxes, const float* scores, const std::vector<int>& cand, const Params& q, Fault f = F_NONE) {
  struct Ent {
    float s;
    int i, from;
  };
  auto worse = [f](const Ent& a, const Ent& b) {  // a pops after b
    if (a.s != b.s) return a.s < b.s;
    return f == F_TIE_HI ? a.i < b.i : a.i > b.i;
  };
  std::priority_queue<Ent, std::vector<Ent>, decltype(worse)> pq(worse);
  for (int i : cand)
    if (scores[i] > q.thresh) pq.push(Ent{scores[i], i, 0});
  const bool soft = q.sigma > 0.f;
  const float scale = soft ? -0.5f / q.sigma : 0.f;
  Sel R;
  while ((int)R.idx.size() < q.max_out && !pq.empty()) {
    Ent e = pq.top();
    pq.pop();
    ++R.pops;
    const float orig = e.s;
    float sc = orig;
    bool hard = false;
    const int nsel = (int)R.idx.size();
    for (int v = 0; v < nsel - e.from; ++v) {
      const int j = f == F_VISIT_OLDEST ? e.from + v : nsel - 1 - v;
      const float sim = iou(boxes + (size_t)e.i * 4, boxes + (size_t)R.idx[j] * 4);
      const bool over = f == F_IOU_GE ? sim >= q.iou : sim > q.iou;
      if (soft) sc *= over ? 0.f : g_expf(scale * sim * sim);
      if (!soft && over) { hard = true; break; }
      if (sc <= q.thresh) break;
    }
    if (hard) { ++R.drops; continue; }
    if (sc == orig) {
      R.idx.push_back(e.i);
      R.sc.push_back(sc);
    } else if (sc > q.thresh) {
      ++R.requeues;
      pq.push(Ent{sc, e.i, nsel});
    }
  }
  return R;
}

struct Out {  // [B] images of kRows rows
  std::vector<float> boxes, scores, classes;
  std::vector<int> count, index;
  void init(int B) {
    boxes.assign((size_t)B * kRows * 4, 0.f);
    scores.assign((size_t)B * kRows, 0.f);
    classes.assign((size_t)B * kRows, 0.f);
    index.assign((size_t)B * kRows, -1);
    count.assign(B, 0);
  }
};

// nms(padded=True) + clip_boxes per image over the candidates i < count[b] (empty: N)
inline Out ref_global(const std::vector<float>& boxes, const std::vector<float>& scores, const std::vector<int>& count,
                      int B, int N, const Params& q, float clip_hi, Fault f = F_NONE) {
  Out o;
  o.init(B);
  for (int b = 0; b < B; ++b) {
    const int n = count.empty() ? N : std::min(std::max(count[b], 0), N);
    std::vector<int> cand(n);
    for (int i = 0; i < n; ++i) cand[i] = i;
    const float* bb = &boxes[(size_t)b * N * 4];
    const Sel s = nms_v5(bb, &scores[(size_t)b * N], cand, q, f);
    o.count[b] = (int)s.idx.size();
    for (size_t k = 0; k < s.idx.size(); ++k) {
      const size_t r = (size_t)b * kRows + k;
      for (int c = 0; c < 4; ++c) o.boxes[r * 4 + c] = fminf(fmaxf(bb[(size_t)s.idx[k] * 4 + c], 0.0f), clip_hi);
      o.scores[r] = s.sc[k];
      o.index[r] = s.idx[k];
    }
  }
  return o;
}

// per_class_nms per image; scales empty: boxes as they are
inline Out ref_per_class(const std::vector<float>& boxes, const std::vector<float>& scores, const std::vector<int>& classes,
                         const std::vector<int>& count, const std::vector<float>& scales, int B, int N, int C,
                         const Params& q, float clip_hi, Fault f = F_NONE) {
  Out o;
  o.init(B);
  struct Row {
    float s;
    int pos, cls, idx;  // idx < 0: one of tf.pad's rows
  };
  for (int b = 0; b < B; ++b) {
    const int n = count.empty() ? N : std::min(std::max(count[b], 0), N);
    const float* bb = &boxes[(size_t)b * N * 4];
    std::vector<Row> rows;
    for (int cid = 0; cid < C; ++cid) {
      std::vector<int> cand;
      for (int i = 0; i < n; ++i)
        if (classes[(size_t)b * N + i] == cid) cand.push_back(i);
      if (cand.empty()) continue;
      const Sel s = nms_v5(bb, &scores[(size_t)b * N], cand, q, f);
      for (size_t k = 0; k < s.idx.size(); ++k) rows.push_back(Row{s.sc[k], (int)rows.size(), cid, s.idx[k]});
    }
    const int total = (int)rows.size();
    for (int k = 0; k < q.max_out; ++k) rows.push_back(Row{0.f, (int)rows.size(), -1, -1});
    std::stable_sort(rows.begin(), rows.end(), [f](const Row& a, const Row& c) {
      if (a.s != c.s) return a.s > c.s;
      if (f == F_MERGE_CLASS_DESC && a.cls != c.cls) return a.cls > c.cls;
      return a.pos < c.pos;
    });
    const int valid = f == F_VALID_UNCAPPED ? std::min(total, kRows) : std::min(q.max_out, total);
    o.count[b] = valid;
    for (int k = 0; k < std::min(valid, (int)rows.size()); ++k) {
      const Row& r = rows[k];
      if (r.idx < 0) continue;
      const size_t w = (size_t)b * kRows + k;
      for (int c = 0; c < 4; ++c) {
        float v = bb[(size_t)r.idx * 4 + c];
        if (f == F_PC_CLIP) v = fminf(fmaxf(v, 0.0f), clip_hi);
        if (!scales.empty()) v = v * scales[b];
        o.boxes[w * 4 + c] = v;
      }
      o.scores[w] = r.s;
      o.classes[w] = (float)(r.cls + 1);
    }
  }
  return o;
}

// ---- cases -------------------------------------------------------------------------------------
enum Kind { K_SEG, K_GLOBAL, K_PC, K_REFUSE };
enum Gen {
  G_RANDOM,      // random boxes on a 512 canvas, distinct random scores in (0, 1)
  G_EQUAL,       // as random, every score 0.75
  G_DUP,         // every box appears four times
  G_ZERO_AREA,   // every third box has zero height or width
  G_FLIPPED,     // every second box has its corners swapped
  G_HALF,        // integer boxes: [0] and [1] at IoU exactly 0.5
  G_HALF_ULP,    // integer boxes: [0] and [1] at IoU 0.5 + 1 ulp
  G_SPARSE,      // small boxes on a wide grid: few overlaps (the large-N cases)
  G_OUTSIDE,     // random boxes reaching outside [0, image]: a clip would show
  G_TWIN_CLASSES // the same boxes and scores in two classes: decayed-score ties across classes
};
struct Case {
  std::string name;
  int kind = K_GLOBAL, gen = G_RANDOM;
  uint32_t seed = 1;
  int B = 1, N = 64, C = 1;
  Params q{0.001f, 0.5f, 0.f, 100};
  std::vector<int> counts;    // K_GLOBAL / K_PC: candidates per image (empty: N)
  std::vector<int> seg_size;  // K_SEG: the size of each of the B*C segments
  int classes_mode = 0;       // K_PC: 0 random in [0, C), 1 all class 3, 2 anchor i -> class i % C, 3 classes 0 and C-1 only
  int empty_image = -1;       // this image's scores all fall below the threshold
  bool scales = false;        // K_PC: image scales 1.5 + b
  bool yardstick = false;     // soft, IoU 1: also bit-equal to k_soft_nms
};

struct Data {
  std::vector<float> boxes, scores, scales;
  std::vector<int> classes, list, seg_off, seg_cnt;
};

struct Rng {
  uint64_t s;
  explicit Rng(uint32_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
  uint32_t next() {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return (uint32_t)(s >> 32);
  }
  float uni() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

inline Data make_data(const Case& c) {
  Data d;
  Rng r(c.seed);
  const size_t BN = (size_t)c.B * c.N;
  d.boxes.resize(BN * 4);
  d.scores.resize(BN);
  d.classes.assign(BN, 0);
  const float S = 512.f;
  for (int b = 0; b < c.B; ++b) {
    for (int i = 0; i < c.N; ++i) {
      float* bx = &d.boxes[((size_t)b * c.N + i) * 4];
      float y = r.uni() * S * 0.8f, x = r.uni() * S * 0.8f, h = 8.f + r.uni() * 120.f, w = 8.f + r.uni() * 120.f;
      if (c.gen == G_SPARSE) {
        y = (float)((i / 700) * 9 % 4000);
        x = (float)((i % 700) * 9);
        h = 6.f + r.uni() * 6.f;
        w = 6.f + r.uni() * 6.f;
      }
      if (c.gen == G_OUTSIDE) { y -= 60.f; x -= 60.f; h += 100.f; w += 100.f; }
      bx[0] = y; bx[1] = x; bx[2] = y + h; bx[3] = x + w;
      float s = 0.002f + 0.996f * r.uni();
      if (c.gen == G_EQUAL) s = 0.75f;
      if (c.gen == G_DUP && (i & 3)) {
        const float* src = &d.boxes[((size_t)b * c.N + (i & ~3)) * 4];
        for (int k = 0; k < 4; ++k) bx[k] = src[k];
      }
      if (c.gen == G_ZERO_AREA && i % 3 == 1) bx[i & 1 ? 2 : 3] = bx[i & 1 ? 0 : 1];
      if (c.gen == G_FLIPPED && (i & 1)) { std::swap(bx[0], bx[2]); std::swap(bx[1], bx[3]); }
      if (c.gen == G_TWIN_CLASSES && i >= c.N / 2) {
        const size_t j = (size_t)b * c.N + i - c.N / 2;
        for (int k = 0; k < 4; ++k) bx[k] = d.boxes[j * 4 + k];
        s = d.scores[j];
      }
      d.scores[(size_t)b * c.N + i] = s;
      int cls = r.below(std::max(1, c.C));
      if (c.classes_mode == 1) cls = std::min(3, c.C - 1);
      if (c.classes_mode == 2) cls = i % c.C;
      if (c.classes_mode == 3) cls = (i & 1) ? c.C - 1 : 0;
      if (c.gen == G_TWIN_CLASSES) cls = i >= c.N / 2 ? std::min(7, c.C - 1) : std::min(2, c.C - 1);
      d.classes[(size_t)b * c.N + i] = cls;
    }
    if (c.gen == G_HALF || c.gen == G_HALF_ULP) {
      // [0] the big box with the higher score; [1] nested: inter / area = 1/2 exactly, or 8380418 / 16760835 which
      // fp32 rounds to 0.5 + 1 ulp; the rest stay random but far away
      float* b0 = &d.boxes[(size_t)b * c.N * 4];
      const float h0 = c.gen == G_HALF ? 10.f : 4095.f, w0 = c.gen == G_HALF ? 10.f : 4093.f;
      const float h1 = c.gen == G_HALF ? 10.f : 4094.f, w1 = c.gen == G_HALF ? 5.f : 2047.f;
      b0[0] = 0; b0[1] = 0; b0[2] = h0; b0[3] = w0;
      d.scores[(size_t)b * c.N] = 0.99f;
      if (c.N > 1) {
        b0[4] = 0; b0[5] = 0; b0[6] = h1; b0[7] = w1;
        d.scores[(size_t)b * c.N + 1] = 0.98f;
      }
      for (int i = 2; i < c.N; ++i)
        for (int k = 0; k < 4; ++k) b0[(size_t)i * 4 + k] += 6000.f;
    }
    if (b == c.empty_image)
      for (int i = 0; i < c.N; ++i) d.scores[(size_t)b * c.N + i] = c.q.thresh > 0.f ? c.q.thresh * 0.5f : -1.f;
    if (c.scales) d.scales.push_back(1.5f + (float)b);
  }
  if (c.kind == K_SEG) {
    // image b's list: a shuffle of its indices; segment sizes from the table, packed one after another
    d.list.resize(BN);
    d.seg_off.resize((size_t)c.B * c.C);
    d.seg_cnt.resize((size_t)c.B * c.C);
    for (int b = 0; b < c.B; ++b) {
      int* l = &d.list[(size_t)b * c.N];
      for (int i = 0; i < c.N; ++i) l[i] = i;
      for (int i = c.N - 1; i > 0; --i) std::swap(l[i], l[r.below(i + 1)]);
      int off = 0;
      for (int s = 0; s < c.C; ++s) {
        const int want = c.seg_size.empty() ? c.N / c.C : c.seg_size[(size_t)(b * c.C + s) % c.seg_size.size()];
        const int n = std::min(want, c.N - off);
        d.seg_off[(size_t)b * c.C + s] = off;
        d.seg_cnt[(size_t)b * c.C + s] = n;
        off += n;
      }
    }
  }
  return d;
}

// ---- the table
inline std::vector<Case> table() {
  std::vector<Case> t;
  auto add = [&](const char* name, int kind, int gen, std::function<void(Case&)> more) {
    Case c;
    c.name = name; c.kind = kind; c.gen = gen; c.seed = 500 + (uint32_t)t.size();
    more(c);
    t.push_back(c);
  };
  const Params hard5{0.001f, 0.5f, 0.f, 100};
  // a. segment sizes 0, 1, max_out-1, max_out, max_out+1 (sparse boxes: every candidate survives), lists shuffled
  add("seg_sizes_mo7", K_SEG, G_SPARSE, [&](Case& c) { c.B = 2; c.N = 257; c.C = 6; c.q = hard5; c.q.max_out = 7; c.seg_size = {0, 1, 6, 7, 8, 0}; });
  add("seg_sizes_mo100", K_SEG, G_SPARSE, [&](Case& c) { c.B = 1; c.N = 3069; c.C = 5; c.q = hard5; c.seg_size = {99, 100, 101, 0, 1}; });
  add("seg_soft_shuffled", K_SEG, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 257; c.C = 3; c.q = {0.001f, 1.f, 0.25f, 100}; });
  // b. N 1, 63, 64, 65, 257, 3069, 49104; the LDS-resident limit of the keys and the chunk factor 2
  add("hard_n1", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 1; c.q = hard5; });
  add("hard_n63", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 63; c.q = hard5; });
  add("hard_n64", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 64; c.q = hard5; });
  add("hard_n65", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 65; c.q = hard5; });
  add("hard_n257", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 257; c.q = hard5; });
  add("hard_n3069_b3_empty_middle", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 3; c.N = 3069; c.q = hard5; c.empty_image = 1; });
  add("hard_n49104", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 49104; c.q = hard5; c.q.thresh = 0.9f; });
  add("hard_n20000_all_candidates_past_lds", K_GLOBAL, G_SPARSE, [&](Case& c) { c.N = 20000; c.q = hard5; c.q.thresh = kNegInf; });
  add("hard_n262208_chunk_factor_2", K_GLOBAL, G_SPARSE, [&](Case& c) { c.N = 262208; c.q = hard5; c.q.thresh = kNegInf; });
  add("hard_count_prefix_clamped", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 3; c.N = 1000; c.q = hard5; c.counts = {1500, 0, 600}; });
  // c. scores and geometry
  add("hard_equal_scores", K_GLOBAL, G_EQUAL, [&](Case& c) { c.B = 2; c.N = 257; c.q = hard5; });
  add("hard_duplicates", K_GLOBAL, G_DUP, [&](Case& c) { c.N = 256; c.q = hard5; });
  add("hard_zero_area", K_GLOBAL, G_ZERO_AREA, [&](Case& c) { c.N = 257; c.q = hard5; });
  add("hard_flipped", K_GLOBAL, G_FLIPPED, [&](Case& c) { c.N = 257; c.q = hard5; });
  // d. thresholds and settings
  add("hard_iou0", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 257; c.q = {0.001f, 0.f, 0.f, 100}; });
  add("hard_iou1", K_GLOBAL, G_DUP, [&](Case& c) { c.N = 256; c.q = {0.001f, 1.f, 0.f, 100}; });
  add("hard_iou_exactly_half_survives", K_GLOBAL, G_HALF, [&](Case& c) { c.N = 65; c.q = hard5; });
  add("hard_iou_half_plus_ulp_goes", K_GLOBAL, G_HALF_ULP, [&](Case& c) { c.N = 65; c.q = hard5; });
  add("hard_thresh_neg_inf", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 257; c.q = {kNegInf, 0.5f, 0.f, 100}; });
  add("hard_thresh_half", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 3069; c.q = {0.5f, 0.5f, 0.f, 100}; });
  add("hard_mo1", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 257; c.q = hard5; c.q.max_out = 1; });
  add("hard_mo7", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 257; c.q = hard5; c.q.max_out = 7; });
  add("soft_sigma025_n3069", K_GLOBAL, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 3069; c.q = {0.001f, 1.f, 0.25f, 100}; c.yardstick = true; });
  add("soft_sigma015_n257", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 257; c.q = {0.001f, 1.f, 0.15f, 100}; c.yardstick = true; });
  add("soft_sigma025_thresh_half_mo7", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 1000; c.q = {0.5f, 1.f, 0.25f, 7}; c.yardstick = true; });
  add("soft_sigma025_duplicates_equal", K_GLOBAL, G_DUP, [&](Case& c) { c.N = 256; c.q = {0.001f, 1.f, 0.25f, 100}; c.yardstick = true; });
  add("soft_sigma025_n49104", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 49104; c.q = {0.9f, 1.f, 0.25f, 100}; c.yardstick = true; });
  add("soft_sigma025_iou_half", K_GLOBAL, G_RANDOM, [&](Case& c) { c.N = 257; c.q = {0.001f, 0.5f, 0.25f, 100}; });
  // e. per class
  add("pc_one_class", K_PC, G_OUTSIDE, [&](Case& c) { c.B = 2; c.N = 257; c.C = 90; c.q = hard5; c.classes_mode = 1; c.scales = true; });
  add("pc_90_classes_one_each", K_PC, G_OUTSIDE, [&](Case& c) { c.N = 90; c.C = 90; c.q = hard5; c.classes_mode = 2; });
  add("pc_classes_0_and_89", K_PC, G_OUTSIDE, [&](Case& c) { c.B = 2; c.N = 257; c.C = 90; c.q = hard5; c.classes_mode = 3; c.scales = true; });
  add("pc_merge_drops_mo7", K_PC, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 1000; c.C = 90; c.q = hard5; c.q.max_out = 7; });
  add("pc_merge_drops_mo100", K_PC, G_SPARSE, [&](Case& c) { c.N = 3069; c.C = 90; c.q = hard5; c.scales = true; });
  add("pc_soft_twin_classes_ties", K_PC, G_TWIN_CLASSES, [&](Case& c) { c.N = 128; c.C = 90; c.q = {0.001f, 1.f, 0.25f, 100}; });
  add("pc_hard_equal_scores_ties", K_PC, G_EQUAL, [&](Case& c) { c.N = 257; c.C = 90; c.q = hard5; c.q.max_out = 7; });
  add("pc_b3_empty_middle", K_PC, G_OUTSIDE, [&](Case& c) { c.B = 3; c.N = 257; c.C = 90; c.q = hard5; c.empty_image = 1; c.scales = true; });
  add("pc_soft_n3069_count_prefix", K_PC, G_RANDOM, [&](Case& c) { c.B = 2; c.N = 3069; c.C = 90; c.q = {0.5f, 1.f, 0.25f, 100}; c.counts = {3000, 77}; });
  add("pc_few_below_mo_valid_len", K_PC, G_SPARSE, [&](Case& c) { c.N = 63; c.C = 90; c.q = hard5; });
  // f. refusals on the host: nothing is launched
  add("refuse_n_beyond_range", K_REFUSE, G_RANDOM, [&](Case& c) { c.N = 1 << 30; });
  add("refuse_max_out_101", K_REFUSE, G_RANDOM, [&](Case& c) { c.N = 64; c.q.max_out = 101; });
  return t;
}
// ---- end of the table

// the reference's outputs of a case under a fault, flattened for comparison
struct RefOut {
  Out out;                       // K_GLOBAL / K_PC
  std::vector<Sel> segs;         // K_SEG
};
inline RefOut run_ref(const Case& c, const Data& d, Fault f = F_NONE) {
  RefOut R;
  const float clip_hi = 512.f;
  if (c.kind == K_GLOBAL) R.out = ref_global(d.boxes, d.scores, c.counts, c.B, c.N, c.q, clip_hi, f);
  if (c.kind == K_PC) R.out = ref_per_class(d.boxes, d.scores, d.classes, c.counts, d.scales, c.B, c.N, c.C, c.q, clip_hi, f);
  if (c.kind == K_SEG)
    for (int s = 0; s < c.B * c.C; ++s) {
      const int b = s / c.C;
      std::vector<int> cand(d.list.begin() + (size_t)b * c.N + d.seg_off[s],
                            d.list.begin() + (size_t)b * c.N + d.seg_off[s] + d.seg_cnt[s]);
      R.segs.push_back(nms_v5(&d.boxes[(size_t)b * c.N * 4], &d.scores[(size_t)b * c.N], cand, c.q, f));
    }
  return R;
}
inline bool same(const RefOut& a, const RefOut& b) {
  if (a.segs.size() != b.segs.size()) return false;
  for (size_t s = 0; s < a.segs.size(); ++s)
    if (a.segs[s].idx != b.segs[s].idx || a.segs[s].sc != b.segs[s].sc) return false;
  return a.out.boxes == b.out.boxes && a.out.scores == b.out.scores && a.out.classes == b.out.classes &&
         a.out.count == b.out.count && a.out.index == b.out.index;
}

}  // namespace nsk
