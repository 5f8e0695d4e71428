// nms_seg_parity — kernel-level parity of the segmented NonMaxSuppressionV5 (kernels_nms_seg.hip) against the host
// reference of nms_seg_check.hpp: selected indices, scores, boxes, classes and counts compared exactly.
//
//   nms_seg_parity --plan   the case table with each case's geometry, the kernel's launch plan for its N (chunk
//                           factor, chunks, LDS-resident positions, LDS bytes) and the reference's pops, re-queues and
//                           hard drops (no GPU is touched)
//   nms_seg_parity          run the table on the GPU: one flushed JSON line per case, then a `done` line
//
// Only the launchers of kernels.hpp are called, on one stream (and k_expf below: the device's expf for the
// reference).  A soft case at IoU threshold 1 also runs k_soft_nms (launch_soft_nms) on the same inputs: bit-equal
// (the yardstick).  The exit status is 0 when every case ran (the verdicts are in the lines); a HIP error ends the
// process at once with a `fatal` line and status 3.
// Build: make -C tests/kernels_nms_seg.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "nms_seg_check.hpp"

using namespace nsk;
using namespace phx;

static const char* g_case = "";
[[noreturn]] static void fatal(const char* what) {
  printf("{\"fatal\":\"%s\",\"case\":\"%s\"}\n", what, g_case);
  fflush(stdout);
  _Exit(3);  // nothing further is launched after a HIP error
}
#define CK(expr)                                        \
  do {                                                  \
    const hipError_t e_ = (expr);                       \
    if (e_ != hipSuccess) fatal(hipGetErrorString(e_)); \
  } while (0)

struct Buf {
  void* d = nullptr;
  size_t bytes = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { if (d) (void)hipFree(d); }
  void alloc(size_t n, int fill = 0xCD) {
    bytes = std::max<size_t>(n, 16);
    CK(hipMalloc(&d, bytes));
    CK(hipMemset(d, fill, bytes));
  }
  template <class T> void put(const std::vector<T>& v) {
    alloc(v.size() * sizeof(T));
    if (!v.empty()) CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  template <class T> std::vector<T> get(size_t n) const {
    std::vector<T> v(n);
    if (n) CK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
  }
  template <class T> T* as() const { return static_cast<T*>(d); }
};

// The device's expf for the reference.  The decay argument scale * iou * iou depends on a pair of boxes alone, not on
// the queue's state, so the reference runs with a cache of device values: an argument it has not seen is answered by
// the host's expf and noted, the noted arguments are evaluated on the device (one launch of the kernel below), and the
// reference runs again until it meets no new argument.  What the checker then compares exactly is everything but
// expf's own rounding, whose error tests/kernels' post_parity measures.
__global__ void k_expf(const float* x, float* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = expf(x[i]);
}
static std::map<uint32_t, float> g_exp_cache;
static std::vector<float> g_exp_miss;
static float cached_expf(float x) {
  uint32_t k;
  memcpy(&k, &x, 4);
  const auto it = g_exp_cache.find(k);
  if (it != g_exp_cache.end()) return it->second;
  g_exp_miss.push_back(x);
  return expf(x);
}
static int fill_exp_cache(hipStream_t s) {
  const int n = (int)g_exp_miss.size();
  if (!n) return 0;
  Buf x, y;
  x.put(g_exp_miss);
  y.alloc((size_t)n * 4);
  hipLaunchKernelGGL(k_expf, dim3((n + 255) / 256), dim3(256), 0, s, x.as<float>(), y.as<float>(), n);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(s));
  const std::vector<float> v = y.get<float>(n);
  for (int i = 0; i < n; ++i) {
    uint32_t k;
    memcpy(&k, &g_exp_miss[i], 4);
    g_exp_cache[k] = v[i];
  }
  g_exp_miss.clear();
  return n;
}
static RefOut run_ref_dev_exp(const Case& c, const Data& d, hipStream_t s, int* rounds) {
  g_expf = cached_expf;
  g_exp_cache.clear();
  g_exp_miss.clear();
  RefOut r;
  for (*rounds = 1;; ++*rounds) {
    r = run_ref(c, d);
    if (!fill_exp_cache(s)) break;
    if (*rounds > 50) fatal("the reference keeps meeting new expf arguments");
  }
  return r;
}

static NmsSegParams to_dev(const Params& q) { return NmsSegParams{q.thresh, q.iou, q.sigma, q.max_out}; }

static std::string jnum(double v) {
  char b[64];
  if (std::isinf(v)) return v < 0 ? "\"-inf\"" : "\"inf\"";
  snprintf(b, sizeof b, "%.9g", v);
  return b;
}

static void plan() {
  for (const Case& c : table()) {
    const NmsSegPlanInfo p = c.kind == K_REFUSE ? NmsSegPlanInfo{} : nms_seg_plan_info(c.N);
    long pops = 0, req = 0, drops = 0, sel = 0;
    if (c.kind != K_REFUSE) {
      const Data d = make_data(c);
      if (c.kind == K_SEG) {
        for (const Sel& s : run_ref(c, d).segs) { pops += s.pops; req += s.requeues; drops += s.drops; sel += (long)s.idx.size(); }
      } else {
        const RefOut r = run_ref(c, d);
        for (int v : r.out.count) sel += v;
        if (c.kind == K_GLOBAL)
          for (int b = 0; b < c.B; ++b) {
            const int n = c.counts.empty() ? c.N : std::min(std::max(c.counts[b], 0), c.N);
            std::vector<int> cand(n);
            for (int i = 0; i < n; ++i) cand[i] = i;
            const Sel s = nms_v5(&d.boxes[(size_t)b * c.N * 4], &d.scores[(size_t)b * c.N], cand, c.q);
            pops += s.pops; req += s.requeues; drops += s.drops;
          }
      }
    }
    printf("{\"case\":\"%s\",\"kind\":%d,\"B\":%d,\"N\":%d,\"C\":%d,\"thresh\":%s,\"iou\":%s,\"sigma\":%s,\"max_out\":%d,"
           "\"plan_m\":%d,\"plan_chunks\":%d,\"plan_lds_positions\":%d,\"plan_lds_bytes\":%d,\"ref_selected\":%ld,"
           "\"ref_pops\":%ld,\"ref_requeues\":%ld,\"ref_hard_drops\":%ld,\"yardstick\":%s}\n",
           c.name.c_str(), c.kind, c.B, c.N, c.C, jnum(c.q.thresh).c_str(), jnum(c.q.iou).c_str(), jnum(c.q.sigma).c_str(),
           c.q.max_out, p.m, p.nchunk, p.cap, p.lds, sel, pops, req, drops, c.yardstick ? "true" : "false");
  }
}

template <class T>
static long diff(const std::vector<T>& a, const std::vector<T>& b) {
  if (a.size() != b.size()) return -1;
  long n = 0;
  for (size_t i = 0; i < a.size(); ++i) n += memcmp(&a[i], &b[i], sizeof(T)) != 0;
  return n;
}

static void run_case(const Case& c, hipStream_t s) {
  g_case = c.name.c_str();
  if (c.kind == K_REFUSE) {
    // the launcher throws on the host; no buffer is needed because nothing may be launched
    bool threw = false;
    try {
      launch_nms_seg_global(nullptr, nullptr, nullptr, 0, nullptr, 1, c.N, to_dev(c.q), 512.f, nullptr, nullptr, nullptr,
                            nullptr, s);
    } catch (const std::exception&) {
      threw = true;
    }
    bool threw_pc = false;
    try {
      launch_nms_seg_per_class(nullptr, nullptr, nullptr, nullptr, 1, c.N, 90, to_dev(c.q), nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, s);
    } catch (const std::exception&) {
      threw_pc = true;
    }
    CK(hipStreamSynchronize(s));
    printf("{\"case\":\"%s\",\"ok\":%s,\"threw_global\":%s,\"threw_per_class\":%s}\n", c.name.c_str(),
           threw && threw_pc ? "true" : "false", threw ? "true" : "false", threw_pc ? "true" : "false");
    fflush(stdout);
    return;
  }
  const Data d = make_data(c);
  int exp_rounds = 0;
  const RefOut ref = run_ref_dev_exp(c, d, s, &exp_rounds);
  Buf boxes, scores, classes, count, scales, work, list, off, cnt;
  boxes.put(d.boxes);
  scores.put(d.scores);
  if (!c.counts.empty()) count.put(c.counts);
  work.alloc(nms_seg_work_floats(c.B, c.N, c.C) * 4);
  const size_t R = (size_t)c.B * kRows;
  long bad_boxes = 0, bad_scores = 0, bad_classes = 0, bad_count = 0, bad_index = 0, bad_yard = 0;
  bool yard_run = false;
  if (c.kind == K_SEG) {
    list.put(d.list);
    off.put(d.seg_off);
    cnt.put(d.seg_cnt);
    const size_t nseg = (size_t)c.B * c.C;
    Buf si, ss, sc;
    si.alloc(nseg * kRows * 4);
    ss.alloc(nseg * kRows * 4);
    sc.alloc(nseg * 4);
    launch_nms_seg_raw(boxes.as<float>(), scores.as<float>(), list.as<int>(), off.as<int>(), cnt.as<int>(), c.B, c.C, c.N,
                       to_dev(c.q), si.as<int>(), ss.as<float>(), sc.as<int>(), work.as<float>(), s);
    CK(hipStreamSynchronize(s));
    const std::vector<int> gi = si.get<int>(nseg * kRows), gc = sc.get<int>(nseg);
    const std::vector<float> gs = ss.get<float>(nseg * kRows);
    for (size_t g = 0; g < nseg; ++g) {
      const Sel& r = ref.segs[g];
      if (gc[g] != (int)r.idx.size()) { ++bad_count; continue; }
      for (size_t k = 0; k < r.idx.size(); ++k) {
        bad_index += gi[g * kRows + k] != r.idx[k];
        bad_scores += memcmp(&gs[g * kRows + k], &r.sc[k], 4) != 0;
      }
    }
    // the inputs the kernel may not write: the lists and their counts
    bad_index += diff(list.get<int>(d.list.size()), d.list) + diff(cnt.get<int>(nseg), d.seg_cnt);
  } else {
    Buf ob, os, ocl, oc, oi;
    ob.alloc(R * 16);
    os.alloc(R * 4);
    ocl.alloc(R * 4);
    oc.alloc((size_t)c.B * 4);
    oi.alloc(R * 4);
    if (c.kind == K_GLOBAL) {
      launch_nms_seg_global(boxes.as<float>(), scores.as<float>(), nullptr, 0, c.counts.empty() ? nullptr : count.as<int>(),
                            c.B, c.N, to_dev(c.q), 512.f, ob.as<float>(), os.as<float>(), oc.as<int>(), work.as<float>(), s,
                            NmsCand{}, oi.as<int>());
    } else {
      classes.put(d.classes);
      if (c.scales) scales.put(d.scales);
      launch_nms_seg_per_class(boxes.as<float>(), scores.as<float>(), classes.as<int>(),
                               c.counts.empty() ? nullptr : count.as<int>(), c.B, c.N, c.C, to_dev(c.q),
                               c.scales ? scales.as<float>() : nullptr, ob.as<float>(), os.as<float>(), ocl.as<float>(),
                               oc.as<int>(), work.as<float>(), s);
    }
    CK(hipStreamSynchronize(s));
    bad_boxes = diff(ob.get<float>(R * 4), ref.out.boxes);
    bad_scores = diff(os.get<float>(R), ref.out.scores);
    bad_count = diff(oc.get<int>(c.B), ref.out.count);
    if (c.kind == K_GLOBAL) bad_index = diff(oi.get<int>(R), ref.out.index);
    if (c.kind == K_PC) bad_classes = diff(ocl.get<float>(R), ref.out.classes);
    if (c.yardstick && c.q.max_out == kRows) {
      // k_soft_nms on the same inputs: every output bit-equal to the segmented kernel's
      yard_run = true;
      Buf yb, ys, yc, yi, yw;
      yb.alloc(R * 16);
      ys.alloc(R * 4);
      yc.alloc((size_t)c.B * 4);
      yi.alloc(R * 4);
      yw.alloc(soft_nms_work_floats(c.B, c.N) * 4);
      launch_soft_nms(boxes.as<float>(), scores.as<float>(), nullptr, 0, c.counts.empty() ? nullptr : count.as<int>(), c.B,
                      c.N, c.q.thresh, c.q.sigma, kRows, 512.f, yb.as<float>(), ys.as<float>(), yc.as<int>(),
                      yw.as<float>(), s, NmsCand{}, yi.as<int>());
      CK(hipStreamSynchronize(s));
      bad_yard = diff(yb.get<float>(R * 4), ob.get<float>(R * 4)) + diff(ys.get<float>(R), os.get<float>(R)) +
                 diff(yc.get<int>(c.B), oc.get<int>(c.B)) + diff(yi.get<int>(R), oi.get<int>(R));
    } else if (c.yardstick) {
      // max_out below 100: k_soft_nms run to 100 and cut (launch_nms_truncate), as the library's run_nms does
      yard_run = true;
      Buf yb, ys, yc, yi, yw;
      yb.alloc(R * 16);
      ys.alloc(R * 4);
      yc.alloc((size_t)c.B * 4);
      yi.alloc(R * 4);
      yw.alloc(soft_nms_work_floats(c.B, c.N) * 4);
      launch_soft_nms(boxes.as<float>(), scores.as<float>(), nullptr, 0, c.counts.empty() ? nullptr : count.as<int>(), c.B,
                      c.N, c.q.thresh, c.q.sigma, kRows, 512.f, yb.as<float>(), ys.as<float>(), yc.as<int>(),
                      yw.as<float>(), s, NmsCand{}, yi.as<int>());
      launch_nms_truncate(yb.as<float>(), ys.as<float>(), yc.as<int>(), yi.as<int>(), c.B, c.q.max_out, s);
      CK(hipStreamSynchronize(s));
      bad_yard = diff(yb.get<float>(R * 4), ob.get<float>(R * 4)) + diff(ys.get<float>(R), os.get<float>(R)) +
                 diff(yc.get<int>(c.B), oc.get<int>(c.B)) + diff(yi.get<int>(R), oi.get<int>(R));
    }
  }
  const bool inputs_ok = diff(boxes.get<float>(d.boxes.size()), d.boxes) == 0 && diff(scores.get<float>(d.scores.size()), d.scores) == 0;
  const bool ok = !bad_boxes && !bad_scores && !bad_classes && !bad_count && !bad_index && !bad_yard && inputs_ok;
  printf("{\"case\":\"%s\",\"ok\":%s,\"bad_boxes\":%ld,\"bad_scores\":%ld,\"bad_classes\":%ld,\"bad_count\":%ld,"
         "\"bad_index\":%ld,\"yardstick_run\":%s,\"bad_yardstick\":%ld,\"inputs_ok\":%s,\"ref_runs\":%d}\n",
         c.name.c_str(), ok ? "true" : "false", bad_boxes, bad_scores, bad_classes, bad_count, bad_index,
         yard_run ? "true" : "false", bad_yard, inputs_ok ? "true" : "false", exp_rounds);
  fflush(stdout);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--plan")) {
    plan();
    return 0;
  }
  hipStream_t s;
  CK(hipStreamCreate(&s));
  int n = 0;
  for (const Case& c : table()) {
    if (argc > 1 && c.name != argv[1]) continue;
    try {
      run_case(c, s);
    } catch (const std::exception& e) {
      printf("{\"case\":\"%s\",\"ok\":false,\"exception\":\"%s\"}\n", c.name.c_str(), e.what());
      fflush(stdout);
    }
    ++n;
  }
  printf("{\"done\":%d}\n", n);
  return 0;
}
