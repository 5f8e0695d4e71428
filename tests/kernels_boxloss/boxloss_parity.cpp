// boxloss_parity — k_idiou_part / k_idiou_merge / k_idiou_batch and k_box_scatter (kernels_boxloss.hip) against
// the fp64 host reference of boxloss_check.hpp on the same fp32 inputs, case by case: one process, one
// stream, one JSON line per case, then {"done": n}.
//   boxloss_parity --plan   the case table's geometry (host code only: no HIP call)
//   boxloss_parity [case]   run the table (or one case)
// Checked per (image, gt): |device max - host max| <= the pair's bound; the device's anchor is the lowest
// host anchor that reaches the host maximum exactly and its tie count is the host's (the generator keeps
// every other kept anchor further below the maximum than twice the bounds involved; that margin is
// asserted here for every (image, gt), none excluded).  Per image and for the batch: the fp32 sums in gt /
// image order within the summed bounds plus one rounding per addition.  k_box_scatter: against the fp64
// dense dx = dY W^T of the same sparse dY (the reference's box-logit gradient), within the bound its
// contributions carry; two launches into zeroed buffers must give identical bytes.
#include <hip/hip_runtime.h>

#include <cstring>

#include "boxloss.hpp"
#include "boxloss_check.hpp"
#include "phx.h"

using namespace boxloss;

static const char* g_case = "";
#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      printf("{\"fatal\":\"%s: %s\",\"case\":\"%s\"}\n", #x, hipGetErrorString(e_), g_case); \
      fflush(stdout);                                                                  \
      exit(3);                                                                         \
    }                                                                                  \
  } while (0)

template <typename T>
static T* up(const std::vector<T>& h) {
  T* d = nullptr;
  CK(hipMalloc(&d, std::max<size_t>(h.size(), 1) * sizeof(T)));
  if (!h.empty()) CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
template <typename T>
static T* dz(size_t n) {
  T* d = nullptr;
  CK(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
  CK(hipMemset(d, 0, std::max<size_t>(n, 1) * sizeof(T)));
  return d;
}
template <typename T>
static std::vector<T> down(const T* d, size_t n) {
  std::vector<T> h(n);
  if (n) CK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

// two levels over the case's A / 9 pixels (the scatter's level lookup and offsets)
struct Levels {
  phx::LevelDesc lev[2];
  long dxoff[2];
  size_t dx_floats, box_floats;
};
static Levels levels_of(const Case& c) {
  const int PT = c.A / kNa, p0 = PT / 3, p1 = PT - p0;
  Levels L{};
  L.lev[0] = phx::LevelDesc{0, 0, p0, 1, 0, 0};
  L.lev[1] = phx::LevelDesc{0, (long)c.B * p0 * kNa * 4, p1, 1, p0 * kNa, 0};
  L.dxoff[0] = 16;  // (a gradient arena offset, not 0)
  L.dxoff[1] = 16 + (long)c.B * p0 * c.K + 48;
  L.dx_floats = (size_t)L.dxoff[1] + (size_t)c.B * p1 * c.K + 16;
  L.box_floats = (size_t)c.B * PT * kNa * 4;
  return L;
}
// the case's logits [B][A][4] in the levels' layout [level][B][pixels][na*4]
static std::vector<float> level_logits(const Case& c, const Levels& L) {
  std::vector<float> o(L.box_floats);
  for (int l = 0; l < 2; ++l) {
    const int n = L.lev[l].h * kNa;
    for (int b = 0; b < c.B; ++b)
      for (int a = 0; a < n; ++a)
        memcpy(&o[L.lev[l].box_off + ((size_t)b * n + a) * 4], &c.logits[((size_t)b * c.A + L.lev[l].anchor0 + a) * 4], 16);
  }
  return o;
}

static void plan() {
  for (const Spec& s : specs()) {
    std::vector<ImageRef> refs;
    const Case c = make_case(s, &refs);
    long kept = 0, kept_last = 0, max_ties = 0, empty_images = 0, degenerate = 0;
    const int S = phx::idiou_chunks(c.A);
    for (int b = 0; b < c.B; ++b) {
      long kb = 0;
      for (int a = 0; a < c.A; ++a)
        if (c.keep[(size_t)b * c.A + a] & 1) {
          ++kb;
          if (a / phx::kIdiouChunk == S - 1) ++kept_last;
        }
      kept += kb;
      empty_images += kb == 0;
      for (const GtRef& r : refs[b].gt) max_ties = std::max<long>(max_ties, (long)r.ties.size());
      for (int g = 0; g < c.G[b]; ++g) {
        const float* q = &c.gts[((size_t)b * kMaxGt + g) * 4];
        degenerate += (q[2] <= q[0]) || (q[3] <= q[1]);
      }
    }
    std::string gs;
    for (int b = 0; b < c.B; ++b) gs += (b ? "," : "") + std::to_string(c.G[b]);
    printf("{\"case\":\"%s\",\"B\":%d,\"A\":%d,\"K\":%d,\"G\":[%s],\"chunk\":%d,\"chunks\":%d,\"kept\":%ld,"
           "\"kept_in_last_chunk\":%ld,\"max_ties\":%ld,\"images_without_kept\":%ld,\"degenerate_gts\":%ld,\"seed\":%d}\n",
           c.name.c_str(), c.B, c.A, c.K, gs.c_str(), phx::kIdiouChunk, S, kept, kept_last, max_ties, empty_images,
           degenerate, c.seed_used);
  }
}

static void run(const Spec& s, hipStream_t st) {
  std::vector<ImageRef> refs;
  const Case c = make_case(s, &refs);
  const int B = c.B, A = c.A, K = c.K;
  const float weight = 0.375f;
  float* d_boxes = up(c.boxes);
  uint8_t* d_keep = up(c.keep);
  float* d_gt = up(c.gts);
  int* d_gc = up(c.G);
  float* d_max = dz<float>((size_t)B * kMaxGt);
  int* d_arg = dz<int>((size_t)B * kMaxGt);
  int* d_nt = dz<int>((size_t)B * kMaxGt);
  float* d_img = dz<float>(B);
  float* d_batch = dz<float>(1);
  int* d_scr = dz<int>(phx::idiou_scratch_ints(B, A));
  std::vector<float> met(PHX_NMETRIC, 0.0f);
  met[PHX_M_LOSS] = 3.0f;
  float* d_met = up(met);
  phx::launch_idiou(d_boxes, d_keep, d_gt, d_gc, B, A, d_max, d_arg, d_nt, d_img, d_batch, d_scr, weight, d_met, st);
  CK(hipStreamSynchronize(st));
  const auto h_max = down(d_max, (size_t)B * kMaxGt);
  const auto h_arg = down(d_arg, (size_t)B * kMaxGt);
  const auto h_nt = down(d_nt, (size_t)B * kMaxGt);
  const auto h_img = down(d_img, B);
  const float h_batch = down(d_batch, 1)[0];
  const float h_loss = down(d_met, PHX_NMETRIC)[PHX_M_LOSS];
  long bad_max = 0, bad_anchor = 0, bad_nties = 0, bad_image = 0, margin_fail = 0, bad_pad = 0;
  double worst = 0, max_bound = 0, batch_ref = 0, batch_bound = 0;
  for (int b = 0; b < B; ++b) {
    double img_bound = 0, run = 0;
    for (int g = 0; g < kMaxGt; ++g) {
      const size_t o = (size_t)b * kMaxGt + g;
      if (g >= c.G[b] || refs[b].gt[g].ties.empty()) {
        bad_pad += !(h_max[o] == 0.0f && h_arg[o] == -1 && h_nt[o] == 0);
        continue;
      }
      const GtRef& r = refs[b].gt[g];
      if (!margin_holds(r)) ++margin_fail;
      const double err = std::fabs((double)h_max[o] - r.max);
      max_bound = std::max(max_bound, r.bound);
      if (r.bound > 0) worst = std::max(worst, err / r.bound);
      bad_max += !(err <= r.bound);
      bad_anchor += h_arg[o] != r.ties.front();
      bad_nties += h_nt[o] != (int)r.ties.size();
      run += std::fabs(r.max);
      img_bound += r.bound + kU * run;  // the fp32 running sum, one rounding per addition
    }
    img_bound += kU * (run + 1e-7);
    bad_image += !(std::fabs((double)h_img[b] - refs[b].value) <= img_bound);
    batch_ref += refs[b].value;
    batch_bound += img_bound + kU * std::fabs(batch_ref);
  }
  const bool bad_batch = !(std::fabs((double)h_batch - batch_ref) <= batch_bound);
  const double loss_ref = 3.0 + (double)weight * batch_ref;
  const bool bad_loss = !(std::fabs((double)h_loss - loss_ref) <= weight * batch_bound + 2 * kU * (3.0 + std::fabs(loss_ref)));

  // ---- scatter
  const Levels L = levels_of(c);
  std::vector<phx::LevelDesc> lev(L.lev, L.lev + 2);
  std::vector<long> dxoff(L.dxoff, L.dxoff + 2);
  phx::LevelDesc* d_lev = up(lev);
  long* d_dxoff = up(dxoff);
  float* d_lg = up(level_logits(c, L));
  float* d_an = up(c.anchors);
  float* d_w = up(c.wpred);
  std::vector<std::vector<float>> got;
  for (int rep = 0; rep < 2; ++rep) {
    float* d_dx = dz<float>(L.dx_floats);
    phx::launch_box_scatter(d_boxes, d_keep, d_gt, d_gc, d_max, d_arg, d_nt, d_lg, d_an, d_lev, 2, A, B, kNa, d_w, K,
                            weight, d_dx, d_dxoff, st);
    CK(hipStreamSynchronize(st));
    got.push_back(down(d_dx, L.dx_floats));
    CK(hipFree(d_dx));
  }
  const bool same_bytes = memcmp(got[0].data(), got[1].data(), L.dx_floats * sizeof(float)) == 0;
  // fp64 dense reference: dY [B][A][4] from the reference's d value / d box through the decode, dx = dY W^T
  std::vector<double> ref(L.dx_floats, 0.0), bnd(L.dx_floats, 0.0), mag(L.dx_floats, 0.0);
  std::vector<int> cnt(L.dx_floats, 0);
  long nz_rows = 0;
  const int N = kNa * 4;
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < A; ++a) {
      const double* d = &refs[b].dpred[(size_t)a * 4];
      const double* de = &refs[b].dpred_bound[(size_t)a * 4];
      if (d[0] == 0 && d[1] == 0 && d[2] == 0 && d[3] == 0 && de[0] == 0 && de[1] == 0 && de[2] == 0 && de[3] == 0) continue;
      const float* an = &c.anchors[(size_t)a * 4];
      const float* lg = &c.logits[((size_t)b * A + a) * 4];
      const double ha = (double)an[2] - an[0], wa = (double)an[3] - an[1];
      const double h = std::exp((double)lg[2]) * ha, w = std::exp((double)lg[3]) * wa;
      const double dt[4] = {weight * (d[0] + d[2]) * ha, weight * (d[1] + d[3]) * wa, weight * (d[2] - d[0]) * 0.5 * h,
                            weight * (d[3] - d[1]) * 0.5 * w};
      // per logit: the box gradient's bound through the same products, + 6 roundings (sum, two or three
      // products, the tie split, expf's 2 ulp)
      const double et[4] = {weight * (de[0] + de[2]) * std::fabs(ha), weight * (de[1] + de[3]) * std::fabs(wa),
                            weight * (de[0] + de[2]) * 0.5 * std::fabs(h), weight * (de[1] + de[3]) * 0.5 * std::fabs(w)};
      const int l = a >= L.lev[1].anchor0 ? 1 : 0;
      const int pix = (a - L.lev[l].anchor0) / kNa, k = (a - L.lev[l].anchor0) % kNa;
      const size_t row = (size_t)L.dxoff[l] + ((size_t)b * L.lev[l].h + pix) * K;
      ++nz_rows;
      for (int j = 0; j < K; ++j) {
        ++cnt[row + j];
        for (int q = 0; q < 4; ++q) {
          const double wv = c.wpred[(size_t)j * N + k * 4 + q];
          ref[row + j] += wv * dt[q];
          bnd[row + j] += std::fabs(wv) * (et[q] + 8 * kU * std::fabs(dt[q]));
          mag[row + j] += std::fabs(wv * dt[q]);
        }
      }
    }
  long bad_dx = 0, stray = 0;
  double dx_worst = 0, ref_norm = 0;
  for (size_t i = 0; i < L.dx_floats; ++i) {
    ref_norm += ref[i] * ref[i];
    if (bnd[i] == 0) {
      stray += got[0][i] != 0.0f;  // (every element no winner touches stays zero, the guard floats included)
      continue;
    }
    // the logit gradients' own bounds through |W|, then per (gt, anchor) contribution of the pixel four
    // products and three additions (4 u of its magnitude) and one rounding of the running sum, which the
    // magnitudes' sum bounds: (4 + n) u sum |w dt| for the pixel's n contributions
    const double tol = bnd[i] + (4.0 + cnt[i]) * kU * mag[i];
    const double err = std::fabs((double)got[0][i] - ref[i]);
    dx_worst = std::max(dx_worst, err / tol);
    bad_dx += !(err <= tol);
  }
  const bool ok = !bad_max && !bad_anchor && !bad_nties && !bad_image && !margin_fail && !bad_pad && !bad_batch && !bad_loss &&
                  same_bytes && !bad_dx && !stray;
  printf("{\"case\":\"%s\",\"ok\":%s,\"bad_max\":%ld,\"bad_anchor\":%ld,\"bad_nties\":%ld,\"bad_image\":%ld,\"bad_pad\":%ld,"
         "\"margin_fail\":%ld,\"bad_batch\":%s,\"bad_loss\":%s,\"worst_err_over_bound\":%.4g,\"max_bound\":%.4g,"
         "\"scatter_same_bytes\":%s,\"bad_dx\":%ld,\"stray_dx\":%ld,\"dx_worst_err_over_bound\":%.4g,\"dx_rows\":%ld,"
         "\"dx_ref_norm\":%.6g,\"batch\":%.9g,\"batch_ref\":%.12g}\n",
         c.name.c_str(), ok ? "true" : "false", bad_max, bad_anchor, bad_nties, bad_image, bad_pad, margin_fail,
         bad_batch ? "true" : "false", bad_loss ? "true" : "false", worst, max_bound, same_bytes ? "true" : "false", bad_dx,
         stray, dx_worst, nz_rows, std::sqrt(ref_norm), (double)h_batch, batch_ref);
  fflush(stdout);
  for (void* p : {(void*)d_boxes, (void*)d_keep, (void*)d_gt, (void*)d_gc, (void*)d_max, (void*)d_arg, (void*)d_nt,
                  (void*)d_img, (void*)d_batch, (void*)d_scr, (void*)d_met, (void*)d_lev, (void*)d_dxoff, (void*)d_lg,
                  (void*)d_an, (void*)d_w})
    CK(hipFree(p));
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--plan")) {
    plan();
    return 0;
  }
  hipStream_t st;
  CK(hipStreamCreate(&st));
  int n = 0;
  for (const Spec& s : specs()) {
    if (argc > 1 && s.name != argv[1]) continue;
    g_case = s.name.c_str();
    try {
      run(s, st);
    } catch (const std::exception& e) {
      printf("{\"case\":\"%s\",\"ok\":false,\"exception\":\"%s\"}\n", s.name.c_str(), e.what());
      fflush(stdout);
    }
    ++n;
  }
  CK(hipStreamDestroy(st));
  printf("{\"done\":%d}\n", n);
  return 0;
}
