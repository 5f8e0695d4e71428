// norm_teeth — the teeth of norm_check.hpp, on the CPU: a stand-in for the kernels of kernels_norm.hip
// evaluated in fp32 (the column reduction with red_plan's lane / chunk / channel-group geometry, the
// finalize's fold, the SE MLP, max-pool, upsample, fuse backward, the gradient copy) is run through the
// same reference and compare functions norm_parity uses.  Unfaulted it must pass every bound; each seeded
// fault must be reported in the field meant to catch it and in no other.  One JSON line per run:
//   {"run": name, "fields": {field: ratio, ...}, "flags": {flag: bool, ...}}
// Build: make -C tests/kernels.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "norm_check.hpp"

using gck::kEps24;
using nck::Field;

enum Fault {
  NONE, DROP_LAST_ROW, IDLE_TWICE, GROUP2_READS_GROUP1, FIN_DROP_1030, FIN_ZERO_CNT, NO_UNSHIFT, NO_BESSEL, MOVING_ORDER,
  SE_NO_GATE, SE_NO_HW, SE_SHARES_SHORT, POOL_LAST_MAX, UPS_SHORT, FUSE_NO_EPS, DROP_CHUNK_ROW
};

struct Out {
  std::map<std::string, double> fields;
  std::map<std::string, bool> flags;
};
static void emit(const char* run, const Out& o) {
  std::string s = std::string("{\"run\":\"") + run + "\",\"fields\":{";
  bool first = true;
  for (auto& kv : o.fields) {
    char b[64];
    snprintf(b, sizeof b, "%.6g", std::isfinite(kv.second) ? kv.second : 1e308);
    s += std::string(first ? "" : ",") + "\"" + kv.first + "\":" + b;
    first = false;
  }
  s += "},\"flags\":{";
  first = true;
  for (auto& kv : o.flags) {
    s += std::string(first ? "" : ",") + "\"" + kv.first + "\":" + (kv.second ? "true" : "false");
    first = false;
  }
  puts((s + "}}").c_str());
}

// ---- the column reduction as k_colred_part / k_colred_final lay it out --------------------------
// (tpr lanes per row and rpi rows per pass in each channel group, chunks of rpc rows, fp32 runs of 64)
struct Geo {
  int rpi_of(int C, int g) const { return 256 / tpr_of(C, g); }
  int tpr_of(int C, int g) const { return std::min(C / 4 - g * 256, 256); }
  long rpc;
};
static void colred_stats(const float* y, long M, int C, const Geo& geo, Fault f, std::vector<double>& s0,
                         std::vector<double>& s1) {
  s0.assign(C, 0.0);
  s1.assign(C, 0.0);
  for (int c = 0; c < C; ++c) {
    const int g = (c / 4) / 256, tpr = geo.tpr_of(C, g), rpi = geo.rpi_of(C, g), cc = (c / 4) % 256;
    const int src = (f == GROUP2_READS_GROUP1 && g > 0) ? c - 1024 : c;
    const float ref = y[src];
    const int lanes = (f == IDLE_TWICE && cc < 256 - tpr * rpi) ? rpi + 1 : rpi;  // the partial row of idle lanes
    for (long m0 = 0; m0 < M; m0 += geo.rpc) {
      long m1 = std::min(M, m0 + geo.rpc);
      if (f == DROP_LAST_ROW && m1 - m0 > 1) --m1;
      for (int rr = 0; rr < lanes; ++rr) {
        long m = m0 + rr;
        while (m < m1) {
          float a0 = 0.f, a1 = 0.f;
          for (int it = 0; it < 64 && m < m1; ++it, m += rpi) {
            const float d = y[m * C + src] - ref;
            a0 += d;
            a1 += d * d;
          }
          s0[c] += a0;
          s1[c] += a1;
        }
      }
    }
  }
}
static Out run_stats(Fault f, bool sums) {
  // C 1152 (two channel groups, the second 32 lanes wide) and C 144 (tpr 36: four idle lanes) in turn
  Out o;
  Field mean, rstd, sc, moving, fs;
  for (int C : {1152, 144}) {
    const long M = C == 144 ? 113 : 19;
    const Geo geo{C == 144 ? 56 : 8};
    std::vector<float> y((size_t)M * C), gamma(C), mm0(C), mv0(C);
    gck::fill_uni(y, 7 + C);
    for (long m = 0; m < M; ++m) {
      y[m * C] += 1000.f;
      y[m * C + 1] = 0.75f;
    }
    gck::fill_uni(gamma, 8, 0.5f, 1.0f);
    gck::fill_uni(mm0, 9);
    gck::fill_uni(mv0, 10, 0.5f, 1.0f);
    std::vector<double> s0, s1;
    colred_stats(y.data(), M, C, geo, f, s0, s1);
    if (sums) {
      std::vector<double> out(3 * (size_t)C);
      for (int c = 0; c < C; ++c) {
        const double r = y[c];
        out[3 * c] = (double)M;
        out[3 * c + 1] = f == NO_UNSHIFT ? s0[c] : s0[c] + M * r;
        out[3 * c + 2] = f == NO_UNSHIFT ? s1[c] : s1[c] + 2.0 * r * s0[c] + M * r * r;
      }
      fs.merge(nck::check_stats_sums(y.data(), M, C, out.data()));
      continue;
    }
    std::vector<float> vm(C), vr(C), vs(C), vmm(C), vmv(C);
    for (int c = 0; c < C; ++c) {  // StatsEpi
      const double dm = s0[c] / M;
      double var = std::max(s1[c] / M - dm * dm, 0.0);
      const double mu = (double)y[c] + dm, rs = 1.0 / std::sqrt(var + (double)1e-3f);
      vm[c] = (float)mu;
      vr[c] = (float)rs;
      vs[c] = (float)(rs * (double)gamma[c]);
      const double uvar = f == NO_BESSEL ? var : var * M / (M - 1);
      vmm[c] = nck::moving_update(mm0[c], mu);
      vmv[c] = nck::moving_update(mv0[c], uvar);
    }
    nck::StatOut so;
    so.mean = vm.data(); so.rstd = vr.data(); so.sc = vs.data(); so.mmean = vmm.data(); so.mvar = vmv.data();
    const nck::StatCheck k = nck::check_stats(y.data(), M, C, gamma.data(), 1e-3f, mm0.data(), mv0.data(), so);
    mean.merge(k.mean); rstd.merge(k.rstd); sc.merge(k.sc); moving.merge(k.moving);
  }
  if (sums) {
    o.fields["sums"] = fs.ratio;
  } else {
    o.fields["mean"] = mean.ratio; o.fields["rstd"] = rstd.ratio; o.fields["sc"] = sc.ratio; o.fields["moving"] = moving.ratio;
  }
  return o;
}

// ---- k_bn_finalize's fold ----------------------------------------------------------------------
static Out run_fin(Fault f) {
  Out o;
  const int C = 8, P = 1100;
  std::vector<float> part, cnt, gamma(C), mm0(C), mv0(C);
  long M, zeros;
  nck::gen_partials(C, P, true, false, 77, part, cnt, &M, &zeros);
  if (f == FIN_ZERO_CNT)  // finite stale values, so that a fold of them shows in the value, not as a NaN
    for (int p = 0; p < P; ++p)
      if (cnt[p] == 0.f)
        for (int c = 0; c < C; ++c) part[2 * ((size_t)c * P + p)] = part[2 * ((size_t)c * P + p) + 1] = 40.f;
  gck::fill_uni(gamma, 8, 0.5f, 1.0f);
  gck::fill_uni(mm0, 9);
  gck::fill_uni(mv0, 10, 0.5f, 1.0f);
  nck::StatCheck k;
  std::vector<float> vm(C), vr(C), vs(C), vmm(C), vmv(C);
  for (int c = 0; c < C; ++c) {
    double s1 = 0, s2 = 0;
    for (int p = 0; p < P; ++p) {
      if (f == FIN_DROP_1030 && p == 1030) continue;
      const double x = part[2 * ((size_t)c * P + p)], q = part[2 * ((size_t)c * P + p) + 1];
      if (cnt[p] > 0.f) {
        s1 += x;
        s2 += q + x * x / cnt[p];
      } else if (f == FIN_ZERO_CNT) {
        s1 += x;
        s2 += q;
      }
    }
    const double dm = s1 / M, var = std::max(s2 / M - dm * dm, 0.0), rs = 1.0 / std::sqrt(var + (double)1e-3f);
    vm[c] = (float)dm; vr[c] = (float)rs; vs[c] = (float)(rs * (double)gamma[c]);
    vmm[c] = nck::moving_update(mm0[c], dm);
    vmv[c] = nck::moving_update(mv0[c], var * M / (M - 1));
    nck::StatOut so;
    so.mean = vm.data(); so.rstd = vr.data(); so.sc = vs.data(); so.mmean = vmm.data(); so.mvar = vmv.data();
    nck::check_stat_chan(nck::stats_from(nck::fold_partials(part.data(), cnt.data(), P, c, false), M, gamma[c],
                                         (double)1e-3f, mm0[c], mv0[c]),
                         so, c, k);
  }
  o.fields["mean"] = k.mean.ratio; o.fields["rstd"] = k.rstd.ratio; o.fields["sc"] = k.sc.ratio;
  o.fields["moving"] = k.moving.ratio;
  return o;
}
static Out run_moving(Fault f) {
  Out o;
  bool ok = true;
  gck::Rng rng(5);
  for (int i = 0; i < 1000; ++i) {
    const float m = rng.uni();
    const double b0 = rng.uni(), b1 = 3.0 * rng.uni();
    const float want = nck::moving_update(nck::moving_update(m, b0), b1);
    const float got = f == MOVING_ORDER ? nck::moving_update(nck::moving_update(m, b1), b0) : want;
    ok &= gck::f2u(want) == gck::f2u(got);
  }
  o.flags["exact"] = ok;
  return o;
}

// ---- squeeze-excite in fp32 ----------------------------------------------------------------------
static Out run_se(Fault f, bool bwd) {
  Out o;
  const int B = 2, HW = 49, C = 144, N = 6;
  const nck::SeShape sh{B, HW, C, N, 1, 5, 29, 8};  // se_plan_info(2, 144, 6): s1 5, cs1 29, jg 8
  const size_t n = (size_t)B * HW * C;
  std::vector<float> x(n), w1((size_t)C * N), b1(N), w2((size_t)N * C), b2(C), dy(n), scale((size_t)B * C),
      hidden((size_t)B * N);
  gck::fill_uni(x, 1);
  gck::fill_uni(w1, 2, 2.0f / std::sqrt((float)C));
  gck::fill_uni(b1, 3, 0.5f);
  gck::fill_uni(w2, 4, 2.0f / std::sqrt((float)N));
  gck::fill_uni(b2, 5, 0.5f);
  gck::fill_uni(dy, 6);
  gck::fill_uni(scale, 7, 0.45f, 0.5f);
  gck::fill_uni(hidden, 8, 3.0f);
  const cck::Val xv = cck::view_inx(cck::BnView{x.data()}, (long)B * HW, C);
  auto swish = [](float z) { return z / (1.0f + std::exp(-z)); };
  if (!bwd) {
    std::vector<float> pool((size_t)B * C), hid((size_t)B * N), sc((size_t)B * C);
    for (int b = 0; b < B; ++b) {
      for (int c = 0; c < C; ++c) {
        float s = 0.f;
        for (int m = 0; m < HW; ++m) s += x[((size_t)b * HW + m) * C + c];
        pool[b * C + c] = s * (1.0f / HW);
      }
      const int cend = f == SE_SHARES_SHORT ? C - 28 : C;  // the last slice (s1 * cs1 = 145 >= C: 28 channels)
      for (int j = 0; j < N; ++j) {
        float h = b1[j];
        for (int c = 0; c < cend; ++c) h += pool[b * C + c] * w1[(size_t)c * N + j];
        hid[b * N + j] = h;
      }
      for (int c = 0; c < C; ++c) {
        float t = b2[c];
        for (int j = 0; j < N; ++j) t += swish(hid[b * N + j]) * w2[(size_t)j * C + c];
        sc[b * C + c] = 1.0f / (1.0f + std::exp(-t));
      }
    }
    const nck::SeFwdRef ref = nck::se_fwd_ref(sh, xv, w1.data(), b1.data(), w2.data(), b2.data());
    o.fields["pool"] = nck::check_arr(ref.pool, pool.data()).ratio;
    o.fields["hidden"] = nck::check_arr(ref.hidden, hid.data()).ratio;
    o.fields["scale"] = nck::check_arr(ref.scale, sc.data()).ratio;
    return o;
  }
  std::vector<float> gsum((size_t)B * C), dx(n);
  for (int b = 0; b < B; ++b) {
    std::vector<float> v(C), dh(N);
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
      for (int m = 0; m < HW; ++m) s += dy[((size_t)b * HW + m) * C + c] * x[((size_t)b * HW + m) * C + c];
      const float sg = scale[b * C + c];
      v[c] = f == SE_NO_GATE ? s : s * sg * (1.f - sg);
    }
    for (int j = 0; j < N; ++j) {
      float q = 0.f;
      for (int c = 0; c < C; ++c) q += v[c] * w2[(size_t)c * N + j];
      const float h = hidden[b * N + j], s = 1.0f / (1.0f + std::exp(-h));
      dh[j] = q * (s * (1.0f + h * (1.0f - s)));
    }
    for (int c = 0; c < C; ++c) {
      float d = 0.f;
      for (int j = 0; j < N; ++j) d += dh[j] * w1[(size_t)c * N + j];
      gsum[b * C + c] = d;
      const float dp = f == SE_NO_HW ? d : d * (1.0f / HW);
      for (int m = 0; m < HW; ++m) {
        const size_t e = ((size_t)b * HW + m) * C + c;
        dx[e] = dy[e] * scale[b * C + c] + dp;
      }
    }
  }
  const nck::SeBwdRef ref = nck::se_bwd_ref(sh, dy.data(), xv, scale.data(), hidden.data(), w2.data(), w1.data(), nullptr);
  o.fields["gsum"] = nck::check_arr(ref.gsum, gsum.data()).ratio;
  o.fields["dx"] = nck::check_arr(ref.dx, dx.data()).ratio;
  return o;
}

// ---- resampling, fuse, gradient copy -------------------------------------------------------------
static Out run_pool(Fault f) {
  Out o;
  const nck::PoolGeo g = nck::pool_geo(2, 9, 7, 8, 3, 2);
  std::vector<float> x((size_t)g.B * g.H * g.W * g.C);
  gck::fill_uni(x, 3);
  for (auto& q : x) q = std::floor(q * 8.f) / 8.f;
  std::vector<float> y;
  std::vector<uint8_t> am;
  const cck::BnView bv{x.data()};
  nck::maxpool_fwd_cpu(g, bv, f == POOL_LAST_MAX, y, am);
  const nck::PoolCheck k = nck::check_maxpool_fwd(g, bv, false, y.data(), am.data());
  o.fields["y"] = k.y.ratio;
  o.flags["amax_ok"] = k.amax_bad == 0;
  return o;
}
static Out run_ups(Fault f) {
  Out o;
  const int B = 2, H = 3, Ho = 5, C = 4;
  std::vector<float> dy((size_t)B * Ho * Ho * C);
  gck::fill_uni(dy, 4);
  const std::vector<float> want = nck::upsample_bwd_replay(B, H, H, C, Ho, Ho, dy.data(), nullptr);
  const std::vector<float> got = nck::upsample_bwd_replay(B, H, H, C, Ho, Ho, dy.data(), nullptr, f == UPS_SHORT);
  o.flags["dx_exact"] = std::memcmp(want.data(), got.data(), want.size() * 4) == 0;
  return o;
}
static Out run_fuse(Fault f) {
  Out o;
  const long M = 37;
  const int C = 8;
  std::vector<float> x0((size_t)M * C), x1((size_t)M * C), dy((size_t)M * C);
  gck::fill_uni(x0, 1);
  gck::fill_uni(x1, 2);
  gck::fill_uni(dy, 3);
  cck::FuseRef fr;
  fr.nin = 2; fr.method = 0; fr.act = 1;
  fr.w[0] = 0.002f; fr.w[1] = 0.001f;  // small weights: the 1e-4 is 3 % of the denominator
  fr.x[0] = cck::BnView{x0.data()};
  fr.x[1] = cck::BnView{x1.data()};
  gck::Reference ref[3];
  const std::vector<float> none[3];
  nck::fuse_bwd_ref(fr, M, C, dy.data(), none, ref);
  const float den = (fr.w[0] + fr.w[1]) + (f == FUSE_NO_EPS ? 0.f : 0.0001f);
  std::vector<float> g0((size_t)M * C), g1((size_t)M * C);
  for (size_t e = 0; e < g0.size(); ++e) {
    const float v = x0[e] * fr.w[0] / den + x1[e] * fr.w[1] / den, s = 1.0f / (1.0f + std::exp(-v));
    const float dv = dy[e] * (s * (1.0f + v * (1.0f - s)));
    g0[e] = dv / den * fr.w[0];
    g1[e] = dv / den * fr.w[1];
  }
  o.fields["dx0"] = nck::check_arr(ref[0], g0.data()).ratio;
  o.fields["dx1"] = nck::check_arr(ref[1], g1.data()).ratio;
  return o;
}
static Out run_copy(Fault f) {
  Out o;
  const int B = 3, C = 8;
  const long rows_img = 37, rows = B * rows_img, rpc = 50;  // chunks of 50 rows: an image boundary inside
  std::vector<float> src((size_t)rows * C), keep = {1.f, 0.f, 1.f}, got((size_t)rows * C);
  gck::fill_uni(src, 9);
  for (long m = 0; m < rows; ++m) {
    const long img = f == DROP_CHUNK_ROW ? (m % rpc) / rows_img : m / rows_img;
    for (int c = 0; c < C; ++c) got[m * C + c] = (src[m * C + c] * keep[img]) / 0.8f;
  }
  const std::vector<float> want = nck::copy_grad_replay(src.data(), rows, C, keep.data(), 0.8f, rows_img, nullptr);
  o.flags["dst_exact"] = std::memcmp(want.data(), got.data(), want.size() * 4) == 0;
  return o;
}

int main() {
  emit("clean_stats", run_stats(NONE, false));
  emit("clean_stats_sums", run_stats(NONE, true));
  emit("clean_finalize", run_fin(NONE));
  emit("clean_moving", run_moving(NONE));
  emit("clean_se_fwd", run_se(NONE, false));
  emit("clean_se_bwd", run_se(NONE, true));
  emit("clean_maxpool", run_pool(NONE));
  emit("clean_upsample", run_ups(NONE));
  emit("clean_fuse_bwd", run_fuse(NONE));
  emit("clean_copy_grad", run_copy(NONE));
  emit("chunk_last_row_dropped", run_stats(DROP_LAST_ROW, false));
  emit("idle_lane_rows_twice", run_stats(IDLE_TWICE, false));
  emit("group2_reads_group1", run_stats(GROUP2_READS_GROUP1, false));
  emit("finalize_partial_1030_dropped", run_fin(FIN_DROP_1030));
  emit("finalize_zero_cnt_folded", run_fin(FIN_ZERO_CNT));
  emit("sums_not_unshifted", run_stats(NO_UNSHIFT, true));
  emit("bessel_missing", run_stats(NO_BESSEL, false));
  emit("moving_two_pass_order", run_moving(MOVING_ORDER));
  emit("se_gate_derivative_missing", run_se(SE_NO_GATE, true));
  emit("se_dpool_not_divided", run_se(SE_NO_HW, true));
  emit("se_shares_one_slice_short", run_se(SE_SHARES_SHORT, false));
  emit("maxpool_last_maximum", run_pool(POOL_LAST_MAX));
  emit("upsample_bwd_candidate_short", run_ups(UPS_SHORT));
  emit("fuse_eps_missing", run_fuse(FUSE_NO_EPS));
  emit("dropview_chunk_row", run_copy(DROP_CHUNK_ROW));
  printf("{\"done\":true}\n");
  return 0;
}
