// exec_plan_json.hpp — one JSON line for an executor plan (tests/kernels/exec_plan.cpp).  The writer
// takes named scalars and named integer vectors, so whoever fills a PlanDump field for field prints a
// comparable line.  Each vector is reported as its length, its count of set (non-zero, non-negative)
// entries and an FNV-1a 64 hash of its values as little-endian int64; with `full`, the values too.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

struct PlanDump {
  std::vector<std::pair<std::string, long long>> scalars;
  std::vector<std::pair<std::string, std::vector<long long>>> vectors;
  void s(const char* k, long long v) { scalars.emplace_back(k, v); }
  template <typename V>
  void v(const char* k, const V& x) {
    vectors.emplace_back(k, std::vector<long long>(x.begin(), x.end()));
  }
  void vf(const char* k, const std::vector<float>& x) {  // floats by their bits
    std::vector<long long> o;
    for (float f : x) {
      uint32_t u;
      std::memcpy(&u, &f, 4);
      o.push_back(u);
    }
    vectors.emplace_back(k, o);
  }
};

inline uint64_t plan_fnv(const std::vector<long long>& x) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (long long v : x)
    for (int b = 0; b < 8; ++b) {
      h ^= (uint64_t)(((unsigned long long)v >> (8 * b)) & 0xff);
      h *= 0x100000001b3ull;
    }
  return h;
}

inline std::string plan_json(const std::string& config, const PlanDump& d, bool full) {
  std::string o = "{\"config\":\"" + config + "\"";
  for (const auto& kv : d.scalars) o += ",\"" + kv.first + "\":" + std::to_string(kv.second);
  for (const auto& kv : d.vectors) {
    long long set = 0;
    for (long long v : kv.second) set += v > 0;
    char h[32];
    snprintf(h, sizeof h, "%016llx", (unsigned long long)plan_fnv(kv.second));
    o += ",\"" + kv.first + "\":{\"n\":" + std::to_string(kv.second.size()) + ",\"set\":" + std::to_string(set) +
         ",\"hash\":\"" + h + "\"";
    if (full) {
      o += ",\"v\":[";
      for (size_t i = 0; i < kv.second.size(); ++i) o += (i ? "," : "") + std::to_string(kv.second[i]);
      o += "]";
    }
    o += "}";
  }
  return o + "}";
}

// Fills `d` from anything with the plan's field names (an ExecPlan).
template <typename Plan>
void plan_dump_fields(const Plan& E, PlanDump& d) {
  const auto& P = E.prog;
  d.s("B", E.B);
  d.s("tag", E.tag);
  d.s("bf16", E.bf16);
  d.s("abf", E.abf);
  d.s("infer_plan", E.infer_plan);
  d.s("n_ops", (long long)P.ops.size());
  d.s("n_tensors", (long long)P.tensors.size());
  d.s("n_slots", P.n_slots);
  d.s("act_floats", (long long)P.act_floats);
  d.s("grad_floats", (long long)P.grad_floats);
  d.s("n_mov", E.n_mov);
  d.s("mov_cmax", E.mov_cmax);
  d.s("ntiles", E.ntiles);
  d.s("ndrop", E.ndrop);
  d.s("ed_B", E.ed.B);
  d.s("ed_H", E.ed.H);
  d.s("ed_W", E.ed.W);
  d.s("ed_maxb", E.ed.maxb);
  d.s("ed_P", E.ed.P);
  d.s("ed_span_stride", E.ed.span_stride);
  d.s("ed_rcap", E.ed.rcap);
  d.s("sp_region", (long long)E.sp_region);
  d.s("sc_region", (long long)E.sc_region);
  d.s("n_groups", (long long)E.groups.size());
  std::vector<long long> gs, gm;
  for (const auto& g : E.groups) {
    gs.push_back((long long)g.size());
    for (int i : g) gm.push_back(i);
  }
  d.v("group_sizes", gs);
  d.v("group_members", gm);
  // a fused sepconv whose depthwise ops are grouped and whose pointwise ops are not
  long long mixed = 0;
  for (size_t i = 0; i + 1 < E.sep.size(); ++i) mixed += E.sep[i] && E.grp_of[i] >= 0 && E.grp_of[i + 1] < 0;
  d.s("sep_grouped_dw_ungrouped_pw", mixed);
  d.v("se_of_tensor", E.se_of_tensor);
  d.v("bn_of_tensor", E.bn_of_tensor);
  d.v("bn_consumer", E.bn_consumer);
  d.v("fused_bn", E.fused_bn);
  d.v("gfused_bn", E.gfused_bn);
  d.v("gstat_P", E.gstat_P);
  d.v("grp_of", E.grp_of);
  d.v("fuse_folded", E.fuse_folded);
  d.v("sep", E.sep);
  d.v("sepb", E.sepb);
  d.v("drop_slot", E.drop_slot);
  d.v("side_off", E.side_off);
  d.v("dxoff", E.dxoff);
  std::vector<long long> lev;
  for (const auto& l : E.lev) {
    const long long f[6] = {l.cls_off, l.box_off, l.h, l.w, l.anchor0, l.tile0};
    lev.insert(lev.end(), f, f + 6);
  }
  d.v("lev", lev);
}
