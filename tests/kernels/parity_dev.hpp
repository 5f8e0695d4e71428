// parity_dev.hpp — device plumbing shared by the kernel parity checkers (gemm_parity.cpp,
// conv_parity.cpp): checked HIP calls that end the process on the first error, input buffers, output
// buffers between guard regions, and the JSON helpers of the verdict lines.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gemm_check.hpp"

using gck::kGuardBytes;

[[noreturn]] inline void fatal(const char* what, const char* name) {
  printf("{\"fatal\":\"%s\",\"case\":\"%s\"}\n", what, name);
  fflush(stdout);
  _Exit(3);  // nothing further is launched after a HIP error
}
inline const char* g_case = "";
#define CK(expr)                                         \
  do {                                                   \
    const hipError_t e_ = (expr);                        \
    if (e_ != hipSuccess) fatal(hipGetErrorString(e_), g_case); \
  } while (0)

struct Dev {  // an input buffer
  void* d = nullptr;
  Dev() = default;
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() { if (d) (void)hipFree(d); }
  void put(const void* h, size_t bytes) {
    CK(hipMalloc(&d, std::max<size_t>(bytes, 16)));
    if (bytes) CK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
  }
  const float* f() const { return static_cast<const float*>(d); }
};
inline void put_f(Dev& d, const std::vector<float>& v) { d.put(v.data(), v.size() * 4); }
// bf16 storage: rounds v in place to the stored values and uploads the 16-bit words
inline void put_bf(Dev& d, std::vector<float>& v) {
  std::vector<uint16_t> h(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    h[i] = gck::f2bf(v[i]);
    v[i] = gck::bf2f(h[i]);
  }
  d.put(h.data(), h.size() * 2);
}

struct Guarded {  // an output buffer between two guard regions
  uint8_t* d = nullptr;
  size_t n = 0;
  std::vector<uint8_t> init, got;
  Guarded() = default;
  Guarded(const Guarded&) = delete;
  Guarded& operator=(const Guarded&) = delete;
  ~Guarded() { if (d) (void)hipFree(d); }
  void alloc(size_t bytes) {
    n = std::max<size_t>(bytes, 16);
    init.assign(n + 2 * kGuardBytes, gck::kGuardByte);
    CK(hipMalloc(reinterpret_cast<void**>(&d), init.size()));
  }
  uint8_t* fill() { return init.data() + kGuardBytes; }
  void fill32(uint32_t w) {
    for (size_t i = 0; i + 4 <= n; i += 4) std::memcpy(fill() + i, &w, 4);
  }
  void fill16(uint16_t w) {
    for (size_t i = 0; i + 2 <= n; i += 2) std::memcpy(fill() + i, &w, 2);
  }
  void upload() { CK(hipMemcpy(d, init.data(), init.size(), hipMemcpyHostToDevice)); }
  void download() {
    got.resize(init.size());
    CK(hipMemcpy(got.data(), d, got.size(), hipMemcpyDeviceToHost));
  }
  float* ptr() const { return reinterpret_cast<float*>(d + kGuardBytes); }
  const uint8_t* out() const { return got.data() + kGuardBytes; }
  bool intact() const { return gck::guards_intact(got.data(), n); }
};

inline std::string esc(const std::string& s) {
  std::string o;
  for (char ch : s) {
    if (ch == '"' || ch == '\\') o += '\\';
    o += (ch == '\n') ? ' ' : ch;
  }
  return o;
}
inline std::string num(double x) {
  char b[40];
  if (std::isfinite(x)) snprintf(b, sizeof b, "%.6g", x);
  else snprintf(b, sizeof b, "1e308");  // JSON has no infinity
  return b;
}
