// div_check — GPU check that phx::div_surv (common.hpp: the division without v_div_fmas) equals IEEE
// float division n / d bit for bit, 2^26 random numerators per round (magnitudes 2^-110 .. 2^110,
// both signs, zeros) over two denominator sets:
//   * drop connect: the survival probabilities of D1-D7 and random d in (0.5, 1];
//   * the histogram matcher (through phx::div_exact): the knot spacings of its grid FS (about 1/255),
//     pixel counts minus one and CDF steps j / (pixels - 1) of the sizes the tests and the attack use,
//     and random d with exponents 2^-20 .. 2^20 (div_exact's whole range); a few beyond it, which take
//     the plain division.
// Build: make -C tools div_check; run on a GPU: ./tools/div_check
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mladversarialobjectdetection_amd/csrc/common.hpp"

__global__ void k_check(const float* ds, int nd, unsigned long long n, unsigned long long seed, int exact,
                        unsigned long long* bad, float* example) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long x = (i + 1) * 0x9e3779b97f4a7c15ull ^ seed;
  x ^= x >> 31; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 29;
  const unsigned e = 127 - 110 + (unsigned)((x >> 8) % 221);  // exponent 2^-110 .. 2^110
  unsigned bits = ((unsigned)x & 0x807fffffu) | (e << 23);
  if ((x >> 40) % 997 == 0) bits &= 0x80000000u;                  // signed zeros
  const float num = __uint_as_float(bits);
  const float d = ds[(x >> 20) % nd];
  const float a = exact ? phx::div_exact(num, d) : phx::div_surv(num, d), b = num / d;
  if (__float_as_uint(a) != __float_as_uint(b)) {
    const unsigned long long k = atomicAdd(bad, 1ull);
    if (k == 0) { example[0] = num; example[1] = d; example[2] = a; example[3] = b; }
  }
}

static int run(const char* what, const std::vector<float>& ds, int exact) {
  float *dd, *ex;
  unsigned long long* bad;
  hipMalloc(&dd, ds.size() * 4);
  hipMalloc(&ex, 16);
  hipMalloc(&bad, 8);
  hipMemcpy(dd, ds.data(), ds.size() * 4, hipMemcpyHostToDevice);
  hipMemset(bad, 0, 8);
  const unsigned long long n = 1ull << 30;
  for (int r = 0; r < 4; ++r)
    hipLaunchKernelGGL(k_check, dim3((unsigned)(n / 256)), dim3(256), 0, 0, dd, (int)ds.size(), n, 1234ull + r, exact,
                       bad, ex);
  unsigned long long hb = 0;
  float he[4] = {0, 0, 0, 0};
  hipMemcpy(&hb, bad, 8, hipMemcpyDeviceToHost);
  hipMemcpy(he, ex, 16, hipMemcpyDeviceToHost);
  printf("%s vs n / d: %llu mismatches in %llu pairs (%zu denominators)\n", what, hb, 4 * n, ds.size());
  if (hb) printf("  e.g. %a / %a: %a vs %a\n", he[0], he[1], he[2], he[3]);
  hipFree(dd); hipFree(ex); hipFree(bad);
  return hb ? 1 : 0;
}

int main() {
  std::vector<float> ds;
  for (int n : {16, 23, 32, 39, 45, 55, 64}) for (int b = 0; b < n; ++b) ds.push_back(1.f - 0.2f * (float)b / (float)n);
  srand(7);
  for (int k = 0; k < 256; ++k) ds.push_back(0.5f + 0.5f * (float)rand() / (float)RAND_MAX);
  int rc = run("div_surv (drop connect)", ds, 0);

  std::vector<float> dm;
  auto fs = [](int k) { return std::min(std::max((float)k * (1.0f / 255.0f), 0.0f), 1.0f); };
  for (int k = 0; k < 255; ++k) dm.push_back(fs(k + 1) - fs(k));
  for (long px : {37L * 37, 24L * 40, 96L * 96, 128L * 128, 512L * 512, 640L * 640, 1024L * 1024}) {
    const float m = (float)(px - 1);
    dm.push_back(m);
    for (long j : {1L, 2L, 3L, 17L, 255L, 4097L, px / 3, px - 2})
      if (j >= 1 && j < px) dm.push_back((float)j / m);
  }
  for (int k = 0; k < 640; ++k) {
    const float mant = 1.0f + (float)rand() / ((float)RAND_MAX + 1.0f);
    dm.push_back(std::ldexp(mant, -20 + k % 40) * (k % 7 == 0 ? -1.0f : 1.0f));
  }
  for (float d : {0x1p-21f, 0x1.8p-30f, 0x1.2p21f, 0x1p40f, 0x1p20f, 0x1p-20f}) dm.push_back(d);
  rc |= run("div_exact (histogram matcher)", dm, 1);
  return rc;
}
