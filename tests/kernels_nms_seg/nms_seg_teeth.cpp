// nms_seg_teeth — host only: each seeded fault of nms_seg_check.hpp's reference (the CPU stand-in for the kernel)
// must change the answer on at least one case of nms_seg_parity's table, or the table could not tell that fault from
// a correct kernel.  One JSON line per fault ({"fault", "tripped", "first_case"}), then {"done", "all_tripped"}.  The
// two largest cases are left out (their inputs are sparse boxes that no fault touches).
#include <cstdio>

#include "nms_seg_check.hpp"

using namespace nsk;

int main() {
  std::vector<Case> cases;
  for (const Case& c : table())
    if (c.kind != K_REFUSE && c.N <= 4096) cases.push_back(c);
  std::vector<Data> data;
  std::vector<RefOut> good;
  for (const Case& c : cases) {
    data.push_back(make_data(c));
    good.push_back(run_ref(c, data.back()));
  }
  int all = 1;
  for (int f = F_NONE + 1; f < F_COUNT; ++f) {
    int tripped = 0;
    const char* first = "";
    for (size_t i = 0; i < cases.size(); ++i)
      if (!same(good[i], run_ref(cases[i], data[i], (Fault)f))) {
        if (!tripped) first = cases[i].name.c_str();
        ++tripped;
      }
    printf("{\"fault\":\"%s\",\"tripped\":%d,\"first_case\":\"%s\"}\n", fault_name(f), tripped, first);
    all &= tripped > 0;
  }
  // the clean stand-in against itself: a fault-free run must not trip
  int clean = 0;
  for (size_t i = 0; i < cases.size(); ++i) clean += !same(good[i], run_ref(cases[i], data[i], F_NONE));
  printf("{\"done\":%d,\"all_tripped\":%s,\"clean_trips\":%d}\n", F_COUNT - 1, all && !clean ? "true" : "false", clean);
  return 0;
}
