// boxloss_teeth — host only: faults seeded into the reference of boxloss_check.hpp must change its answer
// (an image's value, or its gradient with respect to the pred boxes) on at least one case of the table
// below, which is the parity table's small cases plus three hand-made ones.  Prints one JSON line per
// fault and exits non-zero if a fault goes unnoticed: a reference that cannot tell these apart would not
// catch a kernel that made the same mistake.
#include "boxloss_check.hpp"

using namespace boxloss;

struct Hand {
  std::vector<Box> gt, pred;
};

// relative change of (value, gradient) between two references of one image
static double change(const ImageRef& a, const ImageRef& b) {
  double d = std::fabs(a.value - b.value) / std::max(1e-12, std::fabs(a.value));
  double n = 0, m = 0;
  for (size_t i = 0; i < a.dpred.size() && i < b.dpred.size(); ++i) {
    n += (a.dpred[i] - b.dpred[i]) * (a.dpred[i] - b.dpred[i]);
    m += a.dpred[i] * a.dpred[i];
  }
  if (m > 0) d = std::max(d, std::sqrt(n / m));
  return d;
}

int main() {
  std::vector<Hand> hands = {
      // a pred that shares ymin with its gt and is inside it otherwise (tie routing), beside a far one
      {{{0, 0, 10, 10}}, {{0, 2, 8, 9}, {50, 50, 60, 60}}},
      // exact duplicates of the best pred (equal split) and a flipped gt (unclamped height)
      {{{0, 0, 10, 10}, {30, 5, 20, 25}}, {{1, 2, 8, 9}, {1, 2, 8, 9}, {22, 6, 31, 20}, {1, 2, 8, 9}}},
      // two gts, three preds: max over preds per gt differs from max over gts per pred
      {{{0, 0, 10, 10}, {40, 40, 70, 80}}, {{1, 1, 9, 9}, {2, 2, 12, 12}, {41, 42, 69, 77}}},
  };
  struct F {
    const char* name;
    Faults f;
  };
  std::vector<F> faults(6);
  faults[0].name = "real_centres";   faults[0].f.real_centres = true;
  faults[1].name = "clamp_gt";       faults[1].f.clamp_gt = true;
  faults[2].name = "tie_to_pred";    faults[2].f.tie_to_pred = true;
  faults[3].name = "first_tie_only"; faults[3].f.first_tie_only = true;
  faults[4].name = "no_epsilon";     faults[4].f.no_epsilon = true;
  faults[5].name = "max_over_gts";   faults[5].f.max_over_gts = true;
  // the table cases small enough for a host-only run
  std::vector<Case> cases;
  for (const Spec& s : specs())
    if (s.A <= 3069 && s.B * (long)s.G[0] <= 300) cases.push_back(make_case(s));
  int missed = 0;
  for (const F& ft : faults) {
    double worst = 0;
    std::string where = "-";
    auto note = [&](double d, const std::string& w) {
      if (d > worst) {
        worst = d;
        where = w;
      }
    };
    for (size_t h = 0; h < hands.size(); ++h) {
      const Hand& H = hands[h];
      std::vector<uint8_t> keep(H.pred.size(), 1);
      const ImageRef a = image_ref(H.gt.data(), (int)H.gt.size(), H.pred.data(), keep.data(), (int)H.pred.size());
      const ImageRef b = image_ref(H.gt.data(), (int)H.gt.size(), H.pred.data(), keep.data(), (int)H.pred.size(), ft.f);
      note(change(a, b), "hand" + std::to_string(h));
    }
    for (const Case& c : cases) {
      const auto a = refs_of(c);
      std::vector<ImageRef> b;
      try {
        b = refs_of(c, ft.f);
      } catch (const std::runtime_error&) {
        continue;  // (the faulted arithmetic met a zero test that is not exact on this case)
      }
      for (size_t i = 0; i < a.size(); ++i) note(change(a[i], b[i]), c.name);
    }
    // a change a thousand times the largest bound a value carries in the table (~1e-5) is a different answer
    const bool seen = worst > 1e-6;
    missed += !seen;
    printf("{\"fault\":\"%s\",\"seen\":%s,\"largest_change\":%.4g,\"on\":\"%s\"}\n", ft.name, seen ? "true" : "false",
           worst, where.c_str());
  }
  printf("{\"done\":%d,\"missed\":%d}\n", (int)faults.size(), missed);
  return missed ? 1 : 0;
}
