// dispatch_main.cpp -- the launch layer's dispatch helpers (pico_tree_amd/csrc/ptk_dispatch.hpp) against the ladders,
// switches and macros they replaced, each written out here as it stood.  Host only: the header names the metric types of
// the kernel headers and needs none of them.  Exits non-zero on the first difference and says which.
#include "ptk_dispatch.hpp"

#include <cstdio>
#include <cstring>
#include <typeinfo>

namespace {

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++failures;                              \
      std::fprintf(stderr, "FAILED: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");              \
    }                                          \
  } while (0)

// ---- the ladders as the launch wrappers had them ----
int ladder_reg(uint32_t k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }
int ladder_capped64(uint32_t k) { return k == 1 ? 1 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

// ---- the metric macros and switches as they stood: the name of the type each id was bound to ----
enum Name { L2, L1, LInf, LNInf, SO2, SE2, L2_64, L1_64, LInf_64, LNInf_64, SO2_64, SE2_64 };
Name old_with_metric(int id) {  // PTK_WITH_METRIC
  switch (id) {
    case PTK_METRIC_L1: return L1;
    case PTK_METRIC_LPINF: return LInf;
    case PTK_METRIC_LNINF: return LNInf;
    default: return L2;
  }
}
Name old_with_topo(int id) { return id == PTK_METRIC_SO2 ? SO2 : SE2; }  // PTK_WITH_TOPO
Name old_with_euclid64(int id) {  // PTK_WITH_EUCLID64 and the switch (metric) blocks of the float64 self entry points
  if (id == PTK_METRIC_L1) return L1_64;
  if (id == PTK_METRIC_LPINF) return LInf_64;
  if (id == PTK_METRIC_LNINF) return LNInf_64;
  return L2_64;
}
Name old_with_metric64(int id) {  // PTK_WITH_METRIC64
  if (id == PTK_METRIC_L1) return L1_64;
  if (id == PTK_METRIC_LPINF) return LInf_64;
  if (id == PTK_METRIC_LNINF) return LNInf_64;
  if (id == PTK_METRIC_SO2) return SO2_64;
  if (id == PTK_METRIC_SE2_SQUARED) return SE2_64;
  return L2_64;
}

template <class T>
struct name_of;
#define NAME_OF(T, N)                      \
  template <>                              \
  struct name_of<T> {                      \
    static constexpr Name value = N;       \
  }
NAME_OF(ptk::MetricL2, L2);
NAME_OF(ptk::MetricL1, L1);
NAME_OF(ptk::MetricLInf, LInf);
NAME_OF(ptk::MetricLNInf, LNInf);
NAME_OF(ptk::TopoSO2, SO2);
NAME_OF(ptk::TopoSE2, SE2);
NAME_OF(ptk::Metric64L2, L2_64);
NAME_OF(ptk::Metric64L1, L1_64);
NAME_OF(ptk::Metric64LInf, LInf_64);
NAME_OF(ptk::Metric64LNInf, LNInf_64);
NAME_OF(ptk::Topo64SO2, SO2_64);
NAME_OF(ptk::Topo64SE2, SE2_64);

// (the status a lambda returns is the tag's value plus this: a helper that dropped or changed it would show)
constexpr int kBase = 1000;

}  // namespace

int main() {
  // with_slots: both slot lists, k = 0 .. 200, against the ladders; the lambda's value comes back.
  for (uint32_t k = 0; k <= 200; ++k) {
    const int reg = ptkd::with_slots<4, 8, 16, 32, 64>(k, [](auto K) { return kBase + decltype(K)::value; });
    CHECK(reg == kBase + ladder_reg(k), "with_slots<4..64>(%u) = %d, the ladder picks %d", k, reg - kBase, ladder_reg(k));
    const int cap = ptkd::with_slots<1, 4, 8, 16, 32>(k, [](auto K) { return -decltype(K)::value; });
    // (k = 0 is the one value the two differ at: the ladder's first arm was `k == 1`, so it fell to 4 slots, the first
    // slot >= 0 is 1.  check_k refuses k = 0 before any launch wrapper is reached.)
    const int want_cap = k == 0 ? 1 : ladder_capped64(k);
    CHECK(cap == -want_cap, "with_slots<1..32>(%u) = %d, the ladder picks %d", k, -cap, want_cap);
    if (k + 1 <= 64) {  // knn_self passes k + 1
      const int self = ptkd::with_slots<4, 8, 16, 32, 64>(k + 1, [](auto K) { return (int)decltype(K)::value; });
      CHECK(self == ladder_reg(k + 1), "with_slots(k + 1 = %u) = %d", k + 1, self);
    }
  }
  // with_bool / with_bools: every tag exactly once over all inputs.
  {
    int seen[2] = {0, 0}, seen2[2][2] = {{0, 0}, {0, 0}};
    for (int b = 0; b < 2; ++b) {
      const int rc = ptkd::with_bool(b != 0, [&](auto B) {
        ++seen[decltype(B)::value ? 1 : 0];
        return kBase + (decltype(B)::value ? 1 : 0);
      });
      CHECK(rc == kBase + b, "with_bool(%d) returned %d", b, rc);
      for (int c = 0; c < 2; ++c) {
        const int rc2 = ptkd::with_bools(b != 0, c != 0, [&](auto B, auto C) {
          ++seen2[decltype(B)::value ? 1 : 0][decltype(C)::value ? 1 : 0];
          return kBase + 2 * (decltype(B)::value ? 1 : 0) + (decltype(C)::value ? 1 : 0);
        });
        CHECK(rc2 == kBase + 2 * b + c, "with_bools(%d, %d) returned %d", b, c, rc2);
      }
    }
    CHECK(seen[0] == 1 && seen[1] == 1, "with_bool reached its tags %d / %d times", seen[0], seen[1]);
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c) CHECK(seen2[b][c] == 1, "with_bools reached <%d, %d> %d times", b, c, seen2[b][c]);
  }
  // with_ovf: the three classes, and `none` for everything else.
  for (int cls = -2; cls <= 5; ++cls) {
    const int rc = ptkd::with_ovf<64, 256, 2048>(cls, [](auto O) { return (int)decltype(O)::value; }, [] { return -7; });
    const int want = cls == 0 ? 64 : cls == 1 ? 256 : cls == 2 ? 2048 : -7;
    CHECK(rc == want, "with_ovf(%d) = %d, not %d", cls, rc, want);
  }
  // The metric helpers: every PTK_METRIC_* id, and ids that are none (-1, 6, 1000).
  const int ids[] = {PTK_METRIC_L2_SQUARED, PTK_METRIC_L1, PTK_METRIC_LPINF, PTK_METRIC_LNINF, PTK_METRIC_SO2,
                     PTK_METRIC_SE2_SQUARED, -1, 6, 1000};
  auto name = [](auto m) { return kBase + (int)name_of<ptkd::type_of<decltype(m)>>::value; };
  for (int id : ids) {
    CHECK(ptkd::with_metric(id, name) == kBase + old_with_metric(id), "with_metric(%d)", id);
    CHECK(ptkd::with_topo(id, name) == kBase + old_with_topo(id), "with_topo(%d)", id);
    CHECK(ptkd::with_euclid64(id, name) == kBase + old_with_euclid64(id), "with_euclid64(%d)", id);
    CHECK(ptkd::with_metric64(id, name) == kBase + old_with_metric64(id), "with_metric64(%d)", id);
  }
  if (failures != 0) return 1;
  std::puts("dispatch OK");
  return 0;
}
