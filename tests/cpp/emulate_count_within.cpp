// tests/cpp/emulate_count_within.cpp -- TEST INFRASTRUCTURE: the side table and the count kernel of count_within
// (pico_tree_amd/csrc/ptk_kernels_count.hpp) run lane by lane on the CPU, on the emulator of
// tests/cpp/emulate_kernels.cpp (whose handles, encoders and lane scheduler this unit reuses).
// Built by tests/test_count_within.py with the same g++ line and HIP stand-in as the emulator itself.

#include "emulate_kernels.cpp"
#include "ptk_kernels_count.hpp"
#include "ptk_kernels_count64.hpp"

namespace {
template <class M>
void count_metric(Emu* t, const ptk::CountBox* table, const float* q, uint64_t nq, float radius, uint64_t max_count,
                  uint32_t shortcut, uint64_t* counts, uint32_t* stats) {
  for_each_lane(nq, [&] {
    ptk::count_within_kernel<16, 2048, 64, 4, M>(t->dev, table, q, t->dim, nullptr, nq, radius, max_count, shortcut, counts,
                                                 stats);
  }, 64);
}
template <class M>
void count64_metric(Emu64* t, const ptk::CountBox64* table, const double* q, uint64_t nq, double radius, uint64_t max_count,
                    uint32_t shortcut, uint64_t* counts, uint32_t* stats) {
  for_each_lane64(t, nq, [&](uint64_t q0, uint64_t m) {
    ptk::count64_within_kernel<M>(t->dev, table, q, nullptr, q0, m, radius, max_count, shortcut, counts, t->stack.data(),
                                  t->slots, stats);
  });
}
}  // namespace

extern "C" {

// counts[i] of count_within_kernel (dim <= 3), the side table built by the table kernels first.  stats[3]: the
// shortcuts taken (inside, outside) and the inside tests refused for a subnormal radius, summed over the batch.
int emu_count_within(void* h, const float* q, uint64_t nq, float radius, uint64_t max_count, int shortcut, uint64_t* counts,
                     uint32_t* stats) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3) return -1;
  const uint32_t nb = (uint32_t)t->enc.nodes.size();
  std::vector<ptk::CountBox> table(nb > 0 ? nb : 1);
  std::vector<uint32_t> info(nb > 0 ? nb : 1), arrive(nb > 0 ? nb : 1);
  if (nb > 0) {
    for_each_lane(nb, [&] { ptk::count_parents_kernel(t->dev, nb, info.data(), arrive.data()); }, 256);
    for_each_lane(nb, [&] { ptk::count_table_kernel(t->dev, nb, info.data(), arrive.data(), table.data()); }, 256);
  }
  stats[0] = stats[1] = stats[2] = 0;
  switch (t->metric) {
    case 1: count_metric<ptk::MetricL1>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    case 2: count_metric<ptk::MetricLInf>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    case 3: count_metric<ptk::MetricLNInf>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    case 0: count_metric<ptk::MetricL2>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    default: return -1;
  }
  return 0;
}

// The same for a float64 tree of tests/emu.py's EmulatedTree64 (dim <= 3): count64_within_kernel and its side table.
int emu64_count_within(void* h, const double* q, uint64_t nq, double radius, uint64_t max_count, int shortcut,
                       uint64_t* counts, uint32_t* stats) {
  auto* t = static_cast<Emu64*>(h);
  if (t->dev.dim > 3) return -1;
  const uint32_t nb = (uint32_t)t->enc.nodes.size();
  std::vector<ptk::CountBox64> table(nb > 0 ? nb : 1);
  std::vector<uint32_t> info(nb > 0 ? nb : 1), arrive(nb > 0 ? nb : 1);
  if (nb > 0) {
    for_each_lane(nb, [&] { ptk::count64_parents_kernel(t->dev, nb, info.data(), arrive.data()); }, 256);
    for_each_lane(nb, [&] { ptk::count64_table_kernel(t->dev, nb, info.data(), arrive.data(), table.data()); }, 256);
  }
  stats[0] = stats[1] = stats[2] = 0;
  switch (t->metric) {
    case 1: count64_metric<ptk::Metric64L1>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    case 2: count64_metric<ptk::Metric64LInf>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    case 3: count64_metric<ptk::Metric64LNInf>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    case 0: count64_metric<ptk::Metric64L2>(t, table.data(), q, nq, radius, max_count, (uint32_t)shortcut, counts, stats); break;
    default: return -1;
  }
  return 0;
}

}  // extern "C"
