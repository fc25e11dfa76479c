// tests/cpp/emulate_radius_radii.cpp -- TEST INFRASTRUCTURE: the two passes of search_radius_radii (the per-row count,
// count_within_radii_kernel with max_count = 0, and the per-row fill, radius_radii_fill_kernel) run lane by lane on the
// CPU, on the emulator of tests/cpp/emulate_kernels.cpp (whose handles, encoders and lane scheduler this unit reuses).
// Built by tests/test_radius_radii.py with the same g++ line and HIP stand-in as the emulator itself.  The scan between
// the passes is the test's.

#include "emulate_kernels.cpp"
#include "ptk_kernels_count.hpp"

namespace {
template <class M>
void count_metric(Emu* t, const ptk::CountBox* table, const float* q, const uint32_t* perm, uint64_t nq, const float* radii,
                  uint64_t* counts) {
  for_each_lane(nq, [&] {
    ptk::count_within_radii_kernel<16, 2048, 64, 4, M>(t->dev, table, q, t->dim, perm, nq, radii, 0, 1u, counts, nullptr);
  }, 64);
}

template <class M>
void fill_metric(Emu* t, const float* q, const uint32_t* perm, uint64_t nq, const float* radii, const uint64_t* offsets,
                 ptk::Neighbor* o) {
  for_each_lane(nq, [&] {
    ptk::radius_radii_fill_kernel<16, 2048, 64, 4, M>(t->dev, q, t->dim, perm, nq, radii, offsets, o);
  }, 64);
}
}  // namespace

extern "C" {

// counts[i] of the count pass: count_within_radii_kernel with both shortcuts on and no limit, its side table built by
// the table kernels first.  `perm` (null: as given) is the launch order; radii[i] belongs to query row i.
int emu_radius_radii_count(void* h, const float* q, const uint32_t* perm, uint64_t nq, const float* radii,
                           uint64_t* counts) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3) return -1;
  const uint32_t nb = (uint32_t)t->enc.nodes.size();
  std::vector<ptk::CountBox> table(nb > 0 ? nb : 1);
  std::vector<uint32_t> info(nb > 0 ? nb : 1), arrive(nb > 0 ? nb : 1);
  if (nb > 0) {
    for_each_lane(nb, [&] { ptk::count_parents_kernel(t->dev, nb, info.data(), arrive.data()); }, 256);
    for_each_lane(nb, [&] { ptk::count_table_kernel(t->dev, nb, info.data(), arrive.data(), table.data()); }, 256);
  }
  switch (t->metric) {
    case 1: count_metric<ptk::MetricL1>(t, table.data(), q, perm, nq, radii, counts); break;
    case 2: count_metric<ptk::MetricLInf>(t, table.data(), q, perm, nq, radii, counts); break;
    case 3: count_metric<ptk::MetricLNInf>(t, table.data(), q, perm, nq, radii, counts); break;
    case 0: count_metric<ptk::MetricL2>(t, table.data(), q, perm, nq, radii, counts); break;
    default: return -1;
  }
  return 0;
}

// The fill pass: row i at out + offsets[i], in the reference's traversal order.
int emu_radius_radii_fill(void* h, const float* q, const uint32_t* perm, uint64_t nq, const float* radii,
                          const uint64_t* offsets, ptk_neighbor* out) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3) return -1;
  auto* o = reinterpret_cast<ptk::Neighbor*>(out);
  switch (t->metric) {
    case 1: fill_metric<ptk::MetricL1>(t, q, perm, nq, radii, offsets, o); break;
    case 2: fill_metric<ptk::MetricLInf>(t, q, perm, nq, radii, offsets, o); break;
    case 3: fill_metric<ptk::MetricLNInf>(t, q, perm, nq, radii, offsets, o); break;
    case 0: fill_metric<ptk::MetricL2>(t, q, perm, nq, radii, offsets, o); break;
    default: return -1;
  }
  return 0;
}

}  // extern "C"
