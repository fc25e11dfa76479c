// tests/cpp/emulate_within_radii.cpp -- TEST INFRASTRUCTURE: the per-row kernels of search_knn_within_radii and
// count_within_radii (knn_reg_within_radii_kernel, knn_within_radii_kernel, their nd twins, count_within_radii_kernel) run
// lane by lane on the CPU, on the emulator of tests/cpp/emulate_kernels.cpp (whose handles, encoders and lane scheduler
// this unit reuses).  Built by tests/test_within_radii.py with the same g++ line and HIP stand-in as the emulator itself.

#include "emulate_kernels.cpp"
#include "ptk_kernels_count.hpp"

namespace {
// form: 0 the register list, 1 the list in LDS, 2 the list in the output row
template <class M>
int within_radii_metric(Emu* t, const float* q, const uint32_t* perm, uint64_t nq, uint32_t k, const float* radii,
                        uint32_t unseeded, int form, ptk::Neighbor* o) {
  if (t->dim > 3) {
    if (form == 0 && k <= 4)
      for_each_lane(nq, [&] { ptk::knn_nd_reg_within_radii_kernel<4, 16, 2048, M>(t->dev_nd, q, perm, nq, k, o, radii, unseeded); }, 64);
    else if (form == 0 && k <= 16)
      for_each_lane(nq, [&] { ptk::knn_nd_reg_within_radii_kernel<16, 16, 2048, M>(t->dev_nd, q, perm, nq, k, o, radii, unseeded); }, 64);
    else if (form == 0 && k <= 64)
      for_each_lane(nq, [&] { ptk::knn_nd_reg_within_radii_kernel<64, 16, 2048, M>(t->dev_nd, q, perm, nq, k, o, radii, unseeded); }, 64);
    else if (form == 1)
      for_each_lane(nq, [&] { ptk::knn_nd_within_radii_kernel<16, 2048, true, M>(t->dev_nd, q, perm, nq, k, o, radii, unseeded); }, 64);
    else if (form == 2)
      for_each_lane(nq, [&] { ptk::knn_nd_within_radii_kernel<16, 2048, false, M>(t->dev_nd, q, perm, nq, k, o, radii, unseeded); }, 64);
    else
      return -1;
    return 0;
  }
  if (form == 0 && k <= 4)
    for_each_lane(nq, [&] { ptk::knn_reg_within_radii_kernel<4, 16, 2048, 64, 4, M>(t->dev, q, t->dim, perm, nq, k, o, radii, unseeded); }, 64);
  else if (form == 0 && k <= 16)
    for_each_lane(nq, [&] { ptk::knn_reg_within_radii_kernel<16, 16, 2048, 64, 4, M>(t->dev, q, t->dim, perm, nq, k, o, radii, unseeded); }, 64);
  else if (form == 0 && k <= 64)
    for_each_lane(nq, [&] { ptk::knn_reg_within_radii_kernel<64, 16, 2048, 64, 4, M>(t->dev, q, t->dim, perm, nq, k, o, radii, unseeded); }, 64);
  else if (form == 1)
    for_each_lane(nq, [&] { ptk::knn_within_radii_kernel<16, 2048, 64, 4, true, M>(t->dev, q, t->dim, perm, nq, k, o, radii, unseeded); }, 64);
  else if (form == 2)
    for_each_lane(nq, [&] { ptk::knn_within_radii_kernel<16, 2048, 64, 4, false, M>(t->dev, q, t->dim, perm, nq, k, o, radii, unseeded); }, 64);
  else
    return -1;
  return 0;
}

template <class M>
void count_radii_metric(Emu* t, const ptk::CountBox* table, const float* q, const uint32_t* perm, uint64_t nq,
                        const float* radii, uint64_t max_count, uint32_t shortcut, uint64_t* counts, uint32_t* stats) {
  for_each_lane(nq, [&] {
    ptk::count_within_radii_kernel<16, 2048, 64, 4, M>(t->dev, table, q, t->dim, perm, nq, radii, max_count, shortcut,
                                                       counts, stats);
  }, 64);
}
}  // namespace

extern "C" {

// Rows of nq x k: the search_knn_within_radii rows of the kernel `form`; `perm` (null: as given) is the launch order,
// radii[i] belongs to query row i.  The lanes seed their lists as the backend's launch does (unseeded: the metrics
// whose box distance is no lower bound).
int emu_knn_within_radii(void* h, const float* q, const uint32_t* perm, uint64_t nq, uint32_t k, const float* radii,
                         int form, ptk_neighbor* out) {
  auto* t = static_cast<Emu*>(h);
  auto* o = reinterpret_cast<ptk::Neighbor*>(out);
  switch (t->metric) {
    case 1: return within_radii_metric<ptk::MetricL1>(t, q, perm, nq, k, radii, 0u, form, o);
    case 2: return within_radii_metric<ptk::MetricLInf>(t, q, perm, nq, k, radii, 1u, form, o);
    case 3: return within_radii_metric<ptk::MetricLNInf>(t, q, perm, nq, k, radii, 1u, form, o);
    default: return within_radii_metric<ptk::MetricL2>(t, q, perm, nq, k, radii, 0u, form, o);
  }
}

// counts[i] of count_within_radii_kernel (dim <= 3), the side table built by the table kernels first.  stats[3]: the
// shortcuts taken (inside, outside) and the inside tests refused for a subnormal radius, summed over the batch.
int emu_count_within_radii(void* h, const float* q, const uint32_t* perm, uint64_t nq, const float* radii,
                           uint64_t max_count, int shortcut, uint64_t* counts, uint32_t* stats) {
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
  const uint32_t sc = (uint32_t)shortcut;
  switch (t->metric) {
    case 1: count_radii_metric<ptk::MetricL1>(t, table.data(), q, perm, nq, radii, max_count, sc, counts, stats); break;
    case 2: count_radii_metric<ptk::MetricLInf>(t, table.data(), q, perm, nq, radii, max_count, sc, counts, stats); break;
    case 3: count_radii_metric<ptk::MetricLNInf>(t, table.data(), q, perm, nq, radii, max_count, sc, counts, stats); break;
    case 0: count_radii_metric<ptk::MetricL2>(t, table.data(), q, perm, nq, radii, max_count, sc, counts, stats); break;
    default: return -1;
  }
  return 0;
}

}  // extern "C"
