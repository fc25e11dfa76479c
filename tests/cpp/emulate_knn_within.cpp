// tests/cpp/emulate_knn_within.cpp -- TEST INFRASTRUCTURE: the bounded k-NN kernels of search_knn_within
// (knn_reg_within_kernel, knn_within_kernel, knn_nd_reg_within_kernel, knn_nd_within_kernel) run lane by lane on the
// CPU, on the emulator of tests/cpp/emulate_kernels.cpp (whose handles, encoders and lane scheduler this unit reuses).
// Built by tests/test_knn_within.py with the same g++ line and HIP stand-in as the emulator itself.

#include "emulate_kernels.cpp"

namespace {
// form: 0 the register list, 1 the list in LDS, 2 the list in the output row
template <class M>
int within_metric(Emu* t, const float* q, uint64_t nq, uint32_t k, float seed, float radius, int form, ptk::Neighbor* o) {
  if (t->dim > 3) {
    if (form == 0 && k <= 4)
      for_each_lane(nq, [&] { ptk::knn_nd_reg_within_kernel<4, 16, 2048, M>(t->dev_nd, q, nullptr, nq, k, o, seed, radius); }, 64);
    else if (form == 0 && k <= 16)
      for_each_lane(nq, [&] { ptk::knn_nd_reg_within_kernel<16, 16, 2048, M>(t->dev_nd, q, nullptr, nq, k, o, seed, radius); }, 64);
    else if (form == 0 && k <= 64)
      for_each_lane(nq, [&] { ptk::knn_nd_reg_within_kernel<64, 16, 2048, M>(t->dev_nd, q, nullptr, nq, k, o, seed, radius); }, 64);
    else if (form == 1)
      for_each_lane(nq, [&] { ptk::knn_nd_within_kernel<16, 2048, true, M>(t->dev_nd, q, nullptr, nq, k, o, seed, radius); }, 64);
    else if (form == 2)
      for_each_lane(nq, [&] { ptk::knn_nd_within_kernel<16, 2048, false, M>(t->dev_nd, q, nullptr, nq, k, o, seed, radius); }, 64);
    else
      return -1;
    return 0;
  }
  if (form == 0 && k <= 4)
    for_each_lane(nq, [&] { ptk::knn_reg_within_kernel<4, 16, 2048, 64, 4, M>(t->dev, q, t->dim, nullptr, nq, k, o, seed, radius); }, 64);
  else if (form == 0 && k <= 16)
    for_each_lane(nq, [&] { ptk::knn_reg_within_kernel<16, 16, 2048, 64, 4, M>(t->dev, q, t->dim, nullptr, nq, k, o, seed, radius); }, 64);
  else if (form == 0 && k <= 64)
    for_each_lane(nq, [&] { ptk::knn_reg_within_kernel<64, 16, 2048, 64, 4, M>(t->dev, q, t->dim, nullptr, nq, k, o, seed, radius); }, 64);
  else if (form == 1)
    for_each_lane(nq, [&] { ptk::knn_within_kernel<16, 2048, 64, 4, true, M>(t->dev, q, t->dim, nullptr, nq, k, o, seed, radius); }, 64);
  else if (form == 2)
    for_each_lane(nq, [&] { ptk::knn_within_kernel<16, 2048, 64, 4, false, M>(t->dev, q, t->dim, nullptr, nq, k, o, seed, radius); }, 64);
  else
    return -1;
  return 0;
}
}  // namespace

extern "C" {

// Rows of nq x k: the search_knn_within rows of the kernel `form`, its list seeded at `seed` (FLT_MAX: unseeded).
int emu_knn_within(void* h, const float* q, uint64_t nq, uint32_t k, float seed, float radius, int form,
                   ptk_neighbor* out) {
  auto* t = static_cast<Emu*>(h);
  auto* o = reinterpret_cast<ptk::Neighbor*>(out);
  switch (t->metric) {
    case 1: return within_metric<ptk::MetricL1>(t, q, nq, k, seed, radius, form, o);
    case 2: return within_metric<ptk::MetricLInf>(t, q, nq, k, seed, radius, form, o);
    case 3: return within_metric<ptk::MetricLNInf>(t, q, nq, k, seed, radius, form, o);
    default: return within_metric<ptk::MetricL2>(t, q, nq, k, seed, radius, form, o);
  }
}

}  // extern "C"
