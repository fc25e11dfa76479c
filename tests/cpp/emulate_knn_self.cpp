// tests/cpp/emulate_knn_self.cpp -- TEST INFRASTRUCTURE: the kernels of search_knn_self (knn_self_kernel,
// self_queries_kernel, drop_self_kernel) run lane by lane on the CPU, on the emulator of tests/cpp/emulate_kernels.cpp
// (whose handles, encoders and lane scheduler this unit reuses).  Built by tests/test_knn_self.py with the same g++ line
// and HIP stand-in as the emulator itself.

#include "emulate_kernels.cpp"

namespace {

// The direct kernel over leaf positions [lo, hi) in pieces of `piece`, the list size the host picks for k + 1.
template <class M>
int self_direct(Emu* t, uint64_t lo, uint64_t hi, uint32_t k, uint64_t piece, ptk::Neighbor* o) {
  if (t->dim > 3 || k + 1 > 64) return -1;
  for (uint64_t first = lo; first < hi; first += piece) {
    const uint64_t m = std::min(piece, hi - first);
    if (k + 1 <= 4)
      for_each_lane(m, [&] { ptk::knn_self_kernel<4, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, o); }, 64);
    else if (k + 1 <= 8)
      for_each_lane(m, [&] { ptk::knn_self_kernel<8, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, o); }, 64);
    else if (k + 1 <= 16)
      for_each_lane(m, [&] { ptk::knn_self_kernel<16, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, o); }, 64);
    else if (k + 1 <= 32)
      for_each_lane(m, [&] { ptk::knn_self_kernel<32, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, o); }, 64);
    else
      for_each_lane(m, [&] { ptk::knn_self_kernel<64, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, o); }, 64);
  }
  return 0;
}

// The staged route: per piece, self_queries_kernel, the emulator's k-NN search with k + 1 (the kernels emu_knn runs for
// a batch in the caller's order), drop_self_kernel.
int self_staged(void* h, Emu* t, uint64_t lo, uint64_t hi, uint32_t k, uint64_t piece, ptk::Neighbor* o) {
  const float4* recs = t->dim <= 3 ? t->dev.pts : nullptr;
  const float* pts = t->dim <= 3 ? nullptr : t->dev_nd.pts;
  const int32_t* index = t->dim <= 3 ? nullptr : t->dev_nd.index;
  std::vector<float> q((size_t)piece * t->dim);
  std::vector<ptk::Neighbor> rows((size_t)piece * (k + 1));
  for (uint64_t first = lo; first < hi; first += piece) {
    const uint64_t m = std::min(piece, hi - first);
    for_each_lane(m, [&] { ptk::self_queries_kernel<float>(recs, pts, t->dim, t->dim, first, m, q.data()); }, 256);
    const int rc = emu_knn(h, q.data(), m, k + 1, 1.0f, nullptr, 0, 0, reinterpret_cast<ptk_neighbor*>(rows.data()));
    if (rc != 0) return rc;
    for_each_lane(m, [&] {
      ptk::drop_self_kernel<ptk::Neighbor, float>(rows.data(), recs, index, first, m, k, 3.402823466e+38f, o);
    }, 256);
  }
  return 0;
}

}  // namespace

extern "C" {

// The rows of search_knn_self of the points at leaf positions [lo, hi), written to out + index * k (`out`: n_points x k):
// route 1 the direct kernel, 2 the staged route; `piece` leaf positions per launch (0: all at once).
int emu_knn_self(void* h, uint64_t lo, uint64_t hi, uint32_t k, int route, uint64_t piece, ptk_neighbor* out) {
  auto* t = static_cast<Emu*>(h);
  auto* o = reinterpret_cast<ptk::Neighbor*>(out);
  if (piece == 0) piece = hi - lo;
  if (hi <= lo) return 0;
  if (route == 2) return self_staged(h, t, lo, hi, k, piece, o);
  switch (t->metric) {
    case 1: return self_direct<ptk::MetricL1>(t, lo, hi, k, piece, o);
    case 2: return self_direct<ptk::MetricLInf>(t, lo, hi, k, piece, o);
    case 3: return self_direct<ptk::MetricLNInf>(t, lo, hi, k, piece, o);
    default: return self_direct<ptk::MetricL2>(t, lo, hi, k, piece, o);
  }
}

}  // extern "C"
