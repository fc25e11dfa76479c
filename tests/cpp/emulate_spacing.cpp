// tests/cpp/emulate_spacing.cpp -- TEST INFRASTRUCTURE: the kernels of spacing_knn_self
// (pico_tree_amd/csrc/ptk_kernels_spacing.hpp, K24: spacing_self_kernel, spacing_rows_kernel, spacing_level0_kernel,
// spacing_finish_kernel, spacing_keep_kernel, with align_reduce_kernel for the upper levels) run lane by lane on the CPU,
// on the emulator of tests/cpp/emulate_kernels.cpp: the wavefronts of the reducing kernels as 64 fibers that meet at every
// shuffle.  Built by tests/test_spacing_self.py with the emulator's g++ line and HIP stand-in.

#include "emulate_kernels.cpp"
#include "ptk_kernels_spacing.hpp"

namespace {

// The direct kernel over leaf positions [lo, hi) in pieces of `piece`, the list size the host picks for k + 1.
template <class M>
int spacing_direct(Emu* t, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t piece, float* mean, float* kth) {
  if (t->dim > 3 || k + 1 > 64) return -1;
  for (uint64_t first = lo; first < hi; first += piece) {
    const uint64_t m = std::min(piece, hi - first);
    if (k + 1 <= 4)
      for_each_lane(m, [&] { ptk::spacing_self_kernel<4, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, flags, mean, kth); }, 64);
    else if (k + 1 <= 8)
      for_each_lane(m, [&] { ptk::spacing_self_kernel<8, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, flags, mean, kth); }, 64);
    else if (k + 1 <= 16)
      for_each_lane(m, [&] { ptk::spacing_self_kernel<16, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, flags, mean, kth); }, 64);
    else if (k + 1 <= 32)
      for_each_lane(m, [&] { ptk::spacing_self_kernel<32, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, flags, mean, kth); }, 64);
    else
      for_each_lane(m, [&] { ptk::spacing_self_kernel<64, 16, 2048, 64, 5, M>(t->dev, t->dim, first, m, k, flags, mean, kth); }, 64);
  }
  return 0;
}

// The staged route: per piece, self_queries_kernel, the emulator's k-NN search with k + 1, spacing_rows_kernel.
int spacing_staged(void* h, Emu* t, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t piece, float* mean,
                   float* kth) {
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
      ptk::spacing_rows_kernel<ptk::Neighbor, float>(rows.data(), recs, index, first, m, k, flags, mean, kth);
    }, 256);
  }
  return 0;
}

}  // namespace

extern "C" {

// mean[index] and kth[index] (may be null) of the points at leaf positions [lo, hi): route 1 the direct kernel, 2 the
// staged route; `piece` leaf positions per launch (0: all at once).
int emu_spacing_knn_self(void* h, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, int route, uint64_t piece, float* mean,
                         float* kth) {
  auto* t = static_cast<Emu*>(h);
  if (piece == 0) piece = hi - lo;
  if (hi <= lo) return 0;
  if (route == 2) return spacing_staged(h, t, lo, hi, k, flags, piece, mean, kth);
  switch (t->metric) {
    case 1: return spacing_direct<ptk::MetricL1>(t, lo, hi, k, flags, piece, mean, kth);
    case 2: return spacing_direct<ptk::MetricLInf>(t, lo, hi, k, flags, piece, mean, kth);
    case 3: return spacing_direct<ptk::MetricLNInf>(t, lo, hi, k, flags, piece, mean, kth);
    default: return spacing_direct<ptk::MetricL2>(t, lo, hi, k, flags, piece, mean, kth);
  }
}

// The record (64 bytes) and the mask of the statistics kernels over n means: the two passes of the summation tree, their
// finishes, the keep kernel -- the launches of ptk_family_spacing.hip.
int emu_spacing_statistics(const float* mean, uint64_t n, float ratio, uint8_t* keep, void* stats_out) {
  namespace al = pico_tree::internal;
  if (n == 0) return -1;
  auto* stats = static_cast<al::spacing_stats*>(stats_out);
  for (int second = 0; second < 2; ++second) {
    uint64_t m = al::align_blocks(n);
    std::vector<double> sums((size_t)m);
    std::vector<uint64_t> counts((size_t)m);
    for_each_wave((uint32_t)m, [&] {
      if (second == 0)
        ptk::spacing_level0_kernel<float, false>(mean, n, stats, m, sums.data(), counts.data());
      else
        ptk::spacing_level0_kernel<float, true>(mean, n, stats, m, sums.data(), counts.data());
    });
    while (m > 1) {
      const uint64_t up = al::align_blocks(m);
      std::vector<double> next((size_t)up);
      std::vector<uint64_t> next_counts((size_t)up);
      for_each_wave((uint32_t)up, [&] {
        ptk::align_reduce_kernel(sums.data(), counts.data(), m, 1, up, next.data(), next_counts.data());
      });
      sums.swap(next);
      counts.swap(next_counts);
      m = up;
    }
    for_each_lane(64, [&] { ptk::spacing_finish_kernel(sums.data(), counts.data(), second, n, ratio, stats); }, 64);
  }
  for_each_lane(n, [&] { ptk::spacing_keep_kernel<float>(mean, n, stats, keep); }, 256);
  return 0;
}

}  // extern "C"
