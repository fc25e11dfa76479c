// tests/cpp/emulate_aggregate.cpp -- TEST INFRASTRUCTURE: the kernels of aggregate_within_self / aggregate_within
// (pico_tree_amd/csrc/ptk_kernels_aggregate.hpp: aggregate_self_kernel, aggregate_within_kernel) run lane by lane on the
// CPU, on the emulator of tests/cpp/emulate_kernels.cpp with the handles of tests/cpp/emulate_radius_self.cpp.  The
// channel windows and the choice of the vector path are the launch layer's own (ptk::aggregate_windows).  Built by
// tests/test_aggregate_within.py with the emulator's g++ line and HIP stand-in.

#include "emulate_radius_self.cpp"
#include "ptk_kernels_aggregate.hpp"

namespace {

template <class M>
void aggregate_self_m(Emu* t, uint64_t piece, float radius, const float* radii, const float* values, uint32_t channels,
                      uint32_t flags, float* out, uint64_t* counts) {
  const uint64_t n = t->dev.n_points;
  for (uint64_t first = 0; first < n; first += piece) {
    const uint64_t m = std::min(piece, n - first);
    ptkd::with_bool(radii != nullptr, [&](auto per_row) {
      constexpr bool PER_ROW = decltype(per_row)::value;
      return ptk::aggregate_windows(values, out, channels, [&](auto W, auto VEC, uint32_t c0, uint32_t w) {
        for_each_lane(m, [&] {
          ptk::aggregate_self_kernel<W, VEC, 16, 2048, 64, 5, PER_ROW, M>(t->dev, t->dim, first, m, radius, radii, values,
                                                                          channels, c0, w, flags, out, counts);
        }, 64);
        return 0;
      });
    });
  }
}

template <class M>
void aggregate_within_m(Emu* t, const float* q, const uint32_t* perm, uint64_t nq, float radius, const float* radii,
                        const float* values, uint32_t channels, uint32_t flags, float* out, uint64_t* counts) {
  ptkd::with_bool(radii != nullptr, [&](auto per_row) {
    constexpr bool PER_ROW = decltype(per_row)::value;
    return ptk::aggregate_windows(values, out, channels, [&](auto W, auto VEC, uint32_t c0, uint32_t w) {
      for_each_lane(nq, [&] {
        ptk::aggregate_within_kernel<W, VEC, 16, 2048, 64, 5, PER_ROW, M>(t->dev, q, t->dim, perm, nq, radius, radii, values,
                                                                          channels, c0, w, flags, out, counts);
      }, 64);
      return 0;
    });
  });
}

}  // namespace

extern "C" {

// The accumulators a lane holds (the W of the tests' channel counts).
int emu_aggregate_width() { return ptk::kAggWidth; }

// 1 when a call with these buffers takes the vector path in its first window.
int emu_aggregate_vector_path(const float* values, const float* out, uint32_t channels) {
  return ptk::aggregate_vector_path(values, out, channels, 0) ? 1 : 0;
}

// out (n_points x channels by original index) and counts (may be null) of aggregate_self_kernel over every leaf
// position, `piece` positions per launch (0: all at once); radii null: the scalar form.
int emu_aggregate_self(void* h, uint64_t piece, float radius, const float* radii, const float* values, uint32_t channels,
                       uint32_t flags, float* out, uint64_t* counts) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3 || channels == 0) return -1;
  if (t->dev.n_points == 0) return 0;
  if (piece == 0) piece = t->dev.n_points;
  switch (t->metric) {
    case 1: aggregate_self_m<ptk::MetricL1>(t, piece, radius, radii, values, channels, flags, out, counts); break;
    case 2: aggregate_self_m<ptk::MetricLInf>(t, piece, radius, radii, values, channels, flags, out, counts); break;
    case 3: aggregate_self_m<ptk::MetricLNInf>(t, piece, radius, radii, values, channels, flags, out, counts); break;
    case 0: aggregate_self_m<ptk::MetricL2>(t, piece, radius, radii, values, channels, flags, out, counts); break;
    default: return -1;
  }
  return 0;
}

// The same of aggregate_within_kernel over nq query rows launched in the order `perm` (null: the caller's).
int emu_aggregate_within(void* h, const float* q, const uint32_t* perm, uint64_t nq, float radius, const float* radii,
                         const float* values, uint32_t channels, uint32_t flags, float* out, uint64_t* counts) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3 || channels == 0) return -1;
  if (nq == 0) return 0;
  switch (t->metric) {
    case 1: aggregate_within_m<ptk::MetricL1>(t, q, perm, nq, radius, radii, values, channels, flags, out, counts); break;
    case 2: aggregate_within_m<ptk::MetricLInf>(t, q, perm, nq, radius, radii, values, channels, flags, out, counts); break;
    case 3: aggregate_within_m<ptk::MetricLNInf>(t, q, perm, nq, radius, radii, values, channels, flags, out, counts); break;
    case 0: aggregate_within_m<ptk::MetricL2>(t, q, perm, nq, radius, radii, values, channels, flags, out, counts); break;
    default: return -1;
  }
  return 0;
}

}  // extern "C"
