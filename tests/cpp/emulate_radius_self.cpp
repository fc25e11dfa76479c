// tests/cpp/emulate_radius_self.cpp -- TEST INFRASTRUCTURE: the kernels of search_radius_self / count_within_self
// (pico_tree_amd/csrc/ptk_kernels_selfr.hpp: count_self_kernel, radius_self_fill_kernel and their float64 pair) run lane
// by lane on the CPU, on the emulator of tests/cpp/emulate_kernels.cpp (whose handles, encoders and lane scheduler this
// unit reuses).  Built by tests/test_radius_self.py with the same g++ line and HIP stand-in as the emulator itself.

#include "emulate_kernels.cpp"
#include "ptk_kernels_selfr.hpp"

namespace {

// The side table of the count kernels, built by the table kernels themselves (as tests/cpp/emulate_count_within.cpp).
std::vector<ptk::CountBox> table_of(Emu* t) {
  const uint32_t nb = (uint32_t)t->enc.nodes.size();
  std::vector<ptk::CountBox> table(nb > 0 ? nb : 1);
  std::vector<uint32_t> info(nb > 0 ? nb : 1), arrive(nb > 0 ? nb : 1);
  if (nb > 0) {
    for_each_lane(nb, [&] { ptk::count_parents_kernel(t->dev, nb, info.data(), arrive.data()); }, 256);
    for_each_lane(nb, [&] { ptk::count_table_kernel(t->dev, nb, info.data(), arrive.data(), table.data()); }, 256);
  }
  return table;
}
std::vector<ptk::CountBox64> table64_of(Emu64* t) {
  const uint32_t nb = (uint32_t)t->enc.nodes.size();
  std::vector<ptk::CountBox64> table(nb > 0 ? nb : 1);
  std::vector<uint32_t> info(nb > 0 ? nb : 1), arrive(nb > 0 ? nb : 1);
  if (nb > 0) {
    for_each_lane(nb, [&] { ptk::count64_parents_kernel(t->dev, nb, info.data(), arrive.data()); }, 256);
    for_each_lane(nb, [&] { ptk::count64_table_kernel(t->dev, nb, info.data(), arrive.data(), table.data()); }, 256);
  }
  return table;
}

// Leaf positions [lo, hi) in launches of `piece` positions each, the per-row form when `radii` is given.
template <class M>
void count_self_m(Emu* t, const ptk::CountBox* table, uint64_t lo, uint64_t hi, uint64_t piece, float radius, const float* radii,
                  uint64_t max_count, uint32_t shortcut, uint64_t* counts, uint32_t* stats) {
  for (uint64_t first = lo; first < hi; first += piece) {
    const uint64_t m = std::min(piece, hi - first);
    if (radii != nullptr)
      for_each_lane(m, [&] {
        ptk::count_self_kernel<16, 2048, 64, 5, true, M>(t->dev, table, t->dim, first, m, radius, radii, max_count, shortcut,
                                                         counts, stats);
      }, 64);
    else
      for_each_lane(m, [&] {
        ptk::count_self_kernel<16, 2048, 64, 5, false, M>(t->dev, table, t->dim, first, m, radius, radii, max_count, shortcut,
                                                          counts, stats);
      }, 64);
  }
}
template <class M>
void fill_self_m(Emu* t, uint64_t lo, uint64_t hi, uint64_t piece, float radius, const float* radii, const uint64_t* offsets,
                 ptk::Neighbor* o) {
  for (uint64_t first = lo; first < hi; first += piece) {
    const uint64_t m = std::min(piece, hi - first);
    if (radii != nullptr)
      for_each_lane(m, [&] {
        ptk::radius_self_fill_kernel<16, 2048, 64, 5, true, M>(t->dev, t->dim, first, m, radius, radii, offsets, o);
      }, 64);
    else
      for_each_lane(m, [&] {
        ptk::radius_self_fill_kernel<16, 2048, 64, 5, false, M>(t->dev, t->dim, first, m, radius, radii, offsets, o);
      }, 64);
  }
}
template <class M>
void count64_self_m(Emu64* t, const ptk::CountBox64* table, uint64_t piece, double radius, const double* radii,
                    uint64_t max_count, uint32_t shortcut, uint64_t* counts, uint32_t* stats) {
  const uint64_t n = t->dev.n_points;
  for (uint64_t first = 0; first < n; first += piece) {
    for_each_lane64(t, std::min(piece, n - first), [&](uint64_t q0, uint64_t m) {
      if (radii != nullptr)
        ptk::count64_self_kernel<M, true>(t->dev, table, first + q0, m, radius, radii, max_count, shortcut, counts,
                                          t->stack.data(), t->slots, stats);
      else
        ptk::count64_self_kernel<M, false>(t->dev, table, first + q0, m, radius, radii, max_count, shortcut, counts,
                                           t->stack.data(), t->slots, stats);
    });
  }
}
template <class M>
void fill64_self_m(Emu64* t, uint64_t piece, double radius, const double* radii, const uint64_t* offsets, ptk::Neighbor64* o) {
  const uint64_t n = t->dev.n_points;
  for (uint64_t first = 0; first < n; first += piece) {
    for_each_lane64(t, std::min(piece, n - first), [&](uint64_t q0, uint64_t m) {
      if (radii != nullptr)
        ptk::radius64_self_fill_kernel<M, true>(t->dev, first + q0, m, radius, radii, offsets, o, t->stack.data(), t->slots);
      else
        ptk::radius64_self_fill_kernel<M, false>(t->dev, first + q0, m, radius, radii, offsets, o, t->stack.data(), t->slots);
    });
  }
}

}  // namespace

extern "C" {

// counts[index] of count_self_kernel for the points at leaf positions [lo, hi) (`counts`: n_points entries), `piece` leaf
// positions per launch (0: all at once); radii null: the scalar form.  stats[4]: the shortcuts taken (inside, outside),
// the inside tests refused for a subnormal radius and those refused because the box holds the lane's own point.
int emu_count_self(void* h, uint64_t lo, uint64_t hi, uint64_t piece, float radius, const float* radii, uint64_t max_count,
                   int shortcut, uint64_t* counts, uint32_t* stats) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3) return -1;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (hi <= lo) return 0;
  if (piece == 0) piece = hi - lo;
  const std::vector<ptk::CountBox> table = table_of(t);
  const uint32_t sc = (uint32_t)shortcut;
  switch (t->metric) {
    case 1: count_self_m<ptk::MetricL1>(t, table.data(), lo, hi, piece, radius, radii, max_count, sc, counts, stats); break;
    case 2: count_self_m<ptk::MetricLInf>(t, table.data(), lo, hi, piece, radius, radii, max_count, sc, counts, stats); break;
    case 3: count_self_m<ptk::MetricLNInf>(t, table.data(), lo, hi, piece, radius, radii, max_count, sc, counts, stats); break;
    case 0: count_self_m<ptk::MetricL2>(t, table.data(), lo, hi, piece, radius, radii, max_count, sc, counts, stats); break;
    default: return -1;
  }
  return 0;
}

// The rows of radius_self_fill_kernel for leaf positions [lo, hi), written at out + offsets[index]; sort_rows != 0: the
// row sort of the fill forms over that many rows afterwards (`offsets` then holds sort_rows + 1 valid entries).
int emu_radius_self_fill(void* h, uint64_t lo, uint64_t hi, uint64_t piece, float radius, const float* radii,
                         const uint64_t* offsets, ptk_neighbor* out, uint64_t sort_rows) {
  auto* t = static_cast<Emu*>(h);
  auto* o = reinterpret_cast<ptk::Neighbor*>(out);
  if (t->dim > 3) return -1;
  if (hi <= lo) return 0;
  if (piece == 0) piece = hi - lo;
  switch (t->metric) {
    case 1: fill_self_m<ptk::MetricL1>(t, lo, hi, piece, radius, radii, offsets, o); break;
    case 2: fill_self_m<ptk::MetricLInf>(t, lo, hi, piece, radius, radii, offsets, o); break;
    case 3: fill_self_m<ptk::MetricLNInf>(t, lo, hi, piece, radius, radii, offsets, o); break;
    case 0: fill_self_m<ptk::MetricL2>(t, lo, hi, piece, radius, radii, offsets, o); break;
    default: return -1;
  }
  if (sort_rows) for_each_lane(sort_rows, [&] { ptk::sort_rows_kernel(sort_rows, offsets, o); });
  return 0;
}

// The same pair for a float64 tree of tests/emu.py's EmulatedTree64 (dim <= 3), all leaf positions.
int emu64_count_self(void* h, uint64_t piece, double radius, const double* radii, uint64_t max_count, int shortcut,
                     uint64_t* counts, uint32_t* stats) {
  auto* t = static_cast<Emu64*>(h);
  if (t->dev.dim > 3) return -1;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (piece == 0) piece = t->dev.n_points;
  const std::vector<ptk::CountBox64> table = table64_of(t);
  const uint32_t sc = (uint32_t)shortcut;
  switch (t->metric) {
    case 1: count64_self_m<ptk::Metric64L1>(t, table.data(), piece, radius, radii, max_count, sc, counts, stats); break;
    case 2: count64_self_m<ptk::Metric64LInf>(t, table.data(), piece, radius, radii, max_count, sc, counts, stats); break;
    case 3: count64_self_m<ptk::Metric64LNInf>(t, table.data(), piece, radius, radii, max_count, sc, counts, stats); break;
    case 0: count64_self_m<ptk::Metric64L2>(t, table.data(), piece, radius, radii, max_count, sc, counts, stats); break;
    default: return -1;
  }
  return 0;
}

int emu64_radius_self_fill(void* h, uint64_t piece, double radius, const double* radii, const uint64_t* offsets,
                           ptk::Neighbor64* out, int sort) {
  auto* t = static_cast<Emu64*>(h);
  if (t->dev.dim > 3) return -1;
  const uint64_t n = t->dev.n_points;
  if (piece == 0) piece = n;
  switch (t->metric) {
    case 1: fill64_self_m<ptk::Metric64L1>(t, piece, radius, radii, offsets, out); break;
    case 2: fill64_self_m<ptk::Metric64LInf>(t, piece, radius, radii, offsets, out); break;
    case 3: fill64_self_m<ptk::Metric64LNInf>(t, piece, radius, radii, offsets, out); break;
    case 0: fill64_self_m<ptk::Metric64L2>(t, piece, radius, radii, offsets, out); break;
    default: return -1;
  }
  if (sort) for_each_lane(n, [&] { ptk::sort_rows64_kernel(offsets, n, out); });
  return 0;
}

}  // extern "C"
