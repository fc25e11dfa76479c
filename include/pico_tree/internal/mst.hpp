// mst.hpp -- mst_within_self (ptk.h): the weight of an edge, the ORDER of the edges and the minimum
// spanning forest of the rows of search_radius_self, as the contract reads.  ONE statement of the order: compiled for
// the device by the kernels of pico_tree_amd/csrc/ptk_kernels_mst.hpp (K25), for the library's host loop
// (ptk_host_mst_within_self) and for kd_tree::mst_within_self where the backend does not serve.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define PICO_TREE_HD __host__ __device__
#else
#define PICO_TREE_HD
#endif

namespace pico_tree::internal {

//! One edge of the forest, as every form writes it: 12 bytes.
struct mst_edge {
  std::uint32_t lo;
  std::uint32_t hi;
  float w;
};
static_assert(sizeof(mst_edge) == 12, "record layout");

//! The weight of the pair {i, j} at row distance \p d: d without core distances, else max(d, core_i, core_j).
PICO_TREE_HD inline float mst_weight(float d, float core_i, float core_j) {
  float w = d;
  w = core_i > w ? core_i : w;
  w = core_j > w ? core_j : w;
  return w;
}

//! The first two parts of the triple (bits(w), lo, hi) as one word: weights are non-negative, so the bit order is the
//! value order.
PICO_TREE_HD inline std::uint64_t mst_wlo(std::uint32_t w_bits, std::uint32_t lo) {
  return (static_cast<std::uint64_t>(w_bits) << 32) | static_cast<std::uint64_t>(lo);
}

//! THE order of the edges: (bits(w), lo, hi) lexicographically.  The triples of distinct pairs are distinct, so the
//! minimum spanning forest is unique; equal weights are decided here and nowhere else.
PICO_TREE_HD inline bool mst_less(std::uint64_t wlo_a, std::uint32_t hi_a, std::uint64_t wlo_b, std::uint32_t hi_b) {
  return wlo_a < wlo_b || (wlo_a == wlo_b && hi_a < hi_b);
}

PICO_TREE_HD inline std::uint32_t mst_bits(float w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(w);
#else
  std::uint32_t b;
  std::memcpy(&b, &w, sizeof b);
  return b;
#endif
}

inline bool mst_edge_less(mst_edge const& a, mst_edge const& b) {
  return mst_less(mst_wlo(mst_bits(a.w), a.lo), a.hi, mst_wlo(mst_bits(b.w), b.lo), b.hi);
}

//! Ascending in the order of the contract: what the host forms return, so that two calls give identical bytes.
inline void mst_sort(mst_edge* edges, std::size_t n) { std::sort(edges, edges + n, mst_edge_less); }

//! The index of the first NaN or negative entry among \p n core distances, \p n without one.
inline std::size_t mst_first_bad_core(float const* core, std::size_t n) {
  for (std::size_t i = 0; i < n; ++i) {
    if (!(core[i] >= 0.0f)) return i;
  }
  return n;
}

// rows[i]: row i of search_radius_self at `radius` (entries with `index` and `distance` members).
//   edges   {i, j} whenever j is in row i or i is in row j; w = d, or max(d, core_i, core_j) and then only if w < radius
//   result  Kruskal over the edges ascending in mst_less; `edges` (rows.size() - 1 records at most) ascending; labels
//           (may be null): the smallest index of the point's component.  Returns the number of edges written.
template <typename Rows_>
inline std::uint64_t mst_rows(Rows_ const& rows, float radius, float const* core, mst_edge* edges, std::int32_t* labels) {
  std::size_t const n = rows.size();
  std::vector<mst_edge> all;
  for (std::size_t i = 0; i < n; ++i) {
    for (auto const& nb : rows[i]) {
      std::size_t const j = static_cast<std::size_t>(nb.index);
      float const d = static_cast<float>(nb.distance);
      float const w = core != nullptr ? mst_weight(d, core[i], core[j]) : d;
      if (core != nullptr && !(w < radius)) continue;
      all.push_back(mst_edge{static_cast<std::uint32_t>(std::min(i, j)), static_cast<std::uint32_t>(std::max(i, j)), w});
    }
  }
  std::sort(all.begin(), all.end(), mst_edge_less);
  std::vector<std::int32_t> parent(n);
  for (std::size_t i = 0; i < n; ++i) parent[i] = static_cast<std::int32_t>(i);
  auto const find = [&](std::int32_t x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  };
  std::uint64_t count = 0;
  for (mst_edge const& e : all) {
    std::int32_t const a = find(static_cast<std::int32_t>(e.lo)), b = find(static_cast<std::int32_t>(e.hi));
    if (a == b) continue;
    parent[a < b ? b : a] = a < b ? a : b;  // (the smaller index stays the root)
    edges[count++] = e;
  }
  if (labels != nullptr) {
    for (std::size_t i = 0; i < n; ++i) labels[i] = find(static_cast<std::int32_t>(i));
  }
  return count;
}

}  // namespace pico_tree::internal
