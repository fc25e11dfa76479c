// cluster.hpp -- cluster_within_self (ptk.h) as the contract reads, on the host: a sequential union-find
// over the rows of search_radius_self, then the border rule.  Shared by the library's host loop
// (ptk_host_cluster_within_self) and by kd_tree::cluster_within_self where the backend does not serve.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace pico_tree::internal {

// rows[i]: row i of search_radius_self (entries with an `index` member).  labels: rows.size() entries.
//   core      rows[i].size() >= min_neighbors
//   edges     core i -- core j whenever j is in row i (or i in row j: the union takes either direction)
//   labels    core: the smallest index among the core points of its component; non-core: the smallest label among the
//             core points of its own row, -1 without one.  A non-core point passes nothing on.
template <typename Rows_>
inline void cluster_rows(Rows_ const& rows, std::uint64_t min_neighbors, std::int32_t* labels) {
  std::size_t const n = rows.size();
  std::vector<std::int32_t> parent(n);
  std::vector<char> core(n);
  for (std::size_t i = 0; i < n; ++i) {
    parent[i] = static_cast<std::int32_t>(i);
    core[i] = rows[i].size() >= min_neighbors ? 1 : 0;
  }
  auto const find = [&](std::int32_t x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  };
  for (std::size_t i = 0; i < n; ++i) {
    if (!core[i]) continue;
    for (auto const& nb : rows[i]) {
      if (!core[static_cast<std::size_t>(nb.index)]) continue;
      std::int32_t const a = find(static_cast<std::int32_t>(i)), b = find(static_cast<std::int32_t>(nb.index));
      if (a != b) parent[a < b ? b : a] = a < b ? a : b;  // (the smaller index stays the root)
    }
  }
  for (std::size_t i = 0; i < n; ++i) {
    if (core[i]) labels[i] = find(static_cast<std::int32_t>(i));
  }
  for (std::size_t i = 0; i < n; ++i) {
    if (core[i]) continue;
    std::int32_t best = -1;
    for (auto const& nb : rows[i]) {
      std::size_t const j = static_cast<std::size_t>(nb.index);
      if (core[j] && (best < 0 || labels[j] < best)) best = labels[j];
    }
    labels[i] = best;
  }
}

}  // namespace pico_tree::internal
