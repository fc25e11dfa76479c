// ptk_host_loop.hpp -- ptk_host_search_*: the reference's own batch loop on the host, for the calls the DEVICE search
// refuses (PTK_ERR_UNSUPPORTED: a topological tree deeper than the device stack, a dimension beyond the LDS staging).
//
// This is NOT a fallback of ptk_search_*: those entry points never come here -- without a usable device, or on any
// HIP failure, they fail (PTK_ERR_DEVICE) and the caller sees it.  The wrappers (pico_tree_amd.KdTree; the C++ batched
// members do the same with their own per-query members) call these entry points by name, and only after a device search
// has answered PTK_ERR_UNSUPPORTED for a valid tree, with a warning: that call is then served the way the reference
// serves every call -- a loop of per-query searches over the rows, `schedule(dynamic, 128)`
// (_pyco_tree/kd_tree.hpp:117-135, :179-200, :245-268) -- by the header-only host traversal of
// include/pico_tree/internal/flat_search.hpp on the flat tree the handle keeps.  The points are the caller's: a handle
// holds them on the device only.
//
// Included by ptk_backend.hip (needs ptk_tree and fail()).
#pragma once

#include <atomic>
#include <exception>
#include <system_error>
#include <thread>
#include <vector>

#include "pico_tree/internal/aggregate.hpp"
#include "pico_tree/internal/align.hpp"
#include "pico_tree/internal/cluster.hpp"
#include "pico_tree/internal/flat_search.hpp"
#include "pico_tree/internal/suppress.hpp"
#include "pico_tree/internal/spacing.hpp"
#include "pico_tree/internal/local_frame.hpp"
#include "pico_tree/internal/visitors.hpp"
#include "pico_tree/metric.hpp"

namespace ptk_host {

using namespace pico_tree;
using flat_t = internal::flat_tree<int, float, dynamic_extent>;
using space_t = space_map<point_map<float const, dynamic_extent>>;
using view_t = internal::space_view<space_t>;
using query_t = internal::point_view<point_map<float const, dynamic_extent>>;
using neighbor_t = neighbor<int, float>;

inline flat_t make_flat(const ptk_tree* t) {
  static_assert(sizeof(flat_t::node_type) == sizeof(ptk_node), "node layout");
  flat_t flat(t->dim);
  flat.indices.assign(t->indices.begin(), t->indices.end());
  flat.nodes.resize(t->nodes.size());
  std::memcpy(static_cast<void*>(flat.nodes.data()), t->nodes.data(), t->nodes.size() * sizeof(ptk_node));
  for (uint32_t d = 0; d < t->dim; ++d) {
    flat.root_box.min(d) = t->root_min[d];
    flat.root_box.max(d) = t->root_max[d];
  }
  flat.max_depth = t->max_depth;
  if (t->outer.size() == 2 * t->nodes.size()) {
    flat.keep_outer_bounds = true;
    flat.outer_bounds.resize(t->nodes.size());
    std::memcpy(static_cast<void*>(flat.outer_bounds.data()), t->outer.data(), t->outer.size() * sizeof(float));
  }
  return flat;
}
// The handle's flat view: built by the first host search, shared by the later ones (and by concurrent ones).
inline std::shared_ptr<const flat_t> flat_of(const ptk_tree* t) {
  std::lock_guard<std::mutex> lock(t->host_flat_mutex);
  if (!t->host_flat) t->host_flat = std::make_shared<const flat_t>(make_flat(t));
  return std::static_pointer_cast<const flat_t>(t->host_flat);
}

// fn(i) for every row, rows handed out 128 at a time.
template <class Fn>
inline void rows_loop(uint64_t n, Fn fn) {
  constexpr uint64_t chunk = 128;
  unsigned workers = std::thread::hardware_concurrency();
  workers = workers == 0 ? 1u : workers;
  workers = (unsigned)std::min<uint64_t>(workers, (n + chunk - 1) / chunk);
  std::atomic<uint64_t> next{0};
  std::exception_ptr failure;
  std::mutex failure_mutex;
  auto work = [&] {
    try {
      for (;;) {
        const uint64_t lo = next.fetch_add(chunk);
        if (lo >= n) break;
        const uint64_t hi = std::min(n, lo + chunk);
        for (uint64_t i = lo; i < hi; ++i) fn(i);
      }
    } catch (...) {
      std::lock_guard<std::mutex> lock(failure_mutex);
      if (!failure) failure = std::current_exception();
      next.store(n);
    }
  };
  // (a thread that cannot be started -- a limit of the process -- is simply one worker fewer: the rows are dealt out in
  // chunks, whoever is there takes them; and the threads that did start are joined on every way out)
  std::vector<std::thread> pool;
  struct join_all {
    std::vector<std::thread>& threads;
    ~join_all() {
      for (auto& th : threads)
        if (th.joinable()) th.join();
    }
  } joiner{pool};
  try {
    pool.reserve(workers);
    for (unsigned w = 1; w < workers; ++w) pool.emplace_back(work);
  } catch (const std::system_error&) {
  }
  work();
  for (auto& th : pool) th.join();
  if (failure) std::rethrow_exception(failure);
}

// One traversal of query row x with visitor v under the handle's metric.
template <class Visitor>
inline void search_one(const ptk_tree* t, const flat_t& flat, const view_t& view, const float* x, Visitor& v) {
  const point_map<float const, dynamic_extent> row(x, t->dim);  // (the view refers to it)
  query_t q(row);
  switch (t->metric.load()) {
    case PTK_METRIC_L1: internal::nearest_search(flat, view, metric_l1(), q, v); break;
    case PTK_METRIC_LPINF: internal::nearest_search(flat, view, metric_lpinf(), q, v); break;
    case PTK_METRIC_LNINF: internal::nearest_search(flat, view, metric_lninf(), q, v); break;
    case PTK_METRIC_SO2: {
      metric_so2 m;
      internal::nearest_search_topological<flat_t, view_t, metric_so2, query_t, Visitor>(flat, view, m, q, v)();
    } break;
    case PTK_METRIC_SE2_SQUARED: {
      metric_se2_squared m;
      internal::nearest_search_topological<flat_t, view_t, metric_se2_squared, query_t, Visitor>(flat, view, m, q, v)();
    } break;
    default: internal::nearest_search(flat, view, metric_l2_squared(), q, v); break;
  }
}

inline bool topological_without_bounds(const ptk_tree* t, const flat_t& flat) {
  const int m = t->metric.load();
  return (m == PTK_METRIC_SO2 || m == PTK_METRIC_SE2_SQUARED) && !flat.keep_outer_bounds;
}

// The results contract of search_knn_within (ptk.h) as it is written: the reference's search_knn row of min(k, n_points)
// entries, the entries not below the radius dropped, the row padded with {-1, radius}.  `radius_of(i)`: the radius of
// row i -- one value for the scalar entry, the caller's array for the _radii entry.
template <class RadiusOf>
int knn_within_rows(const ptk_tree* t, const float* points, const float* q, uint64_t nq, uint32_t k, ptk_neighbor* out,
                    RadiusOf&& radius_of) {
  try {
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    auto* rows = reinterpret_cast<neighbor_t*>(out);
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, t->n_points);
    rows_loop(nq, [&](uint64_t i) {
      const float radius = radius_of(i);
      neighbor_t* b = rows + i * k;
      std::vector<neighbor_t> full(kk);
      internal::knn_visitor<neighbor_t*> v(full.data(), full.data() + kk);
      search_one(t, flat, view, q + i * t->dim, v);
      // (only what the search wrote: a row no distance is below FLT_MAX from -- NaN, +-Inf -- accepts nothing)
      const uint32_t found = (uint32_t)(v.filled() - full.data());
      uint32_t n = 0;
      while (n < found && full[n].distance < radius) {
        b[n] = full[n];
        ++n;
      }
      for (; n < k; ++n) b[n] = neighbor_t{-1, radius};
    });
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// count_within (ptk.h) as it is written: the reference's radius search of each row, counting instead of pushing.
template <class RadiusOf>
int count_within_rows(const ptk_tree* t, const float* points, const float* q, uint64_t nq, uint64_t max_count,
                      uint64_t* counts, RadiusOf&& radius_of) {
  try {
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    rows_loop(nq, [&](uint64_t i) {
      internal::count_visitor<float> v(radius_of(i), (std::size_t)max_count);
      search_one(t, flat, view, q + i * t->dim, v);
      counts[i] = v.count();
    });
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// search_radius (ptk.h) as it is written: the reference's radius search of each row, the rows laid end to end.
// `radius_of(i)`: the radius of row i, as knn_within_rows takes it.
template <class RadiusOf>
int radius_rows(const ptk_tree* t, const float* points, const float* q, uint64_t nq, float e, int sort, uint64_t* offsets,
                ptk_neighbor** out, RadiusOf&& radius_of) {
  *out = nullptr;
  try {
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    std::vector<std::vector<neighbor_t>> per_row(nq);
    rows_loop(nq, [&](uint64_t i) {
      if (e == 1.0f) {
        internal::radius_visitor<neighbor_t> v(radius_of(i), per_row[i]);
        search_one(t, flat, view, q + i * t->dim, v);
        if (sort) v.sort();
      } else {
        internal::radius_visitor<neighbor_t, true> v(radius_of(i), per_row[i], e);
        search_one(t, flat, view, q + i * t->dim, v);
        if (sort) v.sort();
      }
    });
    offsets[0] = 0;
    for (uint64_t i = 0; i < nq; ++i) offsets[i + 1] = offsets[i] + per_row[i].size();
    auto* rows = static_cast<neighbor_t*>(std::malloc(std::max<size_t>(offsets[nq], 1) * sizeof(neighbor_t)));
    if (rows == nullptr) return fail(PTK_ERR_NOMEM, "out of host memory");
    for (uint64_t i = 0; i < nq; ++i) std::copy(per_row[i].begin(), per_row[i].end(), rows + offsets[i]);
    *out = reinterpret_cast<ptk_neighbor*>(rows);
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// Row i of the self radius searches: the radius search of point i, the own entry removed.
inline void radius_self_row(const ptk_tree* t, const flat_t& flat, const view_t& view, const float* points, uint64_t i,
                            float radius, int sort, std::vector<neighbor_t>& row) {
  internal::radius_visitor<neighbor_t> v(radius, row);
  search_one(t, flat, view, points + i * t->dim, v);
  if (sort) v.sort();
  for (size_t j = 0; j < row.size(); ++j) {
    if (row[j].index == (int)i) {
      row.erase(row.begin() + (std::ptrdiff_t)j);
      break;
    }
  }
}

// search_radius_self (ptk.h) as the contract reads: the reference's radius search of each of the tree's own points, then
// the removal of the entry whose index is the row's (an index occurs at most once in a row).  per_row[i]: row i.
template <class RadiusOf>
void radius_self_rows(const ptk_tree* t, const flat_t& flat, const view_t& view, const float* points, int sort,
                      std::vector<std::vector<neighbor_t>>& per_row, RadiusOf&& radius_of) {
  rows_loop(t->n_points, [&](uint64_t i) { radius_self_row(t, flat, view, points, i, radius_of(i), sort, per_row[i]); });
}

// The argument checks of the two self loops: `radii` null -> the scalar radius; else n_points entries, scanned by row.
inline int check_host_self(const ptk_tree* t, const float* points, float radius, const float* radii) {
  if (t == nullptr || points == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (radii == nullptr) return radius >= 0.0f ? PTK_OK : fail(PTK_ERR_INVALID, "radius must be >= 0 (and not NaN)");
  return check_radii(radii, t->n_points, /*host_values=*/true);
}

}  // namespace ptk_host

extern "C" {

int ptk_host_search_knn(const ptk_tree* t, const float* points, const float* q, uint64_t nq, uint32_t k, float e,
                        ptk_neighbor* out) {
  if (t == nullptr || points == nullptr || (nq > 0 && (q == nullptr || out == nullptr)))
    return fail(PTK_ERR_INVALID, "null argument");
  if (k == 0 || !(e > 0.0f)) return fail(PTK_ERR_INVALID, "k must be >= 1 and e > 0");
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    auto* rows = reinterpret_cast<neighbor_t*>(out);
    // A slot the search did not write (k > n_points; a row no distance is below FLT_MAX from) holds {0, FLT_MAX}, as
    // the device rows (ptk.h): the visitor itself writes the distance of slot k - 1 only, as the reference's.
    auto fill = [](neighbor_t* from, neighbor_t* end) {
      for (; from < end; ++from) *from = neighbor_t{0, std::numeric_limits<float>::max()};
    };
    rows_loop(nq, [&](uint64_t i) {
      neighbor_t* b = rows + i * k;
      if (e == 1.0f) {
        internal::knn_visitor<neighbor_t*> v(b, b + k);
        search_one(t, flat, view, q + i * t->dim, v);
        fill(v.filled(), b + k);
      } else {
        internal::knn_visitor<neighbor_t*, true> v(b, b + k, e);
        search_one(t, flat, view, q + i * t->dim, v);
        fill(v.filled(), b + k);
      }
    });
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// search_knn_self (ptk.h) as it is written: the reference's search_knn row of m = min(k + 1, n_points) entries for each
// tree point, the entry the rule names removed (the first whose index is the row's, else the last), the row padded
// with {-1, FLT_MAX} to `width` records (k, or fewer where the caller reads no more: a row holds at most n_points - 1
// entries).  `dest(i)`: where row i is written; `done(i, row)` is called once it stands there.
extern "C++" {
namespace ptk_host {
template <class Dest, class Done>
int knn_self_rows(const ptk_tree* t, const float* points, uint32_t k, uint32_t width, Dest&& dest, Done&& done) {
  try {
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    const uint32_t m = (uint32_t)std::min<uint64_t>((uint64_t)k + 1, t->n_points);
    const float fmax = std::numeric_limits<float>::max();
    rows_loop(t->n_points, [&](uint64_t i) {
      std::vector<neighbor_t> full(m);
      internal::knn_visitor<neighbor_t*> v(full.data(), full.data() + m);
      search_one(t, flat, view, points + i * t->dim, v);
      const uint32_t found = (uint32_t)(v.filled() - full.data());  // (only what the search wrote)
      uint32_t drop = m - 1;
      for (uint32_t j = 0; j < found; ++j)
        if (full[j].index == (int)i) {
          drop = j;
          break;
        }
      neighbor_t* b = dest(i);
      uint32_t n = 0;
      for (uint32_t j = 0; j < found; ++j)
        if (j != drop && full[j].distance < fmax) b[n++] = full[j];
      for (; n < width; ++n) b[n] = neighbor_t{-1, fmax};
      done(i, b);
    });
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}
}  // namespace ptk_host
}  // extern "C++"

int ptk_host_search_knn_self(const ptk_tree* t, const float* points, uint32_t k, ptk_neighbor* out) {
  if (t == nullptr || points == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (k == 0) return fail(PTK_ERR_INVALID, "k must be >= 1");
  if (out == nullptr && t->n_points > 0) return fail(PTK_ERR_INVALID, "null output buffer");
  auto* rows = reinterpret_cast<ptk_host::neighbor_t*>(out);
  return ptk_host::knn_self_rows(t, points, k, k, [&](uint64_t i) { return rows + i * k; },
                                 [](uint64_t, const ptk_host::neighbor_t*) {});
}

// spacing_knn_self (ptk.h) as the contract reads: each row of the loop above reduced by the rule of
// pico_tree/internal/spacing.hpp, then the record and the mask from the means.
int ptk_host_spacing_knn_self(const ptk_tree* t, const float* points, uint32_t k, uint32_t flags, float ratio, float* mean,
                              float* kth, uint8_t* keep, ptk_spacing_stats* stats) {
  if (t == nullptr || points == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (k == 0) return fail(PTK_ERR_INVALID, "k must be >= 1");
  if (k == 0xFFFFFFFFu) return fail(PTK_ERR_INVALID, "k + 1 does not fit 32 bits");
  if (mean == nullptr && t->n_points > 0) return fail(PTK_ERR_INVALID, "null output buffer");
  int rc = check_spacing_values(flags, ratio, keep != nullptr || stats != nullptr);
  if (rc != PTK_OK) return rc;
  using namespace ptk_host;
  const bool root = (flags & PTK_SPACING_SQRT) != 0u;
  // (a row holds at most n_points - 1 entries, whatever k is: the buffer and the fold are as wide as that, and the buffer
  // lives as long as the row)
  const uint32_t width = (uint32_t)std::min<uint64_t>(k, t->n_points);
  rc = ptk_host::knn_self_rows(
      t, points, k, width,
      [&](uint64_t) {
        thread_local std::vector<ptk_host::neighbor_t> row;
        row.resize(width);
        return row.data();
      },
      [&](uint64_t i, const ptk_host::neighbor_t* row) {
        float m, kd;
        internal::spacing_row<float>([&](uint32_t j) { return row[j].distance; }, width, root, &m, &kd);
        mean[i] = m;
        if (kth != nullptr) kth[i] = kd;
      });
  if (rc != PTK_OK) return rc;
  static_assert(sizeof(ptk_spacing_stats) == sizeof(internal::spacing_stats), "record layout");
  if (keep != nullptr || stats != nullptr)
    internal::spacing_statistics(mean, t->n_points, ratio, reinterpret_cast<internal::spacing_stats*>(stats), keep);
  return PTK_OK;
}

int ptk_host_search_knn_within(const ptk_tree* t, const float* points, const float* q, uint64_t nq, uint32_t k,
                               float radius, ptk_neighbor* out) {
  if (t == nullptr || points == nullptr || (nq > 0 && (q == nullptr || out == nullptr)))
    return fail(PTK_ERR_INVALID, "null argument");
  if (k == 0) return fail(PTK_ERR_INVALID, "k must be >= 1");
  if (!(radius >= 0.0f)) return fail(PTK_ERR_INVALID, "radius must be >= 0 (and not NaN)");
  return ptk_host::knn_within_rows(t, points, q, nq, k, out, [radius](uint64_t) { return radius; });
}

// ... with the row's own radius (ptk.h: row i is the scalar call's row i at radius = radii[i]).
int ptk_host_search_knn_within_radii(const ptk_tree* t, const float* points, const float* q, uint64_t nq, uint32_t k,
                                     const float* radii, ptk_neighbor* out) {
  if (t == nullptr || points == nullptr || (nq > 0 && (q == nullptr || out == nullptr)))
    return fail(PTK_ERR_INVALID, "null argument");
  if (k == 0) return fail(PTK_ERR_INVALID, "k must be >= 1");
  if (nq == 0) return PTK_OK;
  const int rc = check_radii(radii, nq, /*host_values=*/true);
  if (rc != PTK_OK) return rc;
  return ptk_host::knn_within_rows(t, points, q, nq, k, out, [radii](uint64_t i) { return radii[i]; });
}

int ptk_host_search_count_within(const ptk_tree* t, const float* points, const float* q, uint64_t nq, float radius,
                                 uint64_t max_count, uint64_t* counts) {
  if (t == nullptr || points == nullptr || (nq > 0 && (q == nullptr || counts == nullptr)))
    return fail(PTK_ERR_INVALID, "null argument");
  if (!(radius >= 0.0f)) return fail(PTK_ERR_INVALID, "radius must be >= 0 (and not NaN)");
  return ptk_host::count_within_rows(t, points, q, nq, max_count, counts, [radius](uint64_t) { return radius; });
}

int ptk_host_search_count_within_radii(const ptk_tree* t, const float* points, const float* q, uint64_t nq,
                                       const float* radii, uint64_t max_count, uint64_t* counts) {
  if (t == nullptr || points == nullptr || (nq > 0 && (q == nullptr || counts == nullptr)))
    return fail(PTK_ERR_INVALID, "null argument");
  if (nq == 0) return PTK_OK;
  const int rc = check_radii(radii, nq, /*host_values=*/true);
  if (rc != PTK_OK) return rc;
  return ptk_host::count_within_rows(t, points, q, nq, max_count, counts, [radii](uint64_t i) { return radii[i]; });
}

int ptk_host_search_radius(const ptk_tree* t, const float* points, const float* q, uint64_t nq, float radius, float e,
                           int sort, uint64_t* offsets, ptk_neighbor** out) {
  if (t == nullptr || points == nullptr || offsets == nullptr || out == nullptr || (nq > 0 && q == nullptr))
    return fail(PTK_ERR_INVALID, "null argument");
  if (!(e > 0.0f)) return fail(PTK_ERR_INVALID, "approximation ratio e must be > 0");
  return ptk_host::radius_rows(t, points, q, nq, e, sort, offsets, out, [radius](uint64_t) { return radius; });
}

// ... with the row's own radius (ptk.h: row i is the scalar call's row i at radius = radii[i], e = 1).
int ptk_host_search_radius_radii(const ptk_tree* t, const float* points, const float* q, uint64_t nq, const float* radii,
                                 int sort, uint64_t* offsets, ptk_neighbor** out) {
  if (t == nullptr || points == nullptr || offsets == nullptr || out == nullptr || (nq > 0 && q == nullptr))
    return fail(PTK_ERR_INVALID, "null argument");
  *out = nullptr;
  if (nq > 0) {
    const int rc = check_radii(radii, nq, /*host_values=*/true);
    if (rc != PTK_OK) return rc;
  }
  return ptk_host::radius_rows(t, points, q, nq, 1.0f, sort, offsets, out, [radii](uint64_t i) { return radii[i]; });
}

int ptk_host_search_count_within_self(const ptk_tree* t, const float* points, float radius, const float* radii,
                                      uint64_t max_count, uint64_t* counts) {
  const int rc = ptk_host::check_host_self(t, points, radius, radii);
  if (rc != PTK_OK) return rc;
  if (counts == nullptr && t->n_points > 0) return fail(PTK_ERR_INVALID, "null counts buffer");
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    std::vector<std::vector<neighbor_t>> per_row(t->n_points);
    radius_self_rows(t, flat, view, points, 0, per_row, [&](uint64_t i) { return radii != nullptr ? radii[i] : radius; });
    // (the clamp after the own entry has left)
    for (uint64_t i = 0; i < t->n_points; ++i)
      counts[i] = max_count != 0 ? std::min<uint64_t>(per_row[i].size(), max_count) : per_row[i].size();
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

int ptk_host_search_radius_self(const ptk_tree* t, const float* points, float radius, const float* radii, int sort,
                                uint64_t* offsets, ptk_neighbor** out) {
  if (offsets == nullptr || out == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  *out = nullptr;
  const int rc = ptk_host::check_host_self(t, points, radius, radii);
  if (rc != PTK_OK) return rc;
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    const uint64_t np = t->n_points;
    std::vector<std::vector<neighbor_t>> per_row(np);
    radius_self_rows(t, flat, view, points, sort, per_row, [&](uint64_t i) { return radii != nullptr ? radii[i] : radius; });
    offsets[0] = 0;
    for (uint64_t i = 0; i < np; ++i) offsets[i + 1] = offsets[i] + per_row[i].size();
    auto* rows = static_cast<neighbor_t*>(std::malloc(std::max<size_t>(offsets[np], 1) * sizeof(neighbor_t)));
    if (rows == nullptr) return fail(PTK_ERR_NOMEM, "out of host memory");
    for (uint64_t i = 0; i < np; ++i) std::copy(per_row[i].begin(), per_row[i].end(), rows + offsets[i]);
    *out = reinterpret_cast<ptk_neighbor*>(rows);
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// cluster_within_self (ptk.h) as the contract reads: the rows of the self loop above, a sequential union-find over
// them, then the border rule (pico_tree/internal/cluster.hpp).
int ptk_host_cluster_within_self(const ptk_tree* t, const float* points, float radius, const float* radii,
                                 uint64_t min_neighbors, int32_t* labels, uint64_t* n_clusters) {
  if (n_clusters != nullptr) *n_clusters = 0;
  const int rc = ptk_host::check_host_self(t, points, radius, radii);
  if (rc != PTK_OK) return rc;
  if (labels == nullptr && t->n_points > 0) return fail(PTK_ERR_INVALID, "null labels buffer");
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    std::vector<std::vector<neighbor_t>> per_row(t->n_points);
    radius_self_rows(t, flat, view, points, 0, per_row, [&](uint64_t i) { return radii != nullptr ? radii[i] : radius; });
    internal::cluster_rows(per_row, min_neighbors, labels);
    if (n_clusters != nullptr) *n_clusters = count_cluster_roots(labels, t->n_points);
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// normals_within_self (ptk.h) as the contract reads: the row of the self loop above for each point, unsorted, then the
// moments and the frame of pico_tree/internal/local_frame.hpp.  Every float32 handle with dim == 3 and a
// non-topological metric, the deep stack class included.
int ptk_host_normals_within_self(const ptk_tree* t, const float* points, float radius, const float* radii,
                                 uint64_t min_neighbors, const float* viewpoint, ptk_frame* frames, ptk_moments* moments) {
  if (t == nullptr || points == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (t->dim != 3) return fail(PTK_ERR_INVALID, "normals_within_self: a normal is defined for 3-D points, not dim %u", t->dim);
  if (topological(t)) return fail(PTK_ERR_INVALID, "normals_within_self: a normal is not defined under a topological metric");
  const int rc = ptk_host::check_host_self(t, points, radius, radii);
  if (rc != PTK_OK) return rc;
  if (frames == nullptr && moments == nullptr && t->n_points > 0) return fail(PTK_ERR_INVALID, "null output buffer");
  static_assert(sizeof(ptk_frame) == sizeof(pico_tree::internal::frame3), "record layout");
  static_assert(sizeof(ptk_moments) == sizeof(pico_tree::internal::moments3), "record layout");
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    const bool has_view = viewpoint != nullptr;
    const float vx = has_view ? viewpoint[0] : 0.0f, vy = has_view ? viewpoint[1] : 0.0f, vz = has_view ? viewpoint[2] : 0.0f;
    rows_loop(t->n_points, [&](uint64_t i) {
      std::vector<neighbor_t> row;
      radius_self_row(t, flat, view, points, i, radii != nullptr ? radii[i] : radius, 0, row);
      const internal::moment_sums sums = internal::sums_of_row(points, i, row);
      if (frames != nullptr) {
        const internal::frame3 f = internal::frame_of(sums, min_neighbors, has_view, vx, vy, vz, points[3 * i],
                                                      points[3 * i + 1], points[3 * i + 2]);
        std::memcpy(frames + i, &f, sizeof f);
      }
      if (moments != nullptr) {
        const internal::moments3 m = sums.record();
        std::memcpy(moments + i, &m, sizeof m);
      }
    });
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// aggregate_within_self (ptk.h) as the contract reads: the row of the self loop above for each point, unsorted, folded with
// the formulas of pico_tree/internal/aggregate.hpp.  Every float32 handle, the deep stack class and the topological
// metrics included.
int ptk_host_aggregate_within_self(const ptk_tree* t, const float* points, float radius, const float* radii,
                                   const float* values, uint32_t channels, uint32_t op, float* out, uint64_t* counts) {
  if (t == nullptr || points == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  int rc = check_aggregate_args(values, channels, op, /*self_form=*/true, out, t->n_points);
  if (rc == PTK_OK) rc = ptk_host::check_host_self(t, points, radius, radii);
  if (rc != PTK_OK) return rc;
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    const auto kind = static_cast<pico_tree::aggregate_op>(op & ~(uint32_t)PTK_AGG_INCLUDE_SELF);
    const bool include_self = (op & PTK_AGG_INCLUDE_SELF) != 0;
    rows_loop(t->n_points, [&](uint64_t i) {
      std::vector<neighbor_t> row;
      radius_self_row(t, flat, view, points, i, radii != nullptr ? radii[i] : radius, 0, row);
      internal::aggregate_row(values, channels, kind, include_self ? values + i * channels : nullptr, row, out + i * channels);
      if (counts != nullptr) counts[i] = row.size();
    });
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// aggregate_within (ptk.h): the same over the rows of ptk_host_search_radius_radii (e = 1, unsorted); `radii` null: every
// row gets `radius`.
int ptk_host_aggregate_within(const ptk_tree* t, const float* points, const float* q, uint64_t nq, float radius,
                              const float* radii, const float* values, uint32_t channels, uint32_t op, float* out,
                              uint64_t* counts) {
  if (t == nullptr || points == nullptr || (nq > 0 && q == nullptr)) return fail(PTK_ERR_INVALID, "null argument");
  int rc = check_aggregate_args(values, channels, op, /*self_form=*/false, out, nq);
  if (rc != PTK_OK || nq == 0) return rc;
  rc = radii != nullptr ? check_radii(radii, nq, /*host_values=*/true) : check_radius(radius);
  if (rc != PTK_OK) return rc;
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    const auto kind = static_cast<pico_tree::aggregate_op>(op);
    rows_loop(nq, [&](uint64_t i) {
      std::vector<neighbor_t> row;
      internal::radius_visitor<neighbor_t> v(radii != nullptr ? radii[i] : radius, row);
      search_one(t, flat, view, q + i * t->dim, v);
      internal::aggregate_row(values, channels, kind, nullptr, row, out + i * channels);
      if (counts != nullptr) counts[i] = row.size();
    });
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// align_step (ptk.h) as the contract reads: the pose on the host, the rows of ptk_host_search_knn above with k = 1 and
// e = 1, then the terms and the summation tree of pico_tree/internal/align.hpp, a block of 256 rows at a time.
int ptk_host_align_step(const ptk_tree* t, const float* points, const float* q, uint64_t nq, const float* transform,
                        float max_distance, const float* normals, ptk_align_sums* out, ptk_neighbor* rows) {
  int rc = check_align_step(t, q, nq, max_distance, out);
  if (rc != PTK_OK) return rc;
  if (points == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  try {
    using namespace ptk_host;
    std::vector<float> posed;
    const float* qp = q;
    if (transform != nullptr && nq > 0) {
      posed.resize((size_t)nq * 3);
      rows_loop(nq, [&](uint64_t i) { internal::align_pose(transform, q[3 * i], q[3 * i + 1], q[3 * i + 2], &posed[3 * i]); });
      qp = posed.data();
    }
    std::vector<ptk_neighbor> own;
    if (rows == nullptr && nq > 0) {
      own.resize((size_t)nq);
      rows = own.data();
    }
    rc = ptk_host_search_knn(t, points, qp, nq, 1, 1.0f, rows);
    if (rc != PTK_OK) return rc;
    const ptk_neighbor* found = rows;
    internal::align_reduce_rows(
        qp, nq, [&](uint64_t i, int32_t& index, float& distance) { index = found[i].index, distance = found[i].distance; },
        [&](int32_t index) { return points + 3 * (size_t)index; }, normals, max_distance,
        [](uint64_t n, auto&& f) { rows_loop(n, f); },
        reinterpret_cast<internal::align_sums*>(out));
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// suppress_within_self (ptk.h) as the contract reads: the rows of the self loop above, a sort by key, one greedy pass
// in descending key (pico_tree/internal/suppress.hpp).
int ptk_host_suppress_within_self(const ptk_tree* t, const float* points, float radius, const float* radii,
                                  const float* scores, uint8_t* keep, uint64_t* n_kept) {
  if (n_kept != nullptr) *n_kept = 0;
  int rc = ptk_host::check_host_self(t, points, radius, radii);
  if (rc == PTK_OK) rc = check_scores(scores, t->n_points);
  if (rc != PTK_OK) return rc;
  if (keep == nullptr && t->n_points > 0) return fail(PTK_ERR_INVALID, "null keep buffer");
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    std::vector<std::vector<neighbor_t>> per_row(t->n_points);
    radius_self_rows(t, flat, view, points, 0, per_row, [&](uint64_t i) { return radii != nullptr ? radii[i] : radius; });
    const uint64_t kept = internal::suppress_rows(per_row, scores, keep);
    if (n_kept != nullptr) *n_kept = kept;
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

// mst_within_self (ptk.h) as the contract reads: the rows of the self loop above, the edges sorted by (bits(w), lo, hi),
// Kruskal with a union-find (pico_tree/internal/mst.hpp).  Every float32 handle under metric_l2_squared and metric_l1.
int ptk_host_mst_within_self(const ptk_tree* t, const float* points, float radius, const float* core, ptk_mst_edge* edges,
                             uint64_t* n_edges, int32_t* labels) {
  if (n_edges != nullptr) *n_edges = 0;
  int rc = ptk_host::check_host_self(t, points, radius, nullptr);
  if (rc == PTK_OK) rc = check_core(core, t->n_points);
  if (rc != PTK_OK) return rc;
  if (!mst_metric(t))
    return fail(PTK_ERR_UNSUPPORTED, "mst_within_self: the host loop serves metric_l2_squared and metric_l1 only");
  if (edges == nullptr && t->n_points > 1) return fail(PTK_ERR_INVALID, "null edge buffer");
  static_assert(sizeof(ptk_mst_edge) == sizeof(pico_tree::internal::mst_edge), "record layout");
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    std::vector<std::vector<neighbor_t>> per_row(t->n_points);
    radius_self_rows(t, flat, view, points, 0, per_row, [&](uint64_t) { return radius; });
    const uint64_t count =
        internal::mst_rows(per_row, radius, core, reinterpret_cast<pico_tree::internal::mst_edge*>(edges), labels);
    if (n_edges != nullptr) *n_edges = count;
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

int ptk_host_search_box(const ptk_tree* t, const float* points, const float* mins, const float* maxs, uint64_t nb,
                        uint64_t* offsets, int32_t** out) {
  if (t == nullptr || points == nullptr || offsets == nullptr || out == nullptr || (nb > 0 && (mins == nullptr || maxs == nullptr)))
    return fail(PTK_ERR_INVALID, "null argument");
  *out = nullptr;
  try {
    using namespace ptk_host;
    const std::shared_ptr<const flat_t> flat_holder = flat_of(t);
    const flat_t& flat = *flat_holder;
    space_t space(points, t->n_points, t->dim);
    view_t view(space);
    std::vector<std::vector<int>> per_row(nb);
    const int metric = t->metric.load();
    if (metric == PTK_METRIC_SO2 || metric == PTK_METRIC_SE2_SQUARED) {
      // a tree over a topological space: the metric_box_map query of the reference (box.hpp:300-376) -- intervals
      // through the seam of the circle axis, the four-bound intersection tests
      if (topological_without_bounds(t, flat)) return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds)");
      const metric_so2 so2;
      const metric_se2_squared se2;
      rows_loop(nb, [&](uint64_t i) {
        if (metric == PTK_METRIC_SO2)
          internal::box_search<true>(flat, view, mins + i * t->dim, maxs + i * t->dim, per_row[i],
                                     internal::circle_axes_of<metric_so2>{so2});
        else
          internal::box_search<true>(flat, view, mins + i * t->dim, maxs + i * t->dim, per_row[i],
                                     internal::circle_axes_of<metric_se2_squared>{se2});
      });
    } else {
      rows_loop(nb, [&](uint64_t i) { internal::box_search(flat, view, mins + i * t->dim, maxs + i * t->dim, per_row[i]); });
    }
    offsets[0] = 0;
    for (uint64_t i = 0; i < nb; ++i) offsets[i + 1] = offsets[i] + per_row[i].size();
    auto* rows = static_cast<int32_t*>(std::malloc(std::max<size_t>(offsets[nb], 1) * sizeof(int32_t)));
    if (rows == nullptr) return fail(PTK_ERR_NOMEM, "out of host memory");
    for (uint64_t i = 0; i < nb; ++i) std::copy(per_row[i].begin(), per_row[i].end(), rows + offsets[i]);
    *out = rows;
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_INVALID, "host search failed: %s", ex.what());
  }
  return PTK_OK;
}

}  // extern "C"
