#pragma once
//! \file kd_tree.hpp
//! \brief pico_tree::kd_tree -- the public search structure.
//! \details Source-compatible with the reference class
//! (/root/reference/src/pico_tree/pico_tree/kd_tree.hpp:19-435): same template
//! parameters, constructor, per-query members, tags, CTAD guide and
//! make_kd_tree.  Two things differ underneath:
//!
//!  1. The tree is a flat depth-first array (internal/flat_tree.hpp) instead of
//!     pointer-linked nodes.
//!  2. A family of BATCHED members takes a whole query space at once -- the
//!     shape of the reference's only batched caller, the OpenMP loops of its
//!     Python binding (src/pyco_tree/pico_tree/_pyco_tree/kd_tree.hpp:117-268).
//!     For kd_tree<Space, metric_l2_squared | metric_l1 | metric_lpinf, int> over
//!     float they run on the MI355X through the C ABI of include/ptk.h (-lptk).  They have
//!     no host fallback: without a usable backend they throw.
//!
//! The per-query members (search_nn(x, nn), search_knn(x, k, knn), custom
//! visitors, other metrics, double) run on the host, as in the reference.

#include <algorithm>
#include <cmath>
#include <fstream>
#include <iostream>
#include <iterator>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "core.hpp"
#include "internal/access.hpp"
#include "internal/backend.hpp"
#include "internal/aggregate.hpp"
#include "internal/align.hpp"
#include "internal/cluster.hpp"
#include "internal/flat_search.hpp"
#include "internal/flat_tree.hpp"
#include "internal/local_frame.hpp"
#include "internal/mst.hpp"
#include "internal/stream.hpp"
#include "internal/spacing.hpp"
#include "internal/suppress.hpp"
#include "internal/visitors.hpp"
#include "metric.hpp"

namespace pico_tree {

//! Off by default: a batched search the device refuses for a valid tree (PTK_ERR_UNSUPPORTED) throws.  With
//! allow_host_loop(true) such a call is served by the loop of per-query host members the reference runs for every call
//! (_pyco_tree/kd_tree.hpp:128), after one message on stderr.  Process-wide.
inline void allow_host_loop(bool on) { internal::host_loop_flag().store(on); }

template <typename Space_, typename Metric_ = metric_l2_squared, typename Index_ = int>
class kd_tree {
  static_assert(
      std::is_same_v<std::remove_cv_t<Space_>, Space_>,
      "SPACE_TYPE_MUST_BE_NON-CONST_NON-VOLATILE");
  //! Topological metrics (metric_so2, metric_se2_squared): the tree keeps four bounds per branch
  //! (the reference's kd_tree_node_topological) and the per-query members run
  //! internal::nearest_search_topological on the host.
  static constexpr bool topological =
      !std::is_same_v<typename Metric_::space_category, euclidean_space_tag>;

  using plain_space_type = internal::unwrap_ref_t<Space_>;
  using space_view_type = internal::space_view<plain_space_type>;

 public:
  using size_type = size_t;
  using index_type = Index_;
  using scalar_type = typename space_view_type::scalar_type;
  static constexpr size_type dim = space_view_type::dim;
  using space_type = Space_;
  using metric_type = Metric_;
  using neighbor_type = neighbor<index_type, scalar_type>;

 private:
  using tree_type = internal::flat_tree<index_type, scalar_type, dim>;
  static constexpr bool accelerated =
      internal::is_accelerated_v<Metric_, scalar_type, Index_>;
  using api = internal::ptk_api<std::conditional_t<accelerated, scalar_type, float>>;

 public:
  //! Index positions of one leaf: a [begin, end) range into the tree's indices.
  class leaf_range_type {
   public:
    using iterator_type = typename std::vector<index_type>::const_iterator;
    leaf_range_type(iterator_type b, iterator_type e) : b_(b), e_(e) {}
    iterator_type begin() const { return b_; }
    iterator_type end() const { return e_; }

   private:
    iterator_type b_;
    iterator_type e_;
  };

  //! Builds the tree.  \p space is taken by value: move it in, or use
  //! std::reference_wrapper<Space> as the space type to borrow it.
  template <
      typename Stop_,
      typename Bounds_ = bounds_from_space_t,
      typename Rule_ = sliding_midpoint_max_side_t>
  kd_tree(
      space_type space,
      splitter_stop_condition_t<Stop_> const& stop_condition,
      splitter_start_bounds_t<Bounds_> const& start_bounds = Bounds_{},
      splitter_rule_t<Rule_> const& rule = Rule_{})
      : space_(std::move(space)),
        metric_(),
        tree_(internal::build_flat_tree<index_type>(
            view(), stop_condition, start_bounds, rule, topological)) {}

  kd_tree(kd_tree const&) = delete;
  kd_tree(kd_tree&&) = default;
  kd_tree& operator=(kd_tree const&) = delete;
  kd_tree& operator=(kd_tree&&) = default;

  // ---- per-query searches (host) -------------------------------------------

  //! Generic traversal: \p visitor sees every measured point as
  //! visitor(index, distance) and prunes with visitor.max().
  template <typename P_, typename V_>
  inline void search_nearest(P_ const& x, V_& visitor) const {
    using query_view = internal::point_view<P_>;
    static_assert(
        std::is_same_v<scalar_type, typename query_view::scalar_type>,
        "POINT_AND_TREE_SCALAR_TYPES_DIFFER");
    static_assert(
        dim == query_view::dim || dim == dynamic_extent ||
            query_view::dim == dynamic_extent,
        "POINT_AND_TREE_DIMS_DIFFER");
    query_view q(x);
    space_view_type s = view();
    if constexpr (topological) {
      internal::nearest_search_topological<tree_type, space_view_type, metric_type, query_view, V_>(
          tree_, s, metric_, q, visitor)();
    } else {
      internal::nearest_search(tree_, s, metric_, q, visitor);
    }
  }

  template <typename P_>
  inline void search_nn(P_ const& x, neighbor_type& nn) const {
    internal::nn_visitor<neighbor_type> v(nn);
    search_nearest(x, v);
  }

  //! Approximate nn: may return a neighbour up to a factor \p e (in metric
  //! units) farther than the true one; the reported distance is scaled by 1/e.
  template <typename P_>
  inline void search_nn(P_ const& x, scalar_type const e, neighbor_type& nn) const {
    internal::nn_visitor<neighbor_type, true> v(nn, e);
    search_nearest(x, v);
  }

  template <typename P_, typename RandomAccessIterator_>
  inline void search_knn(
      P_ const& x, RandomAccessIterator_ begin, RandomAccessIterator_ end) const {
    static_assert(
        std::is_same_v<
            typename std::iterator_traits<RandomAccessIterator_>::value_type,
            neighbor_type>,
        "ITERATOR_VALUE_TYPE_DOES_NOT_EQUAL_NEIGHBOR_TYPE");
    internal::knn_visitor<RandomAccessIterator_> v(begin, end);
    search_nearest(x, v);
  }

  //! \p knn is resized to min(k, number of points).
  template <typename P_>
  inline void search_knn(
      P_ const& x, size_type const k, std::vector<neighbor_type>& knn) const {
    knn.resize(std::min(k, view().size()));
    search_knn(x, knn.begin(), knn.end());
  }

  //! The k nearest points closer than \p radius (metric units: squared for the
  //! default metric): the search_knn row of min(k, number of points) entries
  //! cut at the first distance >= radius; \p knn is resized to the hits.  The
  //! k-list starts at radius * (1 + 2^-10) instead of the largest scalar, so the
  //! search prunes with min(k-th, that bound); metric_lpinf /
  //! metric_lninf and the topological metrics, whose box distance is no lower
  //! bound of the point distances, search unseeded.
  template <typename P_>
  inline void search_knn_within(
      P_ const& x,
      size_type const k,
      scalar_type const radius,
      std::vector<neighbor_type>& knn) const {
    knn.resize(std::min(k, view().size()));
    if (knn.empty()) return;
    internal::knn_visitor<typename std::vector<neighbor_type>::iterator> v(knn.begin(), knn.end());
    constexpr bool seeded = std::is_same_v<Metric_, metric_l2_squared> || std::is_same_v<Metric_, metric_l1>;
    scalar_type const seed = radius * (scalar_type(1) + scalar_type(1) / scalar_type(1024));
    if (seeded && (radius == scalar_type(0) || std::isnormal(radius)) && std::isfinite(seed)) {
      std::fill(knn.begin(), knn.end(), neighbor_type(index_type(-1), seed));
    }
    search_nearest(x, v);
    // (only the entries the search wrote: a query no distance is below the largest scalar from -- NaN, +-Inf --
    // accepts nothing, and the slots of an unseeded list are then as resize() left them)
    size_type const found = static_cast<size_type>(v.filled() - knn.begin());
    size_type n = 0;
    while (n < found && knn[n].index != index_type(-1) && knn[n].distance < radius) ++n;
    knn.resize(n);
  }

  //! The k nearest OTHER points of the tree's own point \p index (DESIGN.md
  //! §2): the search_knn row of m = min(k + 1, number of points) entries for
  //! that point with one entry removed -- the first whose index is \p index,
  //! else (k + 1 or more other points coincide with it and are visited first)
  //! the last; \p knn is resized to what remains (at most k entries).
  inline void search_knn_self(
      index_type const index, size_type const k, std::vector<neighbor_type>& knn) const {
    auto const points = view();
    if (index < index_type(0) || static_cast<size_type>(index) >= points.size()) {
      throw std::out_of_range("pico_tree: search_knn_self: no such point");
    }
    knn.resize(std::min(k + 1, points.size()));
    internal::knn_visitor<typename std::vector<neighbor_type>::iterator> v(knn.begin(), knn.end());
    auto const x = make_row(points[index], points.sdim());
    search_nearest(x, v);
    // (only the entries the search wrote, as search_knn_within)
    size_type const found = static_cast<size_type>(v.filled() - knn.begin());
    size_type drop = knn.size() - 1;
    for (size_type j = 0; j < found; ++j) {
      if (knn[j].index == index) {
        drop = j;
        break;
      }
    }
    size_type n = 0;
    for (size_type j = 0; j < found; ++j) {
      if (j != drop && knn[j].distance < std::numeric_limits<scalar_type>::max()) knn[n++] = knn[j];
    }
    knn.resize(n);
  }

  template <typename P_, typename RandomAccessIterator_>
  inline void search_knn(
      P_ const& x,
      scalar_type const e,
      RandomAccessIterator_ begin,
      RandomAccessIterator_ end) const {
    static_assert(
        std::is_same_v<
            typename std::iterator_traits<RandomAccessIterator_>::value_type,
            neighbor_type>,
        "ITERATOR_VALUE_TYPE_DOES_NOT_EQUAL_NEIGHBOR_TYPE");
    internal::knn_visitor<RandomAccessIterator_, true> v(begin, end, e);
    search_nearest(x, v);
  }

  template <typename P_>
  inline void search_knn(
      P_ const& x,
      size_type const k,
      scalar_type const e,
      std::vector<neighbor_type>& knn) const {
    knn.resize(std::min(k, view().size()));
    search_knn(x, e, knn.begin(), knn.end());
  }

  //! The number of points with distance < \p radius (metric units: squared
  //! for the default metric): the length of search_radius(x, radius)'s row,
  //! counted by the radius visitor without the row.  Any metric.
  template <typename P_>
  inline size_type count_within(P_ const& x, scalar_type const radius) const {
    internal::count_visitor<scalar_type> v(radius);
    search_nearest(x, v);
    return static_cast<size_type>(v.count());
  }

  //! All points with distance < \p radius (metric units: squared for the
  //! default metric), in traversal order unless \p sort.
  template <typename P_>
  inline void search_radius(
      P_ const& x,
      scalar_type const radius,
      std::vector<neighbor_type>& n,
      bool const sort = false) const {
    internal::radius_visitor<neighbor_type> v(radius, n);
    search_nearest(x, v);
    if (sort) v.sort();
  }

  template <typename P_>
  inline void search_radius(
      P_ const& x,
      scalar_type const radius,
      scalar_type const e,
      std::vector<neighbor_type>& n,
      bool const sort = false) const {
    internal::radius_visitor<neighbor_type, true> v(radius, n, e);
    search_nearest(x, v);
    if (sort) v.sort();
  }

  //! The neighbours of the tree's own point \p index within \p radius among the
  //! OTHER points: the search_radius row of that point without
  //! the entry whose index is \p index, if there is one; the other entries keep
  //! their order (traversal order, ascending distance with \p sort).
  inline void search_radius_self(
      index_type const index,
      scalar_type const radius,
      std::vector<neighbor_type>& n,
      bool const sort = false) const {
    auto const points = view();
    if (index < index_type(0) || static_cast<size_type>(index) >= points.size()) {
      throw std::out_of_range("pico_tree: search_radius_self: no such point");
    }
    n.clear();
    auto const x = make_row(points[index], points.sdim());
    search_radius(x, radius, n, sort);
    for (size_type j = 0; j < n.size(); ++j) {
      if (n[j].index == index) {
        n.erase(n.begin() + static_cast<std::ptrdiff_t>(j));
        break;
      }
    }
  }

  //! All indices inside the closed box [min, max].
  template <typename P_>
  inline void search_box(
      P_ const& min, P_ const& max, std::vector<index_type>& idxs) const {
    idxs.clear();
    space_view_type s = view();
    if constexpr (topological) {  // metric_box_map: intervals through the seam of a circle axis, four-bound tests
      internal::box_search<true>(
          tree_,
          s,
          internal::point_view<P_>(min).data(),
          internal::point_view<P_>(max).data(),
          idxs,
          internal::circle_axes_of<metric_type>{metric_});
    } else {
      internal::box_search(
          tree_,
          s,
          internal::point_view<P_>(min).data(),
          internal::point_view<P_>(max).data(),
          idxs);
    }
  }

  // ---- batched searches (MI355X) -------------------------------------------
  // QuerySpace_ is anything with space_traits<>.  Row i of every output belongs
  // to query i.  Only available for the accelerated instantiation.

  //! out[i] = nearest neighbour of query i.  out must hold queries.size().
  template <typename QuerySpace_>
  inline void search_nn(QuerySpace_ const& queries, neighbor_type* out) const {
    search_knn(queries, size_type(1), out);
  }

  //! out[i * k + j] = j-th nearest neighbour of query i (ascending).  Unlike the
  //! vector overload k is NOT clamped: k <= number of points is required.
  template <typename QuerySpace_>
  inline void search_knn(
      QuerySpace_ const& queries, size_type const k, neighbor_type* out) const {
    batched_knn(queries, k, scalar_type(1.0), out);
  }

  template <typename QuerySpace_>
  inline void search_knn(
      QuerySpace_ const& queries,
      size_type const k,
      scalar_type const e,
      neighbor_type* out) const {
    batched_knn(queries, k, e, out);
  }

  //! out[i * k + j]: row i of search_knn_within -- the k nearest points closer
  //! than \p radius -- padded to k entries with {-1, radius}.  Any k >= 1.
  template <typename QuerySpace_>
  inline void search_knn_within(
      QuerySpace_ const& queries,
      size_type const k,
      scalar_type const radius,
      neighbor_type* out) const {
    batched_knn_within(queries, k, radius, out);
  }

  //! Each point's k nearest other points: \p out is resized to size() * k,
  //! out[i * k + j] is entry j of search_knn_self(i, k, ...), the row padded to
  //! k entries with {-1, largest scalar}.  There is no query space: the
  //! backend holds the points.  Served by the backend (ptk_search_knn_self);
  //! where it refuses (and allow_host_loop is on), and in a build with
  //! PICO_TREE_HOST_ONLY defined, by a loop over the per-point member.  Throws
  //! on failure; k == 0 is std::invalid_argument.
  inline void search_knn_self(size_type const k, std::vector<neighbor_type>& out) const {
    batched_knn_self(k, out);
  }

  //! k-NN spacing of the tree's points (ptk.h, "spacing_knn_self"): mean[i] is
  //! the mean of the distances of search_knn_self(i, k, ...) -- added in rank
  //! order from +0 in scalar_type, one division -- and kth[i] (\p kth may be
  //! null) the last of them; a point without a neighbour gets the largest
  //! scalar for both.  \p sqrt: the square root of every distance is taken
  //! first (lengths under metric_l2_squared / metric_se2_squared).  mean, kth:
  //! size() entries.  Served by the backend (ptk_spacing_knn_self); where it
  //! refuses (and allow_host_loop is on), and in a build with
  //! PICO_TREE_HOST_ONLY defined, by a loop over the per-point member and the
  //! rule of internal/spacing.hpp.  k == 0 is std::invalid_argument.
  inline void spacing_knn_self(size_type const k, bool const sqrt, scalar_type* mean, scalar_type* kth = nullptr) const {
    batched_spacing_knn_self(k, sqrt, 0.0f, mean, kth, nullptr, nullptr);
  }

  //! Statistical outlier removal (PCL's StatisticalOutlierRemoval): keep[i] = 1
  //! iff point i has a neighbour, a finite mean spacing x_i, and with
  //! e = x_i - mean: e <= 0 or e * e <= ratio^2 * variance -- mean and sample
  //! variance of the valid x_i in double over the summation tree of
  //! internal/align.hpp; \p stats (may be null) receives the record.  keep:
  //! size() entries.  \p std_ratio must be finite and >= 0
  //! (std::invalid_argument).  Served as spacing_knn_self.
  inline void outliers_knn_self(
      size_type const k, float const std_ratio, bool const sqrt, std::uint8_t* keep, spacing_stats* stats = nullptr) const {
    std::vector<scalar_type> mean(view().size());
    batched_spacing_knn_self(k, sqrt, std_ratio, mean.data(), nullptr, keep, stats);
  }

  //! Every point's neighbours within \p radius among the other points:
  //! rows[i] = search_radius_self(i, radius, ..., sort); rows is resized to
  //! size().  There is no query space: the backend holds the points.  Served
  //! by the backend (ptk_search_radius_self); where it refuses (and
  //! allow_host_loop is on), and in a build with PICO_TREE_HOST_ONLY defined,
  //! by a loop over the per-point member.  \p radius must be >= 0 and not NaN.
  inline void search_radius_self(
      scalar_type const radius, std::vector<std::vector<neighbor_type>>& rows, bool const sort = false) const {
    batched_radius_self(radius, nullptr, rows, sort);
  }

  //! ... with one radius per tree point, by original index; radii.size() must
  //! be size() (std::invalid_argument otherwise), every entry >= 0 and not NaN.
  inline void search_radius_self(
      std::vector<scalar_type> const& radii, std::vector<std::vector<neighbor_type>>& rows, bool const sort = false) const {
    check_radii(radii, view().size());
    batched_radius_self(scalar_type(0), radii.data(), rows, sort);
  }

  //! counts[i] = the length of row i of search_radius_self, clamped to
  //! \p max_count when that is > 0 (after the point itself has left); counts
  //! must hold size() entries.
  inline void count_within_self(scalar_type const radius, size_type* counts, size_type const max_count = 0) const {
    batched_count_within_self(radius, nullptr, counts, max_count);
  }

  inline void count_within_self(
      std::vector<scalar_type> const& radii, size_type* counts, size_type const max_count = 0) const {
    check_radii(radii, view().size());
    batched_count_within_self(scalar_type(0), radii.data(), counts, max_count);
  }

  //! The clusters of the tree's points: the connected components of the
  //! fixed-radius graph, with DBSCAN's core-point rule.  With row i being
  //! search_radius_self's row i: point i is core iff that row has at least
  //! \p min_neighbors entries (0: every point); core points i and j are joined
  //! whenever j is in row i or i in row j.  labels (size() entries): a core
  //! point gets the smallest index among the core points of its component, a
  //! non-core point the smallest label among the core points of its own row,
  //! -1 (noise) without one.  Served by the backend (ptk_cluster_within_self);
  //! where it refuses (and allow_host_loop is on), and in a build with
  //! PICO_TREE_HOST_ONLY defined, by the per-point member plus a union-find.
  inline void cluster_within_self(scalar_type const radius, std::int32_t* labels, size_type const min_neighbors = 0) const {
    batched_cluster_within_self(radius, nullptr, labels, min_neighbors);
  }

  inline void cluster_within_self(
      std::vector<scalar_type> const& radii, std::int32_t* labels, size_type const min_neighbors = 0) const {
    check_radii(radii, view().size());
    batched_cluster_within_self(scalar_type(0), radii.data(), labels, min_neighbors);
  }

  //! The minimum spanning forest of the fixed-radius graph over the tree's
  //! points (float points, metric_l2_squared or metric_l1).  {i, j} is an edge
  //! iff j is in search_radius_self's row i or i in row j; its weight is the
  //! row's distance, or with \p core (size() float entries by original index,
  //! in the metric's unit, none NaN or negative: std::invalid_argument)
  //! max(d, core[i], core[j]), and the edge then exists only if that is below
  //! \p radius too.  Edges are ordered by (bits(w), lo, hi)
  //! (internal/mst.hpp), which makes the forest unique.  edges: size() - 1
  //! records; returned ascending in that order, the return value is their
  //! number (size() minus the number of components).  labels (may be null):
  //! size() entries, the smallest index of the point's component.  Served by
  //! the backend (ptk_mst_within_self); where it refuses (and allow_host_loop
  //! is on), and in a build with PICO_TREE_HOST_ONLY defined, by the per-point
  //! member plus Kruskal.
  inline size_type mst_within_self(
      scalar_type const radius, internal::mst_edge* edges, float const* core = nullptr,
      std::int32_t* labels = nullptr) const {
    return batched_mst_within_self(radius, core, edges, labels);
  }

  //! Greedy radius suppression of the tree's points: thinning to an r-separated
  //! subset, or non-maximum suppression under \p scores.  With row i being
  //! search_radius_self's row i and key(i) = (ord_i << 32) | (0xFFFFFFFF - i)
  //! -- ord_i the total-order map of the bits of scores[i], or fmix32(i) when
  //! \p scores is null (internal/suppress.hpp) -- keep[i] = 1 iff row i holds
  //! no j with key(j) > key(i) and keep[j] == 1, else 0: the greedy pass in
  //! descending key.  keep: size() entries; scores: null or size() float
  //! entries, none NaN (std::invalid_argument).  Served by the backend
  //! (ptk_suppress_within_self); where it refuses (and allow_host_loop is on),
  //! and in a build with PICO_TREE_HOST_ONLY defined, by the per-point member
  //! plus the greedy pass.
  inline void suppress_within_self(scalar_type const radius, std::uint8_t* keep, float const* scores = nullptr) const {
    batched_suppress_within_self(radius, nullptr, scores, keep);
  }

  inline void suppress_within_self(
      std::vector<scalar_type> const& radii, std::uint8_t* keep, float const* scores = nullptr) const {
    check_radii(radii, view().size());
    batched_suppress_within_self(scalar_type(0), radii.data(), scores, keep);
  }

  //! PCA normals and curvature of the tree's points (float points, three
  //! dimensions, a non-topological metric).  The neighbourhood of point i is
  //! row i of search_radius_self (unsorted) plus the point itself; frames[i]
  //! holds the unit normal (the eigenvector of the smallest eigenvalue of the
  //! neighbourhood's covariance), the curvature l0 / (l0 + l1 + l2), the
  //! eigenvalues in ascending order and the row's length.  A row shorter than
  //! max(min_neighbors, 2) gives NaN.  \p viewpoint (3 scalars, or null) turns
  //! every normal towards it; without one the component of largest magnitude
  //! is positive.  \p moments, if given, receives the sums the covariance was
  //! made from.  Served by the backend (ptk_normals_within_self); where it
  //! refuses (and allow_host_loop is on), and in a build with
  //! PICO_TREE_HOST_ONLY defined, by the per-point member with the routine of
  //! internal/local_frame.hpp: the same bytes either way.
  inline void normals_within_self(
      scalar_type const radius,
      std::vector<local_frame>& frames,
      size_type const min_neighbors = 2,
      scalar_type const* viewpoint = nullptr,
      std::vector<local_moments>* moments = nullptr) const {
    batched_normals_within_self(radius, nullptr, frames, min_neighbors, viewpoint, moments);
  }

  inline void normals_within_self(
      std::vector<scalar_type> const& radii,
      std::vector<local_frame>& frames,
      size_type const min_neighbors = 2,
      scalar_type const* viewpoint = nullptr,
      std::vector<local_moments>* moments = nullptr) const {
    check_radii(radii, view().size());
    batched_normals_within_self(scalar_type(0), radii.data(), frames, min_neighbors, viewpoint, moments);
  }

  //! The sum, minimum or maximum of a per-point value over every tree point's
  //! neighbourhood (float points).  \p values holds size() x \p channels floats,
  //! row-major, by original point index; row i of \p out (resized to size() x
  //! channels) folds values[j] over row i of search_radius_self (unsorted),
  //! channel by channel in row order: sum from +0 with acc + v, max from -inf
  //! with (v > acc) ? v : acc, min from +inf with (v < acc) ? v : acc.  With
  //! \p include_self the fold starts at the point's own value.  \p counts, if
  //! given, receives the row lengths.  Served by the backend
  //! (ptk_aggregate_within_self); where it refuses (and allow_host_loop is on),
  //! and in a build with PICO_TREE_HOST_ONLY defined, by a loop over the
  //! per-point member with the fold of internal/aggregate.hpp: the same bytes
  //! either way.
  inline void aggregate_within_self(
      scalar_type const radius,
      scalar_type const* values,
      size_type const channels,
      aggregate_op const op,
      bool const include_self,
      std::vector<scalar_type>& out,
      std::vector<size_type>* counts = nullptr) const {
    batched_aggregate_within_self(radius, nullptr, values, channels, op, include_self, out, counts);
  }

  inline void aggregate_within_self(
      std::vector<scalar_type> const& radii,
      scalar_type const* values,
      size_type const channels,
      aggregate_op const op,
      bool const include_self,
      std::vector<scalar_type>& out,
      std::vector<size_type>* counts = nullptr) const {
    check_radii(radii, view().size());
    batched_aggregate_within_self(scalar_type(0), radii.data(), values, channels, op, include_self, out, counts);
  }

  //! The same over the rows of search_radius (unsorted) of a query batch: row i
  //! of \p out (resized to queries x channels) folds values[j] over the
  //! neighbours of query i.  A query has no own point: this is also the form
  //! for a subset of the tree's points.
  template <typename QuerySpace_>
  inline void aggregate_within(
      QuerySpace_ const& queries,
      scalar_type const radius,
      scalar_type const* values,
      size_type const channels,
      aggregate_op const op,
      std::vector<scalar_type>& out,
      std::vector<size_type>* counts = nullptr) const {
    batched_aggregate_within(queries, radius, nullptr, values, channels, op, out, counts);
  }

  template <typename QuerySpace_>
  inline void aggregate_within(
      QuerySpace_ const& queries,
      std::vector<scalar_type> const& radii,
      scalar_type const* values,
      size_type const channels,
      aggregate_op const op,
      std::vector<scalar_type>& out,
      std::vector<size_type>* counts = nullptr) const {
    batched_aggregate_within(queries, scalar_type(0), &radii, values, channels, op, out, counts);
  }

  //! The normal equations of one ICP iteration (float points, three
  //! dimensions, metric_l2_squared).  Each query is posed by \p transform (12
  //! scalars, row-major [R|t], applied in float32; null: as it is), matched to
  //! its nearest tree point (search_knn with k = 1), rejected where the squared
  //! distance is not below \p max_distance, and the terms of the accepted rows
  //! are summed in double in the fixed order of internal/align.hpp: the
  //! point-to-point sums without \p normals, the point-to-plane sums with them
  //! (size() x 3 scalars by original point index).  \p rows, if given, receives
  //! the unfiltered rows.  Served by the backend (ptk_align_step); where it
  //! refuses (and allow_host_loop is on), and in a build with
  //! PICO_TREE_HOST_ONLY defined, by the per-point member with the routines of
  //! internal/align.hpp: the same bytes either way.
  template <typename QuerySpace_>
  inline align_sums align_step(
      QuerySpace_ const& queries,
      scalar_type const* transform,
      scalar_type const max_distance,
      scalar_type const* normals = nullptr,
      std::vector<neighbor_type>* rows = nullptr) const {
    return batched_align_step(queries, transform, max_distance, normals, rows);
  }

  //! counts[i] = count_within(query i, radius), clamped to \p max_count when
  //! that is > 0.  \p radius must be >= 0 and not NaN.
  template <typename QuerySpace_>
  inline void count_within(
      QuerySpace_ const& queries,
      scalar_type const radius,
      size_type* counts,
      size_type const max_count = 0) const {
    batched_count_within(queries, radius, counts, max_count);
  }

  //! A radius per query row: row i of \p out is row i of the member above
  //! with radius = radii[i] (padded with {-1, radii[i]}); radii.size() must be
  //! the number of queries (std::invalid_argument otherwise), every entry >= 0
  //! and not NaN.  Served by the backend where the scalar form is; where it
  //! refuses (and allow_host_loop is on), and in a build with
  //! PICO_TREE_HOST_ONLY defined (no backend linked), by a loop over the
  //! single-query member.
  template <typename QuerySpace_>
  inline void search_knn_within(
      QuerySpace_ const& queries,
      size_type const k,
      std::vector<scalar_type> const& radii,
      neighbor_type* out) const {
    batched_knn_within_radii(queries, k, radii, out);
  }

  //! counts[i] = count_within(query i, radii[i]), clamped to \p max_count when
  //! that is > 0; \p radii as above.
  template <typename QuerySpace_>
  inline void count_within(
      QuerySpace_ const& queries,
      std::vector<scalar_type> const& radii,
      size_type* counts,
      size_type const max_count = 0) const {
    batched_count_within_radii(queries, radii, counts, max_count);
  }

  //! out[i] = all neighbours of query i within \p radius.
  template <typename QuerySpace_>
  inline void search_radius(
      QuerySpace_ const& queries,
      scalar_type const radius,
      std::vector<std::vector<neighbor_type>>& out,
      bool const sort = false) const {
    batched_radius(queries, radius, scalar_type(1.0), out, sort);
  }

  template <typename QuerySpace_>
  inline void search_radius(
      QuerySpace_ const& queries,
      scalar_type const radius,
      scalar_type const e,
      std::vector<std::vector<neighbor_type>>& out,
      bool const sort = false) const {
    batched_radius(queries, radius, e, out, sort);
  }

  //! Flat ragged form: row i is flat[offsets[i] .. offsets[i + 1]).
  template <typename QuerySpace_>
  inline void search_radius(
      QuerySpace_ const& queries,
      scalar_type const radius,
      std::vector<std::uint64_t>& offsets,
      std::vector<neighbor_type>& flat,
      bool const sort = false) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    offsets.assign(q.rows() + 1, 0);
    typename api::neighbor* rows = nullptr;
    try {
      internal::ptk_check(
          api::radius(
              device(), q.data(), q.rows(), radius, scalar_type(1), sort ? 1 : 0,
              offsets.data(), &rows),
          "ptk_search_radius");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (the batched path has no CPU fallback unless asked for)
      std::vector<std::vector<neighbor_type>> per_row;
      host_radius(q, radius, scalar_type(1), per_row, sort, refused.what());
      for (size_type i = 0; i < q.rows(); ++i) offsets[i + 1] = offsets[i] + per_row[i].size();
      flat.resize(offsets.back());
      for (size_type i = 0; i < q.rows(); ++i) std::copy(per_row[i].begin(), per_row[i].end(), flat.data() + offsets[i]);
      return;
    }
    library_rows keep(rows);  // freed even if the copy below throws
    flat.resize(offsets.back());
    auto const* src = reinterpret_cast<neighbor_type const*>(rows);
    std::copy(src, src + flat.size(), flat.data());
  }

  //! A radius per query row: out[i] = search_radius(query i, radii[i]) -- row i
  //! of the member above with radius = radii[i], exact (no e), sorted ascending
  //! by distance when \p sort.  radii.size() must be the number of queries
  //! (std::invalid_argument otherwise), every entry >= 0 and not NaN.  Served
  //! by the backend where count_within with a vector of radii is; where it
  //! refuses (and allow_host_loop is on), and in a build with
  //! PICO_TREE_HOST_ONLY defined (no backend linked), by a loop over the
  //! single-query member.
  template <typename QuerySpace_>
  inline void search_radius(
      QuerySpace_ const& queries,
      std::vector<scalar_type> const& radii,
      std::vector<std::vector<neighbor_type>>& out,
      bool const sort = false) const {
    std::vector<std::uint64_t> offsets;
    std::vector<neighbor_type> flat;
    if (batched_radius_radii(queries, radii, offsets, flat, &out, sort)) return;
    out.resize(offsets.size() - 1);
    for (size_type i = 0; i + 1 < offsets.size(); ++i) {
      out[i].assign(flat.begin() + offsets[i], flat.begin() + offsets[i + 1]);
    }
  }

  //! ... in the flat ragged form: row i is flat[offsets[i] .. offsets[i + 1]).
  template <typename QuerySpace_>
  inline void search_radius(
      QuerySpace_ const& queries,
      std::vector<scalar_type> const& radii,
      std::vector<std::uint64_t>& offsets,
      std::vector<neighbor_type>& flat,
      bool const sort = false) const {
    std::vector<std::vector<neighbor_type>> per_row;
    if (!batched_radius_radii(queries, radii, offsets, flat, &per_row, sort)) return;
    offsets.assign(per_row.size() + 1, 0);
    for (size_type i = 0; i < per_row.size(); ++i) offsets[i + 1] = offsets[i] + per_row[i].size();
    flat.resize(offsets.back());
    for (size_type i = 0; i < per_row.size(); ++i) std::copy(per_row[i].begin(), per_row[i].end(), flat.data() + offsets[i]);
  }

  //! Batched box search: row i (flat[offsets[i] .. offsets[i + 1])) lists the indices inside the
  //! closed box [mins[i], maxs[i]], in the traversal order of the per-query search_box.
  template <typename BoxSpace_>
  inline void search_box(
      BoxSpace_ const& mins,
      BoxSpace_ const& maxs,
      std::vector<std::uint64_t>& offsets,
      std::vector<index_type>& flat) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    internal::dense_rows<internal::unwrap_ref_t<BoxSpace_>> lo(unwrap(mins)), hi(unwrap(maxs));
    check_query_dim(lo.cols());
    check_query_dim(hi.cols());
    if (lo.rows() != hi.rows()) throw std::invalid_argument("query min and max don't have equal size");
    offsets.assign(lo.rows() + 1, 0);
    std::int32_t* rows = nullptr;
    try {
      internal::ptk_check(
          api::box(device(), lo.data(), hi.data(), lo.rows(), offsets.data(), &rows), "ptk_search_box");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (the batched path has no CPU fallback unless asked for)
      internal::warn_host_loop(refused.what());
      std::vector<std::vector<index_type>> per_row(lo.rows());
      space_view_type s = view();
      internal::host_rows_loop(lo.rows(), [&](size_type i) {
        if constexpr (topological)
          internal::box_search<true>(tree_, s, lo.data() + i * lo.cols(), hi.data() + i * hi.cols(), per_row[i],
                                     internal::circle_axes_of<metric_type>{metric_});
        else
          internal::box_search(tree_, s, lo.data() + i * lo.cols(), hi.data() + i * hi.cols(), per_row[i]);
      });
      for (size_type i = 0; i < lo.rows(); ++i) offsets[i + 1] = offsets[i] + per_row[i].size();
      flat.resize(offsets.back());
      for (size_type i = 0; i < lo.rows(); ++i) std::copy(per_row[i].begin(), per_row[i].end(), flat.data() + offsets[i]);
      return;
    }
    library_rows keep(rows);
    flat.assign(rows, rows + offsets.back());
  }

  //! Uploads the tree to the device now instead of at the first batched call.
  inline void prepare_device() const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    (void)device();
  }

  // ---- introspection --------------------------------------------------------

  //! Index range of every non-empty leaf, in depth-first order.
  inline std::vector<leaf_range_type> leaf_ranges() const {
    std::vector<leaf_range_type> ranges;
    for (auto const& nd : tree_.nodes) {
      if (nd.is_leaf() && nd.begin != nd.end) {
        ranges.emplace_back(
            tree_.indices.cbegin() + nd.begin, tree_.indices.cbegin() + nd.end);
      }
    }
    return ranges;
  }

  inline space_type const& space() const { return space_; }
  inline metric_type const& metric() const { return metric_; }

  // ---- persistence (reference-compatible byte stream) ------------------------

  static kd_tree load(space_type space, std::string const& filename) {
    std::fstream stream =
        internal::open_stream(filename, std::ios::in | std::ios::binary);
    return load(std::move(space), stream);
  }
  static kd_tree load(space_type space, std::iostream& stream) {
    return kd_tree(std::move(space), stream);
  }
  static void save(kd_tree const& tree, std::string const& filename) {
    std::fstream stream =
        internal::open_stream(filename, std::ios::out | std::ios::binary);
    save(tree, stream);
  }
  static void save(kd_tree const& tree, std::iostream& stream) {
    internal::write_flat_tree(tree.tree_, stream);
  }

 private:
  kd_tree(space_type space, std::iostream& stream)
      : space_(std::move(space)),
        metric_(),
        tree_(internal::read_flat_tree<tree_type>(
            stream, topological, space_view_type(unwrap(space_)).sdim(), space_view_type(unwrap(space_)).size())) {}

  //! A result buffer allocated by libptk: released with ptk_free on every path out of the scope.
  struct ptk_free_fn {
    void operator()(void* p) const { ptk_free(p); }
  };
  using library_rows = std::unique_ptr<void, ptk_free_fn>;

  template <typename T_>
  static T_ const& unwrap(T_ const& s) {
    return s;
  }
  template <typename T_>
  static T_ const& unwrap(std::reference_wrapper<T_> const& s) {
    return s.get();
  }

  space_view_type view() const {
    return space_view_type(unwrap(space_));
  }

  typename api::tree* device() const {
    return device_.get(tree_, view(), accelerated ? internal::ptk_metric_v<Metric_> : 0);
  }

  void check_query_dim(size_type qdim) const {
    if (qdim != view().sdim()) {
      throw std::invalid_argument("pico_tree: query dimension differs from the tree's");
    }
  }

  template <typename QuerySpace_>
  void batched_knn(
      QuerySpace_ const& queries, size_type k, scalar_type e, neighbor_type* out) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(sizeof(neighbor_type) == sizeof(typename api::neighbor), "neighbor layout");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    try {
      internal::ptk_check(
          api::knn(
              device(), q.data(), q.rows(), static_cast<std::uint32_t>(k), e,
              reinterpret_cast<typename api::neighbor*>(out)),
          "ptk_search_knn");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (the batched path has no CPU fallback unless asked for)
      // The reference's loop (_pyco_tree/kd_tree.hpp:128-134): row i into out[i * k .. i * k + k).
      internal::warn_host_loop(refused.what());
      using row_point = point_map<scalar_type const, dim>;
      internal::host_rows_loop(q.rows(), [&](size_type i) {
        row_point x = make_row(q.data() + i * q.cols(), q.cols());
        if (e == scalar_type(1)) {
          search_knn(x, out + i * k, out + (i + 1) * k);
        } else {
          search_knn(x, e, out + i * k, out + (i + 1) * k);
        }
      });
    }
  }

  template <typename QuerySpace_>
  void batched_knn_within(
      QuerySpace_ const& queries, size_type k, scalar_type radius, neighbor_type* out) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(sizeof(neighbor_type) == sizeof(typename api::neighbor), "neighbor layout");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    try {
      internal::ptk_check(
          api::knn_within(
              device(), q.data(), q.rows(), static_cast<std::uint32_t>(k), radius,
              reinterpret_cast<typename api::neighbor*>(out)),
          "ptk_search_knn_within");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      using row_point = point_map<scalar_type const, dim>;
      internal::host_rows_loop(q.rows(), [&](size_type i) {
        row_point x = make_row(q.data() + i * q.cols(), q.cols());
        std::vector<neighbor_type> row;
        search_knn_within(x, k, radius, row);
        std::copy(row.begin(), row.end(), out + i * k);
        std::fill(out + i * k + row.size(), out + (i + 1) * k, neighbor_type(index_type(-1), radius));
      });
    }
  }

  template <typename QuerySpace_>
  void batched_count_within(
      QuerySpace_ const& queries, scalar_type radius, size_type* counts, size_type max_count) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    std::vector<std::uint64_t> c(q.rows());
    try {
      internal::ptk_check(
          api::count_within(device(), q.data(), q.rows(), radius, static_cast<std::uint64_t>(max_count), c.data()),
          "ptk_search_count_within");
      std::copy(c.begin(), c.end(), counts);
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      using row_point = point_map<scalar_type const, dim>;
      internal::host_rows_loop(q.rows(), [&](size_type i) {
        row_point x = make_row(q.data() + i * q.cols(), q.cols());
        size_type const n = count_within(x, radius);
        counts[i] = max_count != 0 && n > max_count ? max_count : n;
      });
    }
  }

  void batched_knn_self(size_type k, std::vector<neighbor_type>& out) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(sizeof(neighbor_type) == sizeof(typename api::neighbor), "neighbor layout");
    if (k == 0) throw std::invalid_argument("pico_tree: search_knn_self: k must be >= 1");
    size_type const n = view().size();
    out.resize(n * k);
    // (the per-point member, the row padded)
    auto const rows_loop = [&]() {
      internal::host_rows_loop(n, [&](size_type i) {
        std::vector<neighbor_type> row;
        search_knn_self(static_cast<index_type>(i), k, row);
        std::copy(row.begin(), row.end(), out.begin() + i * k);
        std::fill(
            out.begin() + i * k + row.size(), out.begin() + (i + 1) * k,
            neighbor_type(index_type(-1), std::numeric_limits<scalar_type>::max()));
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    try {
      internal::ptk_check(
          api::knn_self(device(), static_cast<std::uint32_t>(k), reinterpret_cast<typename api::neighbor*>(out.data())),
          "ptk_search_knn_self");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  void batched_spacing_knn_self(
      size_type k, bool sqrt, float ratio, scalar_type* mean, scalar_type* kth, std::uint8_t* keep,
      spacing_stats* stats) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    if (k == 0) throw std::invalid_argument("pico_tree: spacing_knn_self: k must be >= 1");
    bool const reduce = keep != nullptr || stats != nullptr;
    if (reduce && !(ratio >= 0.0f && ratio - ratio == 0.0f)) {
      throw std::invalid_argument("pico_tree: outliers_knn_self: std_ratio must be finite and >= 0");
    }
    size_type const n = view().size();
    // (the per-point member reduced by the one statement of the rule, then the record and the mask from the means)
    auto const rows_loop = [&]() {
      internal::host_rows_loop(n, [&](size_type i) {
        std::vector<neighbor_type> row;
        search_knn_self(static_cast<index_type>(i), k, row);
        scalar_type m, kd;
        internal::spacing_row<scalar_type>(
            [&](std::uint32_t j) { return row[j].distance; }, static_cast<std::uint32_t>(row.size()), sqrt, &m, &kd);
        mean[i] = m;
        if (kth != nullptr) kth[i] = kd;
      });
      if (reduce) internal::spacing_statistics(mean, static_cast<std::uint64_t>(n), ratio, stats, keep);
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    try {
      internal::ptk_check(
          api::spacing_knn_self(
              device(), static_cast<std::uint32_t>(k), sqrt ? internal::spacing_sqrt : 0u, ratio, mean, kth, keep, stats),
          "ptk_spacing_knn_self");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  // (radii null: every point gets `radius`)
  void batched_radius_self(
      scalar_type radius, scalar_type const* radii, std::vector<std::vector<neighbor_type>>& rows, bool sort) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(sizeof(neighbor_type) == sizeof(typename api::neighbor), "neighbor layout");
    size_type const n = view().size();
    auto const rows_loop = [&]() {
      rows.assign(n, std::vector<neighbor_type>());
      internal::host_rows_loop(n, [&](size_type i) {
        search_radius_self(static_cast<index_type>(i), radii != nullptr ? radii[i] : radius, rows[i], sort);
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    std::vector<std::uint64_t> offsets(n + 1, 0);
    typename api::neighbor* flat = nullptr;
    try {
      internal::ptk_check(
          api::radius_self(device(), radius, radii, sort ? 1 : 0, offsets.data(), &flat), "ptk_search_radius_self");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
      return;
    }
    library_rows keep(flat);  // freed even if the copy below throws
    auto const* src = reinterpret_cast<neighbor_type const*>(flat);
    rows.resize(n);
    for (size_type i = 0; i < n; ++i) rows[i].assign(src + offsets[i], src + offsets[i + 1]);
#endif
  }

  void batched_count_within_self(
      scalar_type radius, scalar_type const* radii, size_type* counts, size_type max_count) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    size_type const n = view().size();
    auto const rows_loop = [&]() {
      internal::host_rows_loop(n, [&](size_type i) {
        std::vector<neighbor_type> row;
        search_radius_self(static_cast<index_type>(i), radii != nullptr ? radii[i] : radius, row);
        counts[i] = max_count != 0 && row.size() > max_count ? max_count : row.size();
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    std::vector<std::uint64_t> c(n);
    try {
      internal::ptk_check(
          api::count_within_self(device(), radius, radii, static_cast<std::uint64_t>(max_count), c.data()),
          "ptk_search_count_within_self");
      std::copy(c.begin(), c.end(), counts);
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  void batched_cluster_within_self(
      scalar_type radius, scalar_type const* radii, std::int32_t* labels, size_type min_neighbors) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    size_type const n = view().size();
    auto const rows_loop = [&]() {
      std::vector<std::vector<neighbor_type>> rows(n);
      internal::host_rows_loop(n, [&](size_type i) {
        search_radius_self(static_cast<index_type>(i), radii != nullptr ? radii[i] : radius, rows[i]);
      });
      internal::cluster_rows(rows, static_cast<std::uint64_t>(min_neighbors), labels);
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    try {
      internal::ptk_check(
          api::cluster_within_self(device(), radius, radii, static_cast<std::uint64_t>(min_neighbors), labels),
          "ptk_cluster_within_self");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  size_type batched_mst_within_self(
      scalar_type radius, float const* core, internal::mst_edge* edges, std::int32_t* labels) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(std::is_same<scalar_type, float>::value, "MST_WITHIN_SELF_NEEDS_FLOAT_POINTS");
    size_type const n = view().size();
    if (core != nullptr && internal::mst_first_bad_core(core, n) != n) {
      throw std::invalid_argument("pico_tree: core must not hold a NaN or a negative value");
    }
    if (!(radius >= scalar_type(0))) throw std::invalid_argument("pico_tree: radius must be >= 0 (and not NaN)");
    std::uint64_t count = 0;
    auto const rows_loop = [&]() {
      std::vector<std::vector<neighbor_type>> rows(n);
      internal::host_rows_loop(n, [&](size_type i) { search_radius_self(static_cast<index_type>(i), radius, rows[i]); });
      count = internal::mst_rows(rows, radius, core, edges, labels);
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    try {
      internal::ptk_check(api::mst_within_self(device(), radius, core, edges, &count, labels), "ptk_mst_within_self");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
    return static_cast<size_type>(count);
  }

  void batched_suppress_within_self(
      scalar_type radius, scalar_type const* radii, float const* scores, std::uint8_t* keep) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    size_type const n = view().size();
    if (scores != nullptr && internal::suppress_first_nan(scores, n) != n) {
      throw std::invalid_argument("pico_tree: scores must not hold a NaN");
    }
    auto const rows_loop = [&]() {
      std::vector<std::vector<neighbor_type>> rows(n);
      internal::host_rows_loop(n, [&](size_type i) {
        search_radius_self(static_cast<index_type>(i), radii != nullptr ? radii[i] : radius, rows[i]);
      });
      internal::suppress_rows(rows, scores, keep);
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    try {
      internal::ptk_check(api::suppress_within_self(device(), radius, radii, scores, keep), "ptk_suppress_within_self");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  void batched_normals_within_self(
      scalar_type radius,
      scalar_type const* radii,
      std::vector<local_frame>& frames,
      size_type min_neighbors,
      scalar_type const* viewpoint,
      std::vector<local_moments>* moments) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(std::is_same_v<scalar_type, float>, "NORMALS_WITHIN_SELF_NEEDS_FLOAT_POINTS");
    static_assert(!internal::ptk_topological_v<Metric_>, "NORMALS_WITHIN_SELF_NEEDS_A_NON_TOPOLOGICAL_METRIC");
    auto const points = view();
    if (points.sdim() != 3) throw std::invalid_argument("pico_tree: normals_within_self needs 3-D points");
    size_type const n = points.size();
    frames.resize(n);
    if (moments != nullptr) moments->resize(n);
    auto const rows_loop = [&]() {
      bool const has_view = viewpoint != nullptr;
      float const vx = has_view ? viewpoint[0] : 0.0f, vy = has_view ? viewpoint[1] : 0.0f, vz = has_view ? viewpoint[2] : 0.0f;
      internal::host_rows_loop(n, [&](size_type i) {
        std::vector<neighbor_type> row;
        search_radius_self(static_cast<index_type>(i), radii != nullptr ? radii[i] : radius, row);
        internal::moment_sums sums;
        scalar_type const* p = points[static_cast<index_type>(i)];
        for (neighbor_type const& nb : row) {
          scalar_type const* o = points[nb.index];
          sums.add(p[0] - o[0], p[1] - o[1], p[2] - o[2]);
        }
        frames[i] = internal::frame_of(sums, static_cast<std::uint64_t>(min_neighbors), has_view, vx, vy, vz, p[0], p[1], p[2]);
        if (moments != nullptr) (*moments)[i] = sums.record();
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    static_assert(sizeof(local_frame) == sizeof(ptk_frame) && sizeof(local_moments) == sizeof(ptk_moments), "record layout");
    try {
      internal::ptk_check(
          api::normals_within_self(
              device(), radius, radii, static_cast<std::uint64_t>(min_neighbors), viewpoint,
              reinterpret_cast<ptk_frame*>(frames.data()),
              moments != nullptr ? reinterpret_cast<ptk_moments*>(moments->data()) : nullptr),
          "ptk_normals_within_self");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  template <typename QuerySpace_>
  align_sums batched_align_step(
      QuerySpace_ const& queries,
      scalar_type const* transform,
      scalar_type max_distance,
      scalar_type const* normals,
      std::vector<neighbor_type>* rows) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(std::is_same_v<scalar_type, float>, "ALIGN_STEP_NEEDS_FLOAT_POINTS");
    static_assert(std::is_same_v<Metric_, metric_l2_squared>, "ALIGN_STEP_NEEDS_METRIC_L2_SQUARED");
    static_assert(sizeof(neighbor_type) == sizeof(typename api::neighbor), "neighbor layout");
    auto const points = view();
    if (points.sdim() != 3) throw std::invalid_argument("pico_tree: align_step needs 3-D points");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    if (!(max_distance >= scalar_type(0))) throw std::invalid_argument("pico_tree: align_step needs max_distance >= 0");
    size_type const n = q.rows();
    std::vector<neighbor_type> own;
    std::vector<neighbor_type>& found = rows != nullptr ? *rows : own;
    found.resize(n);
    align_sums out;
    auto const rows_loop = [&]() {
      std::vector<float> posed;
      float const* qp = q.data();
      if (transform != nullptr && n > 0) {
        posed.resize(n * 3);
        internal::host_rows_loop(n, [&](size_type i) {
          internal::align_pose(transform, q.data()[3 * i], q.data()[3 * i + 1], q.data()[3 * i + 2], &posed[3 * i]);
        });
        qp = posed.data();
      }
      // (a slot the search did not write holds {0, FLT_MAX}, as the backend's rows)
      using row_point = point_map<scalar_type const, dim>;
      internal::host_rows_loop(n, [&](size_type i) {
        found[i] = neighbor_type{0, std::numeric_limits<scalar_type>::max()};
        row_point x = make_row(qp + i * 3, 3);
        search_knn(x, &found[i], &found[i] + 1);
      });
      internal::align_reduce_rows(
          qp, n, [&](std::uint64_t i, std::int32_t& index, float& distance) { index = found[i].index, distance = found[i].distance; },
          [&](std::int32_t index) { return points[static_cast<index_type>(index)]; }, normals, max_distance,
          [](std::uint64_t blocks, auto&& f) { internal::host_rows_loop(blocks, [&](size_type b) { f(b); }); }, &out);
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    static_assert(sizeof(align_sums) == sizeof(ptk_align_sums), "record layout");
    try {
      internal::ptk_check(
          api::align_step(
              device(), q.data(), n, transform, max_distance, normals, reinterpret_cast<ptk_align_sums*>(&out),
              reinterpret_cast<typename api::neighbor*>(found.data())),
          "ptk_align_step");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
    return out;
  }

  void check_aggregate(scalar_type const* values, size_type channels) const {
    if (channels == 0 || channels > internal::aggregate_max_channels) {
      throw std::invalid_argument("pico_tree: aggregate_within takes 1 .. 1024 channels");
    }
    if (values == nullptr) throw std::invalid_argument("pico_tree: aggregate_within needs values");
  }

  void batched_aggregate_within_self(
      scalar_type radius,
      scalar_type const* radii,
      scalar_type const* values,
      size_type channels,
      aggregate_op op,
      bool include_self,
      std::vector<scalar_type>& out,
      std::vector<size_type>* counts) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(std::is_same_v<scalar_type, float>, "AGGREGATE_WITHIN_NEEDS_FLOAT_POINTS");
    check_aggregate(values, channels);
    size_type const n = view().size();
    out.assign(n * channels, scalar_type(0));
    if (counts != nullptr) counts->assign(n, 0);
    auto const rows_loop = [&]() {
      internal::host_rows_loop(n, [&](size_type i) {
        std::vector<neighbor_type> row;
        search_radius_self(static_cast<index_type>(i), radii != nullptr ? radii[i] : radius, row);
        internal::aggregate_row(
            values, channels, op, include_self ? values + i * channels : nullptr, row, out.data() + i * channels);
        if (counts != nullptr) (*counts)[i] = row.size();
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    std::vector<std::uint64_t> c(counts != nullptr ? n : 0);
    try {
      internal::ptk_check(
          api::aggregate_within_self(
              device(), radius, radii, values, static_cast<std::uint32_t>(channels),
              static_cast<std::uint32_t>(op) | (include_self ? internal::aggregate_include_self : 0u), out.data(),
              counts != nullptr ? c.data() : nullptr),
          "ptk_aggregate_within_self");
      if (counts != nullptr) std::copy(c.begin(), c.end(), counts->begin());
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  template <typename QuerySpace_>
  void batched_aggregate_within(
      QuerySpace_ const& queries,
      scalar_type radius,
      std::vector<scalar_type> const* radii,
      scalar_type const* values,
      size_type channels,
      aggregate_op op,
      std::vector<scalar_type>& out,
      std::vector<size_type>* counts) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(std::is_same_v<scalar_type, float>, "AGGREGATE_WITHIN_NEEDS_FLOAT_POINTS");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    if (radii != nullptr) check_radii(*radii, q.rows());
    check_aggregate(values, channels);
    size_type const n = q.rows();
    out.assign(n * channels, scalar_type(0));
    if (counts != nullptr) counts->assign(n, 0);
    auto const rows_loop = [&]() {
      using row_point = point_map<scalar_type const, dim>;
      internal::host_rows_loop(n, [&](size_type i) {
        row_point x = make_row(q.data() + i * q.cols(), q.cols());
        std::vector<neighbor_type> row;
        search_radius(x, radii != nullptr ? (*radii)[i] : radius, row);
        internal::aggregate_row(values, channels, op, nullptr, row, out.data() + i * channels);
        if (counts != nullptr) (*counts)[i] = row.size();
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    std::vector<std::uint64_t> c(counts != nullptr ? n : 0);
    try {
      internal::ptk_check(
          api::aggregate_within(
              device(), q.data(), n, radius, radii != nullptr ? radii->data() : nullptr, values,
              static_cast<std::uint32_t>(channels), static_cast<std::uint32_t>(op), out.data(),
              counts != nullptr ? c.data() : nullptr),
          "ptk_aggregate_within");
      if (counts != nullptr) std::copy(c.begin(), c.end(), counts->begin());
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  void check_radii(std::vector<scalar_type> const& radii, size_type rows) const {
    if (radii.size() != rows) {
      throw std::invalid_argument("pico_tree: radii must hold one radius per query");
    }
  }

  template <typename QuerySpace_>
  void batched_knn_within_radii(
      QuerySpace_ const& queries, size_type k, std::vector<scalar_type> const& radii, neighbor_type* out) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(sizeof(neighbor_type) == sizeof(typename api::neighbor), "neighbor layout");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    check_radii(radii, q.rows());
    // (the scalar member's loop with the row's own radius)
    auto const rows_loop = [&]() {
      using row_point = point_map<scalar_type const, dim>;
      internal::host_rows_loop(q.rows(), [&](size_type i) {
        row_point x = make_row(q.data() + i * q.cols(), q.cols());
        std::vector<neighbor_type> row;
        search_knn_within(x, k, radii[i], row);
        std::copy(row.begin(), row.end(), out + i * k);
        std::fill(out + i * k + row.size(), out + (i + 1) * k, neighbor_type(index_type(-1), radii[i]));
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    try {
      internal::ptk_check(
          api::knn_within_radii(
              device(), q.data(), q.rows(), static_cast<std::uint32_t>(k), radii.data(),
              reinterpret_cast<typename api::neighbor*>(out)),
          "ptk_search_knn_within_radii");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  template <typename QuerySpace_>
  void batched_count_within_radii(
      QuerySpace_ const& queries, std::vector<scalar_type> const& radii, size_type* counts, size_type max_count) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    check_radii(radii, q.rows());
    auto const rows_loop = [&]() {
      using row_point = point_map<scalar_type const, dim>;
      internal::host_rows_loop(q.rows(), [&](size_type i) {
        row_point x = make_row(q.data() + i * q.cols(), q.cols());
        size_type const n = count_within(x, radii[i]);
        counts[i] = max_count != 0 && n > max_count ? max_count : n;
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    rows_loop();
#else
    std::vector<std::uint64_t> c(q.rows());
    try {
      internal::ptk_check(
          api::count_within_radii(
              device(), q.data(), q.rows(), radii.data(), static_cast<std::uint64_t>(max_count), c.data()),
          "ptk_search_count_within_radii");
      std::copy(c.begin(), c.end(), counts);
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
    }
#endif
  }

  //! search_radius with a radius per row.  The backend's answer goes to {offsets, flat} (returns false); the loop over
  //! the single-query member -- a refused call under allow_host_loop, a PICO_TREE_HOST_ONLY build -- to per_row (true).
  template <typename QuerySpace_>
  bool batched_radius_radii(
      QuerySpace_ const& queries,
      std::vector<scalar_type> const& radii,
      std::vector<std::uint64_t>& offsets,
      std::vector<neighbor_type>& flat,
      std::vector<std::vector<neighbor_type>>* per_row,
      bool sort) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    static_assert(sizeof(neighbor_type) == sizeof(typename api::neighbor), "neighbor layout");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    check_radii(radii, q.rows());
    // (the scalar member's loop with the row's own radius)
    auto const rows_loop = [&]() {
      per_row->assign(q.rows(), std::vector<neighbor_type>());
      internal::host_rows_loop(q.rows(), [&](size_type i) {
        auto x = make_row(q.data() + i * q.cols(), q.cols());
        search_radius(x, radii[i], (*per_row)[i], sort);
      });
    };
#ifdef PICO_TREE_HOST_ONLY
    (void)offsets;
    (void)flat;
    rows_loop();
    return true;
#else
    offsets.assign(q.rows() + 1, 0);
    typename api::neighbor* rows = nullptr;
    try {
      internal::ptk_check(
          api::radius_radii(device(), q.data(), q.rows(), radii.data(), sort ? 1 : 0, offsets.data(), &rows),
          "ptk_search_radius_radii");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (as batched_knn)
      internal::warn_host_loop(refused.what());
      rows_loop();
      return true;
    }
    library_rows keep(rows);  // freed even if the copy below throws
    flat.resize(offsets.back());
    auto const* src = reinterpret_cast<neighbor_type const*>(rows);
    std::copy(src, src + flat.size(), flat.data());
    return false;
#endif
  }

  //! Row i of a dense query matrix as a point.
  static point_map<scalar_type const, dim> make_row(scalar_type const* p, size_type sdim) {
    if constexpr (dim == dynamic_extent) {
      return point_map<scalar_type const, dim>(p, sdim);
    } else {
      (void)sdim;
      return point_map<scalar_type const, dim>(p);
    }
  }

  template <typename Rows_>
  void host_radius(
      Rows_ const& q,
      scalar_type radius,
      scalar_type e,
      std::vector<std::vector<neighbor_type>>& out,
      bool sort,
      char const* why) const {
    internal::warn_host_loop(why);
    out.resize(q.rows());
    internal::host_rows_loop(q.rows(), [&](size_type i) {
      auto x = make_row(q.data() + i * q.cols(), q.cols());
      if (e == scalar_type(1)) {
        search_radius(x, radius, out[i], sort);
      } else {
        search_radius(x, radius, e, out[i], sort);
      }
    });
  }

  template <typename QuerySpace_>
  void batched_radius(
      QuerySpace_ const& queries,
      scalar_type radius,
      scalar_type e,
      std::vector<std::vector<neighbor_type>>& out,
      bool sort) const {
    static_assert(accelerated, "BATCHED_SEARCH_NEEDS_A_BACKEND_METRIC_FLOAT_OR_DOUBLE_INT");
    internal::dense_rows<internal::unwrap_ref_t<QuerySpace_>> q(unwrap(queries));
    check_query_dim(q.cols());
    std::vector<std::uint64_t> offsets(q.rows() + 1, 0);
    typename api::neighbor* rows = nullptr;
    try {
      internal::ptk_check(
          api::radius(
              device(), q.data(), q.rows(), radius, e, sort ? 1 : 0, offsets.data(), &rows),
          "ptk_search_radius");
    } catch (internal::ptk_unsupported const& refused) {
      if (!internal::host_loop_flag().load()) throw;  // (the batched path has no CPU fallback unless asked for)
      host_radius(q, radius, e, out, sort, refused.what());
      return;
    }
    library_rows keep(rows);
    out.resize(q.rows());
    auto const* src = reinterpret_cast<neighbor_type const*>(rows);
    for (size_type i = 0; i < q.rows(); ++i) {
      out[i].assign(src + offsets[i], src + offsets[i + 1]);
    }
  }

  space_type space_;
  metric_type metric_;
  tree_type tree_;
  internal::device_tree<std::conditional_t<accelerated, scalar_type, float>> device_;
};

template <typename Space_, typename... Args>
kd_tree(Space_, Args...) -> kd_tree<Space_, metric_l2_squared, int>;

template <
    typename Metric_ = metric_l2_squared,
    typename Index_ = int,
    typename Bounds_ = bounds_from_space_t,
    typename Rule_ = sliding_midpoint_max_side_t,
    typename Space_,
    typename Stop_>
kd_tree<std::decay_t<Space_>, Metric_, Index_> make_kd_tree(
    Space_&& space,
    splitter_stop_condition_t<Stop_> const& stop_condition,
    splitter_start_bounds_t<Bounds_> const& start_bounds = Bounds_{},
    splitter_rule_t<Rule_> const& rule = Rule_{}) {
  return kd_tree<std::decay_t<Space_>, Metric_, Index_>(
      std::forward<Space_>(space), stop_condition, start_bounds, rule);
}

}  // namespace pico_tree
