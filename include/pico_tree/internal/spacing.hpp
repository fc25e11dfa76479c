// spacing.hpp -- spacing_knn_self (ptk.h): the reduction of one row of search_knn_self to its mean and k-th
// distance, the validity of a mean, the deviation term, the two finishes of the statistics record and the keep test, as
// the contract reads.  ONE statement of each: compiled for the device by the kernels of
// pico_tree_amd/csrc/ptk_kernels_spacing.hpp (K24) and for the library's host loop (ptk_host_spacing_knn_self).  The sums
// of the record run over align_step's summation tree (pico_tree/internal/align.hpp).
//
// Every operation is one IEEE operation of the stated width, in the order written: the units that include this header
// are compiled with -ffp-contract=off.  The row is reduced in the tree's scalar type; the record is float64.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "pico_tree/internal/align.hpp"

namespace pico_tree::internal {

//! ptk_spacing_stats (ptk.h): 64 bytes.
struct spacing_stats {
  std::uint64_t count;
  std::uint64_t rows;
  double sum, mean, ssd, variance, ratio_squared, reserved;
};
static_assert(sizeof(spacing_stats) == 64, "record layout");

//! PTK_SPACING_SQRT (ptk.h).
constexpr std::uint32_t spacing_sqrt = 1u;

//! The correctly rounded square root of the width.  (Device, float32: the plain square root, which hipcc rounds correctly
//! unless it is told otherwise -- __fsqrt_rn is the NATIVE, approximate one in the default configuration of the device
//! headers.  Device, float64: __dsqrt_rn.)
PICO_TREE_HD inline float spacing_root(float d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_sqrtf(d);
#else
  return std::sqrt(d);
#endif
}
PICO_TREE_HD inline double spacing_root(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(d);
#else
  return std::sqrt(d);
#endif
}

//! The rule of a row, entry by entry in rank order: add() every distance of the row (the pad and everything behind it
//! fails `< fmax` and changes nothing), then read m, kth and mean().
template <class Real>
struct spacing_fold {
  Real s, kth;
  std::uint32_t m;
  PICO_TREE_HD static constexpr Real fmax() { return std::numeric_limits<Real>::max(); }
  PICO_TREE_HD spacing_fold() : s((Real)0), kth(fmax()), m(0u) {}
  PICO_TREE_HD void add(Real distance, bool root) {
    if (distance < fmax()) {
      Real const d = root ? spacing_root(distance) : distance;
      s = s + d;
      kth = d;
      ++m;
    }
  }
  PICO_TREE_HD Real mean() const { return m > 0u ? s / (Real)m : fmax(); }
};

//! The same over a row read through get(j), j < k: the distances of search_knn_self's row.
template <class Real, class Get>
PICO_TREE_HD inline void spacing_row(Get&& get, std::uint32_t k, bool root, Real* mean, Real* kth) {
  spacing_fold<Real> f;
  for (std::uint32_t j = 0; j < k; ++j) f.add(get(j), root);
  *mean = f.mean();
  *kth = f.kth;
}

//! valid_i = m_i > 0 && mean_i is finite, read from the mean alone: m_i == 0 iff mean_i == fmax.  (Every accepted d_j is
//! below fmax and no NaN is accepted.  With m == 1 the mean is d_0 < fmax; with m >= 2 a finite s is at most fmax, so
//! s / m <= fmax / 2; an s that overflowed gives +inf, which fails the second test.)
template <class Real>
PICO_TREE_HD inline bool spacing_valid(Real mean) {
  return mean < std::numeric_limits<Real>::max() && mean - mean == (Real)0;
}
//! x_i
template <class Real>
PICO_TREE_HD inline double spacing_x(Real mean) {
  return spacing_valid(mean) ? (double)mean : 0.0;
}
//! The term of ssd.
template <class Real>
PICO_TREE_HD inline double spacing_deviation(Real mean, double global_mean) {
  if (!spacing_valid(mean)) return 0.0;
  double const e = (double)mean - global_mean;
  return e * e;
}
PICO_TREE_HD inline double spacing_mean_of(std::uint64_t count, double sum) { return count > 0 ? sum / (double)count : 0.0; }
PICO_TREE_HD inline double spacing_variance_of(std::uint64_t count, double ssd) {
  return count > 1 ? ssd / (double)(count - 1) : 0.0;
}
PICO_TREE_HD inline double spacing_ratio_squared(float ratio) { return (double)ratio * (double)ratio; }
//! keep_i
template <class Real>
PICO_TREE_HD inline std::uint8_t spacing_keep(Real mean, double global_mean, double ratio_squared, double variance) {
  if (!spacing_valid(mean)) return 0;
  double const e = (double)mean - global_mean;
  return (e <= 0.0 || e * e <= ratio_squared * variance) ? 1 : 0;
}

//! One sum of the record: align_step's summation tree over term(i), i < n, in index order.
template <class Term>
inline double spacing_tree_sum(std::uint64_t n, Term&& term) {
  if (n == 0) return 0.0;
  std::uint64_t const blocks = align_blocks(n);
  std::vector<double> partials((std::size_t)blocks);
  for (std::uint64_t b = 0; b < blocks; ++b) {
    std::uint64_t const lo = b * align_block;
    std::size_t const len = (std::size_t)(n - lo < (std::uint64_t)align_block ? n - lo : (std::uint64_t)align_block);
    double x[align_block];
    for (std::size_t r = 0; r < len; ++r) x[r] = term(lo + r);
    partials[(std::size_t)b] = align_block_sum(x, len);
  }
  double out = 0.0;
  align_upper_levels(std::move(partials), blocks, 1, &out);
  return out;
}

//! The record and the mask (either may be null) from the n means, on the host.
template <class Real>
inline void spacing_statistics(Real const* mean, std::uint64_t n, float ratio, spacing_stats* stats, std::uint8_t* keep) {
  spacing_stats r;
  r.rows = n;
  r.count = 0;
  for (std::uint64_t i = 0; i < n; ++i) r.count += spacing_valid(mean[i]) ? 1u : 0u;
  r.sum = spacing_tree_sum(n, [&](std::uint64_t i) { return spacing_x(mean[i]); });
  r.mean = spacing_mean_of(r.count, r.sum);
  r.ssd = spacing_tree_sum(n, [&](std::uint64_t i) { return spacing_deviation(mean[i], r.mean); });
  r.variance = spacing_variance_of(r.count, r.ssd);
  r.ratio_squared = spacing_ratio_squared(ratio);
  r.reserved = 0.0;
  if (stats != nullptr) *stats = r;
  if (keep != nullptr)
    for (std::uint64_t i = 0; i < n; ++i) keep[i] = spacing_keep(mean[i], r.mean, r.ratio_squared, r.variance);
}

}  // namespace pico_tree::internal

namespace pico_tree {

//! The record of spacing_knn_self.
using spacing_stats = internal::spacing_stats;

}  // namespace pico_tree
