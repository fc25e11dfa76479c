// align.hpp -- align_step (ptk.h): the pose, the acceptance test, the terms of one ICP iteration's normal
// equations and the fixed summation tree over the caller's row order, as the contract reads.  ONE statement of each:
// compiled for the device by the kernels of pico_tree_amd/csrc/ptk_kernels_align.hpp (K22), for the library's host loop
// (ptk_host_align_step) and for kd_tree::align_step where the backend does not serve.
//
// Every operation is one IEEE operation of the stated width, in the order written: the units that include this header
// are compiled with -ffp-contract=off.  The pose is float32; the terms and the sums are float64.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define PICO_TREE_HD __host__ __device__
#else
#define PICO_TREE_HD
#endif

namespace pico_tree::internal {

//! ptk_align_sums (ptk.h): 384 bytes.
struct align_sums {
  std::uint64_t count;
  std::uint64_t rows;
  double sum_distance;
  double sum_q[3], sum_p[3], sum_qp[9], sum_qq, sum_pp;
  double jtj[21], jtr[6], sum_rr;
};
static_assert(sizeof(align_sums) == 384, "record layout");

//! Rows of one block of the summation tree, and the lanes that share it.
constexpr int align_block = 256;
constexpr int align_lanes = 64;
//! Terms of a row: sum_distance first, then the 17 point-to-point sums or the 28 point-to-plane sums, in the order of the
//! record.  Term j of a mode is double number align_slot(plane, j) of the record, counted from sum_distance.
constexpr int align_point_terms = 18;
constexpr int align_plane_terms = 29;
constexpr int align_max_terms = align_plane_terms;
constexpr int align_record_doubles = 46;
PICO_TREE_HD constexpr int align_terms(bool plane) { return plane ? align_plane_terms : align_point_terms; }
PICO_TREE_HD constexpr int align_slot(bool plane, int j) { return (plane && j > 0) ? j + (align_point_terms - 1) : j; }

//! The blocks of a level of n entries, and the levels of a batch of n rows (at least one level where n > 0).
PICO_TREE_HD constexpr std::uint64_t align_blocks(std::uint64_t n) { return (n + (align_block - 1)) / align_block; }

//! q' = R q + t in float32: ((R_a0*x + R_a1*y) + R_a2*z) + t_a; \p m is row-major [R|t], 12 floats.
PICO_TREE_HD inline void align_pose(float const* m, float x, float y, float z, float* out) {
  for (int a = 0; a < 3; ++a) {
    float const* r = m + 4 * a;
    out[a] = ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
  }
}

PICO_TREE_HD inline bool align_finite(float x) { return x - x == 0.0f; }

//! Is a row accepted: strictly below the rejection distance and below FLT_MAX (the pad and every NaN or infinite row
//! fail the second test).
PICO_TREE_HD inline bool align_accept(float distance, float max_distance) {
  return distance < max_distance && distance < 3.402823466e+38f;
}

//! The 18 point-to-point terms of an accepted row.
PICO_TREE_HD inline void align_point_row(float const* qf, float const* pf, float distance, double* t) {
  double const q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
  double const p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
  t[0] = (double)distance;
  for (int a = 0; a < 3; ++a) t[1 + a] = q[a];
  for (int a = 0; a < 3; ++a) t[4 + a] = p[a];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) t[7 + 3 * a + b] = q[a] * p[b];
  t[16] = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
  t[17] = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
}

//! The 29 point-to-plane terms of an accepted row.
PICO_TREE_HD inline void align_plane_row(float const* qf, float const* pf, float const* nf, float distance, double* t) {
  double const q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
  double const p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
  double const n[3] = {(double)nf[0], (double)nf[1], (double)nf[2]};
  double const ex = q[0] - p[0], ey = q[1] - p[1], ez = q[2] - p[2];
  double const r = ((ex * n[0]) + (ey * n[1])) + (ez * n[2]);
  double J[6];
  J[0] = (q[1] * n[2]) - (q[2] * n[1]);
  J[1] = (q[2] * n[0]) - (q[0] * n[2]);
  J[2] = (q[0] * n[1]) - (q[1] * n[0]);
  J[3] = n[0], J[4] = n[1], J[5] = n[2];
  t[0] = (double)distance;
  int k = 1;
  for (int u = 0; u < 6; ++u)
    for (int v = u; v < 6; ++v) t[k++] = J[u] * J[v];
  for (int u = 0; u < 6; ++u) t[22 + u] = J[u] * r;
  t[28] = r * r;
}

//! What a lane adds up before the butterfly: its four entries of the block, from +0.
PICO_TREE_HD inline double align_lane_fold(double a, double b, double c, double d) {
  return (((0.0 + a) + b) + c) + d;
}

//! The partial of one block: \p x holds \p n <= 256 entries, the entries past the end are +0.
inline double align_block_sum(double const* x, std::size_t n) {
  double v[align_lanes];
  auto at = [&](std::size_t i) { return i < n ? x[i] : 0.0; };
  for (std::size_t l = 0; l < (std::size_t)align_lanes; ++l)
    v[l] = align_lane_fold(at(l), at(l + 64), at(l + 128), at(l + 192));
  for (int s = align_lanes / 2; s >= 1; s /= 2)
    for (int l = 0; l < s; ++l) v[l] = v[l] + v[l + s];
  return v[0];
}

//! The upper levels: \p partials holds \p terms arrays of \p n entries (array j at partials + j * n); reduced level by
//! level until one value per term is left, which goes to out[j].
inline void align_upper_levels(std::vector<double> partials, std::uint64_t n, int terms, double* out) {
  while (n > 1) {
    std::uint64_t const m = align_blocks(n);
    std::vector<double> next((std::size_t)m * (std::size_t)terms);
    for (int j = 0; j < terms; ++j)
      for (std::uint64_t b = 0; b < m; ++b) {
        std::uint64_t const lo = b * align_block;
        std::uint64_t const len = n - lo < (std::uint64_t)align_block ? n - lo : (std::uint64_t)align_block;
        next[(std::size_t)j * m + b] = align_block_sum(partials.data() + (std::size_t)j * n + lo, (std::size_t)len);
      }
    partials.swap(next);
    n = m;
  }
  for (int j = 0; j < terms; ++j) out[j] = partials[(std::size_t)j];
}

//! Writes the record from the reduced terms of a mode: the other mode's sums are +0.
inline void align_record(bool plane, std::uint64_t count, std::uint64_t rows, double const* reduced, align_sums* out) {
  double d[align_record_doubles];
  for (int i = 0; i < align_record_doubles; ++i) d[i] = 0.0;
  if (reduced != nullptr)
    for (int j = 0; j < align_terms(plane); ++j) d[align_slot(plane, j)] = reduced[j];
  out->count = count;
  out->rows = rows;
  std::memcpy(&out->sum_distance, d, sizeof d);
}
static_assert(offsetof(align_sums, sum_distance) == 16 && offsetof(align_sums, jtj) == 16 + 18 * 8, "record layout");

//! align_step on the host over rows that are there already.  \p q: the posed queries q' [nq, 3]; \p index / \p distance
//! of row i through \p row(i, index, distance); \p point(index): the three coordinates of a tree point, \p normals
//! [n_points, 3] (null: point-to-point), both by original index.  \p for_blocks(n, f) calls f(b) for every b in [0, n),
//! in any order, on any threads.
template <class RowFn, class PointFn, class ForBlocks>
inline void align_reduce_rows(
    float const* q, std::uint64_t nq, RowFn&& row, PointFn&& point, float const* normals, float max_distance,
    ForBlocks&& for_blocks, align_sums* out) {
  bool const plane = normals != nullptr;
  int const terms = align_terms(plane);
  if (nq == 0) {
    align_record(plane, 0, 0, nullptr, out);
    return;
  }
  std::uint64_t const blocks = align_blocks(nq);
  std::vector<double> partials((std::size_t)blocks * (std::size_t)terms);
  std::vector<std::uint64_t> counts((std::size_t)blocks);
  for_blocks(blocks, [&](std::uint64_t b) {
    std::uint64_t const lo = b * align_block;
    std::size_t const len = (std::size_t)(nq - lo < (std::uint64_t)align_block ? nq - lo : (std::uint64_t)align_block);
    double x[align_max_terms][align_block];
    std::uint64_t accepted = 0;
    for (std::size_t r = 0; r < len; ++r) {
      double t[align_max_terms];
      for (int j = 0; j < terms; ++j) t[j] = 0.0;
      std::int32_t index = 0;
      float distance = 0.0f;
      row(lo + r, index, distance);
      if (align_accept(distance, max_distance)) {
        float const* qi = q + 3 * (lo + r);
        float const* p = point(index);
        if (!plane) {
          align_point_row(qi, p, distance, t);
          ++accepted;
        } else {
          float const* n = normals + 3 * (std::size_t)index;
          if (align_finite(n[0]) && align_finite(n[1]) && align_finite(n[2])) {
            align_plane_row(qi, p, n, distance, t);
            ++accepted;
          }
        }
      }
      for (int j = 0; j < terms; ++j) x[j][r] = t[j];
    }
    for (int j = 0; j < terms; ++j) partials[(std::size_t)j * blocks + b] = align_block_sum(x[j], len);
    counts[(std::size_t)b] = accepted;
  });
  std::uint64_t count = 0;
  for (std::uint64_t c : counts) count += c;
  double reduced[align_max_terms];
  align_upper_levels(std::move(partials), blocks, terms, reduced);
  align_record(plane, count, nq, reduced, out);
}

}  // namespace pico_tree::internal

namespace pico_tree {

//! The record of kd_tree::align_step.
using align_sums = internal::align_sums;

}  // namespace pico_tree
