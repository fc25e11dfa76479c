// ptk_kernels_spacing.hpp -- spacing_knn_self (ptk.h): the mean and the k-th of each tree point's
// k nearest other points without the rows, and the global statistics and keep mask of statistical outlier removal.
//
//   spacing_self_kernel    route 1.  The traversal of knn_self_kernel (K17: lane j is leaf-order record first + j, a
//                          register list of k + 1 entries), with another exit: the drop rule is applied to the list in
//                          registers, the row is reduced there by the rule of pico_tree/internal/spacing.hpp and 4 (8 with
//                          kth) bytes are stored per point.  Never capped, no scratch beyond K17's.
//   spacing_rows_kernel    route 2.  One lane per row of k + 1 records the handle's own search returned: drop_self_row's
//                          rule and then the same reduction.
//   spacing_level0_kernel  level 0 of align_step's summation tree over x_i (DEV == false) or over the squared deviations
//                          (DEV == true: the mean is read from the record the first finish wrote).  One wavefront per block
//                          of 256 entries, the butterfly of ptk_kernels_align.hpp.  The upper levels are
//                          align_reduce_kernel's with one term.
//   spacing_finish_kernel  one lane: the first or the second half of the 64-byte record, plain 8-byte stores.
//   spacing_keep_kernel    elementwise: the keep test from mean[i] and the record.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pico_tree/internal/spacing.hpp"
#include "ptk_kernels_align.hpp"
#include "ptk_kernels_f64.hpp"

namespace ptk {

namespace sp = pico_tree::internal;

// Route 1 (the prologue and the drop slot are knn_self_kernel's, ptk_kernels.hpp).  `kth` may be null.
template <int K, int S, int OVF, int BLOCK, int LEAFB, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) PTK_KNN_REG_WAVES void spacing_self_kernel(
    DevTree t, uint32_t dim, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, float* __restrict__ mean,
    float* __restrict__ kth) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const int32_t self = (int32_t)__float_as_uint(rec.w);
  pad_query<M>(dim, qy, qz);
  Record spill[OVF > 0 ? OVF : 1];
  Stack<S, OVF, BLOCK> st;
  st.init((LdsWord*)ptk_smem, threadIdx.x, spill);
  KnnRegPolicy<K> pol;
  pol.init(k + 1u, 1.0f);
  traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
  // The k + 1 entries are slots K - 1 - k .. K - 1; slot j of the row is list slot j, or j + 1 from the dropped entry on.
  const uint32_t lo = (uint32_t)K - 1u - k;
  uint32_t drop = (uint32_t)K - 1u;
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {
    if ((uint32_t)j >= lo && pol.li[j] == self && pol.ld[j] < 3.402823466e+38f) drop = (uint32_t)j;
  }
  const bool root = (flags & sp::spacing_sqrt) != 0u;
  sp::spacing_fold<float> fold;
#pragma unroll
  for (int j = 0; j < K - 1; ++j) {
    if ((uint32_t)j >= lo) fold.add((uint32_t)j >= drop ? pol.ld[j + 1] : pol.ld[j], root);
  }
  mean[(uint32_t)self] = fold.mean();
  if (kth != nullptr) kth[(uint32_t)self] = fold.kth;
}

// Route 2: row i of `rows` (k + 1 records, the search's) belongs to leaf position first + i, whose index is the record's
// fourth word or index[first + i].  The entry that leaves is drop_self_row's: the first accepted one whose index is the
// row's, else the last.
template <class Nb, class Real>
__global__ __launch_bounds__(256) void spacing_rows_kernel(
    const Nb* __restrict__ rows, const float4* __restrict__ recs, const int32_t* __restrict__ index, uint64_t first,
    uint64_t n, uint32_t k, uint32_t flags, Real* __restrict__ mean, Real* __restrict__ kth) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int32_t self = recs != nullptr ? (int32_t)__float_as_uint(recs[first + i].w) : index[first + i];
  const Nb* __restrict__ src = rows + i * ((uint64_t)k + 1u);
  const Real fmax = sp::spacing_fold<Real>::fmax();
  uint32_t drop = k;
  for (uint32_t j = 0; j < k; ++j) {
    const Nb nb = src[j];
    if (drop == k && nb.index == self && nb.distance < fmax) drop = j;
  }
  Real m, kd;
  sp::spacing_row<Real>([&](uint32_t j) { return src[j < drop ? j : j + 1u].distance; }, k, (flags & sp::spacing_sqrt) != 0u,
                        &m, &kd);
  mean[(uint32_t)self] = m;
  if (kth != nullptr) kth[(uint32_t)self] = kd;
}

// Level 0 of a sum of the record over the n means.  counts[block]: the valid entries of the block.
template <class Real, bool DEV>
PTK_GLOBAL __launch_bounds__(64) void spacing_level0_kernel(const Real* __restrict__ mean, uint64_t n,
                                                            const sp::spacing_stats* __restrict__ stats, uint64_t blocks,
                                                            double* __restrict__ partials, uint64_t* __restrict__ counts) {
  const uint64_t block = blockIdx.x;
  if (block >= blocks) return;  // (wave-uniform)
  const uint32_t lane = threadIdx.x & 63u;
  double global_mean = 0.0;
  if constexpr (DEV) global_mean = stats->mean;
  double e[4];
  uint32_t valid = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t i = block * align::align_block + lane + 64u * r;
    e[r] = 0.0;
    if (i < n) {
      const Real v = mean[i];
      e[r] = DEV ? sp::spacing_deviation(v, global_mean) : sp::spacing_x(v);
      valid += sp::spacing_valid(v) ? 1u : 0u;
    }
  }
  const double v = align_butterfly(align::align_lane_fold(e[0], e[1], e[2], e[3]));
  const uint32_t c = align_butterfly_count(valid);
  if (lane == 0u) {
    partials[block] = v;
    counts[block] = c;
  }
}

// One lane.  second == 0: count, rows, sum, mean; else ssd, variance, ratio_squared, reserved (the mean and the count are
// read back from the record).
PTK_GLOBAL void spacing_finish_kernel(const double* __restrict__ reduced, const uint64_t* __restrict__ count, int second,
                                      uint64_t rows, float ratio, sp::spacing_stats* __restrict__ stats) {
  if (blockIdx.x != 0u || threadIdx.x != 0u) return;
  if (second == 0) {
    const uint64_t c = count[0];
    const double sum = reduced[0];
    stats->count = c;
    stats->rows = rows;
    stats->sum = sum;
    stats->mean = sp::spacing_mean_of(c, sum);
  } else {
    const double ssd = reduced[0];
    stats->ssd = ssd;
    stats->variance = sp::spacing_variance_of(stats->count, ssd);
    stats->ratio_squared = sp::spacing_ratio_squared(ratio);
    stats->reserved = 0.0;
  }
}

template <class Real>
PTK_GLOBAL __launch_bounds__(256) void spacing_keep_kernel(const Real* __restrict__ mean, uint64_t n,
                                                           const sp::spacing_stats* __restrict__ stats,
                                                           uint8_t* __restrict__ keep) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  keep[i] = sp::spacing_keep(mean[i], stats->mean, stats->ratio_squared, stats->variance);
}

}  // namespace ptk
