// ptk_kernels_align.hpp -- align_step (ptk.h): the normal equations of one ICP iteration from the
// rows of the k = 1 search, for float32 trees with dim == 3 under metric_l2_squared.
//
// Four kernels, none of which searches (the rows are ptk_search_knn_device's):
//   align_pose_kernel     q -> q' = R q + t, one row per lane, float32 as the contract reads
//   align_inverse_kernel  inv[bits(pts[i].w)] = i: the inverse of the leaf permutation, the handle's side table
//   align_terms_kernel    level 0 of the summation tree.  One wavefront takes one block of 256 consecutive rows; lane l
//                         owns rows l, l + 64, l + 128, l + 192 of it (coalesced loads of the rows and of q').  It reads
//                         the row, q', inv[index], pts[inv] and normals[index], forms the terms of the mode in double
//                         (pico_tree/internal/align.hpp: the same lines as the host loop), folds its four rows from +0 and
//                         reduces across the lanes with the butterfly of the contract.  At most 29 double accumulators
//                         and the count.  Lane 0 writes the block's partial: term j of block b at partials[j * blocks + b]
//                         (struct of arrays: the next level reads consecutive doubles).
//   align_reduce_kernel   the upper levels: the same shape over the partials of the level below, term by term
//   align_finish_kernel   the 384-byte record from the last level's single entry per term: 48 lanes, one 8-byte store each
//
// The butterfly.  v[l] = v[l] + v[l + s] for s = 32 .. 1 needs the value of lane l + s: a 64-bit operand crossing rows of
// 16 lanes and, at s = 32, the halves of the wavefront.  It is written with __shfl (two ds_bpermute_b32 per double and
// step, no LDS allocation, no barrier): 29 terms x 6 steps x 2 = 348 permutes per 256 rows, beside 256 rows x 3 dependent
// random loads.  The kernel is bound by those loads, so the DPP forms were not worth a second statement
// of the reduction that the emulator could not run.  Lanes l >= s add an operand the contract does not name; only
// lane 0's value is kept.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pico_tree/internal/align.hpp"
#include "ptk_kernels.hpp"

namespace ptk {

namespace align = pico_tree::internal;

struct AlignPose {
  float m[12];
};

PTK_GLOBAL void align_pose_kernel(const float* __restrict__ q, uint64_t nq, AlignPose pose, float* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  float r[3];
  align::align_pose(pose.m, q[3 * i], q[3 * i + 1], q[3 * i + 2], r);
  out[3 * i] = r[0], out[3 * i + 1] = r[1], out[3 * i + 2] = r[2];
}

PTK_GLOBAL void align_inverse_kernel(const float4* __restrict__ pts, uint32_t n_points, uint32_t* __restrict__ inv) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_points) return;
  const uint32_t index = __float_as_uint(pts[i].w);
  if (index < n_points) inv[index] = (uint32_t)i;
}

// v of lane 0 = the butterfly of the contract over the 64 lanes' v.
__device__ __forceinline__ double align_butterfly(double v) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double other = __shfl(v, (lane + s) & 63);
    v = v + other;
  }
  return v;
}
__device__ __forceinline__ uint32_t align_butterfly_count(uint32_t v) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl((int)v, (lane + s) & 63);
  return v;
}

// Level 0.  One wavefront (= one workgroup of 64) per block of 256 rows; `blocks` of them.  (The bound of 64 threads
// lets the compiler keep the accumulators and the four rows in flight in registers: under the default bound of 1024 it
// stops at 128 VGPRs and spills -- profiles/align_resources.txt.)
template <bool PLANE>
PTK_GLOBAL __launch_bounds__(64) void align_terms_kernel(const Neighbor* __restrict__ rows, const float* __restrict__ q, uint64_t nq,
                                   const uint32_t* __restrict__ inv, const float4* __restrict__ pts, uint32_t n_points,
                                   const float* __restrict__ normals, float max_distance, uint64_t blocks,
                                   double* __restrict__ partials, uint64_t* __restrict__ counts) {
  constexpr int T = align::align_terms(PLANE);
  const uint64_t block = blockIdx.x;
  if (block >= blocks) return;  // (wave-uniform)
  const uint32_t lane = threadIdx.x & 63u;
  double acc[T];
#pragma unroll
  for (int j = 0; j < T; ++j) acc[j] = 0.0;
  uint32_t accepted = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t i = block * align::align_block + lane + 64u * r;
    double t[T];
#pragma unroll
    for (int j = 0; j < T; ++j) t[j] = 0.0;
    if (i < nq) {
      const Neighbor nb = rows[i];
      // (an accepted row's index is a tree point's: the pad {0, FLT_MAX} and every row the search did not fill fail the
      // test; the bound keeps a row that is not the search's from reading outside the tables)
      if (align::align_accept(nb.distance, max_distance) && (uint32_t)nb.index < n_points) {
        const float qi[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
        const uint32_t at = inv[(uint32_t)nb.index];
        if (at < n_points) {
          const float4 rec = pts[at];
          const float p[3] = {rec.x, rec.y, rec.z};
          if constexpr (PLANE) {
            const float* nrow = normals + 3 * (uint64_t)(uint32_t)nb.index;
            const float n[3] = {nrow[0], nrow[1], nrow[2]};
            if (align::align_finite(n[0]) && align::align_finite(n[1]) && align::align_finite(n[2])) {
              align::align_plane_row(qi, p, n, nb.distance, t);
              ++accepted;
            }
          } else {
            align::align_point_row(qi, p, nb.distance, t);
            ++accepted;
          }
        }
      }
    }
    // (((+0 + x[l]) + x[l + 64]) + x[l + 128]) + x[l + 192], one add per row
#pragma unroll
    for (int j = 0; j < T; ++j) acc[j] = acc[j] + t[j];
  }
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const double v = align_butterfly(acc[j]);
    if (lane == 0u) partials[(uint64_t)j * blocks + block] = v;
  }
  const uint32_t c = align_butterfly_count(accepted);
  if (lane == 0u) counts[block] = c;
}

// An upper level: `n_in` entries per term (term j at in + j * n_in) to `n_out` = ceil(n_in / 256) (term j at
// out + j * n_out); the counts likewise.  One wavefront per block of 256 entries, the terms one after the other.
PTK_GLOBAL __launch_bounds__(64) void align_reduce_kernel(const double* __restrict__ in, const uint64_t* __restrict__ counts_in, uint64_t n_in,
                                    int terms, uint64_t n_out, double* __restrict__ out, uint64_t* __restrict__ counts_out) {
  const uint64_t block = blockIdx.x;
  if (block >= n_out) return;  // (wave-uniform)
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t first = block * align::align_block + lane;
  for (int j = 0; j < terms; ++j) {
    const double* x = in + (uint64_t)j * n_in;
    double e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = first + 64u * r < n_in ? x[first + 64u * r] : 0.0;
    const double v = align_butterfly(align::align_lane_fold(e[0], e[1], e[2], e[3]));
    if (lane == 0u) out[(uint64_t)j * n_out + block] = v;
  }
  // (an integer sum: any order; a block holds at most 256 rows, so 32 bits hold a level-0 count and the sums are 64-bit)
  uint64_t c = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) c += first + 64u * r < n_in ? counts_in[first + 64u * r] : 0u;
  const int l = (int)lane;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)c, (l + s) & 63);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(c >> 32), (l + s) & 63);
    c += ((uint64_t)hi << 32) | lo;
  }
  if (lane == 0u) counts_out[block] = c;
}

// The record: 48 words of 8 bytes, one lane and one plain store each.  `reduced`: one entry per term (null: nq == 0, all
// sums +0); `count`: one entry.
PTK_GLOBAL void align_finish_kernel(const double* __restrict__ reduced, const uint64_t* __restrict__ count, int plane,
                                    uint64_t nq, unsigned long long* __restrict__ out) {
  const uint32_t w = threadIdx.x;
  if (w >= 48u) return;
  unsigned long long word = 0ull;  // (+0.0)
  if (w == 0u) {
    word = reduced != nullptr ? count[0] : 0ull;
  } else if (w == 1u) {
    word = nq;
  } else if (reduced != nullptr) {
    const int slot = (int)w - 2;
    const int terms = align::align_terms(plane != 0);
    for (int j = 0; j < terms; ++j)
      if (align::align_slot(plane != 0, j) == slot) word = (unsigned long long)__double_as_longlong(reduced[j]);
  }
  out[w] = word;
}

}  // namespace ptk
