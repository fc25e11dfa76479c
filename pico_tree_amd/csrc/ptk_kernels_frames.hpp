// ptk_kernels_frames.hpp -- normals_within_self (ptk.h): the moments of every tree point's
// neighbourhood and the local frame of their covariance, for 3-D float32 trees and the four non-topological metrics.
//
// frames_self_kernel is radius_self_fill_kernel (ptk_kernels_selfr.hpp) with a policy that accumulates where the fill
// policy stores: lane j of a launch is leaf-order record first + j, one aligned 16-byte load gives the query and its
// index `self`, traverse<> visits the row in the reference's order, and for every accepted point the policy adds the
// offset traverse<> has just computed (visit_at: dx, dy, dz = query - point, one float32 subtraction each) to nine
// accumulators in registers.  Neither shortcut of the count kernels is taken: the inside test swallows subtrees whose
// points would never be seen, and the order of the sums is part of the contract.  After the traversal the stack is dead;
// the lane computes the covariance and the frame with the routine the host shares
// (pico_tree/internal/local_frame.hpp) and writes its records at [self] with 16-byte stores.
#pragma once

#include "pico_tree/internal/local_frame.hpp"
#include "ptk_kernels_selfr.hpp"

namespace ptk {

namespace lf = pico_tree::internal;

// RadiusSelfFillPolicy with the row store replaced by the sums of the row.
struct MomentsPolicy {
  static constexpr bool kOffsetVisit = true;
  float radius;
  int32_t self;
  lf::moment_sums sums;
  __device__ __forceinline__ float max() const { return radius; }
  __device__ __forceinline__ void visit_at(int32_t idx, float d, float dx, float dy, float dz) {
    if (radius > d && idx != self) sums.add(dx, dy, dz);  // strict
  }
};

// One record as 16-byte words (the output arrays are 16-byte aligned: ptk.h).
template <class Rec>
__device__ __forceinline__ void store_record(Rec* __restrict__ out, uint32_t at, const Rec& rec) {
  static_assert(sizeof(Rec) % 16 == 0, "whole 16-byte words");
  uint4 w[sizeof(Rec) / 16];
  memcpy(w, &rec, sizeof(Rec));
  uint4* dst = reinterpret_cast<uint4*>(out + at);
#pragma unroll
  for (uint32_t k = 0; k < sizeof(Rec) / 16; ++k) dst[k] = w[k];
}

// frames[self] and moments[self] (either may be null) of the points at leaf positions [first, first + n).  A NaN or
// negative per-row radius gives the empty result: zero moments, a NaN frame, count 0.
template <int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void frames_self_kernel(
    DevTree t, uint32_t dim, uint64_t first, uint64_t n, float radius_all, const float* __restrict__ radii,
    uint64_t min_neighbors, uint32_t has_view, float vx, float vy, float vz, lf::frame3* __restrict__ frames,
    lf::moments3* __restrict__ moments) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const uint32_t self = __float_as_uint(rec.w);
  const float radius = PER_ROW ? radii[self] : radius_all;
  pad_query<M>(dim, qy, qz);

  MomentsPolicy pol;
  pol.radius = radius;
  pol.self = (int32_t)self;
  if (radius >= 0.0f) {
    PTK_STACK(S, OVF, BLOCK, st, t);
    traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
  }
  if (frames != nullptr)
    store_record(frames, self, lf::frame_of(pol.sums, min_neighbors, has_view != 0u, vx, vy, vz, qx, qy, qz));
  if (moments != nullptr) store_record(moments, self, pol.sums.record());
}

}  // namespace ptk
