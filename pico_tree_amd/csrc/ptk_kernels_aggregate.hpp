// ptk_kernels_aggregate.hpp -- aggregate_within_self / aggregate_within (ptk.h): the sum, minimum
// or maximum of a caller's per-point values over every row of the self radius search or of the per-row radius search,
// for float32 trees with dim <= 3 and the four non-topological metrics.
//
// One policy, two kernels.  AggregatePolicy<W, VEC> accumulates where the fill policies store: for every accepted point
// it loads values[idx * channels + c0 .. + w) and applies the op to W accumulators in registers, in the order traverse<>
// visits the row -- the reference's.  aggregate_self_kernel is radius_self_fill_kernel (ptk_kernels_selfr.hpp) with this
// policy: lane j of a launch is leaf-order record first + j, `self` comes from rec.w.  aggregate_within_kernel is
// radius_radii_fill_kernel (ptk_kernels_count.hpp) with it, self = -1, and a PER_ROW switch for the radius source.
// Neither shortcut of the count kernels is taken: the order of the sums is part of the contract.
//
// A call with channels > W runs one launch per window [c0, c0 + w), w <= W; every window traverses again.  The last
// window's width is the run-time bound `w` (predicated loads and stores), not an instantiation of its own.  `op` and
// INCLUDE_SELF are kernel arguments: a wave-uniform branch at the accept.  VEC (chosen on the host: channels % 4 == 0,
// c0 % 4 == 0, `values` and `out` 16-byte aligned) reads and writes the window as float4; both paths give the same bits.
//
// The accumulation is the contract's, one IEEE float32 operation each (the units are compiled with -ffp-contract=off):
//   SUM  acc = acc + v          MAX  acc = (v > acc) ? v : acc          MIN  acc = (v < acc) ? v : acc
// The compare-selects are written out: v_max_f32 / fmaxf would drop a NaN accumulator (INCLUDE_SELF with a NaN own value).
#pragma once

#include <algorithm>

#include "ptk_dispatch.hpp"
#include "ptk_kernels_count.hpp"

// The kernels are held to the 64 vector registers of the fill and frames kernels they are modelled on (8 wavefronts per
// SIMD): left alone the compiler takes 67 at W = 8 and loses a wavefront; held, it fits them with no private-segment
// bytes beyond the record stack's (profiles/aggregate_resources.txt).
#if defined(__HIPCC__)
#define PTK_AGG_WAVES __attribute__((amdgpu_waves_per_eu(8)))
#else
#define PTK_AGG_WAVES
#endif

namespace ptk {

constexpr uint32_t kAggSum = 0u, kAggMin = 1u, kAggMax = 2u;  // PTK_AGG_* (ptk.h)
constexpr uint32_t kAggOpMask = 0xFFu, kAggIncludeSelf = 0x100u;
constexpr uint32_t kAggMaxChannels = 1024u;
// The accumulators a lane holds: the widest window of {4, 8, 16} whose kernels keep the private segment and the occupancy
// of frames_self_kernel (profiles/aggregate_resources.txt).  One width is compiled.
constexpr int kAggWidth = 8;

// The vector path of a window (checked on the host at the call).
inline bool aggregate_vector_path(const void* values, const void* out, uint32_t channels, uint32_t c0) {
  return channels % 4u == 0u && c0 % 4u == 0u && reinterpret_cast<uintptr_t>(values) % 16u == 0u &&
         reinterpret_cast<uintptr_t>(out) % 16u == 0u;
}

__device__ __forceinline__ float aggregate_identity(uint32_t op) {
  return __uint_as_float(op == kAggSum ? 0u : (op == kAggMax ? 0xFF800000u : 0x7F800000u));  // +0, -inf, +inf
}

// The channel windows of a call: f(int_tag<W>, bool tag VEC, c0, w) for [c0, c0 + w) = [0, W), [W, 2 W) ... in order; the
// first status that is not 0 ends the call.
template <class F>
int aggregate_windows(const void* values, const void* out, uint32_t channels, F&& f) {
  for (uint32_t c0 = 0; c0 < channels; c0 += (uint32_t)kAggWidth) {
    const uint32_t w = std::min<uint32_t>((uint32_t)kAggWidth, channels - c0);
    const int rc = ptkd::with_bool(aggregate_vector_path(values, out, channels, c0),
                                   [&](auto VEC) { return f(ptkd::int_tag<kAggWidth>{}, VEC, c0, w); });
    if (rc != 0) return rc;
  }
  return 0;
}

// v[0 .. W) = row[0 .. w), +0 beyond w.  VEC: w is a multiple of 4 and row is 16-byte aligned.
template <int W, bool VEC>
__device__ __forceinline__ void aggregate_load(const float* __restrict__ row, uint32_t w, float (&v)[W]) {
  if constexpr (VEC) {
    static_assert(W % 4 == 0, "whole float4 words");
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
      float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if ((uint32_t)(4 * k) < w) x = reinterpret_cast<const float4*>(row)[k];
      v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = (uint32_t)c < w ? row[c] : 0.0f;
  }
}

template <int W, bool VEC>
__device__ __forceinline__ void aggregate_store(float* __restrict__ row, uint32_t w, const float (&v)[W]) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < W / 4; ++k)
      if ((uint32_t)(4 * k) < w) reinterpret_cast<float4*>(row)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  } else {
#pragma unroll
    for (int c = 0; c < W; ++c)
      if ((uint32_t)c < w) row[c] = v[c];
  }
}

// RadiusSelfFillPolicy with the row store replaced by the op over the window of the accepted point's values.  An
// accumulator beyond w takes +0s and is never stored.
template <int W, bool VEC>
struct AggregatePolicy {
  float radius;
  int32_t self;  // -1: a query row (no own entry)
  uint32_t op;   // kAggSum / kAggMin / kAggMax, the same in every lane
  uint32_t w;
  uint64_t channels;
  const float* __restrict__ values;  // + c0
  uint64_t count;
  float acc[W];
  __device__ __forceinline__ float max() const { return radius; }
  __device__ __forceinline__ void start(uint32_t include_self, uint64_t own) {
    count = 0;
    if (include_self) {
      aggregate_load<W, VEC>(values + own * channels, w, acc);
    } else {
      const float id = aggregate_identity(op);
#pragma unroll
      for (int c = 0; c < W; ++c) acc[c] = id;
    }
  }
  __device__ __forceinline__ void visit(int32_t idx, float d) {
    if (radius > d && idx != self) {  // strict
      ++count;
      float v[W];
      aggregate_load<W, VEC>(values + (uint64_t)(uint32_t)idx * channels, w, v);
      if (op == kAggSum) {
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] = acc[c] + v[c];
      } else if (op == kAggMax) {
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] = (v[c] > acc[c]) ? v[c] : acc[c];
      } else {
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] = (v[c] < acc[c]) ? v[c] : acc[c];
      }
    }
  }
};

// out[self][c0 .. c0 + w) and, in the window c0 == 0, counts[self] (may be null) of the points at leaf positions
// [first, first + n).  `flags`: the op, | kAggIncludeSelf.  A NaN or negative per-row radius gives the empty row: the
// identity (or the own value) and count 0.
template <int W, bool VEC, int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) PTK_AGG_WAVES void aggregate_self_kernel(
    DevTree t, uint32_t dim, uint64_t first, uint64_t n, float radius_all, const float* __restrict__ radii,
    const float* __restrict__ values, uint32_t channels, uint32_t c0, uint32_t w, uint32_t flags, float* __restrict__ out,
    uint64_t* __restrict__ counts) {
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

  AggregatePolicy<W, VEC> pol;
  pol.radius = radius;
  pol.self = (int32_t)self;
  pol.op = flags & kAggOpMask;
  pol.w = w;
  pol.channels = channels;
  pol.values = values + c0;
  pol.start(flags & kAggIncludeSelf, self);
  if (radius >= 0.0f) {
    PTK_STACK(S, OVF, BLOCK, st, t);
    traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
  }
  aggregate_store<W, VEC>(out + (uint64_t)self * channels + c0, w, pol.acc);
  if (c0 == 0u && counts != nullptr) counts[self] = pol.count;
}

// The same of the query rows: launch position i is row qi = perm[i] (perm null: i) of `queries`, written at out[qi] in the
// caller's order; the radius is radii[qi] (PER_ROW) or radius_all.
template <int W, bool VEC, int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) PTK_AGG_WAVES void aggregate_within_kernel(
    DevTree t, const float* __restrict__ queries, uint32_t dim, const uint32_t* __restrict__ perm, uint64_t nq,
    float radius_all, const float* __restrict__ radii, const float* __restrict__ values, uint32_t channels, uint32_t c0,
    uint32_t w, uint32_t flags, float* __restrict__ out, uint64_t* __restrict__ counts) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= nq) return;
  const uint64_t qi = perm ? perm[i] : i;
  const float radius = PER_ROW ? radii[qi] : radius_all;  // (the row in the caller's order, not the launch position)
  float qx, qy, qz;
  load_query(queries, dim, qi, qx, qy, qz);
  pad_query<M>(dim, qy, qz);

  AggregatePolicy<W, VEC> pol;
  pol.radius = radius;
  pol.self = -1;
  pol.op = flags & kAggOpMask;
  pol.w = w;
  pol.channels = channels;
  pol.values = values + c0;
  pol.start(0u, 0u);
  if (radius >= 0.0f) {
    PTK_STACK(S, OVF, BLOCK, st, t);
    traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
  }
  aggregate_store<W, VEC>(out + qi * channels + c0, w, pol.acc);
  if (c0 == 0u && counts != nullptr) counts[qi] = pol.count;
}

}  // namespace ptk
