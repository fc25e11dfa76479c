// ptk_kernels_cluster.hpp -- cluster_within_self (ptk.h): the connected components of the
// fixed-radius graph over a tree's own points, with DBSCAN's core-point rule, for the handles count_within_self serves
// (3-D float32 and float64 trees, the four non-topological metrics).  No rows are written: the pairs the kernels of
// ptk_kernels_selfr.hpp visit are linked in a lock-free union-find (ptk_union_find.hpp) whose parents ARE the output.
//
// `labels` (int32, n_points entries by ORIGINAL point index) is the only working array.  The passes, each over ALL
// pieces of leaf positions before the next one starts (one stream orders them):
//   1 mark     min_neighbors == 0: labels[i] = i (cluster_init_kernel).  Else count_self_kernel with
//              max_count = min_neighbors and ClusterMarkStore: labels[self] = self when the count reached min_neighbors
//              (core), kClusterNonCore otherwise.  The clamp is the early exit; the inside shortcut counts as ever.
//   2 link     a core lane walks its own row (traverse<>: every neighbour has to be seen, no shortcut) and unites itself
//              with every core point in it.  One direction suffices: i -- j whenever j is in row i OR i is in row j.
//   3 flatten  core i: labels[i] = find(i), the smallest index of its component (cluster_flatten_kernel).
//   4 border   a non-core lane walks its own row and takes the smallest label among the core points in it.  The result
//              stays NEGATIVE for the whole pass (kClusterBorderBase - label; noise keeps kClusterNonCore): another
//              border lane that tests labels[idx] >= 0 for "core" can never take a border point for one.
//   5 decode   kClusterBorderBase - v for v <= kClusterBorderBase (cluster_decode_kernel).
// With min_neighbors == 0 every point is core: passes 4 and 5 have nothing to do and are not launched.
// A NaN or negative per-row radius (the _device forms cannot look) passes no test: the count is 0 and the link and
// border lanes leave at once -- the point is its own cluster at min_neighbors == 0, non-core otherwise, and still
// another point's neighbour.
//
// Every read of a parent in passes 2 and 3 is a relaxed agent-scope atomic load (lanes on all XCDs link the same array;
// a plain load may come from a stale line), every write an atomicCAS / atomicMin: ClusterMem below.
#pragma once

#include "ptk_kernels_selfr.hpp"
#include "ptk_union_find.hpp"

namespace ptk {

constexpr int32_t kClusterNonCore = -1;     // pass 1's mark of a non-core point; what noise keeps
constexpr int32_t kClusterBorderBase = -2;  // pass 4 stores kClusterBorderBase - label

struct ClusterMem {
  static __device__ __forceinline__ int32_t load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ int32_t cas(int32_t* p, int32_t expected, int32_t wanted) {
    return atomicCAS(p, expected, wanted);
  }
  static __device__ __forceinline__ int32_t min(int32_t* p, int32_t v) { return atomicMin(p, v); }
};

// Pass 1 behind count_self_kernel / count64_self_kernel (max_count = min_neighbors > 0).
struct ClusterMarkStore {
  using cell = int32_t;
  static __device__ __forceinline__ void put(cell* __restrict__ out, uint32_t self, uint64_t count, uint64_t min_neighbors) {
    out[self] = count >= min_neighbors ? (int32_t)self : kClusterNonCore;
  }
};

// Pass 2: unites the lane's point with every core point of its row.  `at`: a cell of the lane's own component, as low
// as the lane has seen (where its next find starts).  The one load that tells whether idx is core is idx's parent as
// well: a parent that IS `at` says "same component already" without a find (the common case once the trees are flat),
// and any other parent is where idx's find starts.
template <class Real, bool COMPRESS>
struct ClusterLinkPolicy {
  Real radius;
  int32_t self, at;
  int32_t* labels;
  __device__ __forceinline__ Real max() const { return radius; }
  __device__ __forceinline__ void visit(int32_t idx, Real d) {
    if (radius > d && idx != self) {  // strict
      const int32_t p = ClusterMem::load(labels + idx);
      if (p >= 0 && p != at) at = uf_unite<ClusterMem, COMPRESS>(labels, at, p);  // core; not known to be joined
    }
  }
};

// Pass 4: the smallest label among the core points of the row (labels of core points are final since pass 3; every
// other entry is negative before, during and after this pass).
template <class Real>
struct ClusterBorderPolicy {
  Real radius;
  int32_t self, best;
  const int32_t* labels;
  __device__ __forceinline__ Real max() const { return radius; }
  __device__ __forceinline__ void visit(int32_t idx, Real d) {
    if (radius > d && idx != self) {  // strict
      const int32_t l = labels[idx];
      best = l >= 0 && l < best ? l : best;
    }
  }
};
constexpr int32_t kClusterNoLabel = 0x7FFFFFFF;

__device__ __forceinline__ int32_t cluster_border_value(int32_t best) {
  return best == kClusterNoLabel ? kClusterNonCore : kClusterBorderBase - best;
}

// ---- the elementwise passes, over original indices ---------------------------------------------------------------------
static __global__ __launch_bounds__(256) void cluster_init_kernel(uint64_t n, int32_t* __restrict__ labels) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) labels[i] = (int32_t)i;
}

template <bool COMPRESS>
__global__ __launch_bounds__(256) void cluster_flatten_kernel(uint64_t n, int32_t* labels) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t p = ClusterMem::load(labels + i);
  if (p < 0 || p == (int32_t)i) return;  // non-core; a root
  const int32_t root = uf_find<ClusterMem, COMPRESS>(labels, p);
  if (root != p) (void)ClusterMem::min(labels + i, root);
}

static __global__ __launch_bounds__(256) void cluster_decode_kernel(uint64_t n, int32_t* __restrict__ labels) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t v = labels[i];
  if (v <= kClusterBorderBase) labels[i] = kClusterBorderBase - v;
}

// ---- float32 trees (dim <= 3): one lane per leaf-order record, as radius_self_fill_kernel -------------------------------
template <int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, bool COMPRESS, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void cluster_link_kernel(
    DevTree t, uint32_t dim, uint64_t first, uint64_t n, float radius_all, const float* __restrict__ radii, int32_t* labels) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const uint32_t self = __float_as_uint(rec.w);
  const float radius = PER_ROW ? radii[self] : radius_all;
  if (!(radius >= 0.0f) || ClusterMem::load(labels + self) < 0) return;  // an empty row; not core
  pad_query<M>(dim, qy, qz);

  PTK_STACK(S, OVF, BLOCK, st, t);
  ClusterLinkPolicy<float, COMPRESS> pol;
  pol.radius = radius;
  pol.self = pol.at = (int32_t)self;
  pol.labels = labels;
  traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
}

template <int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void cluster_border_kernel(
    DevTree t, uint32_t dim, uint64_t first, uint64_t n, float radius_all, const float* __restrict__ radii, int32_t* labels) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const uint32_t self = __float_as_uint(rec.w);
  const float radius = PER_ROW ? radii[self] : radius_all;
  if (!(radius >= 0.0f) || labels[self] >= 0) return;  // an empty row: noise, as marked; core
  pad_query<M>(dim, qy, qz);

  PTK_STACK(S, OVF, BLOCK, st, t);
  ClusterBorderPolicy<float> pol;
  pol.radius = radius;
  pol.self = (int32_t)self;
  pol.best = kClusterNoLabel;
  pol.labels = labels;
  traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
  labels[self] = cluster_border_value(pol.best);
}

// ---- float64 trees (dim <= 3): the same two kernels over DevTree64 / Stack64, as radius64_self_fill_kernel -------------
template <class M, bool PER_ROW, bool COMPRESS>
__global__ __launch_bounds__(64) void cluster64_link_kernel(
    DevTree64 t, uint64_t first, uint64_t n, double radius_all, const double* __restrict__ radii, int32_t* labels,
    Rec64* __restrict__ stack, uint32_t slots) {
  const uint64_t i = (uint64_t)xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral) * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t dim = t.dim;
  const double4 rec = *reinterpret_cast<const double4*>(t.pts + (first + i) * kStride64D3);
  const uint32_t self = (uint32_t)__double_as_longlong(rec.w);
  const double radius = PER_ROW ? radii[self] : radius_all;
  if (!(radius >= 0.0) || ClusterMem::load(labels + self) < 0) return;
  const double qy = dim > 1 ? rec.y : metric64_pad<M>();
  const double qz = dim > 2 ? rec.z : metric64_pad<M>();
  Stack64 st;
  st.init(0, 0, stack, slots);
  ClusterLinkPolicy<double, COMPRESS> pol;
  pol.radius = radius;
  pol.self = pol.at = (int32_t)self;
  pol.labels = labels;
  traverse64_3<M>(t, rec.x, qy, qz, pol, st);
}

template <class M, bool PER_ROW>
__global__ __launch_bounds__(64) void cluster64_border_kernel(
    DevTree64 t, uint64_t first, uint64_t n, double radius_all, const double* __restrict__ radii, int32_t* labels,
    Rec64* __restrict__ stack, uint32_t slots) {
  const uint64_t i = (uint64_t)xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral) * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t dim = t.dim;
  const double4 rec = *reinterpret_cast<const double4*>(t.pts + (first + i) * kStride64D3);
  const uint32_t self = (uint32_t)__double_as_longlong(rec.w);
  const double radius = PER_ROW ? radii[self] : radius_all;
  if (!(radius >= 0.0) || labels[self] >= 0) return;
  const double qy = dim > 1 ? rec.y : metric64_pad<M>();
  const double qz = dim > 2 ? rec.z : metric64_pad<M>();
  Stack64 st;
  st.init(0, 0, stack, slots);
  ClusterBorderPolicy<double> pol;
  pol.radius = radius;
  pol.self = (int32_t)self;
  pol.best = kClusterNoLabel;
  pol.labels = labels;
  traverse64_3<M>(t, rec.x, qy, qz, pol, st);
  labels[self] = cluster_border_value(pol.best);
}

}  // namespace ptk
