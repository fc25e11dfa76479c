// ptk_kernels_suppress.hpp -- suppress_within_self (ptk.h): greedy radius suppression of a tree's
// own points -- Poisson-disk thinning in a fixed pseudo-random order, or non-maximum suppression under the caller's
// scores -- for the handles count_within_self serves (float32 and float64 trees with dim <= 3, the four non-topological
// metrics).  No rows are written: a lane walks its own row as radius_self_fill_kernel does and looks at one cell per hit.
//
// `cells` (uint8, n_points entries by ORIGINAL point index) is the caller's output and the only working array:
//   kSuppressOut 0   suppressed: the row holds a kept point of higher key
//   kSuppressKept 1  kept: every point of higher key in the row is suppressed
//   kSuppressOpen 2  undecided; exists only while the call runs
// suppress_init_kernel sets every cell to 2.  A ROUND is one lane per leaf-order record over ALL pieces of leaf
// positions; the host launches rounds until a round leaves no lane undecided (the counter of undecided lanes, one
// atomicAdd per wavefront).  A lane whose cell is not 2 leaves at once.  Otherwise it walks its row; for a hit idx != self
// with key(idx) > key(self) (pico_tree/internal/suppress.hpp: one statement of the key for host and device) it reads
// cells[idx]: a 1 suppresses the lane, a 2 blocks it.  After the walk a suppressed lane stores 0, a lane neither
// suppressed nor blocked stores 1, a lane that stays blocked counts itself and leaves its cell alone.
//
// Why the result does not depend on launch order, lane order, the pieces or what a load happens to see.
//   (1) A cell has ONE writer, the lane that owns the point, and it changes ONCE, from 2 to 0 or 1.  So a load returns
//       either the cell's final value or 2, never a value that is later taken back.
//   (2) keep[] of the contract is unique (well-founded by descending key).  Induction over descending key: suppose every
//       cell of higher key that is not 2 holds its contract value.  A lane stores 0 only after it has read a 1 in a cell
//       of higher key in its row -- by (1) and the hypothesis a kept point of the contract, so 0 is right.  It stores 1
//       only if every cell of higher key in its row read 0 -- all of them final and suppressed, so 1 is right.
//   (3) A STALE 2 (a load served from a line another XCD's L2 holds, or a lane that ran earlier in the same round) can
//       only turn "decide now" into "blocked": it delays, it never changes what is stored.  Reading a 1 early is as good
//       as reading it late: the walk may stop at the first 1, and whether it does changes nothing (results do not depend
//       on the early exit: the lane stores 0 either way).
//   (4) Progress.  The cells are read with relaxed agent-scope atomic loads and written with relaxed agent-scope atomic
//       stores (SuppressMem below: lanes on all eight XCDs read the array, and a plain load may come from a stale line of
//       the reader's own L2), and a kernel boundary orders everything before it.  So at the start of a round every cell
//       above the undecided point of highest key is final AND visible: that point is decided in the round.  At most
//       n_points rounds; the chain that needs them all is in ptk.h.
// No lane ever waits for a cell: a blocked lane leaves and is launched again in the next round.
//
// A NaN or negative per-row radius (the _device forms cannot look) passes no test: the row is empty, the lane stores 1 at
// once, and the point can still suppress others through THEIR rows.
//
// Byte cells, not a 32-bit scratch array with a final pack: a byte store is a store of one byte on this hardware (no
// read-modify-write of the word around it), the call then needs no scratch at all, and the array the rounds gather from
// is a quarter of the size (7.7 MB at the headline cloud: it stays in the MALL).
#pragma once

#include "pico_tree/internal/suppress.hpp"
#include "ptk_kernels_selfr.hpp"

namespace ptk {

constexpr uint8_t kSuppressOut = 0, kSuppressKept = 1, kSuppressOpen = 2;

struct SuppressMem {
  static __device__ __forceinline__ uint8_t load(const uint8_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void store(uint8_t* p, uint8_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The key of a point under the launch's order: SCORED gathers scores[i] (only ever called for the lane itself and for
// hits), the default order is arithmetic on i.
template <bool SCORED>
__device__ __forceinline__ uint64_t suppress_key_at(const float* __restrict__ scores, uint32_t i) {
  namespace in = pico_tree::internal;
  if constexpr (SCORED) return in::suppress_key(i, __float_as_uint(scores[i]));
  return in::suppress_key(i);
}

// The visitor of a round.  `cut` is what max() returns: the radius, until the lane is suppressed -- then -inf, so that
// every far child left is pruned and every leaf point left fails the test (count_self_kernel's clamp leaves the same way).
template <class Real, bool SCORED>
struct SuppressPolicy {
  Real cut;
  int32_t self;
  uint64_t key;
  bool out, blocked;
  const float* scores;
  const uint8_t* cells;
  __device__ __forceinline__ Real max() const { return cut; }
  __device__ __forceinline__ bool settled() const { return out; }
  __device__ __forceinline__ void visit(int32_t idx, Real d) {
    if (cut > d && idx != self) {  // strict
      if (suppress_key_at<SCORED>(scores, (uint32_t)idx) > key) {
        const uint8_t c = SuppressMem::load(cells + idx);
        if (c == kSuppressKept) {
          out = true;
          cut = -std::numeric_limits<Real>::infinity();
        } else if (c == kSuppressOpen) {
          blocked = true;
        }
      }
    }
  }
};

// After the walk: the one store of the lane's cell, or the lane's part in the counter of undecided lanes (the lanes of
// a wavefront that are still here vote; the first of the blocked ones adds their number).
template <class Policy>
__device__ __forceinline__ void suppress_finish(const Policy& pol, uint8_t* cells, uint32_t* undecided) {
  const bool open = !pol.out && pol.blocked;
  if (!open) SuppressMem::store(cells + pol.self, pol.out ? kSuppressOut : kSuppressKept);
  const unsigned long long votes = __ballot(open);
  if (open && (votes & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0ull) atomicAdd(undecided, (uint32_t)__popcll(votes));
}

static __global__ __launch_bounds__(256) void suppress_init_kernel(uint64_t n, uint8_t* __restrict__ cells) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) cells[i] = kSuppressOpen;
}

// ---- float32 trees (dim <= 3): one lane per leaf-order record, launched as cluster_link_kernel ------------------------
template <int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, bool SCORED, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void suppress_round_kernel(
    DevTree t, uint32_t dim, uint64_t first, uint64_t n, float radius_all, const float* __restrict__ radii,
    const float* __restrict__ scores, uint8_t* cells, uint32_t* undecided) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const uint32_t self = __float_as_uint(rec.w);
  if (SuppressMem::load(cells + self) != kSuppressOpen) return;  // decided in an earlier round
  const float radius = PER_ROW ? radii[self] : radius_all;
  SuppressPolicy<float, SCORED> pol;
  pol.cut = radius;
  pol.self = (int32_t)self;
  pol.key = 0;
  pol.out = pol.blocked = false;
  pol.scores = scores;
  pol.cells = cells;
  if (radius >= 0.0f) {  // (else an empty row: kept)
    pol.key = suppress_key_at<SCORED>(scores, self);
    pad_query<M>(dim, qy, qz);
    PTK_STACK(S, OVF, BLOCK, st, t);
    traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
  }
  suppress_finish(pol, cells, undecided);
}

// ---- float64 trees (dim <= 3): the same kernel over DevTree64 / Stack64, as cluster64_link_kernel ----------------------
template <class M, bool PER_ROW, bool SCORED>
__global__ __launch_bounds__(64) void suppress64_round_kernel(
    DevTree64 t, uint64_t first, uint64_t n, double radius_all, const double* __restrict__ radii,
    const float* __restrict__ scores, uint8_t* cells, uint32_t* undecided, Rec64* __restrict__ stack, uint32_t slots) {
  const uint64_t i = (uint64_t)xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral) * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t dim = t.dim;
  const double4 rec = *reinterpret_cast<const double4*>(t.pts + (first + i) * kStride64D3);
  const uint32_t self = (uint32_t)__double_as_longlong(rec.w);
  if (SuppressMem::load(cells + self) != kSuppressOpen) return;
  const double radius = PER_ROW ? radii[self] : radius_all;
  SuppressPolicy<double, SCORED> pol;
  pol.cut = radius;
  pol.self = (int32_t)self;
  pol.key = 0;
  pol.out = pol.blocked = false;
  pol.scores = scores;
  pol.cells = cells;
  if (radius >= 0.0) {
    pol.key = suppress_key_at<SCORED>(scores, self);
    const double qy = dim > 1 ? rec.y : metric64_pad<M>();
    const double qz = dim > 2 ? rec.z : metric64_pad<M>();
    Stack64 st;
    st.init(0, 0, stack, slots);
    traverse64_3<M>(t, rec.x, qy, qz, pol, st);
  }
  suppress_finish(pol, cells, undecided);
}

}  // namespace ptk
