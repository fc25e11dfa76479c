// ptk_kernels_mst.hpp -- mst_within_self (ptk.h): the minimum spanning forest of the fixed-radius
// graph over a tree's own points, by Boruvka rounds, for float32 trees with dim <= 3 under metric_l2_squared and
// metric_l1 (the metrics whose box distance is a lower bound of the point distance).  No rows are written.
//
// Working arrays, all by ORIGINAL point index unless said otherwise (the caller's workspace, ptkf::MstLayout):
//   parent   int32   the lock-free union-find of ptk_union_find.hpp: the root of a set is its smallest index
//   label    int32   label[i] = the root of i as the LAST relabel pass found it: fixed while a round's search runs
//   cand     uint2   {bits(w), j}: the lane's best edge to another component this round, {kMstNone, kMstNone} without
//   best_wlo uint64  per component (at its label): the minimum of (bits(w) << 32) | lo over its lanes' candidates
//   best_hi  uint32  per component: the minimum hi among the candidates that match best_wlo
//   comp     uint32  per BRANCH: the common label of every point of the subtree, kMstMixed if they differ
//   info, arrive     per branch: count_parents_kernel's parent links and arrival counters (ptk_kernels_count.hpp)
// A ROUND is six steps on one stream (the host: ptkf::mst_rounds):
//   1 table    mst_table_kernel: comp[] bottom-up, by the arrival climb of count_table_kernel, with its agent-scope loads
//              and stores and for its reason (an entry is handed from a lane on one XCD to a lane on another).
//   2 search   mst_search_kernel, one lane per leaf-order record, in pieces: the descent of count_self_kernel as a k = 1
//              search that ignores the lane's own component.  `cut` is the weight of the best candidate so far, `radius`
//              before the first: a PER-LANE value that only shrinks.  A candidate is a leaf record j with
//              label[j] != label[self], d < radius (row i's strict test) and w < radius; it replaces the best when its
//              triple (bits(w), lo, hi) is smaller (mst_less, pico_tree/internal/mst.hpp: the one statement of the order).
//              A far child is entered only if radius >= far_nbd -- the reference's test, so nothing outside row i is ever
//              seen -- AND cut + cut * 2^-10 >= max(far_nbd, core[self]): the margin and its argument are
//              knn1_coop_kernel's (a pruned subtree holds no point at a float distance <= cut); non-strict, because an
//              equal weight in another subtree can still win on (lo, hi).  Before the lane steps into a branch it is
//              skipped when comp[branch] is the lane's label (nothing in it is a candidate): every branch at `skip` 2,
//              the library's default -- testing the near children too costs a 4-byte read per level and halves the
//              call at 1 M points --, the root and every far child only at `skip` 1.  The root
//              and every far child are also skipped when the side table's box lies outside: the metric's own
//              accumulation `outside` is >= radius, or max(outside, core[self]) > cut.  No margin there: rounding is
//              monotone, so no point of the box has a float distance below `outside`.  The inside shortcut has no use.
//              The lane stores cand[self] and, with a candidate, does one 64-bit atomicMin into best_wlo[label[self]]
//              (after a look: a cell that is already smaller needs no atomic -- cells only ever shrink, so a stale
//              look costs an atomic and never loses one).
//   3 tie      mst_tie_kernel: a lane whose candidate matches best_wlo of its component does atomicMin(best_hi, hi).
//   4 emit     mst_emit_kernel: the lane whose candidate IS its component's (w, lo, hi) owns the edge: it links lo and hi
//              in the union-find and, IF ITS compare-and-swap made the link, takes a slot (atomicAdd) and writes the
//              record with plain vector stores.
//   5 relabel  mst_relabel_kernel: label[i] = find(i); the best_* cells are reset.
//   6 the host reads the number of edges the round added and ends the call at 0 (or at n_points - 1 edges in all).
// No lane waits for another anywhere.
//
// Why the edges are the minimum spanning forest (symmetric rows).  The triples are distinct, so the order is total and
// the forest unique.  (a) Cut property: step 2 gives every component C its minimum edge leaving C -- every graph edge
// {i, j} with i in C is in row i and the search sees everything in row i that could beat `cut` -- and the minimum edge
// leaving a set of vertices is in the unique forest.  (b) No cycle: suppose the chosen edges of one round closed a cycle
// through components C_1 .. C_k; take its largest edge e, chosen by C_a say.  The cycle leaves C_a by a second edge,
// smaller than e, which is an edge leaving C_a too -- so e was not C_a's minimum.  Hence the chosen edges form a
// forest over the components, every link of step 4 joins two sets that were apart (the one exception: two components
// that chose the SAME edge -- the second lane's unite finds them joined, or loses the compare-and-swap, and emits
// nothing), and every component with an edge leaving it is joined to another: the number of such components halves,
// at most ceil(log2 n) + 1 rounds.
// Where the rows are NOT symmetric (a tree read from a stream that does not belong to its points) a component sees only
// the edges in its own points' rows and (b) fails: the chosen edges may close a cycle.  That is why a record is written
// only by the lane whose compare-and-swap linked two sets: in the order the links happen each emitted edge joins two
// sets that were apart, so the records are a forest whatever the rows are, at most n_points - 1 of them; every record is an
// edge of the graph; a round with any candidate links at least once (the labels are exact roots when it starts), and a
// round without one means no row leaves its component: the labels are cluster_within_self's.  Minimality is not
// promised there (ptk.h).
// A NaN or negative core entry (the _device form cannot look) passes no test: the point has no edges.
#pragma once

#include "pico_tree/internal/mst.hpp"
#include "ptk_kernels_selfr.hpp"
#include "ptk_union_find.hpp"

namespace ptk {

constexpr uint32_t kMstNone = 0xFFFFFFFFu;   // cand: no candidate; best_*: no candidate in the component
constexpr uint32_t kMstMixed = 0xFFFFFFFFu;  // comp: the subtree holds points of several components
constexpr uint32_t kMstEmpty = 0xFFFFFFFEu;  // comp, while it is merged: no point seen yet
// Counters of the emulator (tests): subtrees skipped by comp[], by the box, and leaf records looked at.
constexpr uint32_t kMstStatComp = 0, kMstStatBox = 1, kMstStatScan = 2;

struct MstEdge {
  uint32_t lo, hi;
  float w;
};
static_assert(sizeof(MstEdge) == 12, "record layout");

// The union-find's cells: lanes on all XCDs link the same array (as ClusterMem, ptk_kernels_cluster.hpp).
struct MstMem {
  static __device__ __forceinline__ int32_t load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ int32_t cas(int32_t* p, int32_t expected, int32_t wanted) {
    return atomicCAS(p, expected, wanted);
  }
  static __device__ __forceinline__ int32_t min(int32_t* p, int32_t v) { return atomicMin(p, v); }
};
__device__ __forceinline__ unsigned long long mst_look(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// uf_unite that says whether THIS call made the link (the compare-and-swap that joined two sets was its own).
__device__ __forceinline__ bool mst_link(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find<MstMem, true>(parent, a);
    b = uf_find<MstMem, true>(parent, b);
    if (a == b) return false;
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const int32_t found = MstMem::cas(parent + hi, hi, lo);
    if (found == hi) return true;
    a = found;  // (hi is no root any more: `found` is where it points, below hi)
    b = lo;
  }
}

__device__ __forceinline__ uint32_t mst_merge(uint32_t a, uint32_t b) {
  return a == kMstEmpty ? b : (b == kMstEmpty ? a : (a == b ? a : kMstMixed));
}

// ---- the elementwise passes, over original indices ---------------------------------------------------------------------
static __global__ __launch_bounds__(256) void mst_init_kernel(uint64_t n, int32_t* __restrict__ parent,
                                                               int32_t* __restrict__ label,
                                                               unsigned long long* __restrict__ best_wlo,
                                                               uint32_t* __restrict__ best_hi, uint32_t* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *count = 0u;
  if (i >= n) return;
  parent[i] = (int32_t)i;
  label[i] = (int32_t)i;
  best_wlo[i] = ~0ull;
  best_hi[i] = kMstNone;
}

static __global__ __launch_bounds__(256) void mst_tie_kernel(uint64_t n, const uint2* __restrict__ cand,
                                                              const int32_t* __restrict__ label,
                                                              const unsigned long long* __restrict__ best_wlo,
                                                              uint32_t* best_hi) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint2 c = cand[i];
  if (c.y == kMstNone) return;
  const uint32_t self = (uint32_t)i, lo = self < c.y ? self : c.y, hi = self < c.y ? c.y : self;
  const int32_t l = label[i];
  if (pico_tree::internal::mst_wlo(c.x, lo) == best_wlo[l]) atomicMin(best_hi + l, hi);
}

static __global__ __launch_bounds__(256) void mst_emit_kernel(uint64_t n, const uint2* __restrict__ cand,
                                                               const int32_t* __restrict__ label,
                                                               const unsigned long long* __restrict__ best_wlo,
                                                               const uint32_t* __restrict__ best_hi, int32_t* parent,
                                                               MstEdge* __restrict__ edges, uint32_t capacity,
                                                               uint32_t* count, uint32_t* added) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint2 c = cand[i];
  if (c.y == kMstNone) return;
  const uint32_t self = (uint32_t)i, lo = self < c.y ? self : c.y, hi = self < c.y ? c.y : self;
  const int32_t l = label[i];
  if (pico_tree::internal::mst_wlo(c.x, lo) != best_wlo[l] || best_hi[l] != hi) return;  // not the component's edge
  if (!mst_link(parent, (int32_t)lo, (int32_t)hi)) return;  // the other component chose it too (or: rows not symmetric)
  const uint32_t slot = atomicAdd(count, 1u);
  if (slot < capacity) {  // (always: every record stands for a link, and n points take n - 1 links)
    MstEdge e;
    e.lo = lo;
    e.hi = hi;
    e.w = __uint_as_float(c.x);
    edges[slot] = e;
  }
  atomicAdd(added, 1u);
}

static __global__ __launch_bounds__(256) void mst_relabel_kernel(uint64_t n, int32_t* parent, int32_t* __restrict__ label,
                                                                  unsigned long long* __restrict__ best_wlo,
                                                                  uint32_t* __restrict__ best_hi) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  label[i] = uf_find<MstMem, true>(parent, (int32_t)i);
  best_wlo[i] = ~0ull;
  best_hi[i] = kMstNone;
}

// ---- step 1: the component table ------------------------------------------------------------------------------------------
// The entry of one child (a leaf: the labels of its records; a branch: its finished entry).
__device__ __forceinline__ uint32_t mst_child(const DevTree& t, const uint32_t* comp, const int32_t* __restrict__ label,
                                              uint32_t ref) {
  if (ref & kLeafBit) {
    const uint32_t lv = ref & 0x7FFFFFFFu;
    const uint32_t begin = lv >> t.cbits, count = lv & t.cmask;
    uint32_t v = kMstEmpty;
    for (uint32_t j = 0; j < count; ++j) v = mst_merge(v, (uint32_t)label[__float_as_uint(t.pts[begin + j].w)]);
    return v;
  }
  return table_load(comp + (ref & kBranchIdxMask));
}

// count_table_kernel's climb: a lane starts at a branch whose children are both leaves, writes its entry and climbs; at
// each parent the last of its branch children to arrive goes on.  `arrive` is zero when the kernel starts.
PTK_GLOBAL void mst_table_kernel(DevTree t, uint32_t n_branches, const uint32_t* __restrict__ info,
                                 uint32_t* __restrict__ arrive, const int32_t* __restrict__ label, uint32_t* comp) {
  const uint64_t b0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b0 >= n_branches) return;
  {
    const uint4 nd = t.nodes[b0];
    if (!(nd.z & kLeafBit) || !(nd.w & kLeafBit)) return;
  }
  uint32_t b = (uint32_t)b0;
  for (;;) {
    const uint4 nd = t.nodes[b];
    const uint32_t v = mst_merge(mst_child(t, comp, label, nd.z), mst_child(t, comp, label, nd.w));
    table_store(comp + b, v == kMstEmpty ? kMstMixed : v);
    const uint32_t p = info[b] & kBranchIdxMask;
    if (p == kCountNoParent) return;
    const uint4 pn = t.nodes[p];
    const uint32_t need = ((pn.z & kLeafBit) ? 0u : 1u) + ((pn.w & kLeafBit) ? 0u : 1u);
    device_fence();
    if (atomicAdd(&arrive[p], 1u) + 1u < need) return;
    device_fence();
    b = p;
  }
}

// ---- step 2: the search ---------------------------------------------------------------------------------------------------
// Leaf positions [first, first + n).  `table`, `comp`: null for a tree whose root is a leaf (no branch is ever met).
// `skip`: 0 the search without the component table (test hook mst_skip=0), 1 the root and every far child, 2 every near
// child as well (the default).  `stats` (the emulator only; null on the device): kMstStat*.
template <int S, int OVF, int BLOCK, int LEAFB, bool CORE, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void mst_search_kernel(
    DevTree t, const CountBox* __restrict__ table, const uint32_t* __restrict__ comp, uint32_t dim, uint64_t first,
    uint64_t n, float radius, const float* __restrict__ core, const int32_t* __restrict__ label, uint32_t skip,
    uint2* __restrict__ cand, unsigned long long* best_wlo, uint32_t* __restrict__ stats = nullptr) {
  namespace in = pico_tree::internal;
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const uint32_t self = __float_as_uint(rec.w);
  pad_query<M>(dim, qy, qz);
  const int32_t mine = label[self];
  const float core_self = CORE ? core[self] : 0.0f;
  const bool try_box = is_finite_f(qx) && (dim < 2 || is_finite_f(qy)) && (dim < 3 || is_finite_f(qz));

  // The best candidate so far, as its triple; `cut` its weight (the radius before the first) and `cutm` the far-child
  // bound cut + cut * 2^-10.
  unsigned long long b_wlo = ~0ull;
  uint32_t b_hi = kMstNone, b_j = kMstNone;
  float cut = radius;
  float cutm = f_add(cut, f_mul(cut, 0x1p-10f));

  PTK_STACK(S, OVF, BLOCK, st, t);
  const uint4* __restrict__ nodes = t.nodes;
  const float4* __restrict__ pts = t.pts;
  uint32_t ref = t.root_ref;
  float nbd = 0.0f, off0 = 0.0f, off1 = 0.0f, off2 = 0.0f;
  bool test = true;  // the root, then every far child as it is entered
  // (a NaN or negative core entry, or one not below the radius: no weight of this point is below the radius)
  const bool live = !CORE || (core_self >= 0.0f && core_self < radius);

  for (; live;) {
    while (!(ref & kLeafBit)) {
      const uint32_t idx = ref & kBranchIdxMask;
      const uint4 nd = nodes[idx];  // (issued with the table entries: one round trip for all)
      if ((test && skip != 0u) || skip >= 2u) {
        if (comp[idx] == (uint32_t)mine) {  // every point in there is of the lane's own component
          if (stats != nullptr) atomicAdd(&stats[kMstStatComp], 1u);
          test = false;
          ref = kLeafBit;  // (an empty leaf: on to the unwind)
          break;
        }
      }
      if (test) {
        test = false;
        if (try_box) {
          const CountBox bx = table[idx];
          const float lo[3] = {bx.lo.x, bx.lo.y, bx.lo.z}, hi[3] = {bx.hi.x, bx.hi.y, bx.hi.z};
          const float q[3] = {qx, qy, qz};
          bool finite_b = true;
          float outside = 0.0f;
#pragma unroll
          for (uint32_t a = 0; a < 3; ++a) {
            if (a < dim) {
              finite_b = finite_b && is_finite_f(lo[a]) && is_finite_f(hi[a]);
              const float dl = M::one(f_sub(lo[a], q[a])), dh = M::one(f_sub(hi[a], q[a]));
              const float s = (q[a] >= lo[a] && q[a] <= hi[a]) ? 0.0f : (dl < dh ? dl : dh);
              outside = a == 0 ? s : f_add(outside, s);  // (metric_l2_squared and metric_l1: a sum, as point_distance3)
            }
          }
          const float bound = CORE && core_self > outside ? core_self : outside;
          if (finite_b && (outside >= radius || bound > cut)) {
            if (stats != nullptr) atomicAdd(&stats[kMstStatBox], 1u);
            ref = kLeafBit;
            break;
          }
        }
      }
      const uint32_t axis = (ref >> 29) & 3u;
      const float left_max = __uint_as_float(nd.x);
      const float right_min = __uint_as_float(nd.y);
      const float v = sel3(axis, qx, qy, qz);
      const float s = f_sub(f_sub(f_add(left_max, right_min), v), v);
      const bool go_left = s > 0.0f;
      const float plane = go_left ? right_min : left_max;
      const float new_off = M::one(f_sub(plane, v));
      const float far_nbd = f_add(f_sub(nbd, sel3(axis, off0, off1, off2)), new_off);
      const float far_bound = CORE && core_self > far_nbd ? core_self : far_nbd;
      if (radius >= far_nbd && cutm >= far_bound) st.push(idx | (axis << 28) | (go_left ? kRecSide : 0u), far_nbd);
      ref = go_left ? nd.z : nd.w;
    }

    {  // the leaf, as count_self_kernel scans it
      const uint32_t lv = ref & 0x7FFFFFFFu;
      const uint32_t begin = lv >> t.cbits;
      const uint32_t cnt = lv & t.cmask;
      for (uint32_t j = 0; j < cnt; j += LEAFB) {
        float4 p[LEAFB];
#pragma unroll
        for (int u = 0; u < LEAFB; ++u) p[u] = pts[begin + j + u];
#pragma unroll
        for (int u = 0; u < LEAFB; ++u) {
          if (j + u < cnt) {
            PTK_KEEP4(p[u]);
            const float d = point_distance3<M>(f_sub(qx, p[u].x), f_sub(qy, p[u].y), f_sub(qz, p[u].z));
            if (stats != nullptr) atomicAdd(&stats[kMstStatScan], 1u);
            if (radius > d && d <= cut) {  // row i's strict test; w >= d, so d above the cut cannot win
              const uint32_t other = __float_as_uint(p[u].w);
              if (label[other] != mine) {  // (the own record is of the own component)
                float w = d;
                bool edge = true;
                if (CORE) {
                  const float core_other = core[other];
                  w = in::mst_weight(d, core_self, core_other);
                  edge = core_other >= 0.0f && w < radius;
                }
                const uint32_t lo = self < other ? self : other, hi = self < other ? other : self;
                const unsigned long long wlo = in::mst_wlo(__float_as_uint(w), lo);
                if (edge && in::mst_less(wlo, hi, b_wlo, b_hi)) {
                  b_wlo = wlo;
                  b_hi = hi;
                  b_j = other;
                  cut = w;
                  cutm = f_add(cut, f_mul(cut, 0x1p-10f));
                }
              }
            }
          }
        }
      }
    }

    // Back up to the next far child still worth entering (count_self_kernel's unwind, with the lane's shrinking cut).
    uint32_t enter_meta = 0;
    float enter_val = 0.0f;
    bool enter = false;
    {
      if (st.empty()) break;
      Record rr[decltype(st)::kUnwind];
      const int got = st.peek(rr);
      int used = 0;
#pragma unroll
      for (int k = 0; k < decltype(st)::kUnwind; ++k) {
        if (!enter && k < got) {
          used = k + 1;
          const float val = __uint_as_float(rr[k].y);
          if (rr[k].x & kRecUndo) {
            if (rr[k].x & kRecSide) {
              nbd = val;
            } else {
              const uint32_t axis = (rr[k].x >> 28) & 3u;
              off0 = axis == 0 ? val : off0;
              off1 = axis == 1 ? val : off1;
              off2 = axis == 2 ? val : off2;
            }
          } else if (radius >= val && cutm >= (CORE && core_self > val ? core_self : val)) {
            enter = true;
            enter_meta = rr[k].x;
            enter_val = val;
          }
        }
      }
      st.drop(used);
    }
    if (!enter) {
      if (st.empty()) break;
      ref = kLeafBit;
      continue;
    }
    const uint32_t idx = enter_meta & kRecIdxMask;
    const uint32_t axis = (enter_meta >> 28) & 3u;
    const bool far_is_right = (enter_meta & kRecSide) != 0;
    const uint4 nd = nodes[idx];
    const float plane = far_is_right ? __uint_as_float(nd.y) : __uint_as_float(nd.x);
    const float new_off = M::one(f_sub(plane, sel3(axis, qx, qy, qz)));
    st.push(kRecUndo | (axis << 28), sel3(axis, off0, off1, off2));
    st.push(kRecUndo | kRecSide, nbd);
    off0 = axis == 0 ? new_off : off0;
    off1 = axis == 1 ? new_off : off1;
    off2 = axis == 2 ? new_off : off2;
    nbd = enter_val;
    test = true;
    ref = far_is_right ? nd.w : nd.z;
  }

  cand[self] = make_uint2((uint32_t)(b_wlo >> 32), b_j);
  if (b_j != kMstNone) {
    unsigned long long* cell = best_wlo + mine;
    if (mst_look(cell) > b_wlo) atomicMin(cell, b_wlo);
  }
}

}  // namespace ptk
