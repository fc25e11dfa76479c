// ptk_kernels_selfr.hpp -- search_radius_self / count_within_self (ptk.h): the fixed-radius searches of
// every tree point among the OTHER points of the tree, for 3-D float32 trees (dim <= 3) and the four non-topological
// metrics.  Row i is the reference's search_radius(p_i, r_i) row without the entry whose index is i.
//
// Lane j of a launch is leaf-order record first + j of DevTree::pts, as knn_self_kernel takes it: one aligned 16-byte load
// gives the query and its index `self`; no query buffer, no batch order, no permutation.  The radius is the launch's one
// (PER_ROW = false) or radii[self], indexed by ORIGINAL point index (PER_ROW = true): both forms are the same code.
//
// count_self_kernel is count_within_kernel (ptk_kernels_count.hpp: the descent, the unwind, the outside and inside tests
// on the side table's boxes) with two changes:
//   (a) in a leaf scan a point counts only if it is below the radius AND its index word is not `self`;
//   (b) the inside shortcut is not taken for a branch whose box holds the lane's own point on every real axis
//       (lo_a <= q_a <= hi_a): there the descent goes on.
// Why (b) makes the count exact.  A table box holds every point of its subtree (count_table_kernel merges the points of
// the leaves bottom-up), so a subtree that contains the own record has a box that holds q: such a subtree is never
// swallowed whole, the descent through it goes on until a leaf scan meets the record, and (a) leaves it out there.  A
// subtree that IS swallowed whole has a box that does not hold q, hence does not contain the own record, and its size is
// the number of OTHER points below the radius in it.  Nothing is assumed about where the own record lies in relation to
// the splits: on a tree read from a stream that does not belong to its points the search of p_i may never reach the leaf
// that holds record i -- then the reference's row does not hold i either, nothing is removed, and neither (a) nor (b)
// fires for it.  The outside shortcut is unchanged: a skipped subtree contributes nothing with or without the own point.
// The price of (b): the branches on one root-to-leaf path (those whose boxes hold q) go without the inside test; the far
// children beside that path still take it.
// A NaN or negative per-row radius passes no test (every comparison with it is false or prunes): the count is 0, and the
// fill lane leaves before it touches the output.
#pragma once

#include "ptk_kernels_count.hpp"
#include "ptk_kernels_count64.hpp"

namespace ptk {

// A fourth counter of the emulator beside kCountStat*: inside tests refused because the box holds the lane's own point.
constexpr uint32_t kCountStatOwnBox = 3;

// Where a lane of the count kernels leaves its result: counts[self] = the clamped count.  (The mark pass of
// cluster_within_self, ptk_kernels_cluster.hpp, puts a core / non-core mark into its labels instead.)
struct CountSelfStore {
  using cell = uint64_t;
  static __device__ __forceinline__ void put(cell* __restrict__ out, uint32_t self, uint64_t count, uint64_t) { out[self] = count; }
};

// counts[self] = the points other than `self` below the radius, clamped to max_count (0: no limit) after the own point
// has left.  Leaf positions [first, first + n).  `stats` (the emulator only; null on the device): kCountStat*, kCountStatOwnBox.
template <int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, class M = MetricL2, class Out = CountSelfStore>
__global__ __launch_bounds__(BLOCK) void count_self_kernel(
    DevTree t, const CountBox* __restrict__ table, uint32_t dim, uint64_t first, uint64_t n, float radius_all,
    const float* __restrict__ radii, uint64_t max_count, uint32_t shortcut, typename Out::cell* __restrict__ counts,
    uint32_t* __restrict__ stats = nullptr) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const uint32_t self = __float_as_uint(rec.w);
  pad_query<M>(dim, qy, qz);
  const float radius = PER_ROW ? radii[self] : radius_all;
  // The shortcuts: a finite point (real axes), and for the inside test a radius that is not subnormal.
  const bool finite_q = is_finite_f(qx) && (dim < 2 || is_finite_f(qy)) && (dim < 3 || is_finite_f(qz));
  const bool try_box = shortcut != 0u && finite_q;
  const bool normal_r = radius == 0.0f || (__float_as_uint(radius) & 0x7F800000u) != 0u;
  const uint64_t limit = max_count != 0u ? max_count : ~0ull;

  PTK_STACK(S, OVF, BLOCK, st, t);
  const uint4* __restrict__ nodes = t.nodes;
  const float4* __restrict__ pts = t.pts;
  uint32_t ref = t.root_ref;
  float nbd = 0.0f, off0 = 0.0f, off1 = 0.0f, off2 = 0.0f;
  uint64_t count = 0;
  bool test = try_box;  // the root, then every far child as it is entered

  for (;;) {
    while (!(ref & kLeafBit)) {
      const uint32_t idx = ref & kBranchIdxMask;
      const uint4 nd = nodes[idx];  // (issued with the table entry: one round trip for both)
      if (test) {
        test = false;
        const CountBox bx = table[idx];
        const float lo[3] = {bx.lo.x, bx.lo.y, bx.lo.z}, hi[3] = {bx.hi.x, bx.hi.y, bx.hi.z};
        const float q[3] = {qx, qy, qz}, off[3] = {off0, off1, off2};
        bool finite_b = true, holds_q = true;
        float outside = 0.0f, inside = 0.0f;
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
          if (a < dim) {
            finite_b = finite_b && is_finite_f(lo[a]) && is_finite_f(hi[a]);
            const float dl = M::one(f_sub(lo[a], q[a])), dh = M::one(f_sub(hi[a], q[a]));
            const bool within = q[a] >= lo[a] && q[a] <= hi[a];
            holds_q = holds_q && within;
            const float s = within ? 0.0f : (dl < dh ? dl : dh);
            // (the metric's own accumulation: from the first axis, as point_distance3)
            outside = a == 0 ? s : (M::kMin ? (s < outside ? s : outside)
                                            : (std::is_same<M, MetricLInf>::value ? (outside < s ? s : outside) : f_add(outside, s)));
            const float ta = dl < dh ? dh : dl;
            const float u = ta < off[a] ? off[a] : ta;
            inside = a == 0 ? u : f_add(inside, u);
          }
        }
        if (finite_b) {
          if (outside >= radius) {
            if (stats != nullptr) atomicAdd(&stats[kCountStatOutside], 1u);
            ref = kLeafBit;  // (an empty leaf: on to the unwind)
            break;
          }
          if (is_finite_f(inside) && f_add(inside, f_mul(inside, 0x1p-10f)) < radius) {
            if (holds_q) {  // change (b): the own point may be in there
              if (stats != nullptr) atomicAdd(&stats[kCountStatOwnBox], 1u);
            } else if (normal_r) {
              if (stats != nullptr) atomicAdd(&stats[kCountStatInside], 1u);
              count += __float_as_uint(bx.lo.w);
              ref = kLeafBit;
              break;
            } else if (stats != nullptr) {
              atomicAdd(&stats[kCountStatSubnormal], 1u);
            }
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
      if (radius >= far_nbd) st.push(idx | (axis << 28) | (go_left ? kRecSide : 0u), far_nbd);
      ref = go_left ? nd.z : nd.w;
    }

    {  // the leaf, as radius_kernel scans it -- change (a): the own record does not count
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
            count += (radius > d && __float_as_uint(p[u].w) != self) ? 1u : 0u;  // strict
          }
        }
      }
    }
    if (count >= limit) break;

    // Back up to the next far child still worth entering (traverse<>'s unwind: one batch of kUnwind records per turn,
    // so that a lane with a long way back up does not hold the wavefront here).
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
          } else if (radius >= val) {  // search.hpp:99
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
    test = try_box;
    ref = far_is_right ? nd.w : nd.z;
  }
  Out::put(counts, self, count < limit ? count : limit, max_count);
}

// The fill policy of the self form: RadiusPolicy<kRadiusFill> at e = 1 that appends every accepted point but the lane's own.
struct RadiusSelfFillPolicy {
  float radius;
  int32_t self;
  uint64_t count;
  Neighbor* out;  // first record of this point's row
  __device__ __forceinline__ float max() const { return radius; }
  __device__ __forceinline__ void visit(int32_t idx, float d) {
    if (radius > d && idx != self) {  // strict
      Neighbor nb;
      nb.index = idx;
      nb.distance = d;
      out[count] = nb;
      ++count;
    }
  }
};

// The fill pass behind count_self_kernel(max_count = 0) and a scan of its counts: row `self` is written at
// out + offsets[self] in the reference's traversal order (traverse<>: neither shortcut is taken -- the order inside a
// subtree depends on the query).  A NaN or negative radius -- its count was 0 -- leaves before it touches `out`.
template <int S, int OVF, int BLOCK, int LEAFB, bool PER_ROW, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void radius_self_fill_kernel(
    DevTree t, uint32_t dim, uint64_t first, uint64_t n, float radius_all, const float* __restrict__ radii,
    const uint64_t* __restrict__ offsets, Neighbor* __restrict__ out) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 rec = t.pts[first + i];
  PTK_KEEP4(rec);
  const float qx = rec.x;
  float qy = rec.y, qz = rec.z;
  const uint32_t self = __float_as_uint(rec.w);
  const float radius = PER_ROW ? radii[self] : radius_all;
  if (!(radius >= 0.0f)) return;
  pad_query<M>(dim, qy, qz);

  PTK_STACK(S, OVF, BLOCK, st, t);
  RadiusSelfFillPolicy pol;
  pol.radius = radius;
  pol.self = (int32_t)self;
  pol.count = 0;
  pol.out = out + offsets[self];
  traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
}

// ---- float64 trees (dim <= 3): the same two kernels over the 32-byte {x, y, z, index} records of DevTree64 -------------
// count64_within_kernel (ptk_kernels_count64.hpp) with changes (a) and (b) of the header comment; launch-order entries
// are leaf positions [first, first + n), the record stacks those of a launch of n lanes (Stack64: blockIdx.x).  The
// tiles take the run length of the float32 kernels of this unit (kXcdRunGeneral): consecutive lanes are consecutive
// leaf positions in both precisions, and one run length per unit keeps xcd_runs the code it was for knn_self_kernel.
template <class M, bool PER_ROW, class Out = CountSelfStore>
__global__ __launch_bounds__(64) void count64_self_kernel(
    DevTree64 t, const CountBox64* __restrict__ table, uint64_t first, uint64_t n, double radius_all,
    const double* __restrict__ radii, uint64_t max_count, uint32_t shortcut, typename Out::cell* __restrict__ counts,
    Rec64* __restrict__ stack, uint32_t slots, uint32_t* __restrict__ stats = nullptr) {
  const uint64_t i = (uint64_t)xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral) * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t dim = t.dim;
  const double4 rec = *reinterpret_cast<const double4*>(t.pts + (first + i) * kStride64D3);
  const uint32_t self = (uint32_t)__double_as_longlong(rec.w);
  const double qx = rec.x;
  // (a missing axis: zero like the points' for sums and maxima, +inf for the minimum of metric_lninf)
  const double qy = dim > 1 ? rec.y : metric64_pad<M>();
  const double qz = dim > 2 ? rec.z : metric64_pad<M>();
  const double radius = PER_ROW ? radii[self] : radius_all;
  const bool finite_q = is_finite_d(qx) && (dim < 2 || is_finite_d(qy)) && (dim < 3 || is_finite_d(qz));
  const bool try_box = shortcut != 0u && finite_q;
  const bool normal_r = radius == 0.0 || (__double_as_longlong(radius) & 0x7FF0000000000000ll) != 0;
  const uint64_t limit = max_count != 0u ? max_count : ~0ull;

  Stack64 st;
  st.init(0, 0, stack, slots);
  const Node64* __restrict__ nodes = t.nodes;
  const double* __restrict__ pts = t.pts;
  const uint32_t last = t.n_points - 1;
  uint32_t ref = t.root_ref;
  double nbd = 0.0, o0 = 0.0, o1 = 0.0, o2 = 0.0;
  uint64_t count = 0;
  bool test = try_box;

  for (;;) {
    while (!(ref & kLeafBit)) {
      const Node64 nd = nodes[ref];
      if (test) {
        test = false;
        const CountBox64 bx = table[ref];
        const double lo[3] = {bx.lo.x, bx.lo.y, bx.lo.z}, hi[3] = {bx.hi.x, bx.hi.y, bx.hi.z};
        const double q[3] = {qx, qy, qz}, off[3] = {o0, o1, o2};
        bool finite_b = true, holds_q = true;
        double outside = 0.0, inside = 0.0;
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
          if (a < dim) {
            finite_b = finite_b && is_finite_d(lo[a]) && is_finite_d(hi[a]);
            const double dl = M::one(d_sub(lo[a], q[a])), dh = M::one(d_sub(hi[a], q[a]));
            const bool within = q[a] >= lo[a] && q[a] <= hi[a];
            holds_q = holds_q && within;
            const double s = within ? 0.0 : (dl < dh ? dl : dh);
            outside = a == 0 ? s : (M::kMin ? (s < outside ? s : outside)
                                            : (std::is_same<M, Metric64LInf>::value ? (outside < s ? s : outside) : d_add(outside, s)));
            const double ta = dl < dh ? dh : dl;
            const double u = ta < off[a] ? off[a] : ta;
            inside = a == 0 ? u : d_add(inside, u);
          }
        }
        if (finite_b) {
          if (outside >= radius) {
            if (stats != nullptr) atomicAdd(&stats[kCountStatOutside], 1u);
            ref = kLeafBit;
            break;
          }
          if (is_finite_d(inside) && d_add(inside, d_mul(inside, 0x1p-10)) < radius) {
            if (holds_q) {  // change (b): the own point may be in there
              if (stats != nullptr) atomicAdd(&stats[kCountStatOwnBox], 1u);
            } else if (normal_r) {
              if (stats != nullptr) atomicAdd(&stats[kCountStatInside], 1u);
              count += (uint64_t)__double_as_longlong(bx.lo.w);
              ref = kLeafBit;
              break;
            } else if (stats != nullptr) {
              atomicAdd(&stats[kCountStatSubnormal], 1u);
            }
          }
        }
      }
      const double v = sel3d(nd.axis, qx, qy, qz);
      const bool go_left = d_sub(d_sub(d_add(nd.left_max, nd.right_min), v), v) > 0.0;  // search.hpp:76
      const double new_off = M::one(d_sub(go_left ? nd.right_min : nd.left_max, v));
      const double far_nbd = d_add(d_sub(nbd, sel3d(nd.axis, o0, o1, o2)), new_off);
      if (radius >= far_nbd) st.push(ref | (go_left ? kRecSide : 0u), far_nbd);
      ref = go_left ? nd.left_ref : nd.right_ref;
    }
    {  // change (a): the own record does not count
      const uint32_t lv = ref & 0x7FFFFFFFu;
      const uint32_t begin = lv >> t.cbits;
      const uint32_t cnt = lv & t.cmask;
      for (uint32_t j = 0; j < cnt; j += kLeaf64) {
        double px[kLeaf64], py[kLeaf64], pz[kLeaf64];
        uint32_t pi[kLeaf64];
#pragma unroll
        for (int u = 0; u < kLeaf64; ++u) {
          const uint32_t pu = begin + j + u <= last ? begin + j + u : last;
          const double4 a = *reinterpret_cast<const double4*>(pts + (uint64_t)pu * kStride64D3);
          px[u] = a.x;
          py[u] = a.y;
          pz[u] = a.z;
          pi[u] = (uint32_t)__double_as_longlong(a.w);
        }
#pragma unroll
        for (int u = 0; u < kLeaf64; ++u) {
          if (j + u < cnt) {
            const double d = M::acc(M::acc(M::first(d_sub(qx, px[u])), d_sub(qy, py[u])), d_sub(qz, pz[u]));
            count += (radius > d && pi[u] != self) ? 1u : 0u;  // strict
          }
        }
      }
    }
    if (count >= limit) break;
    bool entered = false;
    for (;;) {
      if (st.empty()) break;
      const Rec64 r = st.pop();
      if (r.x & kRecUndo) {
        if (r.x & kRecSide) {
          nbd = r.val;
        } else {
          const uint32_t axis = r.x & 0x3FFFFFFFu;
          o0 = axis == 0 ? r.val : o0;
          o1 = axis == 1 ? r.val : o1;
          o2 = axis == 2 ? r.val : o2;
        }
        continue;
      }
      if (radius >= r.val) {  // search.hpp:99
        const uint32_t idx = r.x & 0x3FFFFFFFu;
        const bool far_is_right = (r.x & kRecSide) != 0;
        const Node64 nd = nodes[idx];
        const double new_off = M::one(d_sub(far_is_right ? nd.right_min : nd.left_max, sel3d(nd.axis, qx, qy, qz)));
        st.push(kRecUndo | nd.axis, sel3d(nd.axis, o0, o1, o2));
        st.push(kRecUndo | kRecSide, nbd);
        o0 = nd.axis == 0 ? new_off : o0;
        o1 = nd.axis == 1 ? new_off : o1;
        o2 = nd.axis == 2 ? new_off : o2;
        nbd = r.val;
        ref = far_is_right ? nd.right_ref : nd.left_ref;
        test = try_box;
        entered = true;
        break;
      }
    }
    if (!entered) break;
  }
  Out::put(counts, self, count < limit ? count : limit, max_count);
}

// RadiusSelfFillPolicy over double records (the padding word of a record is written as 0).
struct Radius64SelfFillPolicy {
  double radius;
  int32_t self;
  uint64_t count;
  Neighbor64* out;
  __device__ __forceinline__ double max() const { return radius; }
  __device__ __forceinline__ void visit(int32_t idx, double d) {
    if (radius > d && idx != self) {  // strict
      Neighbor64 nb;
      nb.index = idx;
      nb.pad_ = 0;
      nb.distance = d;
      out[count] = nb;
      ++count;
    }
  }
};

// radius_self_fill_kernel over a float64 tree with dim <= 3 (traverse64_3, as radius64_radii_fill_kernel).
template <class M, bool PER_ROW>
__global__ __launch_bounds__(64) void radius64_self_fill_kernel(
    DevTree64 t, uint64_t first, uint64_t n, double radius_all, const double* __restrict__ radii,
    const uint64_t* __restrict__ offsets, Neighbor64* __restrict__ out, Rec64* __restrict__ stack, uint32_t slots) {
  const uint64_t i = (uint64_t)xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral) * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t dim = t.dim;
  const double4 rec = *reinterpret_cast<const double4*>(t.pts + (first + i) * kStride64D3);
  const uint32_t self = (uint32_t)__double_as_longlong(rec.w);
  const double radius = PER_ROW ? radii[self] : radius_all;
  if (!(radius >= 0.0)) return;
  const double qy = dim > 1 ? rec.y : metric64_pad<M>();
  const double qz = dim > 2 ? rec.z : metric64_pad<M>();
  Stack64 st;
  st.init(0, 0, stack, slots);
  Radius64SelfFillPolicy pol;
  pol.radius = radius;
  pol.self = (int32_t)self;
  pol.count = 0;
  pol.out = out + offsets[self];
  traverse64_3<M>(t, rec.x, qy, qz, pol, st);
}

}  // namespace ptk
