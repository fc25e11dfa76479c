// ptk_kernels_count64.hpp -- count_within of float64 trees, dim <= 3, the four non-topological metrics: the side table
// and the count kernel of ptk_kernels_count.hpp in double, over the tree of ptk_kernels_f64.hpp (Node64 branch
// records, {x, y, z, index} point records).  The inside test keeps the margin U + U * 2^-10 < r: in double it covers
// the drift of the incremental box distance on a path of any depth a tree can have, so no tree is excluded.
#pragma once

#include "ptk_kernels_count.hpp"
#include "ptk_kernels_f64.hpp"

namespace ptk {

// One branch: {lo.x, lo.y, lo.z, bits(points of the subtree)}, {hi.x, hi.y, hi.z, 0}.
struct CountBox64 {
  double4 lo;
  double4 hi;
};
static_assert(sizeof(CountBox64) == 64, "count table entry (double)");

__device__ __forceinline__ double box_min64(double a, double b) {
  return (a != a || b != b) ? __longlong_as_double(0x7FF8000000000000ll) : (b < a ? b : a);
}
__device__ __forceinline__ double box_max64(double a, double b) {
  return (a != a || b != b) ? __longlong_as_double(0x7FF8000000000000ll) : (b > a ? b : a);
}
__device__ __forceinline__ bool is_finite_d(double x) {
  return (__double_as_longlong(x) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll;
}
__device__ __forceinline__ void table_store64(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = v;
#endif
}
__device__ __forceinline__ unsigned long long table_load64(const unsigned long long* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(const_cast<unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// info[b] = parent branch (the root: kCountNoParent); arrive[b] = 0.
PTK_GLOBAL void count64_parents_kernel(DevTree64 t, uint32_t n_branches, uint32_t* __restrict__ info,
                                       uint32_t* __restrict__ arrive) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_branches) return;
  arrive[b] = 0u;
  const Node64 nd = t.nodes[b];
  if (!(nd.left_ref & kLeafBit)) info[nd.left_ref] = (uint32_t)b;
  if (!(nd.right_ref & kLeafBit)) info[nd.right_ref] = (uint32_t)b;
  if (b == 0u && !(t.root_ref & kLeafBit)) info[t.root_ref] = kCountNoParent;
}

__device__ __forceinline__ void count64_child(const DevTree64& t, const CountBox64* table, uint32_t ref, double (&lo)[3],
                                              double (&hi)[3], uint64_t& n) {
  if (ref & kLeafBit) {
    const uint32_t lv = ref & 0x7FFFFFFFu;
    const uint32_t begin = lv >> t.cbits, count = lv & t.cmask;
    for (uint32_t j = 0; j < count; ++j) {
      const double4 p = *reinterpret_cast<const double4*>(t.pts + (uint64_t)(begin + j) * kStride64D3);
      lo[0] = box_min64(lo[0], p.x);
      lo[1] = box_min64(lo[1], p.y);
      lo[2] = box_min64(lo[2], p.z);
      hi[0] = box_max64(hi[0], p.x);
      hi[1] = box_max64(hi[1], p.y);
      hi[2] = box_max64(hi[2], p.z);
    }
    n += count;
    return;
  }
  const unsigned long long* w = reinterpret_cast<const unsigned long long*>(table + ref);
  lo[0] = box_min64(lo[0], __longlong_as_double((long long)table_load64(w + 0)));
  lo[1] = box_min64(lo[1], __longlong_as_double((long long)table_load64(w + 1)));
  lo[2] = box_min64(lo[2], __longlong_as_double((long long)table_load64(w + 2)));
  n += table_load64(w + 3);
  hi[0] = box_max64(hi[0], __longlong_as_double((long long)table_load64(w + 4)));
  hi[1] = box_max64(hi[1], __longlong_as_double((long long)table_load64(w + 5)));
  hi[2] = box_max64(hi[2], __longlong_as_double((long long)table_load64(w + 6)));
}

// The bottom-up merge of count_table_kernel.
PTK_GLOBAL void count64_table_kernel(DevTree64 t, uint32_t n_branches, const uint32_t* __restrict__ info,
                                     uint32_t* __restrict__ arrive, CountBox64* __restrict__ table) {
  const uint64_t b0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b0 >= n_branches) return;
  {
    const Node64 nd = t.nodes[b0];
    if (!(nd.left_ref & kLeafBit) || !(nd.right_ref & kLeafBit)) return;
  }
  uint32_t b = (uint32_t)b0;
  for (;;) {
    const Node64 nd = t.nodes[b];
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    uint64_t n = 0;
    count64_child(t, table, nd.left_ref, lo, hi, n);
    count64_child(t, table, nd.right_ref, lo, hi, n);
    const uint32_t axis = nd.axis < 3u ? nd.axis : 2u;
    lo[axis] = box_min64(box_min64(lo[axis], nd.left_max), nd.right_min);  // this branch's own two bounds
    hi[axis] = box_max64(box_max64(hi[axis], nd.left_max), nd.right_min);
    unsigned long long* w = reinterpret_cast<unsigned long long*>(table + b);
    table_store64(w + 0, (unsigned long long)__double_as_longlong(lo[0]));
    table_store64(w + 1, (unsigned long long)__double_as_longlong(lo[1]));
    table_store64(w + 2, (unsigned long long)__double_as_longlong(lo[2]));
    table_store64(w + 3, n);
    table_store64(w + 4, (unsigned long long)__double_as_longlong(hi[0]));
    table_store64(w + 5, (unsigned long long)__double_as_longlong(hi[1]));
    table_store64(w + 6, (unsigned long long)__double_as_longlong(hi[2]));
    table_store64(w + 7, 0ull);
    const uint32_t p = info[b];
    if (p == kCountNoParent) return;
    const Node64 pn = t.nodes[p];
    const uint32_t need = ((pn.left_ref & kLeafBit) ? 0u : 1u) + ((pn.right_ref & kLeafBit) ? 0u : 1u);
    device_fence();
    if (atomicAdd(&arrive[p], 1u) + 1u < need) return;
    device_fence();
    b = p;
  }
}

// One query per lane: radius64_kernel<M, false, true>'s count walk (traverse64_3) with the outside / inside tests of
// count_within_kernel at the root and at every far child it enters.  Launch-order entries [q0, q0 + nq), as
// radius64_kernel; counts[qi] clamped to max_count (0: no limit); `stats`: the emulator's counters (null on the device).
template <class M>
__global__ __launch_bounds__(64) void count64_within_kernel(
    DevTree64 t, const CountBox64* __restrict__ table, const double* __restrict__ queries,
    const uint32_t* __restrict__ perm, uint64_t q0, uint64_t nq, double radius, uint64_t max_count, uint32_t shortcut,
    uint64_t* __restrict__ counts, Rec64* __restrict__ stack, uint32_t slots, uint32_t* __restrict__ stats = nullptr) {
  const uint64_t i = (uint64_t)xcd_runs(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
  if (i >= nq) return;
  const uint64_t qi = perm ? perm[q0 + i] : q0 + i;
  const uint32_t dim = t.dim;
  const double* row = queries + qi * dim;
  const double qx = row[0];
  // (a missing axis: zero like the points' for sums and maxima, +inf for the minimum of metric_lninf)
  const double qy = dim > 1 ? row[1] : metric64_pad<M>();
  const double qz = dim > 2 ? row[2] : metric64_pad<M>();
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
        bool finite_b = true;
        double outside = 0.0, inside = 0.0;
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
          if (a < dim) {
            finite_b = finite_b && is_finite_d(lo[a]) && is_finite_d(hi[a]);
            const double dl = M::one(d_sub(lo[a], q[a])), dh = M::one(d_sub(hi[a], q[a]));
            const double s = (q[a] >= lo[a] && q[a] <= hi[a]) ? 0.0 : (dl < dh ? dl : dh);
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
            if (normal_r) {
              if (stats != nullptr) atomicAdd(&stats[kCountStatInside], 1u);
              count += (uint64_t)__double_as_longlong(bx.lo.w);
              ref = kLeafBit;
              break;
            }
            if (stats != nullptr) atomicAdd(&stats[kCountStatSubnormal], 1u);
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
    {
      const uint32_t lv = ref & 0x7FFFFFFFu;
      const uint32_t begin = lv >> t.cbits;
      const uint32_t n = lv & t.cmask;
      for (uint32_t j = 0; j < n; j += kLeaf64) {
        double px[kLeaf64], py[kLeaf64], pz[kLeaf64];
#pragma unroll
        for (int u = 0; u < kLeaf64; ++u) {
          const uint32_t pu = begin + j + u <= last ? begin + j + u : last;
          const double4 a = *reinterpret_cast<const double4*>(pts + (uint64_t)pu * kStride64D3);
          px[u] = a.x;
          py[u] = a.y;
          pz[u] = a.z;
        }
#pragma unroll
        for (int u = 0; u < kLeaf64; ++u) {
          if (j + u < n) {
            const double d = M::acc(M::acc(M::first(d_sub(qx, px[u])), d_sub(qy, py[u])), d_sub(qz, pz[u]));
            count += radius > d ? 1u : 0u;  // strict
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
  counts[qi] = count < limit ? count : limit;
}

// search64_count_within_radii: count64_within_kernel with the lane's own radius, radii[qi] (a copy, as
// count_within_radii_kernel).
template <class M>
__global__ __launch_bounds__(64) void count64_within_radii_kernel(
    DevTree64 t, const CountBox64* __restrict__ table, const double* __restrict__ queries,
    const uint32_t* __restrict__ perm, uint64_t q0, uint64_t nq, const double* __restrict__ radii, uint64_t max_count,
    uint32_t shortcut,
    uint64_t* __restrict__ counts, Rec64* __restrict__ stack, uint32_t slots, uint32_t* __restrict__ stats = nullptr) {
  const uint64_t i = (uint64_t)xcd_runs(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
  if (i >= nq) return;
  const uint64_t qi = perm ? perm[q0 + i] : q0 + i;
  const double radius = radii[qi];
  const uint32_t dim = t.dim;
  const double* row = queries + qi * dim;
  const double qx = row[0];
  // (a missing axis: zero like the points' for sums and maxima, +inf for the minimum of metric_lninf)
  const double qy = dim > 1 ? row[1] : metric64_pad<M>();
  const double qz = dim > 2 ? row[2] : metric64_pad<M>();
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
        bool finite_b = true;
        double outside = 0.0, inside = 0.0;
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
          if (a < dim) {
            finite_b = finite_b && is_finite_d(lo[a]) && is_finite_d(hi[a]);
            const double dl = M::one(d_sub(lo[a], q[a])), dh = M::one(d_sub(hi[a], q[a]));
            const double s = (q[a] >= lo[a] && q[a] <= hi[a]) ? 0.0 : (dl < dh ? dl : dh);
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
            if (normal_r) {
              if (stats != nullptr) atomicAdd(&stats[kCountStatInside], 1u);
              count += (uint64_t)__double_as_longlong(bx.lo.w);
              ref = kLeafBit;
              break;
            }
            if (stats != nullptr) atomicAdd(&stats[kCountStatSubnormal], 1u);
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
    {
      const uint32_t lv = ref & 0x7FFFFFFFu;
      const uint32_t begin = lv >> t.cbits;
      const uint32_t n = lv & t.cmask;
      for (uint32_t j = 0; j < n; j += kLeaf64) {
        double px[kLeaf64], py[kLeaf64], pz[kLeaf64];
#pragma unroll
        for (int u = 0; u < kLeaf64; ++u) {
          const uint32_t pu = begin + j + u <= last ? begin + j + u : last;
          const double4 a = *reinterpret_cast<const double4*>(pts + (uint64_t)pu * kStride64D3);
          px[u] = a.x;
          py[u] = a.y;
          pz[u] = a.z;
        }
#pragma unroll
        for (int u = 0; u < kLeaf64; ++u) {
          if (j + u < n) {
            const double d = M::acc(M::acc(M::first(d_sub(qx, px[u])), d_sub(qy, py[u])), d_sub(qz, pz[u]));
            count += radius > d ? 1u : 0u;  // strict
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
  counts[qi] = count < limit ? count : limit;
}

}  // namespace ptk
