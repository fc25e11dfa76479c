// ptk_kernels_count.hpp -- count_within (ptk.h): the number of points the reference's radius search
// finds for each query, without the rows, for 3-D float32 trees (dim <= 3) and the four non-topological metrics.
//
// A per-branch side table, built on the device on the first count of a handle, gives every branch the number of
// points of its subtree and a box that holds them AND the left_max / right_min of every branch of the subtree (its
// own included): the second part keeps the inside test below valid for a tree read from a stream that does not
// belong to its points.  The count kernel replays the descent of radius_kernel<false> (ptk_kernels.hpp: the near
// child by the side test, the far child only if r >= its box distance, the same incremental arithmetic), and before
// it steps into a branch b -- the root, and every far child as it enters it (profiles/count_within_bench.json: testing
// every near child of the descent as well paid a table read per level of the home path, where neither test can fire,
// and made the kernel slower than the plain count pass at r = 0.25 and 1.0) -- it tries two shortcuts on b's box, on
// the tree's real axes only, and only when the query row and the box are finite:
//   outside  the metric's own accumulation of s_a (0 inside [lo_a, hi_a], else min(one(lo_a - q_a), one(hi_a - q_a)))
//            is not below r: no point of b has a float distance below r (rounding is monotone) -- b is skipped;
//   inside   U = the float sum, in axis order, of max(t_a, off_a), t_a = max(one(lo_a - q_a), one(hi_a - q_a)),
//            with U finite, r not subnormal and U + U * 2^-10 < r: every point of b is below r and the reference
//            enters every node of b (its box distances there exceed U by no more than the drift the 2^-10 margin of
//            knn1_coop_kernel covers) -- b's size is added without visiting it.
// Counts do not depend on the order of the visits, so the kernel need not keep the reference's leaf order; it keeps
// it anyway (it is the same descent), which is what makes `count_shortcut=0` the plain count pass.
#pragma once

#include "ptk_kernels.hpp"

namespace ptk {

// One branch of the side table: {lo.x, lo.y, lo.z, bits(points of the subtree)}, {hi.x, hi.y, hi.z, 0}.
struct CountBox {
  float4 lo;
  float4 hi;
};
static_assert(sizeof(CountBox) == 32, "count table entry");

constexpr uint32_t kCountNoParent = kBranchIdxMask;
// Counters of the emulator (tests): shortcuts taken, inside / outside, and inside tests refused for a subnormal radius.
constexpr uint32_t kCountStatInside = 0, kCountStatOutside = 1, kCountStatSubnormal = 2;

// NaN-propagating min / max: a box with a NaN coordinate must stay non-finite (fminf would drop the NaN).
__device__ __forceinline__ float box_min(float a, float b) { return (a != a || b != b) ? __uint_as_float(0x7FC00000u) : (b < a ? b : a); }
__device__ __forceinline__ float box_max(float a, float b) { return (a != a || b != b) ? __uint_as_float(0x7FC00000u) : (b > a ? b : a); }
__device__ __forceinline__ bool is_finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// Table words are handed from one lane to another in the bottom-up merge: device-scope atomic accesses, so that a
// lane on another XCD reads what the writer stored, not its own L2's copy.
__device__ __forceinline__ void table_store(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = v;
#endif
}
__device__ __forceinline__ uint32_t table_load(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(const_cast<uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
__device__ __forceinline__ void device_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
  __threadfence();
#endif
}

// info[b] = parent branch | split axis of b << 29 (the root: kCountNoParent); arrive[b] = 0.
PTK_GLOBAL void count_parents_kernel(DevTree t, uint32_t n_branches, uint32_t* __restrict__ info,
                                     uint32_t* __restrict__ arrive) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_branches) return;
  arrive[b] = 0u;
  const uint4 nd = t.nodes[b];
  if (!(nd.z & kLeafBit)) info[nd.z & kBranchIdxMask] = (uint32_t)b | (((nd.z >> 29) & 3u) << 29);
  if (!(nd.w & kLeafBit)) info[nd.w & kBranchIdxMask] = (uint32_t)b | (((nd.w >> 29) & 3u) << 29);
  if (b == 0u && !(t.root_ref & kLeafBit))
    info[t.root_ref & kBranchIdxMask] = kCountNoParent | (((t.root_ref >> 29) & 3u) << 29);
}

// The box and size of one child (a leaf: its points; a branch: its finished table entry).
__device__ __forceinline__ void count_child(const DevTree& t, const CountBox* table, uint32_t ref, float (&lo)[3],
                                            float (&hi)[3], uint32_t& n) {
  if (ref & kLeafBit) {
    const uint32_t lv = ref & 0x7FFFFFFFu;
    const uint32_t begin = lv >> t.cbits, count = lv & t.cmask;
    for (uint32_t j = 0; j < count; ++j) {
      const float4 p = t.pts[begin + j];
      lo[0] = box_min(lo[0], p.x);
      lo[1] = box_min(lo[1], p.y);
      lo[2] = box_min(lo[2], p.z);
      hi[0] = box_max(hi[0], p.x);
      hi[1] = box_max(hi[1], p.y);
      hi[2] = box_max(hi[2], p.z);
    }
    n += count;
    return;
  }
  const uint32_t* w = reinterpret_cast<const uint32_t*>(table + (ref & kBranchIdxMask));
  lo[0] = box_min(lo[0], __uint_as_float(table_load(w + 0)));
  lo[1] = box_min(lo[1], __uint_as_float(table_load(w + 1)));
  lo[2] = box_min(lo[2], __uint_as_float(table_load(w + 2)));
  n += table_load(w + 3);
  hi[0] = box_max(hi[0], __uint_as_float(table_load(w + 4)));
  hi[1] = box_max(hi[1], __uint_as_float(table_load(w + 5)));
  hi[2] = box_max(hi[2], __uint_as_float(table_load(w + 6)));
}

// Bottom-up merge: a lane starts at a branch whose children are both leaves, writes its entry and climbs; at each
// parent the last of its branch children to arrive goes on (the others stop), so every entry is written once, after
// those of its children.
PTK_GLOBAL void count_table_kernel(DevTree t, uint32_t n_branches, const uint32_t* __restrict__ info,
                                   uint32_t* __restrict__ arrive, CountBox* __restrict__ table) {
  const uint64_t b0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b0 >= n_branches) return;
  {
    const uint4 nd = t.nodes[b0];
    if (!(nd.z & kLeafBit) || !(nd.w & kLeafBit)) return;
  }
  uint32_t b = (uint32_t)b0;
  for (;;) {
    const uint4 nd = t.nodes[b];
    const uint32_t axis = (info[b] >> 29) & 3u;
    const float inf = __uint_as_float(0x7F800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    uint32_t n = 0;
    count_child(t, table, nd.z, lo, hi, n);
    count_child(t, table, nd.w, lo, hi, n);
    const float lm = __uint_as_float(nd.x), rm = __uint_as_float(nd.y);  // this branch's own two bounds
    lo[axis] = box_min(box_min(lo[axis], lm), rm);
    hi[axis] = box_max(box_max(hi[axis], lm), rm);
    uint32_t* w = reinterpret_cast<uint32_t*>(table + b);
    table_store(w + 0, __float_as_uint(lo[0]));
    table_store(w + 1, __float_as_uint(lo[1]));
    table_store(w + 2, __float_as_uint(lo[2]));
    table_store(w + 3, n);
    table_store(w + 4, __float_as_uint(hi[0]));
    table_store(w + 5, __float_as_uint(hi[1]));
    table_store(w + 6, __float_as_uint(hi[2]));
    table_store(w + 7, 0u);
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

// One query per lane: the reference's count pass with the two shortcuts of the header comment.  `perm`: the batch
// order (null: as given); counts[qi] = the count, clamped to max_count (0: no limit).  `stats` (the emulator only;
// null on the device): the counters kCountStat*.
template <int S, int OVF, int BLOCK, int LEAFB, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void count_within_kernel(
    DevTree t, const CountBox* __restrict__ table, const float* __restrict__ queries, uint32_t dim,
    const uint32_t* __restrict__ perm, uint64_t nq, float radius, uint64_t max_count, uint32_t shortcut,
    uint64_t* __restrict__ counts, uint32_t* __restrict__ stats = nullptr) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= nq) return;
  const uint64_t qi = perm ? perm[i] : i;
  float qx, qy, qz;
  load_query(queries, dim, qi, qx, qy, qz);
  pad_query<M>(dim, qy, qz);
  // The shortcuts: a finite query row (real axes), and for the inside test a radius that is not subnormal.
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
        bool finite_b = true;
        float outside = 0.0f, inside = 0.0f;
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
          if (a < dim) {
            finite_b = finite_b && is_finite_f(lo[a]) && is_finite_f(hi[a]);
            const float dl = M::one(f_sub(lo[a], q[a])), dh = M::one(f_sub(hi[a], q[a]));
            const float s = (q[a] >= lo[a] && q[a] <= hi[a]) ? 0.0f : (dl < dh ? dl : dh);
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
            if (normal_r) {
              if (stats != nullptr) atomicAdd(&stats[kCountStatInside], 1u);
              count += __float_as_uint(bx.lo.w);
              ref = kLeafBit;
              break;
            }
            if (stats != nullptr) atomicAdd(&stats[kCountStatSubnormal], 1u);
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

    {  // the leaf, as radius_kernel scans it
      const uint32_t lv = ref & 0x7FFFFFFFu;
      const uint32_t begin = lv >> t.cbits;
      const uint32_t n = lv & t.cmask;
      for (uint32_t j = 0; j < n; j += LEAFB) {
        float4 p[LEAFB];
#pragma unroll
        for (int u = 0; u < LEAFB; ++u) p[u] = pts[begin + j + u];
#pragma unroll
        for (int u = 0; u < LEAFB; ++u) {
          if (j + u < n) {
            const float d = point_distance3<M>(f_sub(qx, p[u].x), f_sub(qy, p[u].y), f_sub(qz, p[u].z));
            count += radius > d ? 1u : 0u;  // strict
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
  counts[qi] = count < limit ? count : limit;
}

// count_within_radii (ptk.h): count_within_kernel with the lane's own radius, radii[qi] (a copy: the scalar call's kernel
// stays the code it is -- a change to one belongs in both).  A NaN or negative radius passes no test: the count is 0.
template <int S, int OVF, int BLOCK, int LEAFB, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void count_within_radii_kernel(
    DevTree t, const CountBox* __restrict__ table, const float* __restrict__ queries, uint32_t dim,
    const uint32_t* __restrict__ perm, uint64_t nq, const float* __restrict__ radii, uint64_t max_count,
    uint32_t shortcut,
    uint64_t* __restrict__ counts, uint32_t* __restrict__ stats = nullptr) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= nq) return;
  const uint64_t qi = perm ? perm[i] : i;
  const float radius = radii[qi];  // (the row in the caller's order; `normal_r` below is the lane's with it)
  float qx, qy, qz;
  load_query(queries, dim, qi, qx, qy, qz);
  pad_query<M>(dim, qy, qz);
  // The shortcuts: a finite query row (real axes), and for the inside test a radius that is not subnormal.
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
        bool finite_b = true;
        float outside = 0.0f, inside = 0.0f;
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
          if (a < dim) {
            finite_b = finite_b && is_finite_f(lo[a]) && is_finite_f(hi[a]);
            const float dl = M::one(f_sub(lo[a], q[a])), dh = M::one(f_sub(hi[a], q[a]));
            const float s = (q[a] >= lo[a] && q[a] <= hi[a]) ? 0.0f : (dl < dh ? dl : dh);
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
            if (normal_r) {
              if (stats != nullptr) atomicAdd(&stats[kCountStatInside], 1u);
              count += __float_as_uint(bx.lo.w);
              ref = kLeafBit;
              break;
            }
            if (stats != nullptr) atomicAdd(&stats[kCountStatSubnormal], 1u);
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

    {  // the leaf, as radius_kernel scans it
      const uint32_t lv = ref & 0x7FFFFFFFu;
      const uint32_t begin = lv >> t.cbits;
      const uint32_t n = lv & t.cmask;
      for (uint32_t j = 0; j < n; j += LEAFB) {
        float4 p[LEAFB];
#pragma unroll
        for (int u = 0; u < LEAFB; ++u) p[u] = pts[begin + j + u];
#pragma unroll
        for (int u = 0; u < LEAFB; ++u) {
          if (j + u < n) {
            const float d = point_distance3<M>(f_sub(qx, p[u].x), f_sub(qy, p[u].y), f_sub(qz, p[u].z));
            count += radius > d ? 1u : 0u;  // strict
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
  counts[qi] = count < limit ? count : limit;
}

// search_radius_radii (ptk.h): the fill pass behind count_within_radii_kernel(max_count = 0) and a scan of its counts --
// radius_kernel<FILL = true> (ptk_kernels.hpp) with the lane's own radius, radii[qi], and e = 1 (a copy: the scalar
// call's kernel stays the code it is -- a change to one belongs in both).  Row qi is written at out + offsets[qi] in the
// reference's traversal order; neither shortcut of the count kernel is taken (the inside one cannot be: the order inside a
// subtree depends on the query).  A NaN or negative radius -- its count was 0 -- leaves before it touches `out`.
template <int S, int OVF, int BLOCK, int LEAFB, class M = MetricL2>
__global__ __launch_bounds__(BLOCK) void radius_radii_fill_kernel(
    DevTree t, const float* __restrict__ queries, uint32_t dim,
    const uint32_t* __restrict__ perm, uint64_t nq, const float* __restrict__ radii,
    const uint64_t* __restrict__ offsets, Neighbor* __restrict__ out) {
  const uint32_t tile = xcd_runs(blockIdx.x, gridDim.x, kXcdRunGeneral);
  const uint64_t i = (uint64_t)tile * BLOCK + threadIdx.x;
  if (i >= nq) return;
  const uint64_t qi = perm ? perm[i] : i;
  const float radius = radii[qi];  // (the row in the caller's order, not the launch position)
  if (!(radius >= 0.0f)) return;
  float qx, qy, qz;
  load_query(queries, dim, qi, qx, qy, qz);
  pad_query<M>(dim, qy, qz);

  PTK_STACK(S, OVF, BLOCK, st, t);
  RadiusPolicy<kRadiusFill> pol;
  pol.radius = radius;
  pol.e_inv = 1.0f;
  pol.count = 0;
  pol.out = out + offsets[qi];
  traverse<LEAFB, false, M>(t, qx, qy, qz, pol, st);
}

// counts[i] = min(counts[i], max_count): the count kernels of the other families (no limit of their own).
PTK_GLOBAL void clamp_counts_kernel(uint64_t* __restrict__ counts, uint64_t n, uint64_t max_count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && counts[i] > max_count) counts[i] = max_count;
}

}  // namespace ptk
