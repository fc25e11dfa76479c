// ptk_kernels_build.hpp -- the kernels of the device tree build (ptk_build.hpp has the host driver and the account of
// the method): no runtime and no rocprim calls, so that the CPU tier compiles this header against its HIP stand-in and
// runs the kernels lane by lane (tests/cpp/emulate_build_main.cpp).

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// A kernel that is not a template is defined in a header several translation units include (ptk_backend_core.hpp):
// internal linkage, so every unit that launches it has its own and the units that do not emit nothing.
#ifndef PTK_GLOBAL
#define PTK_GLOBAL static __global__
#endif

namespace ptk {

struct BuildSeg {
  uint32_t begin, end, axis;
  float plane;
  uint32_t m;          // out: points below the plane
  uint32_t pass_left;  // out: of those, already among the first m positions
  uint32_t pad0, pad1;
};

constexpr uint32_t kBuildMaxDim = 8;
constexpr uint32_t kBuildBoxBlocks = 1024;

PTK_GLOBAL __launch_bounds__(256) void build_iota_kernel(int32_t* __restrict__ idx, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) idx[i] = (int32_t)i;
}

// Per block: min and max of every coordinate over a slice of the points (exact: any grouping gives the same box).
PTK_GLOBAL __launch_bounds__(256) void build_box_kernel(
    const float* __restrict__ pts, uint32_t n, uint32_t dim, float* __restrict__ partial) {
  __shared__ float lo[256], hi[256];
  for (uint32_t a = 0; a < dim; ++a) {
    float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
      const float v = pts[i * dim + a];
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
    }
    lo[threadIdx.x] = mn;
    hi[threadIdx.x] = mx;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) {
        lo[threadIdx.x] = lo[threadIdx.x + s] < lo[threadIdx.x] ? lo[threadIdx.x + s] : lo[threadIdx.x];
        hi[threadIdx.x] = hi[threadIdx.x + s] > hi[threadIdx.x] ? hi[threadIdx.x + s] : hi[threadIdx.x];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      partial[(blockIdx.x * dim + a) * 2 + 0] = lo[0];
      partial[(blockIdx.x * dim + a) * 2 + 1] = hi[0];
    }
    __syncthreads();
  }
}

// The node of the level position i lies in (the nodes are in position order); nsegs if none.
__device__ __forceinline__ uint32_t build_find(const BuildSeg* __restrict__ segs, uint32_t nsegs, uint32_t i) {
  uint32_t lo = 0, hi = nsegs;  // first node with begin > i
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (segs[mid].begin <= i) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return nsegs;
  return i < segs[lo - 1].end ? lo - 1 : nsegs;
}

PTK_GLOBAL __launch_bounds__(256) void build_flag_kernel(
    const float* __restrict__ pts, uint32_t dim, const int32_t* __restrict__ idx, const BuildSeg* __restrict__ segs,
    uint32_t nsegs, uint32_t n, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  uint32_t f = 0;
  if (i < n) {
    const uint32_t s = build_find(segs, nsegs, i);
    if (s < nsegs) f = pts[(uint64_t)(uint32_t)idx[i] * dim + segs[s].axis] < segs[s].plane ? 1u : 0u;
  }
  flags[i] = f;  // (flags[n] = 0: the scan then also yields the total)
}

PTK_GLOBAL void build_cut_kernel(const uint32_t* __restrict__ sums, BuildSeg* __restrict__ segs, uint32_t nsegs) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsegs) return;
  const uint32_t b = segs[s].begin;
  const uint32_t m = sums[segs[s].end] - sums[b];
  segs[s].m = m;
  segs[s].pass_left = sums[b + m] - sums[b];
}

PTK_GLOBAL __launch_bounds__(256) void build_list_kernel(
    const uint32_t* __restrict__ flags, const uint32_t* __restrict__ sums, const BuildSeg* __restrict__ segs,
    uint32_t nsegs, uint32_t n, uint32_t* __restrict__ from_left, uint32_t* __restrict__ from_right) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = build_find(segs, nsegs, i);
  if (s >= nsegs) return;
  const uint32_t b = segs[s].begin, m = segs[s].m;
  const uint32_t before = sums[i] - sums[b];  // passing positions of this node before i
  if (i < b + m) {
    if (!flags[i]) from_left[b + (i - b) - before] = i;  // its rank among the failing positions of the left part
  } else if (flags[i]) {
    from_right[b + before - segs[s].pass_left] = i;  // its rank among the passing positions of the right part
  }
}

PTK_GLOBAL __launch_bounds__(256) void build_swap_kernel(
    int32_t* __restrict__ idx, const BuildSeg* __restrict__ segs, uint32_t nsegs, uint32_t n,
    const uint32_t* __restrict__ from_left, const uint32_t* __restrict__ from_right) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = build_find(segs, nsegs, i);
  if (s >= nsegs) return;
  const uint32_t b = segs[s].begin, swaps = segs[s].m - segs[s].pass_left, k = i - b;
  if (k >= swaps) return;
  const uint32_t l = from_left[b + k], r = from_right[b + swaps - 1u - k];
  const int32_t t = idx[l];
  idx[l] = idx[r];
  idx[r] = t;
}

// ---- the sliding step (std::nth_element) ---------------------------------------------------------------------------
// When a partition leaves one side empty the reference slides the plane to the nearest point with std::nth_element
// (internal/kd_tree_builder.hpp:255-275), and the permutation that call leaves is part of the tree.  libstdc++'s
// nth_element is an introselect (bits/stl_algo.h:1964-1986): rounds of "median of three to the front, Hoare partition
// of the rest around it, keep the side that holds nth" until at most three elements are left.  The first rounds --
// the ones that touch a million indices -- are made here; the partition of a round is, like std::partition above,
// a pairing by rank:
//
//   __unguarded_partition(first + 1, last, pivot = first) moves a left pointer up to the next element that is NOT
//   below the pivot and a right pointer down to the next that is NOT above it, swaps the two and goes on, until the
//   pointers meet; until then both pointers only see elements nobody has moved yet.  So the k-th "left stop"
//   (positions with !(v < pivot), ascending) is swapped with the k-th "right stop" (positions with !(pivot < v),
//   descending) for every k below K = the first k whose left stop is not left of its right stop; the function returns
//   where the left pointer stands at the end (slide_pair_kernel).
//
// flags (both kinds, packed in one 64-bit word), one scan, the two rank lists, the pairs; the host reads the cut and
// decides which side is kept, exactly as __introselect does.  Once the range is small the host finishes the SAME
// call -- std::__introselect on what is left, with what is left of its depth limit -- so the outcome is libstdc++'s
// to the last swap (tests/test_device_build.py: byte-identical trees on clouds whose planes slide).
PTK_GLOBAL void slide_pivot_kernel(const float* __restrict__ pts, uint32_t dim, uint32_t axis, int32_t* __restrict__ idx,
                                   uint32_t first, uint32_t last, float* __restrict__ pivot) {
  // __move_median_to_first(result = first, a = first + 1, b = mid, c = last - 1)
  const uint32_t a = first + 1u, b = first + (last - first) / 2u, c = last - 1u;
  auto val = [&](uint32_t i) { return pts[(uint64_t)(uint32_t)idx[i] * dim + axis]; };
  const float va = val(a), vb = val(b), vc = val(c);
  uint32_t pick;
  if (va < vb) {
    if (vb < vc) pick = b;
    else if (va < vc) pick = c;
    else pick = a;
  } else if (va < vc) {
    pick = a;
  } else if (vb < vc) {
    pick = c;
  } else {
    pick = b;
  }
  const int32_t t = idx[first];
  idx[first] = idx[pick];
  idx[pick] = t;
  *pivot = val(first);
}

// flags[i - lo] = {left stop, right stop << 32} for the positions [lo, hi); flags[hi - lo] = 0 (the scan's total).
PTK_GLOBAL __launch_bounds__(256) void slide_flag_kernel(const float* __restrict__ pts, uint32_t dim, uint32_t axis,
                                                         const int32_t* __restrict__ idx, uint32_t lo, uint32_t hi,
                                                         const float* __restrict__ pivot,
                                                         unsigned long long* __restrict__ flags) {
  const uint32_t i = lo + blockIdx.x * 256u + threadIdx.x;
  if (i > hi) return;
  unsigned long long f = 0ull;
  if (i < hi) {
    const float v = pts[(uint64_t)(uint32_t)idx[i] * dim + axis], p = *pivot;
    f = (!(v < p) ? 1ull : 0ull) | (!(p < v) ? 1ull << 32 : 0ull);
  }
  flags[i - lo] = f;
}

// left_list[k] = position of the k-th left stop (ascending), right_list[k] = position of the k-th right stop (descending).
PTK_GLOBAL __launch_bounds__(256) void slide_list_kernel(const unsigned long long* __restrict__ flags,
                                                         const unsigned long long* __restrict__ sums, uint32_t lo,
                                                         uint32_t hi, uint32_t* __restrict__ left_list,
                                                         uint32_t* __restrict__ right_list) {
  const uint32_t i = lo + blockIdx.x * 256u + threadIdx.x;
  if (i >= hi) return;
  const unsigned long long f = flags[i - lo], before = sums[i - lo], total = sums[hi - lo];
  if (f & 0xFFFFFFFFull) left_list[(uint32_t)before] = i;
  if (f >> 32) right_list[(uint32_t)(total >> 32) - (uint32_t)(before >> 32) - 1u] = i;
}

// The pairs below K are swapped (K = the first k whose left stop is missing or not left of its right stop).  What
// the function returns is where the left pointer stands then: it has moved on from left stop K - 1 to the next element
// that is not below the pivot -- left stop K, unless it first meets the element it swapped into right stop K - 1:
// *cut = min(left stop K, right stop K - 1)   (K = 0: left stop 0, which a median-of-three pivot guarantees).
PTK_GLOBAL __launch_bounds__(256) void slide_pair_kernel(int32_t* __restrict__ idx, const unsigned long long* __restrict__ sums,
                                                         uint32_t n_range, const uint32_t* __restrict__ left_list,
                                                         const uint32_t* __restrict__ right_list, uint32_t* __restrict__ cut) {
  const unsigned long long total = sums[n_range];
  const uint32_t n_left = (uint32_t)total, n_right = (uint32_t)(total >> 32);
  const uint32_t pairs = n_left < n_right ? n_left : n_right;
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > pairs) return;
  const bool active = k < pairs && left_list[k] < right_list[k];
  if (active) {
    const uint32_t l = left_list[k], r = right_list[k];
    const int32_t t = idx[l];
    idx[l] = idx[r];
    idx[r] = t;
  } else if (k == 0u || left_list[k - 1u] < right_list[k - 1u]) {  // k = K
    const uint32_t l_k = k < n_left ? left_list[k] : 0xFFFFFFFFu;
    *cut = k == 0u ? l_k : (l_k < right_list[k - 1u] ? l_k : right_list[k - 1u]);
  }
}

}  // namespace ptk
