// ptk_build.hpp -- the top levels of the tree build on the device (tree build acceleration).
//
// The reference builds its tree top-down (internal/kd_tree_builder.hpp:229-276, :352-396: sliding midpoint, box of
// a child = box of the parent cut at the plane, std::partition of the index range).  Everything a level needs is
// known once its parent level is done, and the only part that touches every point is the partition.  The first
// levels of a large cloud are a handful of partitions of millions of indices each -- the part the host's threads
// scale worst on (one std::partition per node, serial at the root) -- so those are made here:
//
//   flags    pass[i] = point[idx[i]][axis] < plane for every position of every node of the level (one launch)
//   scan     exclusive sum of the flags over the whole permutation (rocprim)
//   cut      per node: m = passing points, and how many of them already lie in the first m positions
//   lists    std::partition on a range (libstdc++, bidirectional scheme) swaps the k-th failing position from the
//            left of the cut with the k-th passing position from the right end: both lists, by their scan ranks
//   swap     the pairs
//
// which leaves the permutation std::partition leaves, position for position (the same argument as
// pico_tree::internal::parallel_partition, include/pico_tree/internal/flat_tree.hpp).  Planes, boxes and the split
// axis are computed on the host exactly as the host builder computes them (split_top_levels()); nodes of at most
// `threshold` points go back to the host, where a pool of workers builds each subtree the ordinary way
// (build_flat_tree_below()).  A node whose partition leaves one side empty needs the sliding step, std::nth_element,
// whose permutation only the host library defines: its range makes a round trip to the host (on the scan-like cloud of
// BASELINE config 2 an outlier makes the plane of a 963 k-point node slide four times in a row).
// tests/test_device_build.py compares a tree built this way with the host build byte for byte -- and, by the record of
// ptk_debug_create_route (BuildRoute), that it WAS built this way; tests/cpp/emulate_build_main.cpp runs the kernels of
// ptk_kernels_build.hpp on the CPU against std::partition and std::nth_element.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <utility>
#include <vector>

#include "pico_tree/internal/flat_tree.hpp"
#include "ptk_kernels_build.hpp"

namespace ptk {

// Device buffers of one build (freed on every path).
struct BuildBuffers {
  float* pts = nullptr;
  int32_t* idx = nullptr;
  uint32_t *flags = nullptr, *sums = nullptr, *from_left = nullptr, *from_right = nullptr;
  BuildSeg* segs = nullptr;
  float* partial = nullptr;
  void* scan_tmp = nullptr;
  // the sliding step (allocated on the first slide)
  unsigned long long *flags64 = nullptr, *sums64 = nullptr;
  void* scan_tmp64 = nullptr;
  size_t scan_bytes64 = 0;
  float* pivot = nullptr;  // {pivot value, cut (as uint32)}
  ~BuildBuffers() {
    for (void* p : {(void*)pts, (void*)idx, (void*)flags, (void*)sums, (void*)from_left, (void*)from_right, (void*)segs,
                    (void*)partial, scan_tmp, (void*)flags64, (void*)sums64, scan_tmp64, (void*)pivot})
      if (p != nullptr) (void)hipFree(p);
  }
};

// Builds the sliding-midpoint tree of `points` with the partitions of the large nodes made on the current device.
// Returns false (and leaves `tree` alone) when the build has to be made on the host instead: a HIP failure, a
// plane that slides in the top levels, an unsupported shape.  `top_ms` (optional): time spent in the device levels.
// `route` (optional): what was done, and why not when the answer is false (ptk_debug_create_route).
template <typename SpaceView_, typename Tree_>
bool device_top_build(const float* points, uint64_t n, uint32_t dim, size_t max_leaf_size, unsigned threads,
                      SpaceView_ const& view, Tree_& tree, double* phase_ms = nullptr, BuildRoute* route = nullptr) {
  using namespace pico_tree;
  using box_type = typename Tree_::box_type;
  BuildRoute unused;
  BuildRoute& did = route != nullptr ? *route : unused;
  did = BuildRoute{};
  const char*& reason = did.why;
  reason = "shape not supported";
  if (dim == 0 || dim > kBuildMaxDim || n < 2 || n >= (1ull << 31)) return false;
  const auto t_start = std::chrono::steady_clock::now();
  const bool verbose = std::getenv("PTK_CREATE_TIMING") != nullptr && std::atoi(std::getenv("PTK_CREATE_TIMING")) > 1;
  auto t_last = t_start;
  auto lap = [&](const char* what) {
    if (!verbose) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[ptk build]   %-34s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  double slide_ms = 0.0;
  auto ok = [&reason](hipError_t e) {
    if (e == hipSuccess) return true;
    reason = hipGetErrorString(e);
    (void)hipGetLastError();
    return false;
  };
  const uint32_t n32 = (uint32_t)n;
  // Nodes above this many points are split here: about eight subtrees per worker, none smaller than 16 k points.
  const size_t threshold = std::max<size_t>(std::max<size_t>(16384, max_leaf_size), n / ((size_t)std::max(1u, threads) * 8));
  const size_t max_segs = 2 * (n / threshold) + 64;
  did.threshold = threshold;
  BuildBuffers b;
  size_t scan_bytes = 0;
  if (!ok(rocprim::exclusive_scan(nullptr, scan_bytes, b.flags, b.sums, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(),
                                  (hipStream_t) nullptr)))
    return false;
  if (!ok(hipMalloc((void**)&b.pts, n * dim * sizeof(float))) || !ok(hipMalloc((void**)&b.idx, n * 4)) ||
      !ok(hipMalloc((void**)&b.flags, (n + 1) * 4)) || !ok(hipMalloc((void**)&b.sums, (n + 1) * 4)) ||
      !ok(hipMalloc((void**)&b.from_left, n * 4)) || !ok(hipMalloc((void**)&b.from_right, n * 4)) ||
      !ok(hipMalloc((void**)&b.segs, max_segs * sizeof(BuildSeg))) ||
      !ok(hipMalloc((void**)&b.partial, (size_t)kBuildBoxBlocks * dim * 2 * sizeof(float))) ||
      !ok(hipMalloc(&b.scan_tmp, scan_bytes + 256)))
    return false;
  lap("device buffers");
  if (!ok(hipMemcpy(b.pts, points, n * dim * sizeof(float), hipMemcpyHostToDevice))) return false;
  lap("points to the device");
  const uint32_t blocks = (n32 + 256u) / 256u;  // covers position n as well
  hipLaunchKernelGGL(build_iota_kernel, dim3(blocks), dim3(256), 0, nullptr, b.idx, n32);
  hipLaunchKernelGGL(build_box_kernel, dim3(kBuildBoxBlocks), dim3(256), 0, nullptr, b.pts, n32, dim, b.partial);
  if (!ok(hipGetLastError())) return false;  // (a launch that failed: the caller builds on the host instead)
  std::vector<float> partial((size_t)kBuildBoxBlocks * dim * 2);
  if (!ok(hipMemcpy(partial.data(), b.partial, partial.size() * sizeof(float), hipMemcpyDeviceToHost))) return false;
  box_type root(dim);
  root.invert();
  for (uint32_t blk = 0; blk < kBuildBoxBlocks; ++blk)
    for (uint32_t a = 0; a < dim; ++a) {
      const float lo = partial[((size_t)blk * dim + a) * 2], hi = partial[((size_t)blk * dim + a) * 2 + 1];
      if (lo < root.min(a)) root.min(a) = lo;
      if (hi > root.max(a)) root.max(a) = hi;
    }

  std::vector<BuildSeg> host_segs;
  auto on_device = [&](std::vector<internal::top_segment<float>>& segments) -> bool {
    ++did.levels;
    if (segments.size() > max_segs) {
      reason = "more nodes in a level than planned for";
      return false;
    }
    const uint32_t nsegs = (uint32_t)segments.size();
    host_segs.resize(nsegs);
    for (uint32_t s = 0; s < nsegs; ++s)
      host_segs[s] = BuildSeg{(uint32_t)segments[s].begin, (uint32_t)segments[s].end, segments[s].axis, segments[s].plane, 0, 0, 0, 0};
    if (!ok(hipMemcpy(b.segs, host_segs.data(), nsegs * sizeof(BuildSeg), hipMemcpyHostToDevice))) return false;
    hipLaunchKernelGGL(build_flag_kernel, dim3(blocks), dim3(256), 0, nullptr, b.pts, dim, b.idx, b.segs, nsegs, n32, b.flags);
    size_t bytes = scan_bytes + 256;
    if (!ok(rocprim::exclusive_scan(b.scan_tmp, bytes, b.flags, b.sums, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(),
                                    (hipStream_t) nullptr)))
      return false;
    hipLaunchKernelGGL(build_cut_kernel, dim3((nsegs + 63) / 64), dim3(64), 0, nullptr, b.sums, b.segs, nsegs);
    hipLaunchKernelGGL(build_list_kernel, dim3(blocks), dim3(256), 0, nullptr, b.flags, b.sums, b.segs, nsegs, n32, b.from_left,
                       b.from_right);
    hipLaunchKernelGGL(build_swap_kernel, dim3(blocks), dim3(256), 0, nullptr, b.idx, b.segs, nsegs, n32, b.from_left,
                       b.from_right);
    if (!ok(hipGetLastError())) return false;
    if (!ok(hipMemcpy(host_segs.data(), b.segs, nsegs * sizeof(BuildSeg), hipMemcpyDeviceToHost))) return false;
    for (uint32_t s = 0; s < nsegs; ++s) segments[s].cut = segments[s].begin + host_segs[s].m;
    return true;
  };
  // A plane that slides: the node's range comes to the host, std::nth_element runs on (coordinate, index) pairs -- the
  // comparisons, and with them the permutation, are those of the builder's nth_element on the indices -- and goes back.
  std::vector<int> slid;
  std::vector<std::pair<float, int>> keyed;
  unsigned n_slides = 0;
  auto slide = [&](internal::top_segment<float>& seg, size_t nth) -> bool {
    ++did.slides;
    if (++n_slides > 64) {  // (a pile of coincident outliers peels one point per level: the host builder's business)
      reason = "too many sliding planes in the top levels";
      return false;
    }
    const auto t_in = std::chrono::steady_clock::now();
    struct on_exit {
      double& sum;
      std::chrono::steady_clock::time_point t0;
      ~on_exit() { sum += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    } timer{slide_ms, t_in};
    const uint32_t axis = seg.axis;
    // The rounds of libstdc++'s introselect while the range is large (see slide_pivot_kernel): on the device.
    constexpr size_t kHostBelow = 32768;
    // (The device rounds replay libstdc++'s std::nth_element and hand what is left to its std::__introselect -- internals
    // whose shape is pinned to the releases this was checked against.  Any other standard library, or a libstdc++ from
    // after them, takes the whole range to the host's std::nth_element below: the same permutation, no device rounds.)
#if defined(__GLIBCXX__) && defined(_GLIBCXX_RELEASE) && _GLIBCXX_RELEASE >= 9 && _GLIBCXX_RELEASE <= 15
    constexpr bool kKnownIntroselect = true;
#else
    constexpr bool kKnownIntroselect = false;
#endif
    if (kKnownIntroselect && seg.end - seg.begin > kHostBelow && knob_int("device_slide_off", 0) == 0) {
      size_t first = seg.begin, last = seg.end;
      const size_t nth_pos = seg.begin + nth;
      long depth_limit = 2 * (long)std::__lg((long)(last - first));
      if (b.flags64 == nullptr) {
        if (!ok(rocprim::exclusive_scan(nullptr, b.scan_bytes64, b.flags64, b.sums64, 0ull, (size_t)n + 1,
                                        rocprim::plus<unsigned long long>(), (hipStream_t) nullptr)) ||
            !ok(hipMalloc((void**)&b.flags64, (n + 1) * 8)) || !ok(hipMalloc((void**)&b.sums64, (n + 1) * 8)) ||
            !ok(hipMalloc(&b.scan_tmp64, b.scan_bytes64 + 256)) || !ok(hipMalloc((void**)&b.pivot, 16)))
          return false;
      }
      uint32_t* d_cut = reinterpret_cast<uint32_t*>(b.pivot) + 1;
      while (last - first > kHostBelow && depth_limit > 0) {
        --depth_limit;
        ++did.slide_rounds_device;
        const uint32_t lo = (uint32_t)first + 1u, hi = (uint32_t)last, n_range = hi - lo;
        const uint32_t none = 0xFFFFFFFFu;
        if (!ok(hipMemcpyAsync(d_cut, &none, 4, hipMemcpyHostToDevice, nullptr))) return false;
        hipLaunchKernelGGL(slide_pivot_kernel, dim3(1), dim3(1), 0, nullptr, b.pts, dim, axis, b.idx, (uint32_t)first,
                           (uint32_t)last, b.pivot);
        hipLaunchKernelGGL(slide_flag_kernel, dim3(n_range / 256u + 1u), dim3(256), 0, nullptr, b.pts, dim, axis, b.idx, lo,
                           hi, b.pivot, b.flags64);
        size_t bytes = b.scan_bytes64 + 256;
        if (!ok(rocprim::exclusive_scan(b.scan_tmp64, bytes, b.flags64, b.sums64, 0ull, (size_t)n_range + 1,
                                        rocprim::plus<unsigned long long>(), (hipStream_t) nullptr)))
          return false;
        hipLaunchKernelGGL(slide_list_kernel, dim3(n_range / 256u + 1u), dim3(256), 0, nullptr, b.flags64, b.sums64, lo, hi,
                           b.from_left, b.from_right);
        hipLaunchKernelGGL(slide_pair_kernel, dim3((n_range + 1u) / 256u + 1u), dim3(256), 0, nullptr, b.idx, b.sums64,
                           n_range, b.from_left, b.from_right, d_cut);
        if (!ok(hipGetLastError())) return false;
        uint32_t cut = none;
        if (!ok(hipMemcpy(&cut, d_cut, 4, hipMemcpyDeviceToHost))) return false;
        if (cut == none || cut < lo || cut > hi) {
          reason = "the partition of a sliding step found no cut";
          return false;
        }
        if (cut <= nth_pos) first = cut;
        else last = cut;
      }
      // What is left of the same call, on the host: the range that still holds nth, the depth limit that is left.
      const size_t count = last - first;
      slid.resize(count);
      if (!ok(hipMemcpy(slid.data(), b.idx + first, count * 4, hipMemcpyDeviceToHost))) return false;
      auto below = [&](int x, int y) { return points[(size_t)x * dim + axis] < points[(size_t)y * dim + axis]; };
#if defined(__GLIBCXX__) && defined(_GLIBCXX_RELEASE) && _GLIBCXX_RELEASE >= 9 && _GLIBCXX_RELEASE <= 15
      std::__introselect(slid.begin(), slid.begin() + (nth_pos - first), slid.end(), depth_limit,
                         __gnu_cxx::__ops::__iter_comp_iter(below));
#else
      (void)below;
      reason = "the device rounds of a sliding step need libstdc++'s introselect";
      return false;
#endif
      seg.plane = points[(size_t)slid[nth_pos - first] * dim + axis];
      return ok(hipMemcpy(b.idx + first, slid.data(), count * 4, hipMemcpyHostToDevice));
    }
    ++did.slides_host_whole;
    const size_t count = seg.end - seg.begin;
    slid.resize(count);
    keyed.resize(count);
    if (!ok(hipMemcpy(slid.data(), b.idx + seg.begin, count * 4, hipMemcpyDeviceToHost))) return false;
    auto fill = [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) keyed[i] = std::make_pair(points[(size_t)slid[i] * dim + axis], slid[i]);
    };
    const unsigned workers = (unsigned)std::min<size_t>(std::max(1u, threads), count / 65536 + 1);
    if (workers > 1) {
      std::vector<std::thread> pool;
      const size_t per = (count + workers - 1) / workers;
      for (unsigned w = 1; w < workers; ++w) pool.emplace_back(fill, std::min(count, per * w), std::min(count, per * (w + 1)));
      fill(0, std::min(count, per));
      for (auto& t : pool) t.join();
    } else {
      fill(0, count);
    }
    std::nth_element(keyed.begin(), keyed.begin() + nth, keyed.end(),
                     [](const std::pair<float, int>& x, const std::pair<float, int>& y) { return x.first < y.first; });
    for (size_t i = 0; i < count; ++i) slid[i] = keyed[i].second;
    seg.plane = keyed[nth].first;
    return ok(hipMemcpy(b.idx + seg.begin, slid.data(), count * 4, hipMemcpyHostToDevice));
  };
  std::vector<internal::top_branch<float>> top;
  std::vector<std::pair<size_t, size_t>> frontier;
  reason = "a level of the top failed";
  if (!internal::split_top_levels(root, (size_t)n, threshold, on_device, slide, top, frontier)) return false;
  did.top_branches = top.size();
  did.subtrees = frontier.size();
  lap("levels (slides included)");
  if (verbose) std::fprintf(stderr, "[ptk build]   %-34s %8.2f ms (%zu top branches, %zu subtrees)\n", "of which slides", slide_ms, top.size(), frontier.size());
  std::vector<int> indices(n);
  if (!ok(hipMemcpy(indices.data(), b.idx, n * 4, hipMemcpyDeviceToHost))) return false;
  lap("permutation to the host");
  const auto t_top = std::chrono::steady_clock::now();
  double below_ms[2] = {0, 0};
  tree = internal::build_flat_tree_below<int>(view, max_leaf_size_t(max_leaf_size), sliding_midpoint_max_side, root,
                                              std::move(indices), top, frontier, true, threads, below_ms);
  if (verbose) std::fprintf(stderr, "[ptk build]   %-34s %8.2f ms\n[ptk build]   %-34s %8.2f ms\n", "subtrees (workers)", below_ms[0], "splice", below_ms[1]);
  if (phase_ms != nullptr) {
    phase_ms[0] = std::chrono::duration<double, std::milli>(t_top - t_start).count();
    phase_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_top).count();
  }
  did.on_device = 1;
  reason = "";
  return true;
}

}  // namespace ptk
