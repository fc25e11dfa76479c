// tests/cpp/emulate_build_main.cpp -- TEST INFRASTRUCTURE (tests/test_build_emulation.py): the kernels of the device
// tree build (pico_tree_amd/csrc/ptk_kernels_build.hpp) run lane by lane on the CPU, on the emulator of
// tests/cpp/emulate_kernels.cpp (its lane and block schedulers: all this unit takes from it), in the launch sequence of the two
// callbacks of ptk::device_top_build (ptk_build.hpp) -- restated here with std::exclusive_scan in place of rocprim --
// and checked step by step against the plain standard-library operation on a copy of the same input:
//
//   every level   each segment's range and cut against std::partition(coordinate < plane), position for position;
//                 the positions that belong to no segment are left alone
//   every slide   the range against std::nth_element(begin, begin + nth, end) by the coordinate of the axis, position
//                 for position, and the plane against the coordinate at begin + nth
//   the end       build_flat_tree_below() over the emulated top against build_flat_tree(..., 1 thread)
//   the root box  the reduction of build_box_kernel against a plain loop
//
//   emulate_build_main POINTS n dim leaf threshold host_below [box_blocks]
//
// POINTS: n * dim float32, raw.  `threshold` (nodes above it are split here) and `host_below` (a sliding range above it
// gets the device rounds; 32 768 in the driver) are parameters, so that the slide kernels run on ranges of tens of
// elements; `box_blocks`: the grid of build_box_kernel (the driver's 1 024 by default).  Prints one JSON line of the
// counters of ptk_debug_create_route -- plus how often each of the six outcomes of slide_pivot_kernel's median of three
// applied -- and exits 0; exits 1 on the first difference, naming the level and the segment.  A refusal of the driver
// (more than 64 sliding planes) is no difference: "on_device": 0 with its reason, exit 0.

#define PTK_EMU_SCHEDULERS_ONLY
#include "emulate_kernels.cpp"

#include "pico_tree/internal/flat_tree.hpp"
#include "pico_tree/map.hpp"

// A `__shared__` array of a kernel is one per block: the threads of a block are fibers of one host thread and the blocks
// run one after the other (for_each_block), so a function-local static is exactly that.  (The stand-in's empty
// definition serves the kernels that carve their LDS out of ptk_smem.)
#undef __shared__
#define __shared__ static
#include "ptk_kernels_build.hpp"
#undef __shared__
#define __shared__

#include <cstdarg>
#include <numeric>

// (the device rounds of a slide are followed by libstdc++'s std::__introselect: the guard of ptk_build.hpp)
#if defined(__GLIBCXX__) && defined(_GLIBCXX_RELEASE) && _GLIBCXX_RELEASE >= 9 && _GLIBCXX_RELEASE <= 15
constexpr bool kKnownIntroselect = true;
#else
constexpr bool kKnownIntroselect = false;
#endif

namespace {

[[noreturn]] void differ(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::fprintf(stderr, "emulate_build: ");
  std::vfprintf(stderr, fmt, ap);
  std::fprintf(stderr, "\n");
  va_end(ap);
  std::exit(1);
}

// One launch of a kernel whose threads are independent: `blocks` blocks of `block` threads.
template <typename F>
void launch(uint32_t blocks, uint32_t block, F&& f) {
  for_each_lane((uint64_t)blocks * block, f, block);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: %s POINTS n dim leaf threshold host_below [box_blocks]\n", argv[0]);
    return 2;
  }
  const size_t n = std::strtoull(argv[2], nullptr, 10);
  const uint32_t dim = (uint32_t)std::strtoul(argv[3], nullptr, 10);
  const size_t leaf = std::strtoull(argv[4], nullptr, 10);
  const size_t threshold = std::strtoull(argv[5], nullptr, 10);
  const size_t host_below = std::strtoull(argv[6], nullptr, 10);
  const uint32_t box_blocks = argc > 7 ? (uint32_t)std::strtoul(argv[7], nullptr, 10) : ptk::kBuildBoxBlocks;
  if (dim == 0 || dim > ptk::kBuildMaxDim || n < 2 || n >= (1ull << 31) || leaf == 0 || threshold < leaf || box_blocks == 0) {
    std::fprintf(stderr, "emulate_build: arguments out of range\n");
    return 2;
  }
  std::vector<float> pts_v(n * dim);
  {
    std::FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr || std::fread(pts_v.data(), sizeof(float), pts_v.size(), f) != pts_v.size()) {
      std::fprintf(stderr, "emulate_build: cannot read %zu floats from %s\n", pts_v.size(), argv[1]);
      return 2;
    }
    std::fclose(f);
  }
  const float* pts = pts_v.data();
  const uint32_t n32 = (uint32_t)n;

  using namespace pico_tree;
  using space_t = space_map<point_map<float const, dynamic_extent>>;
  using tree_t = internal::flat_tree<int, float, dynamic_extent>;
  using box_type = tree_t::box_type;
  space_t space(pts, n, dim);
  internal::space_view<space_t> view(space);

  // The buffers of ptk::BuildBuffers, each of exactly the size the driver allocates (a sanitized build of this program
  // sees a write past any of them).  What the device leaves uninitialised is poisoned: an index no buffer has.
  constexpr uint32_t kPoison = 0xFFFFFFFFu;
  std::vector<int32_t> idx(n, (int32_t)kPoison);
  std::vector<uint32_t> flags(n + 1, kPoison), sums(n + 1, kPoison), from_left(n, kPoison), from_right(n, kPoison);
  std::vector<unsigned long long> flags64(n + 1, ~0ull), sums64(n + 1, ~0ull);
  std::vector<float> partial((size_t)box_blocks * dim * 2, -7.0f);
  struct {
    float pivot;
    uint32_t cut;
  } cell = {0.0f, 0u};  // the driver's 16 bytes: {pivot value, cut}

  const uint32_t blocks = (n32 + 256u) / 256u;  // covers position n as well
  launch(blocks, 256, [&] { ptk::build_iota_kernel(idx.data(), n32); });
  for (size_t i = 0; i < n; ++i)
    if (idx[i] != (int32_t)i) differ("build_iota_kernel: idx[%zu] = %d", i, idx[i]);
  for_each_block(box_blocks, 256, [&] { ptk::build_box_kernel(pts, n32, dim, partial.data()); });
  box_type root(dim);
  root.invert();
  for (uint32_t blk = 0; blk < box_blocks; ++blk)
    for (uint32_t a = 0; a < dim; ++a) {
      const float lo = partial[((size_t)blk * dim + a) * 2], hi = partial[((size_t)blk * dim + a) * 2 + 1];
      if (lo < root.min(a)) root.min(a) = lo;
      if (hi > root.max(a)) root.max(a) = hi;
    }
  for (uint32_t a = 0; a < dim; ++a) {  // the box of a plain loop
    float lo = pts[a], hi = pts[a];
    for (size_t i = 1; i < n; ++i) {
      lo = std::min(lo, pts[i * dim + a]);
      hi = std::max(hi, pts[i * dim + a]);
    }
    if (std::memcmp(&lo, &root.min(a), 4) != 0 || std::memcmp(&hi, &root.max(a), 4) != 0)
      differ("build_box_kernel: axis %u is [%a, %a], a plain loop finds [%a, %a]", a, (double)root.min(a), (double)root.max(a),
             (double)lo, (double)hi);
  }

  // ---- the counters of ptk::BuildRoute, and what the sweep of the test wants to have seen -------------------------
  const char* why = "";
  unsigned long long levels = 0, slides = 0, slide_rounds_device = 0, slides_host_whole = 0;
  unsigned long long pivot_outcomes[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long max_level_segments = 0, max_level_unsegmented = 0, segments_no_swap = 0, segments_all_swap = 0,
                     max_round_equal_to_pivot = 0;
  const size_t max_segs = 2 * (n / threshold) + 64;

  std::vector<ptk::BuildSeg> segs;
  std::vector<int32_t> want;
  auto on_device = [&](std::vector<internal::top_segment<float>>& segments) -> bool {
    ++levels;
    if (segments.size() > max_segs) {
      why = "more nodes in a level than planned for";
      return false;
    }
    const uint32_t nsegs = (uint32_t)segments.size();
    segs.resize(nsegs);
    for (uint32_t s = 0; s < nsegs; ++s)
      segs[s] = ptk::BuildSeg{(uint32_t)segments[s].begin, (uint32_t)segments[s].end, segments[s].axis, segments[s].plane, 0, 0, 0, 0};
    want = idx;
    std::fill(from_left.begin(), from_left.end(), kPoison);
    std::fill(from_right.begin(), from_right.end(), kPoison);
    launch(blocks, 256, [&] { ptk::build_flag_kernel(pts, dim, idx.data(), segs.data(), nsegs, n32, flags.data()); });
    std::exclusive_scan(flags.begin(), flags.end(), sums.begin(), 0u);
    launch((nsegs + 63) / 64, 64, [&] { ptk::build_cut_kernel(sums.data(), segs.data(), nsegs); });
    launch(blocks, 256, [&] {
      ptk::build_list_kernel(flags.data(), sums.data(), segs.data(), nsegs, n32, from_left.data(), from_right.data());
    });
    launch(blocks, 256, [&] { ptk::build_swap_kernel(idx.data(), segs.data(), nsegs, n32, from_left.data(), from_right.data()); });
    for (uint32_t s = 0; s < nsegs; ++s) segments[s].cut = segments[s].begin + segs[s].m;
    // std::partition of every segment on the copy; everything else stays
    size_t covered = 0;
    for (uint32_t s = 0; s < nsegs; ++s) {
      const auto& g = segments[s];
      const uint32_t a = g.axis;
      const float p = g.plane;
      const size_t cut = (size_t)(std::partition(want.begin() + g.begin, want.begin() + g.end,
                                                 [&](int i) { return pts[(size_t)i * dim + a] < p; }) - want.begin());
      if (cut != g.cut)
        differ("level %llu, segment %u [%zu, %zu) axis %u plane %a: cut %zu, std::partition returns %zu", levels, s, g.begin, g.end,
               a, (double)p, g.cut, cut);
      for (size_t i = g.begin; i < g.end; ++i)
        if (idx[i] != want[i])
          differ("level %llu, segment %u [%zu, %zu) axis %u plane %a: position %zu holds %d, std::partition leaves %d", levels, s,
                 g.begin, g.end, a, (double)p, i, idx[i], want[i]);
      covered += g.end - g.begin;
      const size_t m = segs[s].m, swaps = m - segs[s].pass_left, len = g.end - g.begin;
      if (swaps == 0) ++segments_no_swap;
      if (swaps > 0 && swaps == std::min(m, len - m)) ++segments_all_swap;
    }
    if (idx != want) differ("level %llu: a position outside every segment has changed", levels);
    max_level_segments = std::max<unsigned long long>(max_level_segments, nsegs);
    max_level_unsegmented = std::max<unsigned long long>(max_level_unsegmented, n - covered);
    return true;
  };

  std::vector<int> slid;
  std::vector<std::pair<float, int>> keyed;
  unsigned n_slides = 0;
  auto slide = [&](internal::top_segment<float>& seg, size_t nth) -> bool {
    ++slides;
    if (++n_slides > 64) {
      why = "too many sliding planes in the top levels";
      return false;
    }
    const uint32_t axis = seg.axis;
    auto below = [&](int x, int y) { return pts[(size_t)x * dim + axis] < pts[(size_t)y * dim + axis]; };
    want = idx;
    std::nth_element(want.begin() + seg.begin, want.begin() + seg.begin + nth, want.begin() + seg.end, below);
    if (kKnownIntroselect && seg.end - seg.begin > host_below) {
      size_t first = seg.begin, last = seg.end;
      const size_t nth_pos = seg.begin + nth;
      long depth_limit = 2 * (long)std::__lg((long)(last - first));
      uint32_t* d_cut = &cell.cut;
      while (last - first > host_below && depth_limit > 0) {
        --depth_limit;
        ++slide_rounds_device;
        const uint32_t lo = (uint32_t)first + 1u, hi = (uint32_t)last, n_range = hi - lo;
        const uint32_t none = 0xFFFFFFFFu;
        *d_cut = none;
        {  // which of the six outcomes of the median of three applies (recomputed: __move_median_to_first)
          auto val = [&](size_t i) { return pts[(size_t)idx[i] * dim + axis]; };
          const float va = val(first + 1), vb = val(first + (last - first) / 2), vc = val(last - 1);
          const int outcome = va < vb ? (vb < vc ? 0 : (va < vc ? 1 : 2)) : (va < vc ? 3 : (vb < vc ? 4 : 5));
          ++pivot_outcomes[outcome];
        }
        std::fill(from_left.begin(), from_left.end(), kPoison);
        std::fill(from_right.begin(), from_right.end(), kPoison);
        launch(1, 1, [&] { ptk::slide_pivot_kernel(pts, dim, axis, idx.data(), (uint32_t)first, (uint32_t)last, &cell.pivot); });
        launch(n_range / 256u + 1u, 256, [&] {
          ptk::slide_flag_kernel(pts, dim, axis, idx.data(), lo, hi, &cell.pivot, flags64.data());
        });
        std::exclusive_scan(flags64.begin(), flags64.begin() + n_range + 1, sums64.begin(), 0ull);
        launch(n_range / 256u + 1u, 256, [&] {
          ptk::slide_list_kernel(flags64.data(), sums64.data(), lo, hi, from_left.data(), from_right.data());
        });
        launch((n_range + 1u) / 256u + 1u, 256, [&] {
          ptk::slide_pair_kernel(idx.data(), sums64.data(), n_range, from_left.data(), from_right.data(), d_cut);
        });
        const uint32_t cut = *d_cut;
        if (cut == none || cut < lo || cut > hi) {
          why = "the partition of a sliding step found no cut";
          differ("slide %llu (level %llu), segment [%zu, %zu) nth %zu, round over [%zu, %zu): no cut (%u)", slides, levels, seg.begin,
                 seg.end, nth, first, last, cut);
        }
        unsigned long long equal = 0;
        for (uint32_t i = lo; i < hi; ++i) equal += pts[(size_t)idx[i] * dim + axis] == cell.pivot ? 1u : 0u;
        max_round_equal_to_pivot = std::max(max_round_equal_to_pivot, equal);
        if (cut <= nth_pos) first = cut;
        else last = cut;
      }
      const size_t count = last - first;
      slid.assign(idx.begin() + first, idx.begin() + first + count);
#if defined(__GLIBCXX__) && defined(_GLIBCXX_RELEASE) && _GLIBCXX_RELEASE >= 9 && _GLIBCXX_RELEASE <= 15
      std::__introselect(slid.begin(), slid.begin() + (nth_pos - first), slid.end(), depth_limit,
                         __gnu_cxx::__ops::__iter_comp_iter(below));
#endif
      seg.plane = pts[(size_t)slid[nth_pos - first] * dim + axis];
      std::copy(slid.begin(), slid.end(), idx.begin() + first);
    } else {
      ++slides_host_whole;
      const size_t count = seg.end - seg.begin;
      slid.assign(idx.begin() + seg.begin, idx.begin() + seg.end);
      keyed.resize(count);
      for (size_t i = 0; i < count; ++i) keyed[i] = std::make_pair(pts[(size_t)slid[i] * dim + axis], slid[i]);
      std::nth_element(keyed.begin(), keyed.begin() + nth, keyed.end(),
                       [](const std::pair<float, int>& x, const std::pair<float, int>& y) { return x.first < y.first; });
      for (size_t i = 0; i < count; ++i) slid[i] = keyed[i].second;
      seg.plane = keyed[nth].first;
      std::copy(slid.begin(), slid.end(), idx.begin() + seg.begin);
    }
    for (size_t i = 0; i < n; ++i)
      if (idx[i] != want[i])
        differ("slide %llu (level %llu), segment [%zu, %zu) axis %u nth %zu: position %zu holds %d, std::nth_element leaves %d%s",
               slides, levels, seg.begin, seg.end, axis, nth, i, idx[i], want[i],
               i < seg.begin || i >= seg.end ? " (outside the range)" : "");
    const float at_nth = pts[(size_t)want[seg.begin + nth] * dim + axis];
    if (std::memcmp(&at_nth, &seg.plane, 4) != 0)
      differ("slide %llu (level %llu), segment [%zu, %zu) nth %zu: plane %a, the coordinate at begin + nth is %a", slides, levels,
             seg.begin, seg.end, nth, (double)seg.plane, (double)at_nth);
    return true;
  };

  std::vector<internal::top_branch<float>> top;
  std::vector<std::pair<size_t, size_t>> frontier;
  const bool done = internal::split_top_levels(root, n, threshold, on_device, slide, top, frontier);
  if (done) {
    auto ref = internal::build_flat_tree<int>(view, max_leaf_size_t(leaf), bounds_from_space, sliding_midpoint_max_side, true, 1);
    std::vector<int> indices(idx.begin(), idx.end());
    auto got = internal::build_flat_tree_below<int>(view, max_leaf_size_t(leaf), sliding_midpoint_max_side, root, std::move(indices),
                                                    top, frontier, true, 2);
    if (ref.nodes.size() != got.nodes.size() ||
        std::memcmp(ref.nodes.data(), got.nodes.data(), ref.nodes.size() * sizeof(ref.nodes[0])) != 0)
      differ("the tree below the emulated top: nodes differ (%zu, the host builder makes %zu)", got.nodes.size(), ref.nodes.size());
    if (ref.indices != got.indices) differ("the tree below the emulated top: indices differ");
    if (ref.outer_bounds != got.outer_bounds) differ("the tree below the emulated top: outer bounds differ");
    if (ref.max_depth != got.max_depth || ref.leaf_count != got.leaf_count || ref.max_leaf_points != got.max_leaf_points)
      differ("the tree below the emulated top: max_depth %u / %u, leaf_count %zu / %zu, max_leaf_points %zu / %zu", got.max_depth,
             ref.max_depth, got.leaf_count, ref.leaf_count, got.max_leaf_points, ref.max_leaf_points);
  }
  std::printf(
      "{\"on_device\": %d, \"why\": \"%s\", \"threshold\": %zu, \"levels\": %llu, \"top_branches\": %zu, \"subtrees\": %zu, "
      "\"slides\": %llu, \"slide_rounds_device\": %llu, \"slides_host_whole\": %llu, \"pivot_outcomes\": [%llu, %llu, %llu, %llu, "
      "%llu, %llu], \"introselect_checked\": %d, \"max_level_segments\": %llu, \"max_level_unsegmented\": %llu, "
      "\"segments_no_swap\": %llu, \"segments_all_swap\": %llu, \"max_round_equal_to_pivot\": %llu}\n",
      done ? 1 : 0, done ? "" : why, threshold, levels, done ? top.size() : size_t(0), done ? frontier.size() : size_t(0), slides,
      slide_rounds_device, slides_host_whole, pivot_outcomes[0], pivot_outcomes[1], pivot_outcomes[2], pivot_outcomes[3],
      pivot_outcomes[4], pivot_outcomes[5], kKnownIntroselect ? 1 : 0, max_level_segments, max_level_unsegmented, segments_no_swap,
      segments_all_swap, max_round_equal_to_pivot);
  return 0;
}
