// tests/cpp/emulate_mst.cpp -- TEST INFRASTRUCTURE: the kernels of mst_within_self
// (pico_tree_amd/csrc/ptk_kernels_mst.hpp: the component table, the search, the tie, emit and relabel passes) run lane by
// lane on the CPU, on the emulator of tests/cpp/emulate_kernels.cpp with the handles and side tables of
// tests/cpp/emulate_radius_self.cpp.  Built by tests/test_mst_self.py with the emulator's g++ line and HIP stand-in.
//
// No kernel of the round votes or waits, so lanes run one after the other.  Two schedules of what a lane SEES in a cell
// other lanes write during the same kernel (the union-find's parents, the best_wlo cells), which must give the same
// edges:
//   live      the cell as it is: a lane sees what every lane before it in the kernel has stored;
//   snapshot  the cell as it was when the kernel started -- the stalest view the memory model allows (a kernel boundary
//             makes everything before it visible): the stand-in of the agent-scope load below reads a copy taken before
//             the kernel; compare-and-swap, atomicMin and the stores go to the live array.
// The rounds are driven as ptk_mst_within_self_device drives them (ptk_backend.hip, ptkf::mst_rounds).

#include "emulate_radius_self.cpp"

namespace {
struct Shadow {
  const char* live = nullptr;
  std::vector<char> copy;
  bool on = false;
};
Shadow g_shadow[2];  // the parents, the best_wlo cells

void shadow_take(int which, const void* live, size_t bytes, bool on) {
  Shadow& s = g_shadow[which];
  s.live = static_cast<const char*>(live);
  s.on = on;
  if (on) s.copy.assign(s.live, s.live + bytes);
}
void shadow_off() { g_shadow[0].on = g_shadow[1].on = false; }
}  // namespace

#define __HIP_MEMORY_SCOPE_AGENT 4
template <class T>
inline T __hip_atomic_load(const T* p, int, int) {
  const char* c = reinterpret_cast<const char*>(p);
  for (const Shadow& s : g_shadow) {
    if (s.on && c >= s.live && c < s.live + s.copy.size()) {
      T v;
      std::memcpy(&v, s.copy.data() + (c - s.live), sizeof v);
      return v;
    }
  }
  return *p;
}
template <class T>
inline T atomicCAS(T* p, T expected, T wanted) {
  const T old = *p;
  if (old == expected) *p = wanted;
  return old;
}
template <class T>
inline T atomicMin(T* p, T v) {
  const T old = *p;
  if (v < old) *p = v;
  return old;
}

#include "ptk_kernels_mst.hpp"

namespace {

template <class M, bool CORE>
int mst_m(Emu* t, uint64_t piece, float radius, const float* core, uint32_t skip, int snapshot, ptk::MstEdge* edges,
          int32_t* labels, uint32_t* n_edges, uint32_t* stats) {
  const uint64_t n = t->dev.n_points;
  // (a tree whose root is a leaf has no branch and no component table: the encoder keeps one padding record there)
  const uint32_t nb = (t->dev.root_ref & ptk::kLeafBit) ? 0u : (uint32_t)t->enc.nodes.size();
  const std::vector<ptk::CountBox> table = nb > 0 ? table_of(t) : std::vector<ptk::CountBox>(1);
  std::vector<int32_t> parent(n), label(n);
  std::vector<uint2> cand(n);
  std::vector<unsigned long long> best_wlo(n);
  std::vector<uint32_t> best_hi(n), comp(nb > 0 ? nb : 1, ptk::kMstMixed), info(nb > 0 ? nb : 1), arrive(nb > 0 ? nb : 1);
  uint32_t count = 7;
  for_each_lane(n, [&] { ptk::mst_init_kernel(n, parent.data(), label.data(), best_wlo.data(), best_hi.data(), &count); }, 256);
  if (nb > 0) for_each_lane(nb, [&] { ptk::count_parents_kernel(t->dev, nb, info.data(), arrive.data()); }, 256);
  uint32_t rounds = 0, added = 1;
  uint64_t total = 0;
  while (added != 0 && total + 1 < n && rounds < n) {
    added = 0;
    if (rounds > 0 && skip != 0 && nb > 0) {
      std::fill(arrive.begin(), arrive.end(), 0u);
      std::fill(comp.begin(), comp.end(), 0xDEADBEEFu);  // (every entry has to be written by the climb)
      for_each_lane(nb, [&] { ptk::mst_table_kernel(t->dev, nb, info.data(), arrive.data(), label.data(), comp.data()); }, 256);
      for (uint32_t v : comp)
        if (v == 0xDEADBEEFu) return -2;
    }
    for (uint64_t first = 0; first < n; first += piece) {
      const uint64_t m = std::min(piece, n - first);
      shadow_take(1, best_wlo.data(), n * sizeof(unsigned long long), snapshot != 0);
      for_each_lane(m, [&] {
        ptk::mst_search_kernel<16, 2048, 64, 5, CORE, M>(t->dev, table.data(), comp.data(), t->dim, first, m, radius, core,
                                                         label.data(), skip, cand.data(), best_wlo.data(), stats);
      }, 64);
      shadow_off();
    }
    for_each_lane(n, [&] { ptk::mst_tie_kernel(n, cand.data(), label.data(), best_wlo.data(), best_hi.data()); }, 256);
    shadow_take(0, parent.data(), n * sizeof(int32_t), snapshot != 0);
    for_each_lane(n, [&] {
      ptk::mst_emit_kernel(n, cand.data(), label.data(), best_wlo.data(), best_hi.data(), parent.data(), edges,
                           (uint32_t)(n - 1), &count, &added);
    }, 256);
    shadow_off();
    shadow_take(0, parent.data(), n * sizeof(int32_t), snapshot != 0);
    for_each_lane(n, [&] { ptk::mst_relabel_kernel(n, parent.data(), label.data(), best_wlo.data(), best_hi.data()); }, 256);
    shadow_off();
    total += added;
    ++rounds;
  }
  if (count != total) return -3;
  *n_edges = count;
  std::copy(label.begin(), label.end(), labels);
  return (int)rounds;
}

template <class M>
int mst_any(Emu* t, uint64_t piece, float radius, const float* core, uint32_t skip, int snapshot, ptk::MstEdge* edges,
            int32_t* labels, uint32_t* n_edges, uint32_t* stats) {
  if (core != nullptr) return mst_m<M, true>(t, piece, radius, core, skip, snapshot, edges, labels, n_edges, stats);
  return mst_m<M, false>(t, piece, radius, core, skip, snapshot, edges, labels, n_edges, stats);
}

}  // namespace

extern "C" {

// The edges (n_points - 1 records at most, in the order the lanes wrote them), the labels and the number of edges of the
// rounds over every leaf position, `piece` positions per launch (0: all at once); core null: the plain weight; skip: the
// `skip` argument of the search; snapshot != 0: the stale schedule.  stats[3]: subtrees skipped by the component table,
// by the box, and leaf records looked at, over all rounds.  Returns the rounds run; -1 for a handle the kernels do not
// take, -2 if the climb left a table entry unwritten, -3 if the count and the rounds' sums differ.
int emu_mst_self(void* h, uint64_t piece, float radius, const float* core, uint32_t skip, int snapshot, void* edges,
                 int32_t* labels, uint32_t* n_edges, uint32_t* stats) {
  auto* t = static_cast<Emu*>(h);
  auto* e = static_cast<ptk::MstEdge*>(edges);
  stats[0] = stats[1] = stats[2] = 0;
  *n_edges = 0;
  if (t->dim > 3) return -1;
  if (t->dev.n_points == 0) return 0;
  if (piece == 0) piece = t->dev.n_points;
  switch (t->metric) {
    case 1: return mst_any<ptk::MetricL1>(t, piece, radius, core, skip, snapshot, e, labels, n_edges, stats);
    case 0: return mst_any<ptk::MetricL2>(t, piece, radius, core, skip, snapshot, e, labels, n_edges, stats);
    default: return -1;
  }
}

}  // extern "C"
