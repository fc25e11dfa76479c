// tests/cpp/emulate_suppress.cpp -- TEST INFRASTRUCTURE: the kernels of suppress_within_self
// (pico_tree_amd/csrc/ptk_kernels_suppress.hpp: suppress_init_kernel, suppress_round_kernel and its float64 twin) run on
// the CPU, on the emulator of tests/cpp/emulate_kernels.cpp with the handles of tests/cpp/emulate_radius_self.cpp.  Built
// by tests/test_suppress_self.py with the emulator's g++ line and HIP stand-in.
//
// The round kernel votes (__ballot) after its walk, so a wavefront runs as 64 fibers (each_wave below, the emulator's
// for_each_wave): every lane walks its row to the end, then the lanes that are still there meet at the vote.  Two
// schedules of what a lane SEES in another point's cell, which must give the same array:
//   live      the cell as it is: a lane sees what every lane before it in the round has stored;
//   snapshot  the cell as it was when the round started -- the stalest view the memory model allows (a kernel
//             boundary makes everything before it visible): the stand-in of the agent-scope load below reads the copy
//             taken before the round, the stores go to the live array.
// The rounds are driven as ptkf::suppress_rounds drives them: zero the counter, one round over all pieces, read it.

#include "emulate_radius_self.cpp"

namespace {
const uint8_t* g_live = nullptr;      // the cells of the call
const uint8_t* g_snapshot = nullptr;  // non-null: the copy the loads are served from
uint64_t g_cells = 0;
}  // namespace

#define __HIP_MEMORY_SCOPE_AGENT 4
inline uint8_t __hip_atomic_load(const uint8_t* p, int, int) {
  if (g_snapshot != nullptr && p >= g_live && p < g_live + g_cells) return g_snapshot[p - g_live];
  return *p;
}
inline void __hip_atomic_store(uint8_t* p, uint8_t v, int, int) { *p = v; }

#include "ptk_kernels_suppress.hpp"

namespace {

// for_each_wave of the emulator with ONE set of fiber stacks for the whole unit: a round over pieces of 64 positions is
// thousands of one-block launches, and for_each_wave allocates (and clears) 16 MB of stacks per call.  The body is
// told its block, f(block): the float64 kernels index their stacks by blockIdx.x and are given block 0 there.
template <typename F>
void each_wave(uint32_t blocks, F&& f) {
  static WaveFibers w;
  if (w.stacks.empty()) w.stacks.resize(WaveFibers::kLanes * WaveFibers::kStack);
  g_fibers = &w;
  gridDim.x = blocks;
  blockDim.x = 64;
  uint32_t block = 0;
  w.body = [&] { f(block); };
  for (uint32_t b = 0; b < blocks; ++b) {
    block = blockIdx.x = b;
    for (int l = 0; l < WaveFibers::kLanes; ++l) {
      w.done[l] = false;
      w.pred[l] = false;
      w.value[l] = 0;
      getcontext(&w.lane_ctx[l]);
      w.lane_ctx[l].uc_stack.ss_sp = w.stacks.data() + (size_t)l * WaveFibers::kStack;
      w.lane_ctx[l].uc_stack.ss_size = WaveFibers::kStack;
      w.lane_ctx[l].uc_link = &w.scheduler;
      makecontext(&w.lane_ctx[l], fiber_entry, 0);
    }
    for (;;) {  // every live lane up to its next vote (or to its end), then the vote's result to all of them
      int live = 0;
      for (int l = 0; l < WaveFibers::kLanes; ++l) {
        if (w.done[l]) continue;
        w.current = l;
        threadIdx.x = (uint32_t)l;
        swapcontext(&w.scheduler, &w.lane_ctx[l]);
        if (!w.done[l]) ++live;
      }
      if (live == 0) break;
      unsigned long long bits = 0;
      for (int l = 0; l < WaveFibers::kLanes; ++l) {
        if (!w.done[l] && w.pred[l]) bits |= 1ull << l;
      }
      w.result = bits;
    }
  }
  w.body = nullptr;
  g_fibers = nullptr;
}

// Rounds until one leaves nothing undecided; `round(undecided)` runs one over all pieces.  Returns the rounds run, or 0
// if n rounds did not end it (the bound of ptk.h).
template <class Round>
uint32_t rounds_of(uint64_t n, uint8_t* cells, int snapshot, Round&& round) {
  for_each_lane(n, [&] { ptk::suppress_init_kernel(n, cells); }, 256);
  std::vector<uint8_t> copy;
  g_live = cells;
  g_cells = n;
  uint32_t rounds = 0, undecided = 1;
  while (undecided != 0 && rounds < n) {
    if (snapshot) {
      copy.assign(cells, cells + n);
      g_snapshot = copy.data();
    }
    undecided = 0;
    round(&undecided);
    ++rounds;
  }
  g_snapshot = g_live = nullptr;
  return undecided == 0 ? rounds : 0;
}

template <class M, bool PER_ROW, bool SCORED>
uint32_t suppress_m(Emu* t, uint64_t piece, float radius, const float* radii, const float* scores, int snapshot,
                    uint8_t* cells) {
  const uint64_t n = t->dev.n_points;
  return rounds_of(n, cells, snapshot, [&](uint32_t* undecided) {
    for (uint64_t first = 0; first < n; first += piece) {
      const uint64_t m = std::min(piece, n - first);
      each_wave((uint32_t)((m + 63) / 64), [&](uint32_t) {
        ptk::suppress_round_kernel<16, 2048, 64, 5, PER_ROW, SCORED, M>(t->dev, t->dim, first, m, radius, radii, scores, cells,
                                                                       undecided);
      });
    }
  });
}

template <class M>
uint32_t suppress_any(Emu* t, uint64_t piece, float radius, const float* radii, const float* scores, int snapshot,
                      uint8_t* cells) {
  if (radii != nullptr && scores != nullptr) return suppress_m<M, true, true>(t, piece, radius, radii, scores, snapshot, cells);
  if (radii != nullptr) return suppress_m<M, true, false>(t, piece, radius, radii, scores, snapshot, cells);
  if (scores != nullptr) return suppress_m<M, false, true>(t, piece, radius, radii, scores, snapshot, cells);
  return suppress_m<M, false, false>(t, piece, radius, radii, scores, snapshot, cells);
}

// Float64: every block reuses stack columns [0, slots * 64), as for_each_lane64 -- the lanes of a block see blockIdx.x = 0
// and take their 64 leaf positions from the arguments, by the block each_wave names.
template <class M, bool PER_ROW, bool SCORED>
uint32_t suppress64_m(Emu64* t, uint64_t piece, double radius, const double* radii, const float* scores, int snapshot,
                      uint8_t* cells) {
  const uint64_t n = t->dev.n_points;
  return rounds_of(n, cells, snapshot, [&](uint32_t* undecided) {
    for (uint64_t first = 0; first < n; first += piece) {
      const uint64_t m = std::min(piece, n - first);
      each_wave((uint32_t)((m + 63) / 64), [&](uint32_t block) {
        const uint64_t q0 = (uint64_t)block * 64;
        blockIdx.x = 0;
        gridDim.x = 1;
        ptk::suppress64_round_kernel<M, PER_ROW, SCORED>(t->dev, first + q0, std::min<uint64_t>(64, m - q0), radius, radii,
                                                         scores, cells, undecided, t->stack.data(), t->slots);
      });
    }
  });
}

template <class M>
uint32_t suppress64_any(Emu64* t, uint64_t piece, double radius, const double* radii, const float* scores, int snapshot,
                        uint8_t* cells) {
  if (radii != nullptr && scores != nullptr) return suppress64_m<M, true, true>(t, piece, radius, radii, scores, snapshot, cells);
  if (radii != nullptr) return suppress64_m<M, true, false>(t, piece, radius, radii, scores, snapshot, cells);
  if (scores != nullptr) return suppress64_m<M, false, true>(t, piece, radius, radii, scores, snapshot, cells);
  return suppress64_m<M, false, false>(t, piece, radius, radii, scores, snapshot, cells);
}

}  // namespace

extern "C" {

// keep (n_points cells) of the rounds over every leaf position, `piece` positions per launch (0: all at once); radii
// null: the scalar form; scores null: the default order; snapshot != 0: the stale schedule.  Returns the rounds run, 0
// if the bound of n_points rounds was not enough, -1 for a handle the kernels do not take.
int emu_suppress_self(void* h, uint64_t piece, float radius, const float* radii, const float* scores, int snapshot,
                      uint8_t* keep) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3) return -1;
  if (t->dev.n_points == 0) return 0;
  if (piece == 0) piece = t->dev.n_points;
  switch (t->metric) {
    case 1: return (int)suppress_any<ptk::MetricL1>(t, piece, radius, radii, scores, snapshot, keep);
    case 2: return (int)suppress_any<ptk::MetricLInf>(t, piece, radius, radii, scores, snapshot, keep);
    case 3: return (int)suppress_any<ptk::MetricLNInf>(t, piece, radius, radii, scores, snapshot, keep);
    case 0: return (int)suppress_any<ptk::MetricL2>(t, piece, radius, radii, scores, snapshot, keep);
    default: return -1;
  }
}

int emu64_suppress_self(void* h, uint64_t piece, double radius, const double* radii, const float* scores, int snapshot,
                        uint8_t* keep) {
  auto* t = static_cast<Emu64*>(h);
  if (t->dev.dim > 3) return -1;
  if (t->dev.n_points == 0) return 0;
  if (piece == 0) piece = t->dev.n_points;
  switch (t->metric) {
    case 1: return (int)suppress64_any<ptk::Metric64L1>(t, piece, radius, radii, scores, snapshot, keep);
    case 2: return (int)suppress64_any<ptk::Metric64LInf>(t, piece, radius, radii, scores, snapshot, keep);
    case 3: return (int)suppress64_any<ptk::Metric64LNInf>(t, piece, radius, radii, scores, snapshot, keep);
    case 0: return (int)suppress64_any<ptk::Metric64L2>(t, piece, radius, radii, scores, snapshot, keep);
    default: return -1;
  }
}

}  // extern "C"
