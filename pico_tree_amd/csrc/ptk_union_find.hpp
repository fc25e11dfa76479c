// ptk_union_find.hpp -- the lock-free union-find of cluster_within_self (ptk_kernels_cluster.hpp),
// written once over a memory-ops parameter: the kernels run it over int32_t cells with device atomics, the emulator over
// host stand-ins of those, tests/cpp/cluster_threads.cpp over std::atomic<int32_t> on 16 host threads.
//
//   Mem::load(const Cell*)            a relaxed atomic load that other agents' writes reach (never a cached stale line)
//   Mem::cas(Cell*, expected, wanted) compare-and-swap, returns the value found
//   Mem::min(Cell*, v)                atomic minimum
//
// parent[] lives over original point indices.  Invariant: 0 <= parent[x] <= x for every cell the functions are given
// (the callers never pass a cell with a negative mark).  The only write that joins two trees replaces a ROOT's self-link
// by a smaller index -- cas(&parent[hi], hi, lo) with lo < hi -- so links only ever point downwards: there are no
// cycles, a find ends after at most x steps, and the root of a finished component is its smallest index.  A failed CAS
// means that another caller has linked that root meanwhile, i.e. made progress; the loser re-finds from the value it
// was handed and tries again.  Nobody ever waits for anybody: no locks, no flags.
// COMPRESS: path halving by Mem::min(&parent[x], grandparent) -- monotone, so safe under any interleaving (a cell only
// ever moves to one of its ancestors).
#pragma once

#include <cstdint>

#ifndef PTK_UF_FN
#define PTK_UF_FN __device__ __forceinline__
#endif

namespace ptk {

template <class Mem, bool COMPRESS, class Cell>
PTK_UF_FN int32_t uf_find(Cell* parent, int32_t x) {
  int32_t p = Mem::load(parent + x);
  while (p != x) {
    const int32_t g = Mem::load(parent + p);
    if (COMPRESS && g != p) (void)Mem::min(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// Joins the components of a and b; returns the root both had when the call saw them joined (an ancestor of either from
// then on: a good place for the caller's next find to start).
template <class Mem, bool COMPRESS, class Cell>
PTK_UF_FN int32_t uf_unite(Cell* parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find<Mem, COMPRESS>(parent, a);
    b = uf_find<Mem, COMPRESS>(parent, b);
    if (a == b) return a;
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const int32_t found = Mem::cas(parent + hi, hi, lo);
    if (found == hi) return lo;
    a = found;  // (hi is no root any more: `found` is where it points, below hi)
    b = lo;
  }
}

}  // namespace ptk
