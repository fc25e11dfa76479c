// tests/cpp/cluster_threads.cpp -- TEST PROGRAM: the lock-free union-find of cluster_within_self
// (pico_tree_amd/csrc/ptk_union_find.hpp, the source the kernels run) over std::atomic<int32_t> on 16 host threads.
// Built by tests/test_cluster_self.py with g++ -fsanitize=thread; a stand-alone program.
//
//   cluster_threads            both graphs, with and without path halving; exit status 0 and "threads ok" on success
//
// The 16 threads take the edges of a graph, in shuffled order, 64 at a time from a shared counter and unite their ends.
// Afterwards every cell's root must be the smallest index of its component, and the partition must equal a sequential
// union-find's over the same edges.

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#define PTK_UF_FN inline
#include "ptk_union_find.hpp"

namespace {

struct AtomicMem {
  static int32_t load(const std::atomic<int32_t>* p) { return p->load(std::memory_order_relaxed); }
  static int32_t cas(std::atomic<int32_t>* p, int32_t expected, int32_t wanted) {
    p->compare_exchange_strong(expected, wanted, std::memory_order_relaxed);
    return expected;  // (the value found: `expected` itself on success)
  }
  static int32_t min(std::atomic<int32_t>* p, int32_t v) {
    int32_t old = p->load(std::memory_order_relaxed);
    while (v < old && !p->compare_exchange_weak(old, v, std::memory_order_relaxed)) {
    }
    return old;
  }
};

using Edges = std::vector<std::pair<int32_t, int32_t>>;

std::vector<int32_t> sequential_roots(int32_t n, const Edges& edges) {
  std::vector<int32_t> parent(n);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  for (const auto& e : edges) {
    const int32_t a = find(e.first), b = find(e.second);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  std::vector<int32_t> roots(n);
  for (int32_t i = 0; i < n; ++i) roots[i] = find(i);
  return roots;
}

template <bool COMPRESS>
bool run(const char* what, int32_t n, const Edges& edges) {
  std::vector<std::atomic<int32_t>> parent(n);
  for (int32_t i = 0; i < n; ++i) parent[i].store(i, std::memory_order_relaxed);
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (;;) {
      const size_t lo = next.fetch_add(64);
      if (lo >= edges.size()) break;
      const size_t hi = std::min(edges.size(), lo + 64);
      for (size_t e = lo; e < hi; ++e) (void)ptk::uf_unite<AtomicMem, COMPRESS>(parent.data(), edges[e].first, edges[e].second);
    }
  };
  std::vector<std::thread> pool;
  for (int t = 0; t < 16; ++t) pool.emplace_back(work);
  for (auto& th : pool) th.join();

  const std::vector<int32_t> want = sequential_roots(n, edges);
  // (the sequential roots are component minima: links only ever point at the smaller root)
  std::vector<int32_t> smallest(n);
  std::iota(smallest.begin(), smallest.end(), 0);
  for (int32_t i = 0; i < n; ++i) smallest[want[i]] = std::min(smallest[want[i]], i);
  for (int32_t i = 0; i < n; ++i) {
    const int32_t p = parent[i].load(std::memory_order_relaxed);
    if (p < 0 || p > i) {
      std::fprintf(stderr, "%s: parent[%d] = %d breaks parent[x] <= x\n", what, i, p);
      return false;
    }
    const int32_t got = ptk::uf_find<AtomicMem, COMPRESS>(parent.data(), i);
    if (got != want[i] || got != smallest[want[i]]) {
      std::fprintf(stderr, "%s: root of %d is %d, the sequential union-find has %d (component minimum %d)\n", what, i, got,
                   want[i], smallest[want[i]]);
      return false;
    }
  }
  return true;
}

}  // namespace

int main() {
  std::mt19937 rng(20261019u);
  // a random graph: 10^5 nodes, 4 x 10^5 edges
  const int32_t n = 100000;
  Edges random_edges(400000);
  std::uniform_int_distribution<int32_t> node(0, n - 1);
  for (auto& e : random_edges) e = {node(rng), node(rng)};
  // the chain of 4096 nodes: one long component
  const int32_t chain_n = 4096;
  Edges chain;
  for (int32_t i = 0; i + 1 < chain_n; ++i) chain.push_back(i % 2 ? std::make_pair(i, i + 1) : std::make_pair(i + 1, i));
  std::shuffle(chain.begin(), chain.end(), rng);
  // a sparse graph with many components of a few nodes each
  Edges sparse(30000);
  for (auto& e : sparse) e = {node(rng), node(rng)};

  bool ok = true;
  ok = run<false>("random graph", n, random_edges) && ok;
  ok = run<true>("random graph, path halving", n, random_edges) && ok;
  ok = run<false>("sparse graph", n, sparse) && ok;
  ok = run<true>("sparse graph, path halving", n, sparse) && ok;
  for (int rep = 0; rep < 8; ++rep) {
    std::shuffle(chain.begin(), chain.end(), rng);
    ok = run<false>("chain", chain_n, chain) && ok;
    ok = run<true>("chain, path halving", chain_n, chain) && ok;
  }
  if (!ok) return 1;
  std::printf("threads ok\n");
  return 0;
}
