// io_parts_main.cpp -- the layout of the parts of a host-buffer call inside a device block
// (pico_tree_amd/csrc/ptk_io_parts.hpp).  Host only: the header needs no HIP and nothing else of the library.  Checked for
// the part lists of each of the seventeen fixed-row host entry points (ptk_search64_knn_self, the eighteenth user of
// the body, has the list of ptk_search_knn_self), for every combination of 0 / 1 / 15 / 16 / 17 bytes, and in each case
// with every subset of the optional parts absent.  Exits non-zero on the first difference and says which.
#include "ptk_io_parts.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Spec {
  size_t bytes;
  bool optional;
};
struct Call {
  const char* name;
  std::vector<Spec> parts;
};

char host_memory[1];  // what a present part points at: the layout never reads it
char block[1];        // the base the device pointers are taken from: never dereferenced

[[noreturn]] void fail(const Call& c, unsigned absent, const char* what, int part, size_t got, size_t want) {
  std::fprintf(stderr, "FAILED: %s, parts of", c.name);
  for (const Spec& s : c.parts) std::fprintf(stderr, " %zu", s.bytes);
  std::fprintf(stderr, " bytes, absent mask 0x%x, part %d: %s (got %zu, expected %zu)\n", absent, part, what, got, want);
  std::exit(1);
}

// The list of `c` with the parts of `absent` (a bit per part) absent and those of `empty` present with no bytes.
ptkio::Parts layout(const Call& c, unsigned absent, unsigned empty) {
  ptkio::Part p[ptkio::kMaxParts] = {};
  const int n = (int)c.parts.size();
  for (int i = 0; i < n; ++i) {
    if (absent >> i & 1u)
      p[i] = ptkio::in_part(nullptr, 0);
    else
      p[i] = ptkio::out_part(host_memory, empty >> i & 1u ? 0 : c.parts[i].bytes, /*clear_first=*/i == 0);
  }
  switch (n) {
    case 0: return ptkio::Parts{};
    case 1: return ptkio::Parts{p[0]};
    case 2: return ptkio::Parts{p[0], p[1]};
    default: return ptkio::Parts{p[0], p[1], p[2]};
  }
}

void check(const Call& c) {
  const int n = (int)c.parts.size();
  for (unsigned absent = 0; absent < (1u << n); ++absent) {
    bool allowed = true;
    for (int i = 0; i < n; ++i) allowed = allowed && (c.parts[i].optional || !(absent >> i & 1u));
    if (!allowed) continue;
    const ptkio::Parts got = layout(c, absent, 0);
    const ptkio::Parts zero = layout(c, 0, absent);  // the same call with those parts there and empty
    if (got.size() != n) fail(c, absent, "number of parts", -1, (size_t)got.size(), (size_t)n);
    size_t end = 0;  // the end of the last present part so far
    bool any = false;
    for (int i = 0; i < n; ++i) {
      const bool here = !(absent >> i & 1u);
      if (got.present(i) != here) fail(c, absent, "present()", i, got.present(i), here);
      char* at = got.at<char>(block, i);
      if (!here) {
        if (at != nullptr) fail(c, absent, "an absent part has a device pointer", i, 1, 0);
        if (got.bytes(i) != 0) fail(c, absent, "an absent part has bytes", i, got.bytes(i), 0);
        continue;
      }
      any = true;
      if (got.bytes(i) != c.parts[i].bytes) fail(c, absent, "bytes()", i, got.bytes(i), c.parts[i].bytes);
      if (got.offset(i) % 16 != 0) fail(c, absent, "the offset is no multiple of 16", i, got.offset(i) % 16, 0);
      if (got.offset(i) < end) fail(c, absent, "the part overlaps the one before it", i, got.offset(i), end);
      if (at != block + got.offset(i)) fail(c, absent, "at() is not base + offset", i, (size_t)(at - block), got.offset(i));
      if (got.offset(i) != zero.offset(i))
        fail(c, absent, "an absent part moved this one (against the same part empty)", i, got.offset(i), zero.offset(i));
      if (got.clear_first(i) != (i == 0)) fail(c, absent, "clear_first()", i, got.clear_first(i), i == 0);
      if (got.source(i) != host_memory || got.destination(i) != host_memory) fail(c, absent, "the host pointer", i, 0, 1);
      end = got.offset(i) + got.bytes(i);
    }
    const size_t want_total = (end + 15) / 16 * 16;  // (the blocks grow in whole multiples of the alignment)
    if (got.total() != want_total) fail(c, absent, "total()", -1, got.total(), want_total);
    if (got.any() != any) fail(c, absent, "any()", -1, got.any(), any);
    // Tightly packed: a part begins where the one before it ends, rounded up -- no room is given away.
    size_t next = 0;
    for (int i = 0; i < n; ++i) {
      if (!got.present(i)) continue;
      if (got.offset(i) != next) fail(c, absent, "the part does not follow the one before it", i, got.offset(i), next);
      next = (got.offset(i) + got.bytes(i) + 15) / 16 * 16;
    }
  }
}

}  // namespace

int main() {
  // The shapes of tests/test_host_forms.py: 257 queries of a 3-D tree, k = 16; 130 points for the self forms; 9 channels.
  const size_t nq = 257, np = 130, dim = 3, k = 16, ch = 9, f = 4, d = 8, nb = 8, nb64 = 16, frame = 32, moments = 40;
  const std::vector<Call> calls = {
      // float32: inputs, then outputs
      {"knn_within in", {{nq * dim * f, false}}},
      {"knn_within out", {{nq * k * nb, false}}},
      {"knn_within_radii in", {{nq * dim * f, false}, {nq * f, false}}},
      {"knn_within_radii out", {{nq * k * nb, false}}},
      {"count_within in", {{nq * dim * f, false}}},
      {"count_within out", {{nq * 8, false}}},
      {"count_within_radii in", {{nq * dim * f, false}, {nq * f, false}}},
      {"count_within_radii out", {{nq * 8, false}}},
      {"knn_self in", {}},
      {"knn_self out", {{np * k * nb, false}}},
      {"count_within_self in", {{np * f, true}}},
      {"count_within_self out", {{np * 8, false}}},
      {"cluster_within_self in", {{np * f, true}}},
      {"cluster_within_self out", {{np * 4, false}}},
      {"normals_within_self in", {{np * f, true}}},
      {"normals_within_self out", {{np * frame, true}, {np * moments, true}}},
      {"aggregate_within_self in", {{np * ch * f, false}, {np * f, true}}},
      {"aggregate_within_self out", {{np * ch * f, false}, {np * 8, true}}},
      {"aggregate_within in", {{np * ch * f, false}, {nq * dim * f, false}, {nq * f, true}}},
      {"aggregate_within out", {{nq * ch * f, false}, {nq * 8, true}}},
      {"aggregate_within, 1 channel, out", {{nq * f, false}, {nq * 8, true}}},
      // float64
      {"search64_knn in", {{nq * dim * d, false}}},
      {"search64_knn out", {{nq * k * nb64, false}}},
      {"search64_knn_within in", {{nq * dim * d, false}}},
      {"search64_knn_within out", {{nq * k * nb64, false}}},
      {"search64_knn_within_radii in", {{nq * dim * d, false}, {nq * d, false}}},
      {"search64_knn_within_radii out", {{nq * k * nb64, false}}},
      {"search64_count_within in", {{nq * dim * d, false}}},
      {"search64_count_within out", {{nq * 8, false}}},
      {"search64_count_within_radii in", {{nq * dim * d, false}, {nq * d, false}}},
      {"search64_count_within_radii out", {{nq * 8, false}}},
      {"search64_count_within_self in", {{np * d, true}}},
      {"search64_count_within_self out", {{np * 8, false}}},
      {"search64_cluster_within_self in", {{np * d, true}}},
      {"search64_cluster_within_self out", {{np * 4, false}}},
  };
  for (const Call& c : calls) check(c);

  // Every combination of the sizes around the alignment, one to three parts, each of them optional.
  const size_t sizes[] = {0, 1, 15, 16, 17};
  for (size_t a : sizes) {
    check(Call{"one part of 0 / 1 / 15 / 16 / 17 bytes", {{a, true}}});
    for (size_t b : sizes) {
      check(Call{"two parts of 0 / 1 / 15 / 16 / 17 bytes", {{a, true}, {b, true}}});
      for (size_t c : sizes) check(Call{"three parts of 0 / 1 / 15 / 16 / 17 bytes", {{a, true}, {b, true}, {c, true}}});
    }
  }
  std::printf("io_parts OK\n");
  return 0;
}
