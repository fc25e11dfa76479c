// suppress.hpp -- suppress_within_self (ptk.h): the key of a point and the greedy pass over the rows of
// search_radius_self, as the contract reads.  ONE statement of the key: compiled for the device by the kernels of
// pico_tree_amd/csrc/ptk_kernels_suppress.hpp (K23), for the library's host loop (ptk_host_suppress_within_self) and
// for kd_tree::suppress_within_self where the backend does not serve.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#if defined(__HIPCC__)
#define PICO_TREE_HD __host__ __device__
#else
#define PICO_TREE_HD
#endif

namespace pico_tree::internal {

//! The 32-bit finaliser of MurmurHash3: a bijection of the 32-bit integers.
PICO_TREE_HD inline std::uint32_t suppress_fmix32(std::uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

//! The total-order map of a float32's bits: a higher score gives a higher value, -0.0 lies below +0.0, the infinities
//! are ordinary values, a NaN takes the place its bits give it.
PICO_TREE_HD inline std::uint32_t suppress_ord(std::uint32_t bits) {
  return (bits & 0x80000000u) != 0 ? bits ^ 0xFFFFFFFFu : bits ^ 0x80000000u;
}

//! key(i) = (ord_i << 32) | (0xFFFFFFFF - i): distinct for distinct i; an equal ord is decided by the lower index.
PICO_TREE_HD inline std::uint64_t suppress_key_of(std::uint32_t ord, std::uint32_t i) {
  return (static_cast<std::uint64_t>(ord) << 32) | static_cast<std::uint64_t>(0xFFFFFFFFu - i);
}

//! The key in the default order: ord_i = fmix32(i).
PICO_TREE_HD inline std::uint64_t suppress_key(std::uint32_t i) { return suppress_key_of(suppress_fmix32(i), i); }

//! The key under the caller's scores, given the bits of scores[i].
PICO_TREE_HD inline std::uint64_t suppress_key(std::uint32_t i, std::uint32_t score_bits) {
  return suppress_key_of(suppress_ord(score_bits), i);
}

//! The key of point i: \p scores null gives the default order.
inline std::uint64_t suppress_key(float const* scores, std::size_t i) {
  if (scores == nullptr) return suppress_key(static_cast<std::uint32_t>(i));
  std::uint32_t bits;
  std::memcpy(&bits, scores + i, sizeof bits);
  return suppress_key(static_cast<std::uint32_t>(i), bits);
}

//! The index of the first NaN among \p n scores, \p n without one.
inline std::size_t suppress_first_nan(float const* scores, std::size_t n) {
  for (std::size_t i = 0; i < n; ++i) {
    if (scores[i] != scores[i]) return i;
  }
  return n;
}

// rows[i]: row i of search_radius_self (entries with an `index` member).  keep: rows.size() entries.
//   keep[i] = 1 iff row i holds no j with key(j) > key(i) and keep[j] == 1, else 0
// decided in descending key: every cell a point looks at is final when its turn comes.  Returns the number kept.
template <typename Rows_>
inline std::uint64_t suppress_rows(Rows_ const& rows, float const* scores, std::uint8_t* keep) {
  std::size_t const n = rows.size();
  std::vector<std::uint64_t> key(n);
  for (std::size_t i = 0; i < n; ++i) key[i] = suppress_key(scores, i);
  std::vector<std::uint32_t> order(n);
  std::iota(order.begin(), order.end(), std::uint32_t(0));
  std::sort(order.begin(), order.end(), [&](std::uint32_t a, std::uint32_t b) { return key[a] > key[b]; });
  std::uint64_t kept = 0;
  for (std::uint32_t const i : order) {
    std::uint8_t cell = 1;
    for (auto const& nb : rows[i]) {
      std::size_t const j = static_cast<std::size_t>(nb.index);
      if (key[j] > key[i] && keep[j] == 1) {
        cell = 0;
        break;
      }
    }
    keep[i] = cell;
    kept += cell;
  }
  return kept;
}

}  // namespace pico_tree::internal
