// aggregate.hpp -- aggregate_within_self / aggregate_within (ptk.h): the fold of a caller's per-point values
// over one row of a radius search, with the formulas of the contract verbatim.  Used by the library's host loops
// (ptk_host_aggregate_within_self / ptk_host_aggregate_within) and by kd_tree::aggregate_within_self /
// kd_tree::aggregate_within where the backend does not serve; the device kernels (ptk_kernels_aggregate.hpp) apply the
// same three lines to accumulators in registers.
//
// Every operation is one IEEE float32 operation in row order.  The compare-selects are written out: std::fmax / fmin
// would let a value replace a NaN accumulator.
#pragma once

#include <cstddef>
#include <cstdint>
#include <limits>

namespace pico_tree {

//! The op of kd_tree::aggregate_within_self / aggregate_within (PTK_AGG_SUM / _MIN / _MAX of ptk.h).
enum class aggregate_op : std::uint32_t { sum = 0, min = 1, max = 2 };

namespace internal {

constexpr std::uint32_t aggregate_include_self = 0x100u;  // PTK_AGG_INCLUDE_SELF
constexpr std::uint32_t aggregate_max_channels = 1024u;

//! out[0 .. channels) of one row: \p row holds entries with .index in row order (the own entry removed); \p own is the
//! point's own row of values with INCLUDE_SELF, null without (the accumulators then start at the op's identity).
template <typename Row_>
inline void aggregate_row(
    float const* values, std::size_t channels, aggregate_op op, float const* own, Row_ const& row, float* out) {
  for (std::size_t a = 0; a < channels; ++a) {
    float acc;
    if (own != nullptr) acc = own[a];
    else if (op == aggregate_op::sum) acc = 0.0f;
    else if (op == aggregate_op::max) acc = -std::numeric_limits<float>::infinity();
    else acc = std::numeric_limits<float>::infinity();
    for (auto const& nb : row) {
      float const v = values[static_cast<std::size_t>(nb.index) * channels + a];
      if (op == aggregate_op::sum) acc = acc + v;
      else if (op == aggregate_op::max) acc = (v > acc) ? v : acc;
      else acc = (v < acc) ? v : acc;
    }
    out[a] = acc;
  }
}

}  // namespace internal

}  // namespace pico_tree
