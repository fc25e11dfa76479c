// tests/cpp/emulate_batch_order_narrow.cpp -- TEST INFRASTRUCTURE: the block passes of the batch order on narrow streams
// (radix_key_hist_kernel, radix_digit_hist_kernel, radix_narrow_scatter_kernel of pico_tree_amd/csrc/ptk_sort.hpp) run
// lane by lane on the CPU, on the block scheduler of tests/cpp/emulate_kernels.cpp.  The loop over the passes is the
// one of make_permutation() (ptk_backend.hip): the same choice of item layouts, the same alignment rule for the staged
// row loads, one digit stream that every scatter overwrites.
// Built by tests/test_batch_order_narrow.py with the emulator's g++ line and HIP stand-in.

#include "emulate_kernels.cpp"

extern "C" {

// narrow: the test hook sort_narrow (1 = digit stream, + 2 = packed items into the last pass, + 4 = rows through LDS).
// Returns 1 if the key kernel took its rows through LDS, 0 if it used load_query, -1 for a pair of layouts the host
// has no scatter for.  Every array a kernel writes starts out as 0xEE bytes.
int emu_radix_sort_narrow(const float* q, uint32_t dim, uint64_t nq, const float* lo, const float* inv, const uint32_t* bits,
                          uint32_t key_bits, uint32_t narrow, uint32_t* keys, uint32_t* perm) {
  const float3 l = make_float3(lo[0], lo[1], lo[2]);
  const float3 i = make_float3(inv[0], inv[1], inv[2]);
  const uint3 b3 = make_uint3(bits[0], bits[1], bits[2]);
  const uint32_t tiles = (uint32_t)((nq + ptk::kSortTile - 1) / ptk::kSortTile), stride = (tiles + 3u) & ~3u;
  std::vector<uint32_t> hist((size_t)ptk::kRadixBins * stride, 0xEEEEEEEEu), totals(ptk::kRadixBins, 0xEEEEEEEEu);
  std::vector<uint32_t> k0(nq, 0xEEEEEEEEu), out_perm(nq, 0xEEEEEEEEu);
  std::vector<uint2> pa(nq, uint2{0xEEEEEEEEu, 0xEEEEEEEEu}), pb(nq, uint2{0xEEEEEEEEu, 0xEEEEEEEEu});
  std::vector<uint64_t> digit_words((nq + 7) / 8, 0xEEEEEEEEEEEEEEEEull);  // nq bytes rounded up to 8, 8-byte aligned
  uint8_t* digits = reinterpret_cast<uint8_t*>(digit_words.data());
  const bool staged = (narrow & 4u) != 0u && dim == 3 && (reinterpret_cast<uintptr_t>(q) & 15u) == 0u;
  const bool pack = (narrow & 2u) != 0u && nq <= (1ull << ptk::kPackedRowBits);
  const int passes = ((int)key_bits + 7) / 8;
  const void* from = k0.data();
  uint32_t from_kind = ptk::kItemKeys;
  int rc = staged ? 1 : 0;
  for (int p = 0; p < passes; ++p) {
    const uint32_t shift = 8u * (uint32_t)p;
    const bool last = p + 1 == passes;
    void* to = last ? (void*)out_perm.data() : from == pa.data() ? (void*)pb.data() : (void*)pa.data();
    const uint32_t to_kind =
        last ? ptk::kItemRows : pack && (int)key_bits - 8 * (p + 1) <= 8 ? ptk::kItemPacked : ptk::kItemPairs;
    for_each_block(tiles, ptk::kSortBlock, [&] {
      if (p > 0) ptk::radix_digit_hist_kernel<>(digits, (uint32_t)nq, stride, hist.data());
      else if (staged) ptk::radix_key_hist_kernel<true>(q, dim, (uint32_t)nq, l, i, b3, k0.data(), shift, stride, hist.data());
      else ptk::radix_key_hist_kernel<false>(q, dim, (uint32_t)nq, l, i, b3, k0.data(), shift, stride, hist.data());
    });
    for_each_wave(ptk::kRadixBins, [&] { ptk::radix_scan_kernel(hist.data(), tiles, stride, totals.data()); });
    uint8_t* next = last ? nullptr : digits;
#define EMU_NARROW(IN, OUT)                                                                                              \
  case (IN) * 4u + (OUT):                                                                                                \
    for_each_block(tiles, ptk::kSortBlock, [&] {                                                                         \
      ptk::radix_narrow_scatter_kernel<IN, OUT>(from, to, next, (uint32_t)nq, shift, stride, hist.data(), totals.data()); \
    });                                                                                                                  \
    break
    switch (from_kind * 4u + to_kind) {
      EMU_NARROW(ptk::kItemKeys, ptk::kItemPairs);
      EMU_NARROW(ptk::kItemKeys, ptk::kItemPacked);
      EMU_NARROW(ptk::kItemKeys, ptk::kItemRows);
      EMU_NARROW(ptk::kItemPairs, ptk::kItemPairs);
      EMU_NARROW(ptk::kItemPairs, ptk::kItemPacked);
      EMU_NARROW(ptk::kItemPairs, ptk::kItemRows);
      EMU_NARROW(ptk::kItemPacked, ptk::kItemRows);
      default: rc = -1;
    }
#undef EMU_NARROW
    if (rc < 0) return rc;
    from = to;
    from_kind = to_kind;
  }
  std::memcpy(keys, k0.data(), nq * 4);
  std::memcpy(perm, out_perm.data(), nq * 4);
  return rc;
}

// The keys of radix_key_hist_kernel (order_keys: the rows of a thread side by side) and of morton_kernel (order_key, one
// row at a time) with a table of cell classes: occ[1 << sum(cell_bits)], mode = ptk::kCellsEmptyFirst / kCellsDenseFirst.
void emu_keys_with_cells(const float* q, uint32_t dim, uint64_t nq, const float* lo, const float* inv, const uint32_t* bits,
                         uint32_t key_bits, const uint8_t* occ, const float* cell_inv, const uint32_t* cell_bits,
                         uint32_t mode, uint32_t* keys_tile, uint32_t* keys_row) {
  const float3 l = make_float3(lo[0], lo[1], lo[2]);
  const float3 i = make_float3(inv[0], inv[1], inv[2]);
  const uint3 b3 = make_uint3(bits[0], bits[1], bits[2]);
  ptk::CellTable cells{};
  cells.occ = occ;
  cells.inv = make_float3(cell_inv[0], cell_inv[1], cell_inv[2]);
  cells.bits = make_uint3(cell_bits[0], cell_bits[1], cell_bits[2]);
  cells.key_bits = key_bits;
  cells.mode = mode;
  const uint32_t tiles = (uint32_t)((nq + ptk::kSortTile - 1) / ptk::kSortTile), stride = (tiles + 3u) & ~3u;
  std::vector<uint32_t> hist((size_t)ptk::kRadixBins * stride), ids(nq);
  const bool staged = dim == 3 && (reinterpret_cast<uintptr_t>(q) & 15u) == 0u;
  for_each_block(tiles, ptk::kSortBlock, [&] {
    if (staged) ptk::radix_key_hist_kernel<true>(q, dim, (uint32_t)nq, l, i, b3, keys_tile, 0u, stride, hist.data(), cells);
    else ptk::radix_key_hist_kernel<false>(q, dim, (uint32_t)nq, l, i, b3, keys_tile, 0u, stride, hist.data(), cells);
  });
  for_each_lane(nq, [&] { ptk::morton_kernel(q, dim, nq, l, i, b3, keys_row, ids.data(), cells); });
}

}  // extern "C"
