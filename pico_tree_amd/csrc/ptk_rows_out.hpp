// ptk_rows_out.hpp -- the host forms of the searches whose rows are ragged (radius, per-row radii, self-join, box; float32
// and float64), written once: counts -> offsets -> rows on the host.  Included by ptk_backend.hip and
// ptk_backend_f64.hpp only: the rocprim scan instantiated here belongs to that unit and to no other.

#pragma once

#include "ptk_backend_core.hpp"

namespace ptkb {

// counts (n + 1, the last one 0) -> offsets (n + 1) on the device, the offsets copied to the host.  (A template, so that
// the scan's kernels are instantiated where the first host form uses them, as they were before this header existed.)
template <class Count>
hipError_t scan_counts(Count* d_c, Count* d_o, uint64_t n, Count* offsets) {
  size_t tmp_bytes = 0;
  DeviceBlock tmp;
  hipError_t he = rocprim::exclusive_scan(nullptr, tmp_bytes, d_c, d_o, (Count)0, n + 1, rocprim::plus<Count>(),
                                          (hipStream_t) nullptr);
  if (he == hipSuccess) he = tmp.alloc(tmp_bytes ? tmp_bytes : 16);
  if (he == hipSuccess)
    he = rocprim::exclusive_scan(tmp.p, tmp_bytes, d_c, d_o, (Count)0, n + 1, rocprim::plus<Count>(), (hipStream_t) nullptr);
  if (he == hipSuccess) he = hipMemcpy(offsets, d_o, (n + 1) * sizeof(Count), hipMemcpyDeviceToHost);
  return he;
}

// The rows of a call in a device block of the call's own.
template <class Row>
auto rows_in(DeviceBlock& block) {
  return [&block](size_t bytes, Row** d_rows) {
    const hipError_t he = block.alloc(bytes);
    *d_rows = block.as<Row>();
    return he;
  };
}

// What every such host form does once its arguments are checked and its inputs are on the device (`he`: how that went).
//   count(d_counts) -> status                   the count pass: d_counts[0..n) (zeroed here, with the sentinel d_counts[n])
//   rows_block(bytes, &d_rows) -> hipError_t    the device block of the rows
//   fill(d_offsets, d_rows, total) -> status    the fill pass, with the row sort where the form has one
// offsets[0..n] are written; *out is a malloc block of max(total, 1) records (ptk_free) and NULL after every failure; a
// status of the library wins over a HIP error.
// Every record that comes down was written whole by a fill kernel -- those of ptk_neighbor64 store the padding word as 0
// -- so the device block is not cleared.
template <class Row, class RowsBlock, class Count, class Fill>
int rows_to_host(hipError_t he, uint64_t n, uint64_t* d_counts, uint64_t* d_offsets, uint64_t* offsets, Row** out,
                 RowsBlock&& rows_block, Count&& count, Fill&& fill) {
  *out = nullptr;
  int rc = PTK_OK;
  if (he == hipSuccess) he = hipMemset(d_counts, 0, (n + 1) * 8);
  if (he == hipSuccess) rc = count(d_counts);
  if (he == hipSuccess && rc == PTK_OK) he = scan_counts(d_counts, d_offsets, n, offsets);
  if (he == hipSuccess && rc == PTK_OK) {
    const uint64_t total = offsets[n];
    const size_t bytes = std::max<uint64_t>(total, 1) * sizeof(Row);
    Row* d_rows = nullptr;
    he = rows_block(bytes, &d_rows);
    if (he == hipSuccess) rc = fill(static_cast<const uint64_t*>(d_offsets), d_rows, total);
    if (he == hipSuccess && rc == PTK_OK) {
      *out = static_cast<Row*>(std::malloc(bytes));
      if (*out == nullptr) {
        rc = fail(PTK_ERR_NOMEM, "out of memory");
      } else if (total > 0) {
        he = hipMemcpy(*out, d_rows, total * sizeof(Row), hipMemcpyDeviceToHost);
      }
    }
  }
  if (rc == PTK_OK && he != hipSuccess) rc = fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(he));
  if (rc != PTK_OK) {
    std::free(*out);
    *out = nullptr;
  }
  return rc;
}

}  // namespace ptkb
