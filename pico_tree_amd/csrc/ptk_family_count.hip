// ptk_family_count.hip -- count_within of 3-D float32 trees (ptk_kernels_count.hpp): the per-branch side table and
// the count kernel with its two shortcuts; the clamp of the other families' counts; aggregate_within
// (ptk_kernels_aggregate.hpp, K21): the sum / min / max of a caller's values over the rows of the per-row fill pass.
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_aggregate.hpp"
#include "ptk_kernels_count.hpp"
#include "ptk_kernels_count64.hpp"

static_assert(sizeof(ptk::CountBox) == ptkf::kCountBoxBytes, "count table entry");
static_assert(sizeof(ptk::CountBox64) == ptkf::kCountBox64Bytes, "count table entry (double)");

namespace {

template <int S, int OVF, int LEAFB, class M>
int launch_count_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius,
                        uint64_t max_count, bool shortcut, uint64_t* d_counts, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  Timer timer(t, s);
  hipLaunchKernelGGL((ptk::count_within_kernel<S, OVF, 64, LEAFB, M>), dim3(blocks), dim3(64), (size_t)S * 64 * 8, s, t->dev,
                     static_cast<const ptk::CountBox*>(t->d_count_table), d_q, t->dim, perm, nq, radius, max_count,
                     shortcut ? 1u : 0u, d_counts, nullptr);
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}

// count_within_radii: launch_count_within with the per-row kernel.
template <int S, int OVF, int LEAFB, class M>
int launch_count_within_radii(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, const float* d_radii,
                              uint64_t max_count, bool shortcut, uint64_t* d_counts, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  Timer timer(t, s);
  hipLaunchKernelGGL((ptk::count_within_radii_kernel<S, OVF, 64, LEAFB, M>), dim3(blocks), dim3(64), (size_t)S * 64 * 8, s,
                     t->dev, static_cast<const ptk::CountBox*>(t->d_count_table), d_q, t->dim, perm, nq, d_radii, max_count,
                     shortcut ? 1u : 0u, d_counts, nullptr);
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}

// search_radius_radii: the fill pass behind launch_count_within_radii(max_count = 0).
template <int S, int OVF, int LEAFB, class M>
int launch_radius_radii_fill(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, const float* d_radii,
                             const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  Timer timer(t, s);
  hipLaunchKernelGGL((ptk::radius_radii_fill_kernel<S, OVF, 64, LEAFB, M>), dim3(blocks), dim3(64), (size_t)S * 64 * 8, s,
                     t->dev, d_q, t->dim, perm, nq, d_radii, d_offsets, d_out);
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}

// aggregate_within: the launch geometry of launch_radius_radii_fill, one launch per channel window.
template <int S, int OVF, int LEAFB, class M>
int launch_aggregate_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius,
                            const float* d_radii, const float* d_values, uint32_t channels, uint32_t flags, float* d_out,
                            uint64_t* d_counts, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  Timer timer(t, s);
  ptkd::with_bool(d_radii != nullptr, [&](auto per_row) {
    constexpr bool PER_ROW = decltype(per_row)::value;
    return ptk::aggregate_windows(d_values, d_out, channels, [&](auto W, auto VEC, uint32_t c0, uint32_t w) {
      hipLaunchKernelGGL((ptk::aggregate_within_kernel<W, VEC, S, OVF, 64, LEAFB, PER_ROW, M>), dim3(blocks), dim3(64),
                         (size_t)S * 64 * 8, s, t->dev, d_q, t->dim, perm, nq, radius, d_radii, d_values, channels, c0, w,
                         flags, d_out, d_counts);
      return PTK_OK;
    });
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}

static __global__ void warm_count_kernel() {}

}  // namespace

namespace ptkf {

int count_table(const ptk_tree* t, void** d_table, hipStream_t s) {
  const uint32_t nb = (uint32_t)t->n_branches;
  *d_table = nullptr;
  if (nb == 0u) return PTK_OK;  // (a single leaf: the kernel never meets a branch)
  void* table = nullptr;
  uint32_t* tmp = nullptr;
  PTK_HIP(hipMalloc(&table, (size_t)nb * sizeof(ptk::CountBox)));
  hipError_t he = hipMalloc((void**)&tmp, (size_t)nb * 8);
  if (he == hipSuccess) {
    const uint32_t blocks = (nb + 255u) / 256u;
    hipLaunchKernelGGL(ptk::count_parents_kernel, dim3(blocks), dim3(256), 0, s, t->dev, nb, tmp, tmp + nb);
    hipLaunchKernelGGL(ptk::count_table_kernel, dim3(blocks), dim3(256), 0, s, t->dev, nb, tmp, tmp + nb,
                       static_cast<ptk::CountBox*>(table));
    he = hipGetLastError();
    const hipError_t hs = hipStreamSynchronize(s);  // (the table is shared by every stream from now on)
    if (he == hipSuccess) he = hs;
  }
  if (tmp) (void)hipFree(tmp);
  if (he != hipSuccess) {
    (void)hipFree(table);
    return fail(PTK_ERR_DEVICE, "HIP error while building the count table: %s", hipGetErrorString(he));
  }
  *d_table = table;
  return PTK_OK;
}

int count_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, uint64_t max_count,
                 bool shortcut, uint64_t* d_counts, hipStream_t s) {
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_count_within<16, ovf, kGenLeafB, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, radius, max_count,
        shortcut, d_counts, s);
  });
}

int count_within_radii(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, const float* d_radii,
                        uint64_t max_count, bool shortcut, uint64_t* d_counts, hipStream_t s) {
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_count_within_radii<16, ovf, kGenLeafB, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, d_radii, max_count,
        shortcut, d_counts, s);
  });
}

int radius_radii_fill(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, const float* d_radii,
                      const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_radius_radii_fill<16, ovf, kGenLeafB, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, d_radii, d_offsets,
        d_out, s);
  });
}

int aggregate_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius,
                     const float* d_radii, const float* d_values, uint32_t channels, uint32_t flags, float* d_out,
                     uint64_t* d_counts, hipStream_t s) {
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_aggregate_within<16, ovf, kGenLeafB, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, radius, d_radii,
        d_values, channels, flags, d_out, d_counts, s);
  });
}

int clamp_counts(uint64_t* d_counts, uint64_t n, uint64_t max_count, hipStream_t s) {
  if (max_count == 0u || n == 0u) return PTK_OK;
  hipLaunchKernelGGL(ptk::clamp_counts_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_counts, n, max_count);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int count_table64(const ptk::DevTree64& dev, uint64_t n_branches, void** d_table, hipStream_t s) {
  const uint32_t nb = (uint32_t)n_branches;
  *d_table = nullptr;
  if (nb == 0u) return PTK_OK;
  void* table = nullptr;
  uint32_t* tmp = nullptr;
  PTK_HIP(hipMalloc(&table, (size_t)nb * sizeof(ptk::CountBox64)));
  hipError_t he = hipMalloc((void**)&tmp, (size_t)nb * 8);
  if (he == hipSuccess) {
    const uint32_t blocks = (nb + 255u) / 256u;
    hipLaunchKernelGGL(ptk::count64_parents_kernel, dim3(blocks), dim3(256), 0, s, dev, nb, tmp, tmp + nb);
    hipLaunchKernelGGL(ptk::count64_table_kernel, dim3(blocks), dim3(256), 0, s, dev, nb, tmp, tmp + nb,
                       static_cast<ptk::CountBox64*>(table));
    he = hipGetLastError();
    const hipError_t hs = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hs;
  }
  if (tmp) (void)hipFree(tmp);
  if (he != hipSuccess) {
    (void)hipFree(table);
    return fail(PTK_ERR_DEVICE, "HIP error while building the count table: %s", hipGetErrorString(he));
  }
  *d_table = table;
  return PTK_OK;
}

int count64_within(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, const double* d_q,
                   const uint32_t* perm, uint64_t q0, uint64_t n, double radius, uint64_t max_count, bool shortcut,
                   uint64_t* d_counts, ptk::Rec64* stack, uint32_t slots, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = ptk::lds64_bytes(0, dev.dim);
  const uint32_t sc = shortcut ? 1u : 0u;
  ptkd::with_euclid64(metric, [&](auto m) {
    hipLaunchKernelGGL(ptk::count64_within_kernel<ptkd::type_of<decltype(m)>>, grid, block, smem, s, dev, table, d_q, perm,
                       q0, n, radius, max_count, sc, d_counts, stack, slots, nullptr);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int count64_within_radii(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, const double* d_q,
                         const uint32_t* perm, uint64_t q0, uint64_t n, const double* d_radii, uint64_t max_count,
                         bool shortcut, uint64_t* d_counts, ptk::Rec64* stack, uint32_t slots, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = ptk::lds64_bytes(0, dev.dim);
  const uint32_t sc = shortcut ? 1u : 0u;
  ptkd::with_euclid64(metric, [&](auto m) {
    hipLaunchKernelGGL(ptk::count64_within_radii_kernel<ptkd::type_of<decltype(m)>>, grid, block, smem, s, dev, table, d_q,
                       perm, q0, n, d_radii, max_count, sc, d_counts, stack, slots, nullptr);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// (loads this unit's code object on the calling thread's device: ProcessWarmup of ptk_backend.hip)
void warm_count() {
  hipLaunchKernelGGL(warm_count_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
