// ptk_family_spacing.hip -- spacing_knn_self (ptk_kernels_spacing.hpp, K24): the direct kernel with the reducing exit
// over the tree's own leaf-order records, the row reduction of the staged route (float32 and float64), and the
// statistics: two passes of align_step's summation tree over the means, their one-lane finishes and the keep kernel.
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_spacing.hpp"

static_assert(sizeof(ptk_spacing_stats) == sizeof(pico_tree::internal::spacing_stats) && sizeof(ptk_spacing_stats) == 64,
              "ptk_spacing_stats layout");
static_assert(offsetof(ptk_spacing_stats, variance) == offsetof(pico_tree::internal::spacing_stats, variance),
              "ptk_spacing_stats layout");
static_assert(PTK_SPACING_SQRT == pico_tree::internal::spacing_sqrt, "PTK_SPACING_SQRT");

namespace {

namespace al = pico_tree::internal;

// The launch geometry of launch_knn_self (ptk_family_self.hip).
template <int OVF, class M>
int launch_spacing_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, float* d_mean,
                        float* d_kth, hipStream_t s) {
  constexpr int BLOCK = 64, S = kGenRing;
  const uint32_t blocks = (uint32_t)((n + BLOCK - 1) / BLOCK);
  const size_t smem = (size_t)S * BLOCK * 8;
  Timer timer(t, s);
  ptkd::with_slots<4, 8, 16, 32, 64>(k + 1, [&](auto K) {
    hipLaunchKernelGGL((ptk::spacing_self_kernel<K, S, OVF, BLOCK, kGenLeafB, M>), dim3(blocks), dim3(BLOCK), smem, s, t->dev,
                       t->dim, first, n, k, flags, d_mean, d_kth);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, n);
  return PTK_OK;
}

// The two sums, their finishes and the mask.  A level of m entries in the workspace: m partials, then m counts.
template <class Real>
int statistics(const Real* d_mean, uint64_t n, float ratio, uint8_t* d_keep, ptk_spacing_stats* d_stats, char* d_workspace,
               hipStream_t s) {
  auto* stats = reinterpret_cast<al::spacing_stats*>(d_stats != nullptr ? reinterpret_cast<char*>(d_stats) : d_workspace);
  char* const levels = d_workspace + ptkf::kSpacingRecordBytes;
  const auto sums_of = [](char* level) { return reinterpret_cast<double*>(level); };
  const auto counts_of = [](char* level, uint64_t m) { return reinterpret_cast<uint64_t*>(level + (size_t)m * sizeof(double)); };
  for (int second = 0; second < 2; ++second) {
    uint64_t m = al::align_blocks(n);
    char* level = levels;
    if (second == 0)
      hipLaunchKernelGGL((ptk::spacing_level0_kernel<Real, false>), dim3((uint32_t)m), dim3(64), 0, s, d_mean, n, stats, m,
                         sums_of(level), counts_of(level, m));
    else
      hipLaunchKernelGGL((ptk::spacing_level0_kernel<Real, true>), dim3((uint32_t)m), dim3(64), 0, s, d_mean, n, stats, m,
                         sums_of(level), counts_of(level, m));
    while (m > 1) {
      const uint64_t up = al::align_blocks(m);
      char* next = level + (size_t)m * ptkf::kSpacingEntryBytes;
      hipLaunchKernelGGL(ptk::align_reduce_kernel, dim3((uint32_t)up), dim3(64), 0, s, sums_of(level), counts_of(level, m), m,
                         1, up, sums_of(next), counts_of(next, up));
      level = next;
      m = up;
    }
    hipLaunchKernelGGL(ptk::spacing_finish_kernel, dim3(1), dim3(64), 0, s, sums_of(level), counts_of(level, 1), second, n,
                       ratio, stats);
  }
  if (d_keep != nullptr)
    hipLaunchKernelGGL((ptk::spacing_keep_kernel<Real>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_mean, n, stats,
                       d_keep);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

static __global__ void warm_spacing_kernel() {}

}  // namespace

namespace ptkf {

int spacing_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, float* d_mean, float* d_kth,
                 hipStream_t s) {
  if (k + 1 > 64u || t->dim > 3) return fail(PTK_ERR_INVALID, "spacing_self: not a call of the direct kernel");
  return with_metric_ovf(t, kGenRing, [&](auto m, auto ovf) {
    return launch_spacing_self<ovf, ptkd::type_of<decltype(m)>>(t, first, n, k, flags, d_mean, d_kth, s);
  });
}

int spacing_rows(const ptk::Neighbor* rows, const float4* recs, const int32_t* index, uint64_t first, uint64_t n, uint32_t k,
                 uint32_t flags, float* d_mean, float* d_kth, hipStream_t s) {
  hipLaunchKernelGGL((ptk::spacing_rows_kernel<ptk::Neighbor, float>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                     rows, recs, index, first, n, k, flags, d_mean, d_kth);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int spacing_rows64(const void* rows, const int32_t* index, uint64_t first, uint64_t n, uint32_t k, uint32_t flags,
                   double* d_mean, double* d_kth, hipStream_t s) {
  hipLaunchKernelGGL((ptk::spacing_rows_kernel<ptk::Neighbor64, double>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                     static_cast<const ptk::Neighbor64*>(rows), static_cast<const float4*>(nullptr), index, first, n, k,
                     flags, d_mean, d_kth);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

size_t spacing_workspace_bytes(uint64_t n) {
  uint64_t entries = 0;
  for (uint64_t m = n; m > 0;) {  // (every level's partials, down to the level of one entry)
    m = al::align_blocks(m);
    entries += m;
    if (m == 1) break;
  }
  return n == 0 ? 0 : kSpacingRecordBytes + (size_t)entries * kSpacingEntryBytes;
}

int spacing_statistics(const float* d_mean, uint64_t n, float ratio, uint8_t* d_keep, ptk_spacing_stats* d_stats,
                       char* d_workspace, hipStream_t s) {
  return statistics<float>(d_mean, n, ratio, d_keep, d_stats, d_workspace, s);
}

int spacing_statistics64(const double* d_mean, uint64_t n, float ratio, uint8_t* d_keep, ptk_spacing_stats* d_stats,
                         char* d_workspace, hipStream_t s) {
  return statistics<double>(d_mean, n, ratio, d_keep, d_stats, d_workspace, s);
}

// (loads this unit's code object on the calling thread's device: ProcessWarmup of ptk_backend.hip)
void warm_spacing() {
  hipLaunchKernelGGL(warm_spacing_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
