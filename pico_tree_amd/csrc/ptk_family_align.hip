// ptk_family_align.hip -- align_step (ptk_kernels_align.hpp, K22): the pose kernel, the inverse of the leaf permutation
// (the handle's side table) and the levels of the summation tree over the rows of the k = 1 search.
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_align.hpp"

static_assert(sizeof(ptk_align_sums) == sizeof(pico_tree::internal::align_sums) && sizeof(ptk_align_sums) == 384,
              "ptk_align_sums layout");
static_assert(offsetof(ptk_align_sums, jtj) == offsetof(pico_tree::internal::align_sums, jtj), "ptk_align_sums layout");

namespace {

static __global__ void warm_align_kernel() {}

}  // namespace

namespace ptkf {

namespace al = pico_tree::internal;

AlignLayout align_layout(uint64_t nq) {
  const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  AlignLayout w{};
  w.q = 0;
  w.rows = pad((size_t)nq * 3 * sizeof(float));
  w.partials = w.rows + pad((size_t)nq * sizeof(ptk::Neighbor));
  uint64_t entries = 0;
  for (uint64_t n = nq; n > 0;) {  // (every level's partials, down to the level of one entry)
    n = al::align_blocks(n);
    entries += n;
    if (n == 1) break;
  }
  w.bytes = nq == 0 ? 0 : w.partials + (size_t)entries * kAlignEntryBytes;
  return w;
}

int align_inverse(const ptk_tree* t, void** d_inv, hipStream_t s) {
  *d_inv = nullptr;
  void* table = nullptr;
  PTK_HIP(hipMalloc(&table, std::max<size_t>((size_t)t->n_points, 1) * sizeof(uint32_t)));
  const uint32_t blocks = (uint32_t)((t->n_points + 255) / 256);
  if (blocks > 0)
    hipLaunchKernelGGL(ptk::align_inverse_kernel, dim3(blocks), dim3(256), 0, s, t->dev.pts, (uint32_t)t->n_points,
                       static_cast<uint32_t*>(table));
  hipError_t he = hipGetLastError();
  const hipError_t hs = hipStreamSynchronize(s);  // (the table is shared by every stream from now on)
  if (he == hipSuccess) he = hs;
  if (he != hipSuccess) {
    (void)hipFree(table);
    return fail(PTK_ERR_DEVICE, "HIP error while building the inverse permutation: %s", hipGetErrorString(he));
  }
  *d_inv = table;
  return PTK_OK;
}

int align_pose(const ptk_tree* t, const float* d_q, uint64_t nq, const float* m, float* d_out, hipStream_t s) {
  ptk::AlignPose pose;
  std::memcpy(pose.m, m, sizeof pose.m);
  Timer timer(t, s);
  hipLaunchKernelGGL(ptk::align_pose_kernel, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, s, d_q, nq, pose, d_out);
  PTK_HIP(hipGetLastError());
  timer.stop(2, nq);
  return PTK_OK;
}

int align_reduce(const ptk_tree* t, const ptk::Neighbor* d_rows, const float* d_qp, uint64_t nq, const float* d_normals,
                 float max_distance, char* d_partials, ptk_align_sums* d_out, hipStream_t s) {
  const bool plane = d_normals != nullptr;
  auto* out = reinterpret_cast<unsigned long long*>(d_out);
  Timer timer(t, s);
  if (nq == 0) {
    hipLaunchKernelGGL(ptk::align_finish_kernel, dim3(1), dim3(64), 0, s, nullptr, nullptr, plane ? 1 : 0, nq, out);
    PTK_HIP(hipGetLastError());
    timer.stop(2, nq);
    return PTK_OK;
  }
  const int terms = al::align_terms(plane);
  // A level of n entries: its terms (term j at j * n), then its counts at the offset of a level of the widest mode.
  const auto sums_of = [](char* level) { return reinterpret_cast<double*>(level); };
  const auto counts_of = [](char* level, uint64_t n) {
    return reinterpret_cast<uint64_t*>(level + (size_t)n * al::align_max_terms * sizeof(double));
  };
  uint64_t n = al::align_blocks(nq);
  char* level = d_partials;
  const auto* inv = static_cast<const uint32_t*>(t->d_align_inverse);
  if (plane)
    hipLaunchKernelGGL(ptk::align_terms_kernel<true>, dim3((uint32_t)n), dim3(64), 0, s, d_rows, d_qp, nq, inv, t->dev.pts,
                       (uint32_t)t->n_points, d_normals, max_distance, n, sums_of(level), counts_of(level, n));
  else
    hipLaunchKernelGGL(ptk::align_terms_kernel<false>, dim3((uint32_t)n), dim3(64), 0, s, d_rows, d_qp, nq, inv, t->dev.pts,
                       (uint32_t)t->n_points, d_normals, max_distance, n, sums_of(level), counts_of(level, n));
  while (n > 1) {
    const uint64_t m = al::align_blocks(n);
    char* next = level + (size_t)n * kAlignEntryBytes;
    hipLaunchKernelGGL(ptk::align_reduce_kernel, dim3((uint32_t)m), dim3(64), 0, s, sums_of(level), counts_of(level, n), n,
                       terms, m, sums_of(next), counts_of(next, m));
    level = next;
    n = m;
  }
  hipLaunchKernelGGL(ptk::align_finish_kernel, dim3(1), dim3(64), 0, s, sums_of(level), counts_of(level, 1), plane ? 1 : 0, nq,
                     out);
  PTK_HIP(hipGetLastError());
  timer.stop(2, nq);
  return PTK_OK;
}

void warm_align() {
  hipLaunchKernelGGL(warm_align_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
