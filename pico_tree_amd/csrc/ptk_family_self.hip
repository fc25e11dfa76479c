// ptk_family_self.hip -- search_knn_self: the direct kernel over the tree's own leaf-order
// records (3-D float32 trees, the four non-topological metrics, k + 1 <= 64) and the two small kernels of the staged route
// (the piece's points as query rows; the rule of the contract on the rows the handle's own search returned), float32 and
// float64.
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_f64.hpp"

namespace {

template <int OVF, class M>
int launch_knn_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, ptk::Neighbor* d_out, hipStream_t s) {
  constexpr int BLOCK = 64, S = kGenRing;
  const uint32_t blocks = (uint32_t)((n + BLOCK - 1) / BLOCK);
  const size_t smem = (size_t)S * BLOCK * 8;
  Timer timer(t, s);
#define PTK_LAUNCH_SELF(KK)                                                                                         \
  hipLaunchKernelGGL((ptk::knn_self_kernel<KK, S, OVF, BLOCK, kGenLeafB, M>), dim3(blocks), dim3(BLOCK), smem, s, t->dev, \
                     t->dim, first, n, k, d_out)
  if (k + 1 <= 4) PTK_LAUNCH_SELF(4);
  else if (k + 1 <= 8) PTK_LAUNCH_SELF(8);
  else if (k + 1 <= 16) PTK_LAUNCH_SELF(16);
  else if (k + 1 <= 32) PTK_LAUNCH_SELF(32);
  else PTK_LAUNCH_SELF(64);
#undef PTK_LAUNCH_SELF
  PTK_HIP(hipGetLastError());
  timer.stop(0, n);
  return PTK_OK;
}

static __global__ void warm_self_kernel() {}

}  // namespace

namespace ptkf {

int knn_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, ptk::Neighbor* d_out, hipStream_t s) {
  if (k + 1 > 64u || t->dim > 3) return fail(PTK_ERR_INVALID, "knn_self: not a call of the direct kernel");
  int rc = PTK_OK;
  PTK_WITH_METRIC(PTK_WITH_OVF(kGenRing, (launch_knn_self<OVF, M>(t, first, n, k, d_out, s))));
  return rc;
}

int self_queries(const float4* recs, const float* pts, uint32_t stride, uint32_t dim, uint64_t first, uint64_t n, float* d_q,
                 hipStream_t s) {
  hipLaunchKernelGGL((ptk::self_queries_kernel<float>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, recs, pts, stride,
                     dim, first, n, d_q);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int self_queries64(const double* pts, uint32_t stride, uint32_t dim, uint64_t first, uint64_t n, double* d_q, hipStream_t s) {
  hipLaunchKernelGGL((ptk::self_queries_kernel<double>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                     static_cast<const float4*>(nullptr), pts, stride, dim, first, n, d_q);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int drop_self(const ptk::Neighbor* rows, const float4* recs, const int32_t* index, uint64_t first, uint64_t n, uint32_t k,
              ptk::Neighbor* d_out, hipStream_t s) {
  hipLaunchKernelGGL((ptk::drop_self_kernel<ptk::Neighbor, float>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, rows,
                     recs, index, first, n, k, 3.402823466e+38f, d_out);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int drop_self64(const void* rows, const int32_t* index, uint64_t first, uint64_t n, uint32_t k, void* d_out, hipStream_t s) {
  hipLaunchKernelGGL((ptk::drop_self_kernel<ptk::Neighbor64, double>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                     static_cast<const ptk::Neighbor64*>(rows), static_cast<const float4*>(nullptr), index, first, n, k,
                     ptk::kDblMax, static_cast<ptk::Neighbor64*>(d_out));
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// (loads this unit's code object on the calling thread's device: ProcessWarmup of ptk_backend.hip)
void warm_self() {
  hipLaunchKernelGGL(warm_self_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
