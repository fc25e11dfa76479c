// ptk_family_topo.hip -- the searches under the topological metrics (metric_so2, metric_se2_squared; ptk_kernels_topo.hpp).
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_topo.hpp"

namespace {

template <int OVF>
int launch_knn_topo(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
                    ptk::Neighbor* d_out, hipStream_t s, bool short_tree) {
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  const size_t smem = (size_t)16 * 64 * 8;
  Timer timer(t, s);
  ptkd::with_topo(t->metric.load(), [&](auto m) -> int {
    using T = ptkd::type_of<decltype(m)>;
    if (k <= 64 && !short_tree)
      return ptkd::with_slots<4, 8, 16, 32, 64>(k, [&](auto K) {
        hipLaunchKernelGGL((ptk::knn_topo_reg_kernel<K, 16, OVF, T>), dim3(blocks), dim3(64), smem, s, t->dev, d_q, t->dim,
                           perm, nq, k, inv_ratio(e), d_out);
        return PTK_OK;
      });
    hipLaunchKernelGGL((ptk::knn_topo_kernel<16, OVF, T>), dim3(blocks), dim3(64), smem, s, t->dev, d_q, t->dim, perm, nq,
                       k, inv_ratio(e), d_out);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}

template <int OVF>
int launch_radius_topo(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e,
                       bool fill, uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  const size_t smem = (size_t)16 * 64 * 8;
  Timer timer(t, s);
  ptkd::with_topo(t->metric.load(), [&](auto m) {
    return ptkd::with_bool(fill, [&](auto FILL) {
      hipLaunchKernelGGL((ptk::radius_topo_kernel<16, OVF, FILL, ptkd::type_of<decltype(m)>>), dim3(blocks), dim3(64), smem,
                         s, t->dev, d_q, t->dim, perm, nq, radius, inv_ratio(e), d_counts, d_offsets, d_out);
      return PTK_OK;
    });
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, fill ? 0 : nq);
  return PTK_OK;
}


static __global__ void warm_topo_kernel() {}

}  // namespace

namespace ptkf {

int knn_topo(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
             ptk::Neighbor* d_out, hipStream_t s, bool no_register_list) {
  return with_ovf(t, 16, [&](auto ovf) { return launch_knn_topo<ovf>(t, d_q, perm, nq, k, e, d_out, s, no_register_list); });
}

int radius_topo(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e, bool fill,
                uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  return with_ovf(t, 16, [&](auto ovf) {
    return launch_radius_topo<ovf>(t, d_q, perm, nq, radius, e, fill, d_counts, d_offsets, d_out, s);
  });
}

// (loads this unit's code object on the calling thread's device: ProcessWarmup of ptk_backend.hip)
void warm_topo() {
  hipLaunchKernelGGL(warm_topo_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
