// ptk_family_mst.hip -- mst_within_self (ptk_kernels_mst.hpp, K25): the component table, the search over the tree's own
// leaf-order records under metric_l2_squared and metric_l1, with and without core distances, and the elementwise passes
// of a Boruvka round.  The rounds themselves are driven by ptkf::mst_rounds (ptk_families.hpp).
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_mst.hpp"

namespace {

// One piece of a round's search: the launch geometry of count_self_kernel.  Profile kinds: the first round counts as the
// search, the later ones as its tail.
template <int S, int OVF, class M>
int launch_mst_search(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_core,
                      const ptkf::MstLayout& at, char* ws, uint32_t skip, bool later_round, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = (size_t)S * 64 * 8;
  const auto* table = static_cast<const ptk::CountBox*>(t->d_count_table);
  Timer timer(t, s);
  ptkd::with_bool(d_core != nullptr, [&](auto CORE) {
    hipLaunchKernelGGL((ptk::mst_search_kernel<S, OVF, 64, kGenLeafB, CORE, M>), grid, block, smem, s, t->dev, table,
                       reinterpret_cast<const uint32_t*>(ws + at.comp), t->dim, first, n, radius, d_core,
                       reinterpret_cast<const int32_t*>(ws + at.label), skip, reinterpret_cast<uint2*>(ws + at.cand),
                       reinterpret_cast<unsigned long long*>(ws + at.best_wlo), nullptr);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(later_round ? 3 : 0, n);
  return PTK_OK;
}

static __global__ void warm_mst_kernel() {}

inline dim3 cells(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

namespace ptkf {

int mst_begin(const ptk_tree* t, char* ws, hipStream_t s) {
  const MstLayout at = mst_layout(t->n_points, mst_branches(t));
  const uint64_t n = t->n_points;
  hipLaunchKernelGGL(ptk::mst_init_kernel, cells(n), dim3(256), 0, s, n, reinterpret_cast<int32_t*>(ws + at.parent),
                     reinterpret_cast<int32_t*>(ws + at.label), reinterpret_cast<unsigned long long*>(ws + at.best_wlo),
                     reinterpret_cast<uint32_t*>(ws + at.best_hi), reinterpret_cast<uint32_t*>(ws));
  const uint32_t nb = (uint32_t)mst_branches(t);
  if (nb > 0u) {
    hipLaunchKernelGGL(ptk::count_parents_kernel, cells(nb), dim3(256), 0, s, t->dev, nb,
                       reinterpret_cast<uint32_t*>(ws + at.info), reinterpret_cast<uint32_t*>(ws + at.arrive));
    // (round 1: every point is a component of its own, so every subtree is mixed -- no climb is needed to know that)
    PTK_HIP(hipMemsetAsync(ws + at.comp, 0xFF, (size_t)nb * sizeof(uint32_t), s));
  }
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int mst_table(const ptk_tree* t, char* ws, hipStream_t s) {
  const uint32_t nb = (uint32_t)mst_branches(t);
  if (nb == 0u) return PTK_OK;  // (a single leaf: the search never meets a branch)
  const MstLayout at = mst_layout(t->n_points, mst_branches(t));
  PTK_HIP(hipMemsetAsync(ws + at.arrive, 0, (size_t)nb * sizeof(uint32_t), s));
  hipLaunchKernelGGL(ptk::mst_table_kernel, cells(nb), dim3(256), 0, s, t->dev, nb,
                     reinterpret_cast<const uint32_t*>(ws + at.info), reinterpret_cast<uint32_t*>(ws + at.arrive),
                     reinterpret_cast<const int32_t*>(ws + at.label), reinterpret_cast<uint32_t*>(ws + at.comp));
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int mst_search(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_core, char* ws, uint32_t skip,
               bool later_round, hipStream_t s) {
  if (t->dim > 3) return fail(PTK_ERR_INVALID, "mst_search: not a call of the self kernels");
  const MstLayout at = mst_layout(t->n_points, mst_branches(t));
  return with_ovf(t, 16, [&](auto ovf) {
    if (t->metric.load() == PTK_METRIC_L1)
      return launch_mst_search<16, ovf, ptk::MetricL1>(t, first, n, radius, d_core, at, ws, skip, later_round, s);
    return launch_mst_search<16, ovf, ptk::MetricL2>(t, first, n, radius, d_core, at, ws, skip, later_round, s);
  });
}

int mst_join(const ptk_tree* t, char* ws, ptk_mst_edge* d_edges, uint32_t* d_added, hipStream_t s) {
  const MstLayout at = mst_layout(t->n_points, mst_branches(t));
  const uint64_t n = t->n_points;
  const auto* cand = reinterpret_cast<const uint2*>(ws + at.cand);
  auto* label = reinterpret_cast<int32_t*>(ws + at.label);
  auto* parent = reinterpret_cast<int32_t*>(ws + at.parent);
  auto* best_wlo = reinterpret_cast<unsigned long long*>(ws + at.best_wlo);
  auto* best_hi = reinterpret_cast<uint32_t*>(ws + at.best_hi);
  hipLaunchKernelGGL(ptk::mst_tie_kernel, cells(n), dim3(256), 0, s, n, cand, label, best_wlo, best_hi);
  hipLaunchKernelGGL(ptk::mst_emit_kernel, cells(n), dim3(256), 0, s, n, cand, label, best_wlo, best_hi, parent,
                     reinterpret_cast<ptk::MstEdge*>(d_edges), (uint32_t)(n - 1), reinterpret_cast<uint32_t*>(ws), d_added);
  hipLaunchKernelGGL(ptk::mst_relabel_kernel, cells(n), dim3(256), 0, s, n, parent, label, best_wlo, best_hi);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

void warm_mst() {
  hipLaunchKernelGGL(warm_mst_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
