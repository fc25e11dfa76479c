// ptk_family_self.hip -- search_knn_self: the direct kernel over the tree's own leaf-order
// records (3-D float32 trees, the four non-topological metrics, k + 1 <= 64) and the two small kernels of the staged route
// (the piece's points as query rows; the rule of the contract on the rows the handle's own search returned), float32 and
// float64; search_radius_self / count_within_self (ptk_kernels_selfr.hpp, K18): the count and fill kernels over the tree's
// own records, float32 and float64, each written once over its radius source; cluster_within_self
// (ptk_kernels_cluster.hpp, K19): the mark, link and border kernels over the same records and the elementwise passes;
// normals_within_self (ptk_kernels_frames.hpp, K20): the moments and frames kernel over the same records;
// aggregate_within_self (ptk_kernels_aggregate.hpp, K21): the sum / min / max of a caller's values over the same rows.
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_aggregate.hpp"
#include "ptk_kernels_f64.hpp"
#include "ptk_kernels_cluster.hpp"
#include "ptk_kernels_frames.hpp"
#include "ptk_kernels_selfr.hpp"

namespace {

template <int OVF, class M>
int launch_knn_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, ptk::Neighbor* d_out, hipStream_t s) {
  constexpr int BLOCK = 64, S = kGenRing;
  const uint32_t blocks = (uint32_t)((n + BLOCK - 1) / BLOCK);
  const size_t smem = (size_t)S * BLOCK * 8;
  Timer timer(t, s);
  ptkd::with_slots<4, 8, 16, 32, 64>(k + 1, [&](auto K) {
    hipLaunchKernelGGL((ptk::knn_self_kernel<K, S, OVF, BLOCK, kGenLeafB, M>), dim3(blocks), dim3(BLOCK), smem, s, t->dev,
                       t->dim, first, n, k, d_out);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, n);
  return PTK_OK;
}

// count_within_self / search_radius_self: leaf positions [first, first + n); d_radii null: every point gets `radius`.
template <int S, int OVF, class M>
int launch_count_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, uint64_t max_count,
                      bool shortcut, uint64_t* d_counts, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  const auto* table = static_cast<const ptk::CountBox*>(t->d_count_table);
  Timer timer(t, s);
  ptkd::with_bool(d_radii != nullptr, [&](auto PER_ROW) {
    hipLaunchKernelGGL((ptk::count_self_kernel<S, OVF, 64, kGenLeafB, PER_ROW, M>), dim3(blocks), dim3(64),
                       (size_t)S * 64 * 8, s, t->dev, table, t->dim, first, n, radius, d_radii, max_count,
                       shortcut ? 1u : 0u, d_counts, nullptr);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, n);
  return PTK_OK;
}

template <int S, int OVF, class M>
int launch_radius_self_fill(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii,
                            const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  Timer timer(t, s);
  ptkd::with_bool(d_radii != nullptr, [&](auto PER_ROW) {
    hipLaunchKernelGGL((ptk::radius_self_fill_kernel<S, OVF, 64, kGenLeafB, PER_ROW, M>), dim3(blocks), dim3(64),
                       (size_t)S * 64 * 8, s, t->dev, t->dim, first, n, radius, d_radii, d_offsets, d_out);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, n);
  return PTK_OK;
}

template <class M>
int launch_count64_self(const ptk::DevTree64& dev, const ptk::CountBox64* table, uint64_t first, uint64_t n, double radius,
                        const double* d_radii, uint64_t max_count, bool shortcut, uint64_t* d_counts, ptk::Rec64* stack,
                        uint32_t slots, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = ptk::lds64_bytes(0, dev.dim);
  ptkd::with_bool(d_radii != nullptr, [&](auto PER_ROW) {
    hipLaunchKernelGGL((ptk::count64_self_kernel<M, PER_ROW>), grid, block, smem, s, dev, table, first, n, radius, d_radii,
                       max_count, shortcut ? 1u : 0u, d_counts, stack, slots, nullptr);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

template <class M>
int launch_radius64_self_fill(const ptk::DevTree64& dev, uint64_t first, uint64_t n, double radius, const double* d_radii,
                              const uint64_t* d_offsets, ptk::Neighbor64* d_out, ptk::Rec64* stack, uint32_t slots,
                              hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = ptk::lds64_bytes(0, dev.dim);
  ptkd::with_bool(d_radii != nullptr, [&](auto PER_ROW) {
    hipLaunchKernelGGL((ptk::radius64_self_fill_kernel<M, PER_ROW>), grid, block, smem, s, dev, first, n, radius, d_radii,
                       d_offsets, d_out, stack, slots);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// cluster_within_self: one traversal pass over leaf positions [first, first + n) (ptkf::ClusterPass).  Profile kinds: the
// mark and border passes count as the search, the link pass as its tail.
template <int S, int OVF, class M>
int launch_cluster_self(const ptk_tree* t, int pass, uint64_t first, uint64_t n, float radius, const float* d_radii,
                        uint64_t min_neighbors, bool shortcut, bool compress, int32_t* d_labels, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = (size_t)S * 64 * 8;
  const auto* table = static_cast<const ptk::CountBox*>(t->d_count_table);
  Timer timer(t, s);
  ptkd::with_bools(d_radii != nullptr, compress, [&](auto PER_ROW, auto COMPRESS) {
    if (pass == ptkf::kClusterMark)
      hipLaunchKernelGGL((ptk::count_self_kernel<S, OVF, 64, kGenLeafB, PER_ROW, M, ptk::ClusterMarkStore>), grid, block,
                         smem, s, t->dev, table, t->dim, first, n, radius, d_radii, min_neighbors, shortcut ? 1u : 0u,
                         d_labels, nullptr);
    else if (pass == ptkf::kClusterLink)
      hipLaunchKernelGGL((ptk::cluster_link_kernel<S, OVF, 64, kGenLeafB, PER_ROW, COMPRESS, M>), grid, block, smem, s,
                         t->dev, t->dim, first, n, radius, d_radii, d_labels);
    else
      hipLaunchKernelGGL((ptk::cluster_border_kernel<S, OVF, 64, kGenLeafB, PER_ROW, M>), grid, block, smem, s, t->dev,
                         t->dim, first, n, radius, d_radii, d_labels);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(pass == ptkf::kClusterLink ? 3 : 0, n);
  return PTK_OK;
}

template <class M>
int launch_cluster64_self(const ptk::DevTree64& dev, const ptk::CountBox64* table, int pass, uint64_t first, uint64_t n,
                          double radius, const double* d_radii, uint64_t min_neighbors, bool shortcut, bool compress,
                          int32_t* d_labels, ptk::Rec64* stack, uint32_t slots, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = ptk::lds64_bytes(0, dev.dim);
  ptkd::with_bools(d_radii != nullptr, compress, [&](auto PER_ROW, auto COMPRESS) {
    if (pass == ptkf::kClusterMark)
      hipLaunchKernelGGL((ptk::count64_self_kernel<M, PER_ROW, ptk::ClusterMarkStore>), grid, block, smem, s, dev, table,
                         first, n, radius, d_radii, min_neighbors, shortcut ? 1u : 0u, d_labels, stack, slots, nullptr);
    else if (pass == ptkf::kClusterLink)
      hipLaunchKernelGGL((ptk::cluster64_link_kernel<M, PER_ROW, COMPRESS>), grid, block, smem, s, dev, first, n, radius,
                         d_radii, d_labels, stack, slots);
    else
      hipLaunchKernelGGL((ptk::cluster64_border_kernel<M, PER_ROW>), grid, block, smem, s, dev, first, n, radius, d_radii,
                         d_labels, stack, slots);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// normals_within_self: the launch geometry of the self fill kernel.
template <int S, int OVF, class M>
int launch_frames_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii,
                       uint64_t min_neighbors, const float* view, ptk::lf::frame3* d_frames, ptk::lf::moments3* d_moments,
                       hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  const uint32_t has_view = view != nullptr ? 1u : 0u;
  const float vx = view != nullptr ? view[0] : 0.0f, vy = view != nullptr ? view[1] : 0.0f, vz = view != nullptr ? view[2] : 0.0f;
  Timer timer(t, s);
  ptkd::with_bool(d_radii != nullptr, [&](auto PER_ROW) {
    hipLaunchKernelGGL((ptk::frames_self_kernel<S, OVF, 64, kGenLeafB, PER_ROW, M>), dim3(blocks), dim3(64),
                       (size_t)S * 64 * 8, s, t->dev, t->dim, first, n, radius, d_radii, min_neighbors, has_view, vx, vy,
                       vz, d_frames, d_moments);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, n);
  return PTK_OK;
}

// aggregate_within_self: the launch geometry of the self fill kernel, one launch per channel window.
template <int S, int OVF, class M>
int launch_aggregate_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii,
                          const float* d_values, uint32_t channels, uint32_t flags, float* d_out, uint64_t* d_counts,
                          hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  Timer timer(t, s);
  ptkd::with_bool(d_radii != nullptr, [&](auto per_row) {
    constexpr bool PER_ROW = decltype(per_row)::value;
    return ptk::aggregate_windows(d_values, d_out, channels, [&](auto W, auto VEC, uint32_t c0, uint32_t w) {
      hipLaunchKernelGGL((ptk::aggregate_self_kernel<W, VEC, S, OVF, 64, kGenLeafB, PER_ROW, M>), dim3(blocks), dim3(64),
                         (size_t)S * 64 * 8, s, t->dev, t->dim, first, n, radius, d_radii, d_values, channels, c0, w, flags,
                         d_out, d_counts);
      return PTK_OK;
    });
  });
  PTK_HIP(hipGetLastError());
  timer.stop(0, n);
  return PTK_OK;
}

static __global__ void warm_self_kernel() {}

}  // namespace

namespace ptkf {

int knn_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, ptk::Neighbor* d_out, hipStream_t s) {
  if (k + 1 > 64u || t->dim > 3) return fail(PTK_ERR_INVALID, "knn_self: not a call of the direct kernel");
  return with_metric_ovf(t, kGenRing, [&](auto m, auto ovf) {
    return launch_knn_self<ovf, ptkd::type_of<decltype(m)>>(t, first, n, k, d_out, s);
  });
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

int count_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, uint64_t max_count,
               bool shortcut, uint64_t* d_counts, hipStream_t s) {
  if (t->dim > 3) return fail(PTK_ERR_INVALID, "count_self: not a call of the self kernels");
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_count_self<16, ovf, ptkd::type_of<decltype(m)>>(t, first, n, radius, d_radii, max_count, shortcut,
        d_counts, s);
  });
}

int radius_self_fill(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii,
                     const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  if (t->dim > 3) return fail(PTK_ERR_INVALID, "radius_self_fill: not a call of the self kernels");
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_radius_self_fill<16, ovf, ptkd::type_of<decltype(m)>>(t, first, n, radius, d_radii, d_offsets, d_out, s);
  });
}

int count64_self(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, uint64_t first, uint64_t n,
                 double radius, const double* d_radii, uint64_t max_count, bool shortcut, uint64_t* d_counts,
                 ptk::Rec64* stack, uint32_t slots, hipStream_t s) {
  return ptkd::with_euclid64(metric, [&](auto m) {
    return launch_count64_self<ptkd::type_of<decltype(m)>>(dev, table, first, n, radius, d_radii, max_count, shortcut,
                                                      d_counts, stack, slots, s);
  });
}

int radius64_self_fill(const ptk::DevTree64& dev, int metric, uint64_t first, uint64_t n, double radius, const double* d_radii,
                       const uint64_t* d_offsets, void* d_out, ptk::Rec64* stack, uint32_t slots, hipStream_t s) {
  auto* o = static_cast<ptk::Neighbor64*>(d_out);
  return ptkd::with_euclid64(metric, [&](auto m) {
    return launch_radius64_self_fill<ptkd::type_of<decltype(m)>>(dev, first, n, radius, d_radii, d_offsets, o, stack, slots,
                                                            s);
  });
}

int cluster_self(const ptk_tree* t, int pass, uint64_t first, uint64_t n, float radius, const float* d_radii,
                 uint64_t min_neighbors, bool shortcut, bool compress, int32_t* d_labels, hipStream_t s) {
  if (t->dim > 3) return fail(PTK_ERR_INVALID, "cluster_self: not a call of the self kernels");
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_cluster_self<16, ovf, ptkd::type_of<decltype(m)>>(t, pass, first, n, radius, d_radii, min_neighbors,
        shortcut, compress, d_labels, s);
  });
}

int cluster64_self(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, int pass, uint64_t first, uint64_t n,
                   double radius, const double* d_radii, uint64_t min_neighbors, bool shortcut, bool compress,
                   int32_t* d_labels, ptk::Rec64* stack, uint32_t slots, hipStream_t s) {
  return ptkd::with_euclid64(metric, [&](auto m) {
    return launch_cluster64_self<ptkd::type_of<decltype(m)>>(dev, table, pass, first, n, radius, d_radii, min_neighbors,
                                                            shortcut, compress, d_labels, stack, slots, s);
  });
}

int frames_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, uint64_t min_neighbors,
                const float* view, ptk_frame* d_frames, ptk_moments* d_moments, hipStream_t s) {
  static_assert(sizeof(ptk_frame) == sizeof(ptk::lf::frame3) && sizeof(ptk_moments) == sizeof(ptk::lf::moments3), "record layout");
  if (t->dim != 3) return fail(PTK_ERR_INVALID, "frames_self: not a call of the frames kernel");
  auto* frames = reinterpret_cast<ptk::lf::frame3*>(d_frames);
  auto* moments = reinterpret_cast<ptk::lf::moments3*>(d_moments);
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_frames_self<16, ovf, ptkd::type_of<decltype(m)>>(t, first, n, radius, d_radii, min_neighbors, view, frames,
                                                                  moments, s);
  });
}

int aggregate_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, const float* d_values,
                   uint32_t channels, uint32_t flags, float* d_out, uint64_t* d_counts, hipStream_t s) {
  if (t->dim > 3) return fail(PTK_ERR_INVALID, "aggregate_self: not a call of the self kernels");
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_aggregate_self<16, ovf, ptkd::type_of<decltype(m)>>(t, first, n, radius, d_radii, d_values, channels, flags,
                                                                     d_out, d_counts, s);
  });
}

int cluster_elementwise(int pass, uint64_t n, bool compress, int32_t* d_labels, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
  if (pass == kClusterInit) hipLaunchKernelGGL(ptk::cluster_init_kernel, grid, block, 0, s, n, d_labels);
  else if (pass == kClusterDecode) hipLaunchKernelGGL(ptk::cluster_decode_kernel, grid, block, 0, s, n, d_labels);
  else ptkd::with_bool(compress, [&](auto COMPRESS) {
    hipLaunchKernelGGL(ptk::cluster_flatten_kernel<COMPRESS>, grid, block, 0, s, n, d_labels);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// (loads this unit's code object on the calling thread's device: ProcessWarmup of ptk_backend.hip)
void warm_self() {
  hipLaunchKernelGGL(warm_self_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
