// ptk_family_nd.hip -- the searches of trees of any dimension > 3 (ptk_kernels_nd.hpp): k-NN, radius (traversal and captured log), trees
// deeper than the private stack classes.
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_nd.hpp"

namespace {

template <int OVF, class M = ptk::MetricL2>
int launch_knn_nd(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
                  ptk::Neighbor* d_out, hipStream_t s, bool no_register_list = false) {
  constexpr int S = 16;
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  const size_t base = (size_t)S * 64 * 8 + (size_t)t->dim * 64 * 8;
  if (base > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  if (k <= 64 && !no_register_list) {  // k-list in registers (K = 4 / 8 / 16 / 32 / 64 slots compiled)
    Timer timer(t, s);
    const int rc = ptkd::with_slots<4, 8, 16, 32, 64>(k, [&](auto K) {
      const int lds_rc = allow_lds(ptk::knn_nd_reg_kernel<K, S, OVF, M>, base);
      if (lds_rc == PTK_OK)
        hipLaunchKernelGGL((ptk::knn_nd_reg_kernel<K, S, OVF, M>), dim3(blocks), dim3(64), base, s, t->dev_nd, d_q, perm,
                           nq, k, inv_ratio(e), d_out);
      return lds_rc;
    });
    if (rc != PTK_OK) return rc;
    PTK_HIP(hipGetLastError());
    timer.stop(0, nq);
    return PTK_OK;
  }
  const size_t list_bytes = (size_t)k * 64 * 8;
  const bool list_lds = base + list_bytes <= 64 * 1024;
  const size_t smem = base + (list_lds ? list_bytes : 0);
  Timer timer(t, s);
  if (list_lds) {
    hipLaunchKernelGGL((ptk::knn_nd_kernel<S, OVF, true, M>), dim3(blocks), dim3(64), smem, s, t->dev_nd, d_q, perm, nq, k,
                       inv_ratio(e), d_out);
  } else {
    int rc = allow_lds(ptk::knn_nd_kernel<S, OVF, false, M>, smem);
    if (rc != PTK_OK) return rc;
    hipLaunchKernelGGL((ptk::knn_nd_kernel<S, OVF, false, M>), dim3(blocks), dim3(64), smem, s, t->dev_nd, d_q, perm, nq, k,
                       inv_ratio(e), d_out);
  }
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}

// search_knn_within: launch_knn_nd's kernels in their bounded form.  `r`: ptkf::WithinOne (the scalar
// call's kernels) or ptkf::WithinRows (their per-row forms) -- one dispatch for both.
template <int OVF, class M, class R>
int launch_knn_nd_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, const R& r,
                         ptk::Neighbor* d_out, hipStream_t s) {
  constexpr int S = 16;
  constexpr bool kRows = ptkf::within_rows<R>::value;
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  const size_t base = (size_t)S * 64 * 8 + (size_t)t->dim * 64 * 8;
  if (base > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  Timer timer(t, s);
  // (`a`, `b`: the two arguments a bounded kernel ends with -- the scalar call's or the per-row call's; `smem` bytes of LDS)
  auto launch = [&](auto kernel, size_t smem, auto a, auto b) {
    const int lds_rc = allow_lds(kernel, smem);
    if (lds_rc == PTK_OK) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), smem, s, t->dev_nd, d_q, perm, nq, k, d_out, a,
                                             b);
    return lds_rc;
  };
  int rc;
  if (k <= 64) {
    rc = ptkd::with_slots<4, 8, 16, 32, 64>(k, [&](auto K) {
      if constexpr (kRows) return launch(ptk::knn_nd_reg_within_radii_kernel<K, S, OVF, M>, base, r.radii, r.unseeded);
      else return launch(ptk::knn_nd_reg_within_kernel<K, S, OVF, M>, base, r.seed, r.radius);
    });
  } else {
    const size_t list_bytes = (size_t)k * 64 * 8;
    rc = ptkd::with_bool(base + list_bytes <= 64 * 1024, [&](auto LDS) {
      const size_t smem = base + (LDS ? list_bytes : 0);
      if constexpr (kRows) return launch(ptk::knn_nd_within_radii_kernel<S, OVF, LDS, M>, smem, r.radii, r.unseeded);
      else return launch(ptk::knn_nd_within_kernel<S, OVF, LDS, M>, smem, r.seed, r.radius);
    });
  }
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}

template <int OVF, class M = ptk::MetricL2>
int launch_radius_nd(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, float e, bool fill,
                     uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s,
                     const uint32_t* perm = nullptr, const uint32_t* n_dev = nullptr) {
  constexpr int S = 16;
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  const size_t smem = (size_t)S * 64 * 8 + (size_t)t->dim * 64 * 8;
  if (smem > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  Timer timer(t, s);
  const int rc = ptkd::with_bool(fill, [&](auto FILL) {
    const int lds_rc = allow_lds(ptk::radius_nd_kernel<S, OVF, FILL, M>, smem);
    if (lds_rc == PTK_OK)
      hipLaunchKernelGGL((ptk::radius_nd_kernel<S, OVF, FILL, M>), dim3(blocks), dim3(64), smem, s, t->dev_nd, d_q, nq,
                         radius, inv_ratio(e), d_counts, d_offsets, d_out, perm, FILL ? n_dev : nullptr);
    return lds_rc;
  });
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipGetLastError());
  timer.stop(0, n_dev ? 0 : nq);
  return PTK_OK;
}

template <int OVF, class M = ptk::MetricL2>
int launch_radius_nd_capture(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius,
                             float e, uint64_t* d_counts, const ptk::RadiusCapture& cap, hipStream_t s) {
  constexpr int S = 16;
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  const size_t smem = (size_t)S * 64 * 8 + (size_t)t->dim * 64 * 8 + 16;  // + the cursor of the wavefront's log
  if (smem > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  Timer timer(t, s);
  int rc = allow_lds(ptk::radius_nd_capture_kernel<S, OVF, M>, smem);
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipMemsetAsync(cap.counters, 0, ptk::kCapSubPools * ptk::kCapCounterStride * 4, s));
  hipLaunchKernelGGL((ptk::radius_nd_capture_kernel<S, OVF, M>), dim3(blocks), dim3(64), smem, s, t->dev_nd, d_q, perm,
                     nq, radius, inv_ratio(e), d_counts, cap);
  PTK_HIP(hipGetLastError());
  timer.stop(0, nq);
  return PTK_OK;
}


static __global__ void warm_nd_kernel() {}

}  // namespace

namespace ptkf {

int knn_nd(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
           ptk::Neighbor* d_out, hipStream_t s, bool no_register_list) {
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_knn_nd<ovf, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, k, e, d_out, s, no_register_list);
  });
}

int knn_nd_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float seed,
                  float radius, ptk::Neighbor* d_out, hipStream_t s) {
  const WithinOne<float> r{seed, radius};
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_knn_nd_within<ovf, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, k, r, d_out, s);
  });
}

// search_knn_within_radii (ptk.h): unseeded where within_seed() (ptk_backend.hip) says so for the whole call.
int knn_nd_within_radii(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k,
                        const float* d_radii, ptk::Neighbor* d_out, hipStream_t s) {
  const WithinRows<float> r{d_radii, unseeded_metric(t->metric.load()) ? 1u : 0u};
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_knn_nd_within<ovf, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, k, r, d_out, s);
  });
}

// knn_nd_deep for search_knn_within: unseeded, masked at `radius` when the row is stored.
int knn_nd_within_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k, float radius,
                       ptk::Neighbor* d_out, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  const size_t smem = (size_t)16 * 64 * 8 + (size_t)t->dim * 64 * 8;
  if (smem > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  const int rc = ptkd::with_metric(t->metric.load(), [&](auto m) {
    using M = ptkd::type_of<decltype(m)>;
    const int lds_rc = allow_lds(ptk::knn_nd_within_kernel<16, -1, false, M>, smem);
    if (lds_rc == PTK_OK)
      hipLaunchKernelGGL((ptk::knn_nd_within_kernel<16, -1, false, M>), dim3(blocks), dim3(64), smem, s, dev, d_q, nullptr,
                         n, k, d_out, 3.402823466e+38f, radius);
    return lds_rc;
  });
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// ... and for search_knn_within_radii: unseeded, row j of the piece masked at d_radii[j].
int knn_nd_within_radii_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k,
                             const float* d_radii, ptk::Neighbor* d_out, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  const size_t smem = (size_t)16 * 64 * 8 + (size_t)t->dim * 64 * 8;
  if (smem > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  const int rc = ptkd::with_metric(t->metric.load(), [&](auto m) {
    using M = ptkd::type_of<decltype(m)>;
    const int lds_rc = allow_lds(ptk::knn_nd_within_radii_kernel<16, -1, false, M>, smem);
    if (lds_rc == PTK_OK)
      hipLaunchKernelGGL((ptk::knn_nd_within_radii_kernel<16, -1, false, M>), dim3(blocks), dim3(64), smem, s, dev, d_q,
                         nullptr, n, k, d_out, d_radii, 1u);
    return lds_rc;
  });
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int knn_nd_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k, float e,
                ptk::Neighbor* d_out, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  const size_t smem = (size_t)16 * 64 * 8 + (size_t)t->dim * 64 * 8;
  if (smem > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  const int rc = ptkd::with_metric(t->metric.load(), [&](auto m) {
    using M = ptkd::type_of<decltype(m)>;
    const int lds_rc = allow_lds(ptk::knn_nd_kernel<16, -1, false, M>, smem);
    if (lds_rc == PTK_OK)
      hipLaunchKernelGGL((ptk::knn_nd_kernel<16, -1, false, M>), dim3(blocks), dim3(64), smem, s, dev, d_q, nullptr, n, k,
                         inv_ratio(e), d_out);
    return lds_rc;
  });
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int radius_nd(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, float e, bool fill, uint64_t* d_counts,
              const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s, const uint32_t* perm, const uint32_t* n_dev) {
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_radius_nd<ovf, ptkd::type_of<decltype(m)>>(t, d_q, nq, radius, e, fill, d_counts, d_offsets, d_out, s,
                                                        perm, n_dev);
  });
}

int radius_nd_capture(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e,
                      uint64_t* d_counts, const ptk::RadiusCapture& cap, hipStream_t s) {
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_radius_nd_capture<ovf, ptkd::type_of<decltype(m)>>(t, d_q, perm, nq, radius, e, d_counts, cap, s);
  });
}

int radius_nd_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, float radius, float e,
                   bool fill, uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  const size_t smem = (size_t)16 * 64 * 8 + (size_t)t->dim * 64 * 8;
  if (smem > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device search", t->dim);
  const int rc = ptkd::with_metric(t->metric.load(), [&](auto m) {
    return ptkd::with_bool(fill, [&](auto FILL) {
      using M = ptkd::type_of<decltype(m)>;
      const int lds_rc = allow_lds(ptk::radius_nd_kernel<16, -1, FILL, M>, smem);
      if (lds_rc == PTK_OK)
        hipLaunchKernelGGL((ptk::radius_nd_kernel<16, -1, FILL, M>), dim3(blocks), dim3(64), smem, s, dev, d_q, n, radius,
                           inv_ratio(e), d_counts, d_offsets, d_out, nullptr, nullptr);
      return lds_rc;
    });
  });
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// (loads this unit's code object on the calling thread's device: ProcessWarmup of ptk_backend.hip)
void warm_nd() {
  hipLaunchKernelGGL(warm_nd_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
