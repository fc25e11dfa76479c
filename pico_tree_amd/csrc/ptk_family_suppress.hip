// ptk_family_suppress.hip -- suppress_within_self (ptk_kernels_suppress.hpp, K23): the init kernel, the round kernel over
// the tree's own leaf-order records, float32 and float64, written once over its radius source and its order, and the
// counter of undecided lanes the host reads after every round.
// One of the translation units of libptk.so (ptk_backend_core.hpp).

#include "ptk_families.hpp"
#include "ptk_kernels_f64.hpp"
#include "ptk_kernels_suppress.hpp"

namespace {

// One round over leaf positions [first, first + n): the launch geometry of cluster_link_kernel.  Profile kinds: the first
// round counts as the search, the later ones as its tail.
template <int S, int OVF, class M>
int launch_suppress_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii,
                         const float* d_scores, uint8_t* d_keep, uint32_t* d_undecided, bool later_round, hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = (size_t)S * 64 * 8;
  Timer timer(t, s);
  ptkd::with_bools(d_radii != nullptr, d_scores != nullptr, [&](auto PER_ROW, auto SCORED) {
    hipLaunchKernelGGL((ptk::suppress_round_kernel<S, OVF, 64, kGenLeafB, PER_ROW, SCORED, M>), grid, block, smem, s, t->dev,
                       t->dim, first, n, radius, d_radii, d_scores, d_keep, d_undecided);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  timer.stop(later_round ? 3 : 0, n);
  return PTK_OK;
}

template <class M>
int launch_suppress64_self(const ptk::DevTree64& dev, uint64_t first, uint64_t n, double radius, const double* d_radii,
                           const float* d_scores, uint8_t* d_keep, uint32_t* d_undecided, ptk::Rec64* stack, uint32_t slots,
                           hipStream_t s) {
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  const size_t smem = ptk::lds64_bytes(0, dev.dim);
  ptkd::with_bools(d_radii != nullptr, d_scores != nullptr, [&](auto PER_ROW, auto SCORED) {
    hipLaunchKernelGGL((ptk::suppress64_round_kernel<M, PER_ROW, SCORED>), grid, block, smem, s, dev, first, n, radius,
                       d_radii, d_scores, d_keep, d_undecided, stack, slots);
    return PTK_OK;
  });
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

static __global__ void warm_suppress_kernel() {}

}  // namespace

namespace ptkf {

int suppress_init(uint64_t n, uint8_t* d_keep, hipStream_t s) {
  hipLaunchKernelGGL(ptk::suppress_init_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, n, d_keep);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int suppress_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, const float* d_scores,
                  uint8_t* d_keep, uint32_t* d_undecided, bool later_round, hipStream_t s) {
  if (t->dim > 3) return fail(PTK_ERR_INVALID, "suppress_self: not a call of the self kernels");
  return with_metric_ovf(t, 16, [&](auto m, auto ovf) {
    return launch_suppress_self<16, ovf, ptkd::type_of<decltype(m)>>(t, first, n, radius, d_radii, d_scores, d_keep,
                                                                    d_undecided, later_round, s);
  });
}

int suppress64_self(const ptk::DevTree64& dev, int metric, uint64_t first, uint64_t n, double radius, const double* d_radii,
                    const float* d_scores, uint8_t* d_keep, uint32_t* d_undecided, ptk::Rec64* stack, uint32_t slots,
                    hipStream_t s) {
  return ptkd::with_euclid64(metric, [&](auto m) {
    return launch_suppress64_self<ptkd::type_of<decltype(m)>>(dev, first, n, radius, d_radii, d_scores, d_keep, d_undecided,
                                                             stack, slots, s);
  });
}

namespace {
// The idle counters of every device (SuppressCounter, ptk_families.hpp): never freed.
struct CounterPool {
  struct Pair {
    uint32_t *d_word, *h_word;
    int device;
  };
  std::mutex mutex;
  std::vector<Pair> idle;
};
CounterPool& counter_pool() {
  static CounterPool* pool = new CounterPool;  // (outlives every static destructor: a late call still finds it)
  return *pool;
}
}  // namespace

SuppressCounter::~SuppressCounter() {
  if (d_word == nullptr || h_word == nullptr) return;
  CounterPool& pool = counter_pool();
  std::lock_guard<std::mutex> lock(pool.mutex);
  pool.idle.push_back(CounterPool::Pair{d_word, h_word, device});
}

int SuppressCounter::alloc() {
  if (hipGetDevice(&device) != hipSuccess) return fail(PTK_ERR_DEVICE, "hipGetDevice failed");
  {
    CounterPool& pool = counter_pool();
    std::lock_guard<std::mutex> lock(pool.mutex);
    for (size_t i = 0; i < pool.idle.size(); ++i) {
      if (pool.idle[i].device != device) continue;
      d_word = pool.idle[i].d_word;
      h_word = pool.idle[i].h_word;
      pool.idle.erase(pool.idle.begin() + (std::ptrdiff_t)i);
      return PTK_OK;
    }
  }
  uint32_t *d = nullptr, *h = nullptr;
  if (hipMalloc((void**)&d, sizeof(uint32_t)) != hipSuccess ||
      hipHostMalloc((void**)&h, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    if (d != nullptr) (void)hipFree(d);
    return fail(PTK_ERR_NOMEM, "out of memory (the round counter of suppress_within_self)");
  }
  d_word = d;
  h_word = h;
  return PTK_OK;
}

int SuppressCounter::zero(hipStream_t s) {
  PTK_HIP(hipMemsetAsync(d_word, 0, sizeof(uint32_t), s));
  return PTK_OK;
}

int SuppressCounter::read(hipStream_t s, uint32_t* undecided) {
  PTK_HIP(hipMemcpyAsync(h_word, d_word, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PTK_HIP(hipStreamSynchronize(s));
  *undecided = *h_word;
  return PTK_OK;
}

void warm_suppress() {
  hipLaunchKernelGGL(warm_suppress_kernel, dim3(1), dim3(1), 0, nullptr);
}

}  // namespace ptkf
