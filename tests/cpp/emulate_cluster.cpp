// tests/cpp/emulate_cluster.cpp -- TEST INFRASTRUCTURE: the kernels of cluster_within_self
// (pico_tree_amd/csrc/ptk_kernels_cluster.hpp: the mark pass behind count_self_kernel, cluster_link_kernel,
// cluster_flatten_kernel, cluster_border_kernel, cluster_decode_kernel and their float64 pair) run lane by lane on the
// CPU, on the emulator of tests/cpp/emulate_kernels.cpp with the handles and side tables of
// tests/cpp/emulate_radius_self.cpp.  Built by tests/test_cluster_self.py with the emulator's g++ line and HIP stand-in.
//
// Lanes run one after the other, so the stand-ins of the device atomics below are plain reads and writes: what this
// unit checks is the passes' logic (marks, the OR of the edge rule, the border encoding, pieces); that find / unite hold
// under real interleavings is tests/cpp/cluster_threads.cpp's part.

#include "emulate_radius_self.cpp"

#define __HIP_MEMORY_SCOPE_AGENT 4
template <class T>
inline T __hip_atomic_load(const T* p, int, int) {
  return *p;
}
template <class T>
inline T atomicCAS(T* p, T expected, T wanted) {
  const T old = *p;
  if (old == expected) *p = wanted;
  return old;
}
template <class T>
inline T atomicMin(T* p, T v) {
  const T old = *p;
  if (v < old) *p = v;
  return old;
}

#include "ptk_kernels_cluster.hpp"

namespace {

template <class Pass>
void in_pieces(uint64_t n, uint64_t piece, Pass&& pass) {
  for (uint64_t first = 0; first < n; first += piece) pass(first, std::min(piece, n - first));
}

// The passes in the order of ptk_cluster_within_self_device, each over all pieces before the next.
template <class M, bool PER_ROW, bool COMPRESS>
void cluster_m(Emu* t, uint64_t piece, float radius, const float* radii, uint64_t min_neighbors, uint32_t shortcut,
               int32_t* labels) {
  const uint64_t n = t->dev.n_points;
  if (min_neighbors == 0) {
    for_each_lane(n, [&] { ptk::cluster_init_kernel(n, labels); }, 256);
  } else {
    const std::vector<ptk::CountBox> table = table_of(t);
    in_pieces(n, piece, [&](uint64_t first, uint64_t m) {
      for_each_lane(m, [&] {
        ptk::count_self_kernel<16, 2048, 64, 5, PER_ROW, M, ptk::ClusterMarkStore>(
            t->dev, table.data(), t->dim, first, m, radius, radii, min_neighbors, shortcut, labels, nullptr);
      }, 64);
    });
  }
  in_pieces(n, piece, [&](uint64_t first, uint64_t m) {
    for_each_lane(m, [&] {
      ptk::cluster_link_kernel<16, 2048, 64, 5, PER_ROW, COMPRESS, M>(t->dev, t->dim, first, m, radius, radii, labels);
    }, 64);
  });
  for_each_lane(n, [&] { ptk::cluster_flatten_kernel<COMPRESS>(n, labels); }, 256);
  if (min_neighbors == 0) return;
  in_pieces(n, piece, [&](uint64_t first, uint64_t m) {
    for_each_lane(m, [&] {
      ptk::cluster_border_kernel<16, 2048, 64, 5, PER_ROW, M>(t->dev, t->dim, first, m, radius, radii, labels);
    }, 64);
  });
  for_each_lane(n, [&] { ptk::cluster_decode_kernel(n, labels); }, 256);
}

template <class M>
void cluster_any(Emu* t, uint64_t piece, float radius, const float* radii, uint64_t mn, uint32_t sc, int compress,
                 int32_t* labels) {
  if (radii != nullptr && compress) cluster_m<M, true, true>(t, piece, radius, radii, mn, sc, labels);
  else if (radii != nullptr) cluster_m<M, true, false>(t, piece, radius, radii, mn, sc, labels);
  else if (compress) cluster_m<M, false, true>(t, piece, radius, radii, mn, sc, labels);
  else cluster_m<M, false, false>(t, piece, radius, radii, mn, sc, labels);
}

template <class M, bool PER_ROW, bool COMPRESS>
void cluster64_m(Emu64* t, uint64_t piece, double radius, const double* radii, uint64_t min_neighbors, uint32_t shortcut,
                 int32_t* labels) {
  const uint64_t n = t->dev.n_points;
  if (min_neighbors == 0) {
    for_each_lane(n, [&] { ptk::cluster_init_kernel(n, labels); }, 256);
  } else {
    const std::vector<ptk::CountBox64> table = table64_of(t);
    in_pieces(n, piece, [&](uint64_t first, uint64_t m) {
      for_each_lane64(t, m, [&](uint64_t q0, uint64_t k) {
        ptk::count64_self_kernel<M, PER_ROW, ptk::ClusterMarkStore>(t->dev, table.data(), first + q0, k, radius, radii,
                                                                    min_neighbors, shortcut, labels, t->stack.data(),
                                                                    t->slots, nullptr);
      });
    });
  }
  in_pieces(n, piece, [&](uint64_t first, uint64_t m) {
    for_each_lane64(t, m, [&](uint64_t q0, uint64_t k) {
      ptk::cluster64_link_kernel<M, PER_ROW, COMPRESS>(t->dev, first + q0, k, radius, radii, labels, t->stack.data(), t->slots);
    });
  });
  for_each_lane(n, [&] { ptk::cluster_flatten_kernel<COMPRESS>(n, labels); }, 256);
  if (min_neighbors == 0) return;
  in_pieces(n, piece, [&](uint64_t first, uint64_t m) {
    for_each_lane64(t, m, [&](uint64_t q0, uint64_t k) {
      ptk::cluster64_border_kernel<M, PER_ROW>(t->dev, first + q0, k, radius, radii, labels, t->stack.data(), t->slots);
    });
  });
  for_each_lane(n, [&] { ptk::cluster_decode_kernel(n, labels); }, 256);
}

template <class M>
void cluster64_any(Emu64* t, uint64_t piece, double radius, const double* radii, uint64_t mn, uint32_t sc, int compress,
                   int32_t* labels) {
  if (radii != nullptr && compress) cluster64_m<M, true, true>(t, piece, radius, radii, mn, sc, labels);
  else if (radii != nullptr) cluster64_m<M, true, false>(t, piece, radius, radii, mn, sc, labels);
  else if (compress) cluster64_m<M, false, true>(t, piece, radius, radii, mn, sc, labels);
  else cluster64_m<M, false, false>(t, piece, radius, radii, mn, sc, labels);
}

}  // namespace

extern "C" {

// labels (n_points entries) of the passes over every leaf position, `piece` positions per launch (0: all at once);
// radii null: the scalar form.
int emu_cluster_self(void* h, uint64_t piece, float radius, const float* radii, uint64_t min_neighbors, int shortcut,
                     int compress, int32_t* labels) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim > 3) return -1;
  if (t->dev.n_points == 0) return 0;
  if (piece == 0) piece = t->dev.n_points;
  const uint32_t sc = (uint32_t)shortcut;
  switch (t->metric) {
    case 1: cluster_any<ptk::MetricL1>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    case 2: cluster_any<ptk::MetricLInf>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    case 3: cluster_any<ptk::MetricLNInf>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    case 0: cluster_any<ptk::MetricL2>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    default: return -1;
  }
  return 0;
}

int emu64_cluster_self(void* h, uint64_t piece, double radius, const double* radii, uint64_t min_neighbors, int shortcut,
                       int compress, int32_t* labels) {
  auto* t = static_cast<Emu64*>(h);
  if (t->dev.dim > 3) return -1;
  if (t->dev.n_points == 0) return 0;
  if (piece == 0) piece = t->dev.n_points;
  const uint32_t sc = (uint32_t)shortcut;
  switch (t->metric) {
    case 1: cluster64_any<ptk::Metric64L1>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    case 2: cluster64_any<ptk::Metric64LInf>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    case 3: cluster64_any<ptk::Metric64LNInf>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    case 0: cluster64_any<ptk::Metric64L2>(t, piece, radius, radii, min_neighbors, sc, compress, labels); break;
    default: return -1;
  }
  return 0;
}

}  // extern "C"
