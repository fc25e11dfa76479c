// tests/cpp/emulate_frames.cpp -- TEST INFRASTRUCTURE: the kernel of normals_within_self
// (pico_tree_amd/csrc/ptk_kernels_frames.hpp: frames_self_kernel) run lane by lane on the CPU, on the emulator of
// tests/cpp/emulate_kernels.cpp with the handles of tests/cpp/emulate_radius_self.cpp.  Built by
// tests/test_normals_self.py with the emulator's g++ line and HIP stand-in.

#include "emulate_radius_self.cpp"
#include "ptk_kernels_frames.hpp"

namespace {

template <class M>
void frames_self_m(Emu* t, uint64_t piece, float radius, const float* radii, uint64_t min_neighbors, const float* view,
                   ptk::lf::frame3* frames, ptk::lf::moments3* moments) {
  const uint64_t n = t->dev.n_points;
  const uint32_t has_view = view != nullptr ? 1u : 0u;
  const float vx = has_view ? view[0] : 0.0f, vy = has_view ? view[1] : 0.0f, vz = has_view ? view[2] : 0.0f;
  for (uint64_t first = 0; first < n; first += piece) {
    const uint64_t m = std::min(piece, n - first);
    if (radii != nullptr)
      for_each_lane(m, [&] {
        ptk::frames_self_kernel<16, 2048, 64, 5, true, M>(t->dev, t->dim, first, m, radius, radii, min_neighbors, has_view, vx,
                                                          vy, vz, frames, moments);
      }, 64);
    else
      for_each_lane(m, [&] {
        ptk::frames_self_kernel<16, 2048, 64, 5, false, M>(t->dev, t->dim, first, m, radius, radii, min_neighbors, has_view, vx,
                                                           vy, vz, frames, moments);
      }, 64);
  }
}

}  // namespace

extern "C" {

// frames / moments (n_points records each by original index, 16-byte aligned, either may be null) of frames_self_kernel
// over every leaf position, `piece` positions per launch (0: all at once); radii null: the scalar form; view null: no
// viewpoint.
int emu_frames_self(void* h, uint64_t piece, float radius, const float* radii, uint64_t min_neighbors, const float* view,
                    void* frames, void* moments) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim != 3) return -1;
  if (t->dev.n_points == 0) return 0;
  if (piece == 0) piece = t->dev.n_points;
  auto* f = static_cast<ptk::lf::frame3*>(frames);
  auto* m = static_cast<ptk::lf::moments3*>(moments);
  switch (t->metric) {
    case 1: frames_self_m<ptk::MetricL1>(t, piece, radius, radii, min_neighbors, view, f, m); break;
    case 2: frames_self_m<ptk::MetricLInf>(t, piece, radius, radii, min_neighbors, view, f, m); break;
    case 3: frames_self_m<ptk::MetricLNInf>(t, piece, radius, radii, min_neighbors, view, f, m); break;
    case 0: frames_self_m<ptk::MetricL2>(t, piece, radius, radii, min_neighbors, view, f, m); break;
    default: return -1;
  }
  return 0;
}

}  // extern "C"
