// tests/cpp/emulate_align.cpp -- TEST INFRASTRUCTURE: the kernels of align_step (pico_tree_amd/csrc/ptk_kernels_align.hpp,
// K22: align_pose_kernel, align_inverse_kernel, align_terms_kernel, align_reduce_kernel, align_finish_kernel) run lane by
// lane on the CPU, on the emulator of tests/cpp/emulate_kernels.cpp: the wavefronts of the two reducing kernels as 64
// fibers that meet at every shuffle.  The rows are the caller's (the kernels do not search).  Built by
// tests/test_align_step.py with the emulator's g++ line and HIP stand-in.

#include "emulate_kernels.cpp"
#include "ptk_kernels_align.hpp"

extern "C" {

// The record (384 bytes) of the kernels over `rows` (nq entries, e.g. the host loop's) of the queries q [nq, 3] posed by
// `transform` (12 floats or null); `normals` null: point-to-point.  `posed` (nq x 3, may be null) receives q'.
int emu_align_step(void* h, const float* q, uint64_t nq, const float* transform, float max_distance, const float* normals,
                   const ptk::Neighbor* rows, void* out, float* posed) {
  auto* t = static_cast<Emu*>(h);
  if (t->dim != 3) return -1;
  namespace al = pico_tree::internal;
  const bool plane = normals != nullptr;
  auto* words = static_cast<unsigned long long*>(out);
  if (nq == 0) {
    for_each_lane(64, [&] { ptk::align_finish_kernel(nullptr, nullptr, plane ? 1 : 0, nq, words); }, 64);
    return 0;
  }
  const uint32_t n_points = t->dev.n_points;
  std::vector<uint32_t> inv(n_points, 0xFFFFFFFFu);
  for_each_lane(n_points, [&] { ptk::align_inverse_kernel(t->dev.pts, n_points, inv.data()); }, 256);
  std::vector<float> qp(q, q + 3 * nq);
  if (transform != nullptr) {
    ptk::AlignPose pose;
    std::memcpy(pose.m, transform, sizeof pose.m);
    for_each_lane(nq, [&] { ptk::align_pose_kernel(q, nq, pose, qp.data()); }, 256);
  }
  if (posed != nullptr) std::memcpy(posed, qp.data(), qp.size() * sizeof(float));
  const int terms = al::align_terms(plane);
  uint64_t n = al::align_blocks(nq);
  std::vector<double> sums((size_t)n * terms);
  std::vector<uint64_t> counts((size_t)n);
  for_each_wave((uint32_t)n, [&] {
    if (plane)
      ptk::align_terms_kernel<true>(rows, qp.data(), nq, inv.data(), t->dev.pts, n_points, normals, max_distance, n, sums.data(),
                                    counts.data());
    else
      ptk::align_terms_kernel<false>(rows, qp.data(), nq, inv.data(), t->dev.pts, n_points, normals, max_distance, n,
                                     sums.data(), counts.data());
  });
  while (n > 1) {
    const uint64_t m = al::align_blocks(n);
    std::vector<double> next((size_t)m * terms);
    std::vector<uint64_t> next_counts((size_t)m);
    for_each_wave((uint32_t)m, [&] {
      ptk::align_reduce_kernel(sums.data(), counts.data(), n, terms, m, next.data(), next_counts.data());
    });
    sums.swap(next);
    counts.swap(next_counts);
    n = m;
  }
  for_each_lane(64, [&] { ptk::align_finish_kernel(sums.data(), counts.data(), plane ? 1 : 0, nq, words); }, 64);
  return 0;
}

}  // extern "C"
