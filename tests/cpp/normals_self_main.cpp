// tests/cpp/normals_self_main.cpp -- TEST PROGRAM for kd_tree::normals_within_self (include/pico_tree/kd_tree.hpp).
// Built with -DPICO_TREE_HOST_ONLY (no backend linked: the members run the per-point member with the routine of
// pico_tree/internal/local_frame.hpp) and, for the gpu tier, against libptk.so (the members go through the backend).
//
//   normals_self_main <dir> <radius> <min_neighbors> <leaf size> <l2|l1|lpinf|lninf> [vx vy vz]
//
// <dir> holds points.bin (float32 row-major, 3-D) and radii.bin (float32, one per point) written by
// tests/test_normals_self.py.  Writes scalar.frm / scalar.mom and radii.frm / radii.mom (the 32-byte frames and 48-byte
// moments, n each); the driver compares them byte for byte with the library's.

#include <array>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <pico_tree/array_traits.hpp>
#include <pico_tree/kd_tree.hpp>
#include <pico_tree/vector_traits.hpp>

static std::vector<float> read_floats(std::string const& path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error("cannot open " + path);
  std::streamsize bytes = f.tellg();
  f.seekg(0);
  std::vector<float> v(static_cast<size_t>(bytes) / sizeof(float));
  f.read(reinterpret_cast<char*>(v.data()), bytes);
  return v;
}

template <typename T>
static void write_records(std::string const& path, std::vector<T> const& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

using space = std::vector<std::array<float, 3>>;

template <typename Metric>
static int run(space const& pts, size_t leaf, float radius, std::vector<float> const& radii, size_t min_neighbors,
               float const* view, std::string const& dir) {
  pico_tree::kd_tree<space, Metric> tree(pts, pico_tree::max_leaf_size_t(leaf));
  std::vector<pico_tree::local_frame> frames, only;
  std::vector<pico_tree::local_moments> moments;
  tree.normals_within_self(radius, frames, min_neighbors, view, &moments);
  if (frames.size() != pts.size() || moments.size() != pts.size()) return 3;
  write_records(dir + "/scalar.frm", frames);
  write_records(dir + "/scalar.mom", moments);
  // (without the moments: the same frames)
  tree.normals_within_self(radius, only, min_neighbors, view);
  if (only.size() != frames.size()) return 4;
  for (size_t i = 0; i < only.size(); ++i)
    if (std::memcmp(&only[i], &frames[i], sizeof only[i]) != 0) return 4;
  tree.normals_within_self(radii, frames, min_neighbors, view, &moments);
  write_records(dir + "/radii.frm", frames);
  write_records(dir + "/radii.mom", moments);
  bool threw = false;
  try {
    std::vector<float> few(radii.begin(), radii.begin() + 5);
    tree.normals_within_self(few, frames);
  } catch (std::invalid_argument const&) {
    threw = true;
  }
  return threw ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc != 6 && argc != 9) {
    std::fprintf(stderr, "usage: normals_self_main <dir> <radius> <min_neighbors> <leaf> <metric> [vx vy vz]\n");
    return 2;
  }
  std::string const dir = argv[1];
  float const radius = std::stof(argv[2]);
  size_t const min_neighbors = std::stoul(argv[3]);
  size_t const leaf = std::stoul(argv[4]);
  std::string const metric = argv[5];
  float view[3] = {0, 0, 0};
  if (argc == 9)
    for (int a = 0; a < 3; ++a) view[a] = std::stof(argv[6 + a]);
  float const* vp = argc == 9 ? view : nullptr;
  auto const raw = read_floats(dir + "/points.bin");
  auto const radii = read_floats(dir + "/radii.bin");
  space pts(raw.size() / 3);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = {raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]};
  int rc = 2;
  if (metric == "l2") rc = run<pico_tree::metric_l2_squared>(pts, leaf, radius, radii, min_neighbors, vp, dir);
  else if (metric == "l1") rc = run<pico_tree::metric_l1>(pts, leaf, radius, radii, min_neighbors, vp, dir);
  else if (metric == "lpinf") rc = run<pico_tree::metric_lpinf>(pts, leaf, radius, radii, min_neighbors, vp, dir);
  else if (metric == "lninf") rc = run<pico_tree::metric_lninf>(pts, leaf, radius, radii, min_neighbors, vp, dir);
  if (rc != 0) return rc;
  std::printf("ok\n");
  return 0;
}
