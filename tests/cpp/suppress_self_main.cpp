// tests/cpp/suppress_self_main.cpp -- TEST PROGRAM for kd_tree::suppress_within_self (include/pico_tree/kd_tree.hpp).
// Built with -DPICO_TREE_HOST_ONLY (no backend linked): the members run the per-point member plus the greedy pass of
// pico_tree/internal/suppress.hpp.  Built without it and linked to libptk.so: the batched members on the device.
//
//   suppress_self_main <dir> <radius>
//
// <dir> holds points.bin (float32 row-major, 3-D), radii.bin and scores.bin (float32, one per point) written by
// tests/test_suppress_self.py.  Writes <name>_scalar.u8, <name>_radii.u8, <name>_scored.u8 and <name>_radii_scored.u8
// (uint8 cells, n each) for a float tree under L2 squared (l2) and L1 (l1) and a double tree (l2d); the driver compares
// them with its expected arrays.

#include <array>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <limits>
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
static std::vector<std::array<T, 3>> as_points(std::vector<float> const& v) {
  std::vector<std::array<T, 3>> s(v.size() / 3);
  for (size_t i = 0; i < s.size(); ++i) s[i] = {T(v[3 * i]), T(v[3 * i + 1]), T(v[3 * i + 2])};
  return s;
}

static void write_cells(std::string const& path, std::vector<std::uint8_t> const& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v.data()), static_cast<std::streamsize>(v.size()));
}

template <typename Tree, typename Scalar>
static int run(Tree const& tree, size_t n, Scalar radius, std::vector<Scalar> const& radii, std::vector<float> const& scores,
               std::string const& name) {
  std::vector<std::uint8_t> keep(n, 7);
  tree.suppress_within_self(radius, keep.data());
  write_cells(name + "_scalar.u8", keep);
  keep.assign(n, 7);
  tree.suppress_within_self(radii, keep.data());
  write_cells(name + "_radii.u8", keep);
  keep.assign(n, 7);
  tree.suppress_within_self(radius, keep.data(), scores.data());
  write_cells(name + "_scored.u8", keep);
  keep.assign(n, 7);
  tree.suppress_within_self(radii, keep.data(), scores.data());
  write_cells(name + "_radii_scored.u8", keep);
  // (radius 0 keeps everything)
  tree.suppress_within_self(Scalar(0), keep.data());
  for (std::uint8_t c : keep)
    if (c != 1) return 4;
  int threw = 0;
  try {
    std::vector<Scalar> few(radii.begin(), radii.begin() + 5);
    tree.suppress_within_self(few, keep.data());
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  try {
    std::vector<float> bad(scores);
    bad[n / 2] = std::numeric_limits<float>::quiet_NaN();
    tree.suppress_within_self(radius, keep.data(), bad.data());
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  return threw == 2 ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: suppress_self_main <dir> <radius>\n");
    return 2;
  }
  std::string const dir = argv[1];
  float const radius = std::stof(argv[2]);
  auto const raw = read_floats(dir + "/points.bin");
  auto const rf = read_floats(dir + "/radii.bin");
  auto const scores = read_floats(dir + "/scores.bin");
  std::vector<double> const rd(rf.begin(), rf.end());
  auto pf = as_points<float>(raw);
  auto pd = as_points<double>(raw);
  using spacef = std::vector<std::array<float, 3>>;
  using spaced = std::vector<std::array<double, 3>>;
  try {
    pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
    pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
    pico_tree::kd_tree<spaced> l2d(pd, pico_tree::max_leaf_size_t(10));
    int rc = run(l2, pf.size(), radius, rf, scores, dir + "/l2");
    if (rc == 0) rc = run(l1, pf.size(), radius, rf, scores, dir + "/l1");
    if (rc == 0) rc = run(l2d, pd.size(), static_cast<double>(radius), rd, scores, dir + "/l2d");
    if (rc != 0) return rc;
  } catch (std::exception const& ex) {
    std::fprintf(stderr, "suppress_self_main: %s\n", ex.what());
    return 3;
  }
  std::printf("ok\n");
  return 0;
}
