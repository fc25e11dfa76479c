// tests/cpp/spacing_self_main.cpp -- TEST PROGRAM for kd_tree::spacing_knn_self / outliers_knn_self
// (include/pico_tree/kd_tree.hpp).  Built with -DPICO_TREE_HOST_ONLY (no backend linked): the members run the per-point
// member and the rule of pico_tree/internal/spacing.hpp.  Built without it and linked to libptk.so: the batched members
// on the device.
//
//   spacing_self_main <dir> <k> <ratio>
//
// <dir> holds points.bin (float32 row-major, 3-D) written by tests/test_spacing_self.py.  For a float tree under L2 squared
// (l2, the square root on), under L1 (l1, off) and a double tree (l2d, on) it writes <name>.mean, <name>.kth (scalars),
// <name>.keep (uint8) and <name>.stats (64 bytes); the driver compares them with its expected arrays.

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

static void write_bytes(std::string const& path, void const* p, size_t bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(static_cast<char const*>(p), static_cast<std::streamsize>(bytes));
}

template <typename Tree, typename Scalar>
static int run(Tree const& tree, size_t n, size_t k, float ratio, bool sqrt, std::string const& name) {
  std::vector<Scalar> mean(n, Scalar(-7)), kth(n, Scalar(-7)), only(n, Scalar(-7));
  tree.spacing_knn_self(k, sqrt, mean.data(), kth.data());
  tree.spacing_knn_self(k, sqrt, only.data());
  if (only != mean) return 4;
  std::vector<std::uint8_t> keep(n, 7), again(n, 7);
  pico_tree::spacing_stats stats;
  tree.outliers_knn_self(k, ratio, sqrt, keep.data(), &stats);
  tree.outliers_knn_self(k, ratio, sqrt, again.data());
  if (again != keep) return 5;
  write_bytes(name + ".mean", mean.data(), n * sizeof(Scalar));
  write_bytes(name + ".kth", kth.data(), n * sizeof(Scalar));
  write_bytes(name + ".keep", keep.data(), n);
  write_bytes(name + ".stats", &stats, sizeof stats);
  int threw = 0;
  try {
    tree.spacing_knn_self(0, sqrt, mean.data());
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  float const bad[3] = {-1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
  for (float r : bad) {
    try {
      tree.outliers_knn_self(k, r, sqrt, keep.data());
    } catch (std::invalid_argument const&) {
      ++threw;
    }
  }
  return threw == 4 ? 0 : 6;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: spacing_self_main <dir> <k> <ratio>\n");
    return 2;
  }
  std::string const dir = argv[1];
  size_t const k = static_cast<size_t>(std::stoul(argv[2]));
  float const ratio = std::stof(argv[3]);
  auto const raw = read_floats(dir + "/points.bin");
  auto pf = as_points<float>(raw);
  auto pd = as_points<double>(raw);
  using spacef = std::vector<std::array<float, 3>>;
  using spaced = std::vector<std::array<double, 3>>;
  try {
    pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
    pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
    pico_tree::kd_tree<spaced> l2d(pd, pico_tree::max_leaf_size_t(10));
    int rc = run<decltype(l2), float>(l2, pf.size(), k, ratio, true, dir + "/l2");
    if (rc == 0) rc = run<decltype(l1), float>(l1, pf.size(), k, ratio, false, dir + "/l1");
    if (rc == 0) rc = run<decltype(l2d), double>(l2d, pd.size(), k, ratio, true, dir + "/l2d");
    if (rc != 0) return rc;
  } catch (std::exception const& ex) {
    std::fprintf(stderr, "spacing_self_main: %s\n", ex.what());
    return 3;
  }
  std::printf("ok\n");
  return 0;
}
