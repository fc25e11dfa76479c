// tests/cpp/cluster_self_main.cpp -- TEST PROGRAM for kd_tree::cluster_within_self (include/pico_tree/kd_tree.hpp).
// Built with -DPICO_TREE_HOST_ONLY (no backend linked): the members run the per-point member plus the union-find of
// pico_tree/internal/cluster.hpp.
//
//   cluster_self_main <dir> <radius> <min_neighbors>
//
// <dir> holds points.bin (float32 row-major, 3-D) and radii.bin (float32, one per point) written by
// tests/test_cluster_self.py.  Writes <name>_scalar.i32 and <name>_radii.i32 (int32 labels, n each) for a float tree
// under L2 squared (l2) and L1 (l1) and a double tree (l2d); the driver compares them with its expected labels.

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
static std::vector<std::array<T, 3>> as_points(std::vector<float> const& v) {
  std::vector<std::array<T, 3>> s(v.size() / 3);
  for (size_t i = 0; i < s.size(); ++i) s[i] = {T(v[3 * i]), T(v[3 * i + 1]), T(v[3 * i + 2])};
  return s;
}

static void write_labels(std::string const& path, std::vector<std::int32_t> const& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(std::int32_t)));
}

template <typename Tree, typename Scalar>
static int run(Tree const& tree, size_t n, Scalar radius, std::vector<Scalar> const& radii, size_t min_neighbors,
               std::string const& name) {
  std::vector<std::int32_t> labels(n, -7);
  tree.cluster_within_self(radius, labels.data(), min_neighbors);
  write_labels(name + "_scalar.i32", labels);
  labels.assign(n, -7);
  tree.cluster_within_self(radii, labels.data(), min_neighbors);
  write_labels(name + "_radii.i32", labels);
  // (the default is plain connected components: every point is core, nothing is noise)
  tree.cluster_within_self(radius, labels.data());
  for (std::int32_t l : labels)
    if (l < 0) return 4;
  bool threw = false;
  try {
    std::vector<Scalar> few(radii.begin(), radii.begin() + 5);
    tree.cluster_within_self(few, labels.data());
  } catch (std::invalid_argument const&) {
    threw = true;
  }
  return threw ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: cluster_self_main <dir> <radius> <min_neighbors>\n");
    return 2;
  }
  std::string const dir = argv[1];
  float const radius = std::stof(argv[2]);
  size_t const min_neighbors = std::stoul(argv[3]);
  auto const raw = read_floats(dir + "/points.bin");
  auto const rf = read_floats(dir + "/radii.bin");
  std::vector<double> const rd(rf.begin(), rf.end());
  auto pf = as_points<float>(raw);
  auto pd = as_points<double>(raw);
  using spacef = std::vector<std::array<float, 3>>;
  using spaced = std::vector<std::array<double, 3>>;
  pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spaced> l2d(pd, pico_tree::max_leaf_size_t(10));
  int rc = run(l2, pf.size(), radius, rf, min_neighbors, dir + "/l2");
  if (rc == 0) rc = run(l1, pf.size(), radius, rf, min_neighbors, dir + "/l1");
  if (rc == 0) rc = run(l2d, pd.size(), static_cast<double>(radius), rd, min_neighbors, dir + "/l2d");
  if (rc != 0) return rc;
  std::printf("ok\n");
  return 0;
}
