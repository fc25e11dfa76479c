// tests/cpp/mst_self_main.cpp -- TEST PROGRAM for kd_tree::mst_within_self (include/pico_tree/kd_tree.hpp).
// Built with -DPICO_TREE_HOST_ONLY (no backend linked): the member runs the per-point member plus Kruskal of
// pico_tree/internal/mst.hpp.  Built without it and linked to libptk.so: the batched member on the device.
//
//   mst_self_main <dir> <radius>
//
// <dir> holds points.bin (float32 row-major, 3-D) and core.bin (float32, one per point) written by
// tests/test_mst_self.py.  Writes <name>.edges (12-byte records) and <name>.labels (int32, n) for a float tree under L2
// squared without and with the core distances (l2_plain, l2_core) and under L1 (l1_plain); the driver compares them with
// its expected arrays.

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
static void write_all(std::string const& path, T const* v, size_t n) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v), static_cast<std::streamsize>(n * sizeof(T)));
}

template <typename Tree>
static int run(Tree const& tree, size_t n, float radius, float const* core, std::string const& name) {
  using pico_tree::internal::mst_edge;
  std::vector<mst_edge> edges(n - 1);
  std::vector<std::int32_t> labels(n, -7);
  size_t const count = tree.mst_within_self(radius, edges.data(), core, labels.data());
  if (count > n - 1) return 4;
  write_all(name + ".edges", edges.data(), count);
  write_all(name + ".labels", labels.data(), n);
  // (radius 0: no edges, every point its own component; labels may be left out)
  if (tree.mst_within_self(0.0f, edges.data()) != 0) return 5;
  int threw = 0;
  try {
    std::vector<float> bad(n, 0.0f);
    bad[n / 2] = std::numeric_limits<float>::quiet_NaN();
    tree.mst_within_self(radius, edges.data(), bad.data());
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  try {
    tree.mst_within_self(-1.0f, edges.data());
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  return threw == 2 ? 0 : 6;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: mst_self_main <dir> <radius>\n");
    return 2;
  }
  std::string const dir = argv[1];
  float const radius = std::stof(argv[2]);
  auto const raw = read_floats(dir + "/points.bin");
  auto const core = read_floats(dir + "/core.bin");
  std::vector<std::array<float, 3>> pf(raw.size() / 3);
  for (size_t i = 0; i < pf.size(); ++i) pf[i] = {raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]};
  using spacef = std::vector<std::array<float, 3>>;
  try {
    pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
    pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
    int rc = run(l2, pf.size(), radius, nullptr, dir + "/l2_plain");
    if (rc == 0) rc = run(l2, pf.size(), radius, core.data(), dir + "/l2_core");
    if (rc == 0) rc = run(l1, pf.size(), radius, nullptr, dir + "/l1_plain");
    if (rc != 0) return rc;
  } catch (std::exception const& ex) {
    std::fprintf(stderr, "mst_self_main: %s\n", ex.what());
    return 3;
  }
  std::printf("ok\n");
  return 0;
}
