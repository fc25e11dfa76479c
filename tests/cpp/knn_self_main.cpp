// tests/cpp/knn_self_main.cpp -- TEST PROGRAM for kd_tree::search_knn_self (include/pico_tree/kd_tree.hpp).
//
//   knn_self_main host  <dir> <k>   the per-point member, float (L2 squared, L1, L+inf) and double
//   knn_self_main batch <dir> <k>   the batched member through the C ABI (needs a GPU), float and double, and a
//                                   metric_se2_squared tree (the staged route over the topological search)
//
// <dir> holds points.bin (float32 row-major, 3-D) written by tests/test_knn_self.py.  Every result is written as
// n x k rows padded with {-1, largest scalar}; the driver compares them with the compiled reference.

#include <array>
#include <cstring>
#include <cstdio>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include <pico_tree/array_traits.hpp>
#include <pico_tree/kd_tree.hpp>
#include <pico_tree/vector_traits.hpp>

template <typename T>
static std::vector<std::array<T, 3>> read_points(std::string const& path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error("cannot open " + path);
  std::streamsize bytes = f.tellg();
  f.seekg(0);
  std::vector<float> v(static_cast<size_t>(bytes) / sizeof(float));
  f.read(reinterpret_cast<char*>(v.data()), bytes);
  std::vector<std::array<T, 3>> s(v.size() / 3);
  for (size_t i = 0; i < s.size(); ++i) s[i] = {T(v[3 * i]), T(v[3 * i + 1]), T(v[3 * i + 2])};
  return s;
}

template <typename T>
static void write_raw(std::string const& path, std::vector<T> const& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

// The per-point member, rows padded to k.
template <typename Tree>
static std::vector<typename Tree::neighbor_type> host_rows(Tree const& tree, size_t n, size_t k) {
  using nb = typename Tree::neighbor_type;
  std::vector<nb> out(n * k, nb(-1, std::numeric_limits<typename Tree::scalar_type>::max()));
  std::vector<nb> row;
  for (size_t i = 0; i < n; ++i) {
    tree.search_knn_self(static_cast<int>(i), k, row);
    if (row.size() > k) return {};
    std::copy(row.begin(), row.end(), out.begin() + i * k);
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: knn_self_main host|batch <dir> <k>\n");
    return 2;
  }
  std::string const mode = argv[1], dir = argv[2];
  size_t const k = std::stoul(argv[3]);
  auto pf = read_points<float>(dir + "/points.bin");
  auto pd = read_points<double>(dir + "/points.bin");
  using spacef = std::vector<std::array<float, 3>>;
  using spaced = std::vector<std::array<double, 3>>;
  pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spaced> l2d(pd, pico_tree::max_leaf_size_t(10));
  if (mode == "host") {
    pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
    pico_tree::kd_tree<spacef, pico_tree::metric_lpinf> linf(pf, pico_tree::max_leaf_size_t(10));
    write_raw(dir + "/h_l2.bin", host_rows(l2, pf.size(), k));
    write_raw(dir + "/h_l1.bin", host_rows(l1, pf.size(), k));
    write_raw(dir + "/h_linf.bin", host_rows(linf, pf.size(), k));
    write_raw(dir + "/h_l2d.bin", host_rows(l2d, pd.size(), k));
    std::printf("host ok\n");
    return 0;
  }
#ifndef PTK_TEST_HOST_ONLY
  if (mode == "batch") {
    std::vector<pico_tree::neighbor<int, float>> out;
    l2.search_knn_self(k, out);
    if (out.size() != pf.size() * k) return 3;
    write_raw(dir + "/b_l2.bin", out);
    std::vector<pico_tree::neighbor<int, double>> outd;
    l2d.search_knn_self(k, outd);
    if (outd.size() != pd.size() * k) return 3;
    write_raw(dir + "/b_l2d.bin", outd);
    // metric_se2_squared: the staged route over the topological search; the per-point member gives the same rows
    pico_tree::kd_tree<spacef, pico_tree::metric_se2_squared> se2(pf, pico_tree::max_leaf_size_t(10));
    se2.search_knn_self(k, out);
    auto const want = host_rows(se2, pf.size(), k);
    if (want.size() != out.size() || std::memcmp(want.data(), out.data(), out.size() * sizeof(out[0])) != 0) return 4;
    bool threw = false;
    try {
      l2.search_knn_self(0, out);
    } catch (std::invalid_argument const&) {
      threw = true;
    }
    if (!threw) return 5;
    std::printf("batch ok\n");
    return 0;
  }
#endif
  return 2;
}
