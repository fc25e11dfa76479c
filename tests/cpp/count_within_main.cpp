// tests/cpp/count_within_main.cpp -- TEST PROGRAM for kd_tree::count_within (include/pico_tree/kd_tree.hpp).
//
//   count_within_main host   <dir> <radius>   the single-query member, float (L2 squared, L1, L+inf) and double
//   count_within_main device <dir> <radius>   the batched member through the C ABI (needs a GPU), the same trees,
//                                             without a limit and with max_count = 16 (<name>_16.bin)
//
// <dir> holds points.bin / queries.bin (float32 row-major, 3-D) written by tests/test_count_within.py.  Every result
// is written as nq uint64 counts; the driver compares them with the compiled reference.

#include <array>
#include <cstdint>
#include <cstdio>
#include <fstream>
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

static void write_raw(std::string const& path, std::vector<std::uint64_t> const& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(v[0])));
}

template <typename Tree, typename Space>
static std::vector<std::uint64_t> host_counts(Tree const& tree, Space const& qs, typename Tree::scalar_type radius) {
  std::vector<std::uint64_t> out(qs.size());
  for (size_t i = 0; i < qs.size(); ++i) out[i] = tree.count_within(qs[i], radius);
  return out;
}

#ifndef PTK_TEST_HOST_ONLY
template <typename Tree, typename Space>
static void device_counts(Tree const& tree, Space const& qs, typename Tree::scalar_type radius, std::string const& path) {
  std::vector<typename Tree::size_type> c(qs.size());
  tree.count_within(qs, radius, c.data());
  write_raw(path + ".bin", std::vector<std::uint64_t>(c.begin(), c.end()));
  tree.count_within(qs, radius, c.data(), 16);
  write_raw(path + "_16.bin", std::vector<std::uint64_t>(c.begin(), c.end()));
}
#endif

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: count_within_main host|device <dir> <radius>\n");
    return 2;
  }
  std::string const mode = argv[1], dir = argv[2];
  float const radius = std::stof(argv[3]);
  auto pf = read_points<float>(dir + "/points.bin");
  auto qf = read_points<float>(dir + "/queries.bin");
  auto pd = read_points<double>(dir + "/points.bin");
  auto qd = read_points<double>(dir + "/queries.bin");
  using spacef = std::vector<std::array<float, 3>>;
  using spaced = std::vector<std::array<double, 3>>;
  pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spacef, pico_tree::metric_lpinf> linf(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spaced> l2d(pd, pico_tree::max_leaf_size_t(10));
  if (mode == "host") {
    write_raw(dir + "/l2.bin", host_counts(l2, qf, radius));
    write_raw(dir + "/l1.bin", host_counts(l1, qf, radius));
    write_raw(dir + "/linf.bin", host_counts(linf, qf, radius));
    write_raw(dir + "/l2d.bin", host_counts(l2d, qd, double(radius)));
    std::printf("host ok\n");
    return 0;
  }
#ifndef PTK_TEST_HOST_ONLY
  if (mode == "device") {
    device_counts(l2, qf, radius, dir + "/l2");
    device_counts(l1, qf, radius, dir + "/l1");
    device_counts(linf, qf, radius, dir + "/linf");
    device_counts(l2d, qd, double(radius), dir + "/l2d");
    std::printf("device ok\n");
    return 0;
  }
#endif
  return 2;
}
