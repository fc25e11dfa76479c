// tests/cpp/radius_self_main.cpp -- TEST PROGRAM for kd_tree::search_radius_self / count_within_self
// (include/pico_tree/kd_tree.hpp).
//
//   radius_self_main host  <dir> <radius>   the per-point member, float (L2 squared, L1, L+inf) and double
//   radius_self_main batch <dir> <radius>   the batched members through the C ABI (needs a GPU), float and double: the
//                                           rows and counts at <radius> and at the per-point radii of radii.bin, and a
//                                           metric_se2_squared tree (refused by the device, served by the host loop)
//
// <dir> holds points.bin (float32 row-major, 3-D) and radii.bin (float32, one per point) written by
// tests/test_radius_self.py.  Rows are written as <name>.off (uint64, n + 1) and <name>.bin (the records), counts as
// <name>.cnt (uint64, n); the driver compares them with the compiled reference.

#include <array>
#include <cstdint>
#include <cstdio>
#include <fstream>
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

template <typename T>
static void write_raw(std::string const& path, std::vector<T> const& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

template <typename Nb>
static void write_rows(std::string const& name, std::vector<std::vector<Nb>> const& rows) {
  std::vector<std::uint64_t> off(rows.size() + 1, 0);
  std::vector<Nb> flat;
  for (size_t i = 0; i < rows.size(); ++i) {
    off[i + 1] = off[i] + rows[i].size();
    flat.insert(flat.end(), rows[i].begin(), rows[i].end());
  }
  write_raw(name + ".off", off);
  write_raw(name + ".bin", flat);
}

// The per-point member over every point.
template <typename Tree>
static std::vector<std::vector<typename Tree::neighbor_type>> host_rows(
    Tree const& tree, size_t n, typename Tree::scalar_type radius) {
  std::vector<std::vector<typename Tree::neighbor_type>> rows(n);
  for (size_t i = 0; i < n; ++i) tree.search_radius_self(static_cast<int>(i), radius, rows[i]);
  return rows;
}

template <typename Tree, typename Scalar>
static int batch(Tree const& tree, size_t n, Scalar radius, std::vector<Scalar> const& radii, std::string const& name) {
  using nb = typename Tree::neighbor_type;
  std::vector<std::vector<nb>> rows;
  tree.search_radius_self(radius, rows);
  if (rows.size() != n) return 3;
  write_rows(name + "_scalar", rows);
  tree.search_radius_self(radii, rows, /*sort=*/false);
  if (rows.size() != n) return 3;
  write_rows(name + "_radii", rows);
  std::vector<std::size_t> counts(n);
  tree.count_within_self(radius, counts.data());
  write_raw(name + "_scalar.cnt", std::vector<std::uint64_t>(counts.begin(), counts.end()));
  tree.count_within_self(radii, counts.data(), 7);
  write_raw(name + "_radii7.cnt", std::vector<std::uint64_t>(counts.begin(), counts.end()));
  bool threw = false;
  try {
    std::vector<Scalar> few(radii.begin(), radii.begin() + 5);
    tree.count_within_self(few, counts.data());
  } catch (std::invalid_argument const&) {
    threw = true;
  }
  return threw ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: radius_self_main host|batch <dir> <radius>\n");
    return 2;
  }
  std::string const mode = argv[1], dir = argv[2];
  float const radius = std::stof(argv[3]);
  auto const raw = read_floats(dir + "/points.bin");
  auto pf = as_points<float>(raw);
  auto pd = as_points<double>(raw);
  using spacef = std::vector<std::array<float, 3>>;
  using spaced = std::vector<std::array<double, 3>>;
  pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spaced> l2d(pd, pico_tree::max_leaf_size_t(10));
  if (mode == "host") {
    pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
    pico_tree::kd_tree<spacef, pico_tree::metric_lpinf> linf(pf, pico_tree::max_leaf_size_t(10));
    write_rows(dir + "/h_l2", host_rows(l2, pf.size(), radius));
    write_rows(dir + "/h_l1", host_rows(l1, pf.size(), radius));
    write_rows(dir + "/h_linf", host_rows(linf, pf.size(), radius));
    write_rows(dir + "/h_l2d", host_rows(l2d, pd.size(), static_cast<double>(radius)));
    bool threw = false;
    try {
      std::vector<pico_tree::neighbor<int, float>> row;
      l2.search_radius_self(static_cast<int>(pf.size()), radius, row);
    } catch (std::out_of_range const&) {
      threw = true;
    }
    if (!threw) return 5;
    std::printf("host ok\n");
    return 0;
  }
#ifndef PTK_TEST_HOST_ONLY
  if (mode == "batch") {
    auto const rf = read_floats(dir + "/radii.bin");
    std::vector<double> const rd(rf.begin(), rf.end());
    int rc = batch(l2, pf.size(), radius, rf, dir + "/b_l2");
    if (rc != 0) return rc;
    rc = batch(l2d, pd.size(), static_cast<double>(radius), rd, dir + "/b_l2d");
    if (rc != 0) return rc;
    // metric_se2_squared: the device refuses it; under allow_host_loop the loop over the per-point member serves it
    pico_tree::kd_tree<spacef, pico_tree::metric_se2_squared> se2(pf, pico_tree::max_leaf_size_t(10));
    std::vector<std::vector<pico_tree::neighbor<int, float>>> rows;
    bool refused = false;
    try {
      se2.search_radius_self(radius, rows);
    } catch (std::exception const&) {
      refused = true;
    }
    if (!refused) return 6;
    pico_tree::allow_host_loop(true);
    se2.search_radius_self(radius, rows);
    pico_tree::allow_host_loop(false);
    auto const want = host_rows(se2, pf.size(), radius);
    if (rows.size() != want.size()) return 4;
    for (size_t i = 0; i < rows.size(); ++i) {
      if (rows[i].size() != want[i].size()) return 4;
      for (size_t j = 0; j < rows[i].size(); ++j)
        if (rows[i][j].index != want[i][j].index || rows[i][j].distance != want[i][j].distance) return 4;
    }
    std::printf("batch ok\n");
    return 0;
  }
#endif
  return 2;
}
