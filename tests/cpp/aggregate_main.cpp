// tests/cpp/aggregate_main.cpp -- TEST PROGRAM for kd_tree::aggregate_within_self / kd_tree::aggregate_within
// (include/pico_tree/kd_tree.hpp).  Built with -DPICO_TREE_HOST_ONLY (no backend linked: the members loop over the
// per-point members with the fold of pico_tree/internal/aggregate.hpp; this build also runs under
// -fsanitize=address,undefined) and, for the gpu tier, against libptk.so (the members go through the backend).
//
//   aggregate_main <dir> <radius> <channels> <leaf size> <l2|l1|lpinf|lninf>
//
// <dir> holds points.bin and queries.bin (float32 row-major, 3-D), radii.bin (one per point), qradii.bin (one per query)
// and values.bin (points x channels) written by tests/test_aggregate_within.py.  For each op in sum, min, max it writes
//   self_scalar_<op>.out / .cnt    scalar radius, without the own value
//   self_radii_<op>.out / .cnt     per-point radii, include_self
//   within_scalar_<op>.out / .cnt  the query batch, scalar radius
//   within_radii_<op>.out / .cnt   the query batch, per-row radii
// (.out float32 rows x channels, .cnt uint64 per row); the driver compares them byte for byte with the fold.

#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
static void write_all(std::string const& path, std::vector<T> const& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<char const*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

static void write_pair(std::string const& stem, std::vector<float> const& out, std::vector<size_t> const& counts) {
  write_all(stem + ".out", out);
  write_all(stem + ".cnt", std::vector<std::uint64_t>(counts.begin(), counts.end()));
}

using space = std::vector<std::array<float, 3>>;

static space as_space(std::vector<float> const& raw) {
  space pts(raw.size() / 3);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = {raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]};
  return pts;
}

template <typename Metric>
static int run(space const& pts, space const& queries, size_t leaf, float radius, std::vector<float> const& radii,
               std::vector<float> const& qradii, std::vector<float> const& values, size_t channels, std::string const& dir) {
  pico_tree::kd_tree<space, Metric> tree(pts, pico_tree::max_leaf_size_t(leaf));
  char const* names[3] = {"sum", "min", "max"};
  pico_tree::aggregate_op const ops[3] = {pico_tree::aggregate_op::sum, pico_tree::aggregate_op::min, pico_tree::aggregate_op::max};
  for (int o = 0; o < 3; ++o) {
    std::vector<float> out, only;
    std::vector<size_t> counts;
    tree.aggregate_within_self(radius, values.data(), channels, ops[o], false, out, &counts);
    if (out.size() != pts.size() * channels || counts.size() != pts.size()) return 3;
    write_pair(dir + "/self_scalar_" + names[o], out, counts);
    // (without the counts: the same values)
    tree.aggregate_within_self(radius, values.data(), channels, ops[o], false, only);
    if (only.size() != out.size() || std::memcmp(only.data(), out.data(), out.size() * sizeof(float)) != 0) return 4;
    tree.aggregate_within_self(radii, values.data(), channels, ops[o], true, out, &counts);
    write_pair(dir + "/self_radii_" + names[o], out, counts);
    tree.aggregate_within(queries, radius, values.data(), channels, ops[o], out, &counts);
    if (out.size() != queries.size() * channels || counts.size() != queries.size()) return 5;
    write_pair(dir + "/within_scalar_" + names[o], out, counts);
    tree.aggregate_within(queries, qradii, values.data(), channels, ops[o], out, &counts);
    write_pair(dir + "/within_radii_" + names[o], out, counts);
  }
  int threw = 0;
  std::vector<float> out;
  try {
    std::vector<float> few(radii.begin(), radii.begin() + 5);
    tree.aggregate_within_self(few, values.data(), channels, pico_tree::aggregate_op::sum, false, out);
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  try {
    tree.aggregate_within_self(radius, values.data(), 0, pico_tree::aggregate_op::sum, false, out);
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  try {
    tree.aggregate_within(queries, radius, nullptr, channels, pico_tree::aggregate_op::sum, out);
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  return threw == 3 ? 0 : 6;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: aggregate_main <dir> <radius> <channels> <leaf> <metric>\n");
    return 2;
  }
  std::string const dir = argv[1];
  float const radius = std::stof(argv[2]);
  size_t const channels = std::stoul(argv[3]);
  size_t const leaf = std::stoul(argv[4]);
  std::string const metric = argv[5];
  space const pts = as_space(read_floats(dir + "/points.bin"));
  space const queries = as_space(read_floats(dir + "/queries.bin"));
  auto const radii = read_floats(dir + "/radii.bin");
  auto const qradii = read_floats(dir + "/qradii.bin");
  auto const values = read_floats(dir + "/values.bin");
  if (values.size() != pts.size() * channels || radii.size() != pts.size() || qradii.size() != queries.size()) return 2;
  int rc = 2;
  if (metric == "l2") rc = run<pico_tree::metric_l2_squared>(pts, queries, leaf, radius, radii, qradii, values, channels, dir);
  else if (metric == "l1") rc = run<pico_tree::metric_l1>(pts, queries, leaf, radius, radii, qradii, values, channels, dir);
  else if (metric == "lpinf") rc = run<pico_tree::metric_lpinf>(pts, queries, leaf, radius, radii, qradii, values, channels, dir);
  else if (metric == "lninf") rc = run<pico_tree::metric_lninf>(pts, queries, leaf, radius, radii, qradii, values, channels, dir);
  if (rc != 0) return rc;
  std::printf("ok\n");
  return 0;
}
