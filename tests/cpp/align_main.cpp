// tests/cpp/align_main.cpp -- TEST PROGRAM for kd_tree::align_step (include/pico_tree/kd_tree.hpp).  Built with
// -DPICO_TREE_HOST_ONLY (no backend linked: the member loops over the per-point member with the routines of
// pico_tree/internal/align.hpp; this build also runs under -fsanitize=address,undefined) and, for the gpu tier, against
// libptk.so (the member goes through the backend).
//
//   align_main <dir> <max_distance> <leaf size>
//
// <dir> holds points.bin, queries.bin and normals.bin (float32 row-major, 3-D; normals one row per point) and
// transform.bin (12 floats) written by tests/test_align_step.py.  It writes
//   point.sums / point.rows          point-to-point with the transform, and the unfiltered rows
//   plane.sums                       point-to-plane with the transform
//   point_identity.sums              point-to-point without a transform
// (.sums the 384-byte record, .rows 8 bytes per query); the driver compares them byte for byte with the host loop.

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

static void write_bytes(std::string const& path, void const* p, size_t bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(static_cast<char const*>(p), static_cast<std::streamsize>(bytes));
}

using space = std::vector<std::array<float, 3>>;

static space as_space(std::vector<float> const& raw) {
  space pts(raw.size() / 3);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = {raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]};
  return pts;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: align_main <dir> <max_distance> <leaf>\n");
    return 2;
  }
  std::string const dir = argv[1];
  float const max_distance = std::stof(argv[2]);
  size_t const leaf = std::stoul(argv[3]);
  space const pts = as_space(read_floats(dir + "/points.bin"));
  space const queries = as_space(read_floats(dir + "/queries.bin"));
  auto const normals = read_floats(dir + "/normals.bin");
  auto const transform = read_floats(dir + "/transform.bin");
  if (normals.size() != pts.size() * 3 || transform.size() != 12) return 2;
  pico_tree::kd_tree<space> tree(pts, pico_tree::max_leaf_size_t(leaf));
  std::vector<pico_tree::neighbor<int, float>> rows;
  pico_tree::align_sums s = tree.align_step(queries, transform.data(), max_distance, nullptr, &rows);
  if (rows.size() != queries.size() || s.rows != queries.size()) return 3;
  write_bytes(dir + "/point.sums", &s, sizeof s);
  write_bytes(dir + "/point.rows", rows.data(), rows.size() * sizeof rows[0]);
  s = tree.align_step(queries, transform.data(), max_distance, normals.data());
  write_bytes(dir + "/plane.sums", &s, sizeof s);
  s = tree.align_step(queries, nullptr, max_distance);
  write_bytes(dir + "/point_identity.sums", &s, sizeof s);
  int threw = 0;
  try {
    tree.align_step(queries, nullptr, -1.0f);
  } catch (std::invalid_argument const&) {
    ++threw;
  }
  if (threw != 1) return 6;
  std::printf("ok\n");
  return 0;
}
