// tests/cpp/radius_radii_main.cpp -- TEST PROGRAM for the batched kd_tree::search_radius members that take one radius per
// query (include/pico_tree/kd_tree.hpp).
//
//   radius_radii_main <dir>
//
// Built with -DPICO_TREE_HOST_ONLY (no backend linked): the batched members loop over the single-query member.  <dir>
// holds points.bin / queries.bin (float32 row-major, 3-D) and radii.bin (float32, one per query) written by
// tests/test_radius_radii.py.  Both forms (a vector of rows; offsets + flat), sorted and unsorted, must equal the
// single-query search_radius(x, radii[i], row, sort) row by row, float and double (L2 squared, L1); a radii vector of the
// wrong size must throw; and the scalar overloads must still be callable beside the new ones.  Exit status 0 and "ok"
// when all of that holds.

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
static std::vector<std::array<T, 3>> as_points(std::vector<float> const& v) {
  std::vector<std::array<T, 3>> s(v.size() / 3);
  for (size_t i = 0; i < s.size(); ++i) s[i] = {T(v[3 * i]), T(v[3 * i + 1]), T(v[3 * i + 2])};
  return s;
}

template <typename Nb>
static bool same(Nb const& a, Nb const& b) {
  return a.index == b.index && std::memcmp(&a.distance, &b.distance, sizeof(a.distance)) == 0;
}

// 0: the batched members equal the single-query member and refuse a wrong size; otherwise the first check that failed.
template <typename Tree, typename Space>
static int check(Tree const& tree, Space const& qs, std::vector<typename Tree::scalar_type> const& radii) {
  using nb = typename Tree::neighbor_type;
  for (bool sort : {false, true}) {
    std::vector<std::vector<nb>> rows(3, std::vector<nb>(2, nb(7, 7)));  // (stale contents must not survive)
    tree.search_radius(qs, radii, rows, sort);
    std::vector<std::uint64_t> offsets(5, 9);
    std::vector<nb> flat(11, nb(7, 7));
    tree.search_radius(qs, radii, offsets, flat, sort);
    if (rows.size() != qs.size() || offsets.size() != qs.size() + 1 || offsets[0] != 0) return 1;
    std::vector<nb> row;
    for (size_t i = 0; i < qs.size(); ++i) {
      tree.search_radius(qs[i], radii[i], row, sort);
      if (rows[i].size() != row.size() || offsets[i + 1] - offsets[i] != row.size()) return 2;
      for (size_t j = 0; j < row.size(); ++j) {
        if (!same(rows[i][j], row[j])) return 3;
        if (!same(flat[offsets[i] + j], row[j])) return 4;
      }
    }
    if (flat.size() != offsets.back()) return 5;
  }
  std::vector<typename Tree::scalar_type> wrong(radii.begin(), radii.end() - 1);
  std::vector<std::vector<nb>> rows;
  std::vector<std::uint64_t> offsets;
  std::vector<nb> flat;
  bool threw = false;
  try {
    tree.search_radius(qs, wrong, rows);
  } catch (std::invalid_argument const&) {
    threw = true;
  }
  if (!threw) return 6;
  threw = false;
  wrong.push_back(radii.back());
  wrong.push_back(radii.back());
  try {
    tree.search_radius(qs, wrong, offsets, flat);
  } catch (std::invalid_argument const&) {
    threw = true;
  }
  if (!threw) return 7;
  // the scalar overloads beside the new ones: a literal, a variable and a sort flag still pick them
  typename Tree::scalar_type const one = radii[1];
  std::vector<nb> a, b;
  tree.search_radius(qs[0], one, a);
  tree.search_radius(qs[0], one, b, true);
  tree.search_radius(qs[0], one, typename Tree::scalar_type(1), b, true);
  return a.size() == b.size() ? 0 : 8;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: radius_radii_main <dir>\n");
    return 2;
  }
  std::string const dir = argv[1];
  auto const p = read_floats(dir + "/points.bin"), q = read_floats(dir + "/queries.bin");
  auto const rf = read_floats(dir + "/radii.bin");
  std::vector<double> const rd(rf.begin(), rf.end());
  auto const pf = as_points<float>(p), qf = as_points<float>(q);
  auto const pd = as_points<double>(p), qd = as_points<double>(q);
  using spacef = std::vector<std::array<float, 3>>;
  using spaced = std::vector<std::array<double, 3>>;
  pico_tree::kd_tree<spacef> l2(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spacef, pico_tree::metric_l1> l1(pf, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spaced> l2d(pd, pico_tree::max_leaf_size_t(10));
  pico_tree::kd_tree<spaced, pico_tree::metric_l1> l1d(pd, pico_tree::max_leaf_size_t(10));
  int const rc[4] = {check(l2, qf, rf), check(l1, qf, rf), check(l2d, qd, rd), check(l1d, qd, rd)};
  for (int i = 0; i < 4; ++i) {
    if (rc[i] != 0) {
      std::fprintf(stderr, "tree %d: check %d failed\n", i, rc[i]);
      return 10 + rc[i];
    }
  }
  std::printf("ok\n");
  return 0;
}
