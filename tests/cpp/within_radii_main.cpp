// tests/cpp/within_radii_main.cpp -- TEST PROGRAM for the batched kd_tree::search_knn_within / count_within members that
// take one radius per query (include/pico_tree/kd_tree.hpp).
//
//   within_radii_main <dir> <k>
//
// Built with -DPICO_TREE_HOST_ONLY (no backend linked): the batched members loop over the single-query members.  <dir>
// holds points.bin / queries.bin (float32 row-major, 3-D) and radii.bin (float32, one per query) written by
// tests/test_within_radii.py.  The batched rows and counts must equal the single-query members row by row, float and
// double (L2 squared, L1), with and without max_count; a radii vector of the wrong size must throw.  Exit status 0 and
// "ok" when all of that holds.

#include <array>
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

// 0: the batched members equal the single-query members and refuse a wrong size; otherwise the first check that failed.
template <typename Tree, typename Space>
static int check(Tree const& tree, Space const& qs, std::vector<typename Tree::scalar_type> const& radii, size_t k) {
  using nb = typename Tree::neighbor_type;
  using size_type = typename Tree::size_type;
  std::vector<nb> got(qs.size() * k, nb(7, 7));
  tree.search_knn_within(qs, k, radii, got.data());
  std::vector<nb> row;
  for (size_t i = 0; i < qs.size(); ++i) {
    tree.search_knn_within(qs[i], k, radii[i], row);
    if (row.size() > k) return 1;
    for (size_t j = 0; j < k; ++j) {
      nb const want = j < row.size() ? row[j] : nb(-1, radii[i]);
      nb const have = got[i * k + j];
      if (have.index != want.index || std::memcmp(&have.distance, &want.distance, sizeof(want.distance)) != 0) return 2;
    }
  }
  for (size_type max_count : {size_type(0), size_type(5)}) {
    std::vector<size_type> counts(qs.size(), size_type(77));
    tree.count_within(qs, radii, counts.data(), max_count);
    for (size_t i = 0; i < qs.size(); ++i) {
      size_type want = tree.count_within(qs[i], radii[i]);
      if (max_count != 0 && want > max_count) want = max_count;
      if (counts[i] != want) return 3;
    }
  }
  std::vector<typename Tree::scalar_type> wrong(radii.begin(), radii.end() - 1);
  bool threw = false;
  try {
    tree.search_knn_within(qs, k, wrong, got.data());
  } catch (std::invalid_argument const&) {
    threw = true;
  }
  if (!threw) return 4;
  threw = false;
  std::vector<size_type> counts(qs.size());
  wrong.push_back(radii.back());
  wrong.push_back(radii.back());
  try {
    tree.count_within(qs, wrong, counts.data());
  } catch (std::invalid_argument const&) {
    threw = true;
  }
  return threw ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: within_radii_main <dir> <k>\n");
    return 2;
  }
  std::string const dir = argv[1];
  size_t const k = std::stoul(argv[2]);
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
  int const rc[4] = {check(l2, qf, rf, k), check(l1, qf, rf, k), check(l2d, qd, rd, k), check(l1d, qd, rd, k)};
  for (int i = 0; i < 4; ++i) {
    if (rc[i] != 0) {
      std::fprintf(stderr, "tree %d: check %d failed\n", i, rc[i]);
      return 10 + rc[i];
    }
  }
  std::printf("ok\n");
  return 0;
}
