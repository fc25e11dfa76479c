// ptk_families.hpp -- the entry points of the kernel-family translation units (see ptk_backend_core.hpp).  Each one
// binds the handle's metric and stack class to the template arguments of its launch wrappers; the callers in
// ptk_backend.hip pass plain arguments.
#pragma once

#include "ptk_backend_core.hpp"

namespace ptk {
struct DevTree64;
struct CountBox64;
struct Rec64;
}  // namespace ptk

namespace ptkf {
// What a bounded launch takes its radius from: the scalar entry points' {seed, radius}, or the per-row entry points'
// device array of radii (`unseeded`: the lanes start their lists at FLT_MAX / DBL_MAX whatever the row's radius is).  The
// launch wrappers are written once over either, so the dispatch of the two forms cannot drift apart.
template <class Real>
struct WithinOne {
  Real seed, radius;
};
template <class Real>
struct WithinRows {
  const Real* radii;
  uint32_t unseeded;
};
// Does a bounded k-list of this metric start unseeded whatever the radius is?  metric_lpinf / metric_lninf: their box
// distance is no lower bound of the point distances.  The one statement of it, for the scalar seed
// (within_seed, ptk_backend.hip; ptk_search64_knn_within_device) and for the per-row launches alike.
inline bool unseeded_metric(int metric) { return metric == PTK_METRIC_LPINF || metric == PTK_METRIC_LNINF; }
template <class R>
struct within_rows : std::false_type {};
template <class Real>
struct within_rows<WithinRows<Real>> : std::true_type {};
// ptk_backend.hip: the batch order (the library's radix sort of 32-bit keys; rocprim is compiled into that unit only)
int morton_bits(uint64_t nq);
size_t sort_tmp_bytes(uint64_t nq, int bits);
size_t permutation_scratch_bytes(uint64_t nq);
int sort_pairs_u32(void* tmp, size_t tmp_bytes, uint32_t* keys, uint32_t* keys_out, uint32_t* ids, uint32_t* ids_out,
                   uint64_t nq, int bits, hipStream_t s);
// ptk_family_knn.hip: 3-D float32 trees, k > 1 (and k = 1 of the other metrics)
int knn_reg(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
            ptk::Neighbor* d_out, hipStream_t s, ptkb::Scratch* scratch);
int knn_rows(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
             ptk::Neighbor* d_out, hipStream_t s);
int knn_deep(const ptk_tree* t, const ptk::DevTree& dev, const float* d_q, uint64_t n, uint32_t k, float e,
             ptk::Neighbor* d_out, hipStream_t s);
// search_knn_within: `seed` is the pruning bound the list starts at (FLT_MAX: unseeded), `radius` the
// bound of the stored entries; the deep forms run unseeded
int knn_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float seed, float radius,
               ptk::Neighbor* d_out, hipStream_t s);
int knn_within_deep(const ptk_tree* t, const ptk::DevTree& dev, const float* d_q, uint64_t n, uint32_t k, float radius,
                    ptk::Neighbor* d_out, hipStream_t s);
// search_knn_within_radii (ptk.h): row i bounded by d_radii[i], i the row in the caller's order
int knn_within_radii(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, const float* d_radii,
                     ptk::Neighbor* d_out, hipStream_t s);
int knn_within_radii_deep(const ptk_tree* t, const ptk::DevTree& dev, const float* d_q, uint64_t n, uint32_t k,
                          const float* d_radii, ptk::Neighbor* d_out, hipStream_t s);
void warm_knn();
// ptk_family_radius.hip: 3-D float32 trees
int radius_traverse(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e, bool fill,
                    uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s,
                    const uint32_t* n_dev = nullptr);
int radius_capture(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e,
                   uint64_t* d_counts, const ptk::RadiusCapture& cap, hipStream_t s);
// (far_cap != 0: the capped list pass + the cooperative count of what it hands over; `heavy` is where the batch keeps
// that for the fill pass, `scratch` has radius_coop_scratch_bytes() left)
int radius_list(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e,
                uint64_t* d_counts, const ptk::RadiusCapture& cap, hipStream_t s, uint32_t far_cap = 0,
                ptkb::Scratch* scratch = nullptr, const ptk::RadiusHeavy* heavy = nullptr);
int radius_replay(const ptk_tree* t, const float* d_q, float e, const ptk::RadiusCapture& cap, const uint64_t* d_offsets,
                  ptk::Neighbor* d_out, uint32_t* over_list, uint32_t* n_over, hipStream_t s,
                  const ptk::RadiusHeavy* heavy = nullptr);
int radius_log_scatter(const ptk_tree* t, const ptk::RadiusCapture& cap, const uint64_t* d_offsets, ptk::Neighbor* d_out,
                       uint32_t* over_list, uint32_t* n_over, hipStream_t s);
int radius_deep(const ptk_tree* t, const ptk::DevTree& dev, const float* d_q, uint64_t n, float radius, float e, bool fill,
                uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s);
void warm_radius();
// ptk_family_nd.hip: dim > 3
int knn_nd(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
           ptk::Neighbor* d_out, hipStream_t s, bool no_register_list);
int knn_nd_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k, float e,
                ptk::Neighbor* d_out, hipStream_t s);
int radius_nd(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, float e, bool fill, uint64_t* d_counts,
              const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s, const uint32_t* perm = nullptr,
              const uint32_t* n_dev = nullptr);
int radius_nd_capture(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e,
                      uint64_t* d_counts, const ptk::RadiusCapture& cap, hipStream_t s);
int radius_nd_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, float radius, float e,
                   bool fill, uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s);
int knn_nd_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float seed,
                  float radius, ptk::Neighbor* d_out, hipStream_t s);
int knn_nd_within_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k, float radius,
                       ptk::Neighbor* d_out, hipStream_t s);
int knn_nd_within_radii(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k,
                        const float* d_radii, ptk::Neighbor* d_out, hipStream_t s);
int knn_nd_within_radii_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k,
                             const float* d_radii, ptk::Neighbor* d_out, hipStream_t s);
void warm_nd();
// ptk_family_topo.hip: metric_so2 / metric_se2_squared
int knn_topo(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, uint32_t k, float e,
             ptk::Neighbor* d_out, hipStream_t s, bool no_register_list);
int radius_topo(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, float e, bool fill,
                uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s);
void warm_topo();
// ptk_family_count.hip: count_within of 3-D float32 trees (ptk_kernels_count.hpp); the side table holds kCountBoxBytes per branch
constexpr size_t kCountBoxBytes = 32;
int count_table(const ptk_tree* t, void** d_table, hipStream_t s);
int count_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius, uint64_t max_count,
                 bool shortcut, uint64_t* d_counts, hipStream_t s);
int count_within_radii(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, const float* d_radii,
                        uint64_t max_count, bool shortcut, uint64_t* d_counts, hipStream_t s);
// search_radius_radii (ptk.h): the rows behind count_within_radii(max_count = 0) and a scan of its counts
int radius_radii_fill(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, const float* d_radii,
                      const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s);
// aggregate_within (ptk_kernels_aggregate.hpp): out[qi][0 .. channels) and counts[qi] (may be null) of
// the rows of radius_radii_fill at e = 1; d_radii null: every row gets `radius`.  `flags`: a PTK_AGG_* op.  One launch
// per channel window.
int aggregate_within(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float radius,
                     const float* d_radii, const float* d_values, uint32_t channels, uint32_t flags, float* d_out,
                     uint64_t* d_counts, hipStream_t s);
int clamp_counts(uint64_t* d_counts, uint64_t n, uint64_t max_count, hipStream_t s);
// ... and of float64 trees with dim <= 3 (ptk_kernels_count64.hpp): kCountBox64Bytes per branch
constexpr size_t kCountBox64Bytes = 64;
int count_table64(const ptk::DevTree64& dev, uint64_t n_branches, void** d_table, hipStream_t s);
int count64_within(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, const double* d_q,
                   const uint32_t* perm, uint64_t q0, uint64_t n, double radius, uint64_t max_count, bool shortcut,
                   uint64_t* d_counts, ptk::Rec64* stack, uint32_t slots, hipStream_t s);
int count64_within_radii(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, const double* d_q,
                         const uint32_t* perm, uint64_t q0, uint64_t n, const double* d_radii, uint64_t max_count,
                         bool shortcut, uint64_t* d_counts, ptk::Rec64* stack, uint32_t slots, hipStream_t s);
void warm_count();
// ptk_family_f64.hip
void warm_f64();
// ptk_family_self.hip: search_knn_self.  knn_self: the direct kernel on leaf positions [first, first + n)
// of a float32 tree with dim <= 3, a non-topological metric, a private stack class and k + 1 <= 64 (self_direct below).
// The staged route's two kernels take plain pointers, so that either precision's entry points can call them:
// self_queries* writes the positions' points as dim-wide rows (`recs`: the 16-byte records, else `pts` with `stride`
// scalars per point), drop_self* applies the rule to rows of k + 1 records and writes row `self` of the output.
int knn_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, ptk::Neighbor* d_out, hipStream_t s);
int self_queries(const float4* recs, const float* pts, uint32_t stride, uint32_t dim, uint64_t first, uint64_t n, float* d_q,
                 hipStream_t s);
int self_queries64(const double* pts, uint32_t stride, uint32_t dim, uint64_t first, uint64_t n, double* d_q, hipStream_t s);
int drop_self(const ptk::Neighbor* rows, const float4* recs, const int32_t* index, uint64_t first, uint64_t n, uint32_t k,
              ptk::Neighbor* d_out, hipStream_t s);
int drop_self64(const void* rows, const int32_t* index, uint64_t first, uint64_t n, uint32_t k, void* d_out, hipStream_t s);
// search_radius_self / count_within_self (ptk_kernels_selfr.hpp): leaf positions [first, first + n) of a handle
// ptk_search_count_within_radii serves (check_radius_self); d_radii null: every point gets `radius`, else radii by original
// point index.  The float32 forms read the handle's count side table (built before: count_table_of).
int count_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, uint64_t max_count,
               bool shortcut, uint64_t* d_counts, hipStream_t s);
int radius_self_fill(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii,
                     const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s);
int count64_self(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, uint64_t first, uint64_t n,
                 double radius, const double* d_radii, uint64_t max_count, bool shortcut, uint64_t* d_counts,
                 ptk::Rec64* stack, uint32_t slots, hipStream_t s);
int radius64_self_fill(const ptk::DevTree64& dev, int metric, uint64_t first, uint64_t n, double radius, const double* d_radii,
                       const uint64_t* d_offsets, void* d_out, ptk::Rec64* stack, uint32_t slots, hipStream_t s);
// cluster_within_self (ptk_kernels_cluster.hpp): one pass over d_labels (n_points int32 entries by
// original index, the only working array).  The traversal passes take leaf positions [first, first + n) of a handle
// check_radius_self serves, the elementwise ones all n entries; the caller runs every pass over all pieces before the
// next one, on one stream.  `compress`: find halves its paths.
constexpr bool kClusterCompress = true;  // (DESIGN.md §8 has the measurement behind the value; test hook cluster_compress)
enum ClusterPass { kClusterInit, kClusterMark, kClusterLink, kClusterFlatten, kClusterBorder, kClusterDecode };
int cluster_self(const ptk_tree* t, int pass, uint64_t first, uint64_t n, float radius, const float* d_radii,
                 uint64_t min_neighbors, bool shortcut, bool compress, int32_t* d_labels, hipStream_t s);
int cluster64_self(const ptk::DevTree64& dev, int metric, const ptk::CountBox64* table, int pass, uint64_t first, uint64_t n,
                   double radius, const double* d_radii, uint64_t min_neighbors, bool shortcut, bool compress,
                   int32_t* d_labels, ptk::Rec64* stack, uint32_t slots, hipStream_t s);
int cluster_elementwise(int pass, uint64_t n, bool compress, int32_t* d_labels, hipStream_t s);
// normals_within_self (ptk_kernels_frames.hpp): the frames and / or moments (either may be null) of
// leaf positions [first, first + n) of a float32 handle with dim == 3 that check_radius_self serves; `view` null: no
// viewpoint, else 3 host floats.
int frames_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, uint64_t min_neighbors,
                const float* view, ptk_frame* d_frames, ptk_moments* d_moments, hipStream_t s);
// aggregate_within_self (ptk_kernels_aggregate.hpp): out[index][0 .. channels) and counts[index] (may
// be null) of leaf positions [first, first + n) of a float32 handle that check_radius_self serves.  `flags`: a PTK_AGG_*
// op, | PTK_AGG_INCLUDE_SELF.  One launch per channel window.
int aggregate_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, const float* d_values,
                   uint32_t channels, uint32_t flags, float* d_out, uint64_t* d_counts, hipStream_t s);
void warm_self();
// ptk_family_align.hip: align_step (ptk_kernels_align.hpp).  The caller's workspace holds q', the rows
// (used when the caller keeps none) and the partials of every level: per entry of a level the 29 sums of the wider mode
// and a count.
constexpr size_t kAlignEntryBytes = 30 * 8;
struct AlignLayout {
  size_t q, rows, partials, bytes;  // offsets of the three parts (256-byte aligned), the size of the whole
};
AlignLayout align_layout(uint64_t nq);
// The handle's inverse leaf permutation (uint32 per point): allocated, filled by one scatter kernel on `s`, waited for.
int align_inverse(const ptk_tree* t, void** d_inv, hipStream_t s);
// d_out[i] = R q_i + t; `m`: 12 host floats, row-major [R|t]
int align_pose(const ptk_tree* t, const float* d_q, uint64_t nq, const float* m, float* d_out, hipStream_t s);
// The levels of the summation tree over the rows of the k = 1 search of d_qp, and the record; d_normals null:
// point-to-point.  Reads the handle's inverse permutation (built before: align_inverse_of).
int align_reduce(const ptk_tree* t, const ptk::Neighbor* d_rows, const float* d_qp, uint64_t nq, const float* d_normals,
                 float max_distance, char* d_partials, ptk_align_sums* d_out, hipStream_t s);
void warm_align();
// ptk_family_suppress.hip: suppress_within_self (ptk_kernels_suppress.hpp).  d_keep (n_points uint8
// cells by original index) is the caller's output and the only working array: suppress_init sets every cell to
// "undecided"; suppress_self / suppress64_self is ONE ROUND over leaf positions [first, first + n) of a handle
// check_radius_self serves (d_radii null: every point gets `radius`; d_scores null: the default order) and adds the lanes
// it leaves undecided to *d_undecided.  The caller runs a round over all pieces before the next, on one stream, until a
// round adds nothing.  `later_round`: not the first round of its call (the profile counts it as the search's tail).
int suppress_init(uint64_t n, uint8_t* d_keep, hipStream_t s);
int suppress_self(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_radii, const float* d_scores,
                  uint8_t* d_keep, uint32_t* d_undecided, bool later_round, hipStream_t s);
int suppress64_self(const ptk::DevTree64& dev, int metric, uint64_t first, uint64_t n, double radius, const double* d_radii,
                    const float* d_scores, uint8_t* d_keep, uint32_t* d_undecided, ptk::Rec64* stack, uint32_t slots,
                    hipStream_t s);
// The counter of a call: one device word, zeroed on the stream before a round, and one page-locked word it is copied to
// after the round -- read() WAITS for the stream.  Both belong to the call while it runs (two calls on two streams share
// nothing); they come from a pool the library keeps per device and go back to it when the call returns: nothing is
// freed, because hipFree / hipHostFree wait for the WHOLE device, every other stream's work included.  The pool grows to
// the largest number of calls that ever ran side by side on a device (8 bytes each) and lives as long as the process.
struct SuppressCounter {
  uint32_t* d_word = nullptr;
  uint32_t* h_word = nullptr;
  int device = -1;
  SuppressCounter() = default;
  SuppressCounter(const SuppressCounter&) = delete;
  SuppressCounter& operator=(const SuppressCounter&) = delete;
  ~SuppressCounter();  // back to the pool
  int alloc();         // from the pool of the current device; a new pair on the first calls only
  int zero(hipStream_t s);
  int read(hipStream_t s, uint32_t* undecided);
};
// The rounds of either precision: `round(d_undecided, later_round)` enqueues one round over all pieces.  *n_rounds (may be null): the
// rounds launched.
// The rounds wait on their stream, so a stream under capture cannot take them (ptk.h): refused up front, by name, before
// anything is enqueued or the capture is disturbed.
inline int suppress_check_stream(hipStream_t s) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &status) != hipSuccess) {
    (void)hipGetLastError();
    return PTK_OK;  // (not a stream this call can ask about: the launches below say what is wrong with it)
  }
  if (status != hipStreamCaptureStatusNone)
    return ptkb::fail(PTK_ERR_INVALID,
                      "suppress_within_self: the stream is being captured -- this call waits on its stream once per round "
                      "and cannot be captured into a graph");
  return PTK_OK;
}
template <class Round>
inline int suppress_rounds(uint64_t n_points, uint8_t* d_keep, hipStream_t s, uint32_t* n_rounds, Round&& round) {
  SuppressCounter counter;
  int rc = counter.alloc();
  if (rc == PTK_OK) rc = suppress_init(n_points, d_keep, s);
  uint32_t rounds = 0, undecided = 1;
  // (every round decides at least the undecided point of highest key: at most n_points rounds)
  while (rc == PTK_OK && undecided != 0 && rounds < n_points) {
    rc = counter.zero(s);
    if (rc == PTK_OK) rc = round(counter.d_word, rounds > 0);
    if (rc == PTK_OK) rc = counter.read(s, &undecided);
    ++rounds;
  }
  if (n_rounds != nullptr) *n_rounds = rounds;
  if (rc == PTK_OK && undecided != 0)
    return ptkb::fail(PTK_ERR_DEVICE, "suppress_within_self: %u points undecided after %u rounds", undecided, rounds);
  // (after a failure half-way: nothing of this call is left running on the counter when it goes back to the pool)
  if (rc != PTK_OK) (void)hipStreamSynchronize(s);
  return rc;
}
void warm_suppress();
// ptk_family_spacing.hip: spacing_knn_self (ptk_kernels_spacing.hpp).  spacing_self: route 1, the
// traversal of knn_self on leaf positions [first, first + n) with the reducing exit -- d_mean[index], d_kth[index] (may be
// null).  spacing_rows*: the `drop` step of the staged route over rows of k + 1 records.  spacing_statistics*: the record
// and / or the mask (either may be null, not both) from the n means, enqueued on `s`; d_workspace holds
// spacing_workspace_bytes(n): a record (the mask needs one where the caller keeps none) and per level of the summation
// tree its partials and counts.
int spacing_self(const ptk_tree* t, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, float* d_mean, float* d_kth,
                 hipStream_t s);
int spacing_rows(const ptk::Neighbor* rows, const float4* recs, const int32_t* index, uint64_t first, uint64_t n, uint32_t k,
                 uint32_t flags, float* d_mean, float* d_kth, hipStream_t s);
int spacing_rows64(const void* rows, const int32_t* index, uint64_t first, uint64_t n, uint32_t k, uint32_t flags,
                   double* d_mean, double* d_kth, hipStream_t s);
constexpr size_t kSpacingRecordBytes = 256;  // (the record's slot at the head of the workspace)
constexpr size_t kSpacingEntryBytes = 16;    // (a partial and a count)
size_t spacing_workspace_bytes(uint64_t n);
int spacing_statistics(const float* d_mean, uint64_t n, float ratio, uint8_t* d_keep, ptk_spacing_stats* d_stats,
                       char* d_workspace, hipStream_t s);
int spacing_statistics64(const double* d_mean, uint64_t n, float ratio, uint8_t* d_keep, ptk_spacing_stats* d_stats,
                         char* d_workspace, hipStream_t s);
void warm_spacing();
// The workspace check of the _device forms of either precision: none is needed where neither the mask nor the record is
// asked for.
inline int spacing_check_workspace(uint64_t n, bool reduce, const void* d_workspace, uint64_t workspace_bytes) {
  if (!reduce || n == 0) return PTK_OK;
  const size_t need = spacing_workspace_bytes(n);
  if (d_workspace == nullptr) return ptkb::fail(PTK_ERR_INVALID, "spacing_knn_self: null workspace");
  if (workspace_bytes < need)
    return ptkb::fail(PTK_ERR_INVALID,
                      "spacing_knn_self: the workspace holds %llu bytes, %llu points need %llu (ptk_spacing_knn_self_workspace)",
                      (unsigned long long)workspace_bytes, (unsigned long long)n, (unsigned long long)need);
  return PTK_OK;
}
// The host-buffer form of either precision: one block per call holds the outputs that were asked for and the workspace;
// `device(d_mean, d_kth, d_keep, d_stats, d_workspace, workspace_bytes)` is the _device form on the null stream; the
// outputs come down with blocking copies.  Nothing goes up.  The caller has set the device.
template <class Real, class Device>
inline int spacing_host_form(uint64_t n, Real* mean, Real* kth, uint8_t* keep, ptk_spacing_stats* stats, Device&& device) {
  const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const bool reduce = keep != nullptr || stats != nullptr;
  const size_t real_bytes = (size_t)n * sizeof(Real);
  const size_t o_kth = pad(real_bytes);
  const size_t o_keep = o_kth + (kth != nullptr ? pad(real_bytes) : 0);
  const size_t o_stats = o_keep + (keep != nullptr ? pad((size_t)n) : 0);
  const size_t o_ws = o_stats + (stats != nullptr ? pad(sizeof(ptk_spacing_stats)) : 0);
  const size_t ws_bytes = reduce ? spacing_workspace_bytes(n) : 0;
  ptkb::DeviceBlock block;
  if (block.alloc(o_ws + ws_bytes + 256) != hipSuccess) {
    (void)hipGetLastError();
    return ptkb::fail(PTK_ERR_NOMEM, "out of device memory (the outputs of spacing_knn_self)");
  }
  char* base = block.as<char>();
  int rc = device(reinterpret_cast<Real*>(base), kth != nullptr ? reinterpret_cast<Real*>(base + o_kth) : nullptr,
                  keep != nullptr ? reinterpret_cast<uint8_t*>(base + o_keep) : nullptr,
                  stats != nullptr ? reinterpret_cast<ptk_spacing_stats*>(base + o_stats) : nullptr,
                  reduce ? static_cast<void*>(base + o_ws) : nullptr, (uint64_t)ws_bytes);
  // (the block is freed when this returns: everything enqueued on it has to be done -- also after a refusal half-way)
  hipError_t he = hipStreamSynchronize(nullptr);
  if (rc != PTK_OK) return rc;
  if (he == hipSuccess) he = hipMemcpy(mean, base, real_bytes, hipMemcpyDeviceToHost);
  if (he == hipSuccess && kth != nullptr) he = hipMemcpy(kth, base + o_kth, real_bytes, hipMemcpyDeviceToHost);
  if (he == hipSuccess && keep != nullptr) he = hipMemcpy(keep, base + o_keep, (size_t)n, hipMemcpyDeviceToHost);
  if (he == hipSuccess && stats != nullptr) he = hipMemcpy(stats, base + o_stats, sizeof(ptk_spacing_stats), hipMemcpyDeviceToHost);
  if (he != hipSuccess) return ptkb::fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(he));
  return PTK_OK;
}
// ptk_family_mst.hip: mst_within_self (ptk_kernels_mst.hpp).  The caller's workspace: a 256-byte
// header whose first word is the number of edge records, then the arrays of the kernel header, each 256-byte aligned.
struct MstLayout {
  size_t parent, label, cand, best_wlo, best_hi, comp, info, arrive, bytes;
};
// The branches the component table covers: none for a tree whose root is a leaf (the encoder keeps one padding record).
inline uint64_t mst_branches(const ptk_tree* t) { return (t->dev.root_ref & 0x80000000u) != 0 ? 0 : t->n_branches; }
inline MstLayout mst_layout(uint64_t n, uint64_t n_branches) {
  const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  MstLayout at;
  at.parent = 256;
  at.label = at.parent + pad((size_t)n * 4);
  at.cand = at.label + pad((size_t)n * 4);
  at.best_wlo = at.cand + pad((size_t)n * 8);
  at.best_hi = at.best_wlo + pad((size_t)n * 8);
  at.comp = at.best_hi + pad((size_t)n * 4);
  at.info = at.comp + pad((size_t)n_branches * 4);
  at.arrive = at.info + pad((size_t)n_branches * 4);
  at.bytes = at.arrive + pad((size_t)n_branches * 4);
  return at;
}
// mst_begin: the arrays at their start (every point a component), the branches' parent links.  A round: mst_table (not
// before the first round, and not with skip == 0), mst_search over all pieces of leaf positions, mst_join (the tie pass,
// the emit-and-link pass -- it adds the edges it writes to *d_added --, the relabel pass).
int mst_begin(const ptk_tree* t, char* ws, hipStream_t s);
int mst_table(const ptk_tree* t, char* ws, hipStream_t s);
int mst_search(const ptk_tree* t, uint64_t first, uint64_t n, float radius, const float* d_core, char* ws, uint32_t skip,
               bool later_round, hipStream_t s);
int mst_join(const ptk_tree* t, char* ws, ptk_mst_edge* d_edges, uint32_t* d_added, hipStream_t s);
void warm_mst();
// The rounds: `round(d_added, rounds_before)` enqueues one.  The counter is suppress_within_self's (its pool, its wait);
// the call ends when a round adds nothing, or when the forest is a tree.  *n_edges, *n_rounds: may be null.
template <class Round>
inline int mst_rounds(uint64_t n_points, hipStream_t s, uint64_t* n_edges, uint32_t* n_rounds, Round&& round) {
  SuppressCounter counter;
  int rc = counter.alloc();
  uint32_t rounds = 0, added = 1;
  uint64_t total = 0;
  // (every round that adds an edge joins two components: at most n_points - 1 of them, and one that adds nothing)
  while (rc == PTK_OK && added != 0 && total + 1 < n_points && rounds < n_points) {
    rc = counter.zero(s);
    if (rc == PTK_OK) rc = round(counter.d_word, rounds);
    if (rc == PTK_OK) rc = counter.read(s, &added);
    total += added;
    ++rounds;
  }
  if (n_rounds != nullptr) *n_rounds = rounds;
  if (n_edges != nullptr) *n_edges = rc == PTK_OK ? total : 0;
  // (after a failure half-way: nothing of this call is left running on the counter when it goes back to the pool)
  if (rc != PTK_OK) (void)hipStreamSynchronize(s);
  return rc;
}
// Rows of a piece of the staged route: its two temporaries (the query rows, the k + 1 records per row) stay under
// kSelfStageBytes; test hook self_piece.
constexpr size_t kSelfStageBytes = size_t(256) << 20;
inline uint64_t self_piece_rows(uint32_t dim, uint32_t k, size_t scalar_bytes, size_t record_bytes) {
  const int forced = ptkb::knob_int("self_piece", 0);
  if (forced > 0) return (uint64_t)forced;
  const size_t per_row = (size_t)dim * scalar_bytes + ((size_t)k + 1) * record_bytes;
  return std::max<uint64_t>(64, kSelfStageBytes / per_row);
}
// The staged route over either handle: per piece of leaf positions, the three steps of DESIGN.md §2.  `queries(first, n,
// d_q)`, `search(d_q, n, d_rows)` -- the handle's own device search with k + 1, which takes the handle's scratch lock
// itself -- and `drop(d_rows, first, n)` enqueue on the caller's stream; the temporaries are one per-call block, freed
// after a wait for the stream (this route allocates and waits: it is not enqueue-only, ptk.h).
template <class Real, class Nb, class Queries, class Search, class Drop>
inline int self_staged(uint64_t n_points, uint32_t dim, uint32_t k, hipStream_t s, Queries&& queries, Search&& search,
                       Drop&& drop) {
  const uint64_t max_batch = (uint64_t)std::max(1, ptkb::env_int("PTK_MAX_BATCH", 1 << 25));
  const uint64_t piece = std::min(std::min(self_piece_rows(dim, k, sizeof(Real), sizeof(Nb)), max_batch), n_points);
  const size_t q_bytes = ((size_t)piece * dim * sizeof(Real) + 255) & ~(size_t)255;
  ptkb::DeviceBlock block;
  if (block.alloc(q_bytes + (size_t)piece * ((size_t)k + 1) * sizeof(Nb)) != hipSuccess) {
    (void)hipGetLastError();
    return ptkb::fail(PTK_ERR_NOMEM, "out of device memory (the temporaries of search_knn_self)");
  }
  Real* d_q = block.as<Real>();
  Nb* d_rows = reinterpret_cast<Nb*>(block.as<char>() + q_bytes);
  int rc = PTK_OK;
  for (uint64_t first = 0; first < n_points && rc == PTK_OK; first += piece) {
    const uint64_t n = std::min(piece, n_points - first);
    rc = queries(first, n, d_q);
    if (rc == PTK_OK) rc = search(d_q, n, d_rows);
    if (rc == PTK_OK) rc = drop(d_rows, first, n);
  }
  // (the block is freed when this returns: everything enqueued on it has to be done -- also after a refusal half-way)
  if (hipStreamSynchronize(s) != hipSuccess && rc == PTK_OK)
    rc = ptkb::fail(PTK_ERR_DEVICE, "hipStreamSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
  return rc;
}
}  // namespace ptkf
