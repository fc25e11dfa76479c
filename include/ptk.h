/* ptk.h -- C ABI of the MI355X batched k-NN backend (libptk.so).
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json: batched
 * search_nn / search_knn / search_radius (and search_box) on a pico_tree
 * kd_tree<Space, metric_l2_squared, int> over float32 points.  Plain C types
 * only: no exceptions, no STL, no torch types cross this line.  Every entry
 * point returns PTK_OK (0) or a negative ptk_status; the message for the last
 * failure on the calling thread is available from ptk_last_error().
 *
 * What each entry point replaces in the reference (paths relative to
 * /root/reference):
 *
 *   ptk_tree_create_from_points   kd_tree ctor with max_leaf_size_t, bounds from
 *                                 the space, sliding midpoint rule:
 *                                 src/pico_tree/pico_tree/kd_tree.hpp:76-88,
 *                                 internal/kd_tree_builder.hpp:456-512; as bound
 *                                 by the Python module in
 *                                 src/pyco_tree/pico_tree/_pyco_tree/kd_tree.hpp:112-115
 *   ptk_tree_create               the same tree handed over already built and
 *                                 flattened (what include/pico_tree/kd_tree.hpp
 *                                 does for arbitrary Space types); the node
 *                                 stream is the DFS pre-order of
 *                                 internal/kd_tree_data.hpp:109-135
 *   ptk_search_knn[_device]       the OpenMP batch loop over kd_tree::search_knn:
 *                                 _pyco_tree/kd_tree.hpp:117-135 (exact) and
 *                                 :144-168 (approximate), i.e. kd_tree.hpp:169-181,
 *                                 :205-218 per row; k == 1 is search_nn
 *                                 (kd_tree.hpp:126-129)
 *   ptk_search_radius_*           the batch loop over kd_tree::search_radius:
 *                                 _pyco_tree/kd_tree.hpp:179-200, :211-233, i.e.
 *                                 kd_tree.hpp:257-290 per row
 *   ptk_search_box_*              the batch loop over kd_tree::search_box:
 *                                 _pyco_tree/kd_tree.hpp:245-268, kd_tree.hpp:296-318
 *   ptk_tree_destroy              ~kd_tree
 *   ptk_tree64_* / ptk_search64_* the same entry points for kd_trees over double
 *                                 points (_pyco_tree/kd_tree.hpp:383-445 dispatches
 *                                 on the array dtype)
 *
 * Results contract: neighbour indices are bit-identical to the reference CPU
 * kd_tree on the same inputs, squared distances bit-identical to the reference
 * compiled without FMA contraction (-ffp-contract=off).
 *
 * Non-finite and overflowing inputs (tests/test_non_finite.py):
 *   - A query row or a box corner may hold NaN, +-Inf or any finite value, a
 *     value whose distances overflow included.  Such a row gets what the
 *     reference gives it, in every search (knn, knn_within, count_within,
 *     radius, box; float32 and float64; every metric), for every entry the
 *     reference writes; no query row changes the result of another row; and
 *     the call returns PTK_OK.  (A row with a NaN or an infinite coordinate
 *     accepts no point under the sum metrics: `max > distance` is false.  A
 *     NaN box corner coordinate does not bound its side of the axis:
 *     box.hpp:31-40 tests `min > x || max < x`; under the two topological
 *     metrics the reference's query box is a metric_box_map, which tests
 *     `min <= x && x <= max` (segment.hpp:32,63): there it contains nothing.)
 *   - A k-NN slot the reference's search never writes -- k > n_points; a row
 *     that accepts fewer than k points, where the reference writes the
 *     distance of slot k - 1 only and leaves the rest of the caller's row as
 *     it found it (search_visitor.hpp:50,102) -- holds {index 0, distance
 *     FLT_MAX} ({0, DBL_MAX}, pad_ zero, for ptk_neighbor64) on every path:
 *     every k, any dimension, every metric, device and ptk_host_search_knn.
 *     No slot of an output row is left unwritten.  (search_knn_within keeps
 *     its own padding, {-1, radius}.)
 *   - The POINTS a tree is built from must be finite: ptk_tree_create_from_points,
 *     ptk_tree64_create_from_points and ptk_multi_create_from_points return
 *     PTK_ERR_INVALID, the message naming the first offending point, for a
 *     NaN or +-Inf coordinate (the builder partitions with `<` through
 *     std::nth_element as the reference's, kd_tree_builder.hpp: NaN makes that
 *     undefined, an infinite coordinate makes a NaN split).  +-FLT_MAX is
 *     finite and accepted.  The *_create_from_stream loaders and
 *     ptk_tree_create do not look at the points, as the reference's load.
 *
 * Threading: a ptk_tree is immutable after creation; search calls on one handle
 * may be issued concurrently from several host threads (each call uses its own
 * scratch; calls that share a HIP stream serialise on it).
 */
#ifndef PTK_H_
#define PTK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTK_VERSION 101 /* 0.1.1: ptk_warmup, ptk_profile_get_sized */

typedef enum ptk_status {
  PTK_OK = 0,
  PTK_ERR_INVALID = -1,     /* bad argument (null pointer, k == 0, dim == 0 ...) */
  PTK_ERR_UNSUPPORTED = -2, /* valid request this build cannot run on the GPU   */
  PTK_ERR_DEVICE = -3,      /* HIP runtime error, or no usable gfx950 device    */
  PTK_ERR_NOMEM = -4        /* host or device allocation failed                 */
} ptk_status;

/* Layout-identical to pico_tree::neighbor<int, float> (core.hpp:24-46) and to
 * the Python binding's [('index','<i4'),('distance','<f4')] record. */
typedef struct ptk_neighbor {
  int32_t index;
  float distance;
} ptk_neighbor;

/* One node of the flat tree, DFS pre-order, 16 bytes.  The left child of a
 * branch is the next node (self + 1).
 *   branch: a = bits of float left_max, b = bits of float right_min,
 *           right = index of the right child, split_dim = split axis
 *   leaf:   a = begin, b = end (positions in the indices array, int32),
 *           right = PTK_LEAF, split_dim = 0
 * Field meanings follow internal/kd_tree_node.hpp:31-50. */
#define PTK_LEAF 0xFFFFFFFFu
typedef struct ptk_node {
  uint32_t a;
  uint32_t b;
  uint32_t right;
  uint32_t split_dim;
} ptk_node;

typedef struct ptk_tree_desc {
  uint32_t dim;          /* spatial dimension (>= 1)                            */
  uint64_t n_points;     /* number of points (>= 1, < 2^31)                     */
  const float* points;   /* n_points x dim, row-major, ORIGINAL order (host)    */
  uint64_t n_nodes;      /* number of nodes in the DFS stream                   */
  const ptk_node* nodes; /* host                                                */
  const int32_t* indices;/* n_points entries: leaf-ordered permutation (host)   */
  const float* root_min; /* dim floats: start bounds of the build, or NULL =     */
  const float* root_max; /*   bounding box of the points (both or neither)      */
  uint32_t max_depth;    /* informational; recomputed from the node stream      */
  int32_t device;        /* HIP device ordinal, PTK_DEVICE_CURRENT or _NONE     */
} ptk_tree_desc;

#define PTK_DEVICE_CURRENT (-1) /* whatever hipGetDevice() returns                 */
#define PTK_DEVICE_NONE (-2)    /* host-only handle: structure queries work, every
                                   search returns PTK_ERR_DEVICE                    */

typedef struct ptk_tree ptk_tree; /* opaque */

typedef struct ptk_tree_info {
  uint32_t dim;
  uint64_t n_points;
  uint64_t n_nodes;      /* nodes in the DFS stream (branches + leaves)         */
  uint64_t n_leaves;
  uint32_t max_depth;
  uint32_t max_leaf_count;
  uint64_t device_bytes; /* HBM held by the handle                              */
  int32_t device;
} ptk_tree_info;

/* Query-order policy for the nearest-neighbour kernels.  Coherent (spatially
 * sorted) batches traverse the tree several times faster; with PTK_REORDER_ON
 * the backend sorts the batch along a Morton curve on the device and scatters
 * results back, so the caller-visible row order never changes.  PTK_REORDER_AUTO
 * (the default) sorts batches of 8 192 queries or more; a k = 1 batch is sampled on
 * the device first and, if it already is in a coherent order (a scan in scan order),
 * searched in the caller's order -- the verdict never travels to the host. */
enum { PTK_REORDER_AUTO = 0, PTK_REORDER_ON = 1, PTK_REORDER_OFF = 2 };

/* ---- library ---------------------------------------------------------- */
int ptk_version(void);
const char* ptk_last_error(void); /* thread-local, never NULL */
int ptk_device_count(void);       /* number of visible HIP devices, or < 0; no side effects */
/* Starts loading the library's device code for `device` (< 0: the calling thread's current device)
 * on a thread of the library and returns at once: the first ptk_tree_create* for that device then
 * does not wait for it (~0.2 s).  Optional -- the first creation starts it itself; one load per
 * device and process; PTK_EAGER_WARMUP=0 in the environment turns it off. */
int ptk_warmup(int32_t device);

/* ---- tree lifetime ---------------------------------------------------- */

/* Builds the kd-tree on the host (sliding midpoint, max_leaf_size stop, bounds
 * from the points) and uploads it.  points may be freed after the call.  A point
 * with a NaN or +-Inf coordinate: PTK_ERR_INVALID, no handle ("Non-finite and
 * overflowing inputs" above). */
int ptk_tree_create_from_points(const float* points, uint64_t n_points,
                                uint32_t dim, uint64_t max_leaf_size,
                                int32_t device, ptk_tree** out);

/* Uploads an already built flat tree.  All host arrays may be freed after. */
int ptk_tree_create(const ptk_tree_desc* desc, ptk_tree** out);

void ptk_tree_destroy(ptk_tree* tree);

int ptk_tree_get_info(const ptk_tree* tree, ptk_tree_info* info);

/* Copies the host-side flat tree out (for bindings that save it or inspect it).
 * Pass NULL to skip an array.  nodes needs n_nodes entries, indices n_points. */
int ptk_tree_get_flat(const ptk_tree* tree, ptk_node* nodes, int32_t* indices,
                      float* root_min, float* root_max);

int ptk_tree_set_reorder(ptk_tree* tree, int mode);

/* Metric of the searches on this handle (the tree itself does not depend on it).  The
 * reference's euclidean search is generic over the metric (kd_tree.hpp:23, metric.hpp:72-150):
 *   PTK_METRIC_L2_SQUARED  metric_l2_squared (default): squared distances, radius squared
 *   PTK_METRIC_L1          metric_l1:    sum of |differences|
 *   PTK_METRIC_LPINF       metric_lpinf: max of |differences|
 *   PTK_METRIC_LNINF       metric_lninf: min of |differences| (metric.hpp:157-186)
 *   PTK_METRIC_SO2         metric_so2 (metric.hpp:186-220): points on the circle [0, 1] / 0 ~ 1; dim 1 only
 *   PTK_METRIC_SE2_SQUARED metric_se2_squared (metric.hpp:228-257): x, y on the plane, angle on the circle;
 *                          dim 3 only.  The two topological metrics are searched as the reference's
 *                          search_nearest_topological does (kd_tree_search.hpp:115-229) and need the four
 *                          bounds per branch: trees made by ptk_tree_create_from_points have them; for
 *                          ptk_tree_create hand them over with ptk_tree_set_outer_bounds first.  float32,
 *                          knn and radius searches (the box search of these trees stays on the host members).
 * Set once, before the first search. */
enum { PTK_METRIC_L2_SQUARED = 0, PTK_METRIC_L1 = 1, PTK_METRIC_LPINF = 2, PTK_METRIC_LNINF = 3, PTK_METRIC_SO2 = 4,
       PTK_METRIC_SE2_SQUARED = 5 };
int ptk_tree_set_metric(ptk_tree* tree, int metric);
/* The two bounds of every branch that ptk_node does not hold -- outer[2 i] = min of the left
 * child's box, outer[2 i + 1] = max of the right child's box along the split axis of node i (the
 * other half of the reference's kd_tree_node_topological, kd_tree_node.hpp:56-67); entries of leaf
 * nodes are ignored.  Needed (before ptk_tree_set_metric) by the topological metrics on a tree made
 * by ptk_tree_create. */
int ptk_tree_set_outer_bounds(ptk_tree* tree, const float* outer, uint64_t n_nodes);
/* The same array back (2 floats per node; PTK_ERR_INVALID if the tree has none). */
int ptk_tree_get_outer_bounds(const ptk_tree* tree, float* outer);

/* The tree in the reference's own binary format (kd_tree::save / kd_tree::load,
 * kd_tree.hpp:336-370, internal/kd_tree_data.hpp:43-58,90-135): sdim, indices,
 * root box, nodes depth-first.  Files written by the reference load here and
 * vice versa (the Python module's PKD header, _pyco_tree/kd_tree.hpp:547-614,
 * is added by the binding).  ptk_tree_serialize: pass buf == NULL to get the
 * size; PTK_ERR_INVALID if cap is too small.  Like the reference, loading does
 * not check that the stream belongs to the points (kd_tree.hpp:346-351). */
int ptk_tree_serialize(const ptk_tree* tree, void* buf, uint64_t cap, uint64_t* size);
int ptk_tree_create_from_stream(const float* points, uint64_t n_points, uint32_t dim,
                                const void* stream, uint64_t stream_bytes,
                                int32_t device, ptk_tree** out);
/* The same for a tree over a topological space (kd_tree<space, metric_so2 | metric_se2_squared>::save /
 * ::load): its branches carry four bounds on disk (kd_tree_branch_double, internal/kd_tree_node.hpp:52-67).
 * Loading keeps the two outer ones with the handle (as ptk_tree_set_outer_bounds would), so that
 * ptk_tree_set_metric(PTK_METRIC_SO2 | PTK_METRIC_SE2_SQUARED) can follow at once; writing needs them. */
int ptk_tree_serialize_topological(const ptk_tree* tree, void* buf, uint64_t cap, uint64_t* size);
int ptk_tree_create_from_topological_stream(const float* points, uint64_t n_points, uint32_t dim,
                                            const void* stream, uint64_t stream_bytes,
                                            int32_t device, ptk_tree** out);

/* ---- k nearest neighbours --------------------------------------------- */

/* Host buffers.  queries: nq x dim row-major.  out: nq x k row-major; row i is
 * the ascending k-list of query i.  k > n_points, or a query row that accepts
 * fewer than k points (NaN, +-Inf, distances that overflow): the accepted
 * neighbours in order, then {0, FLT_MAX} in every slot behind them ("Non-finite
 * and overflowing inputs" above).  e is the approximation ratio in metric units
 * (kd_tree.hpp:131-153); e == 1 is the exact search. */
int ptk_search_knn(const ptk_tree* tree, const float* queries, uint64_t nq,
                   uint32_t k, float e, ptk_neighbor* out);

/* Device buffers on the tree's device; asynchronous on `stream` (a hipStream_t,
 * NULL = the default stream).  No host synchronisation is performed: the call only
 * enqueues -- the decisions that depend on the batch (is it already in a coherent order?
 * which queries need the cooperative search?) are taken on the device. */
int ptk_search_knn_device(const ptk_tree* tree, const float* d_queries,
                          uint64_t nq, uint32_t k, float e,
                          ptk_neighbor* d_out, void* stream);

/* ---- the k nearest within a radius --------------------------------------- */

/* Results contract: row i is the reference's search_knn(q_i, min(k, n_points)) row,
 * keeping only the entries with distance < radius (strict, as the radius search:
 * search_visitor.hpp:141), in the same order, padded to k entries with {index = -1,
 * distance = radius}.  radius is in metric units (squared for L2^2).  Every k >= 1 is valid,
 * k > n_points included; k == 0 and a radius that is NaN or negative are PTK_ERR_INVALID.  The
 * search is exact (no e).  The k-list starts at the radius, so no query's search reaches
 * (much) past it.  Topological metrics: PTK_ERR_UNSUPPORTED (ptk_host_search_knn_within serves
 * them).  The host form moves the batch through the handle's device buffers; the device form
 * only enqueues on `stream`, as ptk_search_knn_device. */
int ptk_search_knn_within(const ptk_tree* tree, const float* queries, uint64_t nq,
                          uint32_t k, float radius, ptk_neighbor* out);
int ptk_search_knn_within_device(const ptk_tree* tree, const float* d_queries,
                                 uint64_t nq, uint32_t k, float radius,
                                 ptk_neighbor* d_out, void* stream);

/* ---- each tree point's k nearest other points ---------------------------- */

/* Results contract: n_points rows of k records; row i belongs to the point with original index i.
 * Let m = min(k + 1, n_points) and R the reference's search_knn(p_i, m) row (the same tree, the same metric, exact).
 * Row i is R with ONE entry removed -- the first entry whose index is i if there is one, otherwise the last entry
 * (k + 1 or more other points coincide with p_i and the reference visits them first) --, the remaining entries in
 * their order, padded to k entries with {index = -1, distance = FLT_MAX}: k > n_points - 1, or a slot the reference
 * never accepted (an accepted distance is always < FLT_MAX).  Same indices, same distance bits.  The search is exact
 * (no e).  k == 0 is PTK_ERR_INVALID, a null output with n_points > 0 is PTK_ERR_INVALID, a host-only handle is
 * PTK_ERR_DEVICE.  There is no query buffer: the handle holds every point on the device, in leaf order.
 *   ptk_debug_self_route says which route serves (tree, k): 1 = the direct kernel (dim <= 3, the four non-topological
 * metrics, at most 1 031 levels, k <= 63) -- the device form only enqueues on `stream`: no allocation, no wait --;
 * 2 = the staged route (every other handle): pieces of the tree's points go through ptk_search_knn_device with k + 1
 * and lose their own entry on the device.  That route ALLOCATES a block per call (at most 256 MiB) and WAITS for
 * `stream` before it returns: it is not enqueue-only, and must not be called under a stream capture.  A refusal of the
 * underlying search (PTK_ERR_UNSUPPORTED: a topological tree deeper than the device stack) is passed on unchanged;
 * ptk_host_search_knn_self serves it.  The host form copies the rows back only: nothing is uploaded. */
int ptk_search_knn_self(const ptk_tree* tree, uint32_t k, ptk_neighbor* out);
int ptk_search_knn_self_device(const ptk_tree* tree, uint32_t k, ptk_neighbor* d_out, void* stream);

/* ---- neighbour counts within a radius ------------------------------------ */

/* Results contract: counts[i] is the length of the reference's search_radius(q_i, radius) row -- the
 * points its traversal visits with distance < radius (strict: search_visitor.hpp:141) -- and, with max_count > 0,
 * min(that length, max_count); max_count == 0 means no limit.  radius is in metric units (squared for L2^2); 0 gives
 * zeros, FLT_MAX and +inf are valid; NaN or a negative radius is PTK_ERR_INVALID, as is a null `counts` with nq > 0.
 * Exact (no e).  A query row with NaN or +-Inf coordinates gets what the reference gives it.  Every metric; what the
 * device refuses is PTK_ERR_UNSUPPORTED (ptk_host_search_count_within serves it).  The rows are never built, and the
 * handle's radius capture (ptk_search_radius_count / _fill) is left as it is.  The first call on a handle builds a
 * per-branch side table on the device (ptk_tree_info.device_bytes includes it from then on); the device form
 * otherwise only enqueues on `stream`, as ptk_search_knn_device.  The host form moves the batch through the handle's
 * device buffers. */
int ptk_search_count_within(const ptk_tree* tree, const float* queries, uint64_t nq, float radius,
                            uint64_t max_count, uint64_t* counts);
int ptk_search_count_within_device(const ptk_tree* tree, const float* d_queries, uint64_t nq, float radius,
                                   uint64_t max_count, uint64_t* d_counts, void* stream);

/* ---- a radius per query row ---------------------------------------------- */

/* ptk_search_knn_within and ptk_search_count_within with `radii`, nq entries: entry i bounds query row i, in the
 * caller's order (max_count stays one value per call).  Results contract: row i / counts[i] is, bit for
 * bit, row i / counts[i] of the scalar call on the same batch with radius = radii[i] -- the reference's
 * search_knn(q_i, min(k, n_points)) row filtered with the strict `< radii[i]` and padded with {-1, radii[i]}; the length
 * of the reference's search_radius(q_i, radii[i]) row, clamped to max_count.  No row's radius changes another row: a
 * warm-started ICP iteration passes each row the distance its last iteration found, and no row's search reaches (much)
 * past its own.
 * Arguments: the scalar form's checks, and a null `radii` with nq > 0 is PTK_ERR_INVALID.  The host-buffer forms scan
 * `radii`: a NaN or negative entry is PTK_ERR_INVALID, and ptk_last_error names the first such row.  The _device forms
 * only enqueue (d_radii is device memory on the tree's device, ordered on `stream` like d_queries) and cannot look at
 * the values: there a row whose radius is NaN or negative is all padding {-1, radii[i]} (its count is 0), every other
 * row is what it would be without that row, and the call returns PTK_OK.  +inf, FLT_MAX, 0 and subnormal radii are
 * valid per row and give what the scalar call gives for them.
 * Where the device serves them: ptk_search_knn_within_radii wherever the scalar form is served (every dimension, trees
 * of the deep stack class included; topological metrics PTK_ERR_UNSUPPORTED).  ptk_search_count_within_radii by the
 * side-table count kernel only -- dim <= 3, the four non-topological metrics, not the deep stack class; dim > 3,
 * topological metrics and deep trees, which the scalar call sends through the count pass of the radius search (one
 * radius per launch), are PTK_ERR_UNSUPPORTED for now (ptk_host_search_count_within_radii serves them).
 * The first count of either kind builds the handle's side table. */
int ptk_search_knn_within_radii(const ptk_tree* tree, const float* queries, uint64_t nq, uint32_t k, const float* radii,
                                ptk_neighbor* out);
int ptk_search_knn_within_radii_device(const ptk_tree* tree, const float* d_queries, uint64_t nq, uint32_t k,
                                       const float* d_radii, ptk_neighbor* d_out, void* stream);
int ptk_search_count_within_radii(const ptk_tree* tree, const float* queries, uint64_t nq, const float* radii,
                                  uint64_t max_count, uint64_t* counts);
int ptk_search_count_within_radii_device(const ptk_tree* tree, const float* d_queries, uint64_t nq, const float* d_radii,
                                         uint64_t max_count, uint64_t* d_counts, void* stream);

/* ---- radius search (ragged output) ------------------------------------ */

/* Pass 1: counts[i] = number of points with distance < radius (strict,
 * search_visitor.hpp:141).  radius is in metric units (squared for L2^2). */
int ptk_search_radius_count(const ptk_tree* tree, const float* queries,
                            uint64_t nq, float radius, float e,
                            uint64_t* counts);
/* Pass 2: offsets has nq + 1 entries (exclusive scan of counts); out receives
 * offsets[nq] records, row i in reference traversal order, or ascending by
 * distance when sort != 0 (ties in unspecified order, like std::sort). */
int ptk_search_radius_fill(const ptk_tree* tree, const float* queries,
                           uint64_t nq, float radius, float e,
                           const uint64_t* offsets, ptk_neighbor* out,
                           int sort);

/* Device forms.  The count pass keeps the rows it finds in a block of device
 * memory owned by the handle (PTK_RADIUS_CAPTURE_MB, default 16384,
 * 0 = off).  A fill call whose (d_queries, nq, radius, e, stream) repeat the
 * LAST count call on the handle -- the normal sequence -- copies them out
 * instead of searching again; any other fill call searches again.  The
 * contents of d_queries must not change between the two calls (they must not
 * in the two-pass form either: d_offsets would no longer fit). */
int ptk_search_radius_count_device(const ptk_tree* tree, const float* d_queries,
                                   uint64_t nq, float radius, float e,
                                   uint64_t* d_counts, void* stream);
int ptk_search_radius_fill_device(const ptk_tree* tree, const float* d_queries,
                                  uint64_t nq, float radius, float e,
                                  const uint64_t* d_offsets,
                                  ptk_neighbor* d_out, int sort, void* stream);

/* Convenience: both passes + the scan on the device.  offsets (nq + 1, host)
 * is filled; *out is malloc'ed by the library (free with ptk_free). */
int ptk_search_radius(const ptk_tree* tree, const float* queries, uint64_t nq,
                      float radius, float e, int sort, uint64_t* offsets,
                      ptk_neighbor** out);

/* ---- radius search with a radius per query row ------------------------- */

/* ptk_search_radius with `radii`, nq entries: entry i bounds query row i, in the caller's order, whatever order the
 * batch is searched in.  Results contract: row i is, bit for bit, row i of ptk_search_radius on the same
 * batch with radius = radii[i] and e = 1 -- the points the reference's search_radius(q_i, radii[i]) visits with
 * distance < radii[i] (strict: search_visitor.hpp:141), in the reference's traversal order, or with sort != 0 ascending
 * by distance (ties in unspecified order for float32, by index for float64, as the scalar forms).  Exact only: these
 * forms take no e.  radii are in metric units (squared for L2^2).  No row's radius changes another row.
 * Values: 0 gives an empty row; +inf, FLT_MAX / DBL_MAX and subnormal radii are valid per row; a query row with NaN,
 * +-Inf or overflowing coordinates gets what the reference gives it.  The host-buffer forms and the host loop scan
 * `radii`: a NaN or negative entry is PTK_ERR_INVALID, and ptk_last_error names the first such row.  The _device form
 * only enqueues and cannot look: there a row whose radius is NaN or negative is empty -- its count is 0 and the fill
 * writes nothing for it -- every other row is what it would be without that row, and the call returns PTK_OK.
 * Arguments: a null `radii`, `offsets` or `out` with nq > 0 is PTK_ERR_INVALID; the record buffer of the fill pass may be
 * null when offsets[nq] == 0 (as ptk_search_radius_fill; the _device form cannot look at d_offsets and takes d_out as
 * given).
 * Where the device serves them: exactly the handles ptk_search_count_within_radii serves -- dim <= 3, the four
 * non-topological metrics, float32 trees not of the deep stack class, float64 trees of any depth; every other handle is
 * PTK_ERR_UNSUPPORTED with that call's messages (ptk_host_search_radius_radii serves them).
 * The handle's radius capture (ptk_search_radius_count_device / _fill_device) is neither read nor invalidated: a per-row
 * call between a scalar count / fill pair leaves that pair as it is.
 *
 * The two passes of the _device form: the count pass is ptk_search_count_within_radii_device(..., max_count = 0, ...),
 * whose counts[i] is the length of row i; the caller scans the counts into d_offsets (nq + 1 entries, exclusive) and
 * calls the fill pass below with the same d_queries and d_radii, unchanged in between, on the same stream. */
int ptk_search_radius_radii_fill_device(const ptk_tree* tree, const float* d_queries, uint64_t nq, const float* d_radii,
                                        const uint64_t* d_offsets, ptk_neighbor* d_out, int sort, void* stream);
/* Convenience, as ptk_search_radius: the count, the scan and the fill on the device (the radii go up beside the
 * queries).  offsets (nq + 1, host) is filled; *out is malloc'ed by the library (free with ptk_free). */
int ptk_search_radius_radii(const ptk_tree* tree, const float* queries, uint64_t nq, const float* radii, int sort,
                            uint64_t* offsets, ptk_neighbor** out);

/* ---- the radius searches of the tree's own points ------------------------- */

/* The fixed-radius counterpart of ptk_search_knn_self: every tree point's neighbours among the OTHER points, with no
 * query buffer (radius outlier removal, DBSCAN core-point tests, density estimates, normals over a metric
 * neighbourhood).  Results contract.  Let R_i be the reference's search_radius(p_i, r_i) row on the
 * handle's tree and points: exact (no e), the handle's metric, strict acceptance (distance < r_i); r_i is `radius`, or
 * radii[i] when `radii` is not NULL (n_points entries, indexed by ORIGINAL point index; `radius` is then ignored).
 *   Rows.  Row i is R_i with the entry whose index is i removed if there is one (an index occurs at most once in a
 * row); the other entries keep the reference's traversal order, the same indices and distance bits; with sort != 0
 * they ascend by distance (ties: unspecified order for float32, by index for float64).  Coincident OTHER points stay in
 * the row at distance 0.  Neither "drop the first entry" (the own point is usually not first: rows are in traversal
 * order) nor "the count minus one" (on a tree read from a stream that does not belong to its points a point is often
 * absent from its own row) is this function.
 *   Counts.  counts[i] is the length of row i; with max_count > 0, min(that length, max_count): the clamp applies
 * AFTER the own entry has left.
 *   Ordering.  Rows and counts are indexed by original point index: n_points rows, offsets has n_points + 1 entries.
 *   Radius values.  0 gives empty rows; +inf, FLT_MAX / DBL_MAX and subnormal radii are valid.  A NaN or negative scalar
 * radius is PTK_ERR_INVALID.  A NaN or negative radii entry is PTK_ERR_INVALID in the host-buffer forms and the host
 * loops (the message names the first such row); in the _device forms such a row is empty -- count 0, the fill writes
 * nothing for it -- and every other row is unaffected.
 *   Non-finite points (a handle read from a stream may hold some): such a point's row is whatever the reference gives
 * it, and it changes no other row.
 *   State.  The handle's radius capture (ptk_search_radius_count_device / _fill_device) is neither read nor
 * invalidated.  The first call builds the handle's count side table if it has none, as ptk_search_count_within does.
 * Where the device serves them: exactly the handles ptk_search_count_within_radii serves -- dim <= 3, the four
 * non-topological metrics, float32 trees not of the deep stack class, float64 trees of any depth.  Every other handle
 * is PTK_ERR_UNSUPPORTED; the message names the reason and the host loop that serves it (ptk_host_search_count_within_self
 * / ptk_host_search_radius_self: every float32 handle, the topological metrics included).  There is no staged route.
 * A null output with n_points > 0 is PTK_ERR_INVALID, a host-only handle PTK_ERR_DEVICE.
 * The _device forms only enqueue on `stream`: they allocate nothing and do not wait, except for the first build of the
 * side table.  The count pass that belongs to ptk_search_radius_self_fill_device is ptk_search_count_within_self_device
 * with max_count = 0: the caller scans its counts into d_offsets (n_points + 1 entries, exclusive) and calls the fill
 * with the same radius / d_radii on the same stream.  ptk_search_radius_self: offsets (n_points + 1, host) is filled,
 * *out is malloc'ed by the library (free with ptk_free). */
int ptk_search_count_within_self(const ptk_tree* tree, float radius, const float* radii, uint64_t max_count,
                                 uint64_t* counts);
int ptk_search_count_within_self_device(const ptk_tree* tree, float radius, const float* d_radii, uint64_t max_count,
                                        uint64_t* d_counts, void* stream);
int ptk_search_radius_self(const ptk_tree* tree, float radius, const float* radii, int sort, uint64_t* offsets,
                           ptk_neighbor** out);
int ptk_search_radius_self_fill_device(const ptk_tree* tree, float radius, const float* d_radii, const uint64_t* d_offsets,
                                       ptk_neighbor* d_out, int sort, void* stream);

/* ---- cluster_within_self: the clusters of a tree's own points ------------------------------------------------------
 * The connected components of the fixed-radius graph over the tree's points -- Euclidean cluster extraction -- with
 * DBSCAN's core-point rule when min_neighbors > 0.  No rows are written: the pairs the self radius search visits are
 * linked on the device.
 *   Inputs.  `radius`, or `radii` (n_points entries by ORIGINAL point index; non-NULL: `radius` is ignored), as
 * ptk_search_count_within_self takes them; min_neighbors >= 0.  Let row i be row i of ptk_search_radius_self on the same
 * handle with the same radius or radii (exact, strict <, the handle's metric, the own entry removed).
 *   Core.  Point i is core iff row i has at least min_neighbors entries.  min_neighbors = 0 makes every point core: plain
 * connected components.  DBSCAN's min_samples counts the point itself: min_samples = min_neighbors + 1.
 *   Edges.  Core points i and j are joined whenever j is in row i OR i is in row j: one direction suffices.  (On an
 * ordinary tree with one radius the rows are symmetric; with per-point radii, or on a tree read from a stream that does
 * not belong to its points, they are not.)
 *   Labels (int32, n_points entries by original point index).  A core point's label is the smallest original index among
 * the core points of its component.  A non-core point's label is the smallest label among the core points in ITS OWN
 * row, -1 (noise) if that row holds no core point; a non-core point never passes a label on.  Nothing depends on launch
 * order, lane order or the number of pieces: two calls give identical arrays.  n_clusters (host forms; may be NULL) is
 * the number of i with labels[i] == i.
 *   Radius values, as in the self radius searches.  0 gives empty rows: with min_neighbors = 0 every point is its own
 * cluster (labels[i] = i), with min_neighbors >= 1 everything is -1.  +inf, FLT_MAX / DBL_MAX and subnormal radii are
 * valid.  A NaN or negative scalar is PTK_ERR_INVALID.  A NaN or negative radii entry is PTK_ERR_INVALID in the
 * host-buffer forms and the host loop (the message names the first such row); in the _device forms such a row is empty:
 * the point is its own cluster if min_neighbors = 0, otherwise non-core, and it can still be another point's neighbour.
 *   Where the device serves it: exactly the handles ptk_search_count_within_self serves, refused through the same check
 * with the same messages, naming ptk_host_cluster_within_self (every float32 handle, the topological metrics
 * included).  There is no staged route.  A host-only handle is PTK_ERR_DEVICE, a null labels with n_points > 0
 * PTK_ERR_INVALID.
 *   State.  The handle's radius capture is neither read nor invalidated.  The first call with min_neighbors > 0 builds
 * the handle's count side table if it has none.  The _device forms otherwise only enqueue on `stream`: they allocate
 * nothing, do not wait, and need no scratch beyond d_labels (the float64 form takes the handle's stack block, which
 * grows on first use).  In the host form only the radii go up and the labels come down. */
int ptk_cluster_within_self(const ptk_tree* tree, float radius, const float* radii, uint64_t min_neighbors,
                            int32_t* labels, uint64_t* n_clusters);
int ptk_cluster_within_self_device(const ptk_tree* tree, float radius, const float* d_radii, uint64_t min_neighbors,
                                   int32_t* d_labels, void* stream);

/* ---- suppress_within_self: greedy radius suppression of a tree's own points ------------------------------------------
 * Thins the tree's points to an r-separated subset (Poisson-disk / "spatial" subsampling) or, with scores, keeps the
 * points whose score is a local maximum within r (greedy non-maximum suppression).  No rows are written: a traversal of
 * each point's own radius row looks at one cell per hit, in rounds, on the device.
 *   Inputs.  `radius`, or `radii` (n_points entries by ORIGINAL point index; non-NULL: `radius` is ignored), as
 * ptk_search_count_within_self takes them.  Let row i be row i of ptk_search_radius_self on the same handle with the same
 * radius or radii: the other points j with distance(i, j) < radius_i (exact, strict <, the handle's metric and its unit:
 * squared under metric_l2_squared, the own entry removed).  `scores`: NULL, or n_points float32 entries by original
 * point index (float32 for float64 trees too: the key has 32 bits for them).
 *   Keys.  key(i) = ((uint64_t)ord_i << 32) | (0xFFFFFFFF - i).  With scores, ord_i is the total-order map of the bits b
 * of scores[i]: b ^ 0xFFFFFFFF if the sign bit of b is set, else b ^ 0x80000000 -- a higher score gives a higher key, an
 * equal score is decided by the LOWER index, -0.0 lies below +0.0, +-inf are ordinary values.  With scores == NULL,
 * ord_i = fmix32(i), the 32-bit finaliser
 *     h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16;
 * a bijection of the 32-bit integers: the order is a fixed pseudo-random permutation of the indices.  Keys are distinct
 * in both cases.  (Why hashed and not the index order: the rounds below need a dozen rounds in a hashed order on any
 * cloud measured, and hundreds in index order on a cloud sorted along an axis -- which is how a LiDAR scan arrives.)
 *   Result.  keep (uint8, n_points entries by original point index): keep[i] = 1 iff row i holds no j with
 * key(j) > key(i) and keep[j] == 1; else 0.  This is well-founded by descending key -- it is the greedy pass over the
 * points in key order -- and reads only the point's OWN row, so it stays defined for per-point radii and for rows that
 * are not symmetric.  Nothing depends on launch order, lane order or the number of pieces: two calls give identical
 * arrays.  n_kept (host forms; may be NULL) is the number of i with keep[i] == 1.  What follows:
 *   - Separation.  With a scalar radius under metric_l2_squared or metric_l1 the kept set is a maximal r-separated
 *     subset: no two kept points are closer than r, and every suppressed point has a kept one closer than r.
 *   - Piles.  Of a pile of coincident points exactly one is kept, for any r > 0: the one of highest key.  (Precisely:
 *     at most one, and exactly one unless a kept point OUTSIDE the pile, of higher key still, lies within r of it --
 *     that point then suppresses the whole pile.)
 *   - Radius 0 keeps everything.
 *   Values, as in the self radius searches.  +inf, FLT_MAX / DBL_MAX and subnormal radii are valid.  A NaN or negative
 * scalar radius is PTK_ERR_INVALID.  A NaN or negative radii entry, or a NaN score, is PTK_ERR_INVALID in the
 * host-buffer forms and the host loop (the message names the first such row); the _device forms cannot look: there such
 * a radius gives an empty row -- the point is kept, and it can still suppress others through THEIR rows -- and a NaN
 * score takes the place its bits give it under ord.  A null keep with n_points > 0 is PTK_ERR_INVALID, a host-only handle
 * PTK_ERR_DEVICE; n_points == 0 succeeds.
 *   Where the device serves it: exactly the handles ptk_search_count_within_self serves, refused through the same check
 * with the same messages, naming ptk_host_suppress_within_self (every float32 handle, the topological metrics
 * included).  There is no staged route.
 *   Rounds.  The cells of keep hold a third state, "undecided", while the call runs.  A round walks the row of every
 * undecided point: a kept point of higher key in it suppresses the point, an undecided one blocks it until the next
 * round, otherwise it is kept.  The rounds end when one leaves nothing undecided.  Every round decides at least the
 * undecided point of highest key (all cells above it were final before the launch), so there are at most n_points
 * rounds -- reached by n collinear points at spacing 1 with radius 1.5 (squared: 2.25) whose keys descend along the line:
 * point k waits for point k - 1.  The default order needs about a dozen.  n_rounds (may be NULL) is information only:
 * the rounds launched; it is no part of the results contract and may differ between two calls.
 *   State and waiting.  The handle's radius capture is neither read nor invalidated; no side table is built.  UNLIKE THE
 * OTHER _device FORMS this one WAITS on `stream` once per round and reads 4 bytes back.  It waits on that stream only:
 * the 4-byte counter of the call and its page-locked twin come from a pool the library keeps per device and go back to
 * it (nothing is freed, so nothing waits for the device; the first calls on a device allocate).  It cannot be captured
 * into a graph: a `stream` that is being captured is PTK_ERR_INVALID, by name, before anything is enqueued.  d_keep is
 * the only working array.  The float64 form takes the handle's stack block (it grows on first use) and holds the
 * handle's lock from its first round to its last wait: another thread's float64 search of the SAME handle stands behind
 * the whole call, not behind one launch.  In the host form the radii and scores go up, keep comes down. */
int ptk_suppress_within_self(const ptk_tree* tree, float radius, const float* radii, const float* scores, uint8_t* keep,
                             uint64_t* n_kept, uint32_t* n_rounds);
int ptk_suppress_within_self_device(const ptk_tree* tree, float radius, const float* d_radii, const float* d_scores,
                                    uint8_t* d_keep, uint32_t* n_rounds, void* stream);

/* ---- spacing_knn_self: k-NN spacing and statistical outlier removal of a tree's own points ---------------------------
 * The mean and the k-th of each point's k nearest-neighbour distances, their global mean and sample variance, and the
 * keep mask of statistical outlier removal (PCL's StatisticalOutlierRemoval, Open3D's remove_statistical_outlier),
 * without the rows of ptk_search_knn_self: 4-8 bytes are stored per point instead of 8 k.
 *   Rows.  Row i is ptk_search_knn_self(tree, k)'s row i: k records, the own entry removed by that call's rule, pad
 * {-1, FLT_MAX} (DBL_MAX for a float64 tree).  `Real` is the tree's scalar type.  Every operation below is one IEEE
 * operation of that width, rounded once, in the order written (the units that state it are compiled with
 * -ffp-contract=off; the one statement is pico_tree/internal/spacing.hpp).
 *   Per point.
 *   - m_i = the number of entries of row i whose distance is < FLT_MAX (DBL_MAX).  They are the first m_i entries.
 *   - d_j = the distance of entry j.  With flag PTK_SPACING_SQRT, d_j = sqrt(distance_j) (correctly rounded).
 *   - s_i = ((...((+0 + d_0) + d_1) ...) + d_{m_i-1}), in rank order.
 *   - mean_i = s_i / (Real)m_i.
 *   - kth_i = d_{m_i-1}.
 *   - If m_i == 0: mean_i = kth_i = FLT_MAX (DBL_MAX).
 * The flag turns metric_l2_squared / metric_se2_squared distances into lengths.  The other metrics are called without it.
 *   Validity.
 *   - valid_i = m_i > 0 && mean_i - mean_i == 0 (finite).
 *   - x_i = valid_i ? (double)mean_i : +0.
 *   Statistics.  Record ptk_spacing_stats is 64 bytes:
 *       uint64 count, rows;
 *       double sum, mean, ssd, variance, ratio_squared, reserved;   // reserved = +0
 *   - rows = n_points; count = #valid.
 *   - sum is the value of align_step's summation tree over x_0 ... x_{n-1} in original index order.  That tree is defined
 *     in pico_tree/internal/align.hpp: blocks of 256 entries, align_lane_fold, the butterfly, align_upper_levels.
 *   - mean = count > 0 ? sum / (double)count : +0.
 *   - ssd is the same tree over valid_i ? (x_i - mean) * (x_i - mean) : +0.
 *   - variance = count > 1 ? ssd / (double)(count - 1) : +0.  This is the sample variance, as PCL and Open3D use.
 *   - ratio_squared = (double)ratio * (double)ratio.
 * No square root enters the record or the decision.
 *   Keep.  With e = x_i - mean:
 *       keep[i] = valid_i && (e <= 0.0 || e * e <= ratio_squared * variance), as uint8 0/1.
 * This is PCL's "inlier iff mean distance <= mu + ratio * sigma", stated on squares so that host and device need only
 * + - * /.  `ratio` must be finite and >= 0 whenever keep or stats is asked for; otherwise PTK_ERR_INVALID.
 *   Arguments.  mean (n_points entries of Real by original index) is required; kth (likewise), keep (n_points uint8) and
 * stats (one record) may each be NULL.  A flag bit other than PTK_SPACING_SQRT is PTK_ERR_INVALID; the other checks are
 * ptk_search_knn_self's (k == 0, a null mean with n_points > 0: PTK_ERR_INVALID; a host-only handle: PTK_ERR_DEVICE).
 * With both keep and stats NULL no reduction runs and no workspace is needed (d_workspace may be NULL, workspace_bytes
 * 0).  Otherwise the workspace holds a record and the partials of the summation tree's levels (16 bytes per 256 points
 * and level): ptk_spacing_knn_self_workspace says how many bytes; a null workspace or one smaller than that is
 * PTK_ERR_INVALID (the message gives both sizes).
 *   Routes, as ptk_search_knn_self (ptk_debug_self_route): 1 = the direct kernel, whose lanes reduce their register list
 * as it leaves -- the device form only enqueues on `stream`: no allocation, no wait, and it can be captured --; 2 = the
 * staged route (dim > 3, the topological metrics, trees deeper than 1 031 levels, k >= 64, every float64 tree): pieces of
 * the tree's points go through the handle's k-NN search with k + 1 and one lane per row reduces them.  That route
 * ALLOCATES a block per call and WAITS for `stream` before the reduction is enqueued; it must not be called under a
 * stream capture.  A refusal of the underlying search is passed on unchanged; ptk_host_spacing_knn_self serves every
 * float32 handle.  The statistics and the mask run on `stream` in either route, with no host read-back: a level-0 kernel
 * over mean[] and the upper levels of the tree, a one-lane finish (count, rows, sum, mean), the same for the squared
 * deviations (ssd, variance, ratio_squared, reserved), an elementwise keep kernel.  Plain vector stores throughout.
 *   State.  The handle's radius capture and side tables are neither read nor invalidated.  The host forms upload
 * nothing; they allocate one block per call for the outputs and the workspace and copy the outputs that were asked for
 * back. */
#define PTK_SPACING_SQRT 1u
typedef struct ptk_spacing_stats {
  uint64_t count;        /* valid points */
  uint64_t rows;         /* n_points */
  double sum, mean, ssd, variance, ratio_squared, reserved;
} ptk_spacing_stats; /* 64 bytes */
int ptk_spacing_knn_self(const ptk_tree* tree, uint32_t k, uint32_t flags, float ratio, float* mean, float* kth,
                         uint8_t* keep, ptk_spacing_stats* stats);
int ptk_spacing_knn_self_device(const ptk_tree* tree, uint32_t k, uint32_t flags, float ratio, float* d_mean, float* d_kth,
                                uint8_t* d_keep, ptk_spacing_stats* d_stats, void* d_workspace, uint64_t workspace_bytes,
                                void* stream);
int ptk_spacing_knn_self_workspace(const ptk_tree* tree, uint64_t* bytes);

/* ---- mst_within_self: the minimum spanning forest of a tree's own points ----------------------------------------------
 * The minimum spanning forest (MSF) of the fixed-radius graph over the tree's points: cutting its edges at any r' <= r
 * gives exactly the components ptk_cluster_within_self(r', 0) gives -- the single-linkage dendrogram, for all radii at
 * once -- and with the core distances of ptk_spacing_knn_self (kth) it is HDBSCAN's tree under the mutual-reachability
 * weight.  No rows are written: Boruvka rounds of a k = 1 search that ignores the point's own component, on the device.
 *   Inputs.  A float32 handle; a scalar `radius` (there are no per-point radii); `core`: NULL, or n_points float32
 * entries by ORIGINAL point index in the metric's unit (squared under metric_l2_squared: ptk_spacing_knn_self's kth
 * WITHOUT PTK_SPACING_SQRT).
 *   Graph.  Let row i be row i of ptk_search_radius_self(tree, radius): exact, strict <, the handle's metric and unit, the
 * own entry removed.  {i, j} is an edge iff j is in row i or i is in row j (as ptk_cluster_within_self).  Its weight is
 * w = d, the row's distance bits, when core is NULL; otherwise w = max(d, core[i], core[j]) as float32, and the edge
 * exists only if additionally w < radius.
 *   Order.  Edges are ordered by the triple (bits(w), lo, hi), lo = min(i, j), hi = max(i, j).  Weights are non-negative,
 * so the bit order is the value order; the triples are distinct, so the MSF is unique.  Equal distances are decided by
 * this rule only, never by traversal order.
 *   Result.  n_edges = n_points minus the number of components.  An edge record is 12 bytes, ptk_mst_edge
 * {uint32 lo, uint32 hi, float w}; the edge buffer holds n_points - 1 records (n_points <= 1: no edges, the buffer may be
 * NULL).  labels (may be NULL; int32 by original index): the smallest original index of the point's component.  The
 * host-buffer form and the host loop return the edges ASCENDING in that order, so two calls give identical bytes.  THE
 * _device FORM WRITES THE SAME SET IN UNSPECIFIED ORDER (it may differ between two calls) and leaves the count in the
 * first 4 bytes of the workspace (uint32); sort by (bits(w), lo, hi) for the host forms' bytes.
 *   Values.  radius = 0 gives no edges and labels[i] = i.  +inf and FLT_MAX are valid and give the Euclidean MST of a
 * connected cloud; a pair whose distance overflows to inf is no edge (the test is strict <).  A NaN or negative radius
 * is PTK_ERR_INVALID.  A NaN or negative core entry is PTK_ERR_INVALID in the host-buffer form and the host loop (the
 * message names the row); the _device form cannot look: there such a point has no edges.
 *   Where the rows are not symmetric (a tree read from a stream that does not belong to its points) the call still ends,
 * writes a spanning forest of the same components (labels equal ptk_cluster_within_self(radius, 0)'s) and every edge
 * written is an edge of the graph.  MINIMALITY is promised only where the rows are symmetric.
 *   Where the device serves it: float32 handles with dim <= 3 under metric_l2_squared and metric_l1 (the metrics whose box
 * distance is a lower bound of the point distance), not of the deep stack class.  Everything else is
 * PTK_ERR_UNSUPPORTED, naming the reason and ptk_host_mst_within_self, which serves every float32 handle under those two
 * metrics.  A host-only handle is PTK_ERR_DEVICE.
 *   Rounds.  Every point starts as a component.  A round finds every component's minimum edge to another component (a
 * per-branch table of "all of one component" lets the search skip whole subtrees of its own component), links the
 * components in a lock-free union-find, and relabels.  On symmetric rows there are at most ceil(log2 n) + 1 rounds.
 * n_rounds (may be NULL) is information only.
 *   State and waiting, as ptk_suppress_within_self.  The _device form WAITS on `stream` once per round and reads 4 bytes
 * back, with the counter from the library's per-device pool; a `stream` that is being captured is PTK_ERR_INVALID, by
 * name, before anything is enqueued.  The radius capture is neither read nor invalidated; the count side table is built
 * on first use.  Nothing else is allocated: the caller passes d_workspace of at least ptk_mst_within_self_workspace
 * bytes (a shorter one is PTK_ERR_INVALID).  The host form allocates one block per call; core goes up, the edges and
 * labels come down. */
typedef struct ptk_mst_edge {
  uint32_t lo, hi;
  float w;
} ptk_mst_edge; /* 12 bytes */
int ptk_mst_within_self(const ptk_tree* tree, float radius, const float* core, ptk_mst_edge* edges, uint64_t* n_edges,
                        int32_t* labels, uint32_t* n_rounds);
int ptk_mst_within_self_device(const ptk_tree* tree, float radius, const float* d_core, ptk_mst_edge* d_edges,
                               int32_t* d_labels, void* d_workspace, uint64_t workspace_bytes, uint64_t* n_edges,
                               uint32_t* n_rounds, void* stream);
int ptk_mst_within_self_workspace(const ptk_tree* tree, uint64_t* bytes);

/* ---- normals_within_self: PCA normals and curvature of a tree's own points ------------------------------------------
 * The moments of each point's neighbourhood, their covariance, and the local frame of it (surface normal, curvature,
 * eigenvalues), accumulated inside the traversal of the self radius search: no rows are written.  float32 trees with
 * dim == 3 and the four non-topological metrics.  Contract:
 *   Inputs.  `radius`, or `radii` (n_points entries by ORIGINAL point index; non-NULL: `radius` is ignored), as
 * ptk_search_count_within_self takes them; min_neighbors; viewpoint (3 floats on the host, or NULL).
 *   Row.  Row i is row i of ptk_search_radius_self on the same handle with the same radius or radii and sort = 0: exact,
 * strict <, the handle's metric, the own entry removed, the reference's traversal order.  Write c for its length and
 * j_1 .. j_c for its indices in order.
 *   Offsets.  u_t = p_i - p_{j_t} per component, a float32 subtraction with the query first.  The point itself always
 * belongs to its neighbourhood with offset 0: it adds nothing to the sums and one to the divisor, m = c + 1, whether or
 * not its record was in the reference's row.
 *   Moments.  Every accumulator starts at +0 and takes the offsets in row order: sum[a] = sum[a] + u_a,
 * outer[ab] = outer[ab] + (u_a * u_b) for ab = xx, xy, xz, yy, yz, zz; every + * - is one IEEE float32 operation, no
 * contraction, no reassociation.  count = c, pad_ = 0.  Moments are defined bit for bit; a non-finite point gives whatever
 * this arithmetic gives.
 *   Covariance.  With M = (float)m: inv = 1 / M, mean_a = sum[a] * inv, C_ab = (outer[ab] * inv) - (mean_a * mean_b).
 *   Frame.  Computed from C by one routine (include/pico_tree/internal/local_frame.hpp) compiled for the device, the host
 * loop and the header-only C++ members: cyclic Jacobi with a FIXED 6 sweeps over the pairs (0,1), (0,2), (1,2), a
 * rotation whose off-diagonal element is exactly 0 skipped, no convergence test; the eigenvalues clamped below at +0 and
 * sorted ascending by the fixed network (0,1), (1,2), (0,1) with a strict > swap (equal values keep their columns);
 * normal = the column of eigenvalues[0] divided by its own length; curvature = l0 / ((l0 + l1) + l2), +0 when that sum is
 * 0.  Only + - * / and sqrtf: the frame is a function of the bits of C.
 *   Sign.  With a viewpoint v the normal is flipped when ((n_x * w_x) + (n_y * w_y)) + (n_z * w_z) < 0, w = v - p_i;
 * without one so that its component of largest magnitude is positive (ties: x, then y, then z).
 *   NaN frames.  normal, curvature and eigenvalues all hold the bits 0x7FC00000 and count = c when
 * c < max(min_neighbors, 2) -- a plane needs three points -- or when any entry of C is not finite.
 *   Radius values, as in the self radius searches: 0 gives empty rows (NaN frames, zero moments); +inf, FLT_MAX and
 * subnormal radii are valid; a NaN or negative scalar is PTK_ERR_INVALID; a NaN or negative radii entry is
 * PTK_ERR_INVALID in the host-buffer form and the host loop (the message names the row), an empty row in the _device
 * form.
 *   Outputs.  frames and moments hold n_points records by original point index; either may be NULL, not both
 * (PTK_ERR_INVALID with n_points > 0).  Device buffers must be 16-byte aligned (the records are written with 16-byte
 * stores).
 *   Refusals.  dim != 3 or a topological metric: PTK_ERR_INVALID from every form, the host loop included (a normal is
 * defined for Euclidean 3-D points).  A tree of the deep stack class: PTK_ERR_UNSUPPORTED naming
 * ptk_host_normals_within_self, which serves it.  A host-only handle: PTK_ERR_DEVICE.
 *   State.  The radius capture is neither read nor invalidated; no side table is needed or built (no shortcut is taken:
 * the order of the sums is part of the contract).  The _device form only enqueues on `stream`: no allocation, no wait,
 * no scratch beyond the outputs; `viewpoint` is read at the call.  Two calls give identical bytes.  In the host form only
 * the radii go up and the records come down. */
typedef struct ptk_moments {
  float sum[3];
  uint32_t count;
  float outer[6]; /* xx, xy, xz, yy, yz, zz */
  uint32_t pad_[2];
} ptk_moments; /* 48 bytes */
typedef struct ptk_frame {
  float normal[3];
  float curvature;
  float eigenvalues[3]; /* ascending */
  uint32_t count;
} ptk_frame; /* 32 bytes */
int ptk_normals_within_self(const ptk_tree* tree, float radius, const float* radii, uint64_t min_neighbors,
                            const float* viewpoint, ptk_frame* frames, ptk_moments* moments);
int ptk_normals_within_self_device(const ptk_tree* tree, float radius, const float* d_radii, uint64_t min_neighbors,
                                   const float* viewpoint /* host, 3 floats, read at the call */, ptk_frame* d_frames,
                                   ptk_moments* d_moments, void* stream);

/* ---- aggregate_within: pool a caller's per-point values over radius neighbourhoods ------------------------------------
 * The sum, minimum or maximum of `values` over every row of the self radius search (aggregate_within_self) or of a query
 * batch (aggregate_within), accumulated inside the traversal: no rows are written.  float32 trees.  Contract (DESIGN.md
 * section 2):
 *   Inputs.  `values`: float32, row-major [n_points, channels], indexed by ORIGINAL point index.  `out`: float32,
 * [n_points, channels] by original point index in the self form, [nq, channels] in the caller's query order in the query
 * form.  `counts`: uint64 per row, may be NULL.  `op`: PTK_AGG_SUM, PTK_AGG_MIN or PTK_AGG_MAX; the self forms may OR in
 * PTK_AGG_INCLUDE_SELF.  `radius`, or `radii` when non-NULL: the self forms take them exactly as
 * ptk_search_count_within_self does (n_points entries by original point index), the query forms as
 * ptk_search_radius_radii does (nq entries), with the scalar used when `radii` is NULL.
 *   Row.  Self form: row i of ptk_search_radius_self on the same handle with the same radius or radii and sort = 0 --
 * exact, strict <, the handle's metric, the own entry removed, the reference's traversal order.  Query form: row i of
 * ptk_search_radius_radii with sort = 0.  Write c for its length and j_1 .. j_c for its indices in order.
 *   Accumulation.  Per channel a, independently, in row order; every operation is one IEEE float32 operation, no
 * contraction, no reassociation:
 *     SUM  acc = +0,    then acc = acc + values[j_t][a]
 *     MAX  acc = -inf,  then acc = (v > acc) ? v : acc      with v = values[j_t][a]
 *     MIN  acc = +inf,  then acc = (v < acc) ? v : acc
 * These formulas define the result for NaN, +-inf and signed zero: a NaN value never replaces an accumulator; of -0 and
 * +0 the first seen stays; a NaN accumulator (INCLUDE_SELF below) stays NaN under MIN and MAX, with its bits.  Which NaN
 * an addition gives (its sign and payload) is the processor's: a SUM is defined bit for bit where it is not NaN.
 *   INCLUDE_SELF (self forms).  The accumulator starts at values[i][a] instead of the identity, whether or not the
 * point's own record was in the reference's row (as normals_within_self treats the own point).  In the query forms the
 * flag is PTK_ERR_INVALID.
 *   Counts.  counts[i] = c, in the self form after the own entry has left; INCLUDE_SELF does not change it.  It equals
 * count_within_self / count_within_radii with max_count = 0.
 *   Empty rows.  Radius 0 gives an empty row; a NaN or negative `radii` entry gives an empty row in the _device forms and
 * is PTK_ERR_INVALID in the host-buffer forms and the host loops (the message names the first such row).  An empty row
 * gives the identity (or the own value with INCLUDE_SELF) and count 0.  Every entry of `out` is written by every call.
 *   Arguments.  channels == 0 or channels > 1024, an unknown op, a null `values` or `out` with rows to write and
 * out == values are PTK_ERR_INVALID.  The buffers must not overlap: channel windows re-read `values` while `out` is being
 * written.  No alignment is required (16-byte aligned `values` and `out` with channels % 4 == 0 take 16-byte loads and
 * stores; the bits are the same).
 *   Handles.  float32 trees only.  The self forms are served exactly where ptk_search_count_within_self serves, the
 * query forms where ptk_search_radius_radii does (dim <= 3, the four non-topological metrics, not the deep stack class),
 * refused by the same checks with the same messages: PTK_ERR_UNSUPPORTED naming ptk_host_aggregate_within_self /
 * ptk_host_aggregate_within, which serve every float32 handle, the topological metrics included.  A host-only handle:
 * PTK_ERR_DEVICE.
 *   State.  The radius capture is neither read nor invalidated; no side table is needed or built (the inside shortcut
 * would change the order of the sums).  The _device forms only enqueue on `stream` and do not wait.  The self form
 * allocates nothing; the query form takes the handle's per-stream scratch and orders the batch exactly as
 * ptk_search_count_within_radii_device does, once per call.  A call with more channels than a lane holds accumulators
 * (8) runs one traversal per window of 8 channels.  Two calls give identical bytes.  In the host-buffer forms the radii,
 * queries and values go up and `out` and `counts` come down. */
enum { PTK_AGG_SUM = 0, PTK_AGG_MIN = 1, PTK_AGG_MAX = 2, PTK_AGG_INCLUDE_SELF = 0x100 };
int ptk_aggregate_within_self(const ptk_tree* tree, float radius, const float* radii, const float* values, uint32_t channels,
                              uint32_t op, float* out, uint64_t* counts);
int ptk_aggregate_within_self_device(const ptk_tree* tree, float radius, const float* d_radii, const float* d_values,
                                     uint32_t channels, uint32_t op, float* d_out, uint64_t* d_counts, void* stream);
int ptk_aggregate_within(const ptk_tree* tree, const float* queries, uint64_t nq, float radius, const float* radii,
                         const float* values, uint32_t channels, uint32_t op, float* out, uint64_t* counts);
int ptk_aggregate_within_device(const ptk_tree* tree, const float* d_queries, uint64_t nq, float radius, const float* d_radii,
                                const float* d_values, uint32_t channels, uint32_t op, float* d_out, uint64_t* d_counts,
                                void* stream);

/* ---- align_step: the normal equations of one ICP iteration --------------------------------------------------------------
 * One call poses the source points, runs the k = 1 search, rejects rows by distance and leaves the double-precision sums
 * of one registration step on the device: from them the rigid motion follows on the host, by an SVD (point-to-point) or a
 * 6 x 6 solve (point-to-plane, with the target's normals).  float32 trees with dim == 3 under metric_l2_squared.  Every
 * operation named below is exactly one IEEE operation of the stated width: no contraction, no reassociation.  Contract
 * (DESIGN.md section 2):
 *   Pose.  q'_a = ((R_a0*q_x + R_a1*q_y) + R_a2*q_z) + t_a in float32, `transform` being 12 host floats, row-major
 * [R|t], read at the call (as `viewpoint` is in ptk_normals_within_self).  transform == NULL: q' = q, no arithmetic.
 *   Row.  Row i is ptk_search_knn(q'_i, k = 1, e = 1) on the handle: the same index, the same distance bits.  `rows`
 * (`d_rows`), when given, receives these nq rows, unfiltered.
 *   Acceptance.  Row i is accepted iff distance < max_distance (strict, as the radius searches) and distance < FLT_MAX.
 * The second test excludes the {0, FLT_MAX} pad and every NaN, infinite or overflowing row.  With normals, the three
 * components of the matched point's normal must be finite as well.  max_distance is in metric units (squared); +inf is
 * valid; NaN or a negative value is PTK_ERR_INVALID.  A rejected row contributes +0.0 to every sum and 0 to `count`.
 *   Terms.  q, p, n: the float32 values q'_i, the matched tree point (the caller's bits) and its normal
 * (target_normals[index], [n_points, 3] by ORIGINAL index), converted to double; double operations from there.
 *     point-to-point (normals NULL)   sum_q[a] <- q_a   sum_p[a] <- p_a   sum_qp[3a+b] <- q_a*p_b
 *                                     sum_qq <- (q_x*q_x + q_y*q_y) + q_z*q_z   sum_pp likewise
 *     point-to-plane                  e_a = q_a - p_a   r = ((e_x*n_x) + (e_y*n_y)) + (e_z*n_z)
 *                                     c_x = (q_y*n_z) - (q_z*n_y)  c_y = (q_z*n_x) - (q_x*n_z)  c_z = (q_x*n_y) - (q_y*n_x)
 *                                     J = (c_x, c_y, c_z, n_x, n_y, n_z)
 *                                     jtj[u <= v] <- J_u*J_v (upper triangle, row-major)   jtr[u] <- J_u*r   sum_rr <- r*r
 *     both                            sum_distance <- (double)distance
 * The sums of the other mode are +0.
 *   Order of the sums.  Each sum is a fixed tree over the caller's row order.  Level 0 cuts the rows into blocks of 256
 * consecutive rows, entries past the end being +0.0.  In a block, lane l (0..63) computes
 * ((((+0.0 + x[l]) + x[l+64]) + x[l+128]) + x[l+192]); then for s = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l+s] for l < s;
 * v[0] is the block's partial.  The partials of a level, in block order, are the entries of the next; levels repeat until
 * one value is left (a batch of one row takes one level).  `count` is an integer sum.  nq == 0 writes all zeros.  The
 * result does not depend on PTK_MAX_BATCH, on the batch order of the search, on the launch geometry or on the form:
 * device form, host form, host loop and kd_tree::align_step give identical bytes, and so do two calls.
 *   Arguments.  A null `out` is PTK_ERR_INVALID; with nq > 0 so are a null queries pointer and, in the device form, a null
 * workspace or one smaller than ptk_align_step_workspace says (the message gives both sizes).
 *   Handles.  dim != 3 or another metric is PTK_ERR_INVALID from every form, the host loop included.  Within those
 * handles the device serves whatever ptk_search_knn_device serves with k = 1 -- piles and the deep stack class included --
 * and passes a refusal of the search on unchanged.  A host-only handle: PTK_ERR_DEVICE.
 *   State.  The device form only enqueues on `stream`.  Its temporaries -- q', the rows when d_rows is NULL, the partials
 * of every level -- live in the caller's workspace; the search takes the handle's per-stream scratch as
 * ptk_search_knn_device does.  The one exception: the first call on a handle builds the inverse of the leaf permutation
 * (uint32 per point, one scatter kernel) and waits for it; the handle keeps it, as it keeps the count side table.  The
 * radius capture is neither read nor invalidated.  d_out is written with plain vector stores.  The host form uploads the
 * queries and the normals and downloads the record and, if asked, the rows. */
typedef struct ptk_align_sums {
  uint64_t count;        /* accepted rows */
  uint64_t rows;         /* nq */
  double sum_distance;   /* sum of (double)row distance over accepted rows */
  /* point-to-point (normals == NULL); all +0 in plane mode */
  double sum_q[3], sum_p[3], sum_qp[9] /* [a*3+b] = sum q_a p_b */, sum_qq, sum_pp;
  /* point-to-plane (normals != NULL); all +0 otherwise */
  double jtj[21] /* upper triangle, row-major */, jtr[6], sum_rr;
} ptk_align_sums; /* 384 bytes */
int ptk_align_step_workspace(const ptk_tree* tree, uint64_t nq, uint64_t* bytes);
int ptk_align_step_device(const ptk_tree* tree, const float* d_queries, uint64_t nq,
                          const float* transform /* host, 12 floats row-major [R|t], or NULL */, float max_distance,
                          const float* d_target_normals /* [n_points,3] by ORIGINAL index, or NULL */,
                          ptk_align_sums* d_out, ptk_neighbor* d_rows /* nq, or NULL */, void* d_workspace,
                          uint64_t workspace_bytes, void* stream);
int ptk_align_step(const ptk_tree* tree, const float* queries, uint64_t nq, const float* transform, float max_distance,
                   const float* target_normals, ptk_align_sums* out, ptk_neighbor* rows);

/* ---- box search (ragged output) --------------------------------------- */
/* mins / maxs: nb x dim.  Row i lists the indices inside [min_i, max_i]
 * (closed), in reference traversal order. */
int ptk_search_box(const ptk_tree* tree, const float* mins, const float* maxs,
                   uint64_t nb, uint64_t* offsets, int32_t** out);
/* Device forms, asynchronous on `stream`, as ptk_search_radius_*_device: the
 * count pass, a scan of the counts by the caller (d_offsets: nb + 1 entries),
 * the fill pass.  d_mins / d_maxs must not change between the two calls. */
int ptk_search_box_count_device(const ptk_tree* tree, const float* d_mins,
                                const float* d_maxs, uint64_t nb,
                                uint64_t* d_counts, void* stream);
int ptk_search_box_fill_device(const ptk_tree* tree, const float* d_mins,
                               const float* d_maxs, uint64_t nb,
                               const uint64_t* d_offsets, int32_t* d_out,
                               void* stream);

void ptk_free(void* p);

/* ---- the host loop for calls the device search refuses ------------------- */
/* A device search may answer PTK_ERR_UNSUPPORTED for a valid tree (a topological tree deeper than the
 * device stack, a dimension beyond the LDS staging of the kernels).  The reference answers every call with a loop
 * of per-query searches over the rows (_pyco_tree/kd_tree.hpp:117-135, :179-200, :245-268); these entry points ARE
 * that loop, on the handle's flat tree and the caller's points (n_points x dim, as given at creation: a handle keeps
 * them on the device only), threads taking 128 rows at a time.  Same rows, same order, same bits as the device
 * search would give.  They are never entered by ptk_search_* themselves -- a missing device or a HIP error stays an
 * error; a wrapper calls them by name after PTK_ERR_UNSUPPORTED, with a warning (pico_tree_amd.KdTree does; the C++
 * batched members loop their own per-query members).  float32 handles. */
int ptk_host_search_knn(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq, uint32_t k,
                        float e, ptk_neighbor* out);
int ptk_host_search_knn_within(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq,
                               uint32_t k, float radius, ptk_neighbor* out);
/* (ptk_search_knn_self as it is written: the loop over the tree's own points with min(k + 1, n_points) entries and the
 * rule; every metric, the topological ones included) */
int ptk_host_search_knn_self(const ptk_tree* tree, const float* points, uint32_t k, ptk_neighbor* out);
int ptk_host_search_count_within(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq,
                                 float radius, uint64_t max_count, uint64_t* counts);
/* (the scalar loops with the row's own radius: radii has nq entries, a NaN or negative one is PTK_ERR_INVALID by its row) */
int ptk_host_search_knn_within_radii(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq,
                                     uint32_t k, const float* radii, ptk_neighbor* out);
int ptk_host_search_count_within_radii(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq,
                                       const float* radii, uint64_t max_count, uint64_t* counts);
int ptk_host_search_radius(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq, float radius,
                           float e, int sort, uint64_t* offsets, ptk_neighbor** out); /* *out: ptk_free */
/* (the loop above with the row's own radius and e = 1: radii as for the other ptk_host_*_radii loops) */
int ptk_host_search_radius_radii(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq,
                                 const float* radii, int sort, uint64_t* offsets, ptk_neighbor** out); /* *out: ptk_free */
/* (ptk_search_count_within_self / ptk_search_radius_self as they are written: the radius search of each of the tree's
 * own points -- `points`, n_points rows --, then the removal of the own entry; every metric, the topological ones
 * included; radii NULL: every point gets `radius`) */
int ptk_host_search_count_within_self(const ptk_tree* tree, const float* points, float radius, const float* radii,
                                      uint64_t max_count, uint64_t* counts);
int ptk_host_search_radius_self(const ptk_tree* tree, const float* points, float radius, const float* radii, int sort,
                                uint64_t* offsets, ptk_neighbor** out); /* *out: ptk_free */
/* (ptk_cluster_within_self as the contract reads: the rows of ptk_host_search_radius_self, a sequential union-find over
 * them, then the border rule; every metric, the topological ones included) */
int ptk_host_cluster_within_self(const ptk_tree* tree, const float* points, float radius, const float* radii,
                                 uint64_t min_neighbors, int32_t* labels, uint64_t* n_clusters);
/* (ptk_normals_within_self as the contract reads: the rows of ptk_host_search_radius_self, unsorted, then the moments and
 * the frame of pico_tree/internal/local_frame.hpp; every float32 handle with dim == 3 and a non-topological metric, the
 * deep stack class included; dim != 3 or a topological metric is PTK_ERR_INVALID) */
int ptk_host_normals_within_self(const ptk_tree* tree, const float* points, float radius, const float* radii,
                                 uint64_t min_neighbors, const float* viewpoint, ptk_frame* frames, ptk_moments* moments);
/* (ptk_aggregate_within_self / ptk_aggregate_within as the contract reads: the rows of ptk_host_search_radius_self /
 * ptk_host_search_radius_radii, unsorted, folded with the formulas verbatim; every float32 handle, the deep stack class
 * and the topological metrics included) */
int ptk_host_aggregate_within_self(const ptk_tree* tree, const float* points, float radius, const float* radii,
                                   const float* values, uint32_t channels, uint32_t op, float* out, uint64_t* counts);
int ptk_host_aggregate_within(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq, float radius,
                              const float* radii, const float* values, uint32_t channels, uint32_t op, float* out,
                              uint64_t* counts);
/* (ptk_align_step as the contract reads: the pose on the host, the rows of ptk_host_search_knn with k = 1, then the terms
 * and the summation tree of pico_tree/internal/align.hpp; dim != 3 or another metric than metric_l2_squared is
 * PTK_ERR_INVALID; the deep stack class included) */
int ptk_host_align_step(const ptk_tree* tree, const float* points, const float* queries, uint64_t nq, const float* transform,
                        float max_distance, const float* target_normals, ptk_align_sums* out, ptk_neighbor* rows);
/* (ptk_suppress_within_self as the contract reads: the rows of ptk_host_search_radius_self, a sort by key, one greedy
 * pass in descending key; every metric, the topological ones included) */
int ptk_host_suppress_within_self(const ptk_tree* tree, const float* points, float radius, const float* radii,
                                  const float* scores, uint8_t* keep, uint64_t* n_kept);
/* (ptk_spacing_knn_self as the contract reads: the rows of ptk_host_search_knn_self reduced one by one, the record and
 * the mask from the means; every metric, the topological ones included) */
int ptk_host_spacing_knn_self(const ptk_tree* tree, const float* points, uint32_t k, uint32_t flags, float ratio,
                              float* mean, float* kth, uint8_t* keep, ptk_spacing_stats* stats);
/* (ptk_mst_within_self as the contract reads: the rows of ptk_host_search_radius_self, the edges sorted by
 * (bits(w), lo, hi), Kruskal with a union-find; every float32 handle under metric_l2_squared and metric_l1, any dim, the
 * deep stack class included; another metric is PTK_ERR_UNSUPPORTED.  It keeps every row at once: memory grows with the
 * rows) */
int ptk_host_mst_within_self(const ptk_tree* tree, const float* points, float radius, const float* core,
                             ptk_mst_edge* edges, uint64_t* n_edges, int32_t* labels);
int ptk_host_search_box(const ptk_tree* tree, const float* points, const float* mins, const float* maxs, uint64_t nb,
                        uint64_t* offsets, int32_t** out);                            /* *out: ptk_free */

/* Page-locked host memory for query and result arrays of the host-buffer entry points.  ptk_search_knn copies to
 * and from such arrays directly (no staging through the handle's pinned rings, no first touch of fresh pages per
 * call): a binding that returns a new result array per call -- as _pyco_tree does, def_kd_tree.cpp:73-82 -- keeps a
 * pool of these blocks and hands them out again (pico_tree_amd.KdTree does).  Usable from every device of the node. */
int ptk_host_alloc(uint64_t bytes, void** out);
void ptk_host_free(void* p);
/* Page-locks an array the CALLER owns, in place (hipHostRegister), and releases it again: a query or result array that
 * lives as long as the application -- a ring of scan buffers -- is then moved by ptk_search_* without the staging copy
 * a pageable array needs, exactly like memory from ptk_host_alloc.  The caller must unregister the range before it
 * frees or unmaps it; the library never registers a caller's array on its own (a registration cached by address would
 * outlive the array: an allocator hands the same address out again, and the device would read the old pages). */
int ptk_host_register(void* p, uint64_t bytes);
int ptk_host_unregister(void* p);

/* ---- double precision ---------------------------------------------------- */
/* The reference's kd_tree is generic over the scalar type and its Python module
 * builds KdTree objects over float64 arrays too (dispatch on the array dtype:
 * src/pyco_tree/pico_tree/_pyco_tree/kd_tree.hpp:383-445; neighbor dtype
 * [('index','<i4'),('distance','<f8')], def_core.hpp:17-18).  These entry points
 * are that instantiation: kd_tree<space of double points, metric, int>.  Same
 * meaning, same error behaviour and the same results contract as their float32
 * counterparts above (bit-identical to the reference built over doubles with
 * -ffp-contract=off); the tree file format is the reference's for double
 * scalars (branch records are written as whole structs: 24 bytes). */

/* Layout-identical to pico_tree::neighbor<int, double>: 16 bytes, the distance
 * at offset 8. */
typedef struct ptk_neighbor64 {
  int32_t index;
  int32_t pad_; /* zero */
  double distance;
} ptk_neighbor64;

typedef struct ptk_tree64 ptk_tree64; /* opaque */

int ptk_tree64_create_from_points(const double* points, uint64_t n_points,
                                  uint32_t dim, uint64_t max_leaf_size,
                                  int32_t device, ptk_tree64** out);
int ptk_tree64_create_from_stream(const double* points, uint64_t n_points,
                                  uint32_t dim, const void* stream,
                                  uint64_t stream_bytes, int32_t device,
                                  ptk_tree64** out);
void ptk_tree64_destroy(ptk_tree64* tree);
int ptk_tree64_get_info(const ptk_tree64* tree, ptk_tree_info* info);
/* Any PTK_METRIC_* value.  The two topological metrics -- kd_tree<space of double points, metric_so2 |
 * metric_se2_squared> (metric.hpp:186-257), searched as search_nearest_topological does
 * (internal/kd_tree_search.hpp:115-229) -- need dim 1 / dim 3 and the four bounds per branch: a tree made by
 * ptk_tree64_create_from_points or ptk_tree64_create_from_topological_stream has them, one read from a plain
 * stream does not (PTK_ERR_INVALID). */
int ptk_tree64_set_metric(ptk_tree64* tree, int metric);
int ptk_tree64_serialize(const ptk_tree64* tree, void* buf, uint64_t cap,
                         uint64_t* size);
/* As ptk_tree_serialize_topological / ptk_tree_create_from_topological_stream: the stream kd_tree<topological
 * space of double points, ...>::save writes (kd_tree_branch_double records, kd_tree_node.hpp:52-67: 40 bytes). */
int ptk_tree64_serialize_topological(const ptk_tree64* tree, void* buf,
                                     uint64_t cap, uint64_t* size);
int ptk_tree64_create_from_topological_stream(const double* points,
                                              uint64_t n_points, uint32_t dim,
                                              const void* stream,
                                              uint64_t stream_bytes,
                                              int32_t device, ptk_tree64** out);

/* As ptk_search_knn / ptk_search_knn_device. */
int ptk_search64_knn(const ptk_tree64* tree, const double* queries, uint64_t nq,
                     uint32_t k, double e, ptk_neighbor64* out);
int ptk_search64_knn_device(const ptk_tree64* tree, const double* d_queries,
                            uint64_t nq, uint32_t k, double e,
                            ptk_neighbor64* d_out, void* stream);
/* As ptk_search_knn_self / ptk_search_knn_self_device (the pad: {-1, DBL_MAX}).  Every float64 tree takes the staged
 * route: the device form allocates per call and waits for `stream`. */
int ptk_search64_knn_self(const ptk_tree64* tree, uint32_t k, ptk_neighbor64* out);
int ptk_search64_knn_self_device(const ptk_tree64* tree, uint32_t k, ptk_neighbor64* d_out, void* stream);
/* As ptk_search_knn_within / ptk_search_knn_within_device (the pad: {-1, radius} in double). */
int ptk_search64_knn_within(const ptk_tree64* tree, const double* queries, uint64_t nq,
                            uint32_t k, double radius, ptk_neighbor64* out);
int ptk_search64_knn_within_device(const ptk_tree64* tree, const double* d_queries,
                                   uint64_t nq, uint32_t k, double radius,
                                   ptk_neighbor64* d_out, void* stream);
/* As ptk_search_count_within / ptk_search_count_within_device. */
int ptk_search64_count_within(const ptk_tree64* tree, const double* queries, uint64_t nq, double radius,
                              uint64_t max_count, uint64_t* counts);
int ptk_search64_count_within_device(const ptk_tree64* tree, const double* d_queries, uint64_t nq, double radius,
                                     uint64_t max_count, uint64_t* d_counts, void* stream);
/* As ptk_search_knn_within_radii / ptk_search_count_within_radii and their _device forms: radii in double, the pad
 * {-1, radii[i]}; the count form serves dim <= 3 with the four non-topological metrics (float64 trees have no deep
 * stack class) and refuses the rest with PTK_ERR_UNSUPPORTED. */
int ptk_search64_knn_within_radii(const ptk_tree64* tree, const double* queries, uint64_t nq, uint32_t k,
                                  const double* radii, ptk_neighbor64* out);
int ptk_search64_knn_within_radii_device(const ptk_tree64* tree, const double* d_queries, uint64_t nq, uint32_t k,
                                         const double* d_radii, ptk_neighbor64* d_out, void* stream);
int ptk_search64_count_within_radii(const ptk_tree64* tree, const double* queries, uint64_t nq, const double* radii,
                                    uint64_t max_count, uint64_t* counts);
int ptk_search64_count_within_radii_device(const ptk_tree64* tree, const double* d_queries, uint64_t nq,
                                           const double* d_radii, uint64_t max_count, uint64_t* d_counts, void* stream);
/* As ptk_search_radius: *out is malloc'ed by the library (ptk_free).  With
 * sort != 0 rows ascend by distance, equal distances by index. */
int ptk_search64_radius(const ptk_tree64* tree, const double* queries,
                        uint64_t nq, double radius, double e, int sort,
                        uint64_t* offsets, ptk_neighbor64** out);
/* As ptk_search_radius_radii: radii in double; served where ptk_search64_count_within_radii is. */
int ptk_search64_radius_radii(const ptk_tree64* tree, const double* queries, uint64_t nq, const double* radii, int sort,
                              uint64_t* offsets, ptk_neighbor64** out);
/* As ptk_search_count_within_self / _device and ptk_search_radius_self: radii in double, ptk_neighbor64 records.  (The
 * _device form takes the handle's stack block, which grows on first use.) */
int ptk_search64_count_within_self(const ptk_tree64* tree, double radius, const double* radii, uint64_t max_count,
                                   uint64_t* counts);
int ptk_search64_count_within_self_device(const ptk_tree64* tree, double radius, const double* d_radii, uint64_t max_count,
                                          uint64_t* d_counts, void* stream);
int ptk_search64_radius_self(const ptk_tree64* tree, double radius, const double* radii, int sort, uint64_t* offsets,
                             ptk_neighbor64** out);
/* As ptk_cluster_within_self / _device: radii in double. */
int ptk_search64_cluster_within_self(const ptk_tree64* tree, double radius, const double* radii, uint64_t min_neighbors,
                                     int32_t* labels, uint64_t* n_clusters);
int ptk_search64_cluster_within_self_device(const ptk_tree64* tree, double radius, const double* d_radii,
                                            uint64_t min_neighbors, int32_t* d_labels, void* stream);
/* As ptk_suppress_within_self / _device: radii in double, scores in float32. */
int ptk_search64_suppress_within_self(const ptk_tree64* tree, double radius, const double* radii, const float* scores,
                                      uint8_t* keep, uint64_t* n_kept, uint32_t* n_rounds);
int ptk_search64_suppress_within_self_device(const ptk_tree64* tree, double radius, const double* d_radii,
                                             const float* d_scores, uint8_t* d_keep, uint32_t* n_rounds, void* stream);
/* As ptk_spacing_knn_self / _device / _workspace: mean and kth in double, the pad is DBL_MAX.  Every float64 tree takes
 * the staged route. */
int ptk_search64_spacing_knn_self(const ptk_tree64* tree, uint32_t k, uint32_t flags, float ratio, double* mean, double* kth,
                                  uint8_t* keep, ptk_spacing_stats* stats);
int ptk_search64_spacing_knn_self_device(const ptk_tree64* tree, uint32_t k, uint32_t flags, float ratio, double* d_mean,
                                         double* d_kth, uint8_t* d_keep, ptk_spacing_stats* d_stats, void* d_workspace,
                                         uint64_t workspace_bytes, void* stream);
int ptk_search64_spacing_knn_self_workspace(const ptk_tree64* tree, uint64_t* bytes);
/* As ptk_search_box. */
int ptk_search64_box(const ptk_tree64* tree, const double* mins,
                     const double* maxs, uint64_t nb, uint64_t* offsets,
                     int32_t** out);

/* ---- randomised kd-forest (approximate k-NN in high dimensions) -------- */
/* Replaces the per-query loop over pico_tree::kd_forest::search_nearest /
 * search_nn (examples/pico_understory/pico_understory/kd_forest.hpp:70-85, as
 * driven by examples/kd_forest/kd_forest.cpp:60-100): forest_size trees over
 * Householder-reflected copies of the points (internal/rkd_tree_hh_data.hpp),
 * best-bin-first search bounded by max_leaves_visited per tree
 * (internal/kd_tree_priority_search.hpp:48-63), one k-list shared by the trees.
 * Differences from the reference, both deliberate (see ptk_forest.hpp): the
 * k-list is de-duplicated by index and distances are measured in the original
 * space; reflection vectors derive from `seed` instead of std::random_device.
 * Results are approximate by design; quality is recall against the exact
 * kd_tree, not bit-identity with the reference.
 *
 * Limits and contract:
 *  - k <= 64 (PTK_ERR_INVALID beyond) and dim <= 7072 (the query, its
 *    reflection, the queue and the path fill the kernel's 64 KiB of LDS;
 *    PTK_ERR_UNSUPPORTED beyond).
 *  - A tree may be at most 95 levels deep.  The sliding-midpoint split cannot
 *    separate coincident points, so a pile of several hundred coincident points
 *    under a small max_leaf_size (500 copies, leaf 4: 496 levels), or points
 *    that crowd geometrically towards one value, are refused at creation:
 *    PTK_ERR_UNSUPPORTED, the message names the tree and its depth.
 *  - The points must be finite: a NaN or +-Inf coordinate is refused with
 *    PTK_ERR_INVALID, the message names the first offending point (the same
 *    check as ptk_tree_create_from_points, made before the device is looked
 *    up).  A finite point whose reflection overflows (a coordinate near
 *    FLT_MAX) is refused with PTK_ERR_UNSUPPORTED "tree t: point i ...".
 *  - A query row with a NaN or +-Inf coordinate, or one whose distances
 *    overflow (+-FLT_MAX), comes back all padding, {index -1, distance FLT_MAX}
 *    in every slot, and changes no other row of the batch.  Huge finite rows
 *    whose squared distances stay finite get ordinary full rows.
 *  - ptk_forest_get_dropped is cumulative over the life of the handle: every
 *    search call adds what it dropped, nothing resets it. */
typedef struct ptk_forest ptk_forest; /* opaque */

int ptk_forest_create(const float* points, uint64_t n_points, uint32_t dim,
                      uint64_t max_leaf_size, uint32_t forest_size,
                      uint64_t seed, int32_t device, ptk_forest** out);
void ptk_forest_destroy(ptk_forest* forest);

/* Queue entries dropped so far because a query's per-tree queue (1024 nodes) was full: a
 * dropped node is simply never searched (the result stays a valid approximate answer). */
int ptk_forest_get_dropped(const ptk_forest* forest, uint64_t* dropped);

/* The unit reflection vectors in use: forest_size x dim floats. */
int ptk_forest_get_rotations(const ptk_forest* forest, float* out);

/* Host buffers.  out: nq x k, row i ascending; rows with fewer than k distinct
 * points found are padded with {index -1, distance FLT_MAX}.  k <= 64. */
int ptk_forest_search_knn(const ptk_forest* forest, const float* queries,
                          uint64_t nq, uint32_t k, uint64_t max_leaves_visited,
                          ptk_neighbor* out);
/* Device buffers, asynchronous on `stream`. */
int ptk_forest_search_knn_device(const ptk_forest* forest, const float* d_queries,
                                 uint64_t nq, uint32_t k,
                                 uint64_t max_leaves_visited,
                                 ptk_neighbor* d_out, void* stream);

/* ---- several GPUs of one node ------------------------------------------- */
/* One tree replicated on `n_devices` devices of this process (single process, no launcher):
 * SURVEY.md 8(b) "multi-GPU variant takes a device list", 8(e).  What it replaces in the reference
 * is the same OpenMP loop over query rows as ptk_search_knn (_pyco_tree/kd_tree.hpp:117-135) --
 * queries are independent, so a batch is cut into n contiguous row ranges of ceil(nq / n) rows,
 * range r on devices[r]; results land in the caller's row order.
 *   ptk_multi_search_knn / _radius   host buffers: every device moves its own range; no collective.
 *   ptk_multi_search_knn_device      queries and results on devices[0] (BASELINE configs[3]): the
 *                                    ranges and the (index, distance) rows travel over xGMI as
 *                                    grouped ncclSend / ncclRecv pairs; RCCL is loaded on first use
 *                                    (PTK_ERR_DEVICE if it cannot be).  `stream`: a stream of
 *                                    devices[0], or NULL.  Asynchronous like ptk_search_knn_device. */
typedef struct ptk_multi ptk_multi;
int ptk_multi_create_from_points(const float* points, uint64_t n_points, uint32_t dim, uint64_t max_leaf_size,
                                 const int32_t* devices, uint32_t n_devices, ptk_multi** out);
int ptk_multi_create(const ptk_tree_desc* desc, const int32_t* devices, uint32_t n_devices, ptk_multi** out);
void ptk_multi_destroy(ptk_multi* multi);
int ptk_multi_device_count(const ptk_multi* multi);
/* The replica on devices[i] (owned by `multi`): for ptk_tree_set_metric, ptk_profile_*, ... */
int ptk_multi_get_tree(const ptk_multi* multi, uint32_t i, const ptk_tree** tree);
/* ptk_tree_set_metric on every replica.  Handles made by ptk_multi_create_from_points carry the outer
   bounds the topological metrics need; a descriptor (ptk_multi_create) has none, so metric_so2 /
   metric_se2_squared answer PTK_ERR_INVALID there, as ptk_tree_set_metric does. */
int ptk_multi_set_metric(ptk_multi* multi, int metric);
int ptk_multi_search_knn(const ptk_multi* multi, const float* queries, uint64_t nq, uint32_t k, float e,
                         ptk_neighbor* out);
int ptk_multi_search_radius(const ptk_multi* multi, const float* queries, uint64_t nq, float radius, float e, int sort,
                            uint64_t* offsets, ptk_neighbor** out);
int ptk_multi_search_knn_device(ptk_multi* multi, const float* d_queries, uint64_t nq, uint32_t k, float e,
                                ptk_neighbor* d_out, void* stream);

/* ---- measurement ------------------------------------------------------ */
/* When enabled, every internal kernel launch of this handle is bracketed by HIP
 * events recorded on its stream (no host synchronisation at launch time, so it
 * may stay on inside a timed region).  ptk_profile_get waits for the recorded
 * events and returns the accumulated per-kernel elapsed times. */
typedef struct ptk_profile {
  double search_ms;   /* the traversal kernel(s)                               */
  double reorder_ms;  /* Morton keys + sort + permutation                      */
  double other_ms;    /* scans, fills, copies issued by the backend            */
  uint64_t launches;  /* traversal kernel launches accumulated                 */
  uint64_t queries;   /* queries those launches processed                      */
  double search_tail_ms; /* the part of search_ms behind the first traversal kernel of a call: k = 1 -- phase 2,
                            the cooperative search and the replay (search_ms - search_tail_ms = phase 1)   */
} ptk_profile;
int ptk_profile_enable(ptk_tree* tree, int on);
int ptk_profile_get(const ptk_tree* tree, ptk_profile* out, int reset);
/* The same for a caller built against another version of this header: writes the first `size`
 * bytes of the record only (fields are only ever appended to ptk_profile). */
int ptk_profile_get_sized(const ptk_tree* tree, void* out, uint64_t size, int reset);
/* Counters of the last two-phase k = 1 search on the handle's default scratch block (synchronises
 * the device): counts[0] = queries that needed phase 2, [1] = queries phase 2 handed to the
 * cooperative search, [2] = queries that search could not certify (redone by the reference
 * traversal from the root), [3] = queries of the classes dealt across wavefronts. */
int ptk_debug_knn1_counts(const ptk_tree* tree, uint32_t counts[4]);
/* After a k-NN search with 1 < k <= 56 on a 3-D tree (default metric, exact): {queries the general kernel handed to the
 * cooperative search because they had entered more than the cap of far children (ptk_debug_knn_cap), queries that search could not certify
 * and the reference search redid, and why: a pool of subtrees and its spill that overflowed, more equal distances
 * than the second sweep can rank, a box distance above the k-th distance on the way to a neighbour, a k-th distance
 * outside [1e-30, 1e30]; last: queries whose equal distances a second sweep put in the reference's order}.
 * Synchronises the device. */
int ptk_debug_knn_coop_counts(const ptk_tree* tree, uint32_t counts[7]);
/* After a radius count pass on a 3-D tree whose rows are kept as leaf lists: {queries the list pass handed to a
 * wavefront because they had entered more than its cap of far children (ptk_kernels_coopr.hpp), rows that search could
 * not finish and one lane counted again from the root, sorted leaf entries the fill pass will read}.  Zeros when the
 * pass ran uncapped.  Synchronises the device. */
int ptk_debug_radius_coop_counts(const ptk_tree* tree, uint32_t counts[3]);
/* ptk_debug_knn_coop_counts for the double-precision tree: the counters of the last k-NN call that ran capped (exact,
 * dim <= 3, metric_l2_squared / metric_l1, k <= 32, 32 queries or more: ptk_kernels_coop64.hpp; and of the last radius call, which is capped at any size); zeros if none has
 * since the stack block was last re-allocated.  Synchronises the device. */
int ptk_tree64_debug_knn_coop_counts(const ptk_tree64* tree, uint32_t counts[7]);
/* The far children a query of such a search may enter before a wavefront takes it over, for a batch of nq queries
 * (it follows the batch: a capped launch ends with the lanes that ran to their cap; 0 = this search runs uncapped --
 * e != 1, fewer than 32 queries, k outside 2 .. 56), and the entries of the hand-over list of that batch (a query that
 * finds it full goes on in its lane).  No device needed; honours the test hooks knn_cap / knn_cap_min_nq of PTK_TEST_KNOBS. */
int ptk_debug_knn_cap(uint64_t nq, uint32_t k, float e, uint32_t* cap, uint64_t* list_entries);
/* Piles -- subtrees all of whose points are one and the same point (the reference's builder peels one of them off per
 * level, kd_tree_builder.hpp:255-275) -- of this handle's device replica (dim <= 3): out[0] = piles, [1] = points they
 * hold, [2] = depth of the view without them that the k = 1 searches of the default metric traverse (0 piles: the tree
 * itself is searched and [2] is its depth). */
int ptk_debug_piles(const ptk_tree* tree, uint64_t out[3]);
/* The order a batch of nq query rows (device buffer) is searched in: d_perm[i] (device, nq words) = the row that is
 * searched i-th -- a stable sort of the rows by their Morton keys (ptk_debug_key_bits says how the key bits are spread
 * over the axes).  Synchronises the device. */
int ptk_debug_batch_permutation(const ptk_tree* tree, const float* d_queries, uint64_t nq, uint32_t* d_perm);
/* Where the creation of this handle went, in ms: [0] host build of the tree (ptk_tree_create_from_points only),
 * [1] re-encoding for the device and stream checks, [2] upload and the point gather on the device. */
int ptk_debug_create_phases(const ptk_tree* tree, double ms[3]);
/* How the tree of this handle was built: counts[0] = 1 when the partitions of its top levels were made on the device
 * (ptk_tree_create_from_points with 2^18 points or more on a handle with a device), else 0 and *why (a static string,
 * empty otherwise) says what sent the build to the host: "fewer than 2^18 points", "PTK_DEVICE_BUILD=0", "host-only
 * handle", "not built from points" (the stream and descriptor creators), or what the device build stopped at -- a shape
 * it does not take, more than 64 sliding planes in the top levels, the text of a HIP error.  [1] = nodes of more points
 * than this were split on the device, [2] = levels partitioned there, [3] = branches of the top, [4] = subtrees the
 * host's workers built below it, [5] = planes that slid (std::nth_element), [6] = rounds of that call's introselect made
 * on the device, over all slides, [7] = slides whose whole range went to the host's std::nth_element instead.  After a
 * build that went to the host [1] .. [7] say how far the device build had come. */
int ptk_debug_create_route(const ptk_tree* tree, uint64_t counts[8], const char** why);
/* How a batch of nq queries would be ordered on the device: bits[a] = bits of the Morton key spent on axis a (the
 * first three axes; in proportion to how often a root-to-leaf path of this tree splits on each).  Works on handles
 * without a device replica too. */
int ptk_debug_key_bits(const ptk_tree* tree, uint64_t nq, uint32_t bits[3]);
/* What the last search on the handle's default scratch block did with the order of its batch: 0 = taken as it came
 * (small batch, PTK_REORDER_OFF), 1 = sorted on the device, 2 = sampled, found coherent and searched in the caller's
 * order (k = 1 under PTK_REORDER_AUTO; the reference's loop walks the rows as given, _pyco_tree/kd_tree.hpp:128-134). */
int ptk_debug_batch_order(const ptk_tree* tree, int* how);
/* Launches the last pass of a search made on a tree deeper than the private stack classes (1 032 levels or more: the
 * record stacks spill to an HBM block of at most PTK_DEEP_SPILL_MB, the batch runs in pieces of at least 64 queries);
 * 0 if the handle has made no such search. */
int ptk_debug_deep_pieces(const ptk_tree* tree, uint32_t* pieces);
/* Which route ptk_search_knn_self(tree, k) takes: 1 = the direct kernel, 2 = the staged route (see there). */
int ptk_debug_self_route(const ptk_tree* tree, uint32_t k, int* route);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* PTK_H_ */
