// ptk_backend.hip -- host side of libptk.so: the C ABI of include/ptk.h.
//
// Responsibilities: validate arguments, build (optionally) and re-encode the flat
// tree for the device, keep it resident in HBM, order query batches, launch the
// gfx950 kernels of ptk_kernels.hpp, and move results.  There is no CPU search
// path in this file: without a usable device every search entry point fails with
// PTK_ERR_DEVICE.

#include "ptk_families.hpp"
#include "ptk_kernels_lists.hpp"
#include "ptk_piles.hpp"
#include "ptk_build.hpp"
#include "ptk_sort.hpp"
#include "ptk_forest.hpp"
#include "ptk_rows_out.hpp"
#include "ptk_io_parts.hpp"

namespace {

void axis_bits(const ptk_tree* t, int bits, uint32_t b[3]);

// PTK_CREATE_TIMING=1: the phases of a tree creation on stderr (tools/time_build.py).
struct CreateClock {
  bool on;
  double* sink;  // ptk_tree::create_ms (ptk_debug_create_phases), or null
  std::chrono::steady_clock::time_point t0;
  explicit CreateClock(double* phases = nullptr)
      : on(env_int("PTK_CREATE_TIMING", 0) != 0), sink(phases), t0(std::chrono::steady_clock::now()) {}
  // slot: 0 host build, 1 re-encoding for the device (+ stream checks), 2 upload + point gather on the device
  void lap(const char* what, int slot) {
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (sink != nullptr && slot >= 0) sink[slot] += ms;
    if (on) std::fprintf(stderr, "[ptk create] %-28s %8.2f ms\n", what, ms);
    t0 = t1;
  }
};

int analyse(ptk_tree& t) {
  if (t.builder_made) return PTK_OK;
  ptk::TreeStats st;
  std::string err = ptk::analyse_stream(t.dim, t.n_points, t.nodes.data(), t.nodes.size(), st, nullptr);
  if (!err.empty()) return fail(PTK_ERR_INVALID, "%s", err.c_str());
  t.n_leaves = st.n_leaves;
  t.max_leaf_count = st.max_leaf_count;
  t.max_depth = st.max_depth;
  if (t.dim <= 3) {  // how a root-to-leaf path divides space, per axis (weights: points per leaf)
    struct Frame {
      uint32_t right;
      uint32_t cnt[3];
    };
    std::vector<Frame> stack;
    uint32_t cnt[3] = {0, 0, 0};
    double sum[3] = {0, 0, 0};
    for (size_t i = 0; i < t.nodes.size(); ++i) {
      if (!stack.empty() && stack.back().right == i) {
        std::memcpy(cnt, stack.back().cnt, sizeof(cnt));
        stack.pop_back();
      }
      const ptk_node& nd = t.nodes[i];
      if (nd.right == PTK_LEAF) {
        int32_t b, e;
        std::memcpy(&b, &nd.a, 4);
        std::memcpy(&e, &nd.b, 4);
        for (int a = 0; a < 3; ++a) sum[a] += (double)cnt[a] * (e - b);
      } else {
        ++cnt[nd.split_dim];
        Frame f;
        f.right = nd.right;
        std::memcpy(f.cnt, cnt, sizeof(cnt));
        stack.push_back(f);
      }
    }
    for (int a = 0; a < 3; ++a) t.axis_splits[a] = t.n_points ? sum[a] / (double)t.n_points : 0.0;
  }
  return PTK_OK;
}

int upload(ptk_tree& t, const float* points) {
  CreateClock clock(t.create_ms);
  int rc = analyse(t);
  if (rc != PTK_OK) return rc;
  clock.lap("analyse stream", 1);
  if (clock.on && t.dim <= 3)
    std::fprintf(stderr, "[ptk create] splits per root-to-leaf path: x %.2f  y %.2f  z %.2f (depth %u)\n", t.axis_splits[0],
                 t.axis_splits[1], t.axis_splits[2], t.max_depth);
  if (t.dim > 3) {  // any-dimension layout (ptk_kernels_nd.hpp)
    ptk::TreeStats st;
    ptk::EncodedTreeND enc;
    bool unsupported = false;
    std::string err = ptk::encode_tree_nd(t.dim, t.n_points, points, t.nodes.data(), t.nodes.size(),
                                          t.indices.data(), st, enc, unsupported);
    if (!err.empty()) return fail(unsupported ? PTK_ERR_UNSUPPORTED : PTK_ERR_INVALID, "%s", err.c_str());
    const size_t nb = enc.nodes.size() * sizeof(uint4), ab = enc.axes.size() * 4, pb = enc.points.size() * 4,
                 ib = enc.index.size() * 4;
    PTK_HIP(hipMalloc(&t.d_nodes, nb));
    PTK_HIP(hipMalloc(&t.d_axes, ab));
    PTK_HIP(hipMalloc(&t.d_pts, pb));
    PTK_HIP(hipMalloc(&t.d_index, ib));
    PTK_HIP(hipMemcpy(t.d_nodes, enc.nodes.data(), nb, hipMemcpyHostToDevice));
    PTK_HIP(hipMemcpy(t.d_axes, enc.axes.data(), ab, hipMemcpyHostToDevice));
    PTK_HIP(hipMemcpy(t.d_pts, enc.points.data(), pb, hipMemcpyHostToDevice));
    PTK_HIP(hipMemcpy(t.d_index, enc.index.data(), ib, hipMemcpyHostToDevice));
    const size_t rb = enc.ranges.size() * sizeof(ptk::EncRange);
    PTK_HIP(hipMalloc(&t.d_ranges, rb));
    PTK_HIP(hipMemcpy(t.d_ranges, enc.ranges.data(), rb, hipMemcpyHostToDevice));
    t.device_bytes = nb + ab + pb + ib + rb;
    t.dev_nd.nodes = static_cast<const uint4*>(t.d_nodes);
    t.dev_nd.axes = static_cast<const uint32_t*>(t.d_axes);
    t.dev_nd.pts = static_cast<const float*>(t.d_pts);
    t.dev_nd.index = static_cast<const int32_t*>(t.d_index);
    t.dev_nd.root_ref = enc.root_ref;
    t.dev_nd.cbits = enc.cbits;
    t.dev_nd.cmask = (1u << enc.cbits) - 1u;
    t.dev_nd.dim = t.dim;
    t.gpu_layout = true;
    return PTK_OK;
  }
  ptk::TreeStats st;
  ptk::EncodedTree enc;
  bool unsupported = false;
  // Branch records and references on the host; the 16-byte point records are gathered on the
  // device from the raw points and the leaf-order permutation (no host pass over the points).
  static_assert(ptk::kEncLeafAlign == 1, "encode_points_kernel assumes packed leaves");
  std::string err;
  if (t.builder_made) {
    st.n_leaves = t.n_leaves;
    st.max_leaf_count = t.max_leaf_count;
    st.max_depth = t.max_depth;
    err = ptk::encode_tree_of_builder(t.dim, t.n_points, t.nodes.data(), t.nodes.size(), st, enc, unsupported, build_threads());
  } else {
    err = ptk::encode_tree(t.dim, t.n_points, nullptr, t.nodes.data(), t.nodes.size(), t.indices.data(), st, enc, unsupported,
                           /*with_points=*/false);
  }
  if (!err.empty()) return fail(unsupported ? PTK_ERR_UNSUPPORTED : PTK_ERR_INVALID, "%s", err.c_str());
  clock.lap("encode branch records", 1);
  if (!t.builder_made) {
    for (int32_t idx : t.indices)
      if (idx < 0 || (uint64_t)idx >= t.n_points) return fail(PTK_ERR_INVALID, "index out of range in the permutation");
    clock.lap("check permutation", 1);
  }

  static_assert(sizeof(ptk::EncNode) == sizeof(uint4) && sizeof(ptk::EncPoint) == sizeof(float4), "records");
  const size_t n_records = t.n_points + ptk::kEncLeafPad;
  PTK_HIP(hipMalloc(&t.d_nodes, enc.nodes.size() * sizeof(uint4)));
  PTK_HIP(hipMalloc(&t.d_pts, n_records * sizeof(float4)));
  PTK_HIP(hipMemcpy(t.d_nodes, enc.nodes.data(), enc.nodes.size() * sizeof(uint4), hipMemcpyHostToDevice));
  {
    float* d_raw = nullptr;
    int32_t* d_idx = nullptr;
    const size_t raw_bytes = (size_t)t.n_points * t.dim * sizeof(float);
    hipError_t he = hipMalloc((void**)&d_raw, raw_bytes);
    if (he == hipSuccess) he = hipMalloc((void**)&d_idx, t.n_points * sizeof(int32_t));
    if (he == hipSuccess) he = hipMemcpy(d_raw, points, raw_bytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_idx, t.indices.data(), t.n_points * sizeof(int32_t), hipMemcpyHostToDevice);
    if (he == hipSuccess) {
      const uint32_t blocks = (uint32_t)((n_records + ptk::kBlock - 1) / ptk::kBlock);
      hipLaunchKernelGGL(ptk::encode_points_kernel, dim3(blocks), dim3(ptk::kBlock), 0, nullptr, d_raw, t.dim, d_idx,
                         t.n_points, static_cast<float4*>(t.d_pts));
      he = hipDeviceSynchronize();
    }
    if (d_raw) (void)hipFree(d_raw);
    if (d_idx) (void)hipFree(d_idx);
    if (he != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error while encoding the points: %s", hipGetErrorString(he));
  }
  size_t cell_bytes = 0;
  {
    // The coarse grid of occupied cells (ptk::CellTable): about 32 tree points per cell on average, the cell bits
    // spread over the axes like the bits of the order key.
    int cb = 0;
    while ((64ull << cb) <= t.n_points) ++cb;  // floor(log2(n / 32))
    cb = std::min(std::max(cb, 6), 22);
    {
      uint32_t b[3];
      axis_bits(&t, cb, b);
      float lo[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
      for (uint32_t d = 0; d < t.dim && d < 3; ++d) {
        lo[d] = t.root_min[d];
        const float ext = t.root_max[d] - t.root_min[d];
        inv[d] = ext > 0 ? (float)(1u << b[d]) / ext : 0.0f;
      }
      const size_t n_cells = (size_t)1 << (b[0] + b[1] + b[2]);
      cell_bytes = n_cells;
      uint32_t* d_counts = nullptr;
      PTK_HIP(hipMalloc(&t.d_cells, n_cells));
      PTK_HIP(hipMalloc((void**)&d_counts, n_cells * 4));
      {
        const hipError_t he = hipMemsetAsync(d_counts, 0, n_cells * 4, nullptr);
        if (he != hipSuccess) {
          (void)hipFree(d_counts);
          return fail(PTK_ERR_DEVICE, "hipMemsetAsync failed: %s", hipGetErrorString(he));
        }
      }
      const uint32_t blocks = (uint32_t)((t.n_points + ptk::kBlock - 1) / ptk::kBlock);
      hipLaunchKernelGGL(ptk::cell_count_kernel, dim3(blocks), dim3(ptk::kBlock), 0, nullptr,
                         static_cast<const float4*>(t.d_pts), t.n_points, make_float3(lo[0], lo[1], lo[2]),
                         make_float3(inv[0], inv[1], inv[2]), make_uint3(b[0], b[1], b[2]), d_counts);
      hipLaunchKernelGGL(ptk::cell_class_kernel, dim3((uint32_t)((n_cells + ptk::kBlock - 1) / ptk::kBlock)),
                         dim3(ptk::kBlock), 0, nullptr, d_counts, n_cells, static_cast<uint8_t*>(t.d_cells));
      hipError_t he = hipGetLastError();  // (a launch that failed)
      const hipError_t he_sync = hipDeviceSynchronize();
      if (he == hipSuccess) he = he_sync;
      (void)hipFree(d_counts);
      if (he != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error while counting the grid cells: %s", hipGetErrorString(he));
      t.cells.occ = static_cast<const uint8_t*>(t.d_cells);
      t.cells.inv = make_float3(inv[0], inv[1], inv[2]);
      t.cells.bits = make_uint3(b[0], b[1], b[2]);
    }
  }
  clock.lap("upload + gather points", 2);
  PTK_HIP(hipMalloc(&t.d_ranges, enc.ranges.size() * sizeof(ptk::EncRange)));
  PTK_HIP(hipMemcpy(t.d_ranges, enc.ranges.data(), enc.ranges.size() * sizeof(ptk::EncRange), hipMemcpyHostToDevice));
  t.device_bytes = enc.nodes.size() * sizeof(uint4) + n_records * sizeof(float4) +
                   enc.ranges.size() * sizeof(ptk::EncRange) + cell_bytes;
  t.dev.nodes = static_cast<const uint4*>(t.d_nodes);
  t.dev.pts = static_cast<const float4*>(t.d_pts);
  t.dev.root_ref = enc.root_ref;
  t.dev.cbits = enc.cbits;
  t.dev.cmask = (1u << enc.cbits) - 1u;
  t.dev.n_points = (uint32_t)t.n_points;
  t.n_branches = enc.nodes.size();
  t.gpu_layout = true;
  // Piles -- subtrees of one point many times over: the k = 1 search gets a view in which each is a leaf of one point
  // (ptk_piles.hpp).  A tree of points in general position pays one pass over its branch records here.
  if (knob_int("pile_view", 1) != 0) {
    ptk::PileView view;
    ptk::build_pile_view(t.dim, t.n_points, points, t.nodes.data(), t.nodes.size(), t.indices.data(), view, build_threads());
    if (!view.empty()) {
      ptk::TreeStats st1;
      ptk::EncodedTree enc1;
      bool unsup1 = false;
      const std::string err1 = ptk::encode_tree(t.dim, t.n_points, nullptr, view.nodes.data(), view.nodes.size(), t.indices.data(),
                                                st1, enc1, unsup1, /*with_points=*/false, view.single.data(), enc.cbits);
      if (err1.empty()) {
        static_assert(sizeof(ptk::PileRecord) == sizeof(ptk::DevPileRecord) && sizeof(ptk::PileRecord) == 48, "pile records");
        const size_t nb = enc1.nodes.size() * sizeof(uint4), rb = enc1.ranges.size() * sizeof(ptk::EncRange),
                     ob = view.pile_of_point.size() * 4, pb = view.piles.size() * sizeof(ptk::PileRecord);
        PTK_HIP(hipMalloc(&t.d_nodes1, nb));
        PTK_HIP(hipMalloc(&t.d_ranges1, rb));
        PTK_HIP(hipMalloc(&t.d_pile_of_point, ob));
        PTK_HIP(hipMalloc(&t.d_pile_recs, pb));
        PTK_HIP(hipMemcpy(t.d_nodes1, enc1.nodes.data(), nb, hipMemcpyHostToDevice));
        PTK_HIP(hipMemcpy(t.d_ranges1, enc1.ranges.data(), rb, hipMemcpyHostToDevice));
        PTK_HIP(hipMemcpy(t.d_pile_of_point, view.pile_of_point.data(), ob, hipMemcpyHostToDevice));
        PTK_HIP(hipMemcpy(t.d_pile_recs, view.piles.data(), pb, hipMemcpyHostToDevice));
        t.dev1 = t.dev;
        t.dev1.nodes = static_cast<const uint4*>(t.d_nodes1);
        t.dev1.root_ref = enc1.root_ref;
        t.n_piles = (uint32_t)view.piles.size();
        t.pile_points = view.pile_points;
        t.max_depth1 = st1.max_depth;
        t.device_bytes += nb + rb + ob + pb;
      }  // (a view that cannot be encoded is not needed: the full tree serves every search)
      if (clock.on)
        std::fprintf(stderr, "[ptk create] piles: %zu holding %llu points, view of %zu nodes, depth %u%s%s\n", view.piles.size(),
                     (unsigned long long)view.pile_points, view.nodes.size(), st1.max_depth, err1.empty() ? "" : " -- not used: ",
                     err1.c_str());
    }
    clock.lap("pile view", 1);
  }
  return PTK_OK;
}

// The first kernel launch on a device loads libptk's code object for it (~10 MB: 0.17 s on the bench box,
// profiles/r02_notes.txt item 13).  That load can be started ahead of time on a thread of the library -- by
// ptk_warmup(device), or by the first creation for the device -- so that it runs beside whatever the caller does before
// its first tree (reading the points) and beside the host part of that creation.  One load per device and process;
// wait(device) before the first launch of the calling thread.  PTK_EAGER_WARMUP=0: no thread, the first launch loads.
// (A query about devices -- ptk_device_count() -- starts nothing: in a job of one process per GPU every rank counts the
// devices before it picks its own, and none of them wants a context on device 0.)
__global__ void ptk_warm_kernel() {}
struct ProcessWarmup {
  static constexpr int kMaxDevices = 64;
  std::mutex lock;
  std::thread threads[kMaxDevices];
  bool started[kMaxDevices] = {};
  void start(int32_t device) {
    if (device == kDeviceNone) return;
    const char* sw = std::getenv("PTK_EAGER_WARMUP");
    if (sw != nullptr && std::atoi(sw) == 0) return;
    int dev = device;  // (the device the CALLER is on, not the new thread's default)
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return;
    if (dev < 0 || dev >= kMaxDevices) return;
    std::lock_guard<std::mutex> hold(lock);
    if (started[dev]) return;
    started[dev] = true;
    threads[dev] = std::thread([dev] {
      if (hipSetDevice(dev) != hipSuccess) {
        (void)hipGetLastError();
        return;
      }
      hipLaunchKernelGGL(ptk_warm_kernel, dim3(1), dim3(1), 0, nullptr);
      // (one code object per translation unit: each family loads its own)
      ptkf::warm_knn();
      ptkf::warm_radius();
      ptkf::warm_nd();
      ptkf::warm_topo();
      ptkf::warm_count();
      ptkf::warm_f64();
      ptkf::warm_self();
      ptkf::warm_align();
      ptkf::warm_suppress();
      ptkf::warm_mst();
      ptkf::warm_spacing();
      (void)hipDeviceSynchronize();
      (void)hipGetLastError();
    });
  }
  void wait(int32_t device) {
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return;
    if (dev < 0 || dev >= kMaxDevices) return;
    std::lock_guard<std::mutex> hold(lock);
    if (threads[dev].joinable()) threads[dev].join();
  }
  ~ProcessWarmup() {
    for (auto& th : threads)
      if (th.joinable()) th.join();
  }
};
ProcessWarmup g_warmup;

int finish_create(ptk_tree* t, const float* points, int32_t device, ptk_tree** out) {
  if (t->root_min.empty()) {  // start bounds not supplied: bounding box of the points
    t->root_min.assign(t->dim, std::numeric_limits<float>::max());
    t->root_max.assign(t->dim, std::numeric_limits<float>::lowest());
    for (uint64_t i = 0; i < t->n_points; ++i)
      for (uint32_t d = 0; d < t->dim; ++d) {
        const float v = points[i * t->dim + d];
        t->root_min[d] = std::min(t->root_min[d], v);
        t->root_max[d] = std::max(t->root_max[d], v);
      }
  }
  if (device == kDeviceNone) {
    int rc = analyse(*t);
    if (rc != PTK_OK) {
      delete t;
      return rc;
    }
    t->device = kDeviceNone;
    *out = t;
    return PTK_OK;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    delete t;
    return fail(PTK_ERR_DEVICE, "no HIP device is visible");
  }
  int dev = device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev >= count) {
    delete t;
    return fail(PTK_ERR_INVALID, "device %d out of range (%d visible)", dev, count);
  }
  t->device = dev;
  DeviceGuard guard(dev);
  if (!guard.ok) {
    delete t;
    return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", dev);
  }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
      if (prop.multiProcessorCount > 0) t->cus = prop.multiProcessorCount;
      if (prop.maxSharedMemoryPerMultiProcessor > 0) t->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
      const size_t optin = prop.sharedMemPerBlockOptin > 0 ? (size_t)prop.sharedMemPerBlockOptin : (size_t)prop.sharedMemPerBlock;
      if (optin > 0) t->lds_per_block = std::min(optin, t->lds_per_cu);
      t->hbm_bytes = prop.totalGlobalMem;
    } else {
      (void)hipGetLastError();
    }
  }
  int rc = upload(*t, points);
  if (rc != PTK_OK) {
    ptk_tree_destroy(t);
    return rc;
  }
  *out = t;
  return PTK_OK;
}

bool want_reorder(const ptk_tree* t, uint64_t nq) {
  const int mode = t->reorder.load();
  if (mode == PTK_REORDER_ON) return nq > 1;
  if (mode == PTK_REORDER_OFF) return false;
  return nq >= 8192;
}

// Bits of the Morton key the batch is sorted by.  The search only needs neighbouring lanes to walk neighbouring
// leaves: 24 bits -- three 8-bit radix passes -- spread over the axes the way the tree itself divides space
// (axis_bits below) order the batch as well as 30 bits spent evenly do, for one pass less
// (profiles/r02_notes.txt items 18 and 20).  A small batch is thin in space anyway and pays ~35 us per pass in fixed
// costs: 16 bits (two passes) below 1 M queries (one eighth of BASELINE config 2: 0.537 vs 0.560 ms per step; at
// 1.8 M queries the two are equal, at 3.6 M 24 bits win by 6 %; item 29).
int morton_bits(uint64_t nq) { return nq < (1ull << 20) ? 16 : 24; }

// `bits` key bits over the three axes in proportion to how often a root-to-leaf path splits on each (at most 15
// per axis).  A cloud that is flat along one axis -- most of a LiDAR scan is floor -- gets few bits there and finer
// cells in the plane; a uniform cube gets bits / 3 each.
void axis_bits(const ptk_tree* t, int bits, uint32_t b[3]) {
  b[0] = b[1] = b[2] = 0;
  const uint32_t axes = t->dim < 3 ? t->dim : 3;
  double want[3] = {0, 0, 0};
  const double total = t->axis_splits[0] + t->axis_splits[1] + t->axis_splits[2];
  for (uint32_t a = 0; a < axes; ++a) want[a] = total > 0.0 ? bits * t->axis_splits[a] / total : (double)bits / axes;
  for (int given = 0; given < bits; ++given) {  // largest remaining share first
    int best = -1;
    for (uint32_t a = 0; a < axes; ++a)
      if (b[a] < 15 && (best < 0 || want[a] - b[a] > want[best] - b[best])) best = (int)a;
    if (best < 0) break;
    ++b[best];
  }
}

// rocprim switches from the onesweep radix sort to a merge sort below 1 M items by default -- 24 launches
// and 0.16 ms for the 900 k queries of one eighth of BASELINE config 2 (a shard of configs[3]), where three
// onesweep passes take 0.05 ms (profiles/r02_notes.txt item 17).  The limit is lowered to 128 k items.
using MortonSortConfig =
    rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 131072>;

size_t sort_tmp_bytes(uint64_t nq, int bits) {
  size_t tmp_bytes = 0;
  uint32_t* k32 = nullptr;
  (void)rocprim::radix_sort_pairs<MortonSortConfig>(nullptr, tmp_bytes, k32, k32, k32, k32, nq, 0, bits,
                                                    (hipStream_t) nullptr);
  return tmp_bytes + 256;
}

// The library's own radix sort (ptk_sort.hpp): tiles of `tile` items, one wavefront each.  At most 4096 tiles
// (a row of the digit-by-tile histogram is scanned by one wavefront), at least 512 items per tile (256 / 512 / 1024:
// 68 / 58 / 60 us for 900 k queries).
uint32_t sort_tile(uint64_t nq) {
  const uint64_t t = ((nq + 4095) / 4096 + 63) & ~(uint64_t)63;
  return (uint32_t)std::max<uint64_t>(t, (uint64_t)512);
}
uint32_t sort_tiles(uint64_t nq) { return (uint32_t)((nq + sort_tile(nq) - 1) / sort_tile(nq)); }
uint32_t sort_stride(uint64_t nq) { return (sort_tiles(nq) + 3u) & ~3u;  }  // row of the histogram: 16-byte steps
size_t own_sort_bytes(uint64_t nq) {  // (the histogram of whichever form has more tiles)
  const size_t stride = std::max<size_t>(sort_stride(nq), ((nq + ptk::kSortTile - 1) / ptk::kSortTile + 3) & ~(size_t)3);
  return ((size_t)ptk::kRadixBins * stride + ptk::kRadixBins) * 4 + 2 * nq * sizeof(uint2) + 1024;
}

// Which sort orders the batch: the library's own (ptk_sort.hpp) -- its passes with one wavefront per tile below 0.75 M
// rows (six launches and 58 us for a 900 k-query shard against rocprim's ten launches and 96 us), with blocks of eight
// wavefronts on tiles of 4 096 items from there on (reorder ms, one wavefront per tile / blocks / rocprim's onesweep:
// 900 k rows 0.063 / 0.056 / 0.110, 2 M 0.144 / 0.093 / 0.158, 7.2 M 0.319 / 0.192 / 0.275; profiles/r04_notes.txt
// item 13).  PTK_SORT = 0 forces rocprim's, PTK_SORT_BLOCK = 0 / 1 either form of the own.
bool block_sort(uint64_t nq) {
  const int mode = knob_int("sort_block", -1);
  return mode < 0 ? nq >= (3ull << 18) : mode != 0 && nq >= ptk::kSortTile;
}
// The block form on narrow streams (ptk_sort.hpp, batch_order_narrow): the default wherever the block form is; a forced
// sort_block keeps the passes of r04 unless sort_narrow asks too.  Test hook sort_narrow: 0 = the r04 passes, 1 = the
// digit stream, + 2 = packed items into the last pass, + 4 = the key kernel's rows through LDS.
uint32_t narrow_sort(uint64_t nq) {
  if (!block_sort(nq)) return 0u;
  const int mode = knob_int("sort_narrow", knob_int("sort_block", -1) < 0 ? 7 : 0);
  return mode > 0 ? (uint32_t)mode | 1u : 0u;
}
bool own_sort(uint64_t nq) {
  if (nq >= (1ull << 31)) return false;
  return knob_int("sort", 1) != 0;
}

size_t permutation_scratch_bytes(uint64_t nq) { return 4 * (nq * 4) + sort_tmp_bytes(nq, 30) + own_sort_bytes(nq) + 1024; }

// Device-side Morton ordering of a batch: *perm (device, nq uint32, in `scratch`) lists the
// query rows in launch order.
// heavy_first (ptk::kCellsEmptyFirst / kCellsDenseFirst, 0 = plain Morton order): the queries that will be expensive
// -- by the tree's coarse grid of cell occupancies, ptk::CellTable -- go to the front of the order: for the kernels that
// run every query to its end in its lane.
// may_skip: the batch is sampled first (ptk::coherence_sample_kernel: 256 windows of 64 consecutive rows); if it is
// already in a coherent order -- a scan in scan order, a batch the caller sorted -- the kernels of the sort leave at
// their first instruction and phase 1 of the search takes the rows in the caller's order, as the reference does
// (_pyco_tree/kd_tree.hpp:128-134).  The verdict never leaves the device (two words of the workspace): the entry points
// that take device buffers only enqueue, whatever the batch looks like (r04 waited for the verdict on the host).
const uint32_t* sample_batch(const ptk_tree* t, const float* d_q, uint64_t nq, hipStream_t s, Scratch& scratch, int bits,
                             const float3& lo3, const float3& inv3, const uint3& b3) {
  if (nq < 8192) return nullptr;
  uint8_t* d_fail = scratch.take<uint8_t>(ptk::kCoherenceWindows);
  uint32_t* state = scratch.sample_state();
  if (d_fail == nullptr || state == nullptr) return nullptr;
  // 64 neighbours of a sorted batch cover about 2^bits x 64 / nq cells; five more bits of slack (the box of a window is
  // rounded up per axis, and a window may sit across a cell boundary).
  uint32_t lg = 0;
  while ((128ull << lg) <= nq) ++lg;  // floor(log2(nq / 64))
  const uint32_t max_log2 = (uint32_t)std::min(bits, std::max(bits - (int)lg, 0) + 5);
  hipLaunchKernelGGL(ptk::coherence_sample_kernel, dim3(ptk::kCoherenceWindows), dim3(64), 0, s, d_q, t->dim, nq, lo3, inv3,
                     b3, max_log2, d_fail, state);
  return state + 1;
}

int make_permutation(const ptk_tree* t, const float* d_q, uint64_t nq, hipStream_t s, Scratch& scratch,
                     uint32_t** perm, uint32_t heavy_first = 0, bool may_skip = false) {
  *perm = nullptr;
  if (nq >= (1ull << 32)) return fail(PTK_ERR_UNSUPPORTED, "batches of 2^32 or more queries are not supported");
  Timer timer(t, s);
  const int bits = morton_bits(nq);
  size_t tmp_bytes = sort_tmp_bytes(nq, bits);
  uint32_t* keys = scratch.take<uint32_t>(nq);
  uint32_t* keys_out = scratch.take<uint32_t>(nq);
  uint32_t* ids = scratch.take<uint32_t>(nq);
  uint32_t* ids_out = scratch.take<uint32_t>(nq);
  void* tmp = scratch.take<char>(tmp_bytes);
  if (!keys || !keys_out || !ids || !ids_out || !tmp) return fail(PTK_ERR_NOMEM, "scratch block too small");
  uint32_t b[3];
  axis_bits(t, bits, b);
  float lo[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
  for (uint32_t d = 0; d < t->dim && d < 3; ++d) {
    lo[d] = t->root_min[d];
    const float ext = t->root_max[d] - t->root_min[d];
    inv[d] = ext > 0 ? (float)(1u << b[d]) / ext : 0.0f;
  }
  ptk::CellTable cells{};
  if (heavy_first != 0u && t->cells.occ != nullptr) {
    cells = t->cells;
    cells.key_bits = (uint32_t)bits;
    cells.mode = heavy_first;
  }
  // (only the library's own sort can leave early: the batch is sampled only when that sort runs)
  const uint32_t* as_given = may_skip && own_sort(nq)
                                 ? sample_batch(t, d_q, nq, s, scratch, bits, make_float3(lo[0], lo[1], lo[2]),
                                                make_float3(inv[0], inv[1], inv[2]), make_uint3(b[0], b[1], b[2]))
                                 : nullptr;
  scratch.note_verdict(as_given);
  if (own_sort(nq)) {
    // Key + histogram kernel, then per 8-bit pass: scan of the digit-by-tile histogram, stable scatter (and the
    // histogram of the next digit): 3 launches per pass - 1... nothing to clear, no look-back (ptk_sort.hpp).
    // keys -> pairs A -> [pairs B ->] permutation; the arrays of the rocprim path serve (keys | keys_out + ids = A).
    const bool blocks = block_sort(nq);
    const uint32_t tile = blocks ? ptk::kSortTile : sort_tile(nq);
    const uint32_t tiles = blocks ? (uint32_t)((nq + tile - 1) / tile) : sort_tiles(nq);
    const uint32_t stride = blocks ? (tiles + 3u) & ~3u : sort_stride(nq);
    uint32_t* hist = scratch.take<uint32_t>((size_t)ptk::kRadixBins * stride);
    uint32_t* totals = scratch.take<uint32_t>(ptk::kRadixBins);
    uint2* pairs_a = scratch.take<uint2>(nq);
    uint2* pairs_b = bits > 16 ? scratch.take<uint2>(nq) : pairs_a;
    if (!hist || !totals || !pairs_a || !pairs_b) return fail(PTK_ERR_NOMEM, "scratch block too small");
    const float3 lo3 = make_float3(lo[0], lo[1], lo[2]), inv3 = make_float3(inv[0], inv[1], inv[2]);
    const uint3 b3 = make_uint3(b[0], b[1], b[2]);
    const int passes = (bits + 7) / 8;
    const size_t smem = ptk::kRadixBins * 4;
    if (const uint32_t narrow = narrow_sort(nq)) {
      // The same launches on narrow streams: keys -> pairs [-> packed words] -> permutation, and beside every item its
      // next digit as a byte (in keys_out, which only the rocprim path sorts into) for the next histogram.
      uint8_t* digits = reinterpret_cast<uint8_t*>(keys_out);
      const bool staged = (narrow & 4u) != 0u && t->dim == 3 && (reinterpret_cast<uintptr_t>(d_q) & 15u) == 0u;
      const bool pack = (narrow & 2u) != 0u && nq <= (1ull << ptk::kPackedRowBits);
      const void* from = keys;
      uint32_t from_kind = ptk::kItemKeys;
      for (int p = 0; p < passes; ++p) {
        const uint32_t shift = 8u * (uint32_t)p;
        const bool last = p + 1 == passes;
        void* to = last ? (void*)ids_out : from == pairs_a ? (void*)pairs_b : (void*)pairs_a;
        const uint32_t to_kind = last ? ptk::kItemRows : pack && bits - 8 * (p + 1) <= 8 ? ptk::kItemPacked : ptk::kItemPairs;
        if (p > 0)
          hipLaunchKernelGGL((ptk::radix_digit_hist_kernel<>), dim3(tiles), dim3(ptk::kSortBlock), smem, s, digits,
                             (uint32_t)nq, stride, hist, as_given);
        else if (staged)
          hipLaunchKernelGGL((ptk::radix_key_hist_kernel<true>), dim3(tiles), dim3(ptk::kSortBlock), ptk::kSortKeyStagedLds,
                             s, d_q, t->dim, (uint32_t)nq, lo3, inv3, b3, keys, shift, stride, hist, cells, as_given);
        else
          hipLaunchKernelGGL((ptk::radix_key_hist_kernel<false>), dim3(tiles), dim3(ptk::kSortBlock), ptk::kSortKeyLds, s,
                             d_q, t->dim, (uint32_t)nq, lo3, inv3, b3, keys, shift, stride, hist, cells, as_given);
        hipLaunchKernelGGL(ptk::radix_scan_kernel, dim3(ptk::kRadixBins), dim3(64), 0, s, hist, tiles, stride, totals);
#define PTK_NARROW(IN, OUT)                                                                                            \
  case (IN) * 4u + (OUT):                                                                                              \
    hipLaunchKernelGGL((ptk::radix_narrow_scatter_kernel<IN, OUT>), dim3(tiles), dim3(ptk::kSortBlock),                \
                       ptk::kSortScatterLds, s, from, to, last ? nullptr : digits, (uint32_t)nq, shift, stride, hist,  \
                       totals, as_given);                                                                              \
    break
        switch (from_kind * 4u + to_kind) {
          PTK_NARROW(ptk::kItemKeys, ptk::kItemPairs);
          PTK_NARROW(ptk::kItemKeys, ptk::kItemPacked);
          PTK_NARROW(ptk::kItemKeys, ptk::kItemRows);
          PTK_NARROW(ptk::kItemPairs, ptk::kItemPairs);
          PTK_NARROW(ptk::kItemPairs, ptk::kItemPacked);
          PTK_NARROW(ptk::kItemPairs, ptk::kItemRows);
          PTK_NARROW(ptk::kItemPacked, ptk::kItemRows);
          default: return fail(PTK_ERR_UNSUPPORTED, "batch order: no scatter for this pair of item layouts");
        }
#undef PTK_NARROW
        from = to;
        from_kind = to_kind;
      }
      PTK_HIP(hipGetLastError());
      *perm = ids_out;
      scratch.note_order(1);
      timer.stop(1, 0);
      return PTK_OK;
    }
    const uint2* in = nullptr;
    for (int p = 0; p < passes; ++p) {
      const uint32_t shift = 8u * (uint32_t)p;
      const bool first = p == 0, last = p + 1 == passes;
      uint2* out = in == pairs_a ? pairs_b : pairs_a;
      if (blocks && first)
        hipLaunchKernelGGL((ptk::radix_block_hist_kernel<true>), dim3(tiles), dim3(ptk::kSortBlock), smem, s, d_q, t->dim,
                           (uint32_t)nq, lo3, inv3, b3, keys, in, shift, stride, hist, cells, as_given);
      else if (blocks)
        hipLaunchKernelGGL((ptk::radix_block_hist_kernel<false>), dim3(tiles), dim3(ptk::kSortBlock), smem, s, d_q, t->dim,
                           (uint32_t)nq, lo3, inv3, b3, keys, in, shift, stride, hist, ptk::CellTable{}, as_given);
      else if (first)
        hipLaunchKernelGGL((ptk::radix_hist_kernel<true>), dim3(tiles), dim3(64), smem, s, d_q, t->dim, (uint32_t)nq, lo3,
                           inv3, b3, keys, in, shift, tile, stride, hist, cells, as_given);
      else
        hipLaunchKernelGGL((ptk::radix_hist_kernel<false>), dim3(tiles), dim3(64), smem, s, d_q, t->dim, (uint32_t)nq, lo3,
                           inv3, b3, keys, in, shift, tile, stride, hist, ptk::CellTable{}, as_given);
      // (the scan runs whatever the verdict: it reads `tiles` counters of every digit, whatever they hold)
      hipLaunchKernelGGL(ptk::radix_scan_kernel, dim3(ptk::kRadixBins), dim3(64), 0, s, hist, tiles, stride, totals);
#define PTK_SCATTER(F, L)                                                                                              \
  if (blocks)                                                                                                          \
    hipLaunchKernelGGL((ptk::radix_block_scatter_kernel<F, L>), dim3(tiles), dim3(ptk::kSortBlock),                    \
                       ptk::kSortScatterLds, s, keys, in, out, ids_out, (uint32_t)nq, shift, stride, hist, totals,     \
                       as_given);                                                                                      \
  else                                                                                                                 \
    hipLaunchKernelGGL((ptk::radix_scatter_kernel<F, L>), dim3(tiles), dim3(64), smem, s, keys, in, out, ids_out,      \
                       (uint32_t)nq, shift, tile, stride, hist, totals, as_given)
      if (first && last) PTK_SCATTER(true, true);
      else if (first) PTK_SCATTER(true, false);
      else if (last) PTK_SCATTER(false, true);
      else PTK_SCATTER(false, false);
#undef PTK_SCATTER
      in = out;
    }
    PTK_HIP(hipGetLastError());
    *perm = ids_out;
    scratch.note_order(1);
    timer.stop(1, 0);
    return PTK_OK;
  }
  {
    const uint32_t blocks = (uint32_t)((nq + ptk::kBlock - 1) / ptk::kBlock);
    hipLaunchKernelGGL(ptk::morton_kernel, dim3(blocks), dim3(ptk::kBlock), 0, s, d_q, t->dim, nq,
                       make_float3(lo[0], lo[1], lo[2]), make_float3(inv[0], inv[1], inv[2]),
                       make_uint3(b[0], b[1], b[2]), keys, ids, cells, (uint64_t)0);
  }
  PTK_HIP(rocprim::radix_sort_pairs<MortonSortConfig>(tmp, tmp_bytes, keys, keys_out, ids, ids_out, nq, 0, bits, s));
  *perm = ids_out;
  scratch.note_order(1);
  timer.stop(1, 0);
  return PTK_OK;
}

// The launch order of a batch, as every search that takes one asks for it: reserves `extra_bytes` of the caller's own
// plus, where the handle's reorder mode wants the batch sorted (want_reorder), the arrays of the sort, then sorts
// (make_permutation: `heavy_first` and `may_skip` are its).  *perm: the rows in launch order (Morton order along the
// first three axes, whatever the dimension), or nullptr for a batch that is launched as it came.
int order_batch(const ptk_tree* t, const float* d_q, uint64_t nq, hipStream_t s, Scratch& scratch, size_t extra_bytes,
                uint32_t** perm, uint32_t heavy_first = 0, bool may_skip = false) {
  *perm = nullptr;
  const bool reorder = want_reorder(t, nq);
  const int rc = scratch.reserve(extra_bytes + (reorder ? permutation_scratch_bytes(nq) : 0));
  if (rc != PTK_OK || !reorder) return rc;
  return make_permutation(t, d_q, nq, s, scratch, perm, heavy_first, may_skip);
}

// PTK_RADIUS_CAPTURE_MB: the most device memory the captured rows of a radius batch may take
// (default 16384; 0 switches the capture off and every fill pass repeats the traversal).
size_t capture_budget_bytes(const ptk_tree* t) {
  // default: 16 GiB, but no more than a quarter of the device's memory (a partitioned or smaller device)
  const size_t quarter_mb = t->hbm_bytes ? (t->hbm_bytes >> 22) : 16384;
  const int mb = env_int("PTK_RADIUS_CAPTURE_MB", (int)std::min<size_t>(16384, std::max<size_t>(quarter_mb, 64)));
  return mb <= 0 ? 0 : (size_t)mb << 20;
}

// Sizes (and if needed allocates) the capture block for a batch of nq rows; false = no capture.
// Layout: counters | captured flags (one per wavefront) | query of every lane | chunks.  Every wavefront of the
// launch owns one static chunk; the dynamic pool is sized for 1024 hits per row when the budget allows (the
// scan-like cloud of BASELINE config 3 averages 105); PTK_RADIUS_CAPTURE_CHUNKS overrides chunks per sub-pool (tests).
// with_heavy: room for what a capped list pass keeps of its hand-overs until the fill pass (ptk::RadiusHeavy: counters,
// four words per hand-over, the sorted entries), between the tables and the chunks.
bool prepare_capture(const ptk_tree* t, uint64_t nq, Workspace& ws, bool with_heavy = false) {
  const size_t budget = capture_budget_bytes(t);
  if (budget == 0 || nq == 0 || nq >= (1ull << 31)) return false;
  const size_t waves = (size_t)((nq + 63) / 64);
  const size_t chunk_bytes = (size_t)ptk::kLogChunk * sizeof(ptk::Neighbor);
  const size_t flags_at = (size_t)ptk::kCapSubPools * ptk::kCapCounterStride * 4;
  const size_t qids_at = flags_at + ((waves + 255) & ~(size_t)255);
  const size_t lens_at = qids_at + waves * 64 * 4;
  const size_t tables_at = lens_at + waves * 64 * 4;
  const size_t heavy_at = (tables_at + waves * ptk::kListMaxChunks * 4 + 255) & ~(size_t)255;
  const size_t mh = with_heavy ? (size_t)radius_max_handover(nq) : 0, ecap = with_heavy ? (size_t)radius_entry_cap(nq) : 0;
  const size_t heavy_bytes = with_heavy ? 256 + 4 * ((mh * 4 + 255) & ~(size_t)255) + ecap * 8 : 0;
  const size_t head = (heavy_at + heavy_bytes + 4095) & ~(size_t)4095;
  if (head + waves * chunk_bytes > budget) return false;
  const size_t dyn = std::min<size_t>((budget - head - waves * chunk_bytes) / chunk_bytes, waves * 64 * 2);
  const int forced = knob_int("radius_capture_chunks", -1);
  size_t sub_cap = forced >= 0 ? (size_t)forced : dyn / ptk::kCapSubPools;
  // (a slot of the log is addressed with 32 bits)
  const size_t max_chunks = ((1ull << 32) - 1) / ptk::kLogChunk;
  if (waves >= max_chunks) return false;
  if (waves + sub_cap * ptk::kCapSubPools > max_chunks) sub_cap = (max_chunks - waves) / ptk::kCapSubPools;
  const size_t bytes = head + (waves + sub_cap * ptk::kCapSubPools) * chunk_bytes;
  if (bytes > ws.cap_capacity) {
    drain_workspace(ws);
    if (ws.cap_base) (void)hipFree(ws.cap_base);
    ws.cap_base = nullptr;
    ws.cap_capacity = 0;
    ws.cap_valid = false;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 2) return false;
    if (hipMalloc((void**)&ws.cap_base, bytes) != hipSuccess) {
      (void)hipGetLastError();
      ws.cap_base = nullptr;
      return false;
    }
    ws.cap_capacity = bytes;
  }
  ws.cap.counters = reinterpret_cast<uint32_t*>(ws.cap_base);
  ws.cap.captured = reinterpret_cast<uint8_t*>(ws.cap_base + flags_at);
  ws.cap.qids = reinterpret_cast<uint32_t*>(ws.cap_base + qids_at);
  ws.cap.lens = reinterpret_cast<uint32_t*>(ws.cap_base + lens_at);
  ws.cap.tables = reinterpret_cast<uint32_t*>(ws.cap_base + tables_at);
  ws.cap.chunks = reinterpret_cast<ptk::Neighbor*>(ws.cap_base + head);
  ws.cap.n_static = (uint32_t)waves;
  ws.cap.sub_cap = (uint32_t)sub_cap;
  ws.cap_heavy = ptk::RadiusHeavy{};
  if (with_heavy) {
    const size_t row = (mh * 4 + 255) & ~(size_t)255;
    char* p = ws.cap_base + heavy_at;
    ws.cap_heavy.meta = reinterpret_cast<uint32_t*>(p);
    ws.cap_heavy.rows = reinterpret_cast<uint32_t*>(p + 256);
    ws.cap_heavy.own = reinterpret_cast<uint32_t*>(p + 256 + row);
    ws.cap_heavy.run_at = reinterpret_cast<uint32_t*>(p + 256 + 2 * row);
    ws.cap_heavy.run_n = reinterpret_cast<uint32_t*>(p + 256 + 3 * row);
    ws.cap_heavy.entries = reinterpret_cast<unsigned long long*>(p + 256 + 4 * row);
    ws.cap_heavy.max_heavy = (uint32_t)mh;
    ws.cap_heavy.entry_cap = (uint32_t)std::min<size_t>(ecap, 0xFFFFFFFFu);
  }
  return true;
}

// Narrow tiers of phase 2 (cumulative per-mille marks of the ranked classes, lanes per wavefront).  A search that
// runs every query to its end (e != 1: no cap, see phase2_cap) starts the 6 % most expensive continuations four to
// a wavefront: they are the critical path of the launch (profiles/r01e_notes.txt).  With the cap the long chains go
// to the cooperative search and there is no narrow tier.
ptk::TierSpec phase2_tiers(uint32_t cap) {
  ptk::TierSpec t{};
  if (cap == 0) {
    t.permille[0] = 60;
    t.lanes[0] = 4;
  }
  return t;
}

size_t class_sort_tmp_bytes(uint64_t nq) {
  size_t tmp_bytes = 0;
  ptk::ContKey* k16 = nullptr;
  uint32_t* v32 = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, tmp_bytes, k16, k16, v32, v32, nq, 0, 16, (hipStream_t) nullptr);
  return tmp_bytes + 256;
}

// Queries whose unfinished stack phase 2 can hand to the cooperative search (kMaxTasks records
// each); further ones are searched again from the root.
uint64_t max_handover(uint64_t nq) { return std::max<uint64_t>(nq / 32, std::min<uint64_t>(nq, 16384)); }

// The class order as a counting sort (ptk_kernels.hpp, class_scan_kernel / class_order_kernel): phase 1 counts its
// own tile of 64 slots; the rows of counters are scanned in at most kClassMaxSegs segments of a multiple of 1024
// tiles; the scatter takes chunks of `per` slots, one wavefront each (short chains for a small batch).
struct ClassPlan {
  uint32_t ntiles, stride, seg, segs, per, chunks;
};
ClassPlan class_plan(uint64_t nq) {
  ClassPlan p;
  p.ntiles = (uint32_t)((nq + 63) / 64);
  p.stride = (p.ntiles + 3u) & ~3u;
  p.seg = 1024u * std::max<uint32_t>(1u, (p.ntiles + 1024u * ptk::kClassMaxSegs - 1u) / (1024u * ptk::kClassMaxSegs));
  p.segs = (p.ntiles + p.seg - 1u) / p.seg;
  p.per = nq < (2ull << 20) ? 512u : 1792u;
  p.chunks = (uint32_t)((nq + p.per - 1) / p.per);
  return p;
}

// The cooperative search: 16 lanes per query, a pool of 96 subtrees per group (8 / 32 / 64 lanes were measured:
// 1.91 / 1.90 / slower vs 1.72 ms of traversal kernels, profiles/r02_notes.txt items 6, 12).
constexpr int kCoopLanes = 16, kCoopPool = 96;
// Tasks a group of the cooperative search may park in HBM when its LDS pool is full.
constexpr uint32_t kCoopSpill = 256;
inline int coop_waves(const ptk_tree* t) {
  constexpr size_t smem = (size_t)(64 / kCoopLanes) * (6 * kCoopPool + 2) * 4;
  // As many waves as can be resident at once (LDS-bound: CUs x LDS per CU of the device), each group working
  // through its share of the list: a second round of blocks would start when most of the work is done.
  return t->cus * (int)std::max<size_t>(1, std::min<size_t>(24, t->lds_per_cu / (smem + 512)));
}
size_t coop_spill_bytes(const ptk_tree* t) {
  return (size_t)coop_waves(t) * (64 / kCoopLanes) * kCoopSpill * sizeof(ptk::Task);
}

size_t two_phase_scratch_bytes(const ptk_tree* t, uint64_t nq) {
  return nq * sizeof(float4) + nq * ptk::kContSlots * sizeof(ptk::Record) + nq * sizeof(uint4) + 4 * nq +
         2 * (nq * 4) + 3 * (nq * 4) + max_handover(nq) * ptk::kMaxTasks * sizeof(ptk::Task) + 64 + 2 * coop_spill_bytes(t) +
         class_sort_tmp_bytes(nq) + (size_t)ptk::kClassBuckets * (class_plan(nq).stride + ptk::kClassMaxSegs) * 4 + 2048;
}

// Far children a query may enter in phase 2 before it is handed to the cooperative search
// (PTK_P2_CAP; 0 = phase 2 runs every query to its end).  Exact searches only: the argument that
// makes the cooperative result the reference's (ptk_kernels.hpp, knn1_coop_kernel) needs e = 1.
// The cap is a chain length (cap x ~10 us of dependent rounds in the dealt tier): what a big batch hides behind
// its light tier is exposed on a small one, e.g. one shard of BASELINE configs[3] -- 900 k queries: 0.556 ms per
// step with a cap of 8, 0.604 with 16, 0.612 with 4 (profiles/r02_notes.txt items 4, 17).  With the ranked classes
// taken out of phase 2 (coop_direct_mode): 900 k queries 6 / 8 / 12 / 16 = 0.247 / 0.245 / 0.265 / 0.285 ms of traversal
// kernels, 7.2 M queries 8 / 12 / 16 / 24 / 32 = 1.287 / 1.268 / 1.255 / 1.238 / 1.271 (profiles/r03_notes.txt item 3).
uint32_t phase2_cap(float e, uint64_t nq) {
  if (e != 1.0f) return 0;
  const int cap = knob_int("p2_cap", nq >= (4ull << 20) ? 24 : 8);
  // (never above kP2CapMax: what the ring of the capped phase 2 is sized for, ptk_backend_core.hpp)
  return cap < 0 ? 0u : (uint32_t)std::min(cap, kP2CapMax);
}

// direct_ids == nullptr: the list is `ho`'s.  Otherwise it is the ranked head of the class-sorted entries, searched
// straight from the continuation records of phase 1 (knn1_coop_kernel<.., DIRECT>), `lanes` lanes per query.
template <int G, class M = ptk::MetricL2>
int launch_knn1_coop_direct(const ptk_tree* t, const float4* qs, ptk::Neighbor* d_out, const ptk::Cont& cont,
                            const ptk::Handover& ho, uint32_t* redo_list, hipStream_t s, ptk::Task* spill,
                            const uint32_t* direct_ids) {
  constexpr size_t smem = (size_t)(64 / G) * (6 * kCoopPool + 2) * 4;
  // (the spill block is sized for coop_waves(t) x 64 / kCoopLanes groups: a wider group count would not fit)
  static_assert(G >= kCoopLanes, "the spill block is sized for groups of kCoopLanes lanes");
  const int resident = t->cus * (int)std::max<size_t>(1, std::min<size_t>(32, t->lds_per_cu / (smem + 512)));
  const int waves = std::min(resident, coop_waves(t) * (G / kCoopLanes));
  hipLaunchKernelGGL((ptk::knn1_coop_kernel<G, kCoopPool, true, true, M>), dim3(waves), dim3(64), smem, s, knn1_tree(t),
                     knn1_ranges(t), qs, d_out, cont, ho, redo_list, direct_ids, spill, kCoopSpill);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

template <class M = ptk::MetricL2>
int launch_knn1_coop(const ptk_tree* t, const float4* qs, ptk::Neighbor* d_out, const ptk::Cont& cont,
                     const ptk::Handover& ho, uint32_t* redo_list, hipStream_t s, ptk::Task* spill,
                     const uint32_t* direct_ids = nullptr) {
  constexpr size_t smem = (size_t)(64 / kCoopLanes) * (6 * kCoopPool + 2) * 4;
  const int waves = coop_waves(t);
  const uint32_t spill_cap = spill ? kCoopSpill : 0u;
  if (direct_ids != nullptr) {
    // (32 lanes per query: 16 / 64 were measured, 1.91 / slower vs 1.72 ms of traversal kernels, profiles/r03_notes.txt item 3)
    return launch_knn1_coop_direct<32, M>(t, qs, d_out, cont, ho, redo_list, s, spill, direct_ids);
  }
  // What phase 2 hands over has been tightened by its first far children: a pool of 96 holds it (0 of 152 k queries of
  // BASELINE config 2 overflow; with the spill the step loop is 5 % slower): no spill here.
  (void)spill_cap;
  hipLaunchKernelGGL((ptk::knn1_coop_kernel<kCoopLanes, kCoopPool, false, false, M>), dim3(waves), dim3(64), smem, s, knn1_tree(t),
                       knn1_ranges(t), qs, d_out, cont, ho, redo_list, nullptr, spill, 0u);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

// How the ranked classes of an exact k = 1 batch -- 2 % of the queries, every expensive one among them -- are
// searched (PTK_COOP_DIRECT overrides):
//   0  by phase 2 up to the cap like everything else, what is left cooperatively afterwards
//   1  cooperatively straight from phase 1, on the same stream, before phase 2
//   2  the same on a second stream BESIDE phase 2: the capped traversal of such a query and its cooperative search
//      afterwards are two chains of dependent rounds; taken straight from phase 1 it is searched once, while phase 2
//      works on the rest.  Scan-like cloud (profiles/r03_notes.txt item 3): 900 k queries 0.348 -> 0.245 ms of
//      traversal kernels, 7.2 M queries 1.35 -> 1.23 ms.  A uniform cloud has no expensive queries: there the
//      cooperative search of the ranked classes is merely the dearer way (7.2 M queries 1.31 -> 1.35 ms; 900 k queries
//      0.255 -> 0.242 ms all the same, the GPU being mostly idle).
// The sign of a cloud with expensive queries is a tree much deeper than a balanced one (the sliding midpoint peels
// dense regions level by level: scan-like cloud 33 levels for 2^20 leaves, uniform cloud 23).
int coop_direct_mode(const ptk_tree* t, uint64_t nq) {
  uint32_t balanced = 0;
  while ((1ull << balanced) < t->n_leaves) ++balanced;
  const bool deep = t->max_depth >= balanced + 6u;
  return knob_int("coop_direct", deep || nq < (1ull << 20) ? 2 : 0);
}

// The k = 1 search under the default metric (ptk_kernels.hpp, "the two-phase k = 1 search"): phase 1 (which also
// packs the launch-order records), the class order of the continuations, phase 2, and for exact searches the
// cooperative search of what phase 2 handed over plus the replay of what that could not certify.
template <int OVF, class M = ptk::MetricL2>
int launch_knn1_two_phase(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float e,
                          ptk::Neighbor* d_out, hipStream_t s, Scratch& scratch) {
  constexpr int LEAFB = 4;  // points fetched per round trip
  if (nq >= (1ull << 32)) return fail(PTK_ERR_UNSUPPORTED, "batches of 2^32 or more queries are not supported");
  float4* qs = scratch.take<float4>(nq);
  if (qs == nullptr) return fail(PTK_ERR_NOMEM, "scratch block too small");
  ptk::Cont cont{};
  cont.nq = nq;
  size_t tmp_bytes = class_sort_tmp_bytes(nq);
  cont.rec = scratch.take<ptk::Record>(nq * ptk::kContSlots);
  cont.best = scratch.take<uint4>(nq);
  cont.key = scratch.take<ptk::ContKey>(nq);
  ptk::ContKey* key_out = scratch.take<ptk::ContKey>(nq);
  cont.ids = scratch.take<uint32_t>(nq);
  uint32_t* ids_out = scratch.take<uint32_t>(nq);
  cont.meta = scratch.take<uint32_t>(ptk::kMetaWords);
  void* tmp = scratch.take<char>(tmp_bytes);
  if (!cont.rec || !cont.best || !cont.key || !key_out || !cont.ids || !ids_out || !cont.meta || !tmp)
    return fail(PTK_ERR_NOMEM, "scratch block too small");
  ptk::Handover ho{};
  ho.counter = ptk::kMetaHeavy;
  ho.meta = cont.meta;
  ho.heavy_list = scratch.take<uint32_t>(nq);
  ho.ntasks = scratch.take<uint32_t>(nq);
  ho.max_heavy = (uint32_t)max_handover(nq);
  ho.tasks = scratch.take<ptk::Task>((size_t)ho.max_heavy * ptk::kMaxTasks);
  uint32_t* redo_list = scratch.take<uint32_t>(nq);
  if (!ho.heavy_list || !ho.ntasks || !ho.tasks || !redo_list) return fail(PTK_ERR_NOMEM, "scratch block too small");
  // Where the groups of the cooperative search park subtrees their LDS pool has no room for (one block per launch
  // that may be in flight: the direct one on the second stream, the one behind phase 2).
  ptk::Task* spill_a = reinterpret_cast<ptk::Task*>(scratch.take<char>(coop_spill_bytes(t)));
  ptk::Task* spill_b = reinterpret_cast<ptk::Task*>(scratch.take<char>(coop_spill_bytes(t)));
  if (!spill_a || !spill_b) return fail(PTK_ERR_NOMEM, "scratch block too small");
  scratch.note_meta(cont.meta, 1);
  const uint32_t blocks = (uint32_t)((nq + 63) / 64);
  const float e_inv = inv_ratio(e);
  const uint32_t cap = phase2_cap(e, nq);
  uint32_t* const slot_ids = cont.ids;
  if (cap) cont.ids = nullptr;  // phase 1 need not write slot numbers: the counting sort produces them
  // The grid has room for nq / 64 extra waves in the narrow tiers; the meta kernel cuts the tiers to what fits.
  const ptk::TierSpec tiers = phase2_tiers(cap);
  const uint32_t extra_waves = tiers.permille[0] == 0 ? 0u : (uint32_t)(nq / 64) + 2u;
  // The ranked classes straight to the cooperative search (exact searches only), beside phase 2 if a second stream
  // can be had.
  int direct = cap ? coop_direct_mode(t, nq) : 0;
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  if (direct == 2 && !scratch.side_stream(&side, &fork, &join)) direct = 1;
  // Exact searches: phase 1 counts the class buckets of its tile for the counting sort below.
  const ClassPlan cp = class_plan(nq);
  uint32_t* tile_counts = nullptr;
  uint32_t* seg_totals = nullptr;
  if (cap) {
    tile_counts = scratch.take<uint32_t>((size_t)ptk::kClassBuckets * cp.stride);
    seg_totals = scratch.take<uint32_t>((size_t)ptk::kClassBuckets * ptk::kClassMaxSegs);
    if (!tile_counts || !seg_totals) return fail(PTK_ERR_NOMEM, "scratch block too small");
  }
  // One chain of sections: search (phase 1) | other (class order) | search (phase 2, cooperative search, replay).
  Timer timer(t, s);
  hipLaunchKernelGGL((ptk::knn1_phase1u_kernel<LEAFB, M>), dim3(blocks), dim3(64), 0, s, knn1_tree(t), d_q, t->dim, perm, nq,
                     e_inv, d_out, cont, qs, tile_counts, cp.stride, scratch.batch_verdict());
  timer.next(0, nq);
  if (cap) {
    // With the cap the order inside the heavy classes does not matter (no query runs long), only the three class
    // bits do: 8 buckets, counted per tile by phase 1 -- scan of the counters, stable scatter, which also writes
    // the tier table (ptk_kernels.hpp, "the class order from the tile counts of phase 1").
    hipLaunchKernelGGL(ptk::class_scan_kernel, dim3(ptk::kClassBuckets * cp.segs), dim3(64), 0, s, tile_counts, cp.ntiles,
                       cp.stride, cp.seg, seg_totals);
    hipLaunchKernelGGL(ptk::class_order_kernel, dim3(cp.chunks), dim3(64), 0, s, cont.key, (uint32_t)nq, cp.per,
                       tile_counts, cp.stride, cp.seg, cp.segs, seg_totals, ids_out, cont, tiers, extra_waves,
                       direct ? 1u : 0u);
    PTK_HIP(hipGetLastError());
  } else {
    // Every query runs to its end in phase 2: the full 16-bit key (the ranked classes by how far their
    // home-leaf best is), so that the most expensive continuations start first.
    PTK_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, cont.key, key_out, slot_ids, ids_out, nq, 0, 16, s));
    hipLaunchKernelGGL(ptk::knn1_phase_meta_kernel, dim3(1), dim3(1), 0, s, key_out, (uint32_t)nq, cont, tiers,
                       extra_waves);
  }
  timer.next(2, 0);
  // (a failure between fork and join must not leave the second stream working on a scratch block the next call reuses)
  struct SideGuard {
    hipStream_t side = nullptr;
    ~SideGuard() {
      if (side) (void)hipStreamSynchronize(side);
    }
  } side_guard;
  if (direct == 2) {  // fork: the ranked classes, cooperatively, while phase 2 takes the rest
    side_guard.side = side;
    PTK_HIP(hipEventRecord(fork, s));
    PTK_HIP(hipStreamWaitEvent(side, fork, 0));
    int rc = launch_knn1_coop<M>(t, qs, d_out, cont, ho, redo_list, side, spill_a, ids_out);
    if (rc != PTK_OK) return rc;
    PTK_HIP(hipEventRecord(join, side));
  } else if (direct == 1) {
    int rc = launch_knn1_coop<M>(t, qs, d_out, cont, ho, redo_list, s, spill_a, ids_out);
    if (rc != PTK_OK) return rc;
  }
  const dim3 p2_grid(blocks + 1 + extra_waves);
  // LDS ring of phase 2.  With the cap no stack grows deep: 12 slots = 6 KB per wave = 26 waves per CU beat
  // 16 (20 waves) and 8 (40 waves) on both clouds (profiles/r02_notes.txt items 10, 23); without it 16 slots
  // (r01l_notes item 8).
  if (cap) {
    hipLaunchKernelGGL((ptk::knn1_phase2_kernel<kP2Ring, OVF, LEAFB, M>), p2_grid, dim3(64), (size_t)kP2Ring * 64 * 8, s, knn1_tree(t), qs,
                       e_inv, d_out, cont, ids_out, cap, ho);
  } else {
    hipLaunchKernelGGL((ptk::knn1_phase2_kernel<16, OVF, LEAFB, M>), p2_grid, dim3(64), (size_t)16 * 64 * 8, s, knn1_tree(t), qs,
                       e_inv, d_out, cont, ids_out, 0u, ho);
  }
  PTK_HIP(hipGetLastError());
  if (cap) {  // the queries phase 2 gave up on, then whatever the cooperative search could not certify
    // (the two cooperative launches may run side by side: each has its own spill block, and they append to the one
    // redo list through one atomic counter)
    int rc = launch_knn1_coop<M>(t, qs, d_out, cont, ho, redo_list, s, spill_b);
    if (rc != PTK_OK) return rc;
    if (direct == 2) {  // join: the replay needs both lists complete
      PTK_HIP(hipStreamWaitEvent(s, join, 0));
      side_guard.side = nullptr;
    }
    hipLaunchKernelGGL((ptk::knn1_redo_kernel<16, OVF, LEAFB, M>), dim3(t->cus), dim3(64), (size_t)16 * 64 * 8, s, knn1_tree(t), qs,
                       e_inv, d_out, cont, redo_list);
    PTK_HIP(hipGetLastError());
  }
  if (t->n_piles) {  // rows that name the stand-in of a pile get the point of it the reference reports (ptk_piles.hpp)
    ptk::DevPiles piles;
    piles.of_point = static_cast<const uint32_t*>(t->d_pile_of_point);
    piles.recs = static_cast<const ptk::DevPileRecord*>(t->d_pile_recs);
    piles.n_points = (uint32_t)t->n_points;
    hipLaunchKernelGGL(ptk::resolve_piles_kernel, dim3((uint32_t)((nq + ptk::kBlock - 1) / ptk::kBlock)), dim3(ptk::kBlock), 0, s,
                       d_q, t->dim, nq, piles, d_out);
    PTK_HIP(hipGetLastError());
  }
  timer.stop(3, 0);
  return PTK_OK;
}

// ---- any dimension (dim > 3) -----------------------------------------------------------------
// LDS per 64-lane block: record ring + q[dim] + off[dim] (+ the k-list while it fits).
// (the most dynamic LDS a block may ask for is the handle's lds_per_block, from the device's properties)

template <class M>
int dispatch_knn1_of(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float e,
                     ptk::Neighbor* d_out, hipStream_t s, Scratch& scratch) {
  // (the depth of what is traversed: the view without the piles if there is one)
  return ptkd::with_ovf<ptk::kOvfSlots[0], ptk::kOvfSlots[1], ptk::kOvfSlots[2]>(
      ovf_class_of(knn1_depth(t), 16),
      [&](auto ovf) { return launch_knn1_two_phase<ovf, M>(t, d_q, perm, nq, e, d_out, s, scratch); },
      [&] { return fail(PTK_ERR_UNSUPPORTED, "tree depth %u is too deep for the device stack", knn1_depth(t)); });
}
// The two-phase k = 1 search: metric_l2_squared, and (r06) metric_l1 on trees without piles (see knn1_two_phase()).
int dispatch_knn1(const ptk_tree* t, const float* d_q, const uint32_t* perm, uint64_t nq, float e,
                  ptk::Neighbor* d_out, hipStream_t s, Scratch& scratch) {
  if (t->metric.load() == PTK_METRIC_L1) return dispatch_knn1_of<ptk::MetricL1>(t, d_q, perm, nq, e, d_out, s, scratch);
  return dispatch_knn1_of<ptk::MetricL2>(t, d_q, perm, nq, e, d_out, s, scratch);
}

// A deep tree (deep_tree(t): deeper than the private stack classes, any k, any metric) is searched a few queries at a
// time, the record stacks spilling to HBM.  The spill block comes out of `scratch` -- reserved here (deep_plan) unless
// the caller has reserved it with bytes of its own --, then `launch(dev, lo, n)` runs per piece of the plan, `dev` being
// the handle's tree view with the spill bound to it: ptk::DevTree for dim <= 3, ptk::DevTreeND above.  One profile
// section around all pieces (Timer::stop(kind, queries)); the launch error is looked at after every piece.
template <class Launch>
int deep_pieces(const ptk_tree* t, uint64_t nq, hipStream_t s, Scratch& scratch, int kind, uint64_t queries, Launch&& launch) {
  const DeepPlan plan = deep_plan(t, nq);
  if (!scratch.reserved()) {
    const int rc = scratch.reserve(plan.bytes());
    if (rc != PTK_OK) return rc;
  }
  ptk::Record* spill = scratch.take<ptk::Record>((size_t)plan.piece * plan.cap);
  if (spill == nullptr) return fail(PTK_ERR_NOMEM, "scratch block too small");
  ptk::DevTree dev = t->dev;
  dev.deep_spill = spill;
  dev.deep_cap = plan.cap;
  ptk::DevTreeND dev_nd = t->dev_nd;
  dev_nd.deep_spill = spill;
  dev_nd.deep_cap = plan.cap;
  Timer timer(t, s);
  uint32_t pieces = 0;
  for (uint64_t lo = 0; lo < nq; lo += plan.piece) {
    const uint64_t n = std::min<uint64_t>(plan.piece, nq - lo);
    const int rc = t->dim > 3 ? launch(dev_nd, lo, n) : launch(dev, lo, n);
    if (rc != PTK_OK) return rc;
    PTK_HIP(hipGetLastError());
    ++pieces;
  }
  scratch.note_pieces(pieces);
  timer.stop(kind, queries);
  return PTK_OK;
}
// (the deep launches of ptk_family_nd.hip under the names of their 3-D forms: deep_pieces hands its callable either view)
int knn_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k, float e,
             ptk::Neighbor* d_out, hipStream_t s) {
  return ptkf::knn_nd_deep(t, dev, d_q, n, k, e, d_out, s);
}
int knn_within_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k, float radius,
                    ptk::Neighbor* d_out, hipStream_t s) {
  return ptkf::knn_nd_within_deep(t, dev, d_q, n, k, radius, d_out, s);
}
int radius_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, float radius, float e, bool fill,
                uint64_t* d_counts, const uint64_t* d_offsets, ptk::Neighbor* d_out, hipStream_t s) {
  return ptkf::radius_nd_deep(t, dev, d_q, n, radius, e, fill, d_counts, d_offsets, d_out, s);
}
using ptkf::knn_deep;
using ptkf::knn_within_deep;
int knn_within_radii_deep(const ptk_tree* t, const ptk::DevTreeND& dev, const float* d_q, uint64_t n, uint32_t k,
                          const float* d_radii, ptk::Neighbor* d_out, hipStream_t s) {
  return ptkf::knn_nd_within_radii_deep(t, dev, d_q, n, k, d_radii, d_out, s);
}
using ptkf::knn_within_radii_deep;
using ptkf::radius_deep;

// Very large batches go through in pieces of at most 2^25 queries: the scratch of a piece stays
// at a few GB and every 32-bit index in the kernels holds (PTK_MAX_BATCH shrinks it for tests).
// `search(first, n)` takes rows [first, first + n) of the batch.
template <class Search>
int in_batch_pieces(uint64_t nq, Search&& search) {
  const uint64_t piece = (uint64_t)std::max(1, env_int("PTK_MAX_BATCH", 1 << 25));
  for (uint64_t done = 0; done < nq; done += piece) {
    const int rc = search(done, std::min(piece, nq - done));
    if (rc != PTK_OK) return rc;
  }
  return PTK_OK;
}

}  // namespace

namespace ptkf {
int morton_bits(uint64_t nq) { return ::morton_bits(nq); }
size_t sort_tmp_bytes(uint64_t nq, int bits) { return ::sort_tmp_bytes(nq, bits); }
size_t permutation_scratch_bytes(uint64_t nq) { return ::permutation_scratch_bytes(nq); }
int sort_pairs_u32(void* tmp, size_t tmp_bytes, uint32_t* keys, uint32_t* keys_out, uint32_t* ids, uint32_t* ids_out,
                   uint64_t nq, int bits, hipStream_t s) {
  PTK_HIP(rocprim::radix_sort_pairs<MortonSortConfig>(tmp, tmp_bytes, keys, keys_out, ids, ids_out, nq, 0, bits, s));
  return PTK_OK;
}
}  // namespace ptkf

// =====================================================================================
extern "C" {

int ptk_version(void) { return PTK_VERSION; }

const char* ptk_last_error(void) { return g_error.c_str(); }

int ptk_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return -1;
  return count;
}

int ptk_warmup(int32_t device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(PTK_ERR_DEVICE, "no HIP device is visible");
  if (device >= count) return fail(PTK_ERR_INVALID, "device %d out of range (%d visible)", device, count);
  g_warmup.start(device);
  return PTK_OK;
}

int ptk_tree_create(const ptk_tree_desc* d, ptk_tree** out) {
  if (out == nullptr) return fail(PTK_ERR_INVALID, "null out pointer");
  *out = nullptr;
  if (d == nullptr || d->points == nullptr || d->nodes == nullptr || d->indices == nullptr)
    return fail(PTK_ERR_INVALID, "null descriptor field");
  if (d->dim == 0 || d->n_points == 0 || d->n_nodes == 0)
    return fail(PTK_ERR_INVALID, "dim, n_points and n_nodes must be positive");
  if (d->n_points >= (1ull << 31)) return fail(PTK_ERR_INVALID, "n_points must be < 2^31");
  if (d->n_nodes >= (1ull << 32) - 1) return fail(PTK_ERR_INVALID, "n_nodes must be < 2^32 - 1");
  ptk_tree* t = new (std::nothrow) ptk_tree;
  if (t == nullptr) return fail(PTK_ERR_NOMEM, "out of memory");
  try {
    t->dim = d->dim;
    t->n_points = d->n_points;
    t->nodes.assign(d->nodes, d->nodes + d->n_nodes);
    t->indices.assign(d->indices, d->indices + d->n_points);
    if (d->root_min != nullptr && d->root_max != nullptr) {
      t->root_min.assign(d->root_min, d->root_min + d->dim);
      t->root_max.assign(d->root_max, d->root_max + d->dim);
    }
  } catch (const std::bad_alloc&) {
    delete t;
    return fail(PTK_ERR_NOMEM, "out of memory");
  }
  return finish_create(t, d->points, d->device, out);
}

int ptk_tree_create_from_points(const float* points, uint64_t n_points, uint32_t dim, uint64_t max_leaf_size,
                                int32_t device, ptk_tree** out) {
  if (out == nullptr) return fail(PTK_ERR_INVALID, "null out pointer");
  *out = nullptr;
  if (points == nullptr) return fail(PTK_ERR_INVALID, "null points");
  if (dim == 0 || n_points == 0 || max_leaf_size == 0)
    return fail(PTK_ERR_INVALID, "dim, n_points and max_leaf_size must be positive");
  if (n_points >= (1ull << 31)) return fail(PTK_ERR_INVALID, "n_points must be < 2^31");
  if (const int rc = check_points_finite(points, n_points, dim); rc != PTK_OK) return rc;
  ptk_tree* t = new (std::nothrow) ptk_tree;
  if (t == nullptr) return fail(PTK_ERR_NOMEM, "out of memory");
  g_warmup.start(device);
  try {
    using namespace pico_tree;
    using space_t = space_map<point_map<float const, dynamic_extent>>;
    space_t space(points, n_points, dim);
    internal::space_view<space_t> view(space);
    // (the two outer bounds per branch come for free while the child boxes are at hand; only the
    // topological metrics ever read them)
    CreateClock clock(t->create_ms);
    // Large clouds bound for a device: the partitions of the top levels are made there (ptk_build.hpp), the subtrees
    // below by the host's workers -- the same tree.  PTK_DEVICE_BUILD=0: everything on the host.
    internal::flat_tree<int, float, dynamic_extent> flat(dim);
    bool built = false;
    ptk::BuildRoute& route = t->create_route;
    route.why = device == kDeviceNone                 ? "host-only handle"
                : n_points < (1ull << 18)             ? "fewer than 2^18 points"
                : env_int("PTK_DEVICE_BUILD", 1) == 0 ? "PTK_DEVICE_BUILD=0"
                                                      : "no usable HIP device";
    if (device != kDeviceNone && n_points >= (1ull << 18) && env_int("PTK_DEVICE_BUILD", 1) != 0) {
      int count = 0, dev = device;
      if (hipGetDeviceCount(&count) == hipSuccess && count > 0 && (dev >= 0 || hipGetDevice(&dev) == hipSuccess) && dev < count) {
        DeviceGuard guard(dev);
        g_warmup.wait(dev);
        double ms[2] = {0, 0};
        route.why = "hipSetDevice failed";
        if (guard.ok) built = ptk::device_top_build(points, n_points, dim, (size_t)max_leaf_size, build_threads(), view, flat, ms, &route);
        if (!built && clock.on) std::fprintf(stderr, "[ptk create] top levels not on the device: %s\n", route.why);
        if (built && clock.on)
          std::fprintf(stderr, "[ptk create] top levels on the device     %8.2f ms\n[ptk create] subtrees on the host          %8.2f ms\n",
                       ms[0], ms[1]);
      }
      (void)hipGetLastError();
    }
    if (!built)
      flat = internal::build_flat_tree<int>(view, max_leaf_size_t(max_leaf_size), bounds_from_space,
                                            sliding_midpoint_max_side, true, build_threads());
    clock.lap(built ? "device + host build" : "host build", 0);
    t->dim = dim;
    t->n_points = n_points;
    t->nodes.resize(flat.nodes.size());
    t->outer.resize(flat.outer_bounds.size() * 2);
    ptk::parallel_chunks(flat.nodes.size(), build_threads(), 1u << 16, [&](size_t lo, size_t hi, unsigned) {
      std::memcpy(t->nodes.data() + lo, flat.nodes.data() + lo, (hi - lo) * sizeof(ptk_node));
      if (!flat.outer_bounds.empty()) std::memcpy(t->outer.data() + 2 * lo, flat.outer_bounds.data() + lo, (hi - lo) * 2 * sizeof(float));
    });
    t->indices = std::move(flat.indices);
    t->builder_made = true;
    t->n_leaves = flat.leaf_count;
    t->max_leaf_count = (uint32_t)flat.max_leaf_points;
    t->max_depth = flat.max_depth;
    for (uint32_t a = 0; a < 3; ++a) t->axis_splits[a] = a < dim && a < flat.axis_weight.size() ? flat.axis_weight[a] / (double)n_points : 0.0;
    t->root_min.assign(flat.root_box.min(), flat.root_box.min() + dim);
    t->root_max.assign(flat.root_box.max(), flat.root_box.max() + dim);
    clock.lap("copy into the handle", 1);
  } catch (const std::bad_alloc&) {
    delete t;
    return fail(PTK_ERR_NOMEM, "out of memory");
  } catch (const std::length_error& err) {  // degenerate point set: see flat_builder::grow
    delete t;
    return fail(PTK_ERR_UNSUPPORTED, "%s", err.what());
  }
  return finish_create(t, points, device, out);
}

void ptk_tree_destroy(ptk_tree* t) {
  if (t == nullptr) return;
  if (t->device >= 0) {
    DeviceGuard guard(t->device);
    for (PendingEvent& p : t->profile.pending) {
      (void)hipEventDestroy(p.a);
      if (!p.keep_b) (void)hipEventDestroy(p.b);
    }
    for (hipEvent_t e : t->profile.idle) (void)hipEventDestroy(e);
    auto drop_side = [](Workspace& w) {
      if (w.side) (void)hipStreamSynchronize(w.side);
      if (w.fork) (void)hipEventDestroy(w.fork);
      if (w.join) (void)hipEventDestroy(w.join);
      if (w.side) (void)hipStreamDestroy(w.side);
    };
    drain_workspace(t->ws);
    drop_side(t->ws);
    if (t->ws.done) (void)hipEventDestroy(t->ws.done);
    if (t->ws.base) (void)hipFree(t->ws.base);
    if (t->ws.cap_base) (void)hipFree(t->ws.cap_base);
    for (Workspace& w : t->extra_ws) {
      drain_workspace(w);
      drop_side(w);
      if (w.done) (void)hipEventDestroy(w.done);
      if (w.base) (void)hipFree(w.base);
    }
    if (t->io.d_in) (void)hipFree(t->io.d_in);
    if (t->io.d_out) (void)hipFree(t->io.d_out);
    for (int i = 0; i < HostIo::kRing; ++i) {
      if (t->io.h_in[i]) (void)hipHostFree(t->io.h_in[i]);
      if (t->io.h_out[i]) (void)hipHostFree(t->io.h_out[i]);
      if (t->io.up_done[i]) (void)hipEventDestroy(t->io.up_done[i]);
      if (t->io.down_done[i]) (void)hipEventDestroy(t->io.down_done[i]);
    }
    for (hipStream_t st : {t->io.up, t->io.down, t->io.search[0], t->io.search[1]})
      if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t ev : t->io.searched)
      if (ev) (void)hipEventDestroy(ev);
    if (t->d_nodes) (void)hipFree(t->d_nodes);
    if (t->d_pts) (void)hipFree(t->d_pts);
    if (t->d_ranges) (void)hipFree(t->d_ranges);
    if (t->d_axes) (void)hipFree(t->d_axes);
    if (t->d_index) (void)hipFree(t->d_index);
    if (t->d_outer) (void)hipFree(t->d_outer);
    if (t->d_cells) (void)hipFree(t->d_cells);
    if (t->d_nodes1) (void)hipFree(t->d_nodes1);
    if (t->d_ranges1) (void)hipFree(t->d_ranges1);
    if (t->d_pile_of_point) (void)hipFree(t->d_pile_of_point);
    if (t->d_pile_recs) (void)hipFree(t->d_pile_recs);
    if (t->d_count_table) (void)hipFree(t->d_count_table);
    if (t->d_align_inverse) (void)hipFree(t->d_align_inverse);
  }
  delete t;
}

int ptk_tree_get_info(const ptk_tree* t, ptk_tree_info* info) {
  if (t == nullptr || info == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  info->dim = t->dim;
  info->n_points = t->n_points;
  info->n_nodes = t->nodes.size();
  info->n_leaves = t->n_leaves;
  info->max_depth = t->max_depth;
  info->max_leaf_count = t->max_leaf_count;
  info->device_bytes = t->device_bytes;
  info->device = t->device;
  return PTK_OK;
}

int ptk_tree_get_flat(const ptk_tree* t, ptk_node* nodes, int32_t* indices, float* root_min, float* root_max) {
  if (t == nullptr) return fail(PTK_ERR_INVALID, "null tree");
  if (nodes) std::memcpy(nodes, t->nodes.data(), t->nodes.size() * sizeof(ptk_node));
  if (indices) std::memcpy(indices, t->indices.data(), t->indices.size() * sizeof(int32_t));
  if (root_min) std::memcpy(root_min, t->root_min.data(), t->dim * sizeof(float));
  if (root_max) std::memcpy(root_max, t->root_max.data(), t->dim * sizeof(float));
  return PTK_OK;
}

static int serialize_tree(const ptk_tree* t, bool topological, void* buf, uint64_t cap, uint64_t* size) {
  if (t == nullptr || size == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (topological && t->outer.size() != 2 * t->nodes.size())
    return fail(PTK_ERR_INVALID, "this tree has no outer bounds (ptk_tree_set_outer_bounds): it cannot be written as a topological tree");
  try {
    using tree_t = pico_tree::internal::flat_tree<int, float, pico_tree::dynamic_extent>;
    tree_t flat(t->dim);
    flat.indices.assign(t->indices.begin(), t->indices.end());
    std::memcpy(flat.root_box.min(), t->root_min.data(), t->dim * sizeof(float));
    std::memcpy(flat.root_box.max(), t->root_max.data(), t->dim * sizeof(float));
    flat.nodes.resize(t->nodes.size());
    std::memcpy(static_cast<void*>(flat.nodes.data()), t->nodes.data(), t->nodes.size() * sizeof(ptk_node));
    if (topological) {  // the four bounds of kd_tree_branch_double (kd_tree_node.hpp:52-67)
      flat.keep_outer_bounds = true;
      flat.outer_bounds.resize(t->nodes.size());
      std::memcpy(static_cast<void*>(flat.outer_bounds.data()), t->outer.data(), t->outer.size() * sizeof(float));
    }
    std::ostringstream os(std::ios::out | std::ios::binary);
    pico_tree::internal::write_flat_tree(flat, os);
    const std::string bytes = os.str();
    *size = bytes.size();
    if (buf == nullptr) return PTK_OK;
    if (cap < bytes.size()) return fail(PTK_ERR_INVALID, "buffer of %llu bytes, stream needs %llu",
                                        (unsigned long long)cap, (unsigned long long)bytes.size());
    std::memcpy(buf, bytes.data(), bytes.size());
    return PTK_OK;
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of memory");
  }
}

int ptk_tree_serialize(const ptk_tree* t, void* buf, uint64_t cap, uint64_t* size) {
  return serialize_tree(t, false, buf, cap, size);
}

int ptk_tree_serialize_topological(const ptk_tree* t, void* buf, uint64_t cap, uint64_t* size) {
  return serialize_tree(t, true, buf, cap, size);
}

static int create_from_stream(const float* points, uint64_t n_points, uint32_t dim, const void* stream,
                              uint64_t stream_bytes, bool topological, int32_t device, ptk_tree** out) {
  if (out == nullptr) return fail(PTK_ERR_INVALID, "null out pointer");
  *out = nullptr;
  if (points == nullptr || stream == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (dim == 0 || n_points == 0) return fail(PTK_ERR_INVALID, "dim and n_points must be positive");
  ptk_tree* t = nullptr;
  try {
    using tree_t = pico_tree::internal::flat_tree<int, float, pico_tree::dynamic_extent>;
    std::istringstream is(std::string(static_cast<const char*>(stream), stream_bytes), std::ios::in | std::ios::binary);
    tree_t flat = pico_tree::internal::read_flat_tree<tree_t>(is, topological, dim, n_points);
    if (flat.root_box.size() != dim) return fail(PTK_ERR_INVALID, "stream is %zu-dimensional, points are %u-dimensional",
                                                 (size_t)flat.root_box.size(), dim);
    if (flat.indices.size() != n_points)
      return fail(PTK_ERR_INVALID, "stream indexes %zu points, %llu were given", flat.indices.size(),
                  (unsigned long long)n_points);
    t = new ptk_tree;
    t->dim = dim;
    t->n_points = n_points;
    t->nodes.resize(flat.nodes.size());
    std::memcpy(t->nodes.data(), flat.nodes.data(), flat.nodes.size() * sizeof(ptk_node));
    if (topological) {  // {left_min, right_max} per node: what the topological metrics need besides the 16-byte record
      t->outer.resize(flat.outer_bounds.size() * 2);
      if (!flat.outer_bounds.empty()) std::memcpy(t->outer.data(), flat.outer_bounds.data(), t->outer.size() * sizeof(float));
    }
    t->indices.assign(flat.indices.begin(), flat.indices.end());
    t->root_min.assign(flat.root_box.min(), flat.root_box.min() + dim);
    t->root_max.assign(flat.root_box.max(), flat.root_box.max() + dim);
  } catch (const std::bad_alloc&) {
    delete t;
    return fail(PTK_ERR_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    delete t;
    return fail(PTK_ERR_INVALID, "bad kd_tree stream: %s", e.what());
  }
  return finish_create(t, points, device, out);
}

int ptk_tree_create_from_stream(const float* points, uint64_t n_points, uint32_t dim, const void* stream,
                                uint64_t stream_bytes, int32_t device, ptk_tree** out) {
  return create_from_stream(points, n_points, dim, stream, stream_bytes, false, device, out);
}

int ptk_tree_create_from_topological_stream(const float* points, uint64_t n_points, uint32_t dim, const void* stream,
                                            uint64_t stream_bytes, int32_t device, ptk_tree** out) {
  return create_from_stream(points, n_points, dim, stream, stream_bytes, true, device, out);
}

int ptk_tree_set_outer_bounds(ptk_tree* t, const float* outer, uint64_t n_nodes) {
  if (t == nullptr || outer == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (n_nodes != t->nodes.size()) return fail(PTK_ERR_INVALID, "outer bounds for %llu nodes, the tree has %zu",
                                              (unsigned long long)n_nodes, t->nodes.size());
  try {
    t->outer.assign(outer, outer + 2 * n_nodes);
    {
      std::lock_guard<std::mutex> lock(t->host_flat_mutex);
      t->host_flat.reset();
    }
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of memory");
  }
  return PTK_OK;
}

int ptk_tree_get_outer_bounds(const ptk_tree* t, float* outer) {
  if (t == nullptr || outer == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (t->outer.size() != 2 * t->nodes.size()) return fail(PTK_ERR_INVALID, "this tree has no outer bounds");
  std::memcpy(outer, t->outer.data(), t->outer.size() * sizeof(float));
  return PTK_OK;
}

int ptk_tree_set_metric(ptk_tree* t, int metric) {
  if (t == nullptr || metric < PTK_METRIC_L2_SQUARED || metric > PTK_METRIC_SE2_SQUARED)
    return fail(PTK_ERR_INVALID, "bad metric");
  if (metric == PTK_METRIC_SO2 || metric == PTK_METRIC_SE2_SQUARED) {
    if (metric == PTK_METRIC_SO2 && t->dim != 1) return fail(PTK_ERR_INVALID, "metric_so2 is a metric of 1-dimensional points");
    if (metric == PTK_METRIC_SE2_SQUARED && t->dim != 3)
      return fail(PTK_ERR_INVALID, "metric_se2_squared is a metric of 3-dimensional points (x, y, angle)");
    if (t->outer.size() != 2 * t->nodes.size())
      return fail(PTK_ERR_INVALID, "the topological metrics need the outer bounds of every branch (ptk_tree_set_outer_bounds)");
    if (t->device >= 0 && t->gpu_layout && t->d_outer == nullptr) {  // branch order of the device records
      ptk::TreeStats st;
      std::vector<uint32_t> branch_id;
      std::string err = ptk::analyse_stream(t->dim, t->n_points, t->nodes.data(), t->nodes.size(), st, &branch_id);
      if (!err.empty()) return fail(PTK_ERR_INVALID, "%s", err.c_str());
      std::vector<float> dev_outer(2 * std::max<size_t>(t->nodes.size() - st.n_leaves, 1), 0.0f);
      for (size_t i = 0; i < t->nodes.size(); ++i) {
        if (t->nodes[i].right == PTK_LEAF) continue;
        dev_outer[2 * (size_t)branch_id[i]] = t->outer[2 * i];
        dev_outer[2 * (size_t)branch_id[i] + 1] = t->outer[2 * i + 1];
      }
      DeviceGuard guard(t->device);
      PTK_HIP(hipMalloc(&t->d_outer, dev_outer.size() * sizeof(float)));
      PTK_HIP(hipMemcpy(t->d_outer, dev_outer.data(), dev_outer.size() * sizeof(float), hipMemcpyHostToDevice));
      t->dev.outer = static_cast<const float2*>(t->d_outer);
      t->device_bytes += dev_outer.size() * sizeof(float);
    }
  }
  t->metric.store(metric);
  return PTK_OK;
}

int ptk_tree_set_reorder(ptk_tree* t, int mode) {
  if (t == nullptr || mode < PTK_REORDER_AUTO || mode > PTK_REORDER_OFF)
    return fail(PTK_ERR_INVALID, "bad reorder mode");
  t->reorder.store(mode);
  return PTK_OK;
}

// ---- knn --------------------------------------------------------------------------------

// One piece of a k-NN batch (at most PTK_MAX_BATCH queries), the arguments checked.
static int knn_piece_device(const ptk_tree* t, const float* d_q, uint64_t nq, uint32_t k, float e, ptk::Neighbor* d_out,
                            hipStream_t s) {
  // k > n_points: what the reference's iterator-range search_knn does with a range longer than the
  // tree (search_visitor.hpp:95-110; its Python binding passes k through unclamped): the n_points
  // neighbours in order, the last slot's distance left at the FLT_MAX sentinel.  The slots in
  // between are the caller's in the reference; here they hold {0, FLT_MAX} as every slot a search did
  // not write (ptk.h; KnnPolicy::end_query).  (These rows take the list-in-the-row kernels.)
  const bool short_tree = k > t->n_points;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  const bool l2 = t->metric.load() == PTK_METRIC_L2_SQUARED;
  // k = 1 takes the two-phase search (phase 1, class order, capped phase 2, cooperative search) under the default metric
  // and under metric_l1 on a tree without piles: both are sums of per-axis terms, so the box distance the reference
  // keeps is a lower bound of the point distances below it -- what the cooperative search's certificate needs.  (The
  // pile view resolves its stand-ins for the default metric only.)
  const bool two_phase = k == 1 && t->dim <= 3 && (l2 || (t->metric.load() == PTK_METRIC_L1 && t->n_piles == 0));
  if (topological(t)) {
    if (deep_tree(t)) return fail(PTK_ERR_UNSUPPORTED, "tree depth %u is too deep for the device stack", t->max_depth);
    Scratch scratch(t, s, /*per_stream=*/true);
    uint32_t* perm = nullptr;
    const int rc = order_batch(t, d_q, nq, s, scratch, 0, &perm);
    if (rc != PTK_OK) return rc;
    return ptkf::knn_topo(t, d_q, perm, nq, k, e, d_out, s, short_tree);
  }
  const bool knn1_view = k == 1 && l2 && t->dim <= 3 && t->n_piles != 0 && ovf_class_of(knn1_depth(t), 16) != kDeepClass;
  if (deep_tree(t) && !knn1_view) {  // a few queries at a time, the record stacks spilling to HBM (any k, any metric)
    Scratch scratch(t, s, /*per_stream=*/true);
    return deep_pieces(t, nq, s, scratch, 0, nq, [&](const auto& dev, uint64_t lo, uint64_t n) {
      return knn_deep(t, dev, d_q + lo * t->dim, n, k, e, d_out + lo * k, s);
    });
  }
  Scratch scratch(t, s, /*per_stream=*/true);
  // (the general kernels run every query to its end in its lane: the expensive queries to the front of the launch)
  // (the two-phase k = 1 search orders its own continuations: a batch that arrives coherent is not sorted again --
  // REORDER_AUTO only; the general kernels want the expensive queries in front whatever the order)
  const bool may_skip = two_phase && t->reorder.load() == PTK_REORDER_AUTO;
  uint32_t* perm = nullptr;
  const int rc = order_batch(t, d_q, nq, s, scratch,
                         (two_phase ? two_phase_scratch_bytes(t, nq) : 0) +
                             (k > 1 && k <= 64 && (l2 || t->metric.load() == PTK_METRIC_L1) && t->dim <= 3 && knn_cap(e, nq, k) != 0u
                                  ? knn_coop_scratch_bytes(t, nq)
                                  : 0),
                         &perm, t->dim <= 3 && !two_phase ? ptk::kCellsEmptyFirst : 0u, may_skip);
  if (rc != PTK_OK) return rc;
  if (t->dim > 3) return ptkf::knn_nd(t, d_q, perm, nq, k, e, d_out, s, short_tree);
  if (two_phase) return dispatch_knn1(t, d_q, perm, nq, e, d_out, s, scratch);
  if (k <= knn_reg_max() && !short_tree) return ptkf::knn_reg(t, d_q, perm, nq, k, e, d_out, s, &scratch);
  return ptkf::knn_rows(t, d_q, perm, nq, k, e, d_out, s);
}

int ptk_search_knn_device(const ptk_tree* t, const float* d_q, uint64_t nq, uint32_t k, float e,
                          ptk_neighbor* d_out, void* stream) {
  int rc = check_search(t, d_q, nq);
  if (rc == PTK_OK) rc = check_k(k);
  if (rc == PTK_OK) rc = check_ratio(e);
  if (rc != PTK_OK || nq == 0) return rc;
  if (d_out == nullptr) return fail(PTK_ERR_INVALID, "null output buffer");
  return in_batch_pieces(nq, [&](uint64_t first, uint64_t n) {
    return knn_piece_device(t, d_q + first * t->dim, n, k, e, reinterpret_cast<ptk::Neighbor*>(d_out) + first * k,
                            static_cast<hipStream_t>(stream));
  });
}

// Grow-only device block of the host-buffer entry points (rounded up to 1 MiB; the old contents are dropped).
static int grow_device_block(char** p, size_t* capacity, size_t bytes) {
  if (bytes <= *capacity) return PTK_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *capacity = 0;
  const size_t want = (bytes + (size_t(1) << 20)) & ~((size_t(1) << 20) - 1);
  if (hipMalloc((void**)p, want) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return fail(PTK_ERR_NOMEM, "out of device memory (%zu bytes)", want);
  }
  *capacity = want;
  return PTK_OK;
}

// Grow-only ring of pinned host pieces (the old contents are dropped): the first `slots` entries, `bytes` each.
static int grow_pinned_ring(char* (&ring)[HostIo::kRing], size_t* capacity, size_t bytes, int slots) {
  bool have = bytes <= *capacity;
  for (int i = 0; i < slots && have; ++i) have = ring[i] != nullptr;
  if (have) return PTK_OK;
  const size_t want = std::max(*capacity, (bytes + (size_t(1) << 20)) & ~((size_t(1) << 20) - 1));
  if (want > *capacity) {  // (slots of another size are of no use)
    for (char*& p : ring) {
      if (p) (void)hipHostFree(p);
      p = nullptr;
    }
    *capacity = 0;
  }
  for (int i = 0; i < slots; ++i) {
    if (ring[i] != nullptr) continue;
    if (hipHostMalloc((void**)&ring[i], want, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      ring[i] = nullptr;
      return fail(PTK_ERR_NOMEM, "out of pinned host memory (%zu bytes)", want);
    }
  }
  *capacity = want;
  return PTK_OK;
}

// Is [p, p + bytes) page-locked host memory the runtime knows (ptk_host_alloc, hipHostMalloc, hipHostRegister)?  Copies
// to and from such memory need no staging.
static bool is_pinned_host(const void* p, size_t bytes) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (a.type != hipMemoryTypeHost) return false;
  if (bytes > 1) {
    hipPointerAttribute_t z{};
    if (hipPointerGetAttributes(&z, static_cast<const char*>(p) + bytes - 1) != hipSuccess || z.type != hipMemoryTypeHost) {
      (void)hipGetLastError();
      return false;
    }
  }
  return true;
}

// The pieces a host-buffer batch goes through in: first rows of every piece (and nq at the end).
//   k = 1   eight equal pieces, none below 256 k queries (the pipeline fills and drains by one piece on either side;
//           a search of fewer queries is all fixed cost).  On this platform the copy engine takes uploads and
//           downloads one after the other (48 and 56 GB/s alone, 53 GB/s together, profiles/r03a_pcie.json), so
//           the 144 MB of BASELINE config 2 cannot pass in less than 2.7 ms; ms per batch on one box
//           (profiles/r03_notes.txt item 7): one piece 8.5-22 (pageable copies, nothing overlapped), eight pieces 3.5,
//           four 3.6, two 3.9; a small first and last piece around large ones (the downloads then queue behind long
//           uploads) 3.8-4.3; uploads read by a kernel instead of the copy engine 5.2.
//   k > 1   the general kernels end with the tail of their slowest queries (3.4 ms for ANY piece of config 3 at
//           knn = 16), so a piece costs its tail: at most three pieces of at most 256 MB of rows.  Where the long
//           queries are handed to the cooperative search (`capped`: exact, metric_l2_squared, k <= 32, with a cap that
//           follows the piece -- knn_cap) a piece costs what its size costs, and the rows of the first one can leave
//           a millisecond after the call: eight pieces as for k = 1 (ms per batch of BASELINE config 3, three pieces /
//           eight: knn = 16 20.8 / 19.3 -- the 1 008 MB of the call at the 53 GB/s the link gives both directions
//           together are 19.0 --, knn = 8 15.0 / 10.5, knn = 4 9.9 / 7.0; profiles/r05_notes.txt item 13).
// PTK_HOST_PIECE = n: equal pieces of n queries (experiments).
static std::vector<uint64_t> host_pieces(uint64_t nq, uint32_t k, bool two_phase, bool capped) {
  std::vector<uint64_t> first;
  const int forced = knob_int("host_piece", 0);
  if (forced > 0) {
    for (uint64_t lo = 0; lo < nq; lo += (uint64_t)forced) first.push_back(lo);
  } else if (!two_phase && !capped) {
    const size_t obytes = (size_t)nq * k * sizeof(ptk_neighbor);
    const uint64_t pieces = std::min<uint64_t>(std::max<uint64_t>(obytes / (size_t(256) << 20), 1), 3);
    const uint64_t per = (nq + pieces - 1) / pieces;
    for (uint64_t lo = 0; lo < nq; lo += per) first.push_back(lo);
  } else {
    const uint64_t per = std::max<uint64_t>((nq + 7) / 8, uint64_t(1) << 18);
    for (uint64_t lo = 0; lo < nq; lo += per) first.push_back(lo);
  }
  first.push_back(nq);
  return first;
}

static int search_knn_host(const ptk_tree* t, const float* q, uint64_t nq, uint32_t k, float e, ptk_neighbor* out);
int ptk_search_knn(const ptk_tree* t, const float* q, uint64_t nq, uint32_t k, float e, ptk_neighbor* out) {
  try {  // (containers and threads of the pipeline may throw: nothing leaves through the C boundary)
    return search_knn_host(t, q, nq, k, e, out);
  } catch (const std::bad_alloc&) {
    return fail(PTK_ERR_NOMEM, "out of host memory in the host-buffer search");
  } catch (const std::exception& ex) {
    return fail(PTK_ERR_DEVICE, "host-buffer search failed: %s", ex.what());
  }
}
static int search_knn_host(const ptk_tree* t, const float* q, uint64_t nq, uint32_t k, float e, ptk_neighbor* out) {
  int rc = check_search(t, q, nq);
  if (rc != PTK_OK) return rc;
  if (k == 0) return fail(PTK_ERR_INVALID, "k must be >= 1");
  if (nq == 0) return PTK_OK;
  if (out == nullptr) return fail(PTK_ERR_INVALID, "null output buffer");
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  const size_t row_in = (size_t)t->dim * sizeof(float), row_out = (size_t)k * sizeof(ptk_neighbor);
  HostIo& io = t->io;
  std::lock_guard<std::mutex> lock(io.mutex);
  for (hipStream_t* st : {&io.up, &io.down, &io.search[0], &io.search[1]})
    if (*st == nullptr) PTK_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
  for (int i = 0; i < HostIo::kRing; ++i) {
    if (io.up_done[i] == nullptr) PTK_HIP(hipEventCreateWithFlags(&io.up_done[i], hipEventDisableTiming));
    if (io.down_done[i] == nullptr) PTK_HIP(hipEventCreateWithFlags(&io.down_done[i], hipEventDisableTiming));
  }
  const bool two_phase = k == 1 && t->dim <= 3 && t->metric.load() == PTK_METRIC_L2_SQUARED &&
                         ovf_class_of(knn1_depth(t), 16) != kDeepClass;
  const bool capped = !two_phase && k > 1 && k <= 64 && t->dim <= 3 &&
                      (t->metric.load() == PTK_METRIC_L2_SQUARED || t->metric.load() == PTK_METRIC_L1) &&
                      knn_cap(e, std::max<uint64_t>((nq + 7) / 8, uint64_t(1) << 18), k) != 0u;
  const std::vector<uint64_t> first = host_pieces(nq, k, two_phase, capped);
  const uint64_t pieces = first.size() - 1;
  uint64_t piece = 0;  // the largest piece: the size of a ring slot
  for (uint64_t i = 0; i < pieces; ++i) piece = std::max(piece, first[i + 1] - first[i]);
  while (io.searched.size() < pieces) {
    hipEvent_t ev = nullptr;
    PTK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    io.searched.push_back(ev);
  }
  rc = grow_device_block(&io.d_in, &io.in_capacity, (size_t)nq * row_in);
  if (rc == PTK_OK) rc = grow_device_block(&io.d_out, &io.out_capacity, (size_t)nq * row_out);
  if (rc != PTK_OK) return rc;
  const int n_search_streams = 2;
  // Arrays that are page-locked already (ptk_host_alloc: what the Python wrapper returns its rows in) are copied to
  // and from directly; pageable ones go through the handle's pinned rings.
  const bool in_pinned = knob_int("host_direct", 1) != 0 && is_pinned_host(q, (size_t)nq * row_in);
  const bool out_pinned = knob_int("host_direct", 1) != 0 && is_pinned_host(out, (size_t)nq * row_out);
  if (!in_pinned) rc = grow_pinned_ring(io.h_in, &io.h_in_capacity, (size_t)piece * row_in, (int)std::min<uint64_t>(pieces, HostIo::kRing));
  // The rows of a piece come down in chunks of at most 32 MB, each copied into the caller's array while the next
  // is on the link (a piece of knn = 16 rows is 300 MB: one copy per piece left the host copy exposed).
  const uint64_t out_chunk = std::max<uint64_t>(std::min<uint64_t>(piece, (size_t(32) << 20) / row_out), 1);
  struct Chunk {
    uint64_t piece, lo, n;
  };
  std::vector<Chunk> chunks;
  for (uint64_t pi = 0; pi < pieces; ++pi)
    for (uint64_t lo = first[pi]; lo < first[pi + 1]; lo += out_chunk)
      chunks.push_back(Chunk{pi, lo, std::min(out_chunk, first[pi + 1] - lo)});
  if (rc == PTK_OK && !out_pinned)
    rc = grow_pinned_ring(io.h_out, &io.h_out_capacity, (size_t)out_chunk * row_out,
                          (int)std::min<uint64_t>(chunks.size(), HostIo::kRing));
  if (rc == PTK_ERR_NOMEM) {
    // No pinned memory to be had: the batch goes through piece by piece with plain (pageable) copies -- slower, not a failure.
    for (uint64_t i = 0; i < pieces; ++i) {
      const uint64_t lo = first[i], n = first[i + 1] - lo;
      PTK_HIP(hipMemcpy(io.d_in + lo * row_in, reinterpret_cast<const char*>(q) + lo * row_in, (size_t)n * row_in, hipMemcpyHostToDevice));
      rc = ptk_search_knn_device(t, reinterpret_cast<float*>(io.d_in) + lo * t->dim, n, k, e,
                                 reinterpret_cast<ptk_neighbor*>(io.d_out) + lo * k, io.search[0]);
      if (rc != PTK_OK) return rc;
      PTK_HIP(hipStreamSynchronize(io.search[0]));
      PTK_HIP(hipMemcpy(reinterpret_cast<char*>(out) + lo * row_out, io.d_out + lo * row_out, (size_t)n * row_out, hipMemcpyDeviceToHost));
    }
    return PTK_OK;
  }
  if (rc != PTK_OK) return rc;
  if (io.pool == nullptr) {
    const unsigned hc = std::thread::hardware_concurrency();
    const int want = hc >= 16 ? 8 : (hc >= 4 ? (int)hc / 2 : 1);
    io.pool.reset(new CopyPool((unsigned)std::max(0, want - 1)));  // (the calling threads copy too)
  }
  float* d_q = reinterpret_cast<float*>(io.d_in);
  ptk_neighbor* d_out = reinterpret_cast<ptk_neighbor*>(io.d_out);
  const char* src = reinterpret_cast<const char*>(q);
  char* dst = reinterpret_cast<char*>(out);

  const bool trace = knob_int("host_trace", 0) != 0;
  const auto t_begin = std::chrono::steady_clock::now();
  auto stamp = [&](const char* what, uint64_t i) {
    if (!trace) return;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "[ptk host] %9.1f us  %-22s piece %llu\n", us, what, (unsigned long long)i);
  };
  // What the two threads tell each other: pieces whose search has been enqueued, and whether anything failed.
  std::mutex m;
  std::condition_variable cv;
  uint64_t issued = 0;
  bool failed = false;
  std::string down_error;
  const int device = t->device;

  std::thread downloader([&] {
    if (hipSetDevice(device) != hipSuccess) {
      std::lock_guard<std::mutex> l(m);
      failed = true;
      down_error = "hipSetDevice failed in the download thread";
      return;
    }
    auto bail = [&](hipError_t he) {
      std::lock_guard<std::mutex> l(m);
      failed = true;
      down_error = std::string("HIP error in the download thread: ") + hipGetErrorString(he);
    };
    // `e` chunks have their D2H enqueued, `c` are copied out (c <= e <= c + kRing).  A D2H is enqueued only when the
    // search of its piece HAS finished (see the header of ptk_hostio.hpp); while a search is still running the
    // thread copies out what has arrived.
    const uint64_t n_chunks = chunks.size();
    uint64_t e_ = 0, c_ = 0, searched_pieces = 0;  // pieces [0, searched_pieces) are known to be done
    while (c_ < n_chunks) {
      bool can_enqueue = false;
      if (e_ < n_chunks && e_ < c_ + (uint64_t)HostIo::kRing) {
        const uint64_t pi = chunks[e_].piece;
        can_enqueue = pi < searched_pieces;
        if (!can_enqueue) {
          {
            std::unique_lock<std::mutex> l(m);
            if (e_ == c_) cv.wait(l, [&] { return issued > pi || failed; });  // nothing to copy out meanwhile
            if (failed) return;
            can_enqueue = issued > pi;
          }
          if (can_enqueue) {
            const hipError_t q_ = e_ == c_ ? hipEventSynchronize(io.searched[pi]) : hipEventQuery(io.searched[pi]);
            if (q_ == hipErrorNotReady) {
              (void)hipGetLastError();
              can_enqueue = false;
            } else if (q_ != hipSuccess) {
              return bail(q_);
            } else {
              searched_pieces = pi + 1;
            }
          }
        }
      }
      if (can_enqueue) {
        const Chunk& ch = chunks[e_];
        const int slot = (int)(e_ % HostIo::kRing);
        hipError_t he = hipMemcpyAsync(out_pinned ? dst + ch.lo * row_out : io.h_out[slot], io.d_out + ch.lo * row_out,
                                       (size_t)ch.n * row_out, hipMemcpyDeviceToHost, io.down);
        if (he == hipSuccess) he = hipEventRecord(io.down_done[slot], io.down);
        if (he != hipSuccess) return bail(he);
        stamp("down: D2H enqueued", e_);
        ++e_;
        continue;
      }
      // (c_ < e_ here: the search of the next piece is still running, or the ring is full)
      const Chunk& ch = chunks[c_];
      const int slot = (int)(c_ % HostIo::kRing);
      const hipError_t he = hipEventSynchronize(io.down_done[slot]);
      if (he != hipSuccess) return bail(he);
      stamp("down: copy out", c_);
      if (!out_pinned) io.pool->copy(dst + ch.lo * row_out, io.h_out[slot], (size_t)ch.n * row_out);
      stamp("down: copied", c_);
      ++c_;
    }
  });

  // (whatever throws from here on: the download thread is told to stop and joined before the frame goes)
  struct Joiner {
    std::thread& th;
    std::mutex& m;
    std::condition_variable& cv;
    bool& failed;
    ~Joiner() {
      if (!th.joinable()) return;
      {
        std::lock_guard<std::mutex> l(m);
        failed = true;
      }
      cv.notify_all();
      th.join();
    }
  } joiner{downloader, m, cv, failed};
  hipError_t he = hipSuccess;
  // The copy of piece i + 1 into its ring slot runs on the pool while piece i is issued.
  auto start_copy_in = [&](uint64_t i) {
    const uint64_t lo = first[i], n = first[i + 1] - lo;
    if (in_pinned) return std::shared_ptr<CopyPool::Job>();
    return io.pool->start(io.h_in[i % HostIo::kRing], src + lo * row_in, (size_t)n * row_in);
  };
  std::shared_ptr<CopyPool::Job> copy_in = start_copy_in(0);
  for (uint64_t i = 0; i < pieces && he == hipSuccess && rc == PTK_OK; ++i) {
    const uint64_t lo = first[i], n = first[i + 1] - lo;
    const int slot = (int)(i % HostIo::kRing);
    if (copy_in) io.pool->finish(copy_in);
    stamp("up: copied", i);
    if (i + 1 < pieces && !in_pinned) {
      // (slot of piece i + 1: its last upload, of piece i + 1 - kRing, must have left it)
      if (i + 1 >= (uint64_t)HostIo::kRing) he = hipEventSynchronize(io.up_done[(i + 1) % HostIo::kRing]);
      if (he != hipSuccess) break;
      copy_in = start_copy_in(i + 1);
    }
    he = hipMemcpyAsync(io.d_in + lo * row_in, in_pinned ? src + lo * row_in : io.h_in[slot], (size_t)n * row_in,
                        hipMemcpyHostToDevice, io.up);
    if (he == hipSuccess) he = hipEventRecord(io.up_done[slot], io.up);
    hipStream_t ss = io.search[n_search_streams > 1 ? (i & 1) : 0];  // consecutive pieces on two streams: the tail of one overlaps the next
    if (he == hipSuccess) he = hipStreamWaitEvent(ss, io.up_done[slot], 0);
    if (he != hipSuccess) break;
    rc = ptk_search_knn_device(t, d_q + lo * t->dim, n, k, e, d_out + lo * k, ss);
    if (rc != PTK_OK) break;
    he = hipEventRecord(io.searched[i], ss);
    if (he != hipSuccess) break;
    stamp("up: search enqueued", i);
    {
      std::lock_guard<std::mutex> l(m);
      issued = i + 1;
      if (failed) break;
    }
    cv.notify_all();
  }
  if (copy_in) io.pool->finish(copy_in);  // (a piece copied ahead when the loop was left early: the caller's array is still being read)
  {
    std::lock_guard<std::mutex> l(m);
    if (he != hipSuccess || rc != PTK_OK) failed = true;
  }
  cv.notify_all();
  downloader.join();
  // Nothing of this call may be in flight when the caller's arrays (and, on failure, the ring) are touched again.
  hipError_t hs = hipSuccess;
  for (hipStream_t st : {io.up, io.search[0], io.search[1], io.down}) {
    const hipError_t r = hipStreamSynchronize(st);
    if (hs == hipSuccess) hs = r;
  }
  if (rc != PTK_OK) return rc;
  if (he != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(he));
  if (!down_error.empty()) return fail(PTK_ERR_DEVICE, "%s", down_error.c_str());
  if (hs != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(hs));
  return PTK_OK;
}

// ---- the k nearest within a radius -------------------------------------------

// The pruning bound the bounded k-list starts at: radius * (1 + 2^-10), the margin knn1_coop_kernel derives for the
// ulps the incremental box distance may drift by (ptk_kernels_coopk.hpp).  FLT_MAX -- the plain search, masked when
// the rows are stored -- where that argument does not hold: metrics whose box distance is no lower bound of the point
// distances (metric_lpinf / metric_lninf), a radius that is subnormal or whose margin overflows.
static float within_seed(const ptk_tree* t, float radius) {
  if (ptkf::unseeded_metric(t->metric.load())) return 3.402823466e+38f;
  if (radius != 0.0f && !std::isnormal(radius)) return 3.402823466e+38f;
  const float seed = radius * (1.0f + 0x1p-10f);
  return std::isfinite(seed) ? seed : 3.402823466e+38f;
}

// One piece of a bounded k-NN batch (at most PTK_MAX_BATCH queries, as knn_piece_device), the arguments checked.
static int knn_within_piece_device(const ptk_tree* t, const float* d_q, uint64_t nq, uint32_t k, float radius,
                                   ptk::Neighbor* d_out, hipStream_t s) {
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  Scratch scratch(t, s, /*per_stream=*/true);
  if (deep_tree(t)) {  // the deep stack class: the margin assumes shallower trees -- unseeded, masked at store
    return deep_pieces(t, nq, s, scratch, 0, nq, [&](const auto& dev, uint64_t lo, uint64_t n) {
      return knn_within_deep(t, dev, d_q + lo * t->dim, n, k, radius, d_out + lo * k, s);
    });
  }
  const float seed = within_seed(t, radius);
  // (as the general k-NN kernels: the expensive queries to the front of the launch)
  uint32_t* perm = nullptr;
  const int rc = order_batch(t, d_q, nq, s, scratch, 0, &perm, t->dim <= 3 ? ptk::kCellsEmptyFirst : 0u);
  if (rc != PTK_OK) return rc;
  if (t->dim > 3) return ptkf::knn_nd_within(t, d_q, perm, nq, k, seed, radius, d_out, s);
  return ptkf::knn_within(t, d_q, perm, nq, k, seed, radius, d_out, s);
}

int ptk_search_knn_within_device(const ptk_tree* t, const float* d_q, uint64_t nq, uint32_t k, float radius,
                                 ptk_neighbor* d_out, void* stream) {
  const int rc = check_knn_within(t, d_q, nq, k, radius, d_out);
  if (rc != PTK_OK || nq == 0) return rc;
  return in_batch_pieces(nq, [&](uint64_t first, uint64_t n) {
    return knn_within_piece_device(t, d_q + first * t->dim, n, k, radius,
                                   reinterpret_cast<ptk::Neighbor*>(d_out) + first * k, static_cast<hipStream_t>(stream));
  });
}

// search_knn_within_radii (ptk.h): knn_within_piece_device with a device array of one radius per row of the piece.  The
// lanes derive their seeds (within_seed() on the device: within_seed_row, ptk_kernels.hpp); the batch order is the scalar
// form's.
static int knn_within_radii_piece_device(const ptk_tree* t, const float* d_q, uint64_t nq, uint32_t k, const float* d_radii,
                                         ptk::Neighbor* d_out, hipStream_t s) {
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  Scratch scratch(t, s, /*per_stream=*/true);
  if (deep_tree(t)) {  // unseeded, each row masked at its own radius
    return deep_pieces(t, nq, s, scratch, 0, nq, [&](const auto& dev, uint64_t lo, uint64_t n) {
      return knn_within_radii_deep(t, dev, d_q + lo * t->dim, n, k, d_radii + lo, d_out + lo * k, s);
    });
  }
  uint32_t* perm = nullptr;
  const int rc = order_batch(t, d_q, nq, s, scratch, 0, &perm, t->dim <= 3 ? ptk::kCellsEmptyFirst : 0u);
  if (rc != PTK_OK) return rc;
  if (t->dim > 3) return ptkf::knn_nd_within_radii(t, d_q, perm, nq, k, d_radii, d_out, s);
  return ptkf::knn_within_radii(t, d_q, perm, nq, k, d_radii, d_out, s);
}

int ptk_search_knn_within_radii_device(const ptk_tree* t, const float* d_q, uint64_t nq, uint32_t k, const float* d_radii,
                                       ptk_neighbor* d_out, void* stream) {
  const int rc = check_knn_within_radii(t, d_q, nq, k, d_radii, d_out, /*host_values=*/false);
  if (rc != PTK_OK || nq == 0) return rc;
  return in_batch_pieces(nq, [&](uint64_t first, uint64_t n) {
    return knn_within_radii_piece_device(t, d_q + first * t->dim, n, k, d_radii + first,
                                         reinterpret_cast<ptk::Neighbor*>(d_out) + first * k,
                                         static_cast<hipStream_t>(stream));
  });
}

}  // extern "C"

namespace {

// The host-buffer form of every call whose rows have one size, written once: under the handle's I/O lock the input parts
// go up into the handle's input block, `search(d_in, d_out, stream)` -- the _device form, which finds its device pointers
// with in.at<T>(d_in, i) and out.at<T>(d_out, i) -- runs on one stream of the handle, and the output parts come down
// from its output block.  An absent part (ptk_io_parts.hpp) is neither copied nor given room.
template <class Search>
int host_form(const ptk_tree* t, const ptkio::Parts& in, const ptkio::Parts& out, Search&& search) {
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  HostIo& io = t->io;
  std::lock_guard<std::mutex> lock(io.mutex);
  if (io.search[0] == nullptr) PTK_HIP(hipStreamCreateWithFlags(&io.search[0], hipStreamNonBlocking));
  hipStream_t s = io.search[0];
  int rc = grow_device_block(&io.d_in, &io.in_capacity, in.total());
  if (rc == PTK_OK) rc = grow_device_block(&io.d_out, &io.out_capacity, out.total());
  if (rc != PTK_OK) return rc;
  for (int i = 0; i < in.size(); ++i)
    if (in.present(i)) PTK_HIP(hipMemcpyAsync(io.d_in + in.offset(i), in.source(i), in.bytes(i), hipMemcpyHostToDevice, s));
  rc = search(io.d_in, io.d_out, s);
  if (rc != PTK_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  for (int i = 0; i < out.size(); ++i)
    if (out.present(i)) PTK_HIP(hipMemcpyAsync(out.destination(i), io.d_out + out.offset(i), out.bytes(i), hipMemcpyDeviceToHost, s));
  PTK_HIP(hipStreamSynchronize(s));
  return PTK_OK;
}

}  // namespace

extern "C" {

int ptk_search_knn_within(const ptk_tree* t, const float* q, uint64_t nq, uint32_t k, float radius, ptk_neighbor* out) {
  const int rc = check_knn_within(t, q, nq, k, radius, out);
  if (rc != PTK_OK || nq == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(q, (size_t)nq * t->dim * sizeof(float))};
  const ptkio::Parts rows{ptkio::out_part(out, (size_t)nq * k * sizeof(ptk_neighbor))};
  return host_form(t, in, rows, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_search_knn_within_device(t, in.at<float>(d_in, 0), nq, k, radius, rows.at<ptk_neighbor>(d_out, 0), s);
  });
}

int ptk_search_knn_within_radii(const ptk_tree* t, const float* q, uint64_t nq, uint32_t k, const float* radii,
                                ptk_neighbor* out) {
  const int rc = check_knn_within_radii(t, q, nq, k, radii, out, /*host_values=*/true);
  if (rc != PTK_OK || nq == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(q, (size_t)nq * t->dim * sizeof(float)), ptkio::in_part(radii, (size_t)nq * sizeof(float))};
  const ptkio::Parts rows{ptkio::out_part(out, (size_t)nq * k * sizeof(ptk_neighbor))};
  return host_form(t, in, rows, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_search_knn_within_radii_device(t, in.at<float>(d_in, 0), nq, k, in.at<float>(d_in, 1),
                                              rows.at<ptk_neighbor>(d_out, 0), s);
  });
}

// ---- each tree point's k nearest other points -------------------------------

// Which route serves search_knn_self(k) on this handle: 1 = the direct kernel (ptk_family_self.hip, K17), 2 = the
// staged route.  The direct kernel serves 3-D float32 trees of the four non-topological metrics and the private stack
// classes with k + 1 <= 64; test hook self_route = 2 sends those through the staged route as well.  The rule is the
// capability rule alone: measured on cloud L at 7.73 M and 150 k points, k = 1 / 7 / 15 / 16, the direct kernel takes
// 0.42-0.67 / 0.19-0.37 of the staged route's time and is nowhere slower (profiles/knn_self_bench.json).
static int self_route_of(const ptk_tree* t, uint32_t k) {
  const bool direct = t->dim <= 3 && !topological(t) && !deep_tree(t) && k < 64u;
  return direct && knob_int("self_route", 0) != 2 ? 1 : 2;
}

int ptk_search_knn_self_device(const ptk_tree* t, uint32_t k, ptk_neighbor* d_out, void* stream) {
  const int rc = check_knn_self(t, k, d_out);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ptk::Neighbor* out = reinterpret_cast<ptk::Neighbor*>(d_out);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  if (self_route_of(t, k) == 1) {  // (ranges of leaf positions: no scratch, nothing allocated, nothing waited for)
    return in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) { return ptkf::knn_self(t, first, n, k, out, s); });
  }
  const float4* recs = t->dim <= 3 ? t->dev.pts : nullptr;
  const int32_t* index = t->dim <= 3 ? nullptr : t->dev_nd.index;
  return ptkf::self_staged<float, ptk_neighbor>(
      t->n_points, t->dim, k, s,
      [&](uint64_t first, uint64_t n, float* d_q) {
        return ptkf::self_queries(recs, t->dev_nd.pts, t->dim, t->dim, first, n, d_q, s);
      },
      // (the handle's own search, refusals included -- a topological tree of the deep class -- and its own scratch lock)
      [&](const float* d_q, uint64_t n, ptk_neighbor* d_rows) { return ptk_search_knn_device(t, d_q, n, k + 1u, 1.0f, d_rows, s); },
      [&](const ptk_neighbor* d_rows, uint64_t first, uint64_t n) {
        return ptkf::drop_self(reinterpret_cast<const ptk::Neighbor*>(d_rows), recs, index, first, n, k, out, s);
      });
}

// The host form: nothing goes up -- the rows come down only (through the output block of the handle's host staging).
int ptk_search_knn_self(const ptk_tree* t, uint32_t k, ptk_neighbor* out) {
  const int rc = check_knn_self(t, k, out);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  const ptkio::Parts rows{ptkio::out_part(out, (size_t)t->n_points * k * sizeof(ptk_neighbor))};
  return host_form(t, ptkio::Parts{}, rows, [&](char*, char* d_out, hipStream_t s) {
    return ptk_search_knn_self_device(t, k, rows.at<ptk_neighbor>(d_out, 0), s);
  });
}

int ptk_debug_self_route(const ptk_tree* t, uint32_t k, int* route) {
  if (route == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  const int rc = check_knn_self(t, k, route);
  if (rc != PTK_OK) return rc;
  *route = self_route_of(t, k);
  return PTK_OK;
}

// ---- spacing_knn_self (ptk.h; the kernels: ptk_kernels_spacing.hpp) ------------------------------------

int ptk_spacing_knn_self_workspace(const ptk_tree* t, uint64_t* bytes) {
  if (t == nullptr || bytes == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  *bytes = ptkf::spacing_workspace_bytes(t->n_points);
  return PTK_OK;
}

// The routes of ptk_search_knn_self_device with the reducing exit (route 1: only enqueues; route 2: allocates and waits),
// then the statistics on the same stream.  The radius capture and the side tables are neither read nor invalidated.
int ptk_spacing_knn_self_device(const ptk_tree* t, uint32_t k, uint32_t flags, float ratio, float* d_mean, float* d_kth,
                                uint8_t* d_keep, ptk_spacing_stats* d_stats, void* d_workspace, uint64_t workspace_bytes,
                                void* stream) {
  const bool reduce = d_keep != nullptr || d_stats != nullptr;
  int rc = check_spacing(t, k, flags, ratio, d_mean, reduce);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  rc = ptkf::spacing_check_workspace(t->n_points, reduce, d_workspace, workspace_bytes);
  if (rc != PTK_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  if (self_route_of(t, k) == 1) {  // (ranges of leaf positions: no scratch, nothing allocated, nothing waited for)
    rc = in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) {
      return ptkf::spacing_self(t, first, n, k, flags, d_mean, d_kth, s);
    });
  } else {
    const float4* recs = t->dim <= 3 ? t->dev.pts : nullptr;
    const int32_t* index = t->dim <= 3 ? nullptr : t->dev_nd.index;
    rc = ptkf::self_staged<float, ptk_neighbor>(
        t->n_points, t->dim, k, s,
        [&](uint64_t first, uint64_t n, float* d_q) {
          return ptkf::self_queries(recs, t->dev_nd.pts, t->dim, t->dim, first, n, d_q, s);
        },
        [&](const float* d_q, uint64_t n, ptk_neighbor* d_rows) { return ptk_search_knn_device(t, d_q, n, k + 1u, 1.0f, d_rows, s); },
        [&](const ptk_neighbor* d_rows, uint64_t first, uint64_t n) {
          return ptkf::spacing_rows(reinterpret_cast<const ptk::Neighbor*>(d_rows), recs, index, first, n, k, flags, d_mean,
                                    d_kth, s);
        });
  }
  if (rc != PTK_OK || !reduce) return rc;
  return ptkf::spacing_statistics(d_mean, t->n_points, ratio, d_keep, d_stats, static_cast<char*>(d_workspace), s);
}

// The host form: nothing goes up; the outputs that were asked for come down from a block of the call's own.
int ptk_spacing_knn_self(const ptk_tree* t, uint32_t k, uint32_t flags, float ratio, float* mean, float* kth, uint8_t* keep,
                         ptk_spacing_stats* stats) {
  const int rc = check_spacing(t, k, flags, ratio, mean, keep != nullptr || stats != nullptr);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  return ptkf::spacing_host_form<float>(t->n_points, mean, kth, keep, stats,
                                        [&](float* d_mean, float* d_kth, uint8_t* d_keep, ptk_spacing_stats* d_stats,
                                            void* d_ws, uint64_t ws_bytes) {
                                          return ptk_spacing_knn_self_device(t, k, flags, ratio, d_mean, d_kth, d_keep, d_stats,
                                                                             d_ws, ws_bytes, nullptr);
                                        });
}

// ---- neighbour counts within a radius ---------------------------------------

// The side table of count_within_kernel: built once per handle, on the first count, under the handle's own lock (calls
// that arrive together wait for the one that builds it).
static int count_table_of(const ptk_tree* t, hipStream_t s) {
  std::lock_guard<std::mutex> lock(t->count_table_mutex);
  if (t->count_table_built) return PTK_OK;
  void* table = nullptr;
  const int rc = ptkf::count_table(t, &table, s);
  if (rc != PTK_OK) return rc;
  ptk_tree* m = const_cast<ptk_tree*>(t);
  m->d_count_table = table;
  m->device_bytes += t->n_branches * ptkf::kCountBoxBytes;
  m->count_table_built = true;
  return PTK_OK;
}

// count_within never goes through radius_pass_device: the handle's radius capture (Workspace::cap_*) stays as the last
// count pass left it.  3-D trees of the four non-topological metrics take count_within_kernel (the clamp in the kernel);
// dim > 3, the topological metrics and deep trees the count kernels of the radius search, clamped afterwards.
int ptk_search_count_within_device(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, uint64_t max_count,
                                   uint64_t* d_counts, void* stream) {
  int rc = check_count_within(t, d_q, nq, radius, d_counts);
  if (rc != PTK_OK || nq == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  const bool nd = t->dim > 3;
  if (!nd && !topological(t) && !deep_tree(t)) {
    rc = count_table_of(t, s);
    if (rc != PTK_OK) return rc;
  }
  Scratch scratch(t, s, /*per_stream=*/true);
  uint32_t* perm = nullptr;
  if (topological(t)) {
    if (deep_tree(t)) return fail(PTK_ERR_UNSUPPORTED, "tree depth %u is too deep for the device stack", t->max_depth);
    rc = order_batch(t, d_q, nq, s, scratch, 0, &perm);
    if (rc != PTK_OK) return rc;
    rc = ptkf::radius_topo(t, d_q, perm, nq, radius, 1.0f, false, d_counts, nullptr, nullptr, s);
  } else if (deep_tree(t)) {  // record stacks spilling to HBM, a few queries per launch
    rc = deep_pieces(t, nq, s, scratch, 0, nq, [&](const auto& dev, uint64_t lo, uint64_t n) {
      return radius_deep(t, dev, d_q + lo * t->dim, n, radius, 1.0f, false, d_counts + lo, nullptr, nullptr, s);
    });
  } else {
    // (the batch order of the radius count pass: a query costs what it finds, the densest cells first)
    rc = order_batch(t, d_q, nq, s, scratch, 0, &perm, nd ? 0u : ptk::kCellsDenseFirst);
    if (rc != PTK_OK) return rc;
    if (!nd)
      return ptkf::count_within(t, d_q, perm, nq, radius, max_count, knob_int("count_shortcut", 1) != 0, d_counts, s);
    rc = ptkf::radius_nd(t, d_q, nq, radius, 1.0f, false, d_counts, nullptr, nullptr, s, perm);
  }
  if (rc != PTK_OK) return rc;
  return ptkf::clamp_counts(d_counts, nq, max_count, s);
}

int ptk_search_count_within(const ptk_tree* t, const float* q, uint64_t nq, float radius, uint64_t max_count,
                            uint64_t* counts) {
  const int rc = check_count_within(t, q, nq, radius, counts);
  if (rc != PTK_OK || nq == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(q, (size_t)nq * t->dim * sizeof(float))};
  const ptkio::Parts out{ptkio::out_part(counts, (size_t)nq * sizeof(uint64_t))};
  return host_form(t, in, out, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_search_count_within_device(t, in.at<float>(d_in, 0), nq, radius, max_count, out.at<uint64_t>(d_out, 0), s);
  });
}

// count_within_radii (ptk.h): the side-table kernel -- the table the scalar call builds and uses, whichever comes first --
// with a radius per row; every handle the scalar call sends through the radius search's count pass is refused
// (check_count_within_radii).  The batch order is the scalar call's.
int ptk_search_count_within_radii_device(const ptk_tree* t, const float* d_q, uint64_t nq, const float* d_radii,
                                         uint64_t max_count, uint64_t* d_counts, void* stream) {
  int rc = check_count_within_radii(t, d_q, nq, d_radii, d_counts, /*host_values=*/false);
  if (rc != PTK_OK || nq == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  rc = count_table_of(t, s);
  if (rc != PTK_OK) return rc;
  Scratch scratch(t, s, /*per_stream=*/true);
  uint32_t* perm = nullptr;
  rc = order_batch(t, d_q, nq, s, scratch, 0, &perm, ptk::kCellsDenseFirst);
  if (rc != PTK_OK) return rc;
  return ptkf::count_within_radii(t, d_q, perm, nq, d_radii, max_count, knob_int("count_shortcut", 1) != 0, d_counts, s);
}

int ptk_search_count_within_radii(const ptk_tree* t, const float* q, uint64_t nq, const float* radii, uint64_t max_count,
                                  uint64_t* counts) {
  const int rc = check_count_within_radii(t, q, nq, radii, counts, /*host_values=*/true);
  if (rc != PTK_OK || nq == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(q, (size_t)nq * t->dim * sizeof(float)), ptkio::in_part(radii, (size_t)nq * sizeof(float))};
  const ptkio::Parts out{ptkio::out_part(counts, (size_t)nq * sizeof(uint64_t))};
  return host_form(t, in, out, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_search_count_within_radii_device(t, in.at<float>(d_in, 0), nq, in.at<float>(d_in, 1), max_count,
                                                out.at<uint64_t>(d_out, 0), s);
  });
}

// ---- radius -------------------------------------------------------------------------------

// Rows ascending by distance, in place: one lane per row.
static int sort_rows(const ptk_tree* t, uint64_t n, const uint64_t* d_offsets, ptk::Neighbor* o, hipStream_t s) {
  Timer timer(t, s);
  const uint32_t blocks = (uint32_t)((n + ptk::kBlock - 1) / ptk::kBlock);
  hipLaunchKernelGGL(ptk::sort_rows_kernel, dim3(blocks), dim3(ptk::kBlock), 0, s, n, d_offsets, o);
  PTK_HIP(hipGetLastError());
  timer.stop(2, 0);
  return PTK_OK;
}

static int radius_pass_device(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, float e, bool fill,
                              uint64_t* d_counts, const uint64_t* d_offsets, ptk_neighbor* d_out, int sort,
                              hipStream_t s) {
  int rc = check_search(t, d_q, nq);
  if (rc == PTK_OK) rc = check_ratio(e);
  if (rc != PTK_OK || nq == 0) return rc;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  const bool nd = t->dim > 3;
  const int metric = t->metric.load();
  auto* o = reinterpret_cast<ptk::Neighbor*>(d_out);
  uint32_t* perm = nullptr;
  Scratch scratch(t, s);
  Workspace& ws = t->ws;  // locked by `scratch` for the duration of this call
  // A fill pass that repeats the arguments of the last count pass is served from its capture.
  const bool from_capture = fill && ws.cap_valid && ws.cap_q == d_q && ws.cap_nq == nq && ws.cap_radius == radius &&
                            ws.cap_e == e && ws.cap_metric == metric && ws.cap_stream == s;
  if (from_capture) {
    // (rows to search again: those of wavefronts whose lists were lost, and handed-over rows whose entries were)
    const uint64_t n_over_max = nq + ws.cap_heavy.max_heavy;
    rc = scratch.reserve(n_over_max * 4 + 256);
    if (rc != PTK_OK) return rc;
    uint32_t* over_list = scratch.take<uint32_t>(n_over_max);
    uint32_t* n_over = scratch.take<uint32_t>(1);
    if (over_list == nullptr || n_over == nullptr) return fail(PTK_ERR_NOMEM, "scratch block too small");
    if (ws.cap_lists) {  // (3-D trees: the rows are made from the leaf lists of the count pass)
      rc = ptkf::radius_replay(t, d_q, e, ws.cap, d_offsets, o, over_list, n_over, s,
                               ws.cap_heavy.max_heavy != 0u ? &ws.cap_heavy : nullptr);
      if (rc != PTK_OK) return rc;
    } else {
      rc = ptkf::radius_log_scatter(t, ws.cap, d_offsets, o, over_list, n_over, s);
      if (rc != PTK_OK) return rc;
    }
    // Rows the capture could not hold (possibly none: the blocks then leave at once).
    if (nd) {
      rc = ptkf::radius_nd(t, d_q, nq, radius, e, true, nullptr, d_offsets, o, s, over_list, n_over);
    } else {
      rc = ptkf::radius_traverse(t, d_q, over_list, n_over_max, radius, e, true, nullptr, d_offsets, o, s, n_over);
    }
  } else if (topological(t)) {  // count pass and fill pass both traverse (no capture)
    if (deep_tree(t)) return fail(PTK_ERR_UNSUPPORTED, "tree depth %u is too deep for the device stack", t->max_depth);
    if (!fill) ws.cap_valid = false;
    rc = order_batch(t, d_q, nq, s, scratch, 0, &perm);
    if (rc != PTK_OK) return rc;
    rc = ptkf::radius_topo(t, d_q, perm, nq, radius, e, fill, d_counts, d_offsets, o, s);
  } else if (deep_tree(t)) {  // record stacks spilling to HBM, a few queries per launch, no capture
    if (!fill) ws.cap_valid = false;
    rc = deep_pieces(t, nq, s, scratch, 0, fill ? 0 : nq, [&](const auto& dev, uint64_t lo, uint64_t n) {
      return radius_deep(t, dev, d_q + lo * t->dim, n, radius, e, fill, fill ? nullptr : d_counts + lo,
                         fill ? d_offsets + lo : nullptr, o, s);
    });
  } else {
    // (the long queries of a list pass are handed to wavefronts: ptk_kernels_coopr.hpp)
    const uint32_t far_cap = !fill && !nd && knob_int("radius_lists", 1) != 0 ? radius_cap(t, nq) : 0u;
    const bool capture = !fill && prepare_capture(t, nq, ws, far_cap != 0u);
    const bool lists = capture && !nd && knob_int("radius_lists", 1) != 0;
    if (!fill) ws.cap_valid = false;
    // (a query costs what it finds: the densest cells to the front of the launch)
    rc = order_batch(t, d_q, nq, s, scratch, lists && far_cap ? radius_coop_scratch_bytes(t, nq) : 0, &perm,
                     nd ? 0u : ptk::kCellsDenseFirst);
    if (rc != PTK_OK) return rc;
    if (capture) {
      if (nd) {
        rc = ptkf::radius_nd_capture(t, d_q, perm, nq, radius, e, d_counts, ws.cap, s);
      } else if (lists) {  // the count pass lists the leaves with hits for the fill pass
        rc = ptkf::radius_list(t, d_q, perm, nq, radius, e, d_counts, ws.cap, s, far_cap, &scratch, &ws.cap_heavy);
      } else {
        rc = ptkf::radius_capture(t, d_q, perm, nq, radius, e, d_counts, ws.cap, s);
      }
      if (rc == PTK_OK) {
        ws.cap_valid = true;
        ws.cap_lists = lists;
        ws.cap_q = d_q;
        ws.cap_nq = nq;
        ws.cap_radius = radius;
        ws.cap_e = e;
        ws.cap_metric = metric;
        ws.cap_stream = s;
      }
    } else if (nd) {
      rc = ptkf::radius_nd(t, d_q, nq, radius, e, fill, d_counts, d_offsets, o, s, perm);
    } else {
      rc = ptkf::radius_traverse(t, d_q, perm, nq, radius, e, fill, d_counts, d_offsets, o, s);
    }
  }
  if (rc == PTK_OK && fill && sort) rc = sort_rows(t, nq, d_offsets, o, s);
  return rc;
}

int ptk_search_radius_count_device(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, float e,
                                   uint64_t* d_counts, void* stream) {
  if (nq > 0 && d_counts == nullptr) return fail(PTK_ERR_INVALID, "null counts buffer");
  return radius_pass_device(t, d_q, nq, radius, e, false, d_counts, nullptr, nullptr, 0,
                            static_cast<hipStream_t>(stream));
}

int ptk_search_radius_fill_device(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, float e,
                                  const uint64_t* d_offsets, ptk_neighbor* d_out, int sort, void* stream) {
  if (nq > 0 && d_offsets == nullptr) return fail(PTK_ERR_INVALID, "null offsets buffer");
  return radius_pass_device(t, d_q, nq, radius, e, true, nullptr, d_offsets, d_out, sort,
                            static_cast<hipStream_t>(stream));
}

// The capture of a radius count pass is keyed on the device address of the query batch.  The host
// forms below own that buffer for one call only: once it is freed the address may be handed out
// again for ANOTHER batch, so the capture must not outlive the call.
static void drop_radius_capture(const ptk_tree* t) {
  std::lock_guard<std::mutex> lock(t->ws.mutex);
  t->ws.cap_valid = false;
}

int ptk_search_radius_count(const ptk_tree* t, const float* q, uint64_t nq, float radius, float e,
                            uint64_t* counts) {
  int rc = check_search(t, q, nq);
  if (rc != PTK_OK) return rc;
  if (nq == 0) return PTK_OK;
  if (counts == nullptr) return fail(PTK_ERR_INVALID, "null counts buffer");
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  DeviceBlock d_q, d_c;
  const size_t qbytes = (size_t)nq * t->dim * sizeof(float);
  hipError_t he = d_q.alloc(qbytes);
  if (he == hipSuccess) he = d_c.alloc(nq * 8);
  if (he == hipSuccess) he = hipMemcpy(d_q.p, q, qbytes, hipMemcpyHostToDevice);
  if (he == hipSuccess) {
    rc = ptk_search_radius_count_device(t, d_q.as<float>(), nq, radius, e, d_c.as<uint64_t>(), nullptr);
    if (rc == PTK_OK) he = hipMemcpy(counts, d_c.p, nq * 8, hipMemcpyDeviceToHost);
  }
  drop_radius_capture(t);
  if (rc != PTK_OK) return rc;
  if (he != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(he));
  return PTK_OK;
}

int ptk_search_radius_fill(const ptk_tree* t, const float* q, uint64_t nq, float radius, float e,
                           const uint64_t* offsets, ptk_neighbor* out, int sort) {
  int rc = check_search(t, q, nq);
  if (rc != PTK_OK) return rc;
  if (nq == 0) return PTK_OK;
  if (offsets == nullptr) return fail(PTK_ERR_INVALID, "null offsets buffer");
  const uint64_t total = offsets[nq];
  if (total > 0 && out == nullptr) return fail(PTK_ERR_INVALID, "null output buffer");
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  DeviceBlock d_q, d_o, d_out;
  const size_t qbytes = (size_t)nq * t->dim * sizeof(float);
  hipError_t he = d_q.alloc(qbytes);
  if (he == hipSuccess) he = d_o.alloc((nq + 1) * 8);
  if (he == hipSuccess) he = d_out.alloc(std::max<uint64_t>(total, 1) * 8);
  if (he == hipSuccess) he = hipMemcpy(d_q.p, q, qbytes, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d_o.p, offsets, (nq + 1) * 8, hipMemcpyHostToDevice);
  if (he == hipSuccess) {
    drop_radius_capture(t);  // d_q is this call's own copy: whatever was captured belongs to another buffer
    rc = ptk_search_radius_fill_device(t, d_q.as<float>(), nq, radius, e, d_o.as<uint64_t>(), d_out.as<ptk_neighbor>(), sort,
                                       nullptr);
    if (rc == PTK_OK && total > 0) he = hipMemcpy(out, d_out.p, total * 8, hipMemcpyDeviceToHost);
  }
  if (rc != PTK_OK) return rc;
  if (he != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(he));
  return PTK_OK;
}

int ptk_search_radius(const ptk_tree* t, const float* q, uint64_t nq, float radius, float e, int sort,
                      uint64_t* offsets, ptk_neighbor** out) {
  if (out != nullptr) *out = nullptr;
  if (out == nullptr || offsets == nullptr) return fail(PTK_ERR_INVALID, "null output pointer");
  int rc = check_search(t, q, nq);
  if (rc != PTK_OK) return rc;
  offsets[0] = 0;
  if (nq == 0) return PTK_OK;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  DeviceBlock d_q, d_c, d_o, d_out;
  const size_t qbytes = (size_t)nq * t->dim * sizeof(float);
  hipError_t he = d_q.alloc(qbytes);
  if (he == hipSuccess) he = d_c.alloc((nq + 1) * 8);
  if (he == hipSuccess) he = d_o.alloc((nq + 1) * 8);
  if (he == hipSuccess) he = hipMemcpy(d_q.p, q, qbytes, hipMemcpyHostToDevice);
  rc = rows_to_host(
      he, nq, d_c.as<uint64_t>(), d_o.as<uint64_t>(), offsets, out, rows_in<ptk_neighbor>(d_out),
      [&](uint64_t* d_counts) { return ptk_search_radius_count_device(t, d_q.as<float>(), nq, radius, e, d_counts, nullptr); },
      [&](const uint64_t* d_offsets, ptk_neighbor* d_rows, uint64_t) {
        return ptk_search_radius_fill_device(t, d_q.as<float>(), nq, radius, e, d_offsets, d_rows, sort, nullptr);
      });
  drop_radius_capture(t);
  return rc;
}

// ---- radius, a radius per query row (ptk.h) --------------------------------------------------

// The fill pass behind ptk_search_count_within_radii_device(max_count = 0) and a scan of its counts: the same handles
// (check_count_within_radii), the same batch order, a scratch block of the stream's own.  It never goes through
// radius_pass_device: the handle's radius capture (Workspace::cap_*) is neither read nor invalidated.
int ptk_search_radius_radii_fill_device(const ptk_tree* t, const float* d_q, uint64_t nq, const float* d_radii,
                                        const uint64_t* d_offsets, ptk_neighbor* d_out, int sort, void* stream) {
  int rc = check_radius_radii(t, d_q, nq, d_radii, d_offsets, /*host_values=*/false);
  if (rc != PTK_OK || nq == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  auto* o = reinterpret_cast<ptk::Neighbor*>(d_out);
  Scratch scratch(t, s, /*per_stream=*/true);
  uint32_t* perm = nullptr;
  rc = order_batch(t, d_q, nq, s, scratch, 0, &perm, ptk::kCellsDenseFirst);
  if (rc != PTK_OK) return rc;
  rc = ptkf::radius_radii_fill(t, d_q, perm, nq, d_radii, d_offsets, o, s);
  if (rc == PTK_OK && sort) rc = sort_rows(t, nq, d_offsets, o, s);
  return rc;
}

// Convenience, as ptk_search_radius: the count, the scan and the fill on the device; the radii go up beside the queries.
int ptk_search_radius_radii(const ptk_tree* t, const float* q, uint64_t nq, const float* radii, int sort, uint64_t* offsets,
                            ptk_neighbor** out) {
  if (out != nullptr) *out = nullptr;
  if (out == nullptr || offsets == nullptr) return fail(PTK_ERR_INVALID, "null output pointer");
  int rc = check_radius_radii(t, q, nq, radii, offsets, /*host_values=*/true);
  if (rc != PTK_OK) return rc;
  offsets[0] = 0;
  if (nq == 0) return PTK_OK;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  DeviceBlock d_in, d_c, d_o, d_out;
  const size_t qbytes = (size_t)nq * t->dim * sizeof(float);
  hipError_t he = d_in.alloc(qbytes + nq * sizeof(float));
  if (he == hipSuccess) he = d_c.alloc((nq + 1) * 8);
  if (he == hipSuccess) he = d_o.alloc((nq + 1) * 8);
  if (he == hipSuccess) he = hipMemcpy(d_in.p, q, qbytes, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(static_cast<char*>(d_in.p) + qbytes, radii, nq * sizeof(float), hipMemcpyHostToDevice);
  const float* d_q = d_in.as<float>();
  const float* d_radii = d_q + nq * t->dim;
  return rows_to_host(
      he, nq, d_c.as<uint64_t>(), d_o.as<uint64_t>(), offsets, out, rows_in<ptk_neighbor>(d_out),
      [&](uint64_t* d_counts) { return ptk_search_count_within_radii_device(t, d_q, nq, d_radii, 0, d_counts, nullptr); },
      [&](const uint64_t* d_offsets, ptk_neighbor* d_rows, uint64_t) {
        return ptk_search_radius_radii_fill_device(t, d_q, nq, d_radii, d_offsets, d_rows, sort, nullptr);
      });
}

// ---- the radius searches of the tree's own points (ptk.h) -----------------------

// count_within_self: count_self_kernel over ranges of leaf positions (the piece rule of ptk_search_knn_self) -- no
// scratch, nothing allocated but the handle's count side table on its first use, nothing waited for.  The handle's
// radius capture is neither read nor invalidated.
int ptk_search_count_within_self_device(const ptk_tree* t, float radius, const float* d_radii, uint64_t max_count,
                                        uint64_t* d_counts, void* stream) {
  int rc = check_radius_self(t, radius, d_radii, /*host_values=*/false, d_counts, "count_within_self",
                             "ptk_host_search_count_within_self");
  if (rc != PTK_OK || t->n_points == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  rc = count_table_of(t, s);
  if (rc != PTK_OK) return rc;
  const bool shortcut = knob_int("count_shortcut", 1) != 0;
  return in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) {
    return ptkf::count_self(t, first, n, radius, d_radii, max_count, shortcut, d_counts, s);
  });
}

// The fill pass behind ptk_search_count_within_self_device(max_count = 0) and a scan of its counts.
int ptk_search_radius_self_fill_device(const ptk_tree* t, float radius, const float* d_radii, const uint64_t* d_offsets,
                                       ptk_neighbor* d_out, int sort, void* stream) {
  int rc = check_radius_self(t, radius, d_radii, /*host_values=*/false, d_offsets, "search_radius_self",
                             "ptk_host_search_radius_self");
  if (rc != PTK_OK || t->n_points == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  auto* o = reinterpret_cast<ptk::Neighbor*>(d_out);
  rc = in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) {
    return ptkf::radius_self_fill(t, first, n, radius, d_radii, d_offsets, o, s);
  });
  if (rc == PTK_OK && sort) rc = sort_rows(t, t->n_points, d_offsets, o, s);
  return rc;
}

// The host form: only the radii go up (behind nothing: there are no queries), the counts come down.
int ptk_search_count_within_self(const ptk_tree* t, float radius, const float* radii, uint64_t max_count, uint64_t* counts) {
  const int rc = check_radius_self(t, radius, radii, /*host_values=*/true, counts, "count_within_self",
                                   "ptk_host_search_count_within_self");
  if (rc != PTK_OK || t->n_points == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(radii, (size_t)t->n_points * sizeof(float))};
  const ptkio::Parts out{ptkio::out_part(counts, (size_t)t->n_points * sizeof(uint64_t))};
  return host_form(t, in, out, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_search_count_within_self_device(t, radius, in.at<float>(d_in, 0), max_count, out.at<uint64_t>(d_out, 0), s);
  });
}

// Convenience, as ptk_search_radius_radii: the count, the scan and the fill on the device.
int ptk_search_radius_self(const ptk_tree* t, float radius, const float* radii, int sort, uint64_t* offsets,
                           ptk_neighbor** out) {
  if (out != nullptr) *out = nullptr;
  if (out == nullptr || offsets == nullptr) return fail(PTK_ERR_INVALID, "null output pointer");
  int rc = check_radius_self(t, radius, radii, /*host_values=*/true, offsets, "search_radius_self",
                             "ptk_host_search_radius_self");
  if (rc != PTK_OK) return rc;
  offsets[0] = 0;
  const uint64_t np = t->n_points;
  if (np == 0) return PTK_OK;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  DeviceBlock d_r, d_c, d_o, d_out;
  hipError_t he = d_c.alloc((np + 1) * 8);
  if (he == hipSuccess) he = d_o.alloc((np + 1) * 8);
  if (he == hipSuccess && radii != nullptr) he = d_r.alloc(np * sizeof(float));
  if (he == hipSuccess && radii != nullptr) he = hipMemcpy(d_r.p, radii, np * sizeof(float), hipMemcpyHostToDevice);
  const float* d_radii = d_r.as<float>();  // (null without per-row radii)
  return rows_to_host(
      he, np, d_c.as<uint64_t>(), d_o.as<uint64_t>(), offsets, out, rows_in<ptk_neighbor>(d_out),
      [&](uint64_t* d_counts) { return ptk_search_count_within_self_device(t, radius, d_radii, 0, d_counts, nullptr); },
      [&](const uint64_t* d_offsets, ptk_neighbor* d_rows, uint64_t) {
        return ptk_search_radius_self_fill_device(t, radius, d_radii, d_offsets, d_rows, sort, nullptr);
      });
}

// ---- cluster_within_self (ptk.h; the passes: ptk_kernels_cluster.hpp) -------------------------------------

// Enqueues the passes on `stream`, each over all pieces of leaf positions before the next: d_labels is the only working
// array, nothing is allocated but the handle's count side table on its first use (min_neighbors > 0: the mark pass reads
// it), nothing is waited for.  The handle's radius capture is neither read nor invalidated.
int ptk_cluster_within_self_device(const ptk_tree* t, float radius, const float* d_radii, uint64_t min_neighbors,
                                   int32_t* d_labels, void* stream) {
  int rc = check_radius_self(t, radius, d_radii, /*host_values=*/false, d_labels, "cluster_within_self",
                             "ptk_host_cluster_within_self");
  if (rc != PTK_OK || t->n_points == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  if (min_neighbors > 0) {
    rc = count_table_of(t, s);
    if (rc != PTK_OK) return rc;
  }
  const bool shortcut = knob_int("count_shortcut", 1) != 0;
  const bool compress = knob_int("cluster_compress", ptkf::kClusterCompress ? 1 : 0) != 0;
  const uint64_t np = t->n_points;
  auto traversal = [&](int pass) {
    return in_batch_pieces(np, [&](uint64_t first, uint64_t n) {
      return ptkf::cluster_self(t, pass, first, n, radius, d_radii, min_neighbors, shortcut, compress, d_labels, s);
    });
  };
  auto elementwise = [&](int pass) {
    Timer timer(t, s);
    const int erc = ptkf::cluster_elementwise(pass, np, compress, d_labels, s);
    timer.stop(2, 0);
    return erc;
  };
  rc = min_neighbors == 0 ? elementwise(ptkf::kClusterInit) : traversal(ptkf::kClusterMark);
  if (rc == PTK_OK) rc = traversal(ptkf::kClusterLink);
  if (rc == PTK_OK) rc = elementwise(ptkf::kClusterFlatten);
  if (rc == PTK_OK && min_neighbors > 0) rc = traversal(ptkf::kClusterBorder);
  if (rc == PTK_OK && min_neighbors > 0) rc = elementwise(ptkf::kClusterDecode);
  return rc;
}

// The host form: only the radii go up, the labels come down; n_clusters (may be null) counts the labels[i] == i.
int ptk_cluster_within_self(const ptk_tree* t, float radius, const float* radii, uint64_t min_neighbors, int32_t* labels,
                            uint64_t* n_clusters) {
  if (n_clusters != nullptr) *n_clusters = 0;
  const int rc = check_radius_self(t, radius, radii, /*host_values=*/true, labels, "cluster_within_self",
                                   "ptk_host_cluster_within_self");
  if (rc != PTK_OK || t->n_points == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(radii, (size_t)t->n_points * sizeof(float))};
  const ptkio::Parts out{ptkio::out_part(labels, (size_t)t->n_points * sizeof(int32_t))};
  const int src = host_form(t, in, out, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_cluster_within_self_device(t, radius, in.at<float>(d_in, 0), min_neighbors, out.at<int32_t>(d_out, 0), s);
  });
  if (src == PTK_OK && n_clusters != nullptr) *n_clusters = count_cluster_roots(labels, t->n_points);
  return src;
}

// ---- suppress_within_self (ptk.h; the round: ptk_kernels_suppress.hpp) -----------------------------------

// Enqueues the init kernel and then ROUNDS on `stream`, each over all pieces of leaf positions before the next, until a
// round leaves no point undecided.  d_keep is the only working array.  Unlike the other _device forms this one WAITS on
// the stream once per round and reads 4 bytes (a stream under capture is refused); the call's counter comes from the
// library's pool (ptkf::SuppressCounter: nothing is freed, so nothing waits for the device).  The handle's radius
// capture is neither read nor invalidated; no side table is read.
int ptk_suppress_within_self_device(const ptk_tree* t, float radius, const float* d_radii, const float* d_scores,
                                    uint8_t* d_keep, uint32_t* n_rounds, void* stream) {
  if (n_rounds != nullptr) *n_rounds = 0;
  const int rc = check_radius_self(t, radius, d_radii, /*host_values=*/false, d_keep, "suppress_within_self",
                                   "ptk_host_suppress_within_self");
  if (rc != PTK_OK || t->n_points == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  const int crc = ptkf::suppress_check_stream(s);
  if (crc != PTK_OK) return crc;
  return ptkf::suppress_rounds(t->n_points, d_keep, s, n_rounds, [&](uint32_t* d_undecided, bool later_round) {
    return in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) {
      return ptkf::suppress_self(t, first, n, radius, d_radii, d_scores, d_keep, d_undecided, later_round, s);
    });
  });
}

// The host form: the radii and the scores go up, `keep` comes down; n_kept (may be null) counts the keep[i] == 1.
int ptk_suppress_within_self(const ptk_tree* t, float radius, const float* radii, const float* scores, uint8_t* keep,
                             uint64_t* n_kept, uint32_t* n_rounds) {
  if (n_kept != nullptr) *n_kept = 0;
  if (n_rounds != nullptr) *n_rounds = 0;
  int rc = check_radius_self(t, radius, radii, /*host_values=*/true, keep, "suppress_within_self",
                             "ptk_host_suppress_within_self");
  if (rc == PTK_OK) rc = check_scores(scores, t->n_points);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(radii, (size_t)t->n_points * sizeof(float)),
                        ptkio::in_part(scores, (size_t)t->n_points * sizeof(float))};
  const ptkio::Parts out{ptkio::out_part(keep, (size_t)t->n_points)};
  rc = host_form(t, in, out, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_suppress_within_self_device(t, radius, in.at<float>(d_in, 0), in.at<float>(d_in, 1), out.at<uint8_t>(d_out, 0),
                                           n_rounds, s);
  });
  if (rc == PTK_OK && n_kept != nullptr) *n_kept = count_kept(keep, t->n_points);
  return rc;
}

// ---- mst_within_self (ptk.h; the rounds: ptk_kernels_mst.hpp) ------------------------------------------------

int ptk_mst_within_self_workspace(const ptk_tree* t, uint64_t* bytes) {
  if (t == nullptr || bytes == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  *bytes = ptkf::mst_layout(t->n_points, ptkf::mst_branches(t)).bytes;
  return PTK_OK;
}

// Enqueues Boruvka ROUNDS on `stream` until one adds no edge (or the forest is a tree): per round the component table,
// the search over all pieces of leaf positions, the tie, emit and relabel passes.  As suppress_within_self it WAITS on
// the stream once per round and reads 4 bytes (a stream under capture is refused), with the counter of that call's
// pool.  The radius capture is neither read nor invalidated; the count side table is built on first use; everything
// else lives in the caller's workspace.  Test hook mst_skip: 0 = no component table, 1 = the root and the far children
// tested against it, 2 (the default: DESIGN.md section 8 has the measurement) = every near child too.
int ptk_mst_within_self_device(const ptk_tree* t, float radius, const float* d_core, ptk_mst_edge* d_edges, int32_t* d_labels,
                               void* d_workspace, uint64_t workspace_bytes, uint64_t* n_edges, uint32_t* n_rounds,
                               void* stream) {
  if (n_edges != nullptr) *n_edges = 0;
  if (n_rounds != nullptr) *n_rounds = 0;
  int rc = check_mst_self(t, radius, d_edges);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  const ptkf::MstLayout at = ptkf::mst_layout(t->n_points, ptkf::mst_branches(t));
  if (d_workspace == nullptr) return fail(PTK_ERR_INVALID, "mst_within_self: null workspace");
  if (workspace_bytes < at.bytes)
    return fail(PTK_ERR_INVALID, "mst_within_self: the workspace holds %llu bytes, %llu points need %llu (ptk_mst_within_self_workspace)",
                (unsigned long long)workspace_bytes, (unsigned long long)t->n_points, (unsigned long long)at.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  rc = ptkf::suppress_check_stream(s);
  if (rc != PTK_OK) return rc;
  rc = count_table_of(t, s);
  if (rc != PTK_OK) return rc;
  char* ws = static_cast<char*>(d_workspace);
  const uint32_t skip = (uint32_t)std::max(0, std::min(2, knob_int("mst_skip", 2)));
  rc = ptkf::mst_begin(t, ws, s);
  if (rc != PTK_OK) return rc;
  rc = ptkf::mst_rounds(t->n_points, s, n_edges, n_rounds, [&](uint32_t* d_added, uint32_t rounds_before) {
    int r = PTK_OK;
    if (rounds_before > 0 && skip != 0u) r = ptkf::mst_table(t, ws, s);
    if (r == PTK_OK)
      r = in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) {
        return ptkf::mst_search(t, first, n, radius, d_core, ws, skip, rounds_before > 0, s);
      });
    if (r == PTK_OK) r = ptkf::mst_join(t, ws, d_edges, d_added, s);
    return r;
  });
  if (rc == PTK_OK && d_labels != nullptr)
    PTK_HIP(hipMemcpyAsync(d_labels, ws + at.label, (size_t)t->n_points * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return rc;
}

// The host form: one block per call holds core, the edges, the labels and the workspace; core goes up, the edges come
// down and are sorted into the order of the contract, the labels come down.
int ptk_mst_within_self(const ptk_tree* t, float radius, const float* core, ptk_mst_edge* edges, uint64_t* n_edges,
                        int32_t* labels, uint32_t* n_rounds) {
  if (n_edges != nullptr) *n_edges = 0;
  if (n_rounds != nullptr) *n_rounds = 0;
  int rc = check_mst_self(t, radius, edges);
  if (rc == PTK_OK && t != nullptr) rc = check_core(core, t->n_points);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t n = (size_t)t->n_points;
  const size_t o_edges = pad(n * sizeof(float)), o_labels = o_edges + pad(n * sizeof(ptk_mst_edge));
  const size_t o_ws = o_labels + pad(n * sizeof(int32_t));
  const size_t ws_bytes = ptkf::mst_layout(t->n_points, ptkf::mst_branches(t)).bytes;
  DeviceBlock block;
  if (block.alloc(o_ws + ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PTK_ERR_NOMEM, "out of device memory (the edges and the workspace of mst_within_self)");
  }
  char* base = block.as<char>();
  if (core != nullptr) PTK_HIP(hipMemcpy(base, core, n * sizeof(float), hipMemcpyHostToDevice));
  uint64_t count = 0;
  rc = ptk_mst_within_self_device(t, radius, core != nullptr ? reinterpret_cast<const float*>(base) : nullptr,
                                  reinterpret_cast<ptk_mst_edge*>(base + o_edges), reinterpret_cast<int32_t*>(base + o_labels),
                                  base + o_ws, ws_bytes, &count, n_rounds, nullptr);
  // (the block is freed when this returns: everything enqueued on it has to be done -- also after a refusal half-way)
  hipError_t he = hipStreamSynchronize(nullptr);
  if (rc != PTK_OK) return rc;
  if (he == hipSuccess && count > 0) he = hipMemcpy(edges, base + o_edges, (size_t)count * sizeof(ptk_mst_edge), hipMemcpyDeviceToHost);
  if (he == hipSuccess && labels != nullptr) he = hipMemcpy(labels, base + o_labels, n * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (he != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(he));
  static_assert(sizeof(ptk_mst_edge) == sizeof(pico_tree::internal::mst_edge), "record layout");
  pico_tree::internal::mst_sort(reinterpret_cast<pico_tree::internal::mst_edge*>(edges), (size_t)count);
  if (n_edges != nullptr) *n_edges = count;
  return PTK_OK;
}

// ---- normals_within_self (ptk.h; the kernel: ptk_kernels_frames.hpp) ----------------------------------------

// Enqueues frames_self_kernel over ranges of leaf positions: no scratch, nothing allocated, nothing waited for, no side
// table (no shortcut is taken).  The handle's radius capture is neither read nor invalidated.
int ptk_normals_within_self_device(const ptk_tree* t, float radius, const float* d_radii, uint64_t min_neighbors,
                                   const float* viewpoint, ptk_frame* d_frames, ptk_moments* d_moments, void* stream) {
  const int rc = check_normals_self(t, radius, d_radii, /*host_values=*/false, d_frames, d_moments);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  return in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) {
    return ptkf::frames_self(t, first, n, radius, d_radii, min_neighbors, viewpoint, d_frames, d_moments, s);
  });
}

// The host form: only the radii go up, the records come down through the handle's io blocks.
int ptk_normals_within_self(const ptk_tree* t, float radius, const float* radii, uint64_t min_neighbors,
                            const float* viewpoint, ptk_frame* frames, ptk_moments* moments) {
  const int rc = check_normals_self(t, radius, radii, /*host_values=*/true, frames, moments);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(radii, (size_t)t->n_points * sizeof(float))};
  const ptkio::Parts out{ptkio::out_part(frames, (size_t)t->n_points * sizeof(ptk_frame)),
                         ptkio::out_part(moments, (size_t)t->n_points * sizeof(ptk_moments))};
  return host_form(t, in, out, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_normals_within_self_device(t, radius, in.at<float>(d_in, 0), min_neighbors, viewpoint,
                                          out.at<ptk_frame>(d_out, 0), out.at<ptk_moments>(d_out, 1), s);
  });
}

// ---- aggregate_within_self / aggregate_within (ptk.h; the kernels: ptk_kernels_aggregate.hpp) ---------------

// Enqueues aggregate_self_kernel over ranges of leaf positions, one launch per channel window: no scratch, nothing
// allocated, nothing waited for, no side table.  The handle's radius capture is neither read nor invalidated.
int ptk_aggregate_within_self_device(const ptk_tree* t, float radius, const float* d_radii, const float* d_values,
                                     uint32_t channels, uint32_t op, float* d_out, uint64_t* d_counts, void* stream) {
  const int rc = check_aggregate_self(t, radius, d_radii, /*host_values=*/false, d_values, channels, op, d_out);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  return in_batch_pieces(t->n_points, [&](uint64_t first, uint64_t n) {
    return ptkf::aggregate_self(t, first, n, radius, d_radii, d_values, channels, op, d_out, d_counts, s);
  });
}

// The query form: the batch order of ptk_search_count_within_radii_device in a scratch block of the stream's own,
// computed once for every channel window.  It never goes through radius_pass_device (the radius capture stays).
int ptk_aggregate_within_device(const ptk_tree* t, const float* d_q, uint64_t nq, float radius, const float* d_radii,
                                const float* d_values, uint32_t channels, uint32_t op, float* d_out, uint64_t* d_counts,
                                void* stream) {
  int rc = check_aggregate_within(t, d_q, nq, radius, d_radii, /*host_values=*/false, d_values, channels, op, d_out);
  if (rc != PTK_OK || nq == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  Scratch scratch(t, s, /*per_stream=*/true);
  uint32_t* perm = nullptr;
  rc = order_batch(t, d_q, nq, s, scratch, 0, &perm, ptk::kCellsDenseFirst);
  if (rc != PTK_OK) return rc;
  return ptkf::aggregate_within(t, d_q, perm, nq, radius, d_radii, d_values, channels, op, d_out, d_counts, s);
}

// The host-buffer forms: the values, the queries (the query form) and the radii go up, `out` and the counts come down.
int ptk_aggregate_within_self(const ptk_tree* t, float radius, const float* radii, const float* values, uint32_t channels,
                              uint32_t op, float* out, uint64_t* counts) {
  const int rc = check_aggregate_self(t, radius, radii, /*host_values=*/true, values, channels, op, out);
  if (rc != PTK_OK || t->n_points == 0) return rc;
  const uint64_t np = t->n_points;
  const ptkio::Parts in{ptkio::in_part(values, (size_t)np * channels * sizeof(float)), ptkio::in_part(radii, (size_t)np * sizeof(float))};
  const ptkio::Parts res{ptkio::out_part(out, (size_t)np * channels * sizeof(float)), ptkio::out_part(counts, (size_t)np * sizeof(uint64_t))};
  return host_form(t, in, res, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_aggregate_within_self_device(t, radius, in.at<float>(d_in, 1), in.at<float>(d_in, 0), channels, op,
                                            res.at<float>(d_out, 0), res.at<uint64_t>(d_out, 1), s);
  });
}

int ptk_aggregate_within(const ptk_tree* t, const float* q, uint64_t nq, float radius, const float* radii,
                         const float* values, uint32_t channels, uint32_t op, float* out, uint64_t* counts) {
  const int rc = check_aggregate_within(t, q, nq, radius, radii, /*host_values=*/true, values, channels, op, out);
  if (rc != PTK_OK || nq == 0) return rc;
  const ptkio::Parts in{ptkio::in_part(values, (size_t)t->n_points * channels * sizeof(float)),
                        ptkio::in_part(q, (size_t)nq * t->dim * sizeof(float)), ptkio::in_part(radii, (size_t)nq * sizeof(float))};
  const ptkio::Parts res{ptkio::out_part(out, (size_t)nq * channels * sizeof(float)), ptkio::out_part(counts, (size_t)nq * sizeof(uint64_t))};
  return host_form(t, in, res, [&](char* d_in, char* d_out, hipStream_t s) {
    return ptk_aggregate_within_device(t, in.at<float>(d_in, 1), nq, radius, in.at<float>(d_in, 2), in.at<float>(d_in, 0),
                                       channels, op, res.at<float>(d_out, 0), res.at<uint64_t>(d_out, 1), s);
  });
}

// ---- align_step (ptk.h; the kernels: ptk_kernels_align.hpp) --------------------------------------------------

// The inverse of the leaf permutation: built once per handle, on the first align_step, under the handle's own lock (as
// count_table_of).
static int align_inverse_of(const ptk_tree* t, hipStream_t s) {
  std::lock_guard<std::mutex> lock(t->align_inverse_mutex);
  if (t->align_inverse_built) return PTK_OK;
  void* table = nullptr;
  const int rc = ptkf::align_inverse(t, &table, s);
  if (rc != PTK_OK) return rc;
  ptk_tree* m = const_cast<ptk_tree*>(t);
  m->d_align_inverse = table;
  m->device_bytes += t->n_points * sizeof(uint32_t);
  m->align_inverse_built = true;
  return PTK_OK;
}

int ptk_align_step_workspace(const ptk_tree* t, uint64_t nq, uint64_t* bytes) {
  if (t == nullptr || bytes == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  *bytes = ptkf::align_layout(nq).bytes;
  return PTK_OK;
}

// Enqueues the pose kernel, the k = 1 search of q' (ptk_search_knn_device: its pieces, its batch order, its scratch) and
// the levels of the summation tree.  Nothing is allocated and nothing waited for once the handle has its inverse
// permutation.  The radius capture is neither read nor invalidated (a k-NN search never touches it).
int ptk_align_step_device(const ptk_tree* t, const float* d_q, uint64_t nq, const float* transform, float max_distance,
                          const float* d_normals, ptk_align_sums* d_out, ptk_neighbor* d_rows, void* d_workspace,
                          uint64_t workspace_bytes, void* stream) {
  int rc = check_align_step(t, d_q, nq, max_distance, d_out);
  if (rc == PTK_OK) rc = check_search(t, d_q, nq);
  if (rc != PTK_OK) return rc;
  const ptkf::AlignLayout w = ptkf::align_layout(nq);
  if (nq > 0 && d_workspace == nullptr) return fail(PTK_ERR_INVALID, "align_step: null workspace");
  if (workspace_bytes < w.bytes)
    return fail(PTK_ERR_INVALID, "align_step: the workspace holds %llu bytes, %llu rows need %llu (ptk_align_step_workspace)",
                (unsigned long long)workspace_bytes, (unsigned long long)nq, (unsigned long long)w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  if (nq == 0) return ptkf::align_reduce(t, nullptr, nullptr, 0, d_normals, max_distance, nullptr, d_out, s);
  rc = align_inverse_of(t, s);
  if (rc != PTK_OK) return rc;
  char* ws = static_cast<char*>(d_workspace);
  const float* d_qp = d_q;
  if (transform != nullptr) {
    rc = ptkf::align_pose(t, d_q, nq, transform, reinterpret_cast<float*>(ws + w.q), s);
    if (rc != PTK_OK) return rc;
    d_qp = reinterpret_cast<const float*>(ws + w.q);
  }
  ptk_neighbor* rows = d_rows != nullptr ? d_rows : reinterpret_cast<ptk_neighbor*>(ws + w.rows);
  rc = ptk_search_knn_device(t, d_qp, nq, 1, 1.0f, rows, stream);
  if (rc != PTK_OK) return rc;
  return ptkf::align_reduce(t, reinterpret_cast<const ptk::Neighbor*>(rows), d_qp, nq, d_normals, max_distance,
                            ws + w.partials, d_out, s);
}

// The host-buffer form: the queries and the normals go up in the handle's input block (each part on a 256-byte
// boundary); the record, the rows and the workspace live in its output block; the record and, if asked, the rows come down.
int ptk_align_step(const ptk_tree* t, const float* q, uint64_t nq, const float* transform, float max_distance,
                   const float* normals, ptk_align_sums* out, ptk_neighbor* rows) {
  int rc = check_align_step(t, q, nq, max_distance, out);
  if (rc == PTK_OK) rc = check_search(t, q, nq);
  if (rc != PTK_OK) return rc;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t q_bytes = (size_t)nq * 3 * sizeof(float);
  const size_t normal_bytes = normals != nullptr && nq > 0 ? (size_t)t->n_points * 3 * sizeof(float) : 0;
  const size_t row_bytes = (size_t)nq * sizeof(ptk_neighbor);
  const ptkf::AlignLayout w = ptkf::align_layout(nq);
  HostIo& io = t->io;
  std::lock_guard<std::mutex> lock(io.mutex);
  if (io.search[0] == nullptr) PTK_HIP(hipStreamCreateWithFlags(&io.search[0], hipStreamNonBlocking));
  hipStream_t s = io.search[0];
  rc = grow_device_block(&io.d_in, &io.in_capacity, pad(q_bytes) + pad(normal_bytes) + 256);
  if (rc == PTK_OK) rc = grow_device_block(&io.d_out, &io.out_capacity, pad(sizeof(ptk_align_sums)) + pad(row_bytes) + w.bytes);
  if (rc != PTK_OK) return rc;
  char* d_q = io.d_in;
  char* d_normals = d_q + pad(q_bytes);
  auto* d_out = reinterpret_cast<ptk_align_sums*>(io.d_out);
  auto* d_rows = reinterpret_cast<ptk_neighbor*>(io.d_out + pad(sizeof(ptk_align_sums)));
  char* d_ws = io.d_out + pad(sizeof(ptk_align_sums)) + pad(row_bytes);
  if (q_bytes > 0) PTK_HIP(hipMemcpyAsync(d_q, q, q_bytes, hipMemcpyHostToDevice, s));
  if (normal_bytes > 0) PTK_HIP(hipMemcpyAsync(d_normals, normals, normal_bytes, hipMemcpyHostToDevice, s));
  // (an empty batch reads no normals: only the mode is taken from the pointer)
  rc = ptk_align_step_device(t, reinterpret_cast<const float*>(d_q), nq, transform, max_distance,
                             normals != nullptr ? reinterpret_cast<const float*>(d_normals) : nullptr, d_out, d_rows, d_ws,
                             w.bytes, s);
  if (rc != PTK_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  PTK_HIP(hipMemcpyAsync(out, d_out, sizeof(ptk_align_sums), hipMemcpyDeviceToHost, s));
  if (rows != nullptr && nq > 0) PTK_HIP(hipMemcpyAsync(rows, d_rows, row_bytes, hipMemcpyDeviceToHost, s));
  PTK_HIP(hipStreamSynchronize(s));
  return PTK_OK;
}

}  // extern "C"

namespace {

// One pass of the box search over device buffers: count (FILL == false: d_counts[i] = hits of box i)
// or fill (d_offsets = exclusive scan of the counts; row i of d_out in reference traversal order).
template <bool FILL>
int box_pass_device(const ptk_tree* t, const float* d_mn, const float* d_mx, uint64_t nb, uint64_t* d_counts,
                    const uint64_t* d_offsets, int32_t* d_out, hipStream_t s) {
  int rc = check_search(t, d_mn, nb);
  if (rc != PTK_OK) return rc;
  if (nb > 0 && d_mx == nullptr) return fail(PTK_ERR_INVALID, "null box buffer");
  const size_t nd_smem = (size_t)16 * 64 * 8 + (size_t)4 * t->dim * 64 * 4;
  if (t->dim > 3 && nd_smem > t->lds_per_block)
    return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the LDS staging of the device box search", t->dim);
  if (nb == 0) return PTK_OK;
  if (nb >= (1ull << 32)) return fail(PTK_ERR_UNSUPPORTED, "batches of 2^32 or more boxes are not supported");
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  ptk::BoxState root{0, 0, 0, 0, 0, 0};
  {
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (uint32_t d = 0; d < t->dim && d < 3; ++d) {  // dim > 3 hands its root box over in scratch
      mn[d] = t->root_min[d];
      mx[d] = t->root_max[d];
    }
    root = ptk::BoxState{mn[0], mn[1], mn[2], mx[0], mx[1], mx[2]};
  }
  // A topological tree: circle axes (metric_so2: axis 0; metric_se2_squared: axis 2), the four-bound tests.
  const bool topo = topological(t);
  const uint32_t s1_mask = !topo ? 0u : (t->metric.load() == PTK_METRIC_SO2 ? 1u : 4u);
  if (topo && deep_tree(t))  // (the refusal of the k-NN and radius searches of such a tree, in the same words)
    return fail(PTK_ERR_UNSUPPORTED, "tree depth %u is too deep for the device stack", t->max_depth);
  if (topo && t->dev.outer == nullptr)
    return fail(PTK_ERR_UNSUPPORTED, "the box search of this topological tree runs on the host members (kd_tree::search_box)");
  // Boxes in Morton order of their min corners (launch order only; rows stay in the caller's order); the boxes of a
  // deep tree go as they come.
  const bool deep = deep_tree(t);
  const size_t root_bytes = (size_t)2 * t->dim * sizeof(float) + 512;
  Scratch scratch(t, s);
  uint32_t* perm = nullptr;
  rc = deep ? scratch.reserve(root_bytes + deep_plan(t, nb).bytes()) : order_batch(t, d_mn, nb, s, scratch, root_bytes, &perm);
  if (rc != PTK_OK) return rc;
  float* d_root = nullptr;
  if (t->dim > 3) {  // the root box of the any-dimension kernel: min[dim], max[dim]
    d_root = scratch.take<float>((size_t)2 * t->dim);
    if (d_root == nullptr) return fail(PTK_ERR_NOMEM, "scratch block too small");
    PTK_HIP(hipMemcpyAsync(d_root, t->root_min.data(), t->dim * sizeof(float), hipMemcpyHostToDevice, s));
    PTK_HIP(hipMemcpyAsync(d_root + t->dim, t->root_max.data(), t->dim * sizeof(float), hipMemcpyHostToDevice, s));
  }
  const auto* ranges = static_cast<const uint2*>(t->d_ranges);
  // The launch of boxes [lo, lo + n) over either tree view; ovf = the spill capacity of the lanes' stacks (-1: in HBM).
  auto launch = [&](auto ovf, const auto& dev, uint64_t lo, uint64_t n) -> int {
    constexpr int OVF = decltype(ovf)::value;
    const dim3 grid((uint32_t)((n + 63) / 64));
    const float *mn = d_mn + lo * t->dim, *mx = d_mx + lo * t->dim;
    uint64_t* c = FILL ? nullptr : d_counts + lo;
    const uint64_t* of = FILL ? d_offsets + lo : nullptr;
    if constexpr (std::is_same_v<std::decay_t<decltype(dev)>, ptk::DevTreeND>) {
      const int lrc = allow_lds(ptk::box_nd_kernel<16, OVF, FILL>, nd_smem);
      if (lrc != PTK_OK) return lrc;
      hipLaunchKernelGGL((ptk::box_nd_kernel<16, OVF, FILL>), grid, dim3(64), nd_smem, s, dev, ranges, d_root, mn, mx, n, c,
                         of, d_out, perm);
    } else {
      if constexpr (OVF >= 0) {  // (a deep topological tree has been refused above)
        if (topo) {
          hipLaunchKernelGGL((ptk::box_kernel<16, OVF, FILL, true>), grid, dim3(64), 16 * 64 * 8, s, dev, ranges, root, mn,
                             mx, t->dim, n, c, of, d_out, perm, s1_mask);
          return PTK_OK;
        }
      }
      hipLaunchKernelGGL((ptk::box_kernel<16, OVF, FILL>), grid, dim3(64), 16 * 64 * 8, s, dev, ranges, root, mn, mx, t->dim,
                         n, c, of, d_out, perm, 0u);
    }
    return PTK_OK;
  };
  const int kind = FILL ? 3 : 0;
  const uint64_t queries = FILL ? 0 : nb;
  if (deep) {  // record stacks spilling to HBM, a few boxes per launch
    return deep_pieces(t, nb, s, scratch, kind, queries, [&](const auto& dev, uint64_t lo, uint64_t n) {
      return launch(std::integral_constant<int, -1>{}, dev, lo, n);
    });
  }
  Timer timer(t, s);
  rc = with_ovf(t, 16, [&](auto ovf) { return t->dim > 3 ? launch(ovf, t->dev_nd, 0, nb) : launch(ovf, t->dev, 0, nb); });
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipGetLastError());
  timer.stop(kind, queries);
  return PTK_OK;
}

}  // namespace

extern "C" {

int ptk_search_box_count_device(const ptk_tree* t, const float* d_mins, const float* d_maxs, uint64_t nb,
                                uint64_t* d_counts, void* stream) {
  if (nb > 0 && d_counts == nullptr) return fail(PTK_ERR_INVALID, "null counts buffer");
  return box_pass_device<false>(t, d_mins, d_maxs, nb, d_counts, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int ptk_search_box_fill_device(const ptk_tree* t, const float* d_mins, const float* d_maxs, uint64_t nb,
                               const uint64_t* d_offsets, int32_t* d_out, void* stream) {
  if (nb > 0 && (d_offsets == nullptr || d_out == nullptr)) return fail(PTK_ERR_INVALID, "null offsets / output buffer");
  return box_pass_device<true>(t, d_mins, d_maxs, nb, nullptr, d_offsets, d_out, static_cast<hipStream_t>(stream));
}

int ptk_search_box(const ptk_tree* t, const float* mins, const float* maxs, uint64_t nb, uint64_t* offsets,
                   int32_t** out) {
  if (out != nullptr) *out = nullptr;
  if (out == nullptr || offsets == nullptr) return fail(PTK_ERR_INVALID, "null output pointer");
  int rc = check_search(t, mins, nb);
  if (rc != PTK_OK) return rc;
  if (nb > 0 && maxs == nullptr) return fail(PTK_ERR_INVALID, "null box buffer");
  offsets[0] = 0;
  if (nb == 0) return PTK_OK;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  DeviceBlock d_mn, d_mx, d_c, d_o, d_out;
  const size_t bbytes = (size_t)nb * t->dim * sizeof(float);
  hipError_t he = d_mn.alloc(bbytes);
  if (he == hipSuccess) he = d_mx.alloc(bbytes);
  if (he == hipSuccess) he = d_c.alloc((nb + 1) * 8);
  if (he == hipSuccess) he = d_o.alloc((nb + 1) * 8);
  if (he == hipSuccess) he = hipMemcpy(d_mn.p, mins, bbytes, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d_mx.p, maxs, bbytes, hipMemcpyHostToDevice);
  return rows_to_host(
      he, nb, d_c.as<uint64_t>(), d_o.as<uint64_t>(), offsets, out, rows_in<int32_t>(d_out),
      [&](uint64_t* d_counts) {
        return ptk_search_box_count_device(t, d_mn.as<float>(), d_mx.as<float>(), nb, d_counts, nullptr);
      },
      [&](const uint64_t* d_offsets, int32_t* d_rows, uint64_t) {
        return ptk_search_box_fill_device(t, d_mn.as<float>(), d_mx.as<float>(), nb, d_offsets, d_rows, nullptr);
      });
}

void ptk_free(void* p) { std::free(p); }

int ptk_host_alloc(uint64_t bytes, void** out) {
  if (out == nullptr) return fail(PTK_ERR_INVALID, "null out pointer");
  *out = nullptr;
  if (bytes == 0) return PTK_OK;
  if (hipHostMalloc(out, (size_t)bytes, hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return fail(PTK_ERR_NOMEM, "out of pinned host memory (%llu bytes)", (unsigned long long)bytes);
  }
  return PTK_OK;
}

void ptk_host_free(void* p) {
  if (p != nullptr && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}

int ptk_host_register(void* p, uint64_t bytes) {
  if (p == nullptr || bytes == 0) return fail(PTK_ERR_INVALID, "null or empty range");
  if (hipHostRegister(p, (size_t)bytes, hipHostRegisterPortable) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PTK_ERR_NOMEM, "cannot page-lock %llu bytes at %p", (unsigned long long)bytes, p);
  }
  return PTK_OK;
}

int ptk_host_unregister(void* p) {
  if (p == nullptr) return fail(PTK_ERR_INVALID, "null pointer");
  if (hipHostUnregister(p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PTK_ERR_INVALID, "%p is not a registered range", p);
  }
  return PTK_OK;
}

int ptk_debug_knn1_counts(const ptk_tree* t, uint32_t counts[4]) {
  if (t == nullptr || counts == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (t->device < 0) return fail(PTK_ERR_DEVICE, "this handle has no device replica");
  DeviceGuard guard(t->device);
  // The scratch block of the LAST search on the handle's main workspace or on one of its per-stream ones (a k-NN call
  // on a stream of its own uses those): the first that still holds the counters of a two-phase search.
  Workspace* holder = nullptr;
  for (int i = 0; i <= ptk_tree::kExtraWs && holder == nullptr; ++i) {
    Workspace& w = i == 0 ? t->ws : t->extra_ws[i - 1];
    std::lock_guard<std::mutex> lock(w.mutex);
    if (w.last_meta != nullptr) holder = &w;
  }
  if (holder == nullptr) return fail(PTK_ERR_INVALID, "the last search of this handle was not a two-phase k = 1 search");
  std::lock_guard<std::mutex> lock(holder->mutex);
  if (holder->last_meta == nullptr || holder->last_meta_kind != 1)
    return fail(PTK_ERR_INVALID, "the last search of this handle was not a two-phase k = 1 search");
  uint32_t meta[ptk::kMetaWords];
  PTK_HIP(hipDeviceSynchronize());
  PTK_HIP(hipMemcpy(meta, holder->last_meta, sizeof(meta), hipMemcpyDeviceToHost));
  counts[0] = meta[0];
  counts[1] = meta[ptk::kMetaHeavy];
  counts[2] = meta[ptk::kMetaRedo];
  counts[3] = meta[1];
  return PTK_OK;
}

int ptk_debug_knn_coop_counts(const ptk_tree* t, uint32_t counts[7]) {
  if (t == nullptr || counts == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (t->device < 0) return fail(PTK_ERR_DEVICE, "this handle has no device replica");
  DeviceGuard guard(t->device);
  Workspace* holder = nullptr;
  for (int i = 0; i <= ptk_tree::kExtraWs && holder == nullptr; ++i) {
    Workspace& w = i == 0 ? t->ws : t->extra_ws[i - 1];
    std::lock_guard<std::mutex> lock(w.mutex);
    if (w.last_meta != nullptr) holder = &w;
  }
  if (holder == nullptr) return fail(PTK_ERR_INVALID, "the last search of this handle left no counters");
  std::lock_guard<std::mutex> lock(holder->mutex);
  if (holder->last_meta == nullptr || holder->last_meta_kind != 2)
    return fail(PTK_ERR_INVALID, "the last search of this handle was not a capped k > 1 search");
  uint32_t meta[ptk::kMetaWords];
  PTK_HIP(hipDeviceSynchronize());
  PTK_HIP(hipMemcpy(meta, holder->last_meta, sizeof(meta), hipMemcpyDeviceToHost));
  // (a query that found its list full went on in its lane, Handover::full_keeps: the counters run past the lists)
  counts[0] = std::min(meta[ptk::kMetaHeavy], holder->last_meta_cap[0]) +
              std::min(meta[ptk::kMetaHeavyRest], holder->last_meta_cap[1]);
  counts[1] = meta[ptk::kMetaRedo];
  counts[2] = meta[ptk::kKnnWhyPool];
  counts[3] = meta[ptk::kKnnWhyTie];
  counts[4] = meta[ptk::kKnnWhyBox];
  counts[5] = meta[ptk::kKnnWhyRange];
  counts[6] = meta[ptk::kKnnTieSweeps];
  return PTK_OK;
}

int ptk_debug_radius_coop_counts(const ptk_tree* t, uint32_t counts[3]) {
  if (t == nullptr || counts == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (t->device < 0) return fail(PTK_ERR_DEVICE, "this handle has no device replica");
  DeviceGuard guard(t->device);
  std::lock_guard<std::mutex> lock(t->ws.mutex);
  counts[0] = counts[1] = counts[2] = 0;
  if (!t->ws.cap_valid || !t->ws.cap_lists || t->ws.cap_heavy.max_heavy == 0u) return PTK_OK;
  uint32_t meta[ptk::kMetaWords];
  PTK_HIP(hipDeviceSynchronize());
  PTK_HIP(hipMemcpy(meta, t->ws.cap_heavy.meta, sizeof(meta), hipMemcpyDeviceToHost));
  counts[0] = std::min(meta[ptk::kMetaHeavy], t->ws.cap_heavy.max_heavy);
  counts[1] = meta[ptk::kMetaRedo];
  counts[2] = meta[28];  // ptk::kMetaRcEntries (ptk_kernels_coopr.hpp)
  return PTK_OK;
}

int ptk_debug_knn_cap(uint64_t nq, uint32_t k, float e, uint32_t* cap, uint64_t* list_entries) {
  if (cap == nullptr || list_entries == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  *cap = (k > 1 && k <= 64) ? knn_cap(e, nq, k) : 0u;
  *list_entries = *cap != 0u ? knn_max_handover(nq) : 0;
  return PTK_OK;
}

int ptk_debug_piles(const ptk_tree* t, uint64_t out[3]) {
  if (t == nullptr || out == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  if (t->device < 0) return fail(PTK_ERR_DEVICE, "this handle has no device replica");
  out[0] = t->n_piles;
  out[1] = t->pile_points;
  out[2] = knn1_depth(t);
  return PTK_OK;
}

int ptk_debug_create_phases(const ptk_tree* t, double ms[3]) {
  if (t == nullptr || ms == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  for (int i = 0; i < 3; ++i) ms[i] = t->create_ms[i];
  return PTK_OK;
}

int ptk_debug_create_route(const ptk_tree* t, uint64_t counts[8], const char** why) {
  if (t == nullptr || counts == nullptr || why == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  const ptk::BuildRoute& r = t->create_route;
  const uint64_t c[8] = {(uint64_t)r.on_device, r.threshold, r.levels, r.top_branches, r.subtrees, r.slides, r.slide_rounds_device,
                         r.slides_host_whole};
  std::memcpy(counts, c, sizeof(c));
  *why = r.why;
  return PTK_OK;
}

#if defined(PTK_WAVE_TRACE)
// Experiment builds only (tools/wave_trace.py): where the general kernels leave {start, end, hardware id, cycles} of
// every wavefront (device memory, 32 bytes per block of the next launch; null = off).  Not declared in ptk.h.
int ptk_debug_wave_trace(void* d_trace) {
  unsigned long long* p = static_cast<unsigned long long*>(d_trace);
  PTK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ptk::g_wave_trace), &p, sizeof(p)));
  return PTK_OK;
}
int ptk_debug_wave_trace_select(int kernel) {  // which of the k = 1 kernels records (ptk_kernels.hpp, PTK_TRACE_BEGIN_SEL)
  PTK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ptk::g_wave_trace_sel), &kernel, sizeof(kernel)));
  return PTK_OK;
}
#endif

int ptk_debug_batch_order(const ptk_tree* t, int* how) {
  if (t == nullptr || how == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(t->ws.mutex);
  *how = t->ws.last_order;
  if (t->ws.last_verdict != nullptr && t->device >= 0) {  // sampled: what it was found to be is on the device
    DeviceGuard guard(t->device);
    uint32_t coherent = 0;
    PTK_HIP(hipDeviceSynchronize());
    PTK_HIP(hipMemcpy(&coherent, t->ws.last_verdict, 4, hipMemcpyDeviceToHost));
    if (coherent != 0u) *how = 2;
  }
  return PTK_OK;
}

int ptk_debug_deep_pieces(const ptk_tree* t, uint32_t* pieces) {
  if (t == nullptr || pieces == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(t->ws.mutex);
  *pieces = t->ws.last_deep_pieces;
  return PTK_OK;
}

int ptk_debug_batch_permutation(const ptk_tree* t, const float* d_q, uint64_t nq, uint32_t* d_perm) {
  int rc = check_search(t, d_q, nq);
  if (rc != PTK_OK) return rc;
  if (d_perm == nullptr || nq == 0) return fail(PTK_ERR_INVALID, "null permutation buffer or empty batch");
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", t->device);
  // (not order_batch: the permutation of ANY batch, whatever the handle's reorder mode would do with it)
  Scratch scratch(t, nullptr);
  rc = scratch.reserve(permutation_scratch_bytes(nq));
  if (rc != PTK_OK) return rc;
  uint32_t* perm = nullptr;
  rc = make_permutation(t, d_q, nq, nullptr, scratch, &perm);
  if (rc != PTK_OK) return rc;
  PTK_HIP(hipMemcpyAsync(d_perm, perm, nq * sizeof(uint32_t), hipMemcpyDeviceToDevice, nullptr));
  PTK_HIP(hipStreamSynchronize(nullptr));
  return PTK_OK;
}

int ptk_debug_key_bits(const ptk_tree* t, uint64_t nq, uint32_t bits[3]) {
  if (t == nullptr || bits == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  axis_bits(t, morton_bits(nq), bits);
  return PTK_OK;
}

int ptk_profile_enable(ptk_tree* t, int on) {
  if (t == nullptr) return fail(PTK_ERR_INVALID, "null tree");
  std::lock_guard<std::mutex> lock(t->profile.mutex);
  t->profile.enabled = on != 0;
  return PTK_OK;
}

int ptk_profile_get(const ptk_tree* t, ptk_profile* out, int reset) {
  return ptk_profile_get_sized(t, out, sizeof(ptk_profile), reset);
}

int ptk_profile_get_sized(const ptk_tree* t, void* out_bytes, uint64_t size, int reset) {
  if (t == nullptr || out_bytes == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(t->profile.mutex);
  for (PendingEvent& p : t->profile.pending) {
    float ms = 0;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      if (p.kind == 0) {
        t->profile.acc.search_ms += ms;
        t->profile.acc.launches += 1;
        t->profile.acc.queries += p.queries;
      } else if (p.kind == 3) {  // second traversal kernel of the same search
        t->profile.acc.search_ms += ms;
        t->profile.acc.search_tail_ms += ms;
      } else if (p.kind == 1) {
        t->profile.acc.reorder_ms += ms;
      } else {
        t->profile.acc.other_ms += ms;
      }
    }
    t->profile.idle.push_back(p.a);
    if (!p.keep_b) t->profile.idle.push_back(p.b);
  }
  t->profile.pending.clear();
  std::memcpy(out_bytes, &t->profile.acc, (size_t)std::min<uint64_t>(size, sizeof(ptk_profile)));
  if (reset) t->profile.acc = ptk_profile{};
  return PTK_OK;
}


// ---- kd-forest -----------------------------------------------------------------------------

}  // extern "C"

struct ptk_forest {
  uint32_t dim = 0;
  uint64_t n_points = 0;
  uint32_t n_trees = 0;
  int device = kDeviceNone;
  std::vector<float> rotations;       // n_trees x dim
  std::vector<void*> allocations;     // everything to hipFree
  ptk::ForestDev dev{};
  uint32_t* d_dropped = nullptr;
};

namespace {

template <class T>
int forest_upload(ptk_forest* f, const std::vector<T>& host, const T** dev) {
  void* p = nullptr;
  PTK_HIP(hipMalloc(&p, std::max<size_t>(host.size(), 1) * sizeof(T)));
  f->allocations.push_back(p);
  if (!host.empty()) PTK_HIP(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  *dev = static_cast<const T*>(p);
  return PTK_OK;
}

int forest_build(ptk_forest* f, const float* points, uint64_t max_leaf_size, uint64_t seed) {
  const uint64_t n = f->n_points;
  const uint32_t dim = f->dim;
  std::vector<ptk::ForestTreeDev> trees(f->n_trees);
  std::vector<float> rotated;
  for (uint32_t ti = 0; ti < f->n_trees; ++ti) {
    float* r = f->rotations.data() + (size_t)ti * dim;
    ptk::reflection_vector(seed, ti, dim, r);
    ptk::ForestTreeHost host;
    std::string err = ptk::build_forest_tree(points, n, dim, max_leaf_size, r, rotated, host, build_threads());
    if (!err.empty()) return fail(PTK_ERR_UNSUPPORTED, "tree %u: %s", ti, err.c_str());
    std::vector<float> rot(r, r + dim);
    int rc = forest_upload(f, host.nodes, &trees[ti].nodes);
    if (rc == PTK_OK) rc = forest_upload(f, host.indices, &trees[ti].indices);
    if (rc == PTK_OK) rc = forest_upload(f, rot, &trees[ti].rotation);
    if (rc != PTK_OK) return rc;
    trees[ti].root_ref = host.root_ref;
    trees[ti].cbits = host.cbits;
    trees[ti].cmask = (1u << host.cbits) - 1u;
    trees[ti].pad = 0;
  }
  std::vector<float> pts(points, points + n * dim);
  int rc = forest_upload(f, pts, &f->dev.points);
  if (rc == PTK_OK) rc = forest_upload(f, trees, &f->dev.trees);
  if (rc != PTK_OK) return rc;
  void* d = nullptr;
  PTK_HIP(hipMalloc(&d, 4));
  f->allocations.push_back(d);
  PTK_HIP(hipMemset(d, 0, 4));
  f->d_dropped = static_cast<uint32_t*>(d);
  f->dev.n_trees = f->n_trees;
  f->dev.dim = dim;
  return PTK_OK;
}

}  // namespace

extern "C" {

int ptk_forest_create(const float* points, uint64_t n_points, uint32_t dim, uint64_t max_leaf_size,
                      uint32_t forest_size, uint64_t seed, int32_t device, ptk_forest** out) {
  if (out == nullptr) return fail(PTK_ERR_INVALID, "null out pointer");
  *out = nullptr;
  if (points == nullptr) return fail(PTK_ERR_INVALID, "null points");
  if (dim == 0 || n_points == 0 || max_leaf_size == 0 || forest_size == 0)
    return fail(PTK_ERR_INVALID, "dim, n_points, max_leaf_size and forest_size must be positive");
  if (n_points >= (1ull << 31)) return fail(PTK_ERR_INVALID, "n_points must be < 2^31");
  const size_t lds = ((size_t)2 * dim + 2 * ptk::kForestQueue + 2 * ptk::kForestPath) * 4;
  if (lds > 64 * 1024) return fail(PTK_ERR_UNSUPPORTED, "dimension %u does not fit the forest kernel's LDS", dim);
  // (as ptk_tree_create_from_points: before the device lookup, so the refusal does not depend on a GPU)
  if (int rc = check_points_finite(points, n_points, dim); rc != PTK_OK) return rc;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(PTK_ERR_DEVICE, "no HIP device is visible");
  int dev = device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev >= count) return fail(PTK_ERR_INVALID, "device %d out of range (%d visible)", dev, count);
  ptk_forest* f = new (std::nothrow) ptk_forest;
  if (f == nullptr) return fail(PTK_ERR_NOMEM, "out of memory");
  f->dim = dim;
  f->n_points = n_points;
  f->n_trees = forest_size;
  f->device = dev;
  int rc = PTK_OK;
  try {
    f->rotations.resize((size_t)forest_size * dim);
    DeviceGuard guard(dev);
    rc = guard.ok ? forest_build(f, points, max_leaf_size, seed) : fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", dev);
  } catch (const std::bad_alloc&) {
    rc = fail(PTK_ERR_NOMEM, "out of memory");
  } catch (const std::length_error& err) {
    rc = fail(PTK_ERR_UNSUPPORTED, "%s", err.what());
  }
  if (rc != PTK_OK) {
    ptk_forest_destroy(f);
    return rc;
  }
  *out = f;
  return PTK_OK;
}

void ptk_forest_destroy(ptk_forest* f) {
  if (f == nullptr) return;
  if (f->device >= 0) {
    DeviceGuard guard(f->device);
    for (void* p : f->allocations) (void)hipFree(p);
  }
  delete f;
}

int ptk_forest_get_dropped(const ptk_forest* f, uint64_t* dropped) {
  if (f == nullptr || dropped == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  DeviceGuard guard(f->device);
  uint32_t v = 0;
  PTK_HIP(hipMemcpy(&v, f->d_dropped, 4, hipMemcpyDeviceToHost));
  *dropped = v;
  return PTK_OK;
}

int ptk_forest_get_rotations(const ptk_forest* f, float* out) {
  if (f == nullptr || out == nullptr) return fail(PTK_ERR_INVALID, "null argument");
  std::memcpy(out, f->rotations.data(), f->rotations.size() * sizeof(float));
  return PTK_OK;
}

int ptk_forest_search_knn_device(const ptk_forest* f, const float* d_q, uint64_t nq, uint32_t k,
                                 uint64_t max_leaves_visited, ptk_neighbor* d_out, void* stream) {
  if (f == nullptr) return fail(PTK_ERR_INVALID, "null forest");
  if (k == 0 || k > 64) return fail(PTK_ERR_INVALID, "k must be in 1..64");
  if (nq == 0) return PTK_OK;
  if (d_q == nullptr || d_out == nullptr) return fail(PTK_ERR_INVALID, "null buffer");
  if (nq >= (1ull << 31)) return fail(PTK_ERR_UNSUPPORTED, "too many queries for one launch");
  DeviceGuard guard(f->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", f->device);
  const size_t lds = ((size_t)2 * f->dim + 2 * ptk::kForestQueue + 2 * ptk::kForestPath) * 4;
  const uint32_t leaves = max_leaves_visited > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)max_leaves_visited;
  hipLaunchKernelGGL((ptk::forest_knn_kernel<64>), dim3((uint32_t)nq), dim3(64), lds, static_cast<hipStream_t>(stream),
                     f->dev, d_q, nq, k, leaves, reinterpret_cast<ptk::Neighbor*>(d_out), f->d_dropped);
  PTK_HIP(hipGetLastError());
  return PTK_OK;
}

int ptk_forest_search_knn(const ptk_forest* f, const float* q, uint64_t nq, uint32_t k, uint64_t max_leaves_visited,
                          ptk_neighbor* out) {
  if (f == nullptr) return fail(PTK_ERR_INVALID, "null forest");
  if (nq == 0) return PTK_OK;
  if (q == nullptr || out == nullptr) return fail(PTK_ERR_INVALID, "null buffer");
  DeviceGuard guard(f->device);
  if (!guard.ok) return fail(PTK_ERR_DEVICE, "hipSetDevice(%d) failed", f->device);
  float* d_q = nullptr;
  ptk_neighbor* d_out = nullptr;
  const size_t qb = (size_t)nq * f->dim * 4, ob = (size_t)nq * (k ? k : 1) * sizeof(ptk_neighbor);
  hipError_t he = hipMalloc((void**)&d_q, qb);
  if (he == hipSuccess) he = hipMalloc((void**)&d_out, ob);
  if (he == hipSuccess) he = hipMemcpy(d_q, q, qb, hipMemcpyHostToDevice);
  int rc = PTK_OK;
  if (he == hipSuccess) {
    rc = ptk_forest_search_knn_device(f, d_q, nq, k, max_leaves_visited, d_out, nullptr);
    if (rc == PTK_OK) he = hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost);
  }
  if (d_q) (void)hipFree(d_q);
  if (d_out) (void)hipFree(d_out);
  if (rc != PTK_OK) return rc;
  if (he != hipSuccess) return fail(PTK_ERR_DEVICE, "HIP error: %s", hipGetErrorString(he));
  return PTK_OK;
}

}  // extern "C"

#include "ptk_host_loop.hpp"
#include "ptk_multi.hpp"

