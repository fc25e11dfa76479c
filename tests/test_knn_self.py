"""search_knn_self: each tree point's k nearest OTHER points (ptk.h).

Expected rows always come from the compiled reference: its search_knn row of m = min(k + 1, n) entries for each tree
point with one entry removed -- the first whose index is the row's, else the last --, padded with (index -1, distance
FLT_MAX / DBL_MAX): ``expected`` below.  "Drop the first entry" is a different function wherever points coincide; the
"ties" cloud is the one that tells the two apart, and every parametrisation that uses it asserts that it holds rows where
the point is absent from its own (k + 1)-row and rows where it is present but not first (``row_kinds``).

The CPU tier checks the library's host loop (ptk_host_search_knn_self) on a host-only handle, the real source of
knn_self_kernel, self_queries_kernel and drop_self_kernel in the emulator (tests/cpp/emulate_knn_self.cpp) and the
per-point C++ member (tests/cpp/knn_self_main.cpp); the gpu tier checks both routes of the device search, float32 and
float64, and the batched C++ member.
"""

from __future__ import annotations

import ctypes
import functools
import os
import subprocess
import warnings

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import depth_cases, leaf_cases, poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
METRICS = ["L2Squared", "L1", "LPInf", "LNInf"]
#: both sides of every list size of the direct kernel (k + 1 <= 4 / 8 / 16 / 32 / 64), and beyond it
KS_DIRECT = (1, 3, 4, 15, 16, 31, 63)
KS_HOST = (1, 3, 4, 15, 16, 63, 64, 80)

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")
needs_reference64 = pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")


@functools.lru_cache(maxsize=None)
def cloud(kind):
    """(points, leaf size) of a small test cloud (the clouds of tests/test_knn_within.py); shared and read-only."""
    if kind == "uniform":
        p, leaf = ds.uniform_cloud(3_000, 3, 1), 10
    elif kind == "lidar":
        p, leaf = ds.lidar_cloud(4_000, seed=3), 10
    elif kind == "ties":  # coordinates on a coarse grid: many equal distances, piles of coincident points
        p, leaf = (np.round(ds.uniform_cloud(3_000, 3, 5) * 8) / 8).astype(np.float32), 6
    elif kind == "2d":
        p, leaf = ds.uniform_cloud(2_500, 2, 8), 7
    elif kind == "5d":
        p, leaf = ds.uniform_cloud(2_500, 5, 10), 10
    else:
        raise ValueError(kind)
    p = np.ascontiguousarray(p)
    p.flags.writeable = False
    return p, leaf


def expected(ref, p, k):
    n = len(p); m = min(k + 1, n)
    rows = ref.search_knn(p, m)
    hit = rows["index"] == np.arange(n)[:, None]
    has = hit.any(1)
    pos = np.where(has, hit.argmax(1), m - 1)
    keep = np.ones((n, m), bool); keep[np.arange(n), pos] = False
    out = np.zeros((n, k), dtype=rows.dtype); out["index"] = -1
    out["distance"] = np.finfo(rows["distance"].dtype).max
    out[:, :m - 1] = rows[keep].reshape(n, m - 1)
    return out


def row_kinds(ref, p, k):
    """(rows where the point is absent from its (k + 1)-row, rows where it is present but not first)."""
    n = len(p)
    rows = ref.search_knn(p, min(k + 1, n))
    hit = rows["index"] == np.arange(n)[:, None]
    return int((~hit.any(1)).sum()), int((hit.any(1) & ~hit[:, 0]).sum())


@functools.lru_cache(maxsize=None)
def _reference(kind, metric, dtype):
    p, leaf = cloud(kind)
    p = p.astype(dtype)
    return p, oracle.Oracle(p, leaf, "reference", metric=metric, dtype=dtype)


@functools.lru_cache(maxsize=None)
def want_rows(kind, metric, k, dtype=np.float32):
    """expected() of a cloud, computed once per (cloud, metric, k) and shared; read-only."""
    p, ref = _reference(kind, metric, dtype)
    out = expected(ref, p, k)
    out.flags.writeable = False
    return out


def assert_ties_tell_the_rules_apart(metric, ks, dtype=np.float32):
    """Over the k of a parametrisation, "ties" holds rows of both kinds: the rule is not "drop the first entry"."""
    p, ref = _reference("ties", metric, dtype)
    kinds = [row_kinds(ref, p, k) for k in ks]
    assert sum(a for a, _ in kinds) > 0 and sum(b for _, b in kinds) > 0, kinds


def same_rows(got, want):
    """Index and distance bits equal (float64 records carry padding bytes)."""
    got = np.asarray(got).reshape(want.shape)
    return np.array_equal(got["index"], want["index"]) and \
        np.ascontiguousarray(got["distance"]).tobytes() == np.ascontiguousarray(want["distance"]).tobytes()


def host_loop(tree, k):
    out = np.empty((tree.npts, k), dtype=pt.NEIGHBOR)
    out.view(np.uint8).reshape(-1)[:] = 0xA5  # (every slot is written)
    lib = pt._load()
    rc = lib.ptk_host_search_knn_self(tree._h, tree._pts.ctypes.data, k, out.ctypes.data)
    assert rc == 0, lib.ptk_last_error()
    return out


# ---- CPU tier: the host loop on a host-only handle ---------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "2d", "5d"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_equals_the_reference_rows_without_self(kind, metric):
    p, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    if kind == "ties":
        assert_ties_tell_the_rules_apart(metric, KS_HOST)
    for k in KS_HOST:
        assert host_loop(tree, k).tobytes() == want_rows(kind, metric, k).tobytes(), (kind, metric, k)


def test_ties_is_the_cloud_the_issue_counted():
    """The counts the rule was checked with (L2 squared and L+inf alike): rows where the point is absent from its own
    (k + 1)-row / present but not first."""
    if not oracle.have_reference():
        pytest.skip("compiled reference not present")
    for metric in ("L2Squared", "LPInf"):
        p, ref = _reference("ties", metric, np.float32)
        assert [row_kinds(ref, p, k) for k in (1, 3, 4)] == [(1726, 592), (823, 1495), (527, 1791)], metric
        assert row_kinds(ref, p, 15)[1] == 2318 and row_kinds(ref, p, 63)[1] == 2318
    for kind in ("uniform", "lidar"):
        p, ref = _reference(kind, "L2Squared", np.float32)
        assert [row_kinds(ref, p, k) for k in (1, 4, 16)] == [(0, 0)] * 3, kind


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loop_of_the_topological_metrics(metric):
    rng = np.random.default_rng(12)
    p = rng.random((2_000, 1 if metric == "SO2" else 3), dtype=np.float32)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    for k in (1, 4, 16, 80):
        assert host_loop(tree, k).tobytes() == expected(ref, p, k).tobytes(), (metric, k)


def _tiny_expected(p, k):
    """Rows of a tree of n DISTINCT points: the k-NN row of all n points without the row's own, cut or padded to k."""
    n = len(p)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    out = np.empty((n, n), dtype=pt.NEIGHBOR)
    lib = pt._load()
    assert lib.ptk_host_search_knn(tree._h, p.ctypes.data, p.ctypes.data, n, n, np.float32(1.0), out.ctypes.data) == 0
    want = np.zeros((n, k), dtype=pt.NEIGHBOR)
    want["index"], want["distance"] = -1, np.float32(FLT_MAX)
    for i in range(n):
        row = out[i][out[i]["index"] != i]
        assert len(row) == n - 1  # (distinct points: the row holds its own point once)
        want[i, :min(k, n - 1)] = row[:k]
    return want


@pytest.mark.parametrize("n", [1, 2, 9])
def test_host_loop_of_tiny_trees_pads_the_rows(n):
    p = ds.uniform_cloud(n, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    for k in (1, 12):
        got = host_loop(tree, k)
        assert got.tobytes() == _tiny_expected(p, k).tobytes(), (n, k)
        assert np.all(got["index"][:, min(k, n - 1):] == -1)
        assert np.all(got["distance"][:, min(k, n - 1):] == np.float32(FLT_MAX))


def test_argument_checks_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    out = np.empty((9, 4), dtype=pt.NEIGHBOR)
    assert lib.ptk_host_search_knn_self(tree._h, p.ctypes.data, 0, out.ctypes.data) == -1  # PTK_ERR_INVALID
    assert lib.ptk_host_search_knn_self(tree._h, p.ctypes.data, 4, None) == -1
    assert lib.ptk_host_search_knn_self(tree._h, None, 4, out.ctypes.data) == -1
    assert lib.ptk_host_search_knn_self(None, p.ctypes.data, 4, out.ctypes.data) == -1
    # a host-only handle has no device search: PTK_ERR_DEVICE, from every device entry point
    route = ctypes.c_int(0)
    assert lib.ptk_search_knn_self(tree._h, 4, out.ctypes.data) == -3
    assert lib.ptk_search_knn_self_device(tree._h, 4, out.ctypes.data, None) == -3
    assert lib.ptk_debug_self_route(tree._h, 4, ctypes.byref(route)) == -3
    assert lib.ptk_search_knn_self(None, 4, out.ctypes.data) == -1
    assert lib.ptk_version() == 101
    with pytest.raises(pt.PtkError):
        tree.search_knn_self(4)
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    out64 = np.zeros((9, 4), dtype=pt.NEIGHBOR64)
    assert lib.ptk_search64_knn_self(t64._h, 4, out64.ctypes.data) == -3
    assert lib.ptk_search64_knn_self_device(t64._h, 4, out64.ctypes.data, None) == -3


# ---- CPU tier: the real kernel source in the emulator ----------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_self(tmp_path_factory):
    """tests/cpp/emulate_knn_self.cpp, compiled with the emulator's g++ line and HIP stand-in (__graft_entry__.build)."""
    out = str(tmp_path_factory.mktemp("emu_self") / "libptk_emu_self.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_knn_self.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    lib.emu_set_metric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.emu_knn_self.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                 ctypes.c_uint64, ctypes.c_void_p]
    return lib


def emu_rows(lib, p, leaf, metric, k, route, piece=0, ranges=None, largest_leaf=None):
    """(rows n x k, the original indices whose rows were computed): the emulated route over the leaf positions of
    `ranges` (default: all of them).  Rows nobody computed keep the 0xA5 fill.  `largest_leaf`: what the tree handed to
    the emulator must say of its largest leaf."""
    p = np.ascontiguousarray(p)
    host = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    if largest_leaf is not None:
        leaf_cases.assert_leaf(host, largest_leaf)
    nodes, idx, _, _ = host.flat()
    h = lib.emu_create(p.ctypes.data, len(p), p.shape[1], nodes.ctypes.data, len(nodes), idx.ctypes.data)
    assert h
    try:
        lib.emu_set_metric(h, {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}[metric])
        out = np.empty((len(p), k), dtype=pt.NEIGHBOR)
        out.view(np.uint8).reshape(-1)[:] = 0xA5
        done = []
        for lo, hi in ranges or [(0, len(p))]:
            assert lib.emu_knn_self(h, lo, hi, k, route, piece, out.ctypes.data) == 0
            done.append(np.asarray(idx[lo:hi]))
        return out, np.concatenate(done)
    finally:
        lib.emu_destroy(h)


def lattice():
    """Integer lattice points: every point has neighbours at equal distances on all sides."""
    g = np.arange(0, 10, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g[:5], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


@needs_reference
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_emulated_kernels_equal_the_reference_rows_without_self(emu_self, kind, metric):
    ks = (1, 3, 4, 15, 63)
    if kind == "lattice":
        p, leaf = lattice(), 4
        ref = oracle.Oracle(p, leaf, "reference", metric=metric)
        want = {k: expected(ref, p, k) for k in ks + (64, 80)}
    else:
        p, leaf = cloud(kind)
        want = {k: want_rows(kind, metric, k) for k in ks + (64, 80)}
    if kind == "ties":
        assert_ties_tell_the_rules_apart(metric, ks)
    for k in ks:
        # (647 leaf positions per launch: pieces that end inside a wavefront, and a ragged last one)
        for route, piece in ((1, 0), (1, 647), (2, 0), (2, 647)):
            got, _ = emu_rows(emu_self, p, leaf, metric, k, route, piece)
            assert got.tobytes() == want[k].tobytes(), (kind, metric, k, route, piece)
    for k in (64, 80):  # k + 1 beyond the register list: the staged route only
        got, _ = emu_rows(emu_self, p, leaf, metric, k, 2, 1000)
        assert got.tobytes() == want[k].tobytes(), (kind, metric, k)


@needs_reference
def test_emulated_staged_route_in_five_dimensions(emu_self):
    p, leaf = cloud("5d")
    for metric in ("L2Squared", "L1"):
        for k in (1, 4, 16, 80):
            got, _ = emu_rows(emu_self, p, leaf, metric, k, 2, 900)
            assert got.tobytes() == want_rows("5d", metric, k).tobytes(), (metric, k)


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", depth_cases.EUCLID_CASES)
def test_emulated_kernels_where_the_stack_class_changes(emu_self, dim, leaf, metric, depth):
    """Trees of exactly 39 | 40 and 135 | 136 levels (tests/depth_cases.py).  The rows searched are the far pile of
    coincident points -- each of them the "absent" case of the rule as soon as the pile holds more than k + 1 points, and
    the searches that walk the whole chain of one-point peels -- and the 200 leaf positions on either side of it.  The
    record stacks stay within 2 * depth + 2 and within what the host's spill class for the depth holds."""
    pts, pile = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    host = pt.KdTree(pts, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    _, idx, _, _ = host.flat()
    at = np.flatnonzero(np.asarray(idx) >= 3_000)  # leaf positions of the pile
    lo, hi = max(0, int(at.min()) - 200), min(len(pts), int(at.max()) + 201)
    run = depth_cases.Watch(depth, emu_self)
    n_pile = len(pts) - 3_000
    for k in (5, 31, 80):
        want = expected(ref, pts, k)
        if k + 1 < n_pile:  # (more coincident points than the row holds: some of them are not in their own row)
            assert row_kinds(ref, pts, k)[0] > 0, (depth, k)
        for route in ((1, 2) if dim <= 3 and k < 64 else (2,)):
            got, rows = run(emu_rows, emu_self, pts, leaf, metric, k, route, 0, [(lo, hi)])
            assert len(rows) == hi - lo and np.all(np.isin(np.arange(3_000, len(pts)), rows))
            assert got[rows].tobytes() == want[rows].tobytes(), (k, route)


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_kernels_where_the_leaf_scan_changes(emu_self, L):
    """The CPU half of tests/test_leaf_boundaries.py for these kernels: a tree whose largest leaf has exactly 31 | 32 | 33
    and 64 | 65 points, the direct kernel and the staged route in pieces."""
    pts, blob, q, nb, ref, _ = leaf_cases.case(L)
    pts = np.asarray(pts)
    for k in (7, 40):
        want = expected(ref, pts, k)
        for route, piece in ((1, 0), (2, 647)):
            got, _ = emu_rows(emu_self, pts, L, "L2Squared", k, route, piece, largest_leaf=L)
            assert got.tobytes() == want.tobytes(), (L, k, route)


# ---- the C++ members (tests/cpp/knn_self_main.cpp) -------------------------------------------------------------------

def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "knn_self_main.cpp"), "-o", out]
    if host_only:
        cmd.insert(1, "-DPTK_TEST_HOST_ONLY")
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def _cpp_points(d):
    """4 000 points, a fifth of them snapped to a grid (coincident points) -- in [0, 1)^3, so that the third coordinate
    is an angle of the metric_se2_squared tree as well."""
    p = ds.uniform_cloud(4_000, 3, 91)
    p[::5] = np.round(p[::5] * 4) / 4 * np.float32(0.999)
    p.tofile(os.path.join(d, "points.bin"))
    return p


@needs_reference
@needs_reference64
def test_cpp_per_point_member(tmp_path):
    d = str(tmp_path)
    p = _cpp_points(d)
    exe = os.path.join(d, "knn_self_host")
    _cpp_program(exe, host_only=True)
    for k in (1, 9, 70):
        subprocess.check_call([exe, "host", d, str(k)])
        for name, metric, dtype in (("h_l2", "L2Squared", np.float32), ("h_l1", "L1", np.float32),
                                    ("h_linf", "LPInf", np.float32), ("h_l2d", "L2Squared", np.float64)):
            ref = oracle.Oracle(p.astype(dtype), 10, "reference", metric=metric, dtype=dtype)
            want = expected(ref, p.astype(dtype), k)
            got = np.fromfile(os.path.join(d, name + ".bin"), dtype=want.dtype)
            assert same_rows(got, want), (name, k)


# ---- gpu tier ---------------------------------------------------------------------------------------------------

def device_rows(tree, k, route=None):
    """Host rows of the device search into a buffer prefilled with 0xA5 / 0x5A: what both runs agree on was written."""
    pt.set_test_knobs(self_route=route)
    try:
        runs = []
        for byte in (0xA5, 0x5A):
            out = np.empty((tree.npts, k), dtype=tree.dtype_neighbor)
            out.view(np.uint8).reshape(-1)[:] = byte
            got = tree.search_knn_self(k, out)
            assert got is out or k == 1
            runs.append(got.reshape(tree.npts, k))  # (a view: a copy of float64 records would not copy their padding)
        assert poison.same_rows(runs[0], runs[1]), "a slot of the output was not written"
        return runs[0]
    finally:
        pt.set_test_knobs(self_route=None)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "2d"])
@pytest.mark.parametrize("metric", METRICS)
def test_direct_kernel_and_staged_route_equal_the_reference(gpu, kind, metric):
    """2 500 - 4 000 points (a ragged last wavefront), k on both sides of every list size: the direct kernel, and the
    same call through the staged route, byte-equal to each other and to the expected rows."""
    p, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
    if kind == "ties":
        assert_ties_tell_the_rules_apart(metric, KS_DIRECT)
    for k in KS_DIRECT:
        want = want_rows(kind, metric, k)
        assert tree.self_route(k) == 1
        direct = device_rows(tree, k)
        assert direct.tobytes() == want.tobytes(), (kind, metric, k, "direct")
        pt.set_test_knobs(self_route=2)
        assert tree.self_route(k) == 2
        staged = device_rows(tree, k, route=2)
        assert staged.tobytes() == direct.tobytes() == want.tobytes(), (kind, metric, k, "staged")


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind,metric,ks", [("uniform", "L2Squared", (64, 80)), ("lidar", "L1", (64, 80)),
                                           ("5d", "L2Squared", (1, 4, 16, 64, 80)), ("5d", "L1", (1, 16, 80)),
                                           ("5d", "LPInf", (4, 80))])
def test_staged_route_serves_what_the_direct_kernel_does_not(gpu, kind, metric, ks):
    p, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
    for k in ks:
        assert tree.self_route(k) == 2
        assert device_rows(tree, k).tobytes() == want_rows(kind, metric, k).tobytes(), (kind, metric, k)


@pytest.mark.gpu
@needs_reference
def test_pieces_of_leaf_positions(gpu, monkeypatch):
    """self_piece = 640 on 3 000 points: five pieces of the staged route, the last one of 440; PTK_MAX_BATCH = 1 000:
    three ranges of the direct kernel, all ending inside a wavefront."""
    p, leaf = cloud("ties")
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=gpu)
    assert_ties_tell_the_rules_apart("L2Squared", (3, 16))
    for k in (3, 16):
        want = want_rows("ties", "L2Squared", k)
        pt.set_test_knobs(self_piece=640)
        assert device_rows(tree, k, route=2).tobytes() == want.tobytes(), k
        pt.set_test_knobs(self_piece=None)
        monkeypatch.setenv("PTK_MAX_BATCH", "1000")
        assert tree.self_route(k) == 1
        assert device_rows(tree, k).tobytes() == want.tobytes(), k
        assert device_rows(tree, k, route=2).tobytes() == want.tobytes(), k
        monkeypatch.delenv("PTK_MAX_BATCH")
    p5, leaf5 = cloud("5d")
    t5 = pt.KdTree(p5, pt.Metric.L2Squared, leaf5, device=gpu)
    pt.set_test_knobs(self_piece=640)
    assert device_rows(t5, 4).tobytes() == want_rows("5d", "L2Squared", 4).tobytes()


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136, 1031, 1032])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 10, "L2Squared"), (2, 4, "L1"), (3, 10, "LPInf")])
def test_depths_where_the_dispatch_changes(gpu, dim, leaf, metric, depth):
    """The private stack classes (39 | 40, 135 | 136 levels) and the deep class (1 031 | 1 032), which takes the staged
    route; the far pile of coincident points is the "absent" case at depth."""
    pts, _ = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    tree = pt.KdTree(pts, getattr(pt.Metric, metric), leaf, device=gpu)
    depth_cases.assert_depth(tree, depth)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    for k in (5, 31):
        assert row_kinds(ref, pts, k)[0] > 0, (depth, k)
        want = expected(ref, pts, k)
        assert tree.self_route(k) == (2 if depth >= 1032 else 1), (depth, k)
        assert device_rows(tree, k).tobytes() == want.tobytes(), (depth, k)
        if depth < 1032:
            assert device_rows(tree, k, route=2).tobytes() == want.tobytes(), (depth, k, "staged")


@pytest.mark.gpu
@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "ties", "5d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_float64_trees(gpu, kind, metric):
    import torch

    p, leaf = cloud(kind)
    p64 = p.astype(np.float64)
    tree = pt.KdTree(p64, getattr(pt.Metric, metric), leaf, device=gpu)
    ks = (1, 4, 16, 40)
    if kind == "ties":
        assert_ties_tell_the_rules_apart(metric, ks, np.float64)
    for k in ks:
        want = want_rows(kind, metric, k, np.float64)
        assert tree.self_route(k) == 2
        got = device_rows(tree, k)
        assert poison.same_rows(got, want), (kind, metric, k, poison.first_difference(got, want))  # (padding bytes zero)
        raw = torch.full((len(p), k, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=f"cuda:{gpu}")
        dev = tree.search_knn_self(k, raw).numpy()
        torch.cuda.synchronize()
        assert poison.same_rows(dev.reshape(len(p), k), want), (kind, metric, k, "device")
    with pytest.raises(pt.PtkError):
        tree.search_knn_self(0)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_topological_trees_take_the_staged_route(gpu, metric):
    rng = np.random.default_rng(12)
    p = rng.random((2_000, 1 if metric == "SO2" else 3), dtype=np.float32)
    p[::7] = np.round(p[::7] * 8) / 16  # (coincident points)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=gpu)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    for k in (1, 4, 16, 80):
        assert tree.self_route(k) == 2
        assert device_rows(tree, k).tobytes() == expected(ref, p, k).tobytes(), (metric, k)


@pytest.mark.gpu
def test_refusal_of_the_underlying_search_is_passed_on(gpu):
    """A topological tree of the deep stack class: the device k-NN search refuses it (PTK_ERR_UNSUPPORTED), so does the
    staged route -- unchanged --, and under allow_host_loop the host loop serves the call."""
    pts, _ = depth_cases.cloud_at_depth(1032, 3, 4, space="SE2Squared")
    pts = np.asarray(pts)
    tree = pt.KdTree(pts, pt.Metric.SE2Squared, 4, device=gpu)
    with pytest.raises(pt.PtkError) as refused:
        tree.search_knn_self(3)
    with pytest.raises(pt.PtkError) as refused_knn:
        tree.search_knn(pts[:10], 4)
    assert refused.value.status == refused_knn.value.status == pt.PTK_ERR_UNSUPPORTED
    assert str(refused.value) == str(refused_knn.value)
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got = tree.search_knn_self(3)
    finally:
        pt.allow_host_loop(False)
    assert got.tobytes() == host_loop(tree, 3).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 9])
def test_tiny_trees_on_the_device(gpu, n):
    p = ds.uniform_cloud(n, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=gpu)
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=gpu)
    for k in (1, 12, 80):
        want = _tiny_expected(p, k)
        assert tree.self_route(k) == (1 if k < 64 else 2)
        assert device_rows(tree, k).tobytes() == want.tobytes(), (n, k)
        assert device_rows(tree, k, route=2).tobytes() == want.tobytes(), (n, k, "staged")
        got64 = device_rows(t64, k)
        assert np.array_equal(got64["index"], want["index"]), (n, k)
        assert np.all(got64["distance"][want["index"] < 0] == np.finfo(np.float64).max)


@pytest.mark.gpu
@needs_reference
def test_torch_device_form_on_a_side_stream_and_shapes(gpu):
    import torch

    p, leaf = cloud("lidar")
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    for k, route in ((8, 1), (8, 2), (70, 2)):
        want = want_rows("lidar", "L2Squared", k)
        pt.set_test_knobs(self_route=route)
        with torch.cuda.stream(side):
            got = tree.search_knn_self(k, device=True)
            raw = torch.full((len(p), k, 2), 0x5A5A5A5A, dtype=torch.int32, device=f"cuda:{gpu}")
            again = tree.search_knn_self(k, pt.DeviceNeighbors(raw))
        side.synchronize()
        assert isinstance(got, pt.DeviceNeighbors) and again.raw is raw
        assert got.index.shape == (len(p), k)
        assert got.numpy().tobytes() == want.tobytes() and again.numpy().tobytes() == want.tobytes(), (k, route)
    pt.set_test_knobs(self_route=None)
    one = tree.search_knn_self(1)
    assert one.shape == (len(p),) and one.dtype == pt.NEIGHBOR
    assert one.tobytes() == want_rows("lidar", "L2Squared", 1).tobytes()
    assert tree.search_knn_self(1, device=True).numpy().shape == (len(p),)
    for bad in (0, -1):
        with pytest.raises((pt.PtkError, ValueError, OverflowError, ctypes.ArgumentError)):
            tree.search_knn_self(bad)
    lib = pt._load()
    assert lib.ptk_search_knn_self(tree._h, 4, None) == -1
    assert lib.ptk_search_knn_self_device(tree._h, 0, None, None) == -1


@pytest.mark.gpu
def test_other_searches_of_the_handle_are_left_alone(gpu):
    """One call of search_knn, search_knn_within and count_within before and after a self search on the same handle:
    the handle's scratch and capture are as they were."""
    p, q = ds.uniform_cloud(20_000, 3, 71), ds.uniform_cloud(6_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)

    def others():
        return [tree.search_knn(q, 1).tobytes(), tree.search_knn(q, 16).tobytes(),
                tree.search_knn_within(q, 8, 0.002).tobytes(), tree.count_within(q, 0.002).tobytes(),
                tree.search_radius(q, 0.002).flat.tobytes()]

    before = others()
    rows = {}
    for route in (None, 2):
        pt.set_test_knobs(self_route=route)
        rows[route] = [tree.search_knn_self(k).tobytes() for k in (1, 7, 16)]
        assert others() == before, route
    assert rows[None] == rows[2]


@pytest.mark.gpu
@needs_reference
@needs_reference64
def test_cpp_batched_member(gpu, tmp_path):
    d = str(tmp_path)
    p = _cpp_points(d)
    exe = os.path.join(d, "knn_self_batch")
    _cpp_program(exe, host_only=False)
    for k in (1, 9, 70):
        res = subprocess.run([exe, "batch", d, str(k)], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        for name, dtype in (("b_l2", np.float32), ("b_l2d", np.float64)):
            ref = oracle.Oracle(p.astype(dtype), 10, "reference", dtype=dtype)
            want = expected(ref, p.astype(dtype), k)
            assert same_rows(np.fromfile(os.path.join(d, name + ".bin"), dtype=want.dtype), want), (name, k)
