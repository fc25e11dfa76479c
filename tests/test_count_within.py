"""count_within: neighbour counts within a radius, without the rows (ptk.h).

Expected counts always come from the compiled reference: np.diff of its search_radius(q, r) offsets, clamped for
max_count.  The CPU tier checks the library's host loop (ptk_host_search_count_within) on a host-only handle, the real
source of the count kernel and its side table in the emulator (tests/cpp/emulate_count_within.cpp) and the C++ members
(tests/cpp/count_within_main.cpp); the gpu tier checks the device searches, float32 and float64.
"""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import depth_cases, leaf_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")


def cloud(kind):
    """(points, queries, leaf size) of a small test cloud."""
    if kind == "uniform":
        return ds.uniform_cloud(3_000, 3, 1), ds.uniform_cloud(700, 3, 2), 10
    if kind == "lidar":
        return ds.lidar_cloud(4_000, seed=3), ds.lidar_cloud(600, seed=4, pose=(1.5, 0.5)), 10
    if kind == "ties":  # coordinates on a coarse grid: many equal distances, several coincident points
        p = (np.round(ds.uniform_cloud(3_000, 3, 5) * 8) / 8).astype(np.float32)
        q = (np.round(ds.uniform_cloud(500, 3, 6) * 16) / 16).astype(np.float32)
        return p, q, 6
    if kind == "2d":
        return ds.uniform_cloud(2_500, 2, 8), ds.uniform_cloud(500, 2, 9), 7
    if kind == "5d":
        return ds.uniform_cloud(2_500, 5, 10), ds.uniform_cloud(400, 5, 11), 10
    if kind == "lattice":  # integer coordinates: many points exactly at r, queries on split planes
        g = np.arange(0, 12, dtype=np.float32)
        p = np.stack(np.meshgrid(g, g, g[:8], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        q = (np.stack(np.meshgrid(g[::2], g[1::3], g[::3], indexing="ij"), -1).reshape(-1, 3) * 0.5).astype(np.float32)
        return p, q, 4
    raise ValueError(kind)


def radii(ref, q):
    """0, below every nearest distance, the medians of the first and of the 16th distance, FLT_MAX and +inf."""
    d = ref.search_knn(q, min(16, ref.n))["distance"]
    nearest = float(d[:, 0].min())
    return [0.0, nearest * 0.5, float(np.median(d[:, 0])), float(np.median(d[:, -1])), FLT_MAX, INF]


def expected(ref, q, r, max_count=0):
    off, _ = ref.search_radius(q, r)
    c = np.diff(np.asarray(off)).astype(np.int64)
    return np.minimum(c, max_count) if max_count else c


def host_loop(tree, q, r, max_count=0):
    out = np.full(len(q), -7, dtype=np.int64)
    lib = pt._load()
    q = np.ascontiguousarray(q)
    rc = lib.ptk_host_search_count_within(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), np.float32(r),
                                          max_count, out.ctypes.data)
    assert rc == 0, lib.ptk_last_error()
    return out


# ---- CPU tier: the host loop on a host-only handle ---------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "2d", "5d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_host_loop_equals_the_reference(kind, metric):
    p, q, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, leaf, "reference", metric=metric)
    for r in radii(ref, q):
        want = expected(ref, q, np.float32(r))
        for mc in (0, 1, 7):
            assert np.array_equal(host_loop(tree, q, r, mc), np.minimum(want, mc) if mc else want), (kind, metric, r, mc)


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loop_of_the_topological_metrics(metric):
    rng = np.random.default_rng(12)
    dim = 1 if metric == "SO2" else 3
    p, q = rng.random((2_000, dim), dtype=np.float32), rng.random((400, dim), dtype=np.float32)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    for r in radii(ref, q):
        want = expected(ref, q, np.float32(r))
        for mc in (0, 1, 7):
            assert np.array_equal(host_loop(tree, q, r, mc), np.minimum(want, mc) if mc else want), (metric, r, mc)


def test_argument_checks():
    p, q = ds.uniform_cloud(50, 3, 21), ds.uniform_cloud(40, 3, 22)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    out = np.empty(len(q), dtype=np.int64)
    for r in (-1.0, float("nan")):
        assert lib.ptk_host_search_count_within(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), np.float32(r), 0,
                                                out.ctypes.data) == -1
    assert lib.ptk_host_search_count_within(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), np.float32(1.0), 0,
                                            None) == -1
    assert lib.ptk_search_count_within(None, q.ctypes.data, len(q), np.float32(1.0), 0, out.ctypes.data) == -1
    # a host-only handle has no device search
    assert lib.ptk_search_count_within(tree._h, q.ctypes.data, len(q), np.float32(1.0), 0, out.ctypes.data) < 0
    assert host_loop(tree, q[:0], 1.0).shape == (0,)


# ---- CPU tier: the real kernel source in the emulator -------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_count(tmp_path_factory):
    """tests/cpp/emulate_count_within.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_count") / "libptk_emu_count.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_count_within.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    lib.emu_set_metric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.emu_count_within.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_float, ctypes.c_uint64,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


_EMU_METRIC = {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}


def emu_counts(lib, p, leaf, metric, q, r, max_count=0, shortcut=1, tree_points=None, largest_leaf=None):
    """Counts of the emulated kernel; `tree_points`: build the tree over these and search it over `p` (a stream that
    does not belong to its points); `largest_leaf`: what the tree handed to the emulator must say of its largest leaf."""
    host = pt.KdTree(p if tree_points is None else tree_points, getattr(pt.Metric, metric), leaf,
                     device=pt.PTK_DEVICE_NONE)
    if largest_leaf is not None:
        leaf_cases.assert_leaf(host, largest_leaf)
    nodes, idx, _, _ = host.flat()
    h = lib.emu_create(p.ctypes.data, len(p), p.shape[1], nodes.ctypes.data, len(nodes), idx.ctypes.data)
    assert h
    try:
        lib.emu_set_metric(h, _EMU_METRIC[metric])
        out = np.full(len(q), -7, dtype=np.int64)
        stats = np.zeros(3, dtype=np.uint32)
        q = np.ascontiguousarray(q)
        assert lib.emu_count_within(h, q.ctypes.data, len(q), np.float32(r), max_count, shortcut, out.ctypes.data,
                                    stats.ctypes.data) == 0
        return out, stats
    finally:
        lib.emu_destroy(h)


@needs_reference
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties", "lidar", "2d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_emulated_kernel_equals_the_reference(emu_count, kind, metric):
    p, q, leaf = cloud(kind)
    ref = oracle.Oracle(p, leaf, "reference", metric=metric)
    rs = radii(ref, q)
    if kind == "lattice":
        rs += [1.0, 2.0, 4.0, 9.0, 25.0]  # (integer radii: many points exactly at r)
    fired = np.zeros(3, dtype=np.int64)
    for r in rs:
        want = expected(ref, q, np.float32(r))
        for mc in (0, 7):
            got, stats = emu_counts(emu_count, p, leaf, metric, q, r, mc)
            assert np.array_equal(got, np.minimum(want, mc) if mc else want), (kind, metric, r, mc)
            fired += stats
        off, _ = emu_counts(emu_count, p, leaf, metric, q, r, 0, shortcut=0)
        assert np.array_equal(off, want), (kind, metric, r)
    # the large radii take both shortcuts
    assert fired[0] > 0 and fired[1] > 0, fired


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [c for c in depth_cases.EUCLID_CASES if c[0] <= 3])
def test_emulated_kernel_where_the_stack_class_changes(emu_count, dim, leaf, metric, depth):
    """The CPU half of tests/test_depth_boundaries.py for the count kernel (here, where its emulator is built): trees of
    exactly 39 | 40 and 135 | 136 levels, queries that fill the record stacks, the radius at the distance of the pile
    exactly (out: the test is strict), the next number above it (in) and 0; with and without max_count.  Counts of the
    reference, and no stack above 2 * depth + 2 records nor above what the host's spill class for the depth holds."""
    pts, pile = depth_cases.cloud_at_depth(depth, dim, leaf)
    q, _ = depth_cases.queries(pts, pile)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    run = depth_cases.Watch(depth, emu_count)
    at_corner, peak = [], 0
    for r in depth_cases.edge_radii(ref, q):
        want = expected(ref, q, np.float32(r))
        at_corner.append(int(want[0]))
        for mc in (0, 16):
            got, _ = run(emu_counts, emu_count, np.asarray(pts), leaf, metric, q, r, mc)
            assert np.array_equal(got, np.minimum(want, mc) if mc else want), (r, mc)
        got, _ = run(emu_counts, emu_count, np.asarray(pts), leaf, metric, q, r, 0, shortcut=0)
        assert np.array_equal(got, want), (r, "no shortcut")
        peak = max(peak, run.high)
    if metric in ("L2Squared", "L1"):
        # (the sum metrics: the pile is out at r and in just above it, and the corner queries walk the whole chain; under
        # the max and min metrics the traversal prunes by a SUM over the axes, as the reference's does)
        assert at_corner == [0, len(pts) - 3_000, 0, len(pts)], at_corner
        assert depth_cases.need(depth) - peak <= 8, peak


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_kernel_where_the_leaf_scan_changes(emu_count, L):
    """The CPU half of tests/test_leaf_boundaries.py for the count kernel: a tree whose largest leaf has exactly 31 | 32 | 33
    and 64 | 65 points (the count bits of the leaf reference go 5 -> 6 -> 7), radii that hold a part of that leaf, all of
    it, nothing and the whole tree."""
    pts, blob, q, nb, ref, rs_ = leaf_cases.case(L)
    for r in rs_:
        want = expected(ref, q, r)
        for mc in (0, 16):
            got, _ = emu_counts(emu_count, np.asarray(pts), L, "L2Squared", q, r, mc, largest_leaf=L)
            assert np.array_equal(got, np.minimum(want, mc) if mc else want), (L, r, mc)
        got, _ = emu_counts(emu_count, np.asarray(pts), L, "L2Squared", q, r, 0, shortcut=0, largest_leaf=L)
        assert np.array_equal(got, want), (L, r, "no shortcut")
    assert int(want[0]) == len(pts)  # (the last radius holds the whole tree)


@needs_reference
def test_emulated_kernel_never_takes_the_inside_test_at_a_subnormal_radius(emu_count):
    p = np.zeros((200, 3), dtype=np.float32)
    p[:, 0] = np.arange(200, dtype=np.float32) * np.float32(1e-45)
    q = p[::7].copy()
    ref = oracle.Oracle(p, 4, "reference")
    for r in (1e-44, 1e-40, 3e-39):
        got, stats = emu_counts(emu_count, p, 4, "L2Squared", q, r)
        assert np.array_equal(got, expected(ref, q, np.float32(r))), r
        assert stats[0] == 0 and stats[2] > 0, stats  # (the inside test held, and was refused for the radius)


@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_emulated_kernel_on_a_stream_that_does_not_belong_to_its_points(emu_count, metric, move):
    """A tree built over one cloud, searched over a shrunk or shifted copy of it (ptk_tree_create_from_stream checks
    nothing): many splits then lie outside the hull of the points below them, and only the branch bounds in the side
    table's boxes keep the inside test from adding subtrees the reference does not enter completely.  The counts must
    be those of the reference's traversal of that tree and those points: the host loop on the same pair."""
    p_tree, q = ds.uniform_cloud(3_000, 3, 61), ds.uniform_cloud(500, 3, 63)
    p = (p_tree * np.float32(0.5) + np.float32(0.25)) if move == "shrunk" else (p_tree + np.float32(0.3))
    p = np.ascontiguousarray(p, dtype=np.float32)
    host = pt.KdTree(p_tree, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    inside = 0
    for r in (0.001, 0.01, 0.05, 0.1, 0.3, 1.0, FLT_MAX):
        got, stats = emu_counts(emu_count, p, 8, metric, q, r, tree_points=p_tree)
        inside += int(stats[0])
        want = np.empty(len(q), dtype=np.int64)
        assert lib.ptk_host_search_count_within(host._h, p.ctypes.data, q.ctypes.data, len(q), np.float32(r), 0,
                                                want.ctypes.data) == 0
        assert np.array_equal(got, want), (metric, move, r)
    assert inside > 0


@pytest.fixture(scope="module")
def emu64_count(emu_count):
    lib = emu_count
    lib.emu64_create.restype = ctypes.c_void_p
    lib.emu64_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
    lib.emu64_destroy.argtypes = [ctypes.c_void_p]
    lib.emu64_set_metric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.emu64_count_within.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double,
                                       ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@needs_reference
@pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties", "lidar", "2d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_emulated_float64_kernel_equals_the_reference(emu64_count, kind, metric):
    lib = emu64_count
    p, q, leaf = cloud(kind)
    p, q = p.astype(np.float64) * 1.0000001, np.ascontiguousarray(q.astype(np.float64))
    ref = oracle.Oracle(p, leaf, "reference", metric=metric, dtype=np.float64)
    h = lib.emu64_create(p.ctypes.data, len(p), p.shape[1], leaf)
    assert h
    try:
        lib.emu64_set_metric(h, _EMU_METRIC[metric])
        rs = radii(ref, q) + ([1.0, 2.0, 4.0, 9.0, 25.0] if kind == "lattice" else [])
        fired = np.zeros(3, dtype=np.int64)
        for r in rs:
            want = expected(ref, q, r)
            for mc, sc in ((0, 1), (7, 1), (0, 0)):
                out = np.full(len(q), -7, dtype=np.int64)
                stats = np.zeros(3, dtype=np.uint32)
                assert lib.emu64_count_within(h, q.ctypes.data, len(q), r, mc, sc, out.ctypes.data, stats.ctypes.data) == 0
                assert np.array_equal(out, np.minimum(want, mc) if mc else want), (kind, metric, r, mc, sc)
                fired += stats
        assert fired[0] > 0 and fired[1] > 0, fired
    finally:
        lib.emu64_destroy(h)


# ---- the C++ members (tests/cpp/count_within_main.cpp) ----------------------------------------------------------------

def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "count_within_main.cpp"), "-o", out]
    if host_only:
        cmd.insert(1, "-DPTK_TEST_HOST_ONLY")
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def _cpp_check(exe, d, mode):
    p, q = ds.uniform_cloud(20_000, 3, 91), ds.uniform_cloud(1_500, 3, 92)
    q[:40] = p[:40]  # queries exactly on tree points
    p.tofile(os.path.join(d, "points.bin"))
    q.tofile(os.path.join(d, "queries.bin"))
    for r in (0.0, 0.0004, 0.002, 0.05):
        subprocess.check_call([exe, mode, d, repr(float(np.float32(r)))])
        for name, metric, dtype in (("l2", "L2Squared", np.float32), ("l1", "L1", np.float32),
                                    ("linf", "LPInf", np.float32), ("l2d", "L2Squared", np.float64)):
            ref = oracle.Oracle(p.astype(dtype), 10, "reference", metric=metric, dtype=dtype)
            want = expected(ref, q.astype(dtype), dtype(np.float32(r)))
            got = np.fromfile(os.path.join(d, name + ".bin"), dtype=np.uint64).astype(np.int64)
            assert np.array_equal(got, want), (mode, name, r)
            if mode == "device":
                got16 = np.fromfile(os.path.join(d, name + "_16.bin"), dtype=np.uint64).astype(np.int64)
                assert np.array_equal(got16, np.minimum(want, 16)), (name, r)


@needs_reference
@pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")
def test_cpp_single_query_member(tmp_path):
    d = str(tmp_path)
    exe = os.path.join(d, "count_within_host")
    _cpp_program(exe, host_only=True)
    _cpp_check(exe, d, "host")


# ---- gpu tier ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "2d", "5d", "lattice"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_device_equals_the_reference(gpu, kind, metric):
    import torch

    p, q, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
    ref = oracle.Oracle(p, leaf, "reference", metric=metric)
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    for r in radii(ref, q):
        want = expected(ref, q, np.float32(r))
        for mc in (0, 1, 7):
            w = np.minimum(want, mc) if mc else want
            assert np.array_equal(tree.count_within(q, r, mc), w), (kind, metric, r, mc)
            dev = tree.count_within(dq, r, mc)
            torch.cuda.synchronize()
            assert dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), w), (kind, metric, r, mc)
        assert np.array_equal(tree.count_within(q.T, r), want)  # (column-major: the (sdim, nq) view)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_device_topological_metrics(gpu, metric):
    rng = np.random.default_rng(12)
    dim = 1 if metric == "SO2" else 3
    p, q = rng.random((3_000, dim), dtype=np.float32), rng.random((700, dim), dtype=np.float32)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=gpu)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    for r in radii(ref, q)[:5]:
        want = expected(ref, q, np.float32(r))
        assert np.array_equal(tree.count_within(q, r), want), (metric, r)
        assert np.array_equal(tree.count_within(q, r, 7), np.minimum(want, 7)), (metric, r)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dim", [3, 6])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_device_float64_equals_the_reference(gpu, dim, metric):
    import torch

    p, q = ds.uniform_cloud(4_000, dim, 71).astype(np.float64), ds.uniform_cloud(900, dim, 72).astype(np.float64)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 10, device=gpu)
    ref = oracle.Oracle(p, 10, "reference", metric=metric, dtype=np.float64)
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    for r in radii(ref, q):
        want = expected(ref, q, r)
        assert np.array_equal(tree.count_within(q, r), want), (dim, metric, r)
        assert np.array_equal(tree.count_within(q, r, 7), np.minimum(want, 7)), (dim, metric, r)
        dev = tree.count_within(dq, r)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), want), (dim, metric, r)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("nq", [1, 33, 64, 10_000])
def test_batch_sizes_reorder_and_shortcut_off(gpu, nq, monkeypatch):
    p, q = ds.lidar_cloud(60_000, seed=81), ds.lidar_cloud(nq, seed=82, pose=(2.0, 1.0))
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    ref = oracle.Oracle(p, 10, "reference")
    for r in (0.05, 1.0, 16.0):
        want = expected(ref, q, np.float32(r))
        for mode in (pt.REORDER_ON, pt.REORDER_OFF):
            tree.set_reorder(mode)
            assert np.array_equal(tree.count_within(q, r), want), (nq, r, mode)
        monkeypatch.setenv("PTK_TEST_KNOBS", "count_shortcut=0")
        assert np.array_equal(tree.count_within(q, r), want), (nq, r)
        monkeypatch.delenv("PTK_TEST_KNOBS")


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["piles", "5d"])
def test_fallbacks_equal_the_reference(gpu, kind):
    if kind == "piles":  # thousands of coincident points: a tree of the deep stack class
        rng = np.random.default_rng(5)
        p = np.concatenate([np.repeat(rng.random((3, 3), dtype=np.float32), 4_000, axis=0),
                            rng.random((2_000, 3), dtype=np.float32)])
        q = rng.random((500, 3), dtype=np.float32)
    else:
        p, q = ds.uniform_cloud(5_000, 5, 85), ds.uniform_cloud(700, 5, 86)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 1 if kind == "piles" else 10, device=gpu)
    if kind == "piles":  # (the deep stack class: 2 * depth + 2 beyond the private spill slots)
        assert tree.info()["max_depth"] > 1031, tree.info()
    ref = oracle.Oracle(p, 1 if kind == "piles" else 10, "reference")
    for r in (0.001, 0.05, 0.5):
        want = expected(ref, q, np.float32(r))
        assert np.array_equal(tree.count_within(q, r), want), (kind, r)
        assert np.array_equal(tree.count_within(q, r, 16), np.minimum(want, 16)), (kind, r)


@pytest.mark.gpu
@needs_reference
def test_non_finite_query_rows(gpu):
    p = ds.lidar_cloud(50_000, seed=91)
    q = ds.lidar_cloud(100_000, seed=92, pose=(1.0, 2.0))
    rng = np.random.default_rng(93)
    rows = rng.choice(len(q), 3_000, replace=False)
    vals = np.array([np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX], dtype=np.float32)
    q[rows, rng.integers(0, 3, len(rows))] = vals[rng.integers(0, len(vals), len(rows))]
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    ref = oracle.Oracle(p, 10, "reference")
    for r in (0.5, 4.0, INF):
        assert np.array_equal(tree.count_within(q, r), expected(ref, q, np.float32(r))), r


@pytest.mark.gpu
def test_count_within_leaves_the_radius_capture_alone(gpu):
    import torch

    lib = pt._load()
    p, q = ds.lidar_cloud(200_000, seed=95), ds.lidar_cloud(50_000, seed=96, pose=(1.0, 0.5))
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    dev = f"cuda:{gpu}"
    dq = torch.from_numpy(q).to(dev)
    nq, r = len(q), np.float32(1.0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fill(counts, between):
        offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        total = int(offsets[-1])
        out = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
        between()
        torch.cuda.synchronize()
        assert lib.ptk_profile_get(tree._h, ctypes.byref(prof), 1) == 0  # (reset)
        assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), nq, r, np.float32(1.0), offsets.data_ptr(),
                                                 out.data_ptr(), 1, stream) == 0
        torch.cuda.synchronize()
        assert lib.ptk_profile_get(tree._h, ctypes.byref(prof), 1) == 0
        return out[:total].cpu().numpy().tobytes(), int(prof.queries)

    prof = pt._Profile()
    assert lib.ptk_profile_enable(tree._h, 1) == 0
    rows = {}
    for with_count in (False, True):
        counts = torch.zeros(nq, dtype=torch.int64, device=dev)
        assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), nq, r, np.float32(1.0), counts.data_ptr(),
                                                  stream) == 0
        # (another batch pointer and another radius: a count_within that went through the radius count pass would
        # replace the capture, and the fill would have to search again)
        between = (lambda: (tree.count_within(dq.clone(), 2.0), tree.count_within(dq[: nq // 2], r))) if with_count \
            else (lambda: None)
        rows[with_count], searched = fill(counts, between)
        assert searched == 0, (with_count, searched)  # served from the capture
    assert rows[True] == rows[False]
    # a fill that has no capture to be served from searches again
    counts = torch.zeros(nq, dtype=torch.int64, device=dev)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), nq, r, np.float32(1.0), counts.data_ptr(),
                                              stream) == 0
    other = dq.clone()
    _, searched = fill(counts, lambda: lib.ptk_search_radius_count_device(
        tree._h, other.data_ptr(), nq, r, np.float32(1.0), torch.zeros(nq, dtype=torch.int64, device=dev).data_ptr(),
        stream))
    assert searched == nq


@pytest.mark.gpu
@needs_reference
@pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")
def test_cpp_batched_member(gpu, tmp_path):
    d = str(tmp_path)
    exe = os.path.join(d, "count_within_device")
    _cpp_program(exe, host_only=False)
    _cpp_check(exe, d, "device")


@pytest.mark.gpu
def test_full_size_config3(gpu):
    """BASELINE config 3 (7.73 M points, 7.20 M queries, r = 1.0): the counts of ptk_search_radius_count_device, which
    the SHA test pins to the reference, and their clamp for max_count = 16."""
    import torch

    lib = pt._load()
    p, q = ds.config2_clouds("L")
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    want = torch.zeros(len(q), dtype=torch.int64, device=dq.device)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), len(q), np.float32(1.0), np.float32(1.0),
                                              want.data_ptr(), torch.cuda.current_stream(dq.device).cuda_stream) == 0
    got = tree.count_within(dq, 1.0)
    got16 = tree.count_within(dq, 1.0, 16)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(got16, torch.clamp(want, max=16))
