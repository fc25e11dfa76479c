"""search_knn_within: the k nearest points closer than a radius (ptk.h).

Expected rows always come from the compiled reference: its search_knn row of min(k, n) entries, the entries with
distance >= r dropped, the row padded with (index -1, distance r).  The CPU tier checks the library's host loop
(ptk_host_search_knn_within) on a host-only handle, the real source of the bounded kernels in the emulator
(tests/cpp/emulate_knn_within.cpp) and the single-query C++ member (tests/cpp/knn_within_main.cpp); the gpu tier
checks the device searches, float32 and float64, and the batched C++ member.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import depth_cases, leaf_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
KS = (1, 4, 16, 40, 64, 80)

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
    if kind == "self":
        p = ds.uniform_cloud(2_000, 3, 7)
        return p, p[::3].copy(), 8
    if kind == "2d":
        return ds.uniform_cloud(2_500, 2, 8), ds.uniform_cloud(500, 2, 9), 7
    if kind == "5d":
        return ds.uniform_cloud(2_500, 5, 10), ds.uniform_cloud(400, 5, 11), 10
    raise ValueError(kind)


def radii(ref, q, metric):
    """From "no row has a hit" to FLT_MAX: 0, below the nearest distance of every query, the medians of the first
    and of the 16th distance, and FLT_MAX."""
    d = ref.search_knn(q, min(16, ref.n))["distance"]
    nearest = float(d[:, 0].min())
    return [0.0, nearest * 0.5, float(np.median(d[:, 0])), float(np.median(d[:, -1])), FLT_MAX]


def expected(ref, q, k, r):
    kk = min(k, ref.n)
    rows = ref.search_knn(q, kk)
    real = rows["distance"].dtype.type
    out = np.zeros((len(q), k), dtype=rows.dtype)
    out["index"] = -1
    out["distance"] = real(r)
    keep = rows["distance"] < real(r)  # (a prefix of every row: the rows are ascending)
    out[:, :kk][keep] = rows[keep]
    return out


def same_rows(got, want):
    """Index and distance bits equal (float64 records carry padding bytes)."""
    got = got.reshape(want.shape)
    return np.array_equal(got["index"], want["index"]) and \
        np.ascontiguousarray(got["distance"]).tobytes() == np.ascontiguousarray(want["distance"]).tobytes()


def host_loop(tree, q, k, r):
    out = np.empty((len(q), k), dtype=pt.NEIGHBOR)
    lib = pt._load()
    q = np.ascontiguousarray(q)
    rc = lib.ptk_host_search_knn_within(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), k, np.float32(r),
                                        out.ctypes.data)
    assert rc == 0, lib.ptk_last_error()
    return out


# ---- CPU tier: the host loop on a host-only handle ---------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "self", "2d", "5d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_host_loop_equals_the_filtered_reference(kind, metric):
    p, q, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, leaf, "reference", metric=metric)
    for r in radii(ref, q, metric):
        for k in KS:
            got, want = host_loop(tree, q, k, r), expected(ref, q, k, r)
            assert got.tobytes() == want.tobytes(), (kind, metric, k, r)


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loop_of_the_topological_metrics(metric):
    rng = np.random.default_rng(12)
    if metric == "SO2":
        p, q = rng.random((2_000, 1), dtype=np.float32), rng.random((400, 1), dtype=np.float32)
    else:
        p, q = rng.random((2_000, 3), dtype=np.float32), rng.random((400, 3), dtype=np.float32)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    for r in radii(ref, q, metric):
        for k in (1, 4, 40):
            assert host_loop(tree, q, k, r).tobytes() == expected(ref, q, k, r).tobytes(), (metric, k, r)


def test_host_loop_k_beyond_the_tree_and_argument_checks():
    p, q = ds.uniform_cloud(9, 3, 21), ds.uniform_cloud(40, 3, 22)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    got = host_loop(tree, q, 12, FLT_MAX)
    assert np.all(got["index"][:, :9] >= 0) and np.all(got["index"][:, 9:] == -1)
    assert np.all(got["distance"][:, 9:] == np.float32(FLT_MAX))
    assert np.all(np.diff(got["distance"][:, :9], axis=1) >= 0)
    lib = pt._load()
    out = np.empty((len(q), 4), dtype=pt.NEIGHBOR)
    for k, r in ((0, 1.0), (4, -1.0), (4, float("nan"))):
        assert lib.ptk_host_search_knn_within(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), k,
                                              np.float32(r), out.ctypes.data) == -1
    # a host-only handle has no device search
    assert lib.ptk_search_knn_within(tree._h, q.ctypes.data, len(q), 4, np.float32(1.0), out.ctypes.data) < 0


# ---- CPU tier: the real kernel source of the bounded searches in the emulator ----------------------------------------

@pytest.fixture(scope="module")
def emu_within(tmp_path_factory):
    """tests/cpp/emulate_knn_within.cpp, compiled with the emulator's g++ line and HIP stand-in (__graft_entry__.build)."""
    out = str(tmp_path_factory.mktemp("emu_within") / "libptk_emu_within.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_knn_within.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    lib.emu_set_metric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.emu_knn_within.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float,
                                   ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    return lib


def emu_rows(lib, p, leaf, metric, q, k, r, form, largest_leaf=None):
    """Rows of the emulated kernel; `largest_leaf`: what the tree handed to the emulator must say of its largest leaf."""
    host = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    if largest_leaf is not None:
        leaf_cases.assert_leaf(host, largest_leaf)
    nodes, idx, _, _ = host.flat()
    h = lib.emu_create(p.ctypes.data, len(p), p.shape[1], nodes.ctypes.data, len(nodes), idx.ctypes.data)
    assert h
    try:
        lib.emu_set_metric(h, {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}[metric])
        # the bound the backend seeds with (ptk_backend.hip: within_seed)
        with np.errstate(over="ignore"):
            seed = np.float32(r) * np.float32(1 + 2 ** -10)
        if metric in ("LPInf", "LNInf") or not np.isfinite(seed) or (r != 0 and r < np.finfo(np.float32).tiny):
            seed = np.float32(FLT_MAX)
        out = np.empty((len(q), k), dtype=pt.NEIGHBOR)
        q = np.ascontiguousarray(q)
        assert lib.emu_knn_within(h, q.ctypes.data, len(q), k, seed, np.float32(r), form, out.ctypes.data) == 0
        return out
    finally:
        lib.emu_destroy(h)


def lattice():
    """Integer lattice points; queries on lattice points, on half-integer split planes and in the z = 0 face: point
    distances and box distances hit the integer radii exactly."""
    g = np.arange(0, 12, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g[:6], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = np.concatenate([p[::29], p[::31] + np.float32(0.5), p[::37] * np.float32([1, 1, 0])]).astype(np.float32)
    return p, q


@needs_reference
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties", "5d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf"])
def test_emulated_bounded_kernels_equal_the_filtered_reference(emu_within, kind, metric):
    if kind == "lattice":
        p, q = lattice()
        leaf, rs = 4, (0.0, 1.0, 2.0, 3.0, 0.75)
    else:
        p, q, leaf = cloud(kind)
        q = q[:200]
        rs = None
    ref = oracle.Oracle(p, leaf, "reference", metric=metric)
    for r in rs or radii(ref, q, metric):
        for k in (1, 4, 16, 40, 64, 80):
            want = expected(ref, q, k, r)
            for form in ((0, 1, 2) if k <= 64 else (1, 2)):
                got = emu_rows(emu_within, p, leaf, metric, q, k, r, form)
                assert got.tobytes() == want.tobytes(), (kind, metric, k, r, form)


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", depth_cases.EUCLID_CASES)
def test_emulated_bounded_kernels_where_the_stack_class_changes(emu_within, dim, leaf, metric, depth):
    """The CPU half of tests/test_depth_boundaries.py for these kernels (here, where their emulator is built): trees of
    exactly 39 | 40 and 135 | 136 levels, queries that fill the record stacks, the radius at the distance of the pile
    exactly (out: the test is strict), the next number above it (in) and 0.  Rows of the filtered reference, and no
    stack above 2 * depth + 2 records nor above what the host's spill class for the depth holds."""
    pts, pile = depth_cases.cloud_at_depth(depth, dim, leaf)
    q, _ = depth_cases.queries(pts, pile)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    run = depth_cases.Watch(depth, emu_within)
    peak = 0
    for r in depth_cases.edge_radii(ref, q):
        for k in (5, 80):
            want = expected(ref, q, k, r)
            for form in ((0, 1, 2) if k <= 64 else (1, 2)):
                got = run(emu_rows, emu_within, np.asarray(pts), leaf, metric, q, k, r, form)
                assert got.tobytes() == want.tobytes(), (k, r, form)
                peak = max(peak, run.high)
    if metric in ("L2Squared", "L1"):
        # (the sum metrics: the corner queries walk the whole chain; the last radius, 1e4, reaches the cloud as well)
        assert depth_cases.need(depth) - peak <= 8, peak


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_bounded_kernels_where_the_leaf_scan_changes(emu_within, L):
    """The CPU half of tests/test_leaf_boundaries.py for these kernels: a tree whose largest leaf has exactly 31 | 32 | 33
    and 64 | 65 points (the count bits of the leaf reference go 5 -> 6 -> 7), radii that hold a part of that leaf, all of
    it, nothing and the whole tree."""
    pts, blob, q, nb, ref, rs_ = leaf_cases.case(L)
    for r in rs_:
        for k in (5, 80):
            want = expected(ref, q, k, r)
            for form in ((0, 1, 2) if k <= 64 else (1, 2)):
                got = emu_rows(emu_within, np.asarray(pts), L, "L2Squared", q, k, r, form, largest_leaf=L)
                assert got.tobytes() == want.tobytes(), (L, k, r, form)


# ---- the C++ members (tests/cpp/knn_within_main.cpp) ----------------------------------------------------------------

def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "knn_within_main.cpp"), "-o", out]
    if host_only:
        cmd.insert(1, "-DPTK_TEST_HOST_ONLY")
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def _cpp_inputs(d):
    p, q = ds.uniform_cloud(20_000, 3, 91), ds.uniform_cloud(1_500, 3, 92)
    q[:40] = p[:40]  # queries exactly on tree points
    p.tofile(os.path.join(d, "points.bin"))
    q.tofile(os.path.join(d, "queries.bin"))
    return p, q


@needs_reference
@pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")
def test_cpp_single_query_member(tmp_path):
    d = str(tmp_path)
    p, q = _cpp_inputs(d)
    exe = os.path.join(d, "knn_within_host")
    _cpp_program(exe, host_only=True)
    for k, r in ((1, 0.0004), (9, 0.0004), (70, 0.002), (5, 0.0)):
        subprocess.check_call([exe, "host", d, str(k), repr(float(np.float32(r)))])
        for name, metric, dtype in (("h_l2", "L2Squared", np.float32), ("h_l1", "L1", np.float32),
                                    ("h_linf", "LPInf", np.float32), ("h_l2d", "L2Squared", np.float64)):
            ref = oracle.Oracle(p.astype(dtype), 10, "reference", metric=metric, dtype=dtype)
            want = expected(ref, q.astype(dtype), k, np.float32(r))
            got = np.fromfile(os.path.join(d, name + ".bin"), dtype=want.dtype)
            assert same_rows(got, want), (name, k, r)


# ---- gpu tier ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "self", "2d", "5d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_device_equals_the_filtered_reference(gpu, kind, metric):
    import torch

    p, q, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
    ref = oracle.Oracle(p, leaf, "reference", metric=metric)
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    for r in radii(ref, q, metric):
        for k in KS:
            want = expected(ref, q, k, r)
            got = tree.search_knn_within(q, k, r)
            assert got.reshape(len(q), k).tobytes() == want.tobytes(), (kind, metric, k, r)
            dev = tree.search_knn_within(dq, k, r).numpy()
            torch.cuda.synchronize()
            assert dev.reshape(len(q), k).tobytes() == want.tobytes(), (kind, metric, k, r)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 5])
def test_reorder_on_and_off_give_the_same_rows(gpu, dim):
    p, q = ds.uniform_cloud(20_000, dim, 31), ds.uniform_cloud(12_000, dim, 32)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    rows = {}
    for mode in (pt.REORDER_ON, pt.REORDER_OFF):
        tree.set_reorder(mode)
        rows[mode] = [tree.search_knn_within(q, k, 0.004).tobytes() for k in (1, 8, 70)]
    assert rows[pt.REORDER_ON] == rows[pt.REORDER_OFF]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,metric", [(3, "L2Squared"), (3, "L1"), (3, "LPInf"), (5, "L2Squared")])
def test_flt_max_radius_gives_the_search_knn_rows(gpu, dim, metric):
    p, q = ds.uniform_cloud(6_000, dim, 41), ds.uniform_cloud(3_000, dim, 42)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 10, device=gpu)
    for k in KS:
        assert tree.search_knn_within(q, k, FLT_MAX).tobytes() == tree.search_knn(q, k).tobytes(), (dim, metric, k)


@pytest.mark.gpu
def test_zero_radius_is_all_padding_and_k_beyond_the_tree(gpu):
    p, q = ds.uniform_cloud(3_000, 3, 51), ds.uniform_cloud(500, 3, 52)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    for k in (1, 16, 80):
        got = tree.search_knn_within(p[:500], k, 0.0).reshape(500, k)  # (queries ON points: distance 0 is not < 0)
        assert np.all(got["index"] == -1) and np.all(got["distance"] == 0.0)
    small = ds.uniform_cloud(7, 3, 53)
    t7 = pt.KdTree(small, pt.Metric.L2Squared, 3, device=gpu)
    for k in (8, 12, 100):
        got = t7.search_knn_within(q, k, FLT_MAX)
        assert got[:, :7].tobytes() == t7.search_knn(q, 7).tobytes()
        assert np.all(got["index"][:, 7:] == -1) and np.all(got["distance"][:, 7:] == np.float32(FLT_MAX))


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_points_at_exactly_the_radius_are_excluded(gpu, metric):
    """A lattice with queries on split planes and lattice points: distances and box distances hit r exactly."""
    g = np.arange(0, 16, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g[:8], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = np.concatenate([p[::37], p[::53] + np.float32(0.5), p[::41] * np.float32([1, 1, 0])]).astype(np.float32)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 4, device=gpu)
    ref = oracle.Oracle(p, 4, "reference", metric=metric)
    for r in (1.0, 2.0, 3.0, 4.0, 2.25, 0.75):
        for k in (1, 6, 27, 70):
            want = expected(ref, q, k, r)
            assert tree.search_knn_within(q, k, r).reshape(len(q), k).tobytes() == want.tobytes(), (metric, k, r)


@pytest.mark.gpu
@needs_reference
def test_deep_tree_and_batch_pieces(gpu, monkeypatch):
    pts = np.concatenate([ds.uniform_cloud(60_000, 3, 31) - np.float32(0.5), np.zeros((1_500, 3), np.float32)])
    q = np.concatenate([ds.uniform_cloud(3_000, 3, 32) - np.float32(0.5), np.zeros((3, 3), np.float32)])
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    assert tree.info()["max_depth"] > 1_040
    ref = oracle.Oracle(pts, 10, "reference")
    monkeypatch.setenv("PTK_DEEP_SPILL_MB", "16")
    for k in (1, 5, 40, 80):
        for r in (0.0, 1e-4, 2e-3):
            assert tree.search_knn_within(q, k, r).reshape(len(q), k).tobytes() == expected(ref, q, k, r).tobytes()
    monkeypatch.delenv("PTK_DEEP_SPILL_MB")
    p, qq = ds.uniform_cloud(20_000, 3, 33), ds.uniform_cloud(10_000, 3, 34)
    t = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    whole = [t.search_knn_within(qq, k, 0.003).tobytes() for k in (1, 16)]
    monkeypatch.setenv("PTK_MAX_BATCH", "3001")
    assert [t.search_knn_within(qq, k, 0.003).tobytes() for k in (1, 16)] == whole


@pytest.mark.gpu
@needs_reference
def test_duplicated_points(gpu):
    """Coordinates snapped to a grid: a tree with piles of coincident points."""
    p = (np.round(ds.uniform_cloud(50_000, 3, 61) * 4) / 4).astype(np.float32)
    q = ds.uniform_cloud(5_000, 3, 62)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 4, device=gpu)
    assert tree.piles()["piles"] > 0
    ref = oracle.Oracle(p, 4, "reference")
    for k in (1, 10, 70):
        for r in (0.01, 0.07):
            assert tree.search_knn_within(q, k, r).reshape(len(q), k).tobytes() == expected(ref, q, k, r).tobytes()


@pytest.mark.gpu
def test_device_form_on_a_side_stream_and_layouts(gpu):
    import torch

    p, q = ds.uniform_cloud(10_000, 3, 71), ds.uniform_cloud(4_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    want = tree.search_knn_within(q, 8, 0.002)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        dq = torch.from_numpy(q).to(f"cuda:{gpu}", non_blocking=False)
        got = tree.search_knn_within(dq, 8, 0.002)
    side.synchronize()
    assert got.numpy().tobytes() == want.tobytes()
    assert got.index.shape == (len(q), 8)
    fq = np.asfortranarray(q.T)  # column-major queries, (sdim, nq): the (k, nq) layout of search_knn
    col = tree.search_knn_within(fq, 8, 0.002)
    assert col.shape == (8, len(q)) and col.reshape(-1).tobytes() == want.reshape(-1).tobytes()
    assert tree.search_knn_within(q, 1, 0.002).shape == (len(q),)


@pytest.mark.gpu
def test_invalid_arguments_and_topological_metrics(gpu):
    p, q = ds.uniform_cloud(1_000, 3, 81), ds.uniform_cloud(50, 3, 82)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    for k, r in ((0, 1.0), (4, -1.0), (4, float("nan"))):
        with pytest.raises(pt.PtkError):
            tree.search_knn_within(q, k, r)
    rng = np.random.default_rng(3)
    ps, qs = rng.random((2_000, 3), dtype=np.float32), rng.random((100, 3), dtype=np.float32)
    se2 = pt.KdTree(ps, pt.Metric.SE2Squared, 8, device=gpu)
    with pytest.raises(pt.PtkError):
        se2.search_knn_within(qs, 4, 0.01)
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got = se2.search_knn_within(qs, 4, 0.01)
    finally:
        pt.allow_host_loop(False)
    assert got.tobytes() == host_loop(se2, qs, 4, 0.01).tobytes()



@pytest.mark.gpu
@needs_reference
@pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")
def test_cpp_batched_member(gpu, tmp_path):
    d = str(tmp_path)
    p, q = _cpp_inputs(d)
    exe = os.path.join(d, "knn_within_batch")
    _cpp_program(exe, host_only=False)
    for k, r in ((1, 0.0004), (9, 0.0004), (70, 0.002)):
        res = subprocess.run([exe, "batch", d, str(k), repr(float(np.float32(r)))], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        for name, dtype in (("b_l2", np.float32), ("b_l2d", np.float64)):
            ref = oracle.Oracle(p.astype(dtype), 10, "reference", dtype=dtype)
            want = expected(ref, q.astype(dtype), k, np.float32(r))
            assert same_rows(np.fromfile(os.path.join(d, name + ".bin"), dtype=want.dtype), want), (name, k, r)


@pytest.mark.gpu
@pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")
@pytest.mark.parametrize("dim", [3, 6])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf"])
def test_float64_trees_equal_the_filtered_reference(gpu, dim, metric):
    import torch

    p = ds.uniform_cloud(4_000, dim, 101).astype(np.float64) * 1.0000001
    q = ds.uniform_cloud(600, dim, 102).astype(np.float64) * 1.0000001
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 10, device=gpu)
    ref = oracle.Oracle(p, 10, "reference", metric=metric, dtype=np.float64)
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    d = ref.search_knn(q, 16)["distance"]
    for r in (0.0, float(np.median(d[:, 0])), float(np.median(d[:, -1])), 1.7976931348623157e308):
        for k in (1, 4, 16, 40, 64, 80):
            want = expected(ref, q, k, r)
            assert same_rows(tree.search_knn_within(q, k, r), want), (dim, metric, k, r)
            got = tree.search_knn_within(dq, k, r).numpy()
            torch.cuda.synchronize()
            assert same_rows(got, want), (dim, metric, k, r)
    with pytest.raises(pt.PtkError):
        tree.search_knn_within(q, 0, 1.0)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dim,k", [(3, 100), (5, 120)])
def test_list_in_the_output_row(gpu, dim, k):
    """k beyond the LDS budget of the list: knn_within_kernel / knn_nd_within_kernel with the list in the row."""
    p, q = ds.uniform_cloud(5_000, dim, 111), ds.uniform_cloud(700, dim, 112)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    ref = oracle.Oracle(p, 10, "reference")
    d = ref.search_knn(q, k)["distance"]
    for r in (float(np.median(d[:, k // 2])), FLT_MAX):
        assert tree.search_knn_within(q, k, r).tobytes() == expected(ref, q, k, r).tobytes(), (dim, k, r)
