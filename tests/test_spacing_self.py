"""spacing_knn_self: k-NN spacing and statistical outlier removal of a tree's own points (ptk.h).

Expected values never come from the feature.  ``restate`` below is the contract in numpy over the rows that
tests/test_knn_self.py expects of search_knn_self (the compiled reference's rows with the contract's drop rule):
column-by-column adds in the tree's dtype, ``np.sqrt``, one division, and tests/test_align_step.py's ``tree_sum`` for the
two sums of the record.  Every comparison is equality of bytes: mean, kth, keep and the 64-byte record.  Outputs are
filled with two different byte patterns before two runs of every call; what both runs agree on was written.

The CPU tier checks the library's host loop (ptk_host_spacing_knn_self) on host-only handles and the argument checks; the
gpu tier checks both routes of the device search, float32 and float64, the statistics kernels and the torch device form.

The overflow case.  Eight points on a line at spacing 1.2e19 (squared: 1.44e38) cannot show a finite row with an
infinite mean: the second neighbour of a point lies at squared distance 5.76e38 > FLT_MAX, is never accepted, and the
rows hold at most two entries whose sum, 2.88e38, is finite.  That cloud is kept for the equality of bits; the property
is asserted on a line at spacing 8.5e18 (squared 7.2e37: the 2-step entry 2.9e38 is finite, the row sum 4.3e38 is not)
with four ordinary points beside it, so that valid and invalid points meet in one record (``overflow_cloud``).
"""

from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import depth_cases, leaf_cases
from tests.test_align_step import tree_sum
from tests.test_knn_self import KS_DIRECT, KS_HOST, METRICS, _cpp_points, cloud, expected, lattice, want_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = ctypes.c_float
INVALID, UNSUPPORTED, DEVICE = -1, -2, -3
SQRT = pt.PTK_SPACING_SQRT

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")
needs_reference64 = pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")


# ---- the contract in numpy -------------------------------------------------------------------------------------------

def restate(rows, flags, ratio):
    """(mean, kth, keep, record) of the contract over `rows` (n x k records of search_knn_self)."""
    rows = np.asarray(rows)
    n, k = rows.shape
    d = np.ascontiguousarray(rows["distance"])
    real = d.dtype.type
    fmax = np.finfo(d.dtype).max
    ok = d < fmax
    m = ok.sum(1)
    assert np.array_equal(ok, np.arange(k)[None, :] < m[:, None])  # (they are the first m entries)
    with np.errstate(over="ignore", invalid="ignore"):
        dd = np.sqrt(d) if flags & SQRT else d
        assert dd.dtype == d.dtype
        s = np.zeros(n, dtype=d.dtype)
        for j in range(k):
            s = np.where(ok[:, j], s + dd[:, j], s)
        mean = np.where(m > 0, s / np.maximum(m, 1).astype(d.dtype), fmax).astype(d.dtype)
        kth = np.where(m > 0, dd[np.arange(n), np.maximum(m, 1) - 1], fmax).astype(d.dtype)
        valid = (m > 0) & (mean - mean == 0)
    x = np.where(valid, mean.astype(np.float64), 0.0)
    rec = np.zeros((), dtype=pt.SPACING_STATS)
    rec["count"], rec["rows"] = int(valid.sum()), n
    rec["sum"] = tree_sum(x[:, None])[0][0]
    rec["mean"] = rec["sum"] / np.float64(int(rec["count"])) if rec["count"] > 0 else 0.0
    e = x - rec["mean"]
    rec["ssd"] = tree_sum(np.where(valid, e * e, 0.0)[:, None])[0][0]
    rec["variance"] = rec["ssd"] / np.float64(int(rec["count"]) - 1) if rec["count"] > 1 else 0.0
    rec["ratio_squared"] = np.float64(np.float32(ratio)) * np.float64(np.float32(ratio))
    keep = valid & ((e <= 0.0) | (e * e <= rec["ratio_squared"] * rec["variance"]))
    assert real is mean.dtype.type
    return mean, kth, keep.astype(np.uint8), rec


def same(got, want, what=""):
    """All four outputs, byte for byte."""
    for name, g, w in zip(("mean", "kth", "keep", "record"), got, want):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes(), (what, name, _first_difference(g, w))


def _first_difference(g, w):
    g, w = np.atleast_1d(np.asarray(g)), np.atleast_1d(np.asarray(w))
    if g.shape != w.shape:
        return f"shapes {g.shape} / {w.shape}"
    if g.dtype.names:
        return f"{g} / {w}"
    bad = np.flatnonzero(~((g == w) | ((g != g) & (w != w))))
    return f"{len(bad)} cells, first {bad[:3]}: {g[bad[:3]]} / {w[bad[:3]]}"


# ---- calling the library ---------------------------------------------------------------------------------------------

def call(tree, k, flags, ratio, how, kth=True, keep=True, stats=True):
    """(mean, kth, keep, record) of one entry point -- `how`: "loop" (ptk_host_spacing_knn_self) or "device" (the
    host-buffer form of the device search).  Every output is prefilled with 0xA5, then with 0x5A: what the two runs agree
    on was written.  An output that is not asked for is passed as NULL and comes back as None."""
    lib = pt._load()
    n, real = tree.npts, tree._real
    runs = []
    for byte in (0xA5, 0x5A):
        bufs = [np.empty(n, dtype=real), np.empty(n, dtype=real) if kth else None,
                np.empty(n, dtype=np.uint8) if keep else None, np.empty(1, dtype=pt.SPACING_STATS) if stats else None]
        for b in bufs:
            if b is not None:
                b.view(np.uint8).reshape(-1)[:] = byte
        ptrs = [b.ctypes.data if b is not None else None for b in bufs]
        if how == "loop":
            rc = lib.ptk_host_spacing_knn_self(tree._h, tree._pts.ctypes.data, k, flags, F32(ratio), *ptrs)
        else:
            fn = lib.ptk_search64_spacing_knn_self if tree._f64 else lib.ptk_spacing_knn_self
            rc = fn(tree._h, k, flags, F32(ratio), *ptrs)
        assert rc == 0, lib.ptk_last_error()
        runs.append(bufs)
    for a, b in zip(*runs):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), "a cell of an output was not written"
    out = runs[0]
    return out[0], out[1], out[2], out[3][0] if out[3] is not None else None


# ---- CPU tier: the host loop on a host-only handle ---------------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "2d", "5d"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_equals_the_contract(kind, metric):
    p, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    for k in KS_HOST:
        rows = want_rows(kind, metric, k)
        for flags in (0, SQRT):
            same(call(tree, k, flags, 1.0, "loop"), restate(rows, flags, 1.0), (kind, metric, k, flags))


def _topological_points(metric):
    rng = np.random.default_rng(12)
    p = rng.random((2_000, 1 if metric == "SO2" else 3), dtype=np.float32)
    p[::7] = np.round(p[::7] * 8) / 16  # (coincident points)
    return p


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loop_of_the_topological_metrics(metric):
    p = _topological_points(metric)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    for k in (1, 4, 16, 80):
        rows = expected(ref, p, k)
        for flags in (0, SQRT):
            same(call(tree, k, flags, 2.0, "loop"), restate(rows, flags, 2.0), (metric, k, flags))


def _tiny_rows(p, k):
    """Rows of a tree of n DISTINCT points from a brute-force table in the points' dtype (stable order by distance, then
    index does not matter: the points are random, the distances distinct)."""
    n = len(p)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).astype(p.dtype)
    d = (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]
    rows = np.zeros((n, k), dtype=pt.NEIGHBOR64 if p.dtype == np.float64 else pt.NEIGHBOR)
    rows["index"], rows["distance"] = -1, np.finfo(p.dtype).max
    for i in range(n):
        others = [j for j in np.argsort(d[i], kind="stable") if j != i][:k]
        rows["index"][i, :len(others)] = others
        rows["distance"][i, :len(others)] = d[i, others]
    return rows


def _tiny_checks(got, n):
    mean, kth, keep, rec = got
    fmax = np.finfo(np.float32).max
    if n == 1:  # no neighbour: m = 0
        assert mean[0] == fmax and kth[0] == fmax and keep[0] == 0 and rec["count"] == 0 and rec["mean"] == 0.0
    assert rec["rows"] == n and rec["count"] == (0 if n == 1 else n)
    if n <= 1:
        assert rec["variance"].tobytes() == np.float64(0.0).tobytes()


@pytest.mark.parametrize("n", [1, 2, 9])
def test_host_loop_of_tiny_trees(n):
    p = ds.uniform_cloud(n, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    for k in (1, 12):
        got = call(tree, k, SQRT, 2.0, "loop")
        same(got, restate(_tiny_rows(p, k), SQRT, 2.0), (n, k))
        _tiny_checks(got, n)
    # two coincident points: one valid mean of 0 each, count 2, variance +0, both kept at ratio 0
    q = np.zeros((2, 3), dtype=np.float32)
    got = call(pt.KdTree(q, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE), 1, 0, 0.0, "loop")
    assert got[3]["count"] == 2 and got[3]["variance"] == 0.0 and got[2].tolist() == [1, 1]
    _count_one_checks(call(pt.KdTree(count_one_cloud(), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE), 2, 0, 2.0, "loop"))


def count_one_cloud():
    """Three collinear points at 0 and +-d, d * d = 7.9e37, for k = 2 without the flag: the middle point's row sums to
    1.6e38; an outer point's row holds d * d and 4 d * d = 3.2e38, both finite, whose sum is not.  One valid point."""
    p = np.zeros((3, 3), dtype=np.float32)
    p[:, 0] = np.float32(8.9e18) * np.array([-1, 0, 1], dtype=np.float32)
    return p


def _count_one_checks(got):
    """count == 1: the mean is the one valid x, ssd and variance are +0 (count - 1 == 0 divides nothing)."""
    same(got, restate(_line_rows(count_one_cloud(), 2), 0, 2.0), "count == 1")
    mean, kth, keep, rec = got
    assert np.isinf(mean[[0, 2]]).all() and np.isfinite(kth).all() and np.isfinite(mean[1])
    assert rec["count"] == 1 and rec["rows"] == 3 and rec["mean"] == np.float64(mean[1])
    assert rec["variance"].tobytes() == np.float64(0.0).tobytes() and keep.tolist() == [0, 1, 0]


EDGE_NS = (255, 256, 257, 65_536, 65_537)


@functools.lru_cache(maxsize=None)
def edge_rows(n):
    """search_knn_self's expected rows (k = 4) of the first n points of one uniform cloud; shared and read-only."""
    p = np.ascontiguousarray(ds.uniform_cloud(65_537, 3, 33)[:n])
    p.flags.writeable = False
    rows = expected(oracle.Oracle(p, 10, "reference"), p, 4)
    rows.flags.writeable = False
    return p, rows


@needs_reference
@pytest.mark.parametrize("n", EDGE_NS)
def test_host_loop_at_the_edges_of_the_summation_tree(n):
    """One block short by an entry, full, one entry into the second; the same one level up (256 * 256)."""
    p, rows = edge_rows(n)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=pt.PTK_DEVICE_NONE)
    want = restate(rows, SQRT, 1.5)
    assert tree_sum(np.ones((n, 1)))[1] == (1 if n <= 256 else 2 if n <= 65_536 else 3)
    same(call(tree, 4, SQRT, 1.5, "loop"), want, n)


def overflow_cloud():
    """Four ordinary points and eight on a line at spacing 8.5e18 (module docstring)."""
    x = np.concatenate([np.arange(4, dtype=np.float32), np.float32(8.5e18) * np.arange(1, 9, dtype=np.float32)])
    p = np.zeros((12, 3), dtype=np.float32)
    p[:, 0] = x
    return p


def _line_rows(p, k):
    """Brute-force rows of points on the x axis (distinct distances per row except mirror pairs: ordered by index)."""
    n = len(p)
    with np.errstate(over="ignore"):
        dx = (p[:, None, 0] - p[None, :, 0]).astype(np.float32)
        d = (dx * dx).astype(np.float32)
    fmax = np.finfo(np.float32).max
    rows = np.zeros((n, k), dtype=pt.NEIGHBOR)
    rows["index"], rows["distance"] = -1, fmax
    for i in range(n):
        others = [j for j in np.argsort(d[i], kind="stable") if j != i and d[i, j] < fmax][:k]
        rows["index"][i, :len(others)] = others
        rows["distance"][i, :len(others)] = d[i, others]
    return rows


def _overflow_checks(tree, how):
    p = tree._pts
    rows = _line_rows(p, 3)
    want = restate(rows, 0, 2.0)
    got = call(tree, 3, 0, 2.0, how)
    # mean, kth, keep and the record depend on the distances alone: mirror pairs may come in either order
    same(got, want, ("overflow", how))
    mean, kth, keep, rec = got
    bad = ~np.isfinite(mean)
    assert 0 < bad.sum() < len(p), mean
    assert np.all(np.isinf(mean[bad])) and np.all(np.isfinite(kth[bad]))  # finite rows, infinite means
    assert np.all(np.isfinite(np.where(rows["distance"] < np.finfo(np.float32).max, rows["distance"], 0)))
    assert np.all(keep[bad] == 0) and rec["count"] == len(p) - bad.sum() and np.isfinite(rec["mean"])
    rooted = call(tree, 3, SQRT, 2.0, how)
    same(rooted, restate(rows, SQRT, 2.0), ("overflow, sqrt", how))
    assert np.all(np.isfinite(rooted[0])) and np.all(np.isfinite(rooted[1])) and rooted[3]["count"] == len(p)
    assert all(np.isfinite(rooted[3][f]) for f in ("sum", "mean", "ssd", "variance"))
    return got, rooted


def _issue_line():
    p = np.zeros((8, 3), dtype=np.float32)
    p[:, 0] = np.float32(1.2e19) * np.arange(8, dtype=np.float32)
    return p


def test_host_loop_where_a_row_sum_overflows():
    tree = pt.KdTree(overflow_cloud(), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    _overflow_checks(tree, "loop")
    line = pt.KdTree(_issue_line(), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    for flags in (0, SQRT):
        same(call(line, 3, flags, 2.0, "loop"), restate(_line_rows(line._pts, 3), flags, 2.0), ("line", flags))


def test_argument_checks_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    mean, keep = np.empty(9, dtype=np.float32), np.empty(9, dtype=np.uint8)
    rec = np.empty(1, dtype=pt.SPACING_STATS)
    P, M, K, R = p.ctypes.data, mean.ctypes.data, keep.ctypes.data, rec.ctypes.data
    loop = lib.ptk_host_spacing_knn_self
    assert loop(tree._h, P, 4, 0, F32(1.0), M, None, None, None) == 0
    assert loop(tree._h, P, 0, 0, F32(1.0), M, None, None, None) == INVALID
    assert loop(tree._h, P, 0xFFFFFFFF, 0, F32(1.0), M, None, None, None) == INVALID
    assert loop(tree._h, P, 4, 0, F32(1.0), None, None, K, R) == INVALID  # mean is required
    assert loop(tree._h, None, 4, 0, F32(1.0), M, None, None, None) == INVALID
    assert loop(None, P, 4, 0, F32(1.0), M, None, None, None) == INVALID
    assert loop(tree._h, P, 4, 2, F32(1.0), M, None, None, None) == INVALID  # an unknown flag bit
    for bad in (float("nan"), -1.0, float("inf"), -0.5):
        assert loop(tree._h, P, 4, 0, F32(bad), M, None, K, None) == INVALID, bad
        assert loop(tree._h, P, 4, 0, F32(bad), M, None, None, R) == INVALID, bad
        assert loop(tree._h, P, 4, 0, F32(bad), M, None, None, None) == 0, bad  # (no ratio is read)
    assert loop(tree._h, P, 4, 0, F32(0.0), M, None, K, R) == 0
    # a host-only handle has no device search: PTK_ERR_DEVICE, from every device entry point
    need = ctypes.c_uint64(0)
    assert lib.ptk_spacing_knn_self(tree._h, 4, 0, F32(1.0), M, None, None, None) == DEVICE
    assert lib.ptk_spacing_knn_self_device(tree._h, 4, 0, F32(1.0), M, None, None, None, None, 0, None) == DEVICE
    assert lib.ptk_spacing_knn_self(None, 4, 0, F32(1.0), M, None, None, None) == INVALID
    assert lib.ptk_spacing_knn_self_workspace(tree._h, ctypes.byref(need)) == 0 and need.value >= 16
    assert lib.ptk_spacing_knn_self_workspace(tree._h, None) == INVALID
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    m64 = np.empty(9, dtype=np.float64)
    assert lib.ptk_search64_spacing_knn_self(t64._h, 4, 0, F32(1.0), m64.ctypes.data, None, None, None) == DEVICE
    assert lib.ptk_search64_spacing_knn_self_device(t64._h, 4, 0, F32(1.0), m64.ctypes.data, None, None, None, None, 0,
                                                    None) == DEVICE
    # the wrapper
    with pytest.raises(pt.PtkError):
        tree.spacing_knn_self(4)
    for bad in (float("nan"), -1.0, float("inf"), 1e39):
        with pytest.raises(ValueError):
            tree.outliers_knn_self(4, std_ratio=bad)


def test_wrapper_under_the_host_loop():
    """allow_host_loop serves a float32 tree the device refuses -- here a host-only handle is not such a tree (it raises);
    the wrapper's own arithmetic is checked on the record a host loop call returns."""
    p, leaf = cloud("lidar")
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=pt.PTK_DEVICE_NONE)
    mean, kth, keep, rec = call(tree, 8, SQRT, 2.0, "loop")
    assert 0 < keep.sum() < len(p)
    assert rec["count"] == len(p) and rec["variance"] > 0.0 and np.all(mean <= kth)
    # the decision on squares is PCL's "mean_i <= mu + ratio * sigma" wherever that is not within rounding of the bound
    bound = rec["mean"] + 2.0 * np.sqrt(rec["variance"])
    clear = np.abs(mean.astype(np.float64) - bound) > 1e-9 * bound
    assert np.array_equal(keep[clear] == 1, (mean.astype(np.float64) <= bound)[clear])


# ---- CPU tier: the real kernel source in the emulator (tests/cpp/emulate_spacing.cpp) -----------------------------------

@pytest.fixture(scope="module")
def emu_spacing(tmp_path_factory):
    """tests/cpp/emulate_spacing.cpp, compiled with the emulator's g++ line and HIP stand-in (__graft_entry__.build)."""
    out = str(tmp_path_factory.mktemp("emu_spacing") / "libptk_emu_spacing.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_spacing.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    lib.emu_set_metric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.emu_spacing_knn_self.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_spacing_statistics.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def emulated(lib, p, leaf, metric, k, flags, ratio, route, piece=0, ranges=None, largest_leaf=None):
    """(mean, kth, keep, record, the original indices whose rows were computed) of the emulated kernels over the leaf
    positions of `ranges` (default: all).  The statistics kernels run where every row was computed; else keep and the
    record are None."""
    p = np.ascontiguousarray(p)
    host = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    if largest_leaf is not None:
        leaf_cases.assert_leaf(host, largest_leaf)
    nodes, idx, _, _ = host.flat()
    h = lib.emu_create(p.ctypes.data, len(p), p.shape[1], nodes.ctypes.data, len(nodes), idx.ctypes.data)
    assert h
    try:
        lib.emu_set_metric(h, {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}[metric])
        mean, kth = np.empty(len(p), dtype=np.float32), np.empty(len(p), dtype=np.float32)
        mean.view(np.uint8)[:] = 0xA5
        kth.view(np.uint8)[:] = 0xA5
        done = []
        for lo, hi in ranges or [(0, len(p))]:
            assert lib.emu_spacing_knn_self(h, lo, hi, k, flags, route, piece, mean.ctypes.data, kth.ctypes.data) == 0
            done.append(np.asarray(idx[lo:hi]))
    finally:
        lib.emu_destroy(h)
    keep = rec = None
    if ranges is None:
        keep, rec = np.full(len(p), 0xA5, dtype=np.uint8), np.empty(1, dtype=pt.SPACING_STATS)
        rec.view(np.uint8)[:] = 0xA5
        assert lib.emu_spacing_statistics(mean.ctypes.data, len(p), ratio, keep.ctypes.data, rec.ctypes.data) == 0
        rec = rec[0]
    return mean, kth, keep, rec, np.concatenate(done)


@needs_reference
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_kernels_equal_the_contract(emu_spacing, kind, metric):
    ks = (1, 3, 4, 15, 63)
    if kind == "lattice":
        p, leaf = lattice(), 4
        ref = oracle.Oracle(p, leaf, "reference", metric=metric)
        rows = {k: expected(ref, p, k) for k in ks + (64, 80)}
    else:
        p, leaf = cloud(kind)
        rows = {k: want_rows(kind, metric, k) for k in ks + (64, 80)}
    for k in ks:
        flags = SQRT if k in (3, 15) else 0
        want = restate(rows[k], flags, 1.0)
        # (647 leaf positions per launch: pieces that end inside a wavefront, and a ragged last one)
        for route, piece in ((1, 0), (1, 647), (2, 0), (2, 647)):
            same(emulated(emu_spacing, p, leaf, metric, k, flags, 1.0, route, piece)[:4], want, (kind, metric, k, route, piece))
    for k in (64, 80):  # k + 1 beyond the register list: the staged route only
        same(emulated(emu_spacing, p, leaf, metric, k, SQRT, 1.0, 2, 1000)[:4], restate(rows[k], SQRT, 1.0), (kind, metric, k))


@needs_reference
@pytest.mark.parametrize("n", (255, 256, 257, 65_537))
def test_emulated_statistics_at_the_edges_of_the_summation_tree(emu_spacing, n):
    """The statistics kernels with the butterfly over the means the contract gives (no search)."""
    _, rows = edge_rows(n)
    want = restate(rows, SQRT, 1.5)
    keep, rec = np.full(n, 0xA5, dtype=np.uint8), np.empty(1, dtype=pt.SPACING_STATS)
    assert emu_spacing.emu_spacing_statistics(want[0].ctypes.data, n, 1.5, keep.ctypes.data, rec.ctypes.data) == 0
    assert keep.tobytes() == want[2].tobytes() and rec[0].tobytes() == want[3].tobytes()


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", depth_cases.EUCLID_CASES)
def test_emulated_kernels_where_the_stack_class_changes(emu_spacing, dim, leaf, metric, depth):
    """The rows searched are the far pile of coincident points and the 200 leaf positions on either side of it
    (tests/test_knn_self.py)."""
    pts, pile = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    host = pt.KdTree(pts, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    _, idx, _, _ = host.flat()
    at = np.flatnonzero(np.asarray(idx) >= 3_000)  # leaf positions of the pile
    lo, hi = max(0, int(at.min()) - 200), min(len(pts), int(at.max()) + 201)
    run = depth_cases.Watch(depth, emu_spacing)
    for k in (5, 31, 80):
        want = restate(expected(ref, pts, k), SQRT, 1.0)
        for route in ((1, 2) if dim <= 3 and k < 64 else (2,)):
            mean, kth, _, _, done = run(emulated, emu_spacing, pts, leaf, metric, k, SQRT, 1.0, route, 0, [(lo, hi)])
            assert len(done) == hi - lo
            assert mean[done].tobytes() == want[0][done].tobytes() and kth[done].tobytes() == want[1][done].tobytes(), (k, route)


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_kernels_where_the_leaf_scan_changes(emu_spacing, L):
    pts, blob, q, nb, ref, _ = leaf_cases.case(L)
    pts = np.asarray(pts)
    for k in (7, 40):
        want = restate(expected(ref, pts, k), SQRT, 2.0)
        for route, piece in ((1, 0), (2, 647)):
            same(emulated(emu_spacing, pts, L, "L2Squared", k, SQRT, 2.0, route, piece, largest_leaf=L)[:4], want, (L, k, route))


# ---- the C++ members (tests/cpp/spacing_self_main.cpp) -----------------------------------------------------------------

def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "spacing_self_main.cpp"), "-o", out]
    if host_only:  # (a stand-alone host program: the place for the sanitizers)
        cmd[1:1] = ["-DPICO_TREE_HOST_ONLY", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def check_cpp(exe, d, ks):
    p = _cpp_points(d)
    for k in ks:
        res = subprocess.run([exe, d, str(k), "1.5"], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        for name, metric, dtype, flags in (("l2", "L2Squared", np.float32, SQRT), ("l1", "L1", np.float32, 0),
                                           ("l2d", "L2Squared", np.float64, SQRT)):
            ref = oracle.Oracle(p.astype(dtype), 10, "reference", metric=metric, dtype=dtype)
            want = restate(expected(ref, p.astype(dtype), k), flags, 1.5)
            for ext, w in zip(("mean", "kth", "keep", "stats"), want):
                assert open(os.path.join(d, f"{name}.{ext}"), "rb").read() == np.asarray(w).tobytes(), (name, k, ext)


@needs_reference
@needs_reference64
def test_cpp_per_point_member_under_the_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "spacing_self_host")
    _cpp_program(exe, host_only=True)
    check_cpp(exe, str(tmp_path), (1, 9, 70))


# ---- gpu tier --------------------------------------------------------------------------------------------------------

def both_routes(tree, k, flags, ratio, want, what):
    assert tree.self_route(k) == 1
    same(call(tree, k, flags, ratio, "device"), want, what + ("direct",))
    pt.set_test_knobs(self_route=2)
    try:
        assert tree.self_route(k) == 2
        same(call(tree, k, flags, ratio, "device"), want, what + ("staged",))
    finally:
        pt.set_test_knobs(self_route=None)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "2d"])
@pytest.mark.parametrize("metric", METRICS)
def test_both_routes_equal_the_contract(gpu, kind, metric):
    p, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
    for k in KS_DIRECT:
        rows = want_rows(kind, metric, k)
        for flags in (0, SQRT):
            both_routes(tree, k, flags, 1.0, restate(rows, flags, 1.0), (kind, metric, k, flags))


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
        for flags in (0, SQRT):
            same(call(tree, k, flags, 1.0, "device"), restate(want_rows(kind, metric, k), flags, 1.0), (kind, metric, k, flags))


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_topological_trees_take_the_staged_route(gpu, metric):
    p = _topological_points(metric)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=gpu)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    for k in (1, 4, 16, 80):
        assert tree.self_route(k) == 2
        rows = expected(ref, p, k)
        for flags in (0, SQRT):
            same(call(tree, k, flags, 2.0, "device"), restate(rows, flags, 2.0), (metric, k, flags))


@pytest.mark.gpu
@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "ties", "5d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_float64_trees(gpu, kind, metric):
    """The correctly rounded double square root and division of the device against numpy's, bit for bit."""
    p, leaf = cloud(kind)
    tree = pt.KdTree(p.astype(np.float64), getattr(pt.Metric, metric), leaf, device=gpu)
    for k in (1, 4, 16, 40):
        rows = want_rows(kind, metric, k, np.float64)
        assert tree.self_route(k) == 2
        for flags in (0, SQRT):
            got = call(tree, k, flags, 1.0, "device")
            assert got[0].dtype == np.float64
            same(got, restate(rows, flags, 1.0), (kind, metric, k, flags))


@pytest.mark.gpu
@needs_reference
def test_pieces_of_leaf_positions(gpu, monkeypatch):
    """self_piece = 640 on 3 000 points: five pieces of the staged route, the last one of 440; PTK_MAX_BATCH = 1 000:
    three ranges of the direct kernel, all ending inside a wavefront."""
    p, leaf = cloud("ties")
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=gpu)
    for k in (3, 16):
        want = restate(want_rows("ties", "L2Squared", k), SQRT, 1.0)
        pt.set_test_knobs(self_route=2, self_piece=640)
        same(call(tree, k, SQRT, 1.0, "device"), want, (k, "pieces of 640"))
        pt.set_test_knobs()
        monkeypatch.setenv("PTK_MAX_BATCH", "1000")
        both_routes(tree, k, SQRT, 1.0, want, (k, "PTK_MAX_BATCH"))
        monkeypatch.delenv("PTK_MAX_BATCH")
    p5, leaf5 = cloud("5d")
    t5 = pt.KdTree(p5, pt.Metric.L2Squared, leaf5, device=gpu)
    pt.set_test_knobs(self_piece=640)
    same(call(t5, 4, SQRT, 1.0, "device"), restate(want_rows("5d", "L2Squared", 4), SQRT, 1.0), "5d")


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136, 1031, 1032])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 10, "L2Squared"), (2, 4, "L1"), (3, 10, "LPInf")])
def test_depths_where_the_dispatch_changes(gpu, dim, leaf, metric, depth):
    pts, _ = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    tree = pt.KdTree(pts, getattr(pt.Metric, metric), leaf, device=gpu)
    depth_cases.assert_depth(tree, depth)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    for k in (5, 31):
        want = restate(expected(ref, pts, k), SQRT, 2.0)
        if depth >= 1032:
            assert tree.self_route(k) == 2
            same(call(tree, k, SQRT, 2.0, "device"), want, (depth, k))
        else:
            both_routes(tree, k, SQRT, 2.0, want, (depth, k))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 9])
def test_tiny_trees_on_the_device(gpu, n):
    p = ds.uniform_cloud(n, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=gpu)
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=gpu)
    for k in (1, 12, 80):
        want = restate(_tiny_rows(p, k), SQRT, 2.0)
        if k < 64:
            both_routes(tree, k, SQRT, 2.0, want, (n, k))
        got = call(tree, k, SQRT, 2.0, "device")
        same(got, want, (n, k))
        _tiny_checks(got, n)
        got64 = call(t64, k, SQRT, 2.0, "device")
        same(got64, restate(_tiny_rows(p.astype(np.float64), k), SQRT, 2.0), (n, k, "float64"))
        assert np.all(got64[0][want[0] == np.finfo(np.float32).max] == np.finfo(np.float64).max)
    for route in (None, 2):
        pt.set_test_knobs(self_route=route)
        _count_one_checks(call(pt.KdTree(count_one_cloud(), pt.Metric.L2Squared, 3, device=gpu), 2, 0, 2.0, "device"))
    pt.set_test_knobs()


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("n", EDGE_NS)
def test_edges_of_the_summation_tree(gpu, n):
    p, rows = edge_rows(n)
    want = restate(rows, SQRT, 1.5)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    got = call(tree, 4, SQRT, 1.5, "device")
    same(got, want, n)
    same(call(tree, 4, SQRT, 1.5, "loop"), got, (n, "host loop"))


def planted():
    """The lidar cloud and five points one bounding-box extent beyond its maximum corner, along x, y, z, xy and xyz."""
    p, leaf = cloud("lidar")
    lo, hi = p.min(0), p.max(0)
    ext = hi - lo
    far = np.array([hi + ext * np.array(d, dtype=np.float32) for d in
                    ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1))], dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([p, far])), leaf


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "2d"])
@pytest.mark.parametrize("metric", METRICS)
def test_keep_at_three_ratios(gpu, kind, metric):
    """Every case asserts 0 < kept < n, but for the combinations where numpy says the mask cannot vary: ties at k = 1
    (most means are exactly 0), and ties under LNInf at k = 1 and 8 -- on the 1/8 grid every point has eight others that
    share a coordinate with it, all 3 000 means are exactly 0, the variance is +0 and everything is kept at any ratio
    (restate() gives 3 000 of 3 000 for the six cases).  They stay in the equality check."""
    p, leaf = cloud(kind)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
    flags = SQRT if metric == "L2Squared" else 0
    for k in (1, 8, 16):
        rows = want_rows(kind, metric, k) if k in KS_HOST else expected(oracle.Oracle(p, leaf, "reference", metric=metric), p, k)
        for ratio in (0.0, 1.0, 2.0):
            want = restate(rows, flags, ratio)
            got = call(tree, k, flags, ratio, "device")
            same(got, want, (kind, metric, k, ratio))
            if not (kind == "ties" and (k == 1 or (metric == "LNInf" and k == 8))):
                assert 0 < int(got[2].sum()) < len(p), (kind, metric, k, ratio)


@pytest.mark.gpu
@needs_reference
def test_planted_outliers_are_removed(gpu):
    p, leaf = planted()
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=gpu)
    rows = expected(oracle.Oracle(p, leaf, "reference"), p, 8)
    want = restate(rows, SQRT, 2.0)
    assert int(want[2].sum()) == 3_988 and not want[2][-5:].any()
    both_routes(tree, 8, SQRT, 2.0, want, ("planted",))
    mask, info = tree.outliers_knn_self(8, stats=True)
    assert mask.dtype == bool and mask.tobytes() == want[2].tobytes() and info["record"] == want[3].tobytes()
    assert info["stddev"] == float(np.sqrt(want[3]["variance"])) and info["count"] == len(p)
    kept = tree.outliers_knn_self(8, indices=True)
    assert kept.dtype == np.int64 and np.array_equal(kept, np.flatnonzero(want[2]))


@pytest.mark.gpu
def test_a_row_sum_that_overflows(gpu):
    tree = pt.KdTree(overflow_cloud(), pt.Metric.L2Squared, 3, device=gpu)
    host = pt.KdTree(overflow_cloud(), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    for route in (None, 2):
        pt.set_test_knobs(self_route=route)
        got, rooted = _overflow_checks(tree, "device")
        same(got, call(host, 3, 0, 2.0, "loop"), ("host loop", route))
        same(rooted, call(host, 3, SQRT, 2.0, "loop"), ("host loop, sqrt", route))
    pt.set_test_knobs()
    line = pt.KdTree(_issue_line(), pt.Metric.L2Squared, 3, device=gpu)
    for flags in (0, SQRT):
        same(call(line, 3, flags, 2.0, "device"), restate(_line_rows(line._pts, 3), flags, 2.0), ("line", flags))


@pytest.mark.gpu
@needs_reference
def test_torch_device_form_null_outputs_and_workspace(gpu):
    import torch

    p, leaf = cloud("lidar")
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=gpu)
    n, k = len(p), 8
    want = restate(want_rows("lidar", "L2Squared", k), SQRT, 2.0)
    side = torch.cuda.Stream(device=gpu)
    for route in (1, 2):
        pt.set_test_knobs(self_route=route)
        with torch.cuda.stream(side):
            mean, kth = tree.spacing_knn_self(k, kth=True, device=True)
            only = tree.spacing_knn_self(k, device=True)
            mask, info = tree.outliers_knn_self(k, stats=True, device=True)
            idx = tree.outliers_knn_self(k, indices=True, device=True)
        side.synchronize()
        assert mean.is_cuda and mean.cpu().numpy().tobytes() == want[0].tobytes() == only.cpu().numpy().tobytes()
        assert kth.cpu().numpy().tobytes() == want[1].tobytes()
        assert mask.dtype == torch.bool and mask.cpu().numpy().tobytes() == want[2].astype(bool).tobytes()
        assert info["record"] == want[3].tobytes() and np.array_equal(idx.cpu().numpy(), np.flatnonzero(want[2]))
        # every combination of null optional outputs, through the host-buffer form
        for has_kth in (False, True):
            for has_keep in (False, True):
                for has_stats in (False, True):
                    got = call(tree, k, SQRT, 2.0, "device", kth=has_kth, keep=has_keep, stats=has_stats)
                    for g, w, has in zip(got, want, (True, has_kth, has_keep, has_stats)):
                        assert (g is None) == (not has) and (g is None or np.asarray(g).tobytes() == w.tobytes())
    pt.set_test_knobs()
    # host numpy forms of the wrapper; sqrt=None is on for L2Squared, off for L1
    assert tree.spacing_knn_self(k).tobytes() == want[0].tobytes()
    assert tree.spacing_knn_self(k, sqrt=False).tobytes() == restate(want_rows("lidar", "L2Squared", k), 0, 2.0)[0].tobytes()
    t1 = pt.KdTree(p, pt.Metric.L1, leaf, device=gpu)
    assert t1.spacing_knn_self(k).tobytes() == restate(want_rows("lidar", "L1", k), 0, 2.0)[0].tobytes()
    # the workspace
    lib = pt._load()
    need = ctypes.c_uint64(0)
    assert lib.ptk_spacing_knn_self_workspace(tree._h, ctypes.byref(need)) == 0
    assert 16 * ((n + 255) // 256 + 1) <= need.value <= 16 * ((n + 255) // 256 + 1) + 256
    dev = f"cuda:{gpu}"
    d_mean = torch.empty(n, dtype=torch.float32, device=dev)
    d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    args = (tree._h, k, SQRT, F32(2.0), d_mean.data_ptr(), None, d_keep.data_ptr(), None)
    assert lib.ptk_spacing_knn_self_device(*args, ws.data_ptr(), need.value - 1, None) == INVALID
    assert b"workspace" in lib.ptk_last_error()
    assert lib.ptk_spacing_knn_self_device(*args, None, need.value, None) == INVALID
    torch.cuda.synchronize()
    assert bool((d_keep == 7).all())  # (refused before anything was enqueued)
    assert lib.ptk_spacing_knn_self_device(*args, ws.data_ptr(), need.value, None) == 0
    torch.cuda.synchronize()
    assert d_keep.cpu().numpy().tobytes() == want[2].tobytes()
    # no reduction: no workspace
    assert lib.ptk_spacing_knn_self_device(tree._h, k, SQRT, F32(float("nan")), d_mean.data_ptr(), None, None, None, None, 0,
                                           None) == 0
    torch.cuda.synchronize()
    assert d_mean.cpu().numpy().tobytes() == want[0].tobytes()
    assert lib.ptk_spacing_knn_self_device(tree._h, k, SQRT, F32(float("nan")), d_mean.data_ptr(), None, d_keep.data_ptr(),
                                           None, ws.data_ptr(), need.value, None) == INVALID
    assert lib.ptk_spacing_knn_self_device(tree._h, 0, SQRT, F32(1.0), d_mean.data_ptr(), None, None, None, None, 0,
                                           None) == INVALID
    assert lib.ptk_spacing_knn_self_device(tree._h, k, SQRT, F32(1.0), None, None, None, None, None, 0, None) == INVALID


@pytest.mark.gpu
def test_direct_route_can_be_captured_into_a_graph(gpu):
    """Route 1 with the statistics only enqueues: captured once, replayed, the same bytes as the plain call."""
    import torch

    p, leaf = cloud("uniform")
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=gpu)
    plain = call(tree, 8, SQRT, 2.0, "device")
    lib = pt._load()
    n = len(p)
    need = ctypes.c_uint64(0)
    assert lib.ptk_spacing_knn_self_workspace(tree._h, ctypes.byref(need)) == 0
    dev = f"cuda:{gpu}"
    mean = torch.zeros(n, dtype=torch.float32, device=dev)
    kth = torch.zeros(n, dtype=torch.float32, device=dev)
    keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    rec = torch.zeros(64, dtype=torch.uint8, device=dev)
    ws = torch.zeros(need.value, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        tree.spacing_knn_self(8, device=True)  # (the code objects are loaded before the capture)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            rc = lib.ptk_spacing_knn_self_device(tree._h, 8, SQRT, F32(2.0), mean.data_ptr(), kth.data_ptr(), keep.data_ptr(),
                                                 rec.data_ptr(), ws.data_ptr(), need.value, side.cuda_stream)
        assert rc == 0, lib.ptk_last_error()
        graph.replay()
    side.synchronize()
    got = (mean.cpu().numpy(), kth.cpu().numpy(), keep.cpu().numpy(), rec.cpu().numpy())
    same(got, plain, "graph replay")


@pytest.mark.gpu
def test_other_searches_of_the_handle_are_left_alone(gpu):
    p, q = ds.uniform_cloud(20_000, 3, 71), ds.uniform_cloud(6_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)

    def others():
        return [tree.search_knn(q, 1).tobytes(), tree.search_knn(q, 16).tobytes(), tree.search_knn_self(7).tobytes(),
                tree.search_knn_within(q, 8, 0.002).tobytes(), tree.count_within(q, 0.002).tobytes(),
                tree.search_radius(q, 0.002).flat.tobytes(), tree.count_within_self(0.002).tobytes()]

    before = others()
    got = {}
    for route in (None, 2):
        pt.set_test_knobs(self_route=route)
        got[route] = [np.asarray(x).tobytes() for k in (1, 7, 16) for x in call(tree, k, SQRT, 2.0, "device")]
        assert others() == before, route
    assert got[None] == got[2]


@pytest.mark.gpu
def test_refusal_of_the_underlying_search_is_passed_on(gpu):
    """A topological tree of the deep stack class: the device k-NN search refuses it, so does this call -- unchanged --,
    and under allow_host_loop the host loop serves the wrapper."""
    import warnings

    pts, _ = depth_cases.cloud_at_depth(1032, 3, 4, space="SE2Squared")
    pts = np.asarray(pts)
    tree = pt.KdTree(pts, pt.Metric.SE2Squared, 4, device=gpu)
    with pytest.raises(pt.PtkError) as refused:
        tree.spacing_knn_self(3)
    with pytest.raises(pt.PtkError) as refused_knn:
        tree.search_knn(pts[:10], 4)
    assert refused.value.status == refused_knn.value.status == pt.PTK_ERR_UNSUPPORTED
    assert str(refused.value) == str(refused_knn.value)
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            mask, info = tree.outliers_knn_self(3, stats=True)
    finally:
        pt.allow_host_loop(False)
    want = call(tree, 3, SQRT, 2.0, "loop")
    assert mask.tobytes() == want[2].astype(bool).tobytes() and info["record"] == want[3].tobytes()


@pytest.mark.gpu
@needs_reference
@needs_reference64
def test_cpp_batched_member(gpu, tmp_path):
    exe = os.path.join(str(tmp_path), "spacing_self_batch")
    _cpp_program(exe, host_only=False)
    check_cpp(exe, str(tmp_path), (1, 9, 70))
