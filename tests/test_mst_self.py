"""mst_within_self (ptk.h): the minimum spanning forest of the fixed-radius graph over a tree's
own points.

The expected value is the contract written out below in numpy and plain Python -- the edge list from rows obtained
independently of the feature (the compiled reference's search_radius rows of the tree's own points without the own entry;
``ptk_host_search_radius`` where the reference cannot build the tree), sorted by ``(bits(w), lo, hi)``, Kruskal with a
union-find -- and the comparison is exact: the bytes of the sorted edge array and the labels.  Before a cloud is used its
rows are asserted symmetric, so that a failure points at the feature and not at the input.

CPU tier: the library's host loop on host-only handles, the real kernel source in the CPU emulator
(tests/cpp/emulate_mst.cpp) driven as the backend drives the rounds under the live and the snapshot schedule, the C++
member of a host-only build, the wrapper.  GPU tier: the device rounds.
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
from tests import depth_cases, leaf_cases
from tests import test_radius_self as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
FLT_MAX = np.float32(np.finfo(np.float32).max)
METRICS = ["L2Squared", "L1"]  # the metrics the feature serves
needs_reference = rs.needs_reference
EDGE = pt.MST_EDGE
INVALID, UNSUPPORTED, DEVICE = -1, -2, -3


# ---- the contract, written out ---------------------------------------------------------------------------------------

def symmetric(off, flat):
    n = len(off) - 1
    row, idx = rs.row_ids(off), np.asarray(flat["index"]).astype(np.int64)
    return np.array_equal(np.sort(row * n + idx), np.sort(idx * n + row))


def graph_edges(off, flat, radius, core=None):
    """The edges of the contract, each once, ascending in (bits(w), lo, hi): arrays (wbits, lo, hi)."""
    row, idx = rs.row_ids(off), np.asarray(flat["index"]).astype(np.int64)
    w = np.ascontiguousarray(flat["distance"]).astype(np.float32)
    if core is not None:
        w = np.maximum(np.maximum(w, core[row]), core[idx]).astype(np.float32)
        ok = w < np.float32(radius)
        row, idx, w = row[ok], idx[ok], w[ok]
    lo, hi = np.minimum(row, idx), np.maximum(row, idx)
    bits = np.ascontiguousarray(w).view(np.uint32).astype(np.int64)
    order = np.lexsort((hi, lo, bits))
    bits, lo, hi = bits[order], lo[order], hi[order]
    first = np.ones(len(bits), dtype=bool)
    first[1:] = (bits[1:] != bits[:-1]) | (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    return bits[first], lo[first], hi[first]


def components(n, lo, hi):
    """labels[i] = the smallest index of i's component under the given edges."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(lo.tolist(), hi.tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def expected_mst(off, flat, radius, core=None):
    """(edges as MST_EDGE ascending, labels int32) of the contract: Kruskal over the sorted edge list."""
    n = len(off) - 1
    bits, lo, hi = graph_edges(off, flat, radius, core)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    taken = []
    for k, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
            taken.append(k)
    edges = np.zeros(len(taken), dtype=EDGE)
    edges["lo"], edges["hi"] = lo[taken], hi[taken]
    edges["w"] = bits[taken].astype(np.uint32).view(np.float32)
    return edges, np.array([find(i) for i in range(n)], dtype=np.int32)


def test_the_contract_on_a_case_done_by_hand():
    """Four points on a line at 0, 1, 2, 4 (squared distances) with r = 4.5: edges 0-1 (1), 1-2 (1), 0-2 (4), 2-3 (4);
    the forest is 0-1, 1-2, 2-3 in that order -- (1, 0, 1) < (1, 1, 2) < (4, 0, 2) < (4, 2, 3)."""
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [4, 0, 0]], dtype=np.float32)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 2, device=pt.PTK_DEVICE_NONE)
    rows = host_search_rows(tree, p, np.float32(4.5))
    assert symmetric(*rows)
    edges, labels = expected_mst(*rows, 4.5)
    assert edges.tolist() == [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 4.0)] and labels.tolist() == [0, 0, 0, 0]
    edges, labels = expected_mst(*host_search_rows(tree, p, np.float32(4.0)), 4.0)  # (strict: 2-3 is out)
    assert edges.tolist() == [(0, 1, 1.0), (1, 2, 1.0)] and labels.tolist() == [0, 0, 0, 3]
    core = np.array([0, 0, 3, 0], dtype=np.float32)  # (mutual reachability lifts 1-2 to 3; 0-2 and 2-3 stay 4)
    edges, labels = expected_mst(*rows, 4.5, core)
    assert edges.tolist() == [(0, 1, 1.0), (1, 2, 3.0), (2, 3, 4.0)]
    core[2] = 4.5  # (not below the radius: point 2 is isolated, and so is 3 behind it)
    edges, labels = expected_mst(*rows, 4.5, core)
    assert edges.tolist() == [(0, 1, 1.0)] and labels.tolist() == [0, 0, 2, 3]


# ---- rows, clouds ------------------------------------------------------------------------------------------------------

def host_search_rows(tree, p, r):
    """(offsets, flat) of the library's host loop ptk_host_search_radius over the points themselves, own entries removed."""
    lib = pt._load()
    p = np.ascontiguousarray(p, dtype=np.float32)
    off = np.zeros(len(p) + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    rc = lib.ptk_host_search_radius(tree._h, p.ctypes.data, p.ctypes.data, len(p), np.float32(r), np.float32(1), 0,
                                    off.ctypes.data, ctypes.byref(rows))
    assert rc == 0, lib.ptk_last_error()
    return rs.without_self(off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR))


def lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(nx * 100 + ny * 10 + nz)
    return np.ascontiguousarray(g[rng.permutation(len(g))].astype(np.float32))


def piles():
    """5 coincident points at each of 40 sites, shuffled."""
    sites = ds.uniform_cloud(40, 3, 77)
    p = np.repeat(sites, 5, axis=0)
    return np.ascontiguousarray(p[np.random.default_rng(5).permutation(len(p))])


def blobs(k):
    """k blobs of 300 points, many diameters apart."""
    rng = np.random.default_rng(40 + k)
    centres = np.array([[0, 0, 0], [50, 3, -2], [-20, 70, 9]], dtype=np.float32)[:k]
    p = np.concatenate([c + rng.random((300, 3), dtype=np.float32) for c in centres])
    return np.ascontiguousarray(p[rng.permutation(len(p))].astype(np.float32))


@functools.lru_cache(maxsize=None)
def constructed(name):
    """(points, leaf, radii) of a constructed cloud."""
    if name == "lattice444":
        return lattice(4, 4, 4), 4, ("step", "above", INF)
    if name == "lattice882":
        return lattice(8, 8, 2), 6, ("step", "above", INF)
    if name == "piles":
        return piles(), 4, (np.float32(1e-6), np.float32(0.05), INF)
    if name == "blobs2":
        return blobs(2), 8, (INF, np.float32(0.02))
    if name == "blobs3":
        return blobs(3), 8, (INF, FLT_MAX)
    raise ValueError(name)


CONSTRUCTED = ["lattice444", "lattice882", "piles", "blobs2", "blobs3"]


def radius_value(r, metric):
    """'step': the grid step of a lattice in the metric's unit (neighbours AT r stay out); 'above': the next float."""
    if isinstance(r, str):
        step = np.float32(1.0)
        return step if r == "step" else np.nextafter(step, np.float32(np.inf))
    return np.float32(r)


@functools.lru_cache(maxsize=None)
def _constructed_want(name, metric, r):
    p, leaf, _ = constructed(name)
    if oracle.have_reference():
        ref = oracle.Oracle(p, leaf, "reference", metric=metric)
        rows = rs.without_self(*ref.search_radius(p, np.float32(r)))
    else:
        rows = host_search_rows(pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE), p, r)
    assert symmetric(*rows), (name, metric, r)
    return expected_mst(*rows, r)


def constructed_want(name, metric, r):
    return _constructed_want(name, metric, float(r))


@functools.lru_cache(maxsize=None)
def _case_want(kind, metric, r, with_core):
    c = rs.case(kind, metric)
    rows = c.want(np.float32(r))
    assert symmetric(*rows), (kind, metric, r)
    return expected_mst(*rows, r, c.kth() if with_core else None)


def case_want(c, r, with_core=False):
    """Expected (edges, labels) of an rs.Case at r: computed once, shared by the tiers.  with_core: the 8th-neighbour
    distances of the reference as core distances."""
    return _case_want(c.kind, c.metric, float(r), bool(with_core))


def _ptr(a):
    return None if a is None else a.ctypes.data


def guarded_call(n, call):
    """`call(edges_ptr, labels_ptr, n_edges_ref)` into poisoned, guarded buffers: (edges[:n_edges], labels)."""
    ebuf, edges = rs.guarded(max(n - 1, 0), EDGE)
    lbuf, labels = rs.guarded(n, np.int32)
    count = ctypes.c_uint64(12345)
    rc = call(edges.ctypes.data if n > 1 else None, labels.ctypes.data, ctypes.byref(count))
    assert rc == 0, pt._load().ptk_last_error()
    assert rs.guards_intact(ebuf) and rs.guards_intact(lbuf), "written outside a buffer"
    assert count.value <= max(n - 1, 0)
    assert not np.any(labels == np.int32(-0x5A5A5A5B)), "a label was not written"
    return edges[:count.value].copy(), labels.copy()


def host_mst(tree, r, core=None, points=None):
    lib = pt._load()
    p = tree._pts if points is None else points
    return guarded_call(len(p), lambda e, l, c: lib.ptk_host_mst_within_self(tree._h, p.ctypes.data, np.float32(r),
                                                                           _ptr(core), e, c, l))


def same(got, want, what=None):
    (ge, gl), (we, wl) = got, want
    assert len(ge) == len(we), (what, len(ge), len(we))
    assert ge.tobytes() == we.tobytes(), (what, "edges")
    assert np.array_equal(gl, wl), (what, "labels")
    assert len(ge) == len(gl) - len(np.unique(gl)), (what, "n_edges = n - components")


# ---- CPU tier: the host loop -------------------------------------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_equals_the_contract(kind, metric):
    """The radii of rs.Case.values() (several components), FLT_MAX and +inf on the 600-point cloud; labels equal the
    host loop's cluster_within_self(r, 0), n_edges = n - n_clusters."""
    c = rs.case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    for r in c.values():
        got = host_mst(tree, r)
        same(got, case_want(c, r), (kind, metric, r))
        labels = np.zeros(c.n, dtype=np.int32)
        n_clusters = ctypes.c_uint64(0)
        assert lib.ptk_host_cluster_within_self(tree._h, c.p.ctypes.data, np.float32(r), None, 0, labels.ctypes.data,
                                                ctypes.byref(n_clusters)) == 0
        assert np.array_equal(got[1], labels) and len(got[0]) == c.n - n_clusters.value
    if kind == "small":
        assert len(case_want(c, INF)[0]) == c.n - 1
    r = c.values()[2]
    same(host_mst(tree, r, c.kth()), case_want(c, r, True), (kind, metric, "core"))


@pytest.mark.parametrize("name", CONSTRUCTED)
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_on_the_constructed_clouds(name, metric):
    p, leaf, radii = constructed(name)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    for r in radii:
        r = radius_value(r, metric)
        want = constructed_want(name, metric, r)
        same(host_mst(tree, r), want, (name, metric, r))
    if name.startswith("lattice"):
        assert len(constructed_want(name, metric, radius_value("step", metric))[0]) == 0  # (neighbours AT r stay out)
        above = constructed_want(name, metric, radius_value("above", metric))[0]
        assert len(above) == len(p) - 1 and np.all(above["w"] == 1.0)  # every weight ties: decided by (lo, hi) alone
    if name == "piles":
        zero = constructed_want(name, metric, 1e-6)[0]
        assert len(zero) == 40 * 4 and np.all(zero["w"] == 0)
    if name.startswith("blobs"):
        assert len(constructed_want(name, metric, INF)[0]) == len(p) - 1


def tiny_cases():
    """n = 1, 2, 3; n = leaf size (the root a leaf: no component table); n = leaf size + 1."""
    out = []
    for n, leaf in ((1, 4), (2, 4), (3, 4), (3, 1), (8, 8), (9, 8)):
        out.append((ds.uniform_cloud(n, 3, 100 + n), leaf))
    return out


def tiny_want(p, leaf, metric, r):
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
    rows = host_search_rows(tree, p, r)
    assert symmetric(*rows)
    return tree, expected_mst(*rows, r)


@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_of_tiny_trees_and_the_radii_at_the_edges(metric):
    for p, leaf in tiny_cases():
        for r in (np.float32(0), np.float32(0.3), FLT_MAX, np.float32(INF)):
            tree, want = tiny_want(p, leaf, metric, r)
            got = host_mst(tree, r)
            same(got, want, (len(p), leaf, r))
            if r == 0:
                assert len(got[0]) == 0 and np.array_equal(got[1], np.arange(len(p)))
            if r >= FLT_MAX:
                assert len(got[0]) == len(p) - 1


def core_cases(n, kth, r):
    """(name, core): the k-th neighbour distances; all equal (every weight ties); one entry at the radius (isolated)."""
    flat = np.full(n, np.float32(r) * np.float32(0.5), dtype=np.float32)
    one = np.array(kth, dtype=np.float32)
    one[n // 3] = np.float32(r)
    return [("kth", np.ascontiguousarray(kth, dtype=np.float32)), ("equal", flat), ("isolated", one)]


@functools.lru_cache(maxsize=None)
def core_cloud():
    """2 000 points, the radius (4 x the median 4th-neighbour distance) and the 4th-neighbour distances by the host loop
    of spacing_knn_self (unit of the metric: no square root)."""
    p = ds.uniform_cloud(2_000, 3, 55)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 8, device=pt.PTK_DEVICE_NONE)
    mean, kth = np.zeros(len(p), dtype=np.float32), np.zeros(len(p), dtype=np.float32)
    assert pt._load().ptk_host_spacing_knn_self(tree._h, p.ctypes.data, 4, 0, np.float32(0), mean.ctypes.data,
                                                 kth.ctypes.data, None, None) == 0
    r = np.float32(4) * np.float32(np.median(kth))
    rows = host_search_rows(tree, p, r)
    assert symmetric(*rows)
    return p, r, kth, rows


@functools.lru_cache(maxsize=None)
def core_want(name):
    p, r, kth, rows = core_cloud()
    core = dict(core_cases(len(p), kth, r))[name]
    return expected_mst(*rows, r, core)


@pytest.mark.parametrize("name", ["kth", "equal", "isolated"])
def test_host_loop_with_core_distances(name):
    p, r, kth, rows = core_cloud()
    core = dict(core_cases(len(p), kth, r))[name]
    tree = pt.KdTree(p, pt.Metric.L2Squared, 8, device=pt.PTK_DEVICE_NONE)
    got = host_mst(tree, r, core)
    same(got, core_want(name), name)
    if name == "equal":
        assert len(np.unique(got[0]["w"][got[0]["w"] == core[0]])) == 1 and np.all(got[0]["w"] >= core[0])
    if name == "isolated":
        assert got[1][len(p) // 3] == len(p) // 3 and not np.any(got[0]["lo"] == len(p) // 3) \
            and not np.any(got[0]["hi"] == len(p) // 3)
    if name == "kth":
        plain = expected_mst(*rows, r)[0]
        assert plain.tobytes() != got[0].tobytes()  # (the core distances change the tree)


@needs_reference
def test_cutting_the_forest_gives_the_clusters_of_every_smaller_radius():
    c = rs.case("lidar", "L2Squared")
    r = c.values()[2]
    edges, _ = case_want(c, r)
    for cut in (c.values()[1], np.float32(0.5) * r, np.float32(0.1) * r):
        keep = edges["w"] < cut
        got = components(c.n, edges["lo"][keep].astype(np.int64), edges["hi"][keep].astype(np.int64))
        assert np.array_equal(got, case_want(c, cut)[1]), cut
        assert len(np.unique(got)) > 1


def test_argument_checks_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    edges, labels = np.zeros(8, dtype=EDGE), np.zeros(9, dtype=np.int32)
    count, rounds = ctypes.c_uint64(0), ctypes.c_uint32(0)
    host = lib.ptk_host_mst_within_self
    r = np.float32(0.1)
    assert host(tree._h, p.ctypes.data, r, None, None, None, None) == INVALID
    assert host(tree._h, None, r, None, edges.ctypes.data, None, None) == INVALID
    assert host(None, p.ctypes.data, r, None, edges.ctypes.data, None, None) == INVALID
    assert host(tree._h, p.ctypes.data, r, None, edges.ctypes.data, None, None) == 0  # (n_edges and labels may be null)
    for bad in (np.nan, -0.5, -INF):
        assert host(tree._h, p.ctypes.data, np.float32(bad), None, edges.ctypes.data, None, None) == INVALID
        assert "radius must be >= 0" in lib.ptk_last_error().decode()
    for bad in (np.nan, -1e-3):
        core = np.full(9, 0.01, dtype=np.float32)
        core[4] = core[7] = bad
        assert host(tree._h, p.ctypes.data, r, core.ctypes.data, edges.ctypes.data, None, None) == INVALID
        assert "core[4]" in lib.ptk_last_error().decode()
    for metric in (pt.Metric.LPInf, pt.Metric.LNInf):
        other = pt.KdTree(p, metric, 3, device=pt.PTK_DEVICE_NONE)
        assert host(other._h, p.ctypes.data, r, None, edges.ctypes.data, None, None) == UNSUPPORTED
    # a host-only handle has no device search: PTK_ERR_DEVICE from every device entry point
    assert lib.ptk_mst_within_self(tree._h, r, None, edges.ctypes.data, ctypes.byref(count), labels.ctypes.data,
                                   ctypes.byref(rounds)) == DEVICE
    assert lib.ptk_mst_within_self_device(tree._h, r, None, edges.ctypes.data, None, None, 0, None, None, None) == DEVICE
    assert lib.ptk_mst_within_self(None, r, None, edges.ctypes.data, None, None, None) == INVALID
    need = ctypes.c_uint64(0)
    assert lib.ptk_mst_within_self_workspace(tree._h, ctypes.byref(need)) == 0 and need.value >= 9 * 28
    assert lib.ptk_mst_within_self_workspace(tree._h, None) == INVALID


def test_the_wrapper_checks_its_arguments_and_shapes_its_result(monkeypatch):
    p, r, kth, _ = core_cloud()
    tree = pt.KdTree(p, pt.Metric.L2Squared, 8, device=pt.PTK_DEVICE_NONE)
    n = len(p)
    with pytest.raises(pt.PtkError) as refused:
        tree.mst_within_self(r)
    assert refused.value.status == DEVICE
    for bad in (np.zeros(n - 1, dtype=np.float32), np.zeros((n, 1), dtype=np.float32), "x"):
        with pytest.raises(ValueError):
            tree.mst_within_self(r, core=bad)
    nan = np.zeros(n, dtype=np.float32)
    nan[17] = nan[40] = np.nan
    with pytest.raises(ValueError, match=r"core\[17\]"):
        tree.mst_within_self(r, core=nan)
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 8, device=pt.PTK_DEVICE_NONE)
    with pytest.raises(pt.PtkError) as refused:
        t64.mst_within_self(r)
    assert refused.value.status == UNSUPPORTED and "ptk_host_mst_within_self" in str(refused.value)
    lib = pt._load()

    class Served:  # the device entry point of a host-only handle, answered by the host loop
        def __getattr__(self, name):
            if name == "ptk_mst_within_self":
                def served(h, r, cp, edges, count, labels, n_rounds):
                    ctypes.cast(n_rounds, ctypes.POINTER(ctypes.c_uint32))[0] = 7
                    return lib.ptk_host_mst_within_self(h, p.ctypes.data, r, cp, edges, count, labels)
                return served
            return getattr(lib, name)

    monkeypatch.setattr(pt, "_load", lambda: Served())
    for name, core in [("none", None)] + core_cases(n, kth, r):
        want = host_mst(tree, r, core)
        edges = tree.mst_within_self(r, core=core if name != "kth" else core.astype(np.float64).tolist())
        assert edges.dtype == EDGE and edges.tobytes() == want[0].tobytes(), name
        edges, labels = tree.mst_within_self(r, core=core, labels=True)
        assert labels.dtype == np.int32 and np.array_equal(labels, want[1]) and edges.tobytes() == want[0].tobytes()
        assert tree.last_mst_rounds == 7
    import pico_tree

    assert pico_tree.KdTree.mst_within_self is pt.KdTree.mst_within_self


# ---- CPU tier: the C++ member on a host-only build ---------------------------------------------------------------------

def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mst_self_main.cpp"), "-o", out]
    if host_only:
        cmd.insert(1, "-DPICO_TREE_HOST_ONLY")
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def _cpp_run(d, host_only):
    p, r, kth, rows = core_cloud()
    p.tofile(os.path.join(d, "points.bin"))
    np.ascontiguousarray(kth).tofile(os.path.join(d, "core.bin"))
    exe = os.path.join(d, "mst_self_main")
    _cpp_program(exe, host_only)
    res = subprocess.run([exe, d, repr(float(r))], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
    tree_l1 = pt.KdTree(p, pt.Metric.L1, 10, device=pt.PTK_DEVICE_NONE)
    rows_l1 = host_search_rows(tree_l1, p, r)
    assert symmetric(*rows_l1)
    for name, want in (("l2_plain", expected_mst(*rows, r)), ("l2_core", core_want("kth")),
                       ("l1_plain", expected_mst(*rows_l1, r))):
        edges = np.fromfile(os.path.join(d, name + ".edges"), dtype=EDGE)
        labels = np.fromfile(os.path.join(d, name + ".labels"), dtype=np.int32)
        same((edges, labels), want, name)


def test_cpp_member_on_a_host_only_tree(tmp_path):
    _cpp_run(str(tmp_path), host_only=True)


# ---- CPU tier: the real kernel source in the emulator ----------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/cpp/emulate_mst.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_mst") / "libptk_emu_mst.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_mst.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    lib.emu_create.restype = vp
    lib.emu_create.argtypes = [vp, u64, u32, vp, u64, vp]
    lib.emu_destroy.argtypes = [vp]
    lib.emu_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu_mst_self.argtypes = [vp, u64, ctypes.c_float, vp, u32, ctypes.c_int, vp, vp, vp, vp]
    return lib


def emu_mst(emu, r, core=None, piece=64, snapshot=0, skip=2, info=None):
    """The rounds over an rs.Emulated tree into poisoned, guarded buffers; the edges sorted into the contract's order.
    `info`: a dict that gets the rounds and the three counters."""
    n = emu.n
    ebuf, edges = rs.guarded(max(n - 1, 0), EDGE)
    lbuf, labels = rs.guarded(n, np.int32)
    count = ctypes.c_uint32(0)
    stats = np.zeros(3, dtype=np.uint32)
    rounds = emu.lib.emu_mst_self(emu.h, piece, np.float32(r), _ptr(core), skip, snapshot, edges.ctypes.data,
                                  labels.ctypes.data, ctypes.byref(count), stats.ctypes.data)
    assert rounds >= 0, rounds
    assert rs.guards_intact(ebuf) and rs.guards_intact(lbuf), "written outside a buffer"
    if info is not None:
        info.update(rounds=rounds, comp=int(stats[0]), box=int(stats[1]), scan=int(stats[2]))
    got = edges[:count.value].copy()
    order = np.lexsort((got["hi"], got["lo"], got["w"].view(np.uint32)))
    return got[order], labels.copy()


def emu_both(emu, r, core=None, piece=64, skip=2, info=None):
    """Both schedules must give the same edges and labels."""
    live = emu_mst(emu, r, core, piece, 0, skip, info)
    stale = emu_mst(emu, r, core, piece, 1, skip)
    assert live[0].tobytes() == stale[0].tobytes() and np.array_equal(live[1], stale[1]), \
        "the result depends on what a load happens to see"
    return live


@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_kernels_equal_the_contract(emu_lib, kind, metric):
    """Pieces of 64 leaf positions, 647 (pieces that end inside a wavefront) and the whole tree; both schedules; with and
    without the component table, and with the root and the far children tested only; with core distances."""
    c = rs.case(kind, metric)
    emu = rs.Emulated(emu_lib, c.p, c.leaf, metric)
    bound = int(np.ceil(np.log2(c.n))) + 1
    for turn, r in enumerate(c.values()):
        info = {}
        same(emu_both(emu, r, None, (64, 647, 0)[turn % 3], 2, info), case_want(c, r), (kind, metric, r))
        assert info["rounds"] <= bound, info
    r = c.values()[2]
    for skip in (0, 1):
        same(emu_mst(emu, r, None, 647, 0, skip), case_want(c, r), (kind, metric, "skip", skip))
    same(emu_both(emu, r, c.kth(), 647), case_want(c, r, True), (kind, metric, "core"))


@pytest.mark.parametrize("name", CONSTRUCTED)
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_kernels_on_the_constructed_clouds(emu_lib, name, metric):
    p, leaf, radii = constructed(name)
    emu = rs.Emulated(emu_lib, p, leaf, metric)
    for r in radii:
        r = radius_value(r, metric)
        want = constructed_want(name, metric, r)
        with_table, without = {}, {}
        same(emu_both(emu, r, None, 64, 2, with_table), want, (name, metric, r))
        same(emu_mst(emu, r, None, 0, 0, 0, without), want, (name, metric, r, "mst_skip=0"))
        assert without["comp"] == 0
        if name.startswith("blobs") and r == np.float32(INF):
            # the last rounds join whole subtrees: the component skip fires, and saves most of the leaf scans
            assert with_table["comp"] > 0 and with_table["scan"] < without["scan"] // 2, (with_table, without)


@pytest.mark.parametrize("metric", METRICS)
def test_emulated_kernels_on_tiny_trees(emu_lib, metric):
    for p, leaf in tiny_cases():
        emu = rs.Emulated(emu_lib, p, leaf, metric)
        for r in (np.float32(0), np.float32(0.3), FLT_MAX, np.float32(INF)):
            _, want = tiny_want(p, leaf, metric, r)
            same(emu_both(emu, r), want, (len(p), leaf, r))


@pytest.mark.parametrize("name", ["kth", "equal", "isolated"])
def test_emulated_kernels_with_core_distances(emu_lib, name):
    p, r, kth, _ = core_cloud()
    core = dict(core_cases(len(p), kth, r))[name]
    emu = rs.Emulated(emu_lib, p, 8, "L2Squared")
    same(emu_both(emu, r, core, 647), core_want(name), name)
    same(emu_mst(emu, r, core, 0, 0, 0), core_want(name), (name, "mst_skip=0"))
    if name == "kth":  # a NaN and a negative entry (the _device form cannot look): the point has no edges
        bad = core.copy()
        bad[100], bad[1500] = np.nan, -1.0
        edges, labels = emu_both(emu, r, bad, 64)
        ok = core.copy()
        ok[[100, 1500]] = r  # (the same graph: an entry at the radius isolates its point)
        _, _, _, rows = core_cloud()
        same((edges, labels), expected_mst(*rows, r, ok), "bad core entries")
        assert labels[100] == 100 and labels[1500] == 1500


@pytest.mark.parametrize("L", [1, 8, 32, 33])
def test_emulated_kernels_where_the_leaf_scan_changes(emu_lib, L):
    """Leaf sizes 1 and 8 on a small cloud; a leaf of exactly 32 and 33 points (tests/leaf_cases.py)."""
    if L < 32:
        p = ds.uniform_cloud(700, 3, 200 + L)
    else:
        p, _ = leaf_cases.cloud_with_leaf(L, n=600)
    for metric in METRICS:
        emu = rs.Emulated(emu_lib, p, L, metric)
        for r in (np.float32(0.02), np.float32(INF)):
            rows = host_search_rows(emu.host, p, r)
            assert symmetric(*rows)
            same(emu_both(emu, r, None, 64), expected_mst(*rows, r), (L, metric, r))


@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 10, "L2Squared"), (2, 4, "L1")])
def test_emulated_kernels_where_the_stack_class_changes(emu_lib, dim, leaf, metric, depth):
    pts, _ = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    emu = rs.Emulated(emu_lib, pts, leaf, metric)
    r = np.float32(0.05 if metric == "L1" else 0.003)
    rows = host_search_rows(emu.host, pts, r)
    assert symmetric(*rows)
    same(emu_mst(emu, r, None, 647), expected_mst(*rows, r), (depth, metric))


def foreign_stream(move):
    """(tree points, searched points): a shrunk or shifted copy of the tree's points (tests/test_radius_self.py)."""
    p_tree = ds.uniform_cloud(3_000, 3, 61)
    p = (p_tree * np.float32(0.5) + np.float32(0.25)) if move == "shrunk" else (p_tree + np.float32(0.3))
    return p_tree, np.ascontiguousarray(p, dtype=np.float32)


def check_foreign(got, rows, n, r):
    """A spanning forest of the graph's components whose every edge is in the rows (minimality is not promised)."""
    edges, labels = got
    bits, lo, hi = graph_edges(*rows, r)
    want_labels = components(n, lo, hi)
    assert np.array_equal(labels, want_labels)
    assert len(edges) == n - len(np.unique(want_labels))
    have = set(zip(bits.tolist(), lo.tolist(), hi.tolist()))
    for e in edges:
        assert (int(np.float32(e["w"]).view(np.uint32)), int(e["lo"]), int(e["hi"])) in have
    assert np.array_equal(components(n, edges["lo"].astype(np.int64), edges["hi"].astype(np.int64)), want_labels)


@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_emulated_kernels_on_a_stream_that_does_not_belong_to_its_points(emu_lib, move):
    p_tree, p = foreign_stream(move)
    emu = rs.Emulated(emu_lib, p, 8, "L2Squared", tree_points=p_tree)
    asym = 0
    for r in (np.float32(0.001), np.float32(0.004)):
        rows = host_search_rows(emu.host, p, r)
        asym += 0 if symmetric(*rows) else 1
        for snapshot in (0, 1):
            check_foreign(emu_mst(emu, r, None, 647, snapshot), rows, len(p), r)
        check_foreign(host_mst(emu.host, r, None, points=p), rows, len(p), r)
    assert asym > 0, "every row is symmetric: the stream tells nothing apart"


# ---- gpu tier ---------------------------------------------------------------------------------------------------------

def device_mst(tree, r, core=None, rounds=None):
    """The host-buffer form into poisoned, guarded buffers."""
    lib = pt._load()
    n_rounds = ctypes.c_uint32(0)
    got = guarded_call(tree.npts, lambda e, l, c: lib.ptk_mst_within_self(tree._h, np.float32(r), _ptr(core), e, c, l,
                                                                         ctypes.byref(n_rounds)))
    if rounds is not None:
        rounds.append(n_rounds.value)
    return got


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_equals_the_contract(gpu, kind, metric, monkeypatch):
    c = rs.case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    bound = int(np.ceil(np.log2(c.n))) + 1
    for r in c.values():
        rounds = []
        got = device_mst(tree, r, None, rounds)
        same(got, case_want(c, r), (kind, metric, r))
        assert rounds[0] <= bound
        assert np.array_equal(got[1], tree.cluster_within_self(r, 0))
    r = c.values()[2]
    same(device_mst(tree, r, c.kth()), case_want(c, r, True), (kind, metric, "core"))
    edges, labels = tree.mst_within_self(r, labels=True)
    same((edges, labels), case_want(c, r), "wrapper")
    assert 1 <= tree.last_mst_rounds <= bound
    monkeypatch.setenv("PTK_MAX_BATCH", "1000")  # pieces that end inside a wavefront
    same(device_mst(tree, r), case_want(c, r), (kind, metric, "pieces"))
    monkeypatch.delenv("PTK_MAX_BATCH")
    for skip in (0, 1):
        monkeypatch.setenv("PTK_TEST_KNOBS", f"mst_skip={skip}")
        same(device_mst(tree, r), case_want(c, r), (kind, metric, "mst_skip", skip))
    monkeypatch.delenv("PTK_TEST_KNOBS")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONSTRUCTED)
@pytest.mark.parametrize("metric", METRICS)
def test_constructed_clouds_on_the_device(gpu, name, metric, monkeypatch):
    p, leaf, radii = constructed(name)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
    for r in radii:
        r = radius_value(r, metric)
        want = constructed_want(name, metric, r)
        first = device_mst(tree, r)
        same(first, want, (name, metric, r))
        assert device_mst(tree, r)[0].tobytes() == first[0].tobytes()  # two calls give identical bytes
        monkeypatch.setenv("PTK_TEST_KNOBS", "mst_skip=0")
        same(device_mst(tree, r), want, (name, metric, r, "mst_skip=0"))
        monkeypatch.delenv("PTK_TEST_KNOBS")


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_tiny_trees_on_the_device(gpu, metric):
    for p, leaf in tiny_cases():
        tree = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=gpu)
        for r in (np.float32(0), np.float32(0.3), FLT_MAX, np.float32(INF)):
            _, want = tiny_want(p, leaf, metric, r)
            same(device_mst(tree, r), want, (len(p), leaf, r))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kth", "equal", "isolated"])
def test_core_distances_on_the_device(gpu, name):
    p, r, kth, _ = core_cloud()
    tree = pt.KdTree(p, pt.Metric.L2Squared, 8, device=gpu)
    if name == "kth":  # the recipe: spacing_knn_self(k, kth=True) in the metric's unit -> mst_within_self(core=kth)
        _, dev_kth = tree.spacing_knn_self(4, sqrt=False, kth=True)
        assert dev_kth.tobytes() == kth.tobytes()
    core = dict(core_cases(len(p), kth, r))[name]
    same(device_mst(tree, r, core), core_want(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("n,batch", [(5_000, None), (20_000, 6_000)])
def test_larger_clouds_against_the_host_loop(gpu, n, batch, monkeypatch):
    """5 000 random points: several blocks, about a dozen rounds.  20 000 clustered points with PTK_MAX_BATCH set so that
    a round is several pieces.  Compared with the host loop (itself compared with the contract at n <= 2 000 above)."""
    if batch is None:  # (0.15 squared: some 70 neighbours per row -- the host loop keeps every row -- and one component)
        p, r = ds.uniform_cloud(n, 3, 301), np.float32(0.0225)
    else:
        p, r = ds.lidar_cloud(n, seed=9), None
    host = pt.KdTree(p, pt.Metric.L2Squared, 10, device=pt.PTK_DEVICE_NONE)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    if r is None:
        r = np.float32(8) * np.float32(np.median(tree.spacing_knn_self(8, sqrt=False)))
        monkeypatch.setenv("PTK_MAX_BATCH", str(batch))
    rounds = []
    got = device_mst(tree, r, None, rounds)
    monkeypatch.delenv("PTK_MAX_BATCH", raising=False)
    same(got, host_mst(host, r), n)
    assert 2 <= rounds[0] <= int(np.ceil(np.log2(n))) + 1, rounds
    if batch is None:
        assert len(got[0]) == n - 1


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 8, 32, 33])
def test_leaf_sizes_on_the_device(gpu, L):
    p = ds.uniform_cloud(700, 3, 200 + L) if L < 32 else leaf_cases.cloud_with_leaf(L, n=600)[0]
    for metric in METRICS:
        tree = pt.KdTree(p, getattr(pt.Metric, metric), L, device=gpu)
        for r in (np.float32(0.02), np.float32(INF)):
            rows = host_search_rows(tree, p, r)
            assert symmetric(*rows)
            same(device_mst(tree, r), expected_mst(*rows, r), (L, metric, r))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 10, "L2Squared"), (2, 4, "L1")])
def test_depths_where_the_stack_class_changes(gpu, dim, leaf, metric, depth):
    pts = np.asarray(depth_cases.cloud_at_depth(depth, dim, leaf)[0])
    tree = pt.KdTree(pts, getattr(pt.Metric, metric), leaf, device=gpu)
    depth_cases.assert_depth(tree, depth)
    r = np.float32(0.05 if metric == "L1" else 0.003)
    rows = host_search_rows(tree, pts, r)
    assert symmetric(*rows)
    same(device_mst(tree, r), expected_mst(*rows, r), (depth, metric))


@pytest.mark.gpu
@needs_reference
def test_cutting_the_device_forest_gives_the_device_clusters(gpu):
    c = rs.case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    r = c.values()[2]
    edges = tree.mst_within_self(r)
    for cut in (c.values()[1], np.float32(0.5) * r, np.float32(0.1) * r):
        keep = edges["w"] < cut
        got = components(c.n, edges["lo"][keep].astype(np.int64), edges["hi"][keep].astype(np.int64))
        assert np.array_equal(got, tree.cluster_within_self(cut, 0)), cut


@pytest.mark.gpu
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_streams_that_do_not_belong_to_their_points(gpu, tmp_path, move):
    p_tree, p = foreign_stream(move)
    fn = str(tmp_path / "tree.bin")
    pt.save_kd_tree(pt.KdTree(p_tree, pt.Metric.L2Squared, 8, device=pt.PTK_DEVICE_NONE), fn)
    tree = pt.load_kd_tree(p, fn, device=gpu)
    for r in (np.float32(0.001), np.float32(0.004)):
        rows = host_search_rows(tree, p, r)
        got = device_mst(tree, r)
        check_foreign(got, rows, len(p), r)
        assert np.array_equal(got[1], tree.cluster_within_self(r, 0))


@pytest.mark.gpu
def test_a_stream_under_capture_is_refused_by_name(gpu):
    import torch

    p = rs.cloud("small")[0]
    tree = pt.KdTree(p, pt.Metric.L2Squared, 5, device=gpu)
    lib = pt._load()
    need = ctypes.c_uint64(0)
    assert lib.ptk_mst_within_self_workspace(tree._h, ctypes.byref(need)) == 0
    ws = torch.zeros(need.value, dtype=torch.uint8, device=f"cuda:{gpu}")
    edges = torch.zeros((tree.npts - 1, 3), dtype=torch.int32, device=f"cuda:{gpu}")
    count = ctypes.c_uint64(0)
    side = torch.cuda.Stream(device=gpu)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()

    def call(stream):
        return lib.ptk_mst_within_self_device(tree._h, np.float32(0.01), None, edges.data_ptr(), None, ws.data_ptr(),
                                              need.value, ctypes.byref(count), None, stream)

    with torch.cuda.graph(graph, stream=side):
        edges.fill_(7)
        rc = call(torch.cuda.current_stream().cuda_stream)
        message = lib.ptk_last_error().decode()
    assert rc == INVALID and "captured" in message, (rc, message)
    torch.cuda.synchronize()
    assert call(side.cuda_stream) == 0  # outside a capture the same call serves
    side.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == count.value  # (the count in the workspace's header)


@pytest.mark.gpu
@needs_reference
def test_torch_device_form_on_a_side_stream(gpu):
    """The _device entry point on a side stream with guard bytes around the edge buffer, the labels and the workspace;
    the wrapper's device form, plain and with core as a CUDA tensor (a NaN entry: a point without edges)."""
    import torch

    c = rs.case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    lib = pt._load()
    dev = f"cuda:{gpu}"
    side = torch.cuda.Stream(device=gpu)
    r = c.values()[2]
    need = ctypes.c_uint64(0)
    assert lib.ptk_mst_within_self_workspace(tree._h, ctypes.byref(need)) == 0
    G = 256
    count, n_rounds = ctypes.c_uint64(0), ctypes.c_uint32(0)
    bad = np.array(c.kth())
    bad[100] = np.nan
    with torch.cuda.stream(side):
        ws = torch.full((need.value + 2 * G,), 0xA5, dtype=torch.uint8, device=dev)
        ebuf = torch.full(((c.n - 1) * 12 + 2 * G,), 0xA5, dtype=torch.uint8, device=dev)
        lbuf = torch.full((c.n * 4 + 2 * G,), 0xA5, dtype=torch.uint8, device=dev)
        assert lib.ptk_mst_within_self_device(tree._h, np.float32(r), None, ebuf[G:].data_ptr(), lbuf[G:].data_ptr(),
                                              ws[G:].data_ptr(), need.value, ctypes.byref(count), ctypes.byref(n_rounds),
                                              side.cuda_stream) == 0
        short = lib.ptk_mst_within_self_device(tree._h, np.float32(r), None, ebuf[G:].data_ptr(), None, ws[G:].data_ptr(),
                                               need.value - 1, None, None, side.cuda_stream)
        short_message = lib.ptk_last_error().decode()
        lo, hi, w = tree.mst_within_self(r, device=True)
        (lo2, hi2, w2), labels = tree.mst_within_self(r, core=torch.from_numpy(bad).to(dev), labels=True, device=True)
    side.synchronize()
    want = case_want(c, r)
    for buf in (ws, ebuf, lbuf):
        raw = buf.cpu().numpy()
        assert np.all(raw[:G] == 0xA5) and np.all(raw[-G:] == 0xA5)
    assert short == INVALID and "workspace" in short_message
    assert count.value == len(want[0]) and 1 <= n_rounds.value
    got = ebuf.cpu().numpy()[G:G + 12 * count.value].view(EDGE)
    got = got[np.lexsort((got["hi"], got["lo"], got["w"].view(np.uint32)))]  # (the _device form writes the set unordered)
    assert got.tobytes() == want[0].tobytes()
    assert np.array_equal(lbuf.cpu().numpy()[G:-G].view(np.int32), want[1])
    assert lo.dtype == torch.int32 and w.dtype == torch.float32
    assert np.array_equal(lo.cpu().numpy(), want[0]["lo"]) and np.array_equal(hi.cpu().numpy(), want[0]["hi"])
    assert w.cpu().numpy().tobytes() == want[0]["w"].tobytes()
    ok = np.array(c.kth())
    ok[100] = r
    edges2, labels2 = expected_mst(*c.want(r), r, ok)
    assert np.array_equal(lo2.cpu().numpy(), edges2["lo"]) and np.array_equal(hi2.cpu().numpy(), edges2["hi"])
    assert w2.cpu().numpy().tobytes() == edges2["w"].tobytes() and np.array_equal(labels.cpu().numpy(), labels2)
    with pytest.raises(ValueError):
        tree.mst_within_self(r, core=bad, device=True)  # (a host array is checked before it goes up)


def _refused(tree, reason):
    with pytest.raises(pt.PtkError) as refused:
        tree.mst_within_self(0.01)
    assert refused.value.status == UNSUPPORTED
    assert reason in str(refused.value) and "ptk_host_mst_within_self" in str(refused.value), str(refused.value)


@pytest.mark.gpu
def test_refused_handles_and_the_host_loop_that_serves_them(gpu):
    p = ds.uniform_cloud(2_000, 3, 12)
    _refused(pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 8, device=gpu), "float64")
    _refused(pt.KdTree(p, pt.Metric.LPInf, 8, device=gpu), "metric_lpinf")
    _refused(pt.KdTree(p, pt.Metric.LNInf, 8, device=gpu), "metric_lninf")
    _refused(pt.KdTree(np.ascontiguousarray(p[:, :1]), pt.Metric.SO2, 8, device=gpu), "topological")
    p5 = ds.uniform_cloud(1_500, 5, 13)
    t5 = pt.KdTree(p5, pt.Metric.L2Squared, 8, device=gpu)
    _refused(t5, "dim > 3")
    deep = np.asarray(depth_cases.cloud_at_depth(1032, 3, 10)[0])
    tree = pt.KdTree(deep, pt.Metric.L2Squared, 10, device=gpu)
    _refused(tree, "tree depth 1032")
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got = tree.mst_within_self(0.001, labels=True)
            got5 = t5.mst_within_self(0.05, labels=True)
    finally:
        pt.allow_host_loop(False)
    same(got, expected_mst(*host_search_rows(tree, deep, np.float32(0.001)), 0.001), "deep")
    same(got5, expected_mst(*host_search_rows(t5, p5, np.float32(0.05)), 0.05), "5d")
    # the argument checks of the device entry points
    lib = pt._load()
    small = pt.KdTree(rs.cloud("small")[0], pt.Metric.L2Squared, 5, device=gpu)
    edges = np.zeros(small.npts, dtype=EDGE)
    bad = np.full(small.npts, 0.001, dtype=np.float32)
    bad[7] = bad[9] = np.nan
    assert lib.ptk_mst_within_self(small._h, np.float32(0.1), None, None, None, None, None) == INVALID
    assert lib.ptk_mst_within_self(small._h, np.float32(np.nan), None, edges.ctypes.data, None, None, None) == INVALID
    assert lib.ptk_mst_within_self(small._h, np.float32(-1), None, edges.ctypes.data, None, None, None) == INVALID
    assert lib.ptk_mst_within_self(small._h, np.float32(1), bad.ctypes.data, edges.ctypes.data, None, None, None) == INVALID
    assert "core[7]" in lib.ptk_last_error().decode()
    assert lib.ptk_mst_within_self_device(small._h, np.float32(0.1), None, edges.ctypes.data, None, None, 1 << 30, None, None,
                                          None) == INVALID
    assert lib.ptk_mst_within_self(small._h, np.float32(0.1), None, edges.ctypes.data, None, None, None) == 0


@pytest.mark.gpu
def test_the_radius_capture_and_the_other_searches_are_left_alone(gpu):
    """A scalar search_radius count / fill pair with mst calls between its halves still returns its rows; the other self
    searches of the handle give the bytes they gave before."""
    import torch

    p, q = ds.uniform_cloud(20_000, 3, 71), ds.uniform_cloud(6_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)

    def others():
        return [tree.count_within_self(0.001).tobytes(), tree.search_radius_self(0.001).flat.tobytes(),
                tree.cluster_within_self(0.001, min_neighbors=3).tobytes(), tree.suppress_within_self(0.001).tobytes(),
                tree.search_knn(q, 1).tobytes()]

    before = others()
    lib = pt._load()
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    stream = torch.cuda.current_stream(dq.device).cuda_stream
    want = tree.search_radius(q, 0.002)
    counts = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                              counts.data_ptr(), stream) == 0
    lo, hi, w = tree.mst_within_self(0.001, device=True)
    host_form = tree.mst_within_self(0.001)
    offsets = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    offsets[1:] = torch.cumsum(counts[:len(q)], 0)
    out = torch.empty((max(int(offsets[-1].item()), 1), 2), dtype=torch.int32, device=dq.device)
    assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                             offsets.data_ptr(), out.data_ptr(), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want.offsets)
    assert rs.raw_rows(out)[:len(want.flat)].tobytes() == want.flat.tobytes()
    rows = tree.search_radius_self(0.001)
    assert host_form.tobytes() == expected_mst(rows.offsets, rows.flat, 0.001)[0].tobytes()
    assert np.array_equal(lo.cpu().numpy(), host_form["lo"]) and w.cpu().numpy().tobytes() == host_form["w"].tobytes()
    assert others() == before


@pytest.mark.gpu
def test_cpp_batched_member(gpu, tmp_path):
    _cpp_run(str(tmp_path), host_only=False)
