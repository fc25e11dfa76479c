"""cluster_within_self: the connected components of the fixed-radius graph over a tree's own points, with DBSCAN's
core-point rule (ptk.h).

Every expected value is an integer fixed by the contract.  ``expected_labels`` below is the contract written out -- a
sequential union-find over rows, then the border rule -- applied to rows obtained independently of the feature: the
compiled reference's ``search_radius`` rows of the tree's own points with the own entry removed (the clouds and ``Case``
of tests/test_radius_self.py, shared with it), or, on trees the reference cannot build (streams that do not belong to
their points, the constructed cases), the library's host loop ``ptk_host_search_radius``.  The constructed cases carry a
second, hand-written expectation.  Comparison is exact equality of the whole array.

The CPU tier checks the host loop on a host-only handle, the real kernel source in the emulator
(tests/cpp/emulate_cluster.cpp), the union-find itself on 16 threads under ThreadSanitizer (tests/cpp/cluster_threads.cpp,
a stand-alone program), the C++ members (tests/cpp/cluster_self_main.cpp) and the Python wrapper; the gpu tier checks the
device passes, float32 and float64.
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
FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")
METRICS = rs.METRICS
POISON32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]

needs_reference = rs.needs_reference
needs_reference64 = rs.needs_reference64


# ---- the contract, written out ---------------------------------------------------------------------------------------

def expected_labels(off, flat, min_neighbors):
    """Labels of the rows (offsets, flat records with an ``index`` field; own entries already removed)."""
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    row, idx = rs.row_ids(off), np.asarray(flat["index"]).astype(np.int64)
    core = np.diff(off) >= min_neighbors
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    both = core[row] & core[idx]  # (an edge in either direction joins: the union does not ask which)
    lo, hi = np.minimum(row[both], idx[both]), np.maximum(row[both], idx[both])
    for key in np.unique(lo * n + hi).tolist():
        a, b = find(key // n), find(key % n)
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.full(n, -1, dtype=np.int64)
    for i in np.flatnonzero(core).tolist():
        labels[i] = find(i)  # (the smaller root always stays: the root is the component's smallest index)
    border = ~core[row] & core[idx]  # a non-core point looks at the core points of ITS OWN row only
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, row[border], labels[idx[border]])
    take = ~core & (best < np.iinfo(np.int64).max)
    labels[take] = best[take]
    return labels.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _want_scalar(kind, metric, dtype, r, mn):
    c = rs.case(kind, metric, dtype)
    out = expected_labels(*c.want(c.dtype.type(r)), mn)
    out.flags.writeable = False
    return out


def want_scalar(c, r, mn):
    """Expected labels of a Case at the scalar radius r: computed once, shared by the tiers."""
    return _want_scalar(c.kind, c.metric, c.dtype.name, float(r), int(mn))


@functools.lru_cache(maxsize=None)
def _want_radii(kind, metric, dtype, mn):
    out = expected_labels(*rs.case(kind, metric, dtype).want_per_row(), mn)
    out.flags.writeable = False
    return out


def want_radii(c, mn):
    return _want_radii(c.kind, c.metric, c.dtype.name, int(mn))


def own_radii(c):
    """The scalar radii of a case: 0, the median 8th-neighbour distance, 4 x it; on "ties" the grid step and the next
    number above it as well."""
    return c.values()[:5 if c.kind == "ties" else 3]


def host_search_rows(tree, p, r):
    """(offsets, flat) of the library's host loop ptk_host_search_radius / _radii over the points themselves, the own
    entries removed: the rows of a tree and points pair the reference cannot build."""
    lib = pt._load()
    p = np.ascontiguousarray(p, dtype=np.float32)
    off = np.zeros(len(p) + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    if np.ndim(r) == 0:
        rc = lib.ptk_host_search_radius(tree._h, p.ctypes.data, p.ctypes.data, len(p), np.float32(r), np.float32(1), 0,
                                        off.ctypes.data, ctypes.byref(rows))
    else:
        rc = lib.ptk_host_search_radius_radii(tree._h, p.ctypes.data, p.ctypes.data, len(p), r.ctypes.data, 0,
                                              off.ctypes.data, ctypes.byref(rows))
    assert rc == 0, lib.ptk_last_error()
    return rs.without_self(off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR))


def guarded_labels(n):
    """(whole buffer, the n entries) of an int32 output between two runs of guard entries, all 0xA5 bytes."""
    return rs.guarded(n, np.int32)


def written(buf, labels):
    return rs.guards_intact(buf) and not np.any(labels == POISON32)


def host_labels(tree, r, mn, points=None):
    """ptk_host_cluster_within_self into a guarded buffer; r a scalar or an array."""
    lib = pt._load()
    p = tree._pts if points is None else points
    buf, labels = guarded_labels(len(p))
    n_clusters = ctypes.c_uint64(12345)
    scalar = np.ndim(r) == 0
    rc = lib.ptk_host_cluster_within_self(tree._h, p.ctypes.data, np.float32(r if scalar else 0),
                                          None if scalar else r.ctypes.data, mn, labels.ctypes.data,
                                          ctypes.byref(n_clusters))
    assert rc == 0, lib.ptk_last_error()
    assert written(buf, labels), "a label was not written, or one was written outside"
    assert n_clusters.value == int((labels == np.arange(len(p))).sum())
    return labels.copy()


# ---- CPU tier: the host loop on a host-only handle -------------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "5d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_equals_the_expected_labels(kind, metric):
    c = rs.case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    for r in own_radii(c):
        for mn in (0, 1, 4, c.n):
            got = host_labels(tree, r, mn)
            assert np.array_equal(got, want_scalar(c, r, mn)), (kind, metric, r, mn)
            if mn == c.n:
                assert np.all(got == -1)  # (a row has at most n - 1 entries: nothing is core)
        if r == 0:
            assert np.array_equal(host_labels(tree, r, 0), np.arange(c.n))
    radii = c.radii()
    for mn in (0, 4):
        assert np.array_equal(host_labels(tree, radii, mn), want_radii(c, mn)), (kind, metric, "per row", mn)


@needs_reference
def test_the_expected_labels_tell_the_rules_apart():
    """On the data of this module the pieces of the contract all matter: there are several clusters, border points and
    noise at min_neighbors = 4, border points with core neighbours of two clusters, and asymmetric rows under the
    per-point radii."""
    c = rs.case("lidar", "L2Squared")
    r = own_radii(c)[1]
    off, flat = c.want(r)
    off = off.astype(np.int64)
    labels = want_scalar(c, r, 4)
    core = np.diff(off) >= 4
    assert len(np.unique(labels[core])) > 3 and np.any(labels[~core] >= 0) and np.any(labels == -1)
    row, idx = rs.row_ids(off), flat["index"]
    seen = {}
    for i, j in zip(row[~core[row] & core[idx]].tolist(), idx[~core[row] & core[idx]].tolist()):
        seen.setdefault(i, set()).add(int(labels[j]))
    assert any(len(s) > 1 for s in seen.values()), "no border point sees two clusters: 'first found' would pass"
    off, flat = c.want_per_row()
    row, idx = rs.row_ids(off), flat["index"].astype(np.int64)
    forward = set((row * c.n + idx).tolist())
    assert any((j * c.n + i) not in forward for i, j in zip(row.tolist(), idx.tolist())), "the rows are symmetric"


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loop_of_the_topological_metrics(metric):
    rng = np.random.default_rng(12)
    p = rng.random((2_000, 1 if metric == "SO2" else 3), dtype=np.float32)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    med = np.float32(np.median(ref.search_knn(p, 9)["distance"][:, 8]))
    for r in (np.float32(0), med, np.float32(4) * med):
        rows = rs.without_self(*ref.search_radius(p, r))
        for mn in (0, 1, 4, len(p)):
            assert np.array_equal(host_labels(tree, r, mn), expected_labels(*rows, mn)), (metric, r, mn)


# ---- the constructed cases (1-D, metric_l1, r = 0.4, min_neighbors = 3) ---------------------------------------------
# Every number has a margin of at least 0.05 from the radius.  A case is (values, component of each value or None for a
# non-core point, the components a non-core point's row touches); the hand-written expectation follows from those under
# any order of the points: a component's label is the smallest index of its core points.

A = [0.0, 0.1, 0.2, 0.3]
B = [1.0, 1.1, 1.2, 1.3]
CONSTRUCTED = {
    # A and B are two clusters: the point at 0.65 reaches 0.3 and 1.0 (0.35 < 0.4) but has only those two neighbours --
    # non-core, so it joins nothing, and takes the smaller of the two labels
    "a": (A + B + [0.65], ["A"] * 4 + ["B"] * 4 + [None], {8: ["A", "B"]}),
    # 0.65 reaches 0.3 and 1.0: non-core, a border point of A.  1.0 reaches 0.65 only -- a non-core point -- so it is
    # noise: a border point passes nothing on
    "b": (A + [0.65, 1.0], ["A"] * 4 + [None, None], {4: ["A"], 5: []}),
}


def arrangements(n):
    """(mirror, order): both mirror images, each in the given order and shuffled by two fixed seeds."""
    for mirror in (False, True):
        yield mirror, np.arange(n)
        for seed in (7, 1234):
            yield mirror, np.random.default_rng(seed).permutation(n)


def arrange(values, mirror, order):
    v = np.asarray(values, dtype=np.float32)
    v = (np.float32(v.max()) - v) if mirror else v
    return np.ascontiguousarray(v[order].reshape(-1, 1))


def hand_labels(comps, touches, order):
    """The hand-written expectation after `order` (point k of the new order is point order[k] of the case)."""
    n = len(order)
    smallest = {}
    for k in range(n):
        cname = comps[order[k]]
        if cname is not None:
            smallest.setdefault(cname, k)
    out = np.empty(n, dtype=np.int32)
    for k in range(n):
        cname = comps[order[k]]
        if cname is not None:
            out[k] = smallest[cname]
        else:
            out[k] = min((smallest[t] for t in touches[order[k]]), default=-1)
    return out


def chain_cases():
    """(values, r, min_neighbors, components, touches) of the 4096-chain at spacing 1.0 with r = 1.5."""
    n = 4096
    full = [float(i) for i in range(n)]
    yield "whole", full, 0, ["C"] * n, {}
    # the two end points have one neighbour: border points of the one cluster
    yield "ends", full, 2, [None] + ["C"] * (n - 2) + [None], {0: ["C"], n - 1: ["C"]}
    cut = full[:n // 2] + full[n // 2 + 1:]
    yield "cut", cut, 0, ["L"] * (n // 2) + ["R"] * (n - 1 - n // 2), {}


def pile_cloud():
    """200 coincident points and 50 scattered ones (3-D); point 0 is a scattered one."""
    p = ds.uniform_cloud(250, 3, 44)
    pile = np.arange(250) % 5 != 0  # 200 of them
    p[pile] = np.float32(0.5)
    return np.ascontiguousarray(p), pile


class ByHostLoop:
    """labels(points, metric, leaf, r, min_neighbors) through ptk_host_cluster_within_self on a host-only handle; `rows`
    gives the rows of the same tree by the host loop of search_radius."""

    def tree(self, p, metric, leaf):
        return pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)

    def labels(self, tree, p, r, mn):
        return host_labels(tree, r, mn)


def check_constructed(how):
    """Cases (a) to (e) through `how` (the host loop, the emulator, the device): against the hand-written labels and
    against the contract applied to the host loop's rows."""
    for name, (values, comps, touches) in CONSTRUCTED.items():
        for mirror, order in arrangements(len(values)):
            p = arrange(values, mirror, order)
            tree = how.tree(p, "L1", 2)
            got = how.labels(tree, p, np.float32(0.4), 3)
            assert np.array_equal(got, hand_labels(comps, touches, order)), (name, mirror, order.tolist(), got.tolist())
            assert np.array_equal(got, expected_labels(*host_search_rows(tree, p, np.float32(0.4)), 3)), (name, mirror)
    for name, values, mn, comps, touches in chain_cases():
        for mirror, order in arrangements(len(values)):
            p = arrange(values, mirror, order)
            tree = how.tree(p, "L1", 4)
            got = how.labels(tree, p, np.float32(1.5), mn)
            want = hand_labels(comps, touches, order)
            assert np.array_equal(got, want), (name, mirror, np.flatnonzero(got != want)[:5])
            if name == "whole":
                assert np.all(got == 0)
            if name == "cut":
                assert len(np.unique(got)) == 2
        assert np.array_equal(want, expected_labels(*host_search_rows(tree, p, np.float32(1.5)), mn)), name
    # (d) a pile of coincident points: one cluster at any r > 0, singletons at r = 0
    p, pile = pile_cloud()
    tree = how.tree(p, "L2Squared", 3)
    first = int(np.flatnonzero(pile)[0])
    for r in (np.float32(1e-30), np.float32(1e-6), np.finfo(np.float32).smallest_subnormal):
        got = how.labels(tree, p, r, 0)
        assert np.all(got[pile] == first) and np.array_equal(got[~pile], np.flatnonzero(~pile)), r
        got = how.labels(tree, p, r, 3)
        assert np.all(got[pile] == first) and np.all(got[~pile] == -1), r
    assert np.array_equal(how.labels(tree, p, np.float32(0), 0), np.arange(len(p)))
    assert np.all(how.labels(tree, p, np.float32(0), 1) == -1)
    # (e) n = 1, 2, 3
    for n in (1, 2, 3):
        p = ds.uniform_cloud(n, 3, 21)
        tree = how.tree(p, "L2Squared", 3)
        for r in (0.0, 0.05, 10.0, INF):
            rows = host_search_rows(tree, p, np.float32(r))
            for mn in (0, 1, 2, 3):
                assert np.array_equal(how.labels(tree, p, np.float32(r), mn), expected_labels(*rows, mn)), (n, r, mn)
        assert np.all(how.labels(tree, p, np.float32(INF), 0) == 0)


def test_constructed_cases_on_the_host_loop():
    check_constructed(ByHostLoop())


def test_argument_checks_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    labels = np.zeros(9, dtype=np.int32)
    ok = np.full(9, 0.1, dtype=np.float32)
    n_clusters = ctypes.c_uint64(0)
    INVALID, DEVICE = -1, -3
    host = lib.ptk_host_cluster_within_self
    assert host(tree._h, p.ctypes.data, np.float32(0.1), None, 0, None, None) == INVALID
    assert host(tree._h, None, np.float32(0.1), None, 0, labels.ctypes.data, None) == INVALID
    assert host(None, p.ctypes.data, np.float32(0.1), None, 0, labels.ctypes.data, None) == INVALID
    assert host(tree._h, p.ctypes.data, np.float32(0.1), None, 0, labels.ctypes.data, None) == 0  # (n_clusters may be null)
    for bad in (np.nan, -0.5, -INF):
        assert host(tree._h, p.ctypes.data, np.float32(bad), None, 0, labels.ctypes.data, None) == INVALID
        assert "radius must be >= 0" in lib.ptk_last_error().decode()
        assert host(tree._h, p.ctypes.data, np.float32(bad), ok.ctypes.data, 0, labels.ctypes.data, None) == 0
    for bad in (np.nan, -1e-3):
        radii = ok.copy()
        radii[4] = radii[7] = bad
        assert host(tree._h, p.ctypes.data, np.float32(1), radii.ctypes.data, 0, labels.ctypes.data, None) == INVALID
        assert "radii[4]" in lib.ptk_last_error().decode()
    # a host-only handle has no device search: PTK_ERR_DEVICE from every device entry point
    assert lib.ptk_cluster_within_self(tree._h, np.float32(0.1), None, 0, labels.ctypes.data, ctypes.byref(n_clusters)) == DEVICE
    assert lib.ptk_cluster_within_self_device(tree._h, np.float32(0.1), None, 0, labels.ctypes.data, None) == DEVICE
    assert lib.ptk_cluster_within_self(None, np.float32(0.1), None, 0, labels.ctypes.data, None) == INVALID
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    assert lib.ptk_search64_cluster_within_self(t64._h, 0.1, None, 0, labels.ctypes.data, None) == DEVICE
    assert lib.ptk_search64_cluster_within_self_device(t64._h, 0.1, None, 0, labels.ctypes.data, None) == DEVICE
    assert lib.ptk_version() == 101
    with pytest.raises(pt.PtkError):
        tree.cluster_within_self(0.1)
    for bad in (np.zeros(8, dtype=np.float32), np.zeros((9, 1), dtype=np.float32), "x"):
        with pytest.raises(ValueError):
            tree.cluster_within_self(bad)
    with pytest.raises(ValueError):
        tree.cluster_within_self(0.1, min_neighbors=-1)


def test_compact_renumbers_by_representative(monkeypatch):
    """compact=True: clusters 0..C-1 in ascending order of their representative index, noise stays -1 (the wrapper's own
    work: the host loop serves a host-only handle here in place of the device form)."""
    p, pile = pile_cloud()
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()

    class Served:  # the device entry point of a host-only handle, answered by the host loop
        def __getattr__(self, name):
            if name == "ptk_cluster_within_self":
                return lambda h, r, rp, mn, labels, ncl: lib.ptk_host_cluster_within_self(h, p.ctypes.data, r, rp, mn,
                                                                                          labels, ncl)
            return getattr(lib, name)

    monkeypatch.setattr(pt, "_load", lambda: Served())
    for r, mn in ((1e-6, 0), (1e-6, 3), (0.0, 0), (0.0, 1), (0.02, 2)):
        plain = tree.cluster_within_self(r, min_neighbors=mn)
        assert plain.dtype == np.int32 and np.array_equal(plain, host_labels(tree, np.float32(r), mn))
        compact = tree.cluster_within_self(r, min_neighbors=mn, compact=True)
        assert compact.dtype == np.int32
        reps = np.unique(plain[plain >= 0])  # ascending representatives
        assert np.array_equal(compact == -1, plain == -1)
        assert np.array_equal(reps[compact[plain >= 0]], plain[plain >= 0])
        assert compact.max(initial=-1) == len(reps) - 1


# ---- CPU tier: the union-find on 16 threads (a stand-alone program under ThreadSanitizer) ------------------------------

def test_union_find_on_sixteen_threads(tmp_path):
    exe = str(tmp_path / "cluster_threads")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread",
                           "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "cluster_threads.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "threads ok", res.stdout + res.stderr


# ---- CPU tier: the C++ members on a host-only build --------------------------------------------------------------------

def test_cpp_members_on_a_host_only_tree(tmp_path):
    d = str(tmp_path)
    p = ds.uniform_cloud(4_000, 3, 91)
    p[::5] = np.round(p[::5] * 4) / 4 * np.float32(0.999)  # a fifth snapped to a grid: coincident points
    p.tofile(os.path.join(d, "points.bin"))
    r, mn = np.float32(0.004), 3
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=pt.PTK_DEVICE_NONE)
    tree_l1 = pt.KdTree(p, pt.Metric.L1, 10, device=pt.PTK_DEVICE_NONE)
    radii = np.full(len(p), r, dtype=np.float32)
    radii[3::50] = 0
    radii[7::90] = np.float32(0.02)
    radii.tofile(os.path.join(d, "radii.bin"))
    exe = os.path.join(d, "cluster_self_main")
    subprocess.check_call(["g++", "-DPICO_TREE_HOST_ONLY", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cluster_self_main.cpp"),
                           "-o", exe])
    res = subprocess.run([exe, d, repr(float(r)), str(mn)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr

    def got(name):
        return np.fromfile(os.path.join(d, name + ".i32"), dtype=np.int32)

    for name, t in (("l2", tree), ("l1", tree_l1)):
        assert np.array_equal(got(name + "_scalar"), expected_labels(*host_search_rows(t, p, r), mn)), name
        assert np.array_equal(got(name + "_radii"), expected_labels(*host_search_rows(t, p, radii), mn)), name
    assert len(np.unique(got("l2_scalar"))) > 10 and np.any(got("l2_scalar") == -1)
    if oracle.have_reference64():
        pd = p.astype(np.float64)
        ref = oracle.Oracle(pd, 10, "reference", dtype=np.float64)
        want = expected_labels(*rs.without_self(*ref.search_radius(pd, np.float64(r))), mn)
        assert np.array_equal(got("l2d_scalar"), want)


# ---- CPU tier: the real kernel source in the emulator ----------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/cpp/emulate_cluster.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_cluster") / "libptk_emu_cluster.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_cluster.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.emu_create.restype = vp
    lib.emu_create.argtypes = [vp, u64, ctypes.c_uint32, vp, u64, vp]
    lib.emu_destroy.argtypes = [vp]
    lib.emu_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu_cluster_self.argtypes = [vp, u64, ctypes.c_float, vp, u64, ctypes.c_int, ctypes.c_int, vp]
    lib.emu64_create.restype = vp
    lib.emu64_create.argtypes = [vp, u64, ctypes.c_uint32, u64]
    lib.emu64_destroy.argtypes = [vp]
    lib.emu64_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu64_cluster_self.argtypes = [vp, u64, ctypes.c_double, vp, u64, ctypes.c_int, ctypes.c_int, vp]
    return lib


def emu_labels(emu, r, mn, piece=0, shortcut=1, compress=1):
    """The passes over an rs.Emulated tree into a poisoned, guarded buffer: every entry written, nothing outside."""
    buf, labels = guarded_labels(emu.n)
    scalar = np.ndim(r) == 0
    assert emu.lib.emu_cluster_self(emu.h, piece, np.float32(r if scalar else 0), None if scalar else r.ctypes.data, mn,
                                    shortcut, compress, labels.ctypes.data) == 0
    assert written(buf, labels), "a label was not written, or one was written outside"
    return labels.copy()


class ByEmulator:
    def __init__(self, lib):
        self.lib = lib
        self.turn = 0

    def tree(self, p, metric, leaf):
        emu = rs.Emulated(self.lib, p, leaf, metric)
        emu._pts, emu._h = emu.host._pts, emu.host._h  # (host_search_rows takes the host tree of the same points)
        return emu

    def labels(self, emu, p, r, mn):
        self.turn += 1  # pieces, the shortcuts and path halving take turns
        return emu_labels(emu, r, mn, piece=(0, 647, 5)[self.turn % 3], shortcut=self.turn % 2, compress=(self.turn // 2) % 2)


@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_kernels_equal_the_expected_labels(emu_lib, kind, metric):
    """Scalar and per-row; 647 leaf positions per launch: pieces that end inside a wavefront and a ragged last one, every
    pass over all of them before the next; the shortcuts of the mark pass on and off; find with and without halving."""
    c = rs.case(kind, metric)
    emu = rs.Emulated(emu_lib, c.p, c.leaf, metric)
    for r in own_radii(c):
        for mn, piece, sc, compress in ((0, 647, 1, 1), (1, 0, 1, 0), (4, 647, 1, 1), (4, 0, 0, 0), (c.n, 647, 1, 1)):
            got = emu_labels(emu, r, mn, piece, sc, compress)
            assert np.array_equal(got, want_scalar(c, r, mn)), (kind, metric, r, mn, piece, sc, compress)
    radii = c.radii()
    for mn, piece, compress in ((0, 647, 0), (4, 647, 1), (4, 0, 0)):
        assert np.array_equal(emu_labels(emu, radii, mn, piece, 1, compress), want_radii(c, mn)), (kind, metric, mn)


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_kernels_where_the_leaf_scan_changes(emu_lib, L):
    """The CPU half of tests/test_leaf_boundaries.py for these kernels: a tree whose largest leaf has exactly 31 | 32 | 33
    and 64 | 65 points; at the radius that holds the whole leaf its points are one cluster."""
    pts, blob, q, nb, ref, radii = leaf_cases.case(L)
    pts = np.asarray(pts)
    emu = rs.Emulated(emu_lib, pts, L, "L2Squared")
    leaf_cases.assert_leaf(emu.host, L)
    for r in leaf_cases.self_radii(L, radii):
        rows = leaf_cases.self_rows(ref, pts, r)
        for mn, piece, sc, compress in ((0, 647, 1, 1), (2, 0, 1, 0), (2, 647, 0, 1)):
            got = emu_labels(emu, r, mn, piece, sc, compress)
            assert np.array_equal(got, expected_labels(*rows, mn)), (L, r, mn, piece)
        if r == radii[1]:
            assert len(np.unique(got[len(pts) - L:])) == 1 and got[-1] >= 0


@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "1d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_emulated_float64_kernels_equal_the_expected_labels(emu_lib, kind, metric):
    c = rs.case(kind, metric, "float64")
    lib = emu_lib
    h = lib.emu64_create(c.p.ctypes.data, c.n, c.p.shape[1], c.leaf)
    assert h
    try:
        lib.emu64_set_metric(h, rs._EMU_METRIC[metric])

        def labels(r, mn, piece, sc, compress):
            buf, out = guarded_labels(c.n)
            scalar = np.ndim(r) == 0
            assert lib.emu64_cluster_self(h, piece, float(r) if scalar else 0.0, None if scalar else r.ctypes.data, mn, sc,
                                          compress, out.ctypes.data) == 0
            assert written(buf, out)
            return out.copy()

        for r in own_radii(c):
            for mn, piece, sc, compress in ((0, 647, 1, 1), (1, 0, 1, 0), (4, 647, 0, 1), (c.n, 0, 1, 0)):
                assert np.array_equal(labels(r, mn, piece, sc, compress), want_scalar(c, r, mn)), (kind, metric, r, mn)
        radii = c.radii()
        for mn, piece in ((0, 0), (4, 647)):
            assert np.array_equal(labels(radii, mn, piece, 1, 1), want_radii(c, mn)), (kind, metric, "per row", mn)
    finally:
        lib.emu64_destroy(h)


def test_emulated_kernels_on_the_constructed_cases(emu_lib):
    check_constructed(ByEmulator(emu_lib))


def foreign_stream(move):
    """(tree points, searched points): a shrunk or shifted copy of the tree's points (tests/test_radius_self.py)."""
    p_tree = ds.uniform_cloud(3_000, 3, 61)
    p = (p_tree * np.float32(0.5) + np.float32(0.25)) if move == "shrunk" else (p_tree + np.float32(0.3))
    return p_tree, np.ascontiguousarray(p, dtype=np.float32)


def asymmetric_pairs(off, flat):
    """Pairs (i, j) with j in row i and i not in row j."""
    n = len(off) - 1
    row, idx = rs.row_ids(off), np.asarray(flat["index"]).astype(np.int64)
    return int(np.setdiff1d(row * n + idx, idx * n + row).size)


@pytest.mark.parametrize("metric", ["L2Squared", "LPInf"])
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_emulated_kernels_on_a_stream_that_does_not_belong_to_its_points(emu_lib, metric, move):
    """The rows of such a stream are asymmetric: the OR of the edge rule matters, and a border point looks at its own
    row only.  Expected: the contract over the host loop's rows of the same tree and points pair; the host loop of the
    feature on that pair as well."""
    p_tree, p = foreign_stream(move)
    emu = rs.Emulated(emu_lib, p, 8, metric, tree_points=p_tree)
    asym = 0
    for r in (0.01, 0.05, 0.3):
        rows = host_search_rows(emu.host, p, np.float32(r))
        asym += asymmetric_pairs(*rows)
        for mn, piece in ((0, 647), (4, 0), (9, 647)):
            want = expected_labels(*rows, mn)
            assert np.array_equal(emu_labels(emu, r, mn, piece), want), (metric, move, r, mn)
            assert np.array_equal(host_labels(emu.host, r, mn, points=p), want), (metric, move, r, mn, "host loop")
    assert asym > 0, "every row is symmetric: the stream tells nothing apart"


def test_emulated_kernels_on_a_stream_with_non_finite_points(emu_lib):
    p_tree, leaf = rs.cloud("uniform")
    p = np.array(p_tree)
    p[700, 1], p[1900, 0] = np.nan, np.inf
    emu = rs.Emulated(emu_lib, p, leaf, "L2Squared", tree_points=p_tree)
    for r in (0.01, 0.1):
        rows = host_search_rows(emu.host, p, np.float32(r))
        for mn, piece in ((0, 0), (4, 647)):
            assert np.array_equal(emu_labels(emu, r, mn, piece), expected_labels(*rows, mn)), (r, mn)


def test_emulated_per_row_radii_that_pass_no_test(emu_lib):
    """A NaN and a negative radii entry (the _device forms cannot look): the row is empty -- its own cluster at
    min_neighbors = 0, non-core otherwise -- and the point is still another point's neighbour."""
    p, leaf = rs.cloud("uniform")
    emu = rs.Emulated(emu_lib, p, leaf, "L2Squared")
    radii = np.full(len(p), 0.01, dtype=np.float32)
    off, flat = host_search_rows(emu.host, p, radii)
    bad = radii.copy()
    bad[100], bad[2000] = np.nan, -1.0
    keep = ~np.isin(rs.row_ids(off), [100, 2000])
    lens = np.diff(off.astype(np.int64))
    assert lens[100] > 0 and lens[2000] > 0
    lens[[100, 2000]] = 0
    off2 = np.zeros(len(off), dtype=np.uint64)
    off2[1:] = np.cumsum(lens)
    for mn in (0, 4):
        got = emu_labels(emu, bad, mn, 647)
        assert np.array_equal(got, expected_labels(off2, flat[keep], mn)), mn
    # (still a neighbour: at min_neighbors = 0 the point is joined through the rows that hold it)
    assert emu_labels(emu, bad, 0)[100] == emu_labels(emu, radii, 0)[100]


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 10, "L2Squared"), (2, 4, "L1")])
def test_emulated_kernels_where_the_stack_class_changes(emu_lib, dim, leaf, metric, depth):
    """Trees of exactly 39 | 40 and 135 | 136 levels (tests/depth_cases.py): the pile of coincident points walks the chain
    of one-point peels in every traversal pass.  The record stacks stay within 2 * depth + 2 and within what the host's
    spill class for the depth holds.  At r = 1e4 every row holds every other point: one cluster, label 0."""
    pts, _ = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    emu = rs.Emulated(emu_lib, pts, leaf, metric)
    run = depth_cases.Watch(depth, emu_lib)
    rows = rs.without_self(*ref.search_radius(pts, np.float32(0.05)))
    n_pile = len(pts) - 3_000
    assert np.all(rs.clamp(rows[0], 0)[3_000:] >= n_pile - 1)
    highs = []
    for mn in (0, 4, n_pile):
        got = run(emu_labels, emu, np.float32(0.05), mn)
        highs.append(run.high)
        assert np.array_equal(got, expected_labels(*rows, mn)), (depth, mn)
    whole = rs.clamp(ref.search_radius(pts[:64], np.float32(1e4))[0], 0)
    assert np.all(whole == len(pts))  # (own entry included)
    for mn in (0, 4):
        assert np.all(run(emu_labels, emu, np.float32(1e4), mn) == 0), (depth, mn)
        highs.append(run.high)
    # (a tree's own points never stand beside the chain the way the corner queries of tests/depth_cases.py do: the
    # stacks hold depth + 3 to depth + 5 records here, not 2 * depth + 2 -- but every pass walks the whole chain)
    assert min(highs) > depth, highs


# ---- gpu tier ---------------------------------------------------------------------------------------------------------

def device_labels(tree, r, mn):
    """Labels through the host-buffer entry point into a guarded 0xA5 buffer."""
    lib = pt._load()
    buf, labels = guarded_labels(tree.npts)
    n_clusters = ctypes.c_uint64(12345)
    scalar = np.ndim(r) == 0
    fn = lib.ptk_search64_cluster_within_self if tree._f64 else lib.ptk_cluster_within_self
    rc = fn(tree._h, tree._real(r if scalar else 0), None if scalar else r.ctypes.data, mn, labels.ctypes.data,
            ctypes.byref(n_clusters))
    assert rc == 0, lib.ptk_last_error()
    assert written(buf, labels), "a label was not written, or one was written outside"
    assert n_clusters.value == int((labels == np.arange(tree.npts)).sum())
    return labels.copy()


class ByDevice:
    def __init__(self, gpu):
        self.gpu = gpu

    def tree(self, p, metric, leaf):
        return pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=self.gpu)

    def labels(self, tree, p, r, mn):
        return device_labels(tree, r, mn)


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_equals_the_expected_labels(gpu, kind, metric, monkeypatch):
    c = rs.case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    for r in own_radii(c):
        for mn in (0, 4):
            assert np.array_equal(device_labels(tree, r, mn), want_scalar(c, r, mn)), (kind, metric, r, mn)
    r = own_radii(c)[2]
    assert np.array_equal(tree.cluster_within_self(r, min_neighbors=4), want_scalar(c, r, 4))
    # pieces of leaf positions that end inside a wavefront: every pass over all of them before the next
    monkeypatch.setenv("PTK_MAX_BATCH", "1000")
    for mn in (0, 4):
        assert np.array_equal(device_labels(tree, r, mn), want_scalar(c, r, mn)), (kind, metric, "pieces", mn)
    monkeypatch.delenv("PTK_MAX_BATCH")
    # find without path halving
    pt.set_test_knobs(cluster_compress=0)
    try:
        assert np.array_equal(device_labels(tree, r, 4), want_scalar(c, r, 4)), (kind, metric, "no halving")
    finally:
        pt.set_test_knobs(cluster_compress=None)


@pytest.mark.gpu
@needs_reference
@needs_reference64
def test_device_per_point_radii_in_both_precisions(gpu):
    for dtype in ("float32", "float64"):
        c = rs.case("uniform", "L2Squared", dtype)
        tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
        radii = c.radii()
        for mn in (0, 4):
            assert np.array_equal(device_labels(tree, radii, mn), want_radii(c, mn)), (dtype, mn)
        assert np.array_equal(tree.cluster_within_self(radii, min_neighbors=4), want_radii(c, 4)), dtype


@pytest.mark.gpu
@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "1d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_float64_trees(gpu, kind, metric):
    import torch

    c = rs.case(kind, metric, "float64")
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    for r in own_radii(c):
        for mn in (0, 4):
            assert np.array_equal(device_labels(tree, r, mn), want_scalar(c, r, mn)), (kind, metric, r, mn)
    r = own_radii(c)[1]
    dev = tree.cluster_within_self(r, min_neighbors=4, device=True)
    assert dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), want_scalar(c, r, 4))


@pytest.mark.gpu
def test_constructed_cases_on_the_device(gpu):
    """Cases (a) to (d), n = 1, 2, 3, and the 4096-chain in shuffled order: one long component, where linking across
    XCDs and long find paths show."""
    check_constructed(ByDevice(gpu))


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 10, "L2Squared"), (2, 4, "L1")])
def test_depths_where_the_stack_class_changes(gpu, dim, leaf, metric, depth):
    pts, _ = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    tree = pt.KdTree(pts, getattr(pt.Metric, metric), leaf, device=gpu)
    depth_cases.assert_depth(tree, depth)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    rows = rs.without_self(*ref.search_radius(pts, np.float32(0.05)))
    for mn in (0, 4, len(pts) - 3_000):
        assert np.array_equal(device_labels(tree, np.float32(0.05), mn), expected_labels(*rows, mn)), (depth, mn)
    for mn in (0, 4):  # (every row holds every other point: one cluster)
        assert np.all(device_labels(tree, np.float32(1e4), mn) == 0), (depth, mn)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["L2Squared", "LPInf"])
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_streams_that_do_not_belong_to_their_points(gpu, tmp_path, metric, move):
    p_tree, p = foreign_stream(move)
    fn = str(tmp_path / "tree.bin")
    pt.save_kd_tree(pt.KdTree(p_tree, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE), fn)
    tree = pt.load_kd_tree(p, fn, device=gpu)
    asym = 0
    for r in (0.01, 0.05, 0.3):
        rows = host_search_rows(tree, p, np.float32(r))
        asym += asymmetric_pairs(*rows)
        for mn in (0, 4, 9):
            assert np.array_equal(device_labels(tree, np.float32(r), mn), expected_labels(*rows, mn)), (metric, move, r, mn)
    assert asym > 0


@pytest.mark.gpu
@needs_reference
def test_two_calls_give_identical_arrays(gpu):
    c = rs.case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    for r in own_radii(c)[1:]:
        for mn in (0, 4):
            first = device_labels(tree, r, mn)
            assert np.array_equal(first, device_labels(tree, r, mn)) and np.array_equal(first, want_scalar(c, r, mn))


@pytest.mark.gpu
@needs_reference
def test_torch_device_form_on_a_side_stream(gpu):
    """The _device entry point on a side stream into a poisoned, guarded tensor; the wrapper's device form, plain and
    compact; a NaN and a negative d_radii entry."""
    import torch

    c = rs.case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    lib = pt._load()
    side = torch.cuda.Stream(device=gpu)
    r = own_radii(c)[2]
    radii = c.radii()
    G = rs.GUARD
    with torch.cuda.stream(side):
        buf = torch.full((c.n + 2 * G,), int(POISON32), dtype=torch.int32, device=f"cuda:{gpu}")
        assert lib.ptk_cluster_within_self_device(tree._h, np.float32(r), None, 4, buf[G:].data_ptr(), side.cuda_stream) == 0
        plain = tree.cluster_within_self(r, min_neighbors=4, device=True)
        compact = tree.cluster_within_self(r, min_neighbors=4, compact=True, device=True)
        d_radii = torch.from_numpy(radii).to(f"cuda:{gpu}")
        per_row = tree.cluster_within_self(d_radii, min_neighbors=4, device=True)
        bad = radii.copy()
        bad[100], bad[2000] = np.nan, -1.0
        d_bad = torch.from_numpy(bad).to(f"cuda:{gpu}")
        per_row_bad = [tree.cluster_within_self(d_bad, min_neighbors=mn, device=True) for mn in (0, 4)]
    side.synchronize()
    raw = buf.cpu().numpy()
    want = want_scalar(c, r, 4)
    assert np.all(raw[:G] == POISON32) and np.all(raw[-G:] == POISON32) and np.array_equal(raw[G:-G], want)
    assert plain.dtype == torch.int32 and np.array_equal(plain.cpu().numpy(), want)
    reps = np.unique(want[want >= 0])
    got = compact.cpu().numpy()
    assert compact.dtype == torch.int32 and np.array_equal(got == -1, want == -1)
    assert np.array_equal(reps[got[want >= 0]], want[want >= 0]) and got.max() == len(reps) - 1
    assert np.array_equal(per_row.cpu().numpy(), want_radii(c, 4))
    off, flat = c.want_per_row()
    lens = np.diff(off.astype(np.int64))
    assert lens[100] > 0 and lens[2000] > 0
    keep = ~np.isin(rs.row_ids(off), [100, 2000])
    lens[[100, 2000]] = 0
    off2 = np.zeros(len(off), dtype=np.uint64)
    off2[1:] = np.cumsum(lens)
    for mn, got in zip((0, 4), per_row_bad):
        assert np.array_equal(got.cpu().numpy(), expected_labels(off2, flat[keep], mn)), mn
    for wrong in (d_bad[:5], d_bad.double(), d_bad.reshape(-1, 1)):
        with pytest.raises(ValueError):
            tree.cluster_within_self(wrong, device=True)


def _refused(tree, points, reason, want):
    with pytest.raises(pt.PtkError) as refused:
        tree.cluster_within_self(0.01, min_neighbors=3)
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
    assert reason in str(refused.value) and "ptk_host_cluster_within_self" in str(refused.value), str(refused.value)
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got = tree.cluster_within_self(0.01, min_neighbors=3)
    finally:
        pt.allow_host_loop(False)
    assert np.array_equal(got, want), reason


@pytest.mark.gpu
@needs_reference
def test_refused_handles_and_the_host_loop_that_serves_them(gpu):
    c5 = rs.case("5d", "L2Squared")
    _refused(pt.KdTree(c5.p, pt.Metric.L2Squared, c5.leaf, device=gpu), c5.p, "dim > 3",
             expected_labels(*c5.want(np.float32(0.01)), 3))
    rng = np.random.default_rng(12)
    pt3 = rng.random((2_000, 3), dtype=np.float32)
    ref = oracle.Oracle(pt3, 8, "reference", metric="SE2Squared")
    _refused(pt.KdTree(pt3, pt.Metric.SE2Squared, 8, device=gpu), pt3, "topological",
             expected_labels(*rs.without_self(*ref.search_radius(pt3, np.float32(0.01))), 3))
    deep, _ = depth_cases.cloud_at_depth(1032, 3, 10)
    deep = np.asarray(deep)
    tree = pt.KdTree(deep, pt.Metric.L2Squared, 10, device=gpu)
    _refused(tree, deep, "tree depth 1032", expected_labels(*host_search_rows(tree, deep, np.float32(0.01)), 3))
    # the argument checks of the device entry points
    lib = pt._load()
    small = pt.KdTree(rs.cloud("small")[0], pt.Metric.L2Squared, 5, device=gpu)
    labels = np.zeros(small.npts, dtype=np.int32)
    bad = np.full(small.npts, 0.1, dtype=np.float32)
    bad[7] = bad[9] = np.nan
    assert lib.ptk_cluster_within_self(small._h, np.float32(0.1), None, 0, None, None) == -1
    assert lib.ptk_cluster_within_self(small._h, np.float32(np.nan), None, 0, labels.ctypes.data, None) == -1
    assert lib.ptk_cluster_within_self(small._h, np.float32(-1), None, 0, labels.ctypes.data, None) == -1
    assert lib.ptk_cluster_within_self(small._h, np.float32(1), bad.ctypes.data, 0, labels.ctypes.data, None) == -1
    assert "radii[7]" in lib.ptk_last_error().decode()
    assert lib.ptk_cluster_within_self_device(small._h, np.float32(0.1), None, 0, None, None) == -1
    with pytest.raises(ValueError):
        small.cluster_within_self(bad, device=True)


@pytest.mark.gpu
def test_the_radius_capture_and_the_self_searches_are_left_alone(gpu):
    """A scalar search_radius count / fill pair with a cluster call between its halves still returns its rows;
    count_within_self and search_radius_self of the same handle are what they were before."""
    import torch

    p, q = ds.uniform_cloud(20_000, 3, 71), ds.uniform_cloud(6_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)

    def others():
        return [tree.count_within_self(0.001).tobytes(), tree.count_within_self(0.001, max_count=3).tobytes(),
                tree.search_radius_self(0.001).flat.tobytes(), tree.search_knn(q, 1).tobytes()]

    before = others()
    lib = pt._load()
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    stream = torch.cuda.current_stream(dq.device).cuda_stream
    want = tree.search_radius(q, 0.002)
    counts = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                              counts.data_ptr(), stream) == 0
    labels = tree.cluster_within_self(0.001, min_neighbors=3, device=True)
    labels_host = tree.cluster_within_self(np.full(len(p), 0.001, dtype=np.float32), min_neighbors=3)
    offsets = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    offsets[1:] = torch.cumsum(counts[:len(q)], 0)
    out = torch.empty((max(int(offsets[-1].item()), 1), 2), dtype=torch.int32, device=dq.device)
    assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                             offsets.data_ptr(), out.data_ptr(), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want.offsets)
    assert rs.raw_rows(out)[:len(want.flat)].tobytes() == want.flat.tobytes()
    rows = tree.search_radius_self(0.001)
    assert np.array_equal(labels.cpu().numpy(), expected_labels(rows.offsets, rows.flat, 3))
    assert np.array_equal(labels_host, labels.cpu().numpy())
    assert others() == before
