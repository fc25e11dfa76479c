"""search_knn_within / count_within with one radius per query row (ptk.h: the _radii entry points).

Row i / counts[i] of a per-row call is row i / counts[i] of the scalar call with radius = radii[i].  Expected values
always come from the compiled reference: its search_knn row of min(k, n) entries filtered with the strict
``distance < r_i`` and padded with (index -1, distance r_i); the lengths of its search_radius rows, run once per distinct
radius on the rows that carry it.

The radii of a batch (``mixed_radii``) put rows with no hit, some hits and k hits side by side in one wavefront: the five
values of tests/test_knn_within.py's radii() cycled over the rows (a period of 5, no multiple of 64), every seventh row
its OWN reference distance of slot min(k, n) // 2 (the strict `<` at a bound that differs per row), every eleventh +inf.

The CPU tier checks the two host loops on a host-only handle, the argument checks, the real source of the per-row
kernels in the emulator (tests/cpp/emulate_within_radii.cpp) -- with a launch order that is not the identity --, the C++
members (tests/cpp/within_radii_main.cpp) and the Python validation; the gpu tier checks the device searches.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)
INF = float("inf")
KS = (1, 4, 16, 40, 64, 80)
METRICS = ("L2Squared", "L1", "LPInf", "LNInf")

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")
needs_reference64 = pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")


def cloud(kind):
    """(points, queries, leaf size): the clouds of tests/test_knn_within.py."""
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


class Case:
    """A cloud with its reference tree; the reference's k-NN rows are computed once per k and shared."""

    def __init__(self, p, q, leaf, metric, dtype=np.float32):
        self.p, self.q, self.leaf, self.metric, self.dtype = p, np.ascontiguousarray(q), leaf, metric, np.dtype(dtype)
        self.ref = oracle.Oracle(p, leaf, "reference", metric=metric, dtype=dtype)
        self._knn = {}

    def knn(self, k):
        kk = min(k, self.ref.n)
        if kk not in self._knn:
            rows = self.ref.search_knn(self.q, kk)
            rows.setflags(write=False)
            self._knn[kk] = rows
        return self._knn[kk]

    def five(self):
        """radii() of tests/test_knn_within.py: 0, half the smallest nearest distance, the medians of the first and of
        the 16th distance, and the largest finite number."""
        d = self.knn(16)["distance"]
        return [0.0, float(d[:, 0].min()) * 0.5, float(np.median(d[:, 0])), float(np.median(d[:, -1])),
                float(np.finfo(self.dtype).max)]

    def mixed_radii(self, k):
        """The radii recipe of the module docstring for a search of k."""
        n = len(self.q)
        i = np.arange(n)
        r = np.array(self.five(), dtype=self.dtype)[i % 5]
        kk = min(k, self.ref.n)
        own = self.knn(k)["distance"].reshape(n, kk)[:, kk // 2]
        r[i % 7 == 3] = own[i % 7 == 3]
        r[i % 11 == 5] = INF
        return r

    def rows(self, k, r):
        """The filtered reference rows for the per-row radii r."""
        kk = min(k, self.ref.n)
        rows = self.knn(k).reshape(len(self.q), kk)
        out = np.zeros((len(self.q), k), dtype=rows.dtype)
        out["index"] = -1
        out["distance"] = r[:, None]
        keep = rows["distance"] < r[:, None]  # (a prefix of every row: the rows are ascending)
        out[:, :kk][keep] = rows[keep]
        return out

    def counts(self, r, max_count=0):
        """The lengths of the reference's search_radius rows, one run per distinct radius on the rows that carry it."""
        c = np.zeros(len(self.q), dtype=np.int64)
        for v in np.unique(r):
            at = np.flatnonzero(r == v)
            off, _ = self.ref.search_radius(np.ascontiguousarray(self.q[at]), v)
            c[at] = np.diff(np.asarray(off)).astype(np.int64)
        return np.minimum(c, max_count) if max_count else c


_cases = {}


def case(kind, metric, dtype=np.float32):
    key = (kind, metric, np.dtype(dtype).name)
    if key not in _cases:
        p, q, leaf = cloud(kind)
        if np.dtype(dtype) == np.float64:
            p, q = p.astype(np.float64) * 1.0000001, q.astype(np.float64) * 1.0000001
        _cases[key] = Case(p, q, leaf, metric, dtype)
    return _cases[key]


def same_rows(got, want):
    """Index and distance bits equal (float64 records carry padding bytes)."""
    got = got.reshape(want.shape)
    return np.array_equal(got["index"], want["index"]) and \
        np.ascontiguousarray(got["distance"]).tobytes() == np.ascontiguousarray(want["distance"]).tobytes()


def host_knn(tree, q, k, r):
    out = np.empty((len(q), k), dtype=pt.NEIGHBOR)
    lib = pt._load()
    rc = lib.ptk_host_search_knn_within_radii(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), k, r.ctypes.data,
                                              out.ctypes.data)
    assert rc == 0, lib.ptk_last_error()
    return out


def host_counts(tree, q, r, max_count=0):
    out = np.full(len(q), -7, dtype=np.int64)
    lib = pt._load()
    rc = lib.ptk_host_search_count_within_radii(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), r.ctypes.data,
                                                max_count, out.ctypes.data)
    assert rc == 0, lib.ptk_last_error()
    return out


# ---- CPU tier: the host loops on a host-only handle ---------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "self", "2d", "5d"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loops_equal_the_filtered_reference(kind, metric):
    c = case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    for k in KS:
        r = c.mixed_radii(k)
        assert host_knn(tree, c.q, k, r).tobytes() == c.rows(k, r).tobytes(), (kind, metric, k)
    r = c.mixed_radii(16)
    want = c.counts(r)
    for mc in (0, 1, 5):
        assert np.array_equal(host_counts(tree, c.q, r, mc), np.minimum(want, mc) if mc else want), (kind, metric, mc)


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loops_of_the_topological_metrics(metric):
    rng = np.random.default_rng(12)
    dim = 1 if metric == "SO2" else 3
    p, q = rng.random((2_000, dim), dtype=np.float32), rng.random((400, dim), dtype=np.float32)
    c = Case(p, q, 8, metric)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    for k in KS:
        r = c.mixed_radii(k)
        assert host_knn(tree, c.q, k, r).tobytes() == c.rows(k, r).tobytes(), (metric, k)
    r = c.mixed_radii(16)
    want = c.counts(r)
    for mc in (0, 1, 5):
        assert np.array_equal(host_counts(tree, c.q, r, mc), np.minimum(want, mc) if mc else want), (metric, mc)


def test_argument_checks_of_the_host_loops_and_host_forms():
    p, q = ds.uniform_cloud(50, 3, 21), ds.uniform_cloud(40, 3, 22)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    h, pp, qq, n = tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q)
    rows = np.empty((n, 4), dtype=pt.NEIGHBOR)
    counts = np.empty(n, dtype=np.int64)
    good = np.full(n, 0.01, dtype=np.float32)
    # null radii, k = 0, null outputs
    assert lib.ptk_host_search_knn_within_radii(h, pp, qq, n, 4, None, rows.ctypes.data) == -1
    assert lib.ptk_host_search_count_within_radii(h, pp, qq, n, None, 0, counts.ctypes.data) == -1
    assert lib.ptk_host_search_knn_within_radii(h, pp, qq, n, 0, good.ctypes.data, rows.ctypes.data) == -1
    assert lib.ptk_host_search_knn_within_radii(h, pp, qq, n, 4, good.ctypes.data, None) == -1
    assert lib.ptk_host_search_count_within_radii(h, pp, qq, n, good.ctypes.data, 0, None) == -1
    # a NaN and a negative entry: refused, and the first offending row is named
    for bad, row in ((float("nan"), 17), (-1.0, 5)):
        r = good.copy()
        r[row] = bad
        r[row + 9] = bad
        assert lib.ptk_host_search_knn_within_radii(h, pp, qq, n, 4, r.ctypes.data, rows.ctypes.data) == -1
        assert f"radii[{row}]" in lib.ptk_last_error().decode()
        assert lib.ptk_host_search_count_within_radii(h, pp, qq, n, r.ctypes.data, 0, counts.ctypes.data) == -1
        assert f"radii[{row}]" in lib.ptk_last_error().decode()
    # +inf, FLT_MAX, 0 and a subnormal radius are valid entries
    r = good.copy()
    r[:4] = [INF, FLT_MAX, 0.0, 1e-42]
    assert lib.ptk_host_search_knn_within_radii(h, pp, qq, n, 4, r.ctypes.data, rows.ctypes.data) == 0
    assert lib.ptk_host_search_count_within_radii(h, pp, qq, n, r.ctypes.data, 0, counts.ctypes.data) == 0
    assert counts[0] == 50 and counts[1] == 50 and counts[2] == 0
    # an empty batch with null buffers
    assert lib.ptk_host_search_knn_within_radii(h, pp, None, 0, 4, None, None) == 0
    assert lib.ptk_host_search_count_within_radii(h, pp, None, 0, None, 0, None) == 0
    # the host forms: a null tree and null radii are invalid, a host-only handle has no device search
    assert lib.ptk_search_knn_within_radii(None, qq, n, 4, good.ctypes.data, rows.ctypes.data) == -1
    assert lib.ptk_search_count_within_radii(None, qq, n, good.ctypes.data, 0, counts.ctypes.data) == -1
    assert lib.ptk_search_knn_within_radii(h, qq, n, 4, good.ctypes.data, rows.ctypes.data) < 0
    assert lib.ptk_search_count_within_radii(h, qq, n, good.ctypes.data, 0, counts.ctypes.data) < 0
    p64 = p.astype(np.float64)
    t64 = pt.KdTree(p64, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    q64, good64 = q.astype(np.float64), good.astype(np.float64)
    rows64 = np.empty((n, 4), dtype=pt.NEIGHBOR64)
    assert lib.ptk_search64_knn_within_radii(t64._h, q64.ctypes.data, n, 4, good64.ctypes.data, rows64.ctypes.data) < 0
    assert lib.ptk_search64_count_within_radii(t64._h, q64.ctypes.data, n, good64.ctypes.data, 0, counts.ctypes.data) < 0
    assert lib.ptk_search64_knn_within_radii(None, q64.ctypes.data, n, 4, good64.ctypes.data, rows64.ctypes.data) == -1


# ---- CPU tier: the real kernel source of the per-row kernels in the emulator ----------------------------------------

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/cpp/emulate_within_radii.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_within_radii") / "libptk_emu_within_radii.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_within_radii.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    lib.emu_set_metric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.emu_knn_within_radii.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.emu_count_within_radii.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p]
    return lib


_EMU_METRIC = {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}


class EmuTree:
    def __init__(self, lib, p, leaf, metric):
        host = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
        nodes, idx, _, _ = host.flat()
        self.lib = lib
        self.h = lib.emu_create(p.ctypes.data, len(p), p.shape[1], nodes.ctypes.data, len(nodes), idx.ctypes.data)
        assert self.h
        lib.emu_set_metric(self.h, _EMU_METRIC[metric])

    def close(self):
        self.lib.emu_destroy(self.h)

    def knn(self, q, perm, k, r, form):
        out = np.empty((len(q), k), dtype=pt.NEIGHBOR)
        assert self.lib.emu_knn_within_radii(self.h, q.ctypes.data, None if perm is None else perm.ctypes.data, len(q), k,
                                             r.ctypes.data, form, out.ctypes.data) == 0
        return out

    def counts(self, q, perm, r, max_count=0, shortcut=1):
        out = np.full(len(q), -7, dtype=np.int64)
        stats = np.zeros(3, dtype=np.uint32)
        assert self.lib.emu_count_within_radii(self.h, q.ctypes.data, None if perm is None else perm.ctypes.data, len(q),
                                               r.ctypes.data, max_count, shortcut, out.ctypes.data, stats.ctypes.data) == 0
        return out, stats


def shuffle(n):
    """A fixed launch order that is not the identity: entry i of the launch is row perm[i]."""
    return np.random.default_rng(77).permutation(n).astype(np.uint32)


def lattice():
    """The lattice of tests/test_knn_within.py: point distances and box distances hit the integer radii exactly."""
    g = np.arange(0, 12, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g[:6], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = np.concatenate([p[::29], p[::31] + np.float32(0.5), p[::37] * np.float32([1, 1, 0])]).astype(np.float32)
    return p, q


def emu_case(kind, metric):
    """(case, radii per k): the lattice with integer radii mixed per row, the other clouds with the recipe."""
    if kind == "lattice":
        key = ("lattice", metric, "float32")
        if key not in _cases:
            p, q = lattice()
            _cases[key] = Case(p, q, 4, metric)
        c = _cases[key]
        r = np.array([0.0, 1.0, 2.0, 3.0, 0.75, 4.0, INF], dtype=np.float32)[(np.arange(len(c.q)) * 3) % 7]
        return c, (lambda k: r)
    c = case(kind, metric)
    if len(c.q) > 200:
        key = (kind + ":200", metric, "float32")
        if key not in _cases:
            _cases[key] = Case(c.p, c.q[:200], c.leaf, metric)
        c = _cases[key]
    return c, c.mixed_radii


@needs_reference
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties", "5d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf"])
def test_emulated_per_row_kernels_equal_the_filtered_reference(emu, kind, metric):
    c, radii_of = emu_case(kind, metric)
    t = EmuTree(emu, c.p, c.leaf, metric)
    perm = shuffle(len(c.q))
    try:
        for k in KS:  # (4, 16, 64: the register lists compiled for the emulator; 1 and 40 share them; 80: the lists)
            r = radii_of(k)
            want = c.rows(k, r).tobytes()
            for form in ((0, 1, 2) if k <= 64 else (1, 2)):
                assert t.knn(c.q, None, k, r, form).tobytes() == want, (kind, metric, k, form)
                # a kernel that indexes `radii` by launch position fails here
                assert t.knn(c.q, perm, k, r, form).tobytes() == want, (kind, metric, k, form, "perm")
    finally:
        t.close()


@needs_reference
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_per_row_count_kernel_equals_the_reference(emu, kind, metric):
    c, radii_of = emu_case(kind, metric)
    r = radii_of(16)
    want = c.counts(r)
    t = EmuTree(emu, c.p, c.leaf, metric)
    perm = shuffle(len(c.q))
    try:
        for pm in (None, perm):
            for mc in (0, 5):
                got, stats = t.counts(c.q, pm, r, mc)
                assert np.array_equal(got, np.minimum(want, mc) if mc else want), (kind, metric, mc, pm is not None)
                if mc == 0:  # the mixed batch takes both shortcuts: the inside one at the large radii, the outside one at 0
                    assert stats[0] > 0 and stats[1] > 0, stats
            got, stats = t.counts(c.q, pm, r, 0, shortcut=0)
            assert np.array_equal(got, want), (kind, metric, "no shortcut")
            assert not stats.any()
    finally:
        t.close()


@needs_reference
def test_emulated_count_kernel_rows_with_a_subnormal_radius_take_neither_shortcut(emu):
    """Points a subnormal distance apart; the rows alternate between subnormal radii and radii far beyond the cloud.  The
    shortcut counters are per batch, so the batch is also run as its two halves: the rows with a subnormal radius take
    neither the inside shortcut (refused for the radius: counter 2) nor -- every box reaching them -- the outside one;
    the rows with a large radius take the inside one; and the mixed batch reports the sum of the two."""
    p = np.zeros((200, 3), dtype=np.float32)
    p[:, 0] = np.arange(200, dtype=np.float32) * np.float32(1e-45)
    q = np.ascontiguousarray(p[::3])
    n = len(q)
    sub = np.array([1e-40, 3e-39, 1e-38 * 0.5], dtype=np.float32)  # (the three are subnormal, and beyond the cloud)
    r = np.where(np.arange(n) % 2 == 0, sub[np.arange(n) % 3], np.float32(1.0)).astype(np.float32)
    c = Case(p, q, 4, "L2Squared")
    want = c.counts(r)
    assert np.all(want == 200)
    t = EmuTree(emu, p, 4, "L2Squared")
    try:
        got, mixed = t.counts(q, shuffle(n), r)
        assert np.array_equal(got, want)
        even, odd = np.ascontiguousarray(q[0::2]), np.ascontiguousarray(q[1::2])
        got_sub, s_sub = t.counts(even, None, np.ascontiguousarray(r[0::2]))
        got_big, s_big = t.counts(odd, None, np.ascontiguousarray(r[1::2]))
        assert np.all(got_sub == 200) and np.all(got_big == 200)
        assert s_sub[0] == 0 and s_sub[1] == 0 and s_sub[2] > 0, s_sub
        assert s_big[0] > 0 and s_big[2] == 0, s_big
        assert np.array_equal(mixed, s_sub + s_big), (mixed, s_sub, s_big)
    finally:
        t.close()


# ---- CPU tier: the C++ members (tests/cpp/within_radii_main.cpp) ---------------------------------------------------

def test_cpp_batched_radii_members_equal_the_single_query_members(tmp_path):
    d = str(tmp_path)
    p, q = ds.uniform_cloud(20_000, 3, 91), ds.uniform_cloud(1_500, 3, 92)
    q[:40] = p[:40]  # queries exactly on tree points
    i = np.arange(len(q))
    r = np.array([0.0, 0.0004, 0.002, 1e-42, FLT_MAX], dtype=np.float32)[i % 5]
    r[i % 11 == 5] = INF
    p.tofile(os.path.join(d, "points.bin"))
    q.tofile(os.path.join(d, "queries.bin"))
    r.tofile(os.path.join(d, "radii.bin"))
    exe = os.path.join(d, "within_radii_main")
    subprocess.check_call(["g++", "-DPICO_TREE_HOST_ONLY", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "within_radii_main.cpp"),
                           "-o", exe])
    for k in (1, 9, 70):
        res = subprocess.run([exe, d, str(k)], capture_output=True, text=True)
        assert res.returncode == 0 and res.stdout.strip() == "ok", (k, res.stdout + res.stderr)


# ---- CPU tier: the Python wrapper's validation ------------------------------------------------------------------------

def test_python_validation_on_a_host_only_handle():
    p, q = ds.uniform_cloud(100, 3, 23), ds.uniform_cloud(30, 3, 24)
    for dtype in (np.float32, np.float64):
        tree = pt.KdTree(p.astype(dtype), pt.Metric.L2Squared, 5, device=pt.PTK_DEVICE_NONE)
        qq = q.astype(dtype)
        for bad in (np.zeros(29), np.zeros(31), np.zeros((30, 1)), np.zeros((2, 15)), ["a"] * 30):
            with pytest.raises(ValueError):
                tree.search_knn_within(qq, 4, bad)
            with pytest.raises(ValueError):
                tree.count_within(qq, bad)
        # a well-formed array passes the validation and reaches the library, which has no device here
        with pytest.raises(pt.PtkError):
            tree.search_knn_within(qq, 4, [0.01] * 30)
        with pytest.raises(pt.PtkError):
            tree.count_within(qq, np.full(30, 0.01, dtype=np.float64))


# ---- gpu tier ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "self", "2d", "5d"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_rows_and_counts_equal_the_filtered_reference(gpu, kind, metric):
    import torch

    c = case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    dq = torch.from_numpy(c.q).to(f"cuda:{gpu}")
    for k in KS:
        r = c.mixed_radii(k)
        want = c.rows(k, r).tobytes()
        assert tree.search_knn_within(c.q, k, r).reshape(len(c.q), k).tobytes() == want, (kind, metric, k)
        dev = tree.search_knn_within(dq, k, torch.from_numpy(r).to(dq.device)).numpy()
        assert dev.reshape(len(c.q), k).tobytes() == want, (kind, metric, k, "torch")
    r = c.mixed_radii(16)
    want = c.counts(r)
    if kind == "5d":  # the device serves the per-row count for dim <= 3 only (ptk.h)
        with pytest.raises(pt.PtkError) as refused:
            tree.count_within(c.q, r)
        assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
        return
    dr = torch.from_numpy(r).to(dq.device)
    for mc in (0, 5):
        w = np.minimum(want, mc) if mc else want
        assert np.array_equal(tree.count_within(c.q, r, mc), w), (kind, metric, mc)
        assert np.array_equal(tree.count_within(dq, dr, mc).cpu().numpy(), w), (kind, metric, mc, "torch")


@pytest.mark.gpu
@needs_reference64
@pytest.mark.parametrize("dim", [3, 6])
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_float64_device_rows_and_counts_equal_the_filtered_reference(gpu, dim, metric):
    import torch

    p = ds.uniform_cloud(4_000, dim, 101).astype(np.float64) * 1.0000001
    q = ds.uniform_cloud(600, dim, 102).astype(np.float64) * 1.0000001
    c = Case(p, q, 10, metric, np.float64)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 10, device=gpu)
    dq = torch.from_numpy(c.q).to(f"cuda:{gpu}")
    for k in KS:
        r = c.mixed_radii(k)
        want = c.rows(k, r)
        assert same_rows(tree.search_knn_within(c.q, k, r), want), (dim, metric, k)
        assert same_rows(tree.search_knn_within(dq, k, torch.from_numpy(r).to(dq.device)).numpy(), want), (dim, metric, k)
    r = c.mixed_radii(16)
    if dim > 3:
        with pytest.raises(pt.PtkError) as refused:
            tree.count_within(c.q, r)
        assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
        return
    want = c.counts(r)
    dr = torch.from_numpy(r).to(dq.device)
    for mc in (0, 5):
        w = np.minimum(want, mc) if mc else want
        assert np.array_equal(tree.count_within(c.q, r, mc), w), (dim, metric, mc)
        assert np.array_equal(tree.count_within(dq, dr, mc).cpu().numpy(), w), (dim, metric, mc, "torch")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_constant_radii_array_gives_the_bytes_of_the_scalar_call(gpu, dtype):
    p, q = ds.uniform_cloud(6_000, 3, 41).astype(dtype), ds.uniform_cloud(3_000, 3, 42).astype(dtype)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    d1 = tree.search_knn(q, 1)["distance"]
    for r in (0.0, float(np.median(d1)), float(np.finfo(dtype).max), INF):
        const = np.full(len(q), r, dtype=dtype)
        for k in KS:
            assert same_rows(tree.search_knn_within(q, k, const), tree.search_knn_within(q, k, r)), (dtype, k, r)
        for mc in (0, 16):
            assert np.array_equal(tree.count_within(q, const, mc), tree.count_within(q, r, mc)), (dtype, mc, r)


def hashed_radii(n, values):
    """A pseudo-random function of the row index into a few values (so that the reference runs once per value)."""
    i = np.arange(n, dtype=np.uint64)
    return np.asarray(values, dtype=np.float32)[((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(len(values))]


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dim", [3, 5])
def test_batch_order_and_pieces_do_not_change_a_row(gpu, dim, monkeypatch):
    p, q = ds.uniform_cloud(20_000, dim, 31), ds.uniform_cloud(12_000, dim, 32)  # (12 000 > 8 192: REORDER_AUTO sorts)
    c = Case(p, q, 10, "L2Squared")
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    d = c.knn(16)["distance"]
    values = [0.0, float(np.median(d[:, 0])), float(np.median(d[:, 3])), float(np.median(d[:, 15])),
              float(d[:, 15].max()) * 2, FLT_MAX, INF, float(d[:, 0].min()) * 0.5]
    r = hashed_radii(len(q), values)
    ks = (1, 4, 16, 70)
    want = {k: c.rows(k, r).tobytes() for k in ks}
    for mode in (pt.REORDER_ON, pt.REORDER_OFF):
        tree.set_reorder(mode)
        for k in ks:
            assert tree.search_knn_within(c.q, k, r).reshape(len(q), k).tobytes() == want[k], (dim, mode, k)
    tree.set_reorder(pt.REORDER_AUTO)
    monkeypatch.setenv("PTK_MAX_BATCH", "3001")
    for k in ks:
        assert tree.search_knn_within(c.q, k, r).reshape(len(q), k).tobytes() == want[k], (dim, "pieces", k)
    monkeypatch.delenv("PTK_MAX_BATCH")
    if dim == 3:
        rc = hashed_radii(len(q), values[:5])  # (the finite values: the rows of the reference stay small)
        wc = c.counts(rc)
        for mode in (pt.REORDER_ON, pt.REORDER_OFF):
            tree.set_reorder(mode)
            assert np.array_equal(tree.count_within(c.q, rc), wc), mode


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("nq", [64 * 5, 64 * 5 + 17])
def test_full_and_partial_wavefronts_of_the_register_list(gpu, nq):
    """k = 4 and k = 16 with k == K: a full wavefront leaves through the LDS row write-out of
    knn_reg_within_radii_kernel, the last 17 rows of the other batch through the plain store."""
    import torch

    p = ds.uniform_cloud(5_000, 3, 33)
    c = Case(p, ds.uniform_cloud(nq, 3, 34), 10, "L2Squared")
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    dq = torch.from_numpy(c.q).to(f"cuda:{gpu}")
    for k in (4, 16):
        r = c.mixed_radii(k)
        want = c.rows(k, r).tobytes()
        assert tree.search_knn_within(c.q, k, r).tobytes() == want, (nq, k)
        # (an output that is 8 but not 16 bytes aligned takes the write-out's other branch)
        raw = torch.empty((nq * k + 1, 2), dtype=torch.int32, device=dq.device)
        out = raw[1:].view(nq, k, 2)
        got = tree.search_knn_within(dq, k, torch.from_numpy(r).to(dq.device), out).numpy()
        assert got.tobytes() == want, (nq, k, "unaligned")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "ties", "self"])
def test_warm_start_gives_the_nearest_neighbour_or_nothing(gpu, kind):
    p, q, leaf = cloud(kind)
    tree = pt.KdTree(p, pt.Metric.L2Squared, leaf, device=gpu)
    nn = tree.search_knn(q, 1)
    d1 = np.ascontiguousarray(nn["distance"])
    if kind == "self":
        assert np.all(d1 == 0)
    above = np.nextafter(d1, np.float32(INF))
    assert tree.search_knn_within(q, 1, above).tobytes() == nn.tobytes()
    at = tree.search_knn_within(q, 1, d1)
    assert np.all(at["index"] == -1) and at["distance"].tobytes() == d1.tobytes()


@pytest.mark.gpu
@needs_reference
def test_deep_tree(gpu, monkeypatch):
    pts = np.concatenate([ds.uniform_cloud(60_000, 3, 31) - np.float32(0.5), np.zeros((1_500, 3), np.float32)])
    q = np.concatenate([ds.uniform_cloud(400, 3, 32) - np.float32(0.5), np.zeros((3, 3), np.float32)])
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    assert tree.info()["max_depth"] > 1_040
    c = Case(pts, q, 10, "L2Squared")
    monkeypatch.setenv("PTK_DEEP_SPILL_MB", "16")
    for k in (1, 5, 40, 80):
        r = c.mixed_radii(k)
        assert tree.search_knn_within(c.q, k, r).reshape(len(q), k).tobytes() == c.rows(k, r).tobytes(), k
    monkeypatch.delenv("PTK_DEEP_SPILL_MB")
    r = c.mixed_radii(16)
    _refused_then_served(tree, c, r)


def _refused_then_served(tree, c, r):
    """count_within per row: refused by the device with PTK_ERR_UNSUPPORTED, served by the host loop when allowed."""
    with pytest.raises(pt.PtkError) as refused:
        tree.count_within(c.q, r)
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED == -2
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got = tree.count_within(c.q, r)
            got5 = tree.count_within(c.q, r, 5)
    finally:
        pt.allow_host_loop(False)
    want = c.counts(r)
    assert np.array_equal(got, want) and np.array_equal(got5, np.minimum(want, 5))


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["5d", "se2"])
def test_count_of_the_handles_the_device_refuses(gpu, kind):
    if kind == "5d":
        c = case("5d", "L2Squared")
        metric = pt.Metric.L2Squared
    else:
        rng = np.random.default_rng(3)
        c = Case(rng.random((2_000, 3), dtype=np.float32), rng.random((400, 3), dtype=np.float32), 8, "SE2Squared")
        metric = pt.Metric.SE2Squared
    tree = pt.KdTree(c.p, metric, c.leaf, device=gpu)
    _refused_then_served(tree, c, c.mixed_radii(16))
    if kind == "se2":  # the bounded k-NN of a topological tree: refused as the scalar form, served by the host loop
        r = c.mixed_radii(4)
        with pytest.raises(pt.PtkError) as refused:
            tree.search_knn_within(c.q, 4, r)
        assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
        pt.allow_host_loop(True)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = tree.search_knn_within(c.q, 4, r)
        finally:
            pt.allow_host_loop(False)
        assert got.tobytes() == c.rows(4, r).tobytes()


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_form_with_a_nan_and_a_negative_radius(gpu, dtype):
    import torch

    if dtype == np.float64 and not oracle.have_reference64():
        pytest.skip("compiled double reference not present")
    p = ds.uniform_cloud(3_000, 3, 1).astype(dtype)
    q = ds.uniform_cloud(200, 3, 2).astype(dtype)
    c = Case(p, q, 10, "L2Squared", dtype)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    dq = torch.from_numpy(c.q).to(f"cuda:{gpu}")
    bits = np.uint32 if dtype == np.float32 else np.uint64
    for k in (1, 4, 16, 80):
        r = c.mixed_radii(k)
        good = r.copy()
        r[37], r[101] = np.nan, -1.0
        got = tree.search_knn_within(dq, k, torch.from_numpy(r).to(dq.device)).numpy().reshape(len(q), k)  # (PTK_OK)
        for row in (37, 101):
            assert np.all(got["index"][row] == -1)
            assert np.all(np.ascontiguousarray(got["distance"][row]).view(bits) == r[row:row + 1].view(bits)[0])
        want = c.rows(k, good)
        others = np.ones(len(q), dtype=bool)
        others[[37, 101]] = False
        assert same_rows(np.ascontiguousarray(got[others]), np.ascontiguousarray(want[others])), k
        with pytest.raises(pt.PtkError) as invalid:
            tree.search_knn_within(c.q, k, r)
        assert invalid.value.status == -1 and "radii[37]" in str(invalid.value)
    r = c.mixed_radii(16)
    want = c.counts(r)
    r[37], r[101] = np.nan, -1.0
    want[[37, 101]] = 0
    got = tree.count_within(dq, torch.from_numpy(r).to(dq.device)).cpu().numpy()
    assert np.array_equal(got, want)
    with pytest.raises(pt.PtkError) as invalid:
        tree.count_within(c.q, r)
    assert invalid.value.status == -1 and "radii[37]" in str(invalid.value)


@pytest.mark.gpu
def test_side_stream_layouts_and_validation(gpu):
    import torch

    p, q = ds.uniform_cloud(10_000, 3, 71), ds.uniform_cloud(4_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    r = hashed_radii(len(q), [0.0, 0.0005, 0.002, 0.01, INF])
    want = tree.search_knn_within(q, 8, r)
    want_counts = tree.count_within(q, r)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        dq = torch.from_numpy(q).to(f"cuda:{gpu}", non_blocking=False)
        dr = torch.from_numpy(r).to(f"cuda:{gpu}", non_blocking=False) * 1.0  # (made by a kernel of this stream)
        got = tree.search_knn_within(dq, 8, dr)
        got_counts = tree.count_within(dq, dr)
    side.synchronize()
    assert got.numpy().tobytes() == want.tobytes()
    assert np.array_equal(got_counts.cpu().numpy(), want_counts)
    # a caller-supplied nns, host and device
    nns = np.empty((len(q), 8), dtype=pt.NEIGHBOR)
    assert tree.search_knn_within(q, 8, r, nns) is nns and nns.tobytes() == want.tobytes()
    raw = torch.empty((len(q), 8, 2), dtype=torch.int32, device=dq.device)
    assert tree.search_knn_within(dq, 8, dr, raw).raw is raw
    torch.cuda.synchronize()
    assert pt.DeviceNeighbors(raw).numpy().tobytes() == want.tobytes()
    # column-major queries, (sdim, nq): the (k, nq) layout of search_knn
    fq = np.asfortranarray(q.T)
    col = tree.search_knn_within(fq, 8, r)
    assert col.shape == (8, len(q)) and col.reshape(-1).tobytes() == want.reshape(-1).tobytes()
    assert np.array_equal(tree.count_within(fq, r), want_counts)
    assert tree.search_knn_within(q, 1, r).shape == (len(q),)
    # a list of python floats, and radii of another float type, are converted to the tree's dtype
    assert tree.search_knn_within(q[:100], 8, [float(x) for x in r[:100]]).tobytes() == want[:100].tobytes()
    assert np.array_equal(tree.count_within(q, r.astype(np.float64)), want_counts)
    # CUDA queries: radii on the host, of the wrong dtype, length, shape or layout are refused before any library call
    for bad in (r, torch.from_numpy(r), dr.double(), dr[:-1], dr.reshape(-1, 1), torch.stack([dr, dr], 1)[:, 0]):
        with pytest.raises(ValueError):
            tree.search_knn_within(dq, 8, bad)
        with pytest.raises(ValueError):
            tree.count_within(dq, bad)
    with pytest.raises(ValueError):
        tree.search_knn_within(q, 8, dr)  # (host queries take host radii)


@pytest.mark.gpu
@needs_reference
def test_counts_from_below_the_leaf_spacing_to_beyond_the_cloud(gpu):
    """The piles cloud of tests/test_knn_within.py::test_duplicated_points; radii from far below the grid spacing to
    beyond the cloud's diameter in one batch."""
    p = (np.round(ds.uniform_cloud(50_000, 3, 61) * 4) / 4).astype(np.float32)
    q = ds.uniform_cloud(1_200, 3, 62)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 4, device=gpu)
    assert tree.piles()["piles"] > 0
    c = Case(p, q, 4, "L2Squared")
    r = hashed_radii(len(q), [1e-9, 1e-4, 0.01, 0.07, 0.3, 1.0, 4.0, INF])
    want = c.counts(r)
    assert want.min() == 0 and want.max() == len(p)
    for mc in (0, 16):
        assert np.array_equal(tree.count_within(c.q, r, mc), np.minimum(want, mc) if mc else want), mc
