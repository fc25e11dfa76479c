"""search_radius_self / count_within_self: each tree point's neighbours within a radius among the OTHER points (ptk.h,
DESIGN.md §2).

Expected rows always come from the compiled reference: its ``search_radius(p_i, r_i)`` row for each tree point with the
entry whose index is i removed (``without_self``).  Only on streams that do not belong to their points do they come from
the library's host loop ``ptk_host_search_radius`` on the same tree and points pair, as tests/test_count_within.py does.

Neither "drop the first entry" nor "the count minus one" is this function, and the tests say on their own data why:
``own_kinds`` counts the rows whose own point is the first entry / a later entry / absent, and every parametrisation
that could pass for the wrong reason asserts the mix it relies on.

The CPU tier checks the host loops on a host-only handle, the real source of count_self_kernel /
radius_self_fill_kernel and their float64 pair in the emulator (tests/cpp/emulate_radius_self.cpp) and the per-point C++
member (tests/cpp/radius_self_main.cpp); the gpu tier checks the device search, float32 and float64, and the batched C++
members.
"""

from __future__ import annotations

import contextlib
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
INF = float("inf")
METRICS = ["L2Squared", "L1", "LPInf", "LNInf"]
_EMU_METRIC = {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")
needs_reference64 = pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")


# ---- clouds, radii and expected values --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cloud(kind):
    """(points, leaf size) of a small test cloud (the clouds of tests/test_knn_self.py); shared and read-only."""
    if kind == "uniform":
        p, leaf = ds.uniform_cloud(3_000, 3, 1), 10
    elif kind == "lidar":
        p, leaf = ds.lidar_cloud(4_000, seed=3), 10
    elif kind == "ties":  # coordinates on a 1/8 grid: many equal distances, piles of coincident points
        p, leaf = (np.round(ds.uniform_cloud(3_000, 3, 5) * 8) / 8).astype(np.float32), 6
    elif kind == "2d":
        p, leaf = ds.uniform_cloud(2_500, 2, 8), 7
    elif kind == "5d":
        p, leaf = ds.uniform_cloud(2_500, 5, 10), 10
    elif kind == "small":  # the cloud of the whole-tree rows
        p, leaf = ds.uniform_cloud(600, 3, 17), 5
    elif kind == "1d":
        p, leaf = ds.uniform_cloud(2_000, 1, 19), 6
    else:
        raise ValueError(kind)
    p = np.ascontiguousarray(p)
    p.flags.writeable = False
    return p, leaf


def row_ids(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(np.asarray(off).astype(np.int64)))


def without_self(off, flat):
    """(offsets, flat) of rows computed for the tree's own points, each without the entry whose index is the row's."""
    rows = row_ids(off)
    own = flat["index"] == rows
    per_row = np.bincount(rows[own], minlength=len(off) - 1)
    assert per_row.max(initial=0) <= 1  # (an index occurs at most once in a row)
    out = np.zeros(len(off), dtype=np.uint64)
    out[1:] = np.cumsum(np.diff(np.asarray(off).astype(np.int64)) - per_row)
    return out, np.ascontiguousarray(flat[~own])


def own_kinds(off, flat):
    """(rows whose own point is the first entry, rows where it is a later entry, rows without it)."""
    rows = row_ids(off)
    own = np.flatnonzero(flat["index"] == rows)
    first = int((own == np.asarray(off).astype(np.int64)[rows[own]]).sum())
    return first, len(own) - first, len(off) - 1 - len(own)


@contextlib.contextmanager
def reference_threads(ref, n):
    """At most n OpenMP threads for the reference calls inside, whatever thread count another test module has left on the
    process-wide runtime (every core of the machine, where a test process may use a few of them: oversubscribed regions
    take many times as long); the count found is put back."""
    threads = ref.max_threads()
    ref.set_threads(min(n, threads))
    try:
        yield
    finally:
        ref.set_threads(threads)


def reference_rows_per_row(ref, p, radii, sort=False):
    """(offsets, flat) of the reference with one radius per row: one run per row, every radius being its own.  The runs
    go single-threaded: a call of one query is one OpenMP region, and thousands of oversubscribed regions take minutes
    where this takes a fraction of a second."""
    with reference_threads(ref, 1):
        per_row = [ref.search_radius(p[i:i + 1], radii[i], sort=sort)[1] for i in range(len(p))]
    off = np.zeros(len(p) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in per_row])
    return off, np.concatenate(per_row)


class Case:
    """A cloud with its reference tree; what the reference gives is computed once per (radius, sort) and shared."""

    def __init__(self, kind, metric, dtype=np.float32):
        p, self.leaf = cloud(kind)
        self.kind, self.metric, self.dtype = kind, metric, np.dtype(dtype)
        self.p = np.ascontiguousarray(p.astype(dtype))
        self.n = len(self.p)
        self.ref = oracle.Oracle(self.p, self.leaf, "reference", metric=metric, dtype=dtype)
        self._raw, self._per_row, self._values = {}, {}, None
        self._kth = None

    def kth(self):
        """The distance of each point's 8th nearest OTHER point: row 7 of search_knn_self(8) as the reference has it (the
        9-row without its first entry of index i, else without its last)."""
        if self._kth is None:
            with reference_threads(self.ref, 8):
                rows = self.ref.search_knn(self.p, 9)
            hit = rows["index"] == np.arange(self.n)[:, None]
            pos = np.where(hit.any(1), hit.argmax(1), 8)
            keep = np.ones(hit.shape, dtype=bool)
            keep[np.arange(self.n), pos] = False
            self._kth = np.ascontiguousarray(rows[keep].reshape(self.n, 8)["distance"][:, 7])
        return self._kth

    def values(self, rows=True):
        """The scalar radii of the module: 0, the median and 4 x the median of the 8th-neighbour distance; on "ties" the
        grid step exactly (neighbours AT r stay out) and the next number above it; for counts FLT_MAX / DBL_MAX and +inf
        as well; for rows a whole-tree radius only on the 600-point cloud."""
        if self._values is None:
            t = self.dtype.type
            with reference_threads(self.ref, 8):
                med = t(np.median(self.ref.search_knn(self.p, 9)["distance"][:, 8]))
            v = [t(0), med, t(4) * med]
            if self.kind == "ties":
                step = t(0.125 * 0.125) if self.metric == "L2Squared" else t(0.125)
                v += [step, np.nextafter(step, t(np.inf))]
            self._values = v
        huge = [self.dtype.type(np.finfo(self.dtype).max), self.dtype.type(np.inf)]
        return self._values + (huge if not rows or self.kind == "small" else [])

    def raw(self, r, sort=False):
        """The reference's rows of the tree's own points at the scalar radius r, own entries included."""
        key = (self.dtype.type(r).tobytes(), bool(sort))
        if key not in self._raw:
            with reference_threads(self.ref, 8):
                off, flat = self.ref.search_radius(self.p, r, sort=sort)
            off.setflags(write=False)
            flat.setflags(write=False)
            self._raw[key] = (off, flat)
        return self._raw[key]

    def want(self, r, sort=False):
        return without_self(*self.raw(r, sort))

    def radii(self):
        """One radius per point: the 8th-neighbour distance (the 8th neighbour itself is out: strict), with entries set
        to 0, a subnormal, +inf and the largest finite number."""
        r = self.kth().astype(self.dtype).copy()
        r[5::97] = 0
        r[11::211] = np.finfo(self.dtype).smallest_subnormal
        r[17::701] = np.inf
        r[23::997] = np.finfo(self.dtype).max
        return r

    def raw_per_row(self, sort=False):
        """The reference's rows with radii(): one run per row (every radius is its own)."""
        if sort not in self._per_row:
            self._per_row[sort] = reference_rows_per_row(self.ref, self.p, self.radii(), sort)
        return self._per_row[sort]

    def want_per_row(self, sort=False):
        return without_self(*self.raw_per_row(sort))


@functools.lru_cache(maxsize=None)
def case(kind, metric, dtype="float32"):
    return Case(kind, metric, np.dtype(dtype))


def clamp(off, mc):
    c = np.diff(np.asarray(off).astype(np.int64))
    return np.minimum(c, mc) if mc else c


def check_rows(got_off, got_flat, want, sort, what):
    """sort = 0: equal offsets, indices and distance bits.  sort = 1: equal distance bits, equal index sets per row (ties
    are in unspecified order for float32)."""
    off, flat = want
    assert np.array_equal(np.asarray(got_off).astype(np.uint64), off), what
    got_flat = np.asarray(got_flat)
    assert len(got_flat) == len(flat), what
    assert np.ascontiguousarray(got_flat["distance"]).tobytes() == np.ascontiguousarray(flat["distance"]).tobytes(), what
    if not sort:
        assert np.array_equal(got_flat["index"], flat["index"]), what
        return
    row = row_ids(off)
    a, b = got_flat["index"], flat["index"]
    assert np.array_equal(a[np.lexsort((a, row))], b[np.lexsort((b, row))]), what


def assert_own_point_is_not_always_first(c):
    """On a tree built from its points every point is in its own row; some rows have it first and some later."""
    r = max(c.values()[:5])  # (the largest of the cloud's own radii: non-empty rows -- under the minimum metric the
    first, later, absent = own_kinds(*c.raw(r))  # median 8th-neighbour distance of "ties" is 0)
    assert first > 0 and later > 0 and absent == 0, (c.kind, c.metric, first, later, absent)


def assert_ties_keep_coincident_points(c):
    off, flat = c.want(max(c.values()[:5]))
    assert (flat["distance"] == 0).sum() > 0, (c.kind, c.metric)


GUARD = 8


def guarded(n, dtype):
    """An output array of n entries between two runs of GUARD entries, all 0xA5 bytes: (whole buffer, the n entries)."""
    buf = np.empty(n + 2 * GUARD, dtype=dtype)
    buf.view(np.uint8).reshape(-1)[:] = 0xA5
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    raw = buf.view(np.uint8).reshape(len(buf), -1)
    return bool(np.all(raw[:GUARD] == 0xA5) and np.all(raw[-GUARD:] == 0xA5))


def host_counts(tree, r, mc=0, points=None):
    """ptk_host_search_count_within_self into a guarded buffer; r a scalar or an array."""
    lib = pt._load()
    p = tree._pts if points is None else points
    buf, counts = guarded(len(p), np.int64)
    scalar = np.ndim(r) == 0
    rc = lib.ptk_host_search_count_within_self(tree._h, p.ctypes.data, np.float32(r if scalar else 0),
                                               None if scalar else r.ctypes.data, mc, counts.ctypes.data)
    assert rc == 0, lib.ptk_last_error()
    assert guards_intact(buf) and not np.any(counts == np.int64(-0x5A5A5A5A5A5A5A5B)), "a count was not written"
    return counts.copy()


def host_rows(tree, r, sort=0, points=None):
    lib = pt._load()
    p = tree._pts if points is None else points
    buf, offsets = guarded(len(p) + 1, np.uint64)
    rows = ctypes.c_void_p()
    scalar = np.ndim(r) == 0
    rc = lib.ptk_host_search_radius_self(tree._h, p.ctypes.data, np.float32(r if scalar else 0),
                                         None if scalar else r.ctypes.data, sort, offsets.ctypes.data, ctypes.byref(rows))
    assert rc == 0, lib.ptk_last_error()
    assert guards_intact(buf)
    return offsets.copy(), pt._adopt(lib, rows, int(offsets[-1]), pt.NEIGHBOR)


# ---- CPU tier: the host loops on a host-only handle ---------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "5d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loops_equal_the_reference_rows_without_self(kind, metric):
    c = case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    if kind != "5d":
        assert_own_point_is_not_always_first(c)
    if kind == "ties":
        assert_ties_keep_coincident_points(c)
    for r in c.values(rows=False):
        off, _ = c.want(r)
        for mc in (0, 7):
            assert np.array_equal(host_counts(tree, r, mc), clamp(off, mc)), (kind, metric, r, mc)
    for r in c.values():
        for sort in (0, 1):
            got_off, got = host_rows(tree, r, sort)
            check_rows(got_off, got, c.want(r, sort), sort, (kind, metric, r, sort))
    radii = c.radii()
    off, _ = c.want_per_row()
    for mc in (0, 7):
        assert np.array_equal(host_counts(tree, radii, mc), clamp(off, mc)), (kind, metric, "per row", mc)
    for sort in (0, 1):
        got_off, got = host_rows(tree, radii, sort)
        check_rows(got_off, got, c.want_per_row(sort), sort, (kind, metric, "per row", sort))


@needs_reference
def test_the_clamp_applies_after_the_own_entry_has_left():
    """max_count = c with rows whose length BEFORE the removal is exactly c + 1: min(len - own, c) = c there, where
    min(len, c) - own would give c - 1."""
    c = case("uniform", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=pt.PTK_DEVICE_NONE)
    r = c.values()[1]
    off, flat = c.raw(r)
    before = np.diff(off.astype(np.int64))
    mc = 7
    at = np.flatnonzero(before == mc + 1)
    assert len(at) > 0
    got = host_counts(tree, r, mc)
    assert np.all(got[at] == mc)
    assert np.array_equal(got, clamp(c.want(r)[0], mc))


def test_the_reference_rows_are_the_ones_the_issue_counted():
    if not oracle.have_reference():
        pytest.skip("compiled reference not present")
    # (metric units: the squared radius -- r = 0.1 on "uniform" is 0.01, r = 32 on "lidar" is 1 024)
    c = case("uniform", "L2Squared")
    assert own_kinds(*c.raw(np.float32(0.01))) == (735, 2265, 0)
    lidar = case("lidar", "L2Squared")
    assert own_kinds(*lidar.raw(np.float32(1024.0))) == (1535, 2465, 0)
    # r^2 = 1e-60 underflows to 0 in float32: empty rows, the own point included
    assert own_kinds(*c.raw(np.float32(1e-60))) == (0, 0, 3000)


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loops_of_the_topological_metrics(metric):
    rng = np.random.default_rng(12)
    p = rng.random((2_000, 1 if metric == "SO2" else 3), dtype=np.float32)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    ref = oracle.Oracle(p, 8, "reference", metric=metric)
    med = np.float32(np.median(ref.search_knn(p, 9)["distance"][:, 8]))
    for r in (np.float32(0), med, np.float32(4) * med):
        want = without_self(*ref.search_radius(p, r))
        assert np.array_equal(host_counts(tree, r), clamp(want[0], 0)), (metric, r)
        assert np.array_equal(host_counts(tree, r, 3), clamp(want[0], 3)), (metric, r)
        got_off, got = host_rows(tree, r)
        check_rows(got_off, got, want, 0, (metric, r))
    radii = np.full(len(p), med, dtype=np.float32)
    radii[::3] = 0
    got_off, got = host_rows(tree, radii)
    want = without_self(*ref.search_radius(p, med))
    lens = np.diff(want[0].astype(np.int64))
    lens[::3] = 0
    assert np.array_equal(np.diff(got_off.astype(np.int64)), lens)


def _tiny_expected(p, r):
    """Rows of a tiny tree by brute force over the host loop of search_radius: every other point below r."""
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    off = np.zeros(len(p) + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    assert lib.ptk_host_search_radius(tree._h, p.ctypes.data, p.ctypes.data, len(p), np.float32(r), np.float32(1), 0,
                                      off.ctypes.data, ctypes.byref(rows)) == 0
    return without_self(off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_host_loops_of_tiny_trees(n):
    p = ds.uniform_cloud(n, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    for r in (0.0, 0.05, 10.0, INF):
        want = _tiny_expected(p, r)
        if r >= 10.0:
            assert np.all(np.diff(want[0].astype(np.int64)) == n - 1)
        assert np.array_equal(host_counts(tree, r), clamp(want[0], 0)), (n, r)
        got_off, got = host_rows(tree, r)
        check_rows(got_off, got, want, 0, (n, r))


def test_argument_checks_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    counts = np.zeros(9, dtype=np.int64)
    off = np.zeros(10, dtype=np.uint64)
    rows = ctypes.c_void_p()
    ok = np.full(9, 0.1, dtype=np.float32)
    INVALID, DEVICE = -1, -3
    # null arguments
    assert lib.ptk_host_search_count_within_self(tree._h, p.ctypes.data, np.float32(0.1), None, 0, None) == INVALID
    assert lib.ptk_host_search_count_within_self(tree._h, None, np.float32(0.1), None, 0, counts.ctypes.data) == INVALID
    assert lib.ptk_host_search_count_within_self(None, p.ctypes.data, np.float32(0.1), None, 0, counts.ctypes.data) == INVALID
    assert lib.ptk_host_search_radius_self(tree._h, p.ctypes.data, np.float32(0.1), None, 0, None, ctypes.byref(rows)) == INVALID
    assert lib.ptk_host_search_radius_self(tree._h, p.ctypes.data, np.float32(0.1), None, 0, off.ctypes.data, None) == INVALID
    # a NaN or negative scalar radius
    for bad in (np.nan, -0.5, -INF):
        assert lib.ptk_host_search_count_within_self(tree._h, p.ctypes.data, np.float32(bad), None, 0,
                                                     counts.ctypes.data) == INVALID
        assert lib.ptk_host_search_radius_self(tree._h, p.ctypes.data, np.float32(bad), None, 0, off.ctypes.data,
                                               ctypes.byref(rows)) == INVALID
        assert "radius must be >= 0" in lib.ptk_last_error().decode()
        # (ignored when an array is given)
        assert lib.ptk_host_search_count_within_self(tree._h, p.ctypes.data, np.float32(bad), ok.ctypes.data, 0,
                                                     counts.ctypes.data) == 0
    # a NaN or negative entry is named by its row: the first such row
    for bad in (np.nan, -1e-3):
        radii = ok.copy()
        radii[4] = radii[7] = bad
        assert lib.ptk_host_search_count_within_self(tree._h, p.ctypes.data, np.float32(1), radii.ctypes.data, 0,
                                                     counts.ctypes.data) == INVALID
        assert "radii[4]" in lib.ptk_last_error().decode()
        assert lib.ptk_host_search_radius_self(tree._h, p.ctypes.data, np.float32(1), radii.ctypes.data, 0, off.ctypes.data,
                                               ctypes.byref(rows)) == INVALID
        assert "radii[4]" in lib.ptk_last_error().decode()
    # a host-only handle has no device search: PTK_ERR_DEVICE, from every device entry point
    assert lib.ptk_search_count_within_self(tree._h, np.float32(0.1), None, 0, counts.ctypes.data) == DEVICE
    assert lib.ptk_search_count_within_self_device(tree._h, np.float32(0.1), None, 0, counts.ctypes.data, None) == DEVICE
    assert lib.ptk_search_radius_self(tree._h, np.float32(0.1), None, 0, off.ctypes.data, ctypes.byref(rows)) == DEVICE
    assert lib.ptk_search_radius_self_fill_device(tree._h, np.float32(0.1), None, off.ctypes.data, counts.ctypes.data, 0,
                                                  None) == DEVICE
    assert lib.ptk_search_count_within_self(None, np.float32(0.1), None, 0, counts.ctypes.data) == INVALID
    assert lib.ptk_search_radius_self(tree._h, np.float32(0.1), None, 0, None, ctypes.byref(rows)) == INVALID
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    assert lib.ptk_search64_count_within_self(t64._h, 0.1, None, 0, counts.ctypes.data) == DEVICE
    assert lib.ptk_search64_count_within_self_device(t64._h, 0.1, None, 0, counts.ctypes.data, None) == DEVICE
    assert lib.ptk_search64_radius_self(t64._h, 0.1, None, 0, off.ctypes.data, ctypes.byref(rows)) == DEVICE
    assert lib.ptk_version() == 101
    with pytest.raises(pt.PtkError):
        tree.count_within_self(0.1)
    with pytest.raises(pt.PtkError):
        tree.search_radius_self(0.1)
    for bad in (np.zeros(8, dtype=np.float32), np.zeros((9, 1), dtype=np.float32), "x"):
        with pytest.raises(ValueError):
            tree.count_within_self(bad)
    with pytest.raises(ValueError):
        tree.count_within_self(0.1, max_count=-1)


# ---- CPU tier: the real kernel source in the emulator ----------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/cpp/emulate_radius_self.cpp, compiled with the emulator's g++ line and HIP stand-in (__graft_entry__.build)."""
    out = str(tmp_path_factory.mktemp("emu_rself") / "libptk_emu_rself.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_radius_self.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.emu_create.restype = vp
    lib.emu_create.argtypes = [vp, u64, ctypes.c_uint32, vp, u64, vp]
    lib.emu_destroy.argtypes = [vp]
    lib.emu_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu_count_self.argtypes = [vp, u64, u64, u64, ctypes.c_float, vp, u64, ctypes.c_int, vp, vp]
    lib.emu_radius_self_fill.argtypes = [vp, u64, u64, u64, ctypes.c_float, vp, vp, vp, u64]
    lib.emu64_create.restype = vp
    lib.emu64_create.argtypes = [vp, u64, ctypes.c_uint32, u64]
    lib.emu64_destroy.argtypes = [vp]
    lib.emu64_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu64_count_self.argtypes = [vp, u64, ctypes.c_double, vp, u64, ctypes.c_int, vp, vp]
    lib.emu64_radius_self_fill.argtypes = [vp, u64, ctypes.c_double, vp, vp, vp, ctypes.c_int]
    return lib


class Emulated:
    """The float32 kernels over a tree built by the product's host builder over `tree_points` (default: the points
    themselves) and searched over `p`: a stream that does not belong to its points when the two differ."""

    def __init__(self, lib, p, leaf, metric, tree_points=None):
        self.lib, self.p = lib, np.ascontiguousarray(p, dtype=np.float32)
        self.host = pt.KdTree(self.p if tree_points is None else tree_points, getattr(pt.Metric, metric), leaf,
                              device=pt.PTK_DEVICE_NONE)
        nodes, self.idx, _, _ = self.host.flat()
        self.n = len(self.p)
        self.h = lib.emu_create(self.p.ctypes.data, self.n, self.p.shape[1], nodes.ctypes.data, len(nodes),
                                self.idx.ctypes.data)
        assert self.h
        lib.emu_set_metric(self.h, _EMU_METRIC[metric])

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.emu_destroy(self.h)
            self.h = None

    def counts(self, r, mc=0, shortcut=1, piece=0, span=None):
        """(counts with -7 where no lane wrote, the four counters)."""
        lo, hi = span or (0, self.n)
        out = np.full(self.n, -7, dtype=np.int64)
        stats = np.zeros(4, dtype=np.uint32)
        scalar = np.ndim(r) == 0
        assert self.lib.emu_count_self(self.h, lo, hi, piece, np.float32(r if scalar else 0),
                                       None if scalar else r.ctypes.data, mc, shortcut, out.ctypes.data,
                                       stats.ctypes.data) == 0
        return out, stats

    def rows(self, r, counts, sort=0, piece=0, span=None):
        """The fill pass behind `counts` (those of max_count = 0; rows nobody counted are empty)."""
        lo, hi = span or (0, self.n)
        off = np.zeros(self.n + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.maximum(counts, 0))
        buf, out = guarded(int(off[-1]), pt.NEIGHBOR)
        scalar = np.ndim(r) == 0
        assert self.lib.emu_radius_self_fill(self.h, lo, hi, piece, np.float32(r if scalar else 0),
                                             None if scalar else r.ctypes.data, off.ctypes.data, out.ctypes.data,
                                             self.n if sort else 0) == 0
        assert guards_intact(buf)
        return off, out.copy()


@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_kernels_equal_the_reference_rows_without_self(emu_lib, kind, metric):
    """Scalar and per-row, shortcut on and off, counts with and without max_count, rows in both orders; 647 leaf positions
    per launch: pieces that end inside a wavefront, and a ragged last one."""
    c = case(kind, metric)
    emu = Emulated(emu_lib, c.p, c.leaf, metric)
    assert_own_point_is_not_always_first(c)
    fired = np.zeros(4, dtype=np.int64)
    for r in c.values(rows=False):
        off, _ = c.want(r)
        want = clamp(off, 0)
        for mc, sc, piece in ((0, 1, 0), (7, 1, 647), (0, 0, 647)):
            got, stats = emu.counts(r, mc, sc, piece)
            assert np.array_equal(got, np.minimum(want, mc) if mc else want), (kind, metric, r, mc, sc)
            fired += stats
            assert sc or not stats.any()
    # (the whole-tree radii swallow subtrees; the root's box holds every point of a tree built from its points)
    assert fired[0] > 0 and fired[1] > 0 and fired[3] > 0, fired
    for r in c.values():
        want = c.want(r)
        counts = clamp(want[0], 0)
        for sort, piece in ((0, 647), (1, 0)):
            got_off, got = emu.rows(r, counts, sort, piece)
            check_rows(got_off, got, c.want(r, sort), sort, (kind, metric, r, sort))
    radii = c.radii()
    want = c.want_per_row()
    for mc, sc, piece in ((0, 1, 647), (7, 1, 0), (0, 0, 0)):
        got, _ = emu.counts(radii, mc, sc, piece)
        assert np.array_equal(got, clamp(want[0], mc)), (kind, metric, "per row", mc, sc)
    for sort in (0, 1):
        got_off, got = emu.rows(radii, clamp(want[0], 0), sort, 647)
        check_rows(got_off, got, c.want_per_row(sort), sort, (kind, metric, "per row", sort))


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_kernels_where_the_leaf_scan_changes(emu_lib, L):
    """The CPU half of tests/test_leaf_boundaries.py for these kernels: a tree whose largest leaf has exactly 31 | 32 | 33
    and 64 | 65 points (the count bits of the leaf reference go 5 -> 6 -> 7); radii that hold a part of that leaf from
    its own points, all of it, and nothing."""
    pts, blob, q, nb, ref, radii = leaf_cases.case(L)
    pts = np.asarray(pts)
    emu = Emulated(emu_lib, pts, L, "L2Squared")
    leaf_cases.assert_leaf(emu.host, L)
    for r in leaf_cases.self_radii(L, radii):
        want = leaf_cases.self_rows(ref, pts, r)
        counts = clamp(want[0], 0)
        assert r != radii[1] or np.all(counts[len(pts) - L:] == L - 1)  # (r_all: every blob point's row is the blob)
        for mc, sc, piece in ((0, 1, 0), (7, 1, 647), (0, 0, 647)):
            got, _ = emu.counts(r, mc, sc, piece)
            assert np.array_equal(got, np.minimum(counts, mc) if mc else counts), (L, r, mc, sc)
        for sort, piece in ((0, 647), (1, 0)):
            got_off, got = emu.rows(r, counts, sort, piece)
            check_rows(got_off, got, leaf_cases.self_rows(ref, pts, r, sort=bool(sort)), sort, (L, r, sort))


@needs_reference
def test_emulated_count_with_max_count_tells_the_two_clamps_apart(emu_lib):
    c = case("uniform", "L2Squared")
    emu = Emulated(emu_lib, c.p, c.leaf, "L2Squared")
    r, mc = c.values()[1], 7
    before = np.diff(c.raw(r)[0].astype(np.int64))
    at = np.flatnonzero(before == mc + 1)
    assert len(at) > 0
    got, _ = emu.counts(r, mc)
    assert np.all(got[at] == mc) and np.array_equal(got, clamp(c.want(r)[0], mc))


def test_emulated_per_row_radii_that_pass_no_test(emu_lib):
    """A NaN and a negative radii entry (the _device forms cannot look): count 0, the fill lane leaves before it touches
    the output, every other row is unaffected."""
    p, leaf = cloud("uniform")
    emu = Emulated(emu_lib, p, leaf, "L2Squared")
    radii = np.full(len(p), 0.01, dtype=np.float32)
    clean, _ = emu.counts(radii)
    clean_off, clean_rows = emu.rows(radii, clean)
    radii[100], radii[2000] = np.nan, -1.0
    got, _ = emu.counts(radii)
    assert got[100] == 0 and got[2000] == 0
    keep = np.ones(len(p), dtype=bool)
    keep[[100, 2000]] = False
    assert np.array_equal(got[keep], clean[keep]) and clean[100] > 0 and clean[2000] > 0
    off, rows = emu.rows(radii, got)
    rid, crid = row_ids(off), row_ids(clean_off)
    assert rows.tobytes() == clean_rows[keep[crid]].tobytes() and not np.any(np.isin(rid, [100, 2000]))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_emulated_kernels_on_a_stream_that_does_not_belong_to_its_points(emu_lib, metric, move):
    """A tree built over one cloud, searched over a shrunk or shifted copy of it (ptk_tree_create_from_stream checks
    nothing): a point is then often absent from its own row, so "the count minus one" is a different function.  Expected:
    the library's host loop ptk_host_search_radius on the same tree and points pair, the own entries removed."""
    p_tree = ds.uniform_cloud(3_000, 3, 61)
    p = (p_tree * np.float32(0.5) + np.float32(0.25)) if move == "shrunk" else (p_tree + np.float32(0.3))
    p = np.ascontiguousarray(p, dtype=np.float32)
    emu = Emulated(emu_lib, p, 8, metric, tree_points=p_tree)
    lib = pt._load()
    fired = np.zeros(4, dtype=np.int64)
    mixed = False
    for r in (0.001, 0.01, 0.05, 0.1, 0.3, 1.0, FLT_MAX):
        off = np.zeros(len(p) + 1, dtype=np.uint64)
        rows = ctypes.c_void_p()
        assert lib.ptk_host_search_radius(emu.host._h, p.ctypes.data, p.ctypes.data, len(p), np.float32(r), np.float32(1),
                                          0, off.ctypes.data, ctypes.byref(rows)) == 0
        raw = (off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR))
        first, later, absent = own_kinds(*raw)
        mixed = mixed or (first + later > 0 and absent > 0)
        if metric == "L2Squared" and r == 0.05:
            assert first + later == (2496 if move == "shrunk" else 42), (move, first, later, absent)
        want = without_self(*raw)
        for sc in (1, 0):
            got, stats = emu.counts(r, 0, sc)
            assert np.array_equal(got, clamp(want[0], 0)), (metric, move, r, sc)
            fired += stats
        got7, _ = emu.counts(r, 7)
        assert np.array_equal(got7, clamp(want[0], 7)), (metric, move, r)
        if r <= 0.3:
            got_off, got_rows = emu.rows(r, got)
            check_rows(got_off, got_rows, want, 0, (metric, move, r))
        # the host loops of the self form on the same pair
        assert np.array_equal(host_counts(emu.host, r, points=p), clamp(want[0], 0)), (metric, move, r)
        if r <= 0.3:
            h_off, h_rows = host_rows(emu.host, r, points=p)
            check_rows(h_off, h_rows, want, 0, (metric, move, r, "host loop"))
    assert mixed, "every row with, or every row without, its own point: the streams tell nothing apart"
    # inside shortcuts taken, and inside shortcuts refused for the lane's own point
    assert fired[0] > 0 and fired[3] > 0, fired


def test_emulated_kernels_on_a_stream_with_non_finite_points(emu_lib):
    """A handle read from a stream may hold non-finite points: one NaN and one +Inf coordinate.  Such a point's row is
    what the reference's traversal gives it (the host loop on the same pair), and it changes no other row."""
    p_tree, leaf = cloud("uniform")
    p = np.array(p_tree)
    p[700, 1], p[1900, 0] = np.nan, np.inf
    emu = Emulated(emu_lib, p, leaf, "L2Squared", tree_points=p_tree)
    clean = Emulated(emu_lib, p_tree, leaf, "L2Squared")
    lib = pt._load()
    for r in (0.01, 0.1, FLT_MAX, INF):
        off = np.zeros(len(p) + 1, dtype=np.uint64)
        rows = ctypes.c_void_p()
        assert lib.ptk_host_search_radius(emu.host._h, p.ctypes.data, p.ctypes.data, len(p), np.float32(r), np.float32(1),
                                          0, off.ctypes.data, ctypes.byref(rows)) == 0
        want = without_self(off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR))
        for sc in (1, 0):
            got, _ = emu.counts(r, 0, sc)
            assert np.array_equal(got, clamp(want[0], 0)), (r, sc)
        if r <= 0.1:
            got_off, got_rows = emu.rows(r, got)
            check_rows(got_off, got_rows, want, 0, r)
            # no other row changes: the rows of the clean cloud without the two points
            c_counts, _ = clean.counts(r)
            c_off, c_rows = clean.rows(r, c_counts)
            keep = ~np.isin(row_ids(c_off), [700, 1900]) & ~np.isin(c_rows["index"], [700, 1900])
            mine = ~np.isin(row_ids(got_off), [700, 1900]) & ~np.isin(got_rows["index"], [700, 1900])
            assert got_rows[mine].tobytes() == c_rows[keep].tobytes(), r


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [c for c in depth_cases.EUCLID_CASES if c[0] <= 3])
def test_emulated_kernels_where_the_stack_class_changes(emu_lib, dim, leaf, metric, depth):
    """Trees of exactly 39 | 40 and 135 | 136 levels (tests/depth_cases.py).  The rows searched are the far pile of
    coincident points -- every one of them keeps the others at distance 0 and walks the chain of one-point peels -- and
    the 200 leaf positions on either side of it, at a radius that holds the pile only and at one that holds the tree.
    The record stacks stay within 2 * depth + 2 and within what the host's spill class for the depth holds."""
    pts, _ = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    emu = Emulated(emu_lib, pts, leaf, metric)
    at = np.flatnonzero(np.asarray(emu.idx) >= 3_000)  # leaf positions of the pile
    lo, hi = max(0, int(at.min()) - 200), min(len(pts), int(at.max()) + 201)
    rows_done = np.asarray(emu.idx[lo:hi])
    assert np.all(np.isin(np.arange(3_000, len(pts)), rows_done))
    run = depth_cases.Watch(depth, emu_lib)
    n_pile = len(pts) - 3_000
    for r in (np.float32(0.05), np.float32(1e4)):
        want_off, want_flat = without_self(*ref.search_radius(pts, r))
        want = clamp(want_off, 0)
        assert np.all(want[3_000:] >= n_pile - 1)  # (the rest of the pile, at distance 0)
        for mc, sc in ((0, 1), (16, 1), (0, 0)):
            got, _ = run(emu.counts, r, mc, sc, 0, (lo, hi))
            assert np.array_equal(got[rows_done], (np.minimum(want, mc) if mc else want)[rows_done]), (depth, r, mc, sc)
            assert np.all(np.delete(got, rows_done) == -7)
        counts = np.where(np.isin(np.arange(len(pts)), rows_done), want, 0)
        got_off, got_rows = run(emu.rows, r, counts, 0, 0, (lo, hi))
        keep = np.isin(row_ids(want_off), rows_done)
        assert got_rows.tobytes() == want_flat[keep].tobytes(), (depth, r)


@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "ties", "1d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf", "LNInf"])
def test_emulated_float64_kernels_equal_the_reference(emu_lib, kind, metric):
    c = case(kind, metric, "float64")
    lib = emu_lib
    h = lib.emu64_create(c.p.ctypes.data, c.n, c.p.shape[1], c.leaf)
    assert h
    try:
        lib.emu64_set_metric(h, _EMU_METRIC[metric])
        fired = np.zeros(4, dtype=np.int64)

        def counts(r, mc, sc, piece):
            out = np.full(c.n, -7, dtype=np.int64)
            stats = np.zeros(4, dtype=np.uint32)
            scalar = np.ndim(r) == 0
            assert lib.emu64_count_self(h, piece, float(r) if scalar else 0.0, None if scalar else r.ctypes.data, mc, sc,
                                        out.ctypes.data, stats.ctypes.data) == 0
            return out, stats

        def rows(r, cnt, sort, piece):
            off = np.zeros(c.n + 1, dtype=np.uint64)
            off[1:] = np.cumsum(cnt)
            buf, out = guarded(int(off[-1]), pt.NEIGHBOR64)
            scalar = np.ndim(r) == 0
            assert lib.emu64_radius_self_fill(h, piece, float(r) if scalar else 0.0, None if scalar else r.ctypes.data,
                                              off.ctypes.data, out.ctypes.data, sort) == 0
            assert guards_intact(buf)
            assert not poison.record_bytes(out)[:, 4:8].any(), "the padding word of a record is not zero"
            return off, out  # (a view: a copy of float64 records would not copy their padding)

        for r in c.values(rows=False):
            want = clamp(c.want(r)[0], 0)
            for mc, sc, piece in ((0, 1, 0), (7, 1, 647), (0, 0, 647)):
                got, stats = counts(r, mc, sc, piece)
                assert np.array_equal(got, np.minimum(want, mc) if mc else want), (kind, metric, r, mc, sc)
                fired += stats
        assert fired[0] > 0 and fired[1] > 0 and fired[3] > 0, fired
        for r in c.values():
            for sort, piece in ((0, 647), (1, 0)):
                got_off, got = rows(r, clamp(c.want(r)[0], 0), sort, piece)
                want = c.want(r, sort)
                check_rows(got_off, got, want, sort, (kind, metric, r, sort))
                if sort:  # (float64: ties by index)
                    rid = row_ids(got_off)
                    order = np.lexsort((got["index"], got["distance"], rid))
                    assert np.array_equal(order, np.arange(len(got)))
        radii = c.radii()
        want = c.want_per_row()
        for mc, sc in ((0, 1), (7, 1), (0, 0)):
            got, _ = counts(radii, mc, sc, 647)
            assert np.array_equal(got, clamp(want[0], mc)), (kind, metric, "per row", mc, sc)
        got_off, got = rows(radii, clamp(want[0], 0), 0, 0)
        check_rows(got_off, got, want, 0, (kind, metric, "per row"))
    finally:
        lib.emu64_destroy(h)


# ---- the C++ members (tests/cpp/radius_self_main.cpp) ----------------------------------------------------------------

def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "radius_self_main.cpp"), "-o", out]
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


def _read_rows(d, name, dtype):
    return (np.fromfile(os.path.join(d, name + ".off"), dtype=np.uint64),
            np.fromfile(os.path.join(d, name + ".bin"), dtype=dtype))


@needs_reference
@needs_reference64
def test_cpp_per_point_member(tmp_path):
    d = str(tmp_path)
    p = _cpp_points(d)
    exe = os.path.join(d, "radius_self_host")
    _cpp_program(exe, host_only=True)
    for r in (0.0, 0.004, 0.05):
        subprocess.check_call([exe, "host", d, repr(r)])
        for name, metric, dtype in (("h_l2", "L2Squared", np.float32), ("h_l1", "L1", np.float32),
                                    ("h_linf", "LPInf", np.float32), ("h_l2d", "L2Squared", np.float64)):
            ref = oracle.Oracle(p.astype(dtype), 10, "reference", metric=metric, dtype=dtype)
            want = without_self(*ref.search_radius(p.astype(dtype), np.float32(r)))
            got_off, got = _read_rows(d, name, want[1].dtype)
            check_rows(got_off, got, want, 0, (name, r))


# ---- gpu tier ---------------------------------------------------------------------------------------------------

def device_counts(tree, r, mc=0):
    """counts through the host-buffer entry point into a guarded 0xA5 buffer."""
    lib = pt._load()
    buf, counts = guarded(tree.npts, np.int64)
    scalar = np.ndim(r) == 0
    fn = lib.ptk_search64_count_within_self if tree._f64 else lib.ptk_search_count_within_self
    rc = fn(tree._h, tree._real(r if scalar else 0), None if scalar else r.ctypes.data, mc, counts.ctypes.data)
    assert rc == 0, lib.ptk_last_error()
    assert guards_intact(buf)
    return counts.copy()


def check_device(tree, c, what):
    """Scalar and per-row, counts (max_count 0 and 7) and rows (sort 0 and 1) of one tree against its Case."""
    for r in c.values(rows=False):
        off, _ = c.want(r)
        for mc in (0, 7):
            assert np.array_equal(device_counts(tree, r, mc), clamp(off, mc)), (what, r, mc)
        assert np.array_equal(tree.count_within_self(r), clamp(off, 0)), (what, r)
    for r in c.values():
        for sort in (False, True):
            got = tree.search_radius_self(r, sort=sort)
            check_rows(got.offsets, got.flat, c.want(r, sort), sort, (what, r, sort))
    radii = c.radii()
    off, _ = c.want_per_row()
    for mc in (0, 7):
        assert np.array_equal(device_counts(tree, radii, mc), clamp(off, mc)), (what, "per row", mc)
    for sort in (False, True):
        got = tree.search_radius_self(radii, sort=sort)
        check_rows(got.offsets, got.flat, c.want_per_row(sort), sort, (what, "per row", sort))


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_equals_the_reference_rows_without_self(gpu, kind, metric, monkeypatch):
    c = case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    assert_own_point_is_not_always_first(c)
    if kind == "ties":
        assert_ties_keep_coincident_points(c)
    check_device(tree, c, (kind, metric))
    # pieces of leaf positions that end inside a wavefront (the piece rule of search_knn_self), and the shortcuts off
    r = c.values()[2]
    monkeypatch.setenv("PTK_MAX_BATCH", "1000")
    assert np.array_equal(device_counts(tree, r, 7), clamp(c.want(r)[0], 7))
    got = tree.search_radius_self(r)
    check_rows(got.offsets, got.flat, c.want(r), 0, (kind, metric, "pieces"))
    monkeypatch.delenv("PTK_MAX_BATCH")
    pt.set_test_knobs(count_shortcut=0)
    try:
        big = c.values(rows=False)[-1]
        assert np.array_equal(device_counts(tree, big), clamp(c.want(big)[0], 0))
    finally:
        pt.set_test_knobs(count_shortcut=None)


@pytest.mark.gpu
@needs_reference
def test_device_max_count_tells_the_two_clamps_apart(gpu):
    c = case("uniform", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    r, mc = c.values()[1], 7
    at = np.flatnonzero(np.diff(c.raw(r)[0].astype(np.int64)) == mc + 1)
    assert len(at) > 0
    got = tree.count_within_self(r, max_count=mc)
    assert np.all(got[at] == mc) and np.array_equal(got, clamp(c.want(r)[0], mc))


@pytest.mark.gpu
@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "1d"])
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_float64_trees(gpu, kind, metric):
    c = case(kind, metric, "float64")
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    assert_own_point_is_not_always_first(c)
    check_device(tree, c, (kind, metric, "float64"))
    got = tree.search_radius_self(c.values()[2], sort=True)
    assert not poison.record_bytes(got.flat)[:, 4:8].any(), "the padding word of a record is not zero"
    import torch
    dev = tree.count_within_self(c.radii(), max_count=5, device=True)
    assert dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), clamp(c.want_per_row()[0], 5))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["L2Squared", "LPInf"])
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_streams_that_do_not_belong_to_their_points(gpu, tmp_path, metric, move):
    """ptk_tree_create_from_stream over a shrunk / shifted copy of the tree's points: some rows hold their own point,
    some do not; expected is the host loop ptk_host_search_radius on the same pair, the own entries removed."""
    p_tree = ds.uniform_cloud(3_000, 3, 61)
    p = (p_tree * np.float32(0.5) + np.float32(0.25)) if move == "shrunk" else (p_tree + np.float32(0.3))
    p = np.ascontiguousarray(p, dtype=np.float32)
    fn = str(tmp_path / "tree.bin")
    pt.save_kd_tree(pt.KdTree(p_tree, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE), fn)
    tree = pt.load_kd_tree(p, fn, device=gpu)
    lib = pt._load()
    mixed = False
    for r in (0.01, 0.05, 0.3, FLT_MAX):
        off = np.zeros(len(p) + 1, dtype=np.uint64)
        rows = ctypes.c_void_p()
        assert lib.ptk_host_search_radius(tree._h, p.ctypes.data, p.ctypes.data, len(p), np.float32(r), np.float32(1), 0,
                                          off.ctypes.data, ctypes.byref(rows)) == 0
        raw = (off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR))
        first, later, absent = own_kinds(*raw)
        mixed = mixed or (first + later > 0 and absent > 0)
        want = without_self(*raw)
        for mc in (0, 7):
            assert np.array_equal(device_counts(tree, r, mc), clamp(want[0], mc)), (metric, move, r, mc)
        if r <= 0.3:
            got = tree.search_radius_self(r)
            check_rows(got.offsets, got.flat, want, 0, (metric, move, r))
    assert mixed


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
    n_pile = len(pts) - 3_000
    for r in (np.float32(0.05), np.float32(1e4)):
        want = without_self(*ref.search_radius(pts, r))
        assert np.all(clamp(want[0], 0)[3_000:] >= n_pile - 1)
        for mc in (0, 16):
            assert np.array_equal(device_counts(tree, r, mc), clamp(want[0], mc)), (depth, r, mc)
        if r < 1:
            got = tree.search_radius_self(r)
            check_rows(got.offsets, got.flat, want, 0, (depth, r))


def _refused(tree, points, reason, loop):
    """Both calls are PTK_ERR_UNSUPPORTED with the reason and the host loop in the message, and allow_host_loop serves
    them with the host loop's own answer."""
    for call, name in ((lambda: tree.count_within_self(0.01), "ptk_host_search_count_within_self"),
                       (lambda: tree.search_radius_self(0.01), "ptk_host_search_radius_self")):
        with pytest.raises(pt.PtkError) as refused:
            call()
        assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
        assert reason in str(refused.value) and name in str(refused.value), str(refused.value)
    if not loop:
        return
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            counts = tree.count_within_self(0.01, max_count=4)
            rows = tree.search_radius_self(0.01)
    finally:
        pt.allow_host_loop(False)
    assert np.array_equal(counts, host_counts(tree, 0.01, 4, points=points))
    off, flat = host_rows(tree, 0.01, points=points)
    assert np.array_equal(rows.offsets, off) and rows.flat.tobytes() == flat.tobytes()


@pytest.mark.gpu
def test_refused_handles_and_the_host_loop_that_serves_them(gpu):
    p5, leaf5 = cloud("5d")
    _refused(pt.KdTree(p5, pt.Metric.L2Squared, leaf5, device=gpu), p5, "dim > 3", True)
    rng = np.random.default_rng(12)
    pt3 = rng.random((2_000, 3), dtype=np.float32)
    _refused(pt.KdTree(pt3, pt.Metric.SE2Squared, 8, device=gpu), pt3, "topological", True)
    deep, _ = depth_cases.cloud_at_depth(1032, 3, 10)
    deep = np.asarray(deep)
    _refused(pt.KdTree(deep, pt.Metric.L2Squared, 10, device=gpu), deep, "tree depth 1032", True)
    # one level less is served
    ok, _ = depth_cases.cloud_at_depth(1031, 3, 10)
    tree = pt.KdTree(np.asarray(ok), pt.Metric.L2Squared, 10, device=gpu)
    assert np.array_equal(tree.count_within_self(0.01, max_count=9), host_counts(tree, 0.01, 9))
    # float64: dim > 3 is refused too (no host loop for double handles: the exception stands)
    t64 = pt.KdTree(p5.astype(np.float64), pt.Metric.L2Squared, leaf5, device=gpu)
    with pytest.raises(pt.PtkError) as refused:
        t64.count_within_self(0.01)
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED and "dim > 3" in str(refused.value)
    # the argument checks of the device entry points
    lib = pt._load()
    small = pt.KdTree(cloud("small")[0], pt.Metric.L2Squared, 5, device=gpu)
    counts = np.zeros(small.npts, dtype=np.int64)
    off = np.zeros(small.npts + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    bad = np.full(small.npts, 0.1, dtype=np.float32)
    bad[7] = bad[9] = np.nan
    assert lib.ptk_search_count_within_self(small._h, np.float32(0.1), None, 0, None) == -1
    assert lib.ptk_search_count_within_self(small._h, np.float32(np.nan), None, 0, counts.ctypes.data) == -1
    assert lib.ptk_search_count_within_self(small._h, np.float32(-1), None, 0, counts.ctypes.data) == -1
    assert lib.ptk_search_count_within_self(small._h, np.float32(1), bad.ctypes.data, 0, counts.ctypes.data) == -1
    assert "radii[7]" in lib.ptk_last_error().decode()
    assert lib.ptk_search_radius_self(small._h, np.float32(1), bad.ctypes.data, 0, off.ctypes.data, ctypes.byref(rows)) == -1
    assert "radii[7]" in lib.ptk_last_error().decode()
    assert lib.ptk_search_radius_self(small._h, np.float32(-1), None, 0, off.ctypes.data, ctypes.byref(rows)) == -1
    assert lib.ptk_search_count_within_self_device(small._h, np.float32(0.1), None, 0, None, None) == -1
    assert lib.ptk_search_radius_self_fill_device(small._h, np.float32(0.1), None, None, None, 0, None) == -1
    with pytest.raises(ValueError):
        small.count_within_self(bad, device=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_trees_on_the_device(gpu, n):
    p = ds.uniform_cloud(n, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=gpu)
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=gpu)
    for r in (0.0, 0.05, 10.0, INF):
        want = _tiny_expected(p, r)
        assert np.array_equal(device_counts(tree, r), clamp(want[0], 0)), (n, r)
        got = tree.search_radius_self(r)
        check_rows(got.offsets, got.flat, want, 0, (n, r))
        assert np.array_equal(device_counts(t64, r), clamp(want[0], 0)), (n, r, "float64")
        got64 = t64.search_radius_self(r)
        assert np.array_equal(got64.offsets, want[0]) and np.array_equal(got64.flat["index"], want[1]["index"])


def raw_rows(raw):
    """The (total, 2) int32 tensor of the torch device form as NEIGHBOR records."""
    return np.ascontiguousarray(raw.cpu().numpy()).view(pt.NEIGHBOR).reshape(-1)


@pytest.mark.gpu
@needs_reference
def test_torch_device_forms_on_a_side_stream(gpu):
    import torch

    c = case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    r = c.values()[2]
    radii = c.radii()
    with torch.cuda.stream(side):
        d_radii = torch.from_numpy(radii).to(f"cuda:{gpu}")
        counts = tree.count_within_self(r, max_count=7, device=True)
        off, raw = tree.search_radius_self(r, device=True)
        off_s, raw_s = tree.search_radius_self(r, sort=True, device=True)
        counts_r = tree.count_within_self(d_radii, device=True)
        off_r, raw_r = tree.search_radius_self(d_radii, device=True)
        off_h, raw_h = tree.search_radius_self(radii, device=True)  # (host radii: checked, then uploaded)
    side.synchronize()
    assert counts.dtype == torch.int64 and off.dtype == torch.int64 and raw.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy(), clamp(c.want(r)[0], 7))
    check_rows(off.cpu().numpy(), raw_rows(raw), c.want(r), 0, "scalar")
    check_rows(off_s.cpu().numpy(), raw_rows(raw_s), c.want(r, True), 1, "scalar, sorted")
    assert np.array_equal(counts_r.cpu().numpy(), clamp(c.want_per_row()[0], 0))
    check_rows(off_r.cpu().numpy(), raw_rows(raw_r), c.want_per_row(), 0, "per row")
    check_rows(off_h.cpu().numpy(), raw_rows(raw_h), c.want_per_row(), 0, "per row, host radii")
    # a NaN and a negative d_radii entry: empty rows, the neighbours unchanged
    bad = radii.copy()
    bad[100], bad[2000] = np.nan, -1.0
    want_off, want_flat = c.want_per_row()
    lens = np.diff(want_off.astype(np.int64))
    assert lens[100] > 0 and lens[2000] > 0
    keep = ~np.isin(row_ids(want_off), [100, 2000])
    lens[[100, 2000]] = 0
    with torch.cuda.stream(side):
        d_bad = torch.from_numpy(bad).to(f"cuda:{gpu}")
        counts_b = tree.count_within_self(d_bad, device=True)
        off_b, raw_b = tree.search_radius_self(d_bad, device=True)
    side.synchronize()
    assert np.array_equal(counts_b.cpu().numpy(), lens)
    assert np.array_equal(np.diff(off_b.cpu().numpy()), lens) and raw_rows(raw_b).tobytes() == want_flat[keep].tobytes()
    for wrong in (d_bad[:5], d_bad.double(), d_bad.reshape(-1, 1)):
        with pytest.raises(ValueError):
            tree.count_within_self(wrong, device=True)


@pytest.mark.gpu
def test_the_radius_capture_and_the_other_searches_are_left_alone(gpu):
    """A scalar search_radius count / fill pair with a self call between its halves still returns its rows; search_knn,
    count_within and search_knn_self of the same handle are what they were before."""
    import torch

    p, q = ds.uniform_cloud(20_000, 3, 71), ds.uniform_cloud(6_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)

    def others():
        return [tree.search_knn(q, 1).tobytes(), tree.search_knn(q, 16).tobytes(), tree.count_within(q, 0.002).tobytes(),
                tree.search_knn_self(7).tobytes(), tree.search_radius(q, 0.002).flat.tobytes()]

    before = others()
    lib = pt._load()
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    stream = torch.cuda.current_stream(dq.device).cuda_stream
    want = tree.search_radius(q, 0.002)
    counts = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                              counts.data_ptr(), stream) == 0
    self_counts = tree.count_within_self(0.001, device=True)
    self_rows = tree.search_radius_self(np.full(len(p), 0.001, dtype=np.float32))
    offsets = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    offsets[1:] = torch.cumsum(counts[:len(q)], 0)
    out = torch.empty((max(int(offsets[-1].item()), 1), 2), dtype=torch.int32, device=dq.device)
    assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                             offsets.data_ptr(), out.data_ptr(), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want.offsets)
    assert raw_rows(out)[:len(want.flat)].tobytes() == want.flat.tobytes()
    assert np.array_equal(self_counts.cpu().numpy(), np.diff(self_rows.offsets.astype(np.int64)))
    assert others() == before


@pytest.mark.gpu
@needs_reference
@needs_reference64
def test_cpp_batched_members(gpu, tmp_path):
    d = str(tmp_path)
    p = _cpp_points(d)
    exe = os.path.join(d, "radius_self_batch")
    _cpp_program(exe, host_only=False)
    r = np.float32(0.004)
    ref32 = oracle.Oracle(p, 10, "reference")
    radii = np.ascontiguousarray(ref32.search_knn(p, 9)["distance"][:, 8])
    radii[3::50] = 0
    radii.tofile(os.path.join(d, "radii.bin"))
    res = subprocess.run([exe, "batch", d, repr(float(r))], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    for name, dtype in (("b_l2", np.float32), ("b_l2d", np.float64)):
        pd = p.astype(dtype)
        ref = oracle.Oracle(pd, 10, "reference", dtype=dtype)
        want = without_self(*ref.search_radius(pd, r))
        got_off, got = _read_rows(d, name + "_scalar", want[1].dtype)
        check_rows(got_off, got, want, 0, (name, "scalar"))
        assert np.array_equal(np.fromfile(os.path.join(d, name + "_scalar.cnt"), dtype=np.uint64), clamp(want[0], 0))
        want_r = without_self(*reference_rows_per_row(ref, pd, radii.astype(dtype)))
        got_off, got = _read_rows(d, name + "_radii", want[1].dtype)
        check_rows(got_off, got, want_r, 0, (name, "radii"))
        assert np.array_equal(np.fromfile(os.path.join(d, name + "_radii7.cnt"), dtype=np.uint64), clamp(want_r[0], 7))
