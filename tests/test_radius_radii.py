"""search_radius with one radius per query row (ptk.h: ptk_search_radius_radii, ptk_search64_radius_radii,
ptk_search_radius_radii_fill_device, ptk_host_search_radius_radii).

Row i of a per-row call is row i of the scalar search_radius with radius = radii[i] and e = 1.  Expected rows always come
from the compiled reference: one ``Oracle.search_radius`` run per distinct radius on the rows that carry it (the recipe
of ``Case.counts`` in tests/test_within_radii.py, with the rows kept), at most 8 distinct radii per case.

The radii of a batch (``Case.radii``) are seven values assigned by a hash of the row index, so that empty rows, short
rows, long rows and rows that hold the whole cloud sit side by side in one wavefront: 0, half the smallest nearest
distance, the medians of the first and of the 16th neighbour distance, twice the largest 16th distance, the largest finite
number and +inf.

With ``sort = 0`` rows and offsets must be byte-equal; with ``sort = 1`` the distance column must be byte-equal and every
row must hold the same set of indices (ties are in unspecified order for float32).

The CPU tier checks the host loop on a host-only handle, the real source of the two kernels in the emulator
(tests/cpp/emulate_radius_radii.cpp) under a launch order that is not the identity, the argument checks, the C++ members
(tests/cpp/radius_radii_main.cpp) and the Python validation; the gpu tier checks the device searches.  The radius entry
points do not cut a batch into PTK_MAX_BATCH pieces, so there is no case for that.
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
INF = float("inf")
METRICS = ("L2Squared", "L1", "LPInf", "LNInf")
GUARD = 64  # poisoned records behind offsets[nq]

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")
needs_reference64 = pytest.mark.skipif(not oracle.have_reference64(), reason="compiled double reference not present")


def cloud(kind):
    """(points, queries, leaf size): the clouds of tests/test_within_radii.py."""
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


def hashed(n, values, dtype=np.float32):
    """A pseudo-random function of the row index into a few values (so that the reference runs once per value)."""
    i = np.arange(n, dtype=np.uint64)
    return np.asarray(values, dtype=dtype)[((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(len(values))]


class Case:
    """A cloud with its reference tree; the reference's rows are computed once per (radii, sort) and shared."""

    def __init__(self, p, q, leaf, metric, dtype=np.float32):
        self.p, self.q, self.leaf, self.metric, self.dtype = p, np.ascontiguousarray(q), leaf, metric, np.dtype(dtype)
        self.ref = oracle.Oracle(p, leaf, "reference", metric=metric, dtype=dtype)
        self._values = None
        self._rows = {}

    def values(self):
        """The seven radii of the module docstring."""
        if self._values is None:
            d = self.ref.search_knn(self.q, 16)["distance"]
            self._values = [0.0, float(d[:, 0].min()) * 0.5, float(np.median(d[:, 0])), float(np.median(d[:, -1])),
                            float(d[:, -1].max()) * 2, float(np.finfo(self.dtype).max), INF]
        return self._values

    def radii(self, finite_only=False):
        v = self.values()
        return hashed(len(self.q), v[:5] if finite_only else v, self.dtype)

    def rows(self, r, sort=False):
        """(offsets, flat) of the reference for the per-row radii r: one run per distinct radius on its rows."""
        key = (r.tobytes(), bool(sort))
        if key not in self._rows:
            n = len(self.q)
            assert len(np.unique(r)) <= 8
            per_row = [None] * n
            for v in np.unique(r):
                at = np.flatnonzero(r == v)
                off, flat = self.ref.search_radius(np.ascontiguousarray(self.q[at]), v, sort=sort)
                off = np.asarray(off).astype(np.int64)
                for j, i in enumerate(at):
                    per_row[i] = flat[off[j]:off[j + 1]]
            offsets = np.zeros(n + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum([len(x) for x in per_row])
            flat = np.concatenate(per_row) if n else np.empty(0, dtype=self.ref.neighbor)
            offsets.setflags(write=False)
            flat.setflags(write=False)
            self._rows[key] = (offsets, flat)
        return self._rows[key]


_cases = {}


def case(kind, metric, dtype=np.float32, nq=None):
    key = (kind, metric, np.dtype(dtype).name, nq)
    if key not in _cases:
        p, q, leaf = cloud(kind)
        if np.dtype(dtype) == np.float64:
            p, q = p.astype(np.float64) * 1.0000001, q.astype(np.float64) * 1.0000001
        _cases[key] = Case(p, q if nq is None else q[:nq], leaf, metric, dtype)
    return _cases[key]


def prefix(want, nq):
    """The first nq rows of an (offsets, flat) pair."""
    off, flat = want
    return off[:nq + 1], flat[:int(off[nq])]


def check_rows(got_off, got_flat, want, sort, what):
    """sort = 0: byte-equal rows and offsets.  sort = 1: byte-equal distances, equal index sets per row."""
    off, flat = want
    assert np.array_equal(np.asarray(got_off).astype(np.uint64), off), what
    got_flat = np.asarray(got_flat)
    assert len(got_flat) == len(flat), what
    assert np.ascontiguousarray(got_flat["distance"]).tobytes() == np.ascontiguousarray(flat["distance"]).tobytes(), what
    if not sort:
        assert np.array_equal(got_flat["index"], flat["index"]), what
        return
    row = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    a, b = got_flat["index"], flat["index"]
    assert np.array_equal(a[np.lexsort((a, row))], b[np.lexsort((b, row))]), what


def raw_rows(raw):
    """The (total, 2) int32 tensor of the torch device form as NEIGHBOR records."""
    return np.ascontiguousarray(raw.cpu().numpy()).view(pt.NEIGHBOR).reshape(-1)


def host_loop(tree, q, r, sort=0):
    lib = pt._load()
    offsets = np.zeros(len(q) + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    rc = lib.ptk_host_search_radius_radii(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), r.ctypes.data, sort,
                                          offsets.ctypes.data, ctypes.byref(rows))
    assert rc == 0, lib.ptk_last_error()
    return offsets, pt._adopt(lib, rows, int(offsets[-1]), pt.NEIGHBOR)


# ---- CPU tier: the host loop on a host-only handle ------------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "self", "2d", "5d"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_equals_the_reference(kind, metric):
    c = case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    r = c.radii()
    for sort in (0, 1):
        off, flat = host_loop(tree, c.q, r, sort)
        check_rows(off, flat, c.rows(r, sort), sort, (kind, metric, sort))


@needs_reference
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_host_loop_of_the_topological_metrics(metric):
    rng = np.random.default_rng(12)
    dim = 1 if metric == "SO2" else 3
    p, q = rng.random((2_000, dim), dtype=np.float32), rng.random((400, dim), dtype=np.float32)
    c = Case(p, q, 8, metric)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE)
    r = c.radii()
    for sort in (0, 1):
        off, flat = host_loop(tree, c.q, r, sort)
        check_rows(off, flat, c.rows(r, sort), sort, (metric, sort))


def test_scalar_host_loop_is_the_per_row_loop_with_one_radius():
    """ptk_host_search_radius and ptk_host_search_radius_radii share one body: a constant array gives the scalar bytes."""
    p, q = ds.uniform_cloud(2_000, 3, 51), ds.uniform_cloud(300, 3, 52)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    for radius in (0.0, 0.004, INF):
        for sort in (0, 1):
            offsets = np.zeros(len(q) + 1, dtype=np.uint64)
            rows = ctypes.c_void_p()
            assert lib.ptk_host_search_radius(tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q), np.float32(radius),
                                              np.float32(1.0), sort, offsets.ctypes.data, ctypes.byref(rows)) == 0
            flat = pt._adopt(lib, rows, int(offsets[-1]), pt.NEIGHBOR)
            off2, flat2 = host_loop(tree, q, np.full(len(q), radius, dtype=np.float32), sort)
            assert np.array_equal(offsets, off2) and flat.tobytes() == flat2.tobytes(), (radius, sort)


def test_argument_checks():
    p, q = ds.uniform_cloud(50, 3, 21), ds.uniform_cloud(40, 3, 22)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    h, pp, qq, n = tree._h, tree._pts.ctypes.data, q.ctypes.data, len(q)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    good = np.full(n, 0.01, dtype=np.float32)
    oo, rr = offsets.ctypes.data, ctypes.byref(rows)
    # the host loop: null pointers
    assert lib.ptk_host_search_radius_radii(None, pp, qq, n, good.ctypes.data, 0, oo, rr) == -1
    assert lib.ptk_host_search_radius_radii(h, None, qq, n, good.ctypes.data, 0, oo, rr) == -1
    assert lib.ptk_host_search_radius_radii(h, pp, None, n, good.ctypes.data, 0, oo, rr) == -1
    assert lib.ptk_host_search_radius_radii(h, pp, qq, n, None, 0, oo, rr) == -1
    assert lib.ptk_host_search_radius_radii(h, pp, qq, n, good.ctypes.data, 0, None, rr) == -1
    assert lib.ptk_host_search_radius_radii(h, pp, qq, n, good.ctypes.data, 0, oo, None) == -1
    # a NaN and a negative entry: refused, and the first offending row is named
    for bad, row in ((float("nan"), 17), (-1.0, 5)):
        r = good.copy()
        r[row] = bad
        r[row + 9] = bad
        assert lib.ptk_host_search_radius_radii(h, pp, qq, n, r.ctypes.data, 0, oo, rr) == -1
        assert f"radii[{row}]" in lib.ptk_last_error().decode()
        assert not rows.value
    # +inf, FLT_MAX, 0 and a subnormal radius are valid entries
    r = good.copy()
    r[:4] = [INF, float(np.finfo(np.float32).max), 0.0, 1e-42]
    assert lib.ptk_host_search_radius_radii(h, pp, qq, n, r.ctypes.data, 0, oo, rr) == 0
    flat = pt._adopt(lib, rows, int(offsets[-1]), pt.NEIGHBOR)
    assert offsets[1] == 50 and offsets[2] == 100 and offsets[3] == 100 and len(flat) == offsets[-1]
    # an empty batch
    rows = ctypes.c_void_p()
    assert lib.ptk_host_search_radius_radii(h, pp, None, 0, None, 0, oo, ctypes.byref(rows)) == 0
    assert offsets[0] == 0
    lib.ptk_free(rows)
    # the device entry points: null pointers are invalid before anything else; a host-only handle has no device search
    rows = ctypes.c_void_p()
    rr = ctypes.byref(rows)
    assert lib.ptk_search_radius_radii(None, qq, n, good.ctypes.data, 0, oo, rr) == -1
    assert lib.ptk_search_radius_radii(h, qq, n, good.ctypes.data, 0, None, rr) == -1
    assert lib.ptk_search_radius_radii(h, qq, n, good.ctypes.data, 0, oo, None) == -1
    assert lib.ptk_search_radius_radii(h, qq, n, good.ctypes.data, 0, oo, rr) < 0 and not rows.value
    assert lib.ptk_search_radius_radii_fill_device(None, qq, n, good.ctypes.data, oo, None, 0, None) == -1
    assert lib.ptk_search_radius_radii_fill_device(h, qq, n, good.ctypes.data, oo, None, 0, None) < 0
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    q64, good64 = q.astype(np.float64), good.astype(np.float64)
    assert lib.ptk_search64_radius_radii(None, q64.ctypes.data, n, good64.ctypes.data, 0, oo, rr) == -1
    assert lib.ptk_search64_radius_radii(t64._h, q64.ctypes.data, n, good64.ctypes.data, 0, None, rr) == -1
    assert lib.ptk_search64_radius_radii(t64._h, q64.ctypes.data, n, good64.ctypes.data, 0, oo, rr) < 0 and not rows.value


def test_python_validation_on_a_host_only_handle():
    p, q = ds.uniform_cloud(100, 3, 23), ds.uniform_cloud(30, 3, 24)
    for dtype in (np.float32, np.float64):
        tree = pt.KdTree(p.astype(dtype), pt.Metric.L2Squared, 5, device=pt.PTK_DEVICE_NONE)
        qq = q.astype(dtype)
        for bad in (np.zeros(29), np.zeros(31), np.zeros((30, 1)), np.zeros((2, 15)), ["a"] * 30):
            with pytest.raises(ValueError):
                tree.search_radius(qq, bad)
        # the per-row form is exact: e may not be given, in either position the overload set takes it
        with pytest.raises(ValueError, match="e may not be given"):
            tree.search_radius(qq, np.full(30, 0.01), 1.0)
        with pytest.raises(ValueError, match="e may not be given"):
            tree.search_radius(qq, [0.01] * 30, 2.0, True)
        # a well-formed array passes the validation and reaches the library, which has no device here
        with pytest.raises(pt.PtkError):
            tree.search_radius(qq, [0.01] * 30)
        with pytest.raises(pt.PtkError):
            tree.search_radius(qq, np.full(30, 0.01, dtype=np.float64), sort=True)
    import pico_tree

    assert pico_tree.KdTree.search_radius is pt.KdTree.search_radius
    assert pico_tree.KdTree.search_radius_device is pt.KdTree.search_radius_device


# ---- CPU tier: the real kernel source in the emulator -----------------------------------------------------------------

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/cpp/emulate_radius_radii.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_radius_radii") / "libptk_emu_radius_radii.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_radius_radii.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    lib.emu_set_metric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.emu_radius_radii_count.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_radius_radii_fill.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


_EMU_METRIC = {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}


def poisoned(n):
    out = np.empty(n, dtype=pt.NEIGHBOR)
    out.view(np.uint32)[:] = 0xDEADBEEF
    return out


def lattice():
    """The lattice of tests/test_knn_within.py: point distances and box distances hit the integer radii exactly."""
    g = np.arange(0, 12, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g[:6], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = np.concatenate([p[::29], p[::31] + np.float32(0.5), p[::37] * np.float32([1, 1, 0])]).astype(np.float32)
    return p, q


def emu_case(kind, metric):
    """(case, radii): the lattice with integer radii mixed per row, the other clouds (200 queries) with the recipe."""
    key = ("emu", kind, metric)
    if key not in _cases:
        if kind == "lattice":
            p, q = lattice()
            _cases[key] = Case(p, q, 4, metric)
        else:
            p, q, leaf = cloud(kind)
            _cases[key] = Case(p, q[:200], leaf, metric)
    c = _cases[key]
    if kind == "lattice":
        return c, np.array([0.0, 1.0, 2.0, 3.0, 0.75, 4.0, INF], dtype=np.float32)[(np.arange(len(c.q)) * 3) % 7]
    return c, c.radii()


@needs_reference
@pytest.mark.parametrize("kind", ["lattice", "uniform", "ties"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_count_scan_fill_equal_the_reference(emu, kind, metric):
    c, r = emu_case(kind, metric)
    n = len(c.q)
    off, flat = c.rows(r)
    want_counts = np.diff(off.astype(np.int64))
    # rows with a NaN and a negative radius: count 0, and the fill writes nothing even where there is room
    bad = np.array([3, 64, n - 1])
    r_bad = r.copy()
    r_bad[bad] = [np.nan, -1.0, -INF]
    slack = np.zeros(n, dtype=np.int64)
    slack[bad] = 4
    host = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    nodes, idx, _, _ = host.flat()
    h = emu.emu_create(c.p.ctypes.data, len(c.p), c.p.shape[1], nodes.ctypes.data, len(nodes), idx.ctypes.data)
    assert h
    emu.emu_set_metric(h, _EMU_METRIC[metric])
    perm = np.random.default_rng(77).permutation(n).astype(np.uint32)  # (a launch order that is not the identity)
    try:
        for pm in (None, perm):
            pmp = None if pm is None else pm.ctypes.data
            for radii, room in ((r, np.zeros(n, dtype=np.int64)), (r_bad, slack)):
                counts = np.full(n, -7, dtype=np.int64)
                assert emu.emu_radius_radii_count(h, c.q.ctypes.data, pmp, n, radii.ctypes.data, counts.ctypes.data) == 0
                w = want_counts.copy()
                if radii is r_bad:
                    w[bad] = 0
                assert np.array_equal(counts, w), (kind, metric, pm is not None)
                # the scan (with room nobody may use behind the refused rows)
                offsets = np.zeros(n + 1, dtype=np.uint64)
                offsets[1:] = np.cumsum(counts + room)
                total = int(offsets[-1])
                out = poisoned(total + GUARD)
                expect = out.copy()
                for i in range(n):
                    if w[i]:
                        expect[int(offsets[i]):int(offsets[i]) + w[i]] = flat[int(off[i]):int(off[i + 1])]
                assert emu.emu_radius_radii_fill(h, c.q.ctypes.data, pmp, n, radii.ctypes.data, offsets.ctypes.data,
                                                 out.ctypes.data) == 0
                # rows, their order, the untouched room and the guard in one comparison; a kernel that indexes `radii`
                # or `offsets` by launch position fails under `perm`
                assert out.tobytes() == expect.tobytes(), (kind, metric, pm is not None, radii is r_bad)
    finally:
        emu.emu_destroy(h)


# ---- CPU tier: the C++ members (tests/cpp/radius_radii_main.cpp) ------------------------------------------------------

def _cpp_files(d):
    p, q = ds.uniform_cloud(20_000, 3, 91), ds.uniform_cloud(1_500, 3, 92)
    q[:40] = p[:40]  # queries exactly on tree points
    i = np.arange(len(q))
    r = np.array([0.0, 0.0004, 0.002, 1e-42, 0.01], dtype=np.float32)[i % 5]
    r[i % 97 == 5] = INF
    p.tofile(os.path.join(d, "points.bin"))
    q.tofile(os.path.join(d, "queries.bin"))
    r.tofile(os.path.join(d, "radii.bin"))


def test_cpp_batched_radii_members_equal_the_single_query_member(tmp_path):
    d = str(tmp_path)
    _cpp_files(d)
    exe = os.path.join(d, "radius_radii_main")
    subprocess.check_call(["g++", "-DPICO_TREE_HOST_ONLY", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "radius_radii_main.cpp"),
                           "-o", exe])
    res = subprocess.run([exe, d], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


# ---- gpu tier ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "self", "2d"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_rows_equal_the_reference(gpu, kind, metric):
    import torch

    full = 64 * 5 + 17
    c = case(kind, metric, nq=full)
    r = c.radii()
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    for nq in (64 * 5, full):  # (full wavefronts only; a partial last one)
        q, rq = np.ascontiguousarray(c.q[:nq]), np.ascontiguousarray(r[:nq])
        dq, dr = torch.from_numpy(q).to(f"cuda:{gpu}"), torch.from_numpy(rq).to(f"cuda:{gpu}")
        for sort in (False, True):
            want = prefix(c.rows(r, sort), nq)
            got = tree.search_radius(q, rq, sort=sort)
            check_rows(got.offsets, got.flat, want, sort, (kind, metric, nq, sort, "host form"))
            off, raw = tree.search_radius_device(dq, dr, sort=sort)
            check_rows(off.cpu().numpy(), raw_rows(raw), want, sort, (kind, metric, nq, sort, "torch"))


@pytest.mark.gpu
@needs_reference64
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_float64_device_rows_equal_the_reference(gpu, metric):
    p = ds.uniform_cloud(4_000, 3, 101).astype(np.float64) * 1.0000001
    q = ds.uniform_cloud(600, 3, 102).astype(np.float64) * 1.0000001
    c = Case(p, q, 10, metric, np.float64)
    tree = pt.KdTree(p, getattr(pt.Metric, metric), 10, device=gpu)
    r = c.radii()
    assert r.dtype == np.float64 and np.finfo(np.float64).max in r
    for sort in (False, True):
        got = tree.search_radius(c.q, r, sort=sort)
        # (float64 rows with sort: ties by index, so the rows are the reference's whenever its sort is stable in them --
        # the set comparison holds either way)
        check_rows(got.offsets, got.flat, c.rows(r, sort), sort, (metric, sort))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_constant_radii_array_gives_the_bytes_of_the_scalar_call(gpu, dtype):
    """The scalar call runs through the capture, the leaf lists and the cooperative search; the per-row call through none
    of them."""
    p, q = ds.uniform_cloud(6_000, 3, 41).astype(dtype), ds.uniform_cloud(3_000, 3, 42).astype(dtype)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    d1 = float(np.median(tree.search_knn(q, 1)["distance"]))
    for r in (0.0, d1, 8 * d1):
        want = tree.search_radius(q, r)
        got = tree.search_radius(q, np.full(len(q), r, dtype=dtype))
        assert np.array_equal(got.offsets, want.offsets), (dtype, r)
        assert np.array_equal(got.flat["index"], want.flat["index"]), (dtype, r)
        assert np.ascontiguousarray(got.flat["distance"]).tobytes() == \
            np.ascontiguousarray(want.flat["distance"]).tobytes(), (dtype, r)
        if dtype == np.float32:
            assert got.flat.tobytes() == want.flat.tobytes()
        assert (len(want.flat) > 0) == (r > 0)


@pytest.mark.gpu
@needs_reference
def test_batch_order_does_not_change_a_row(gpu):
    import torch

    p, q = ds.uniform_cloud(20_000, 3, 31), ds.uniform_cloud(12_000, 3, 32)  # (12 000 > 8 192: REORDER_AUTO sorts)
    c = Case(p, q, 10, "L2Squared")
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    r = c.radii(finite_only=True)  # (the finite values: the rows of the reference stay small)
    want = c.rows(r)
    dq, dr = torch.from_numpy(c.q).to(f"cuda:{gpu}"), torch.from_numpy(r).to(f"cuda:{gpu}")
    for mode in (pt.REORDER_ON, pt.REORDER_OFF, pt.REORDER_AUTO):
        tree.set_reorder(mode)
        got = tree.search_radius(c.q, r)
        check_rows(got.offsets, got.flat, want, False, mode)
        off, raw = tree.search_radius_device(dq, dr)
        check_rows(off.cpu().numpy(), raw_rows(raw), want, False, (mode, "torch"))


@pytest.mark.gpu
def test_device_form_with_a_nan_and_a_negative_radius(gpu):
    import torch

    p, q = ds.uniform_cloud(3_000, 3, 1), ds.uniform_cloud(200, 3, 2)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    d1 = float(np.median(tree.search_knn(q, 1)["distance"]))
    good = hashed(len(q), [0.0, d1, 4 * d1, 30 * d1, INF])
    good[37], good[101] = 4 * d1, 30 * d1
    empty = good.copy()
    empty[[37, 101]] = 0.0  # (what the refused rows must look like: empty, every other row as it is)
    bad = good.copy()
    bad[37], bad[101] = np.nan, -1.0
    dev = f"cuda:{gpu}"
    dq = torch.from_numpy(q).to(dev)
    lib = pt._load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for sort in (0, 1):
        want_off, want_raw = tree.search_radius_device(dq, torch.from_numpy(empty).to(dev), sort=bool(sort))
        assert int(want_off[38] - want_off[37]) == 0 and int(want_off[102] - want_off[101]) == 0
        with_rows = tree.search_radius_device(dq, torch.from_numpy(good).to(dev))[0]
        assert int(with_rows[38] - with_rows[37]) > 0 and int(with_rows[102] - with_rows[101]) > 0
        # the C entry points themselves, with a poisoned guard behind the rows
        dr = torch.from_numpy(bad).to(dev)
        counts = torch.zeros(len(q) + 1, dtype=torch.int64, device=dev)
        assert lib.ptk_search_count_within_radii_device(tree._h, dq.data_ptr(), len(q), dr.data_ptr(), 0, counts.data_ptr(),
                                                        stream) == 0
        offsets = torch.zeros(len(q) + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts[:len(q)], 0)
        assert torch.equal(offsets, want_off)
        total = int(offsets[-1])
        out = torch.full((total + GUARD, 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        assert lib.ptk_search_radius_radii_fill_device(tree._h, dq.data_ptr(), len(q), dr.data_ptr(), offsets.data_ptr(),
                                                       out.data_ptr(), sort, stream) == 0  # (PTK_OK)
        torch.cuda.synchronize()
        assert torch.equal(out[:total], want_raw), sort
        assert bool((out[total:] == 0x5A5A5A5A).all()), sort
    # the host-buffer form scans the values: refused, the first such row named
    with pytest.raises(pt.PtkError) as invalid:
        tree.search_radius(q, bad)
    assert invalid.value.status == -1 and "radii[37]" in str(invalid.value)


@pytest.mark.gpu
def test_a_per_row_call_leaves_the_radius_capture_alone(gpu):
    """tests/test_count_within.py::test_count_within_leaves_the_radius_capture_alone with a per-row radius search between
    the scalar count pass and its fill pass."""
    import torch

    lib = pt._load()
    p, q = ds.lidar_cloud(200_000, seed=95), ds.lidar_cloud(50_000, seed=96, pose=(1.0, 0.5))
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    dev = f"cuda:{gpu}"
    dq = torch.from_numpy(q).to(dev)
    nq, r = len(q), np.float32(1.0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    prof = pt._Profile()
    assert lib.ptk_profile_enable(tree._h, 1) == 0
    other_radii = torch.from_numpy(hashed(nq, [0.0, 0.25, 2.0])).to(dev)
    rows, coop = {}, {}
    for with_call in (False, True):
        counts = torch.zeros(nq, dtype=torch.int64, device=dev)
        assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), nq, r, np.float32(1.0), counts.data_ptr(),
                                                  stream) == 0
        offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        total = int(offsets[-1])
        out = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
        if with_call:  # (the same batch pointer, other radii; and another batch pointer)
            off_a, raw_a = tree.search_radius_device(dq, other_radii)
            off_b, raw_b = tree.search_radius_device(dq.clone(), other_radii, sort=True)
            assert torch.equal(off_a, off_b) and int(off_a[-1]) > 0
        torch.cuda.synchronize()
        assert lib.ptk_profile_get(tree._h, ctypes.byref(prof), 1) == 0  # (reset)
        assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), nq, r, np.float32(1.0), offsets.data_ptr(),
                                                 out.data_ptr(), 1, stream) == 0
        torch.cuda.synchronize()
        assert lib.ptk_profile_get(tree._h, ctypes.byref(prof), 1) == 0
        assert int(prof.queries) == 0, (with_call, int(prof.queries))  # served from the capture: nothing searched again
        rows[with_call] = out[:total].cpu().numpy().tobytes()
        coop[with_call] = tree.radius_coop_counts()
    assert rows[True] == rows[False]
    assert coop[True] == coop[False]


@pytest.mark.gpu
def test_side_stream(gpu):
    import torch

    p, q = ds.uniform_cloud(10_000, 3, 71), ds.uniform_cloud(4_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    r = hashed(len(q), [0.0, 0.0005, 0.002, 0.01, 0.05])
    want = tree.search_radius(q, r)
    want_sorted = tree.search_radius(q, r, sort=True)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        dq = torch.from_numpy(q).to(f"cuda:{gpu}", non_blocking=False)
        dr = torch.from_numpy(r).to(f"cuda:{gpu}", non_blocking=False) * 1.0  # (made by a kernel of this stream)
        off, raw = tree.search_radius_device(dq, dr)
        off_s, raw_s = tree.search_radius_device(dq, dr, sort=True)
    side.synchronize()
    assert np.array_equal(off.cpu().numpy().astype(np.uint64), want.offsets)
    assert raw_rows(raw).tobytes() == want.flat.tobytes()
    assert np.array_equal(off_s.cpu().numpy().astype(np.uint64), want_sorted.offsets)
    assert raw_rows(raw_s)["distance"].tobytes() == np.ascontiguousarray(want_sorted.flat["distance"]).tobytes()
    # CUDA queries: radii on the host, of the wrong dtype, length or shape, and an e, are refused before any library call
    for bad in (r, torch.from_numpy(r), dr.double(), dr[:-1], dr.reshape(-1, 1)):
        with pytest.raises(ValueError):
            tree.search_radius_device(dq, bad)
    with pytest.raises(ValueError, match="e may not be given"):
        tree.search_radius_device(dq, dr, 1.0)
    with pytest.raises(ValueError):
        tree.search_radius(q, dr)  # (host queries take host radii)


def _refused_then_served(tree, c, r):
    """Refused by the device with PTK_ERR_UNSUPPORTED, served by the host loop when allowed."""
    with pytest.raises(pt.PtkError) as refused:
        tree.search_radius(c.q, r)
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED == -2
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got = tree.search_radius(c.q, r)
            got_sorted = tree.search_radius(c.q, r, sort=True)
    finally:
        pt.allow_host_loop(False)
    check_rows(got.offsets, got.flat, c.rows(r), False, "host loop")
    check_rows(got_sorted.offsets, got_sorted.flat, c.rows(r, True), True, "host loop, sorted")


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["5d", "se2", "deep"])
def test_handles_the_device_refuses(gpu, kind):
    import torch

    if kind == "5d":
        c = case("5d", "L2Squared")
        metric = pt.Metric.L2Squared
        r = c.radii()
    elif kind == "se2":
        rng = np.random.default_rng(3)
        c = Case(rng.random((2_000, 3), dtype=np.float32), rng.random((400, 3), dtype=np.float32), 8, "SE2Squared")
        metric = pt.Metric.SE2Squared
        r = c.radii()
    else:  # (the cloud of tests/test_within_radii.py::test_deep_tree)
        pts = np.concatenate([ds.uniform_cloud(60_000, 3, 31) - np.float32(0.5), np.zeros((1_500, 3), np.float32)])
        q = np.concatenate([ds.uniform_cloud(400, 3, 32) - np.float32(0.5), np.zeros((3, 3), np.float32)])
        c = Case(pts, q, 10, "L2Squared")
        metric = pt.Metric.L2Squared
        r = c.radii(finite_only=True)
    tree = pt.KdTree(c.p, metric, c.leaf, device=gpu)
    if kind == "deep":
        assert tree.info()["max_depth"] > 1_040
    _refused_then_served(tree, c, r)
    # the device form is refused through the same check
    dq, dr = torch.from_numpy(c.q).to(f"cuda:{gpu}"), torch.from_numpy(r).to(f"cuda:{gpu}")
    with pytest.raises(pt.PtkError) as refused:
        tree.search_radius_device(dq, dr)
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
    message = str(refused.value)
    with pytest.raises(pt.PtkError) as refused:
        tree.count_within(dq, dr)
    assert str(refused.value) == message  # (check_count_within_radii: the same messages)
    lib = pt._load()
    offsets = torch.zeros(len(c.q) + 1, dtype=torch.int64, device=dq.device)
    assert lib.ptk_search_radius_radii_fill_device(tree._h, dq.data_ptr(), len(c.q), dr.data_ptr(), offsets.data_ptr(), None,
                                                   0, torch.cuda.current_stream(dq.device).cuda_stream) == -2
    assert lib.ptk_last_error().decode() in message
