"""aggregate_within_self / aggregate_within: pool a caller's per-point values over radius neighbourhoods (ptk.h,
DESIGN.md §2, §4.1 K21).

Expected values are the contract folded in numpy float32 (``fold``: vectorised over rows, sequential over the rank inside
a row, one float32 operation per step; the compare-selects written out with ``np.where``) over rows the project already
trusts: the ``(offsets, flat)`` of the library's host row loops ``ptk_host_search_radius`` / ``_radii`` (for the self
forms over the points themselves, the own entries removed).  They never come from the code under test.  Everything is
compared bit for bit.

The CPU tier runs the host loops on host-only handles, the real kernel source of both kernels in the emulator
(tests/cpp/emulate_aggregate.cpp: the launch layer's own channel windows and vector-path choice), the C++ members
(tests/cpp/aggregate_main.cpp, -DPICO_TREE_HOST_ONLY under -fsanitize=address,undefined) and the argument checks; the gpu
tier the device forms.
"""

from __future__ import annotations

import ctypes
import functools
import os
import subprocess
import warnings

import numpy as np
import pytest

import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import depth_cases, leaf_cases
from tests.test_radius_self import cloud, without_self

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")
FLT_MAX = F32(np.finfo(np.float32).max)
METRICS = ["L2Squared", "L1", "LPInf", "LNInf"]
KINDS = ["uniform", "lidar", "ties", "small"]
_EMU_METRIC = {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}
_CPP_METRIC = {"L2Squared": "l2", "L1": "l1", "LPInf": "lpinf", "LNInf": "lninf"}
OPS = {"sum": 0, "min": 1, "max": 2}
INCLUDE_SELF = 0x100
INVALID, UNSUPPORTED, DEVICE = -1, -2, -3
#: the accumulators a lane holds (ptk_kernels_aggregate.hpp: kAggWidth); the emulator library reports the compiled value
#: and test_the_width_is_the_documented_one holds the two together
W = 8
CHANNELS = [1, 3, 4, W - 1, W, W + 1, 2 * W + 1]
MARK = 0xA5


# ---- the contract in numpy ------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_numbers(a, b):
    """same(), but any NaN equals any NaN: which NaN an addition gives (sign, payload) is the processor's, not IEEE's --
    inf - inf is 0xFFC00000 on x86 and 0x7FC00000 on the GPU.  (A NaN under max / min is a copy: same() holds there.)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def fold(values, off, flat, op, own=None, reverse=False):
    """out[n, channels] of the rows (off, flat): per channel, in row order (``reverse``: from the row's last entry to its
    first), one float32 operation per entry.  ``own``: the starting accumulators (INCLUDE_SELF), default the identity."""
    values = np.asarray(values)
    assert values.dtype == np.float32 and values.ndim == 2
    off = np.asarray(off).astype(np.int64)
    n, cnt = len(off) - 1, np.diff(off)
    idx = np.asarray(flat["index"]).astype(np.int64)
    if own is not None:
        acc = np.array(own, dtype=np.float32, copy=True)
    else:
        acc = np.full((n, values.shape[1]), {"sum": 0.0, "max": -INF, "min": INF}[op], dtype=np.float32)
    with np.errstate(all="ignore"):
        for t in range(int(cnt.max(initial=0))):
            rows = np.flatnonzero(cnt > t)
            at = off[rows] + (cnt[rows] - 1 - t if reverse else t)
            v, a = values[idx[at]], acc[rows]
            if op == "sum":
                new = a + v
            elif op == "max":
                new = np.where(v > a, v, a)
            else:
                new = np.where(v < a, v, a)
            assert new.dtype == np.float32
            acc[rows] = new
    return acc


def spread_values(n, channels, seed):
    """Magnitudes spread over many binades, mixed signs: a float32 sum of them depends on its order."""
    rng = np.random.default_rng(seed)
    m = (1.0 + rng.random((n, channels))) * np.exp2(rng.integers(-20, 21, (n, channels)))
    return np.ascontiguousarray((m * np.where(rng.random((n, channels)) < 0.5, -1.0, 1.0)).astype(np.float32))


def search_rows(tree, p, q, r):
    """(offsets, flat) of ptk_host_search_radius / _radii of the rows q, unsorted, e = 1."""
    lib = pt._load()
    p, q = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32)
    off = np.zeros(len(q) + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    if np.ndim(r) == 0:
        rc = lib.ptk_host_search_radius(tree._h, p.ctypes.data, q.ctypes.data, len(q), F32(r), F32(1), 0, off.ctypes.data,
                                        ctypes.byref(rows))
    else:
        r = np.ascontiguousarray(r, dtype=np.float32)
        rc = lib.ptk_host_search_radius_radii(tree._h, p.ctypes.data, q.ctypes.data, len(q), r.ctypes.data, 0,
                                              off.ctypes.data, ctypes.byref(rows))
    assert rc == 0, lib.ptk_last_error()
    return off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR)


def self_rows(tree, p, r):
    """The same over the points themselves, the own entries removed (test_normals_self.py::host_search_rows)."""
    return without_self(*search_rows(tree, p, p, r))


def host_tree(p, leaf, metric):
    return pt.KdTree(np.ascontiguousarray(p), getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)


def kth_distance(tree, p, k=8):
    """The distance of each point's k-th nearest OTHER point (ptk_host_search_knn_self)."""
    out = np.zeros((len(p), k), dtype=pt.NEIGHBOR)
    assert pt._load().ptk_host_search_knn_self(tree._h, p.ctypes.data, k, out.ctypes.data) == 0
    return np.ascontiguousarray(out["distance"][:, k - 1])


class Case:
    """A cloud, its host-only tree, its radii, a query batch with its radii, and the rows of each: computed once."""

    def __init__(self, kind, metric):
        self.kind, self.metric = kind, metric
        self.p, self.leaf = cloud(kind)
        self.n = len(self.p)
        self.tree = host_tree(self.p, self.leaf, metric)
        kth = kth_distance(self.tree, self.p)
        med = F32(np.median(kth))
        self.scalars = [F32(0), med, F32(4) * med]
        if kind == "ties":  # the grid step exactly (neighbours AT r stay out) and the next number above it
            step = F32(0.125 * 0.125) if metric == "L2Squared" else F32(0.125)
            self.scalars += [step, np.nextafter(step, F32(np.inf))]
        if kind == "small":  # whole-tree rows
            self.scalars += [F32(10.0), F32(np.inf), FLT_MAX]
        r = kth.copy()
        r[5::97] = 0
        r[11::211] = np.finfo(np.float32).smallest_subnormal
        r[17::701] = np.inf
        r[23::997] = FLT_MAX
        self.radii = r
        # the query batch: points of the tree (zero distances) and points beside them, shuffled; one radius each
        rng = np.random.default_rng(1234)
        nq = min(1500, self.n)
        take = rng.permutation(self.n)[:nq]
        q = self.p[take].copy()
        q[nq // 3:] += (rng.random((nq - nq // 3, 3)) - 0.5).astype(np.float32) * F32(0.02)
        self.q = np.ascontiguousarray(q[rng.permutation(nq)], dtype=np.float32)
        qr = (kth[take] * F32(2)).astype(np.float32)
        qr[3::89] = 0
        qr[7::301] = np.inf
        self.qradii = np.ascontiguousarray(qr)
        self.launch = np.ascontiguousarray(rng.permutation(nq).astype(np.uint32))  # a launch order of the emulator
        self._rows = {}

    def sources(self):
        """[(name, radius or radii)] of the self forms."""
        return [(f"r{i}", r) for i, r in enumerate(self.scalars)] + [("per row", self.radii)]

    def qsources(self):
        return [("scalar", self.scalars[2] if self.scalars[2] > 0 else self.scalars[-1]), ("per row", self.qradii)]

    def rows(self, name, r):
        key = ("self", name)
        if key not in self._rows:
            self._rows[key] = self_rows(self.tree, self.p, r)
        return self._rows[key]

    def qrows(self, name, r):
        key = ("query", name)
        if key not in self._rows:
            self._rows[key] = search_rows(self.tree, self.p, self.q, r)
        return self._rows[key]


@functools.lru_cache(maxsize=None)
def case(kind, metric):
    return Case(kind, metric)


# ---- calling the forms: placed buffers, markers, guards --------------------------------------------------------------------

def placed(shape, offset, fill=None):
    """A float32 array of `shape` whose first byte lies at 16 k (+ 4 with `offset`), inside a buffer of MARK bytes: (buffer,
    array).  `fill`: copied in."""
    count = int(np.prod(shape))
    buf = np.empty(count + 16, dtype=np.float32)
    buf.view(np.uint8)[:] = MARK
    at = (-buf.ctypes.data % 16) // 4 + 4 + (1 if offset else 0)
    arr = buf[at:at + count].reshape(shape)
    assert arr.ctypes.data % 16 == (4 if offset else 0)
    if fill is not None:
        arr[...] = fill
    return buf, arr


def guards_intact(buf, arr):
    raw = buf.view(np.uint8)
    lo = arr.ctypes.data - buf.ctypes.data
    return bool(np.all(raw[:lo] == MARK) and np.all(raw[lo + arr.nbytes:] == MARK))


def call(fn, lead, rows, r, values, op, inc=False, counts=True, offset=False, status=0):
    """fn(*lead, radius, radii, values, channels, op, out, counts) with `values` and `out` placed at 16 k (+ 4), `out` and
    `counts` pre-filled with a marker.  Returns (out, counts or None)."""
    values = np.asarray(values, dtype=np.float32)
    channels = values.shape[1]
    _, v = placed(values.shape, offset, values)
    obuf, out = placed((rows, channels), offset)
    cnt = np.full(rows, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    scalar = np.ndim(r) == 0
    radii = None if scalar else np.ascontiguousarray(r, dtype=np.float32)
    rc = fn(*lead, F32(r if scalar else 0), None if scalar else radii.ctypes.data, v.ctypes.data, channels,
            OPS[op] | (INCLUDE_SELF if inc else 0), out.ctypes.data, cnt.ctypes.data if counts else None)
    assert rc == status, (rc, pt._load().ptk_last_error())
    assert guards_intact(obuf, out), "a write outside the output"
    if status == 0:
        assert not np.any(bits(out) == 0xA5A5A5A5), "an entry of out was not written"
        assert not counts or not np.any(cnt == 0xA5A5A5A5A5A5A5A5), "a count was not written"
    return out.copy(), (cnt.astype(np.int64) if counts else None)


def host_self(tree, p, r, values, op, **kw):
    return call(pt._load().ptk_host_aggregate_within_self, (tree._h, p.ctypes.data), len(p), r, values, op, **kw)


def host_within(tree, p, q, r, values, op, **kw):
    return call(pt._load().ptk_host_aggregate_within, (tree._h, p.ctypes.data, q.ctypes.data, len(q)), len(q), r, values, op,
                **kw)


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/cpp/emulate_aggregate.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_aggregate") / "libptk_emu_aggregate.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "cpp"),
        os.path.join(ROOT, "tests", "cpp", "emulate_aggregate.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    lib.emu_create.restype = vp
    lib.emu_create.argtypes = [vp, u64, u32, vp, u64, vp]
    lib.emu_destroy.argtypes = [vp]
    lib.emu_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu_aggregate_self.argtypes = [vp, u64, ctypes.c_float, vp, vp, u32, u32, vp, vp]
    lib.emu_aggregate_within.argtypes = [vp, vp, vp, u64, ctypes.c_float, vp, vp, u32, u32, vp, vp]
    lib.emu_aggregate_vector_path.argtypes = [vp, vp, u32]
    return lib


class Emulated:
    """Both kernels over a tree built by the product's host builder over `tree_points` (default: the points)."""

    def __init__(self, lib, p, leaf, metric, tree_points=None):
        self.lib, self.p = lib, np.ascontiguousarray(p, dtype=np.float32)
        self.host = host_tree(self.p if tree_points is None else tree_points, leaf, metric)
        nodes, self.idx, _, _ = self.host.flat()
        self.n = len(self.p)
        self.h = lib.emu_create(self.p.ctypes.data, self.n, self.p.shape[1], nodes.ctypes.data, len(nodes), self.idx.ctypes.data)
        assert self.h
        lib.emu_set_metric(self.h, _EMU_METRIC[metric])

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.emu_destroy(self.h)
            self.h = None

    def self_form(self, r, values, op, piece=0, **kw):
        return call(self.lib.emu_aggregate_self, (self.h, piece), self.n, r, values, op, **kw)

    def within(self, q, r, values, op, perm=None, **kw):
        lead = (self.h, q.ctypes.data, None if perm is None else perm.ctypes.data, len(q))
        return call(self.lib.emu_aggregate_within, lead, len(q), r, values, op, **kw)


def lengths(off):
    return np.diff(np.asarray(off).astype(np.int64))


# ---- CPU tier ----------------------------------------------------------------------------------------------------------

def test_the_width_is_the_documented_one(emu_lib):
    assert emu_lib.emu_aggregate_width() == W


def test_the_order_of_a_sum_shows_in_its_bits():
    """Not vacuous: on the rows the order tests run over, the same fold from the other end of each row differs in bits for
    at least a quarter of the rows that have three entries or more (two entries commute)."""
    for kind, metric in (("uniform", "L2Squared"), ("lidar", "L1"), ("ties", "LPInf"), ("small", "LNInf")):
        c = case(kind, metric)
        name, r = c.sources()[2]
        off, flat = c.rows(name, r)
        values = spread_values(c.n, 2, 7)
        forward, backward = fold(values, off, flat, "sum"), fold(values, off, flat, "sum", reverse=True)
        long = lengths(off) >= 3
        differs = (bits(forward) != bits(backward)).any(1)
        assert long.sum() >= 100 and differs[long].sum() >= long.sum() / 4, (kind, metric, int(long.sum()), int(differs.sum()))
        # max and min do not depend on the order where no NaN or signed zero is about
        assert same(fold(values, off, flat, "max"), fold(values, off, flat, "max", reverse=True))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric", METRICS)
def test_host_loops_and_emulated_kernels(emu_lib, kind, metric):
    """Both host loops and both kernels (launches of 1 000 positions and of the whole tree; a shuffled launch order of
    the query rows), scalar and per-row radii, the three ops, with and without the own value: the fold, bit for bit;
    the counts the row lengths, which the count loops give as well."""
    c = case(kind, metric)
    emu = Emulated(emu_lib, c.p, c.leaf, metric)
    values = spread_values(c.n, 2, 11)
    lib = pt._load()
    nonempty = 0
    for turn, (name, r) in enumerate(c.sources()):
        off, flat = c.rows(name, r)
        cnt = lengths(off)
        nonempty += int(cnt.sum())
        host_counts = np.zeros(c.n, dtype=np.int64)
        scalar = np.ndim(r) == 0
        assert lib.ptk_host_search_count_within_self(c.tree._h, c.p.ctypes.data, F32(r if scalar else 0),
                                                     None if scalar else r.ctypes.data, 0, host_counts.ctypes.data) == 0
        assert np.array_equal(host_counts, cnt)
        for op in OPS:
            for inc in (False, True):
                want = fold(values, off, flat, op, own=values if inc else None)
                what = (kind, metric, name, op, inc)
                got, got_cnt = host_self(c.tree, c.p, r, values, op, inc=inc)
                assert same(got, want) and np.array_equal(got_cnt, cnt), what
                piece = 1000 if (turn + inc) % 2 else 0
                got, got_cnt = emu.self_form(r, values, op, piece=piece, inc=inc)
                assert same(got, want) and np.array_equal(got_cnt, cnt), what
        if scalar and r == 0:
            assert not cnt.any()
            assert np.all(host_self(c.tree, c.p, r, values, "max")[0] == -INF)
            assert np.all(host_self(c.tree, c.p, r, values, "min")[0] == INF)
            assert not bits(host_self(c.tree, c.p, r, values, "sum")[0]).any()
    assert nonempty > 0
    for name, r in c.qsources():
        off, flat = c.qrows(name, r)
        cnt = lengths(off)
        assert cnt.sum() > 0
        for op in OPS:
            want = fold(values, off, flat, op)
            what = (kind, metric, "query", name, op)
            got, got_cnt = host_within(c.tree, c.p, c.q, r, values, op)
            assert same(got, want) and np.array_equal(got_cnt, cnt), what
            got, got_cnt = emu.within(c.q, r, values, op, perm=c.launch if op != "min" else None)
            assert same(got, want) and np.array_equal(got_cnt, cnt), what


@pytest.mark.parametrize("channels", CHANNELS)
def test_channel_counts_alignment_and_columns(emu_lib, channels):
    """1, 3, 4, W - 1, W, W + 1 and 2 W + 1 channels, 16-byte aligned and offset by one float: the vector path, the scalar
    path and the run-time width of the last window.  No column leaks into another."""
    c = case("uniform", "L2Squared")
    emu = Emulated(emu_lib, c.p, c.leaf, "L2Squared")
    name, r = c.sources()[2]
    off, flat = c.rows(name, r)
    qoff, qflat = c.qrows("per row", c.qradii)
    values = spread_values(c.n, channels, 100 + channels)
    for offset in (False, True):
        _, v = placed(values.shape, offset, values)
        _, o = placed(values.shape, offset)
        assert emu_lib.emu_aggregate_vector_path(v.ctypes.data, o.ctypes.data, channels) == (channels % 4 == 0 and not offset)
        for op, inc in (("sum", False), ("max", True)):
            want = fold(values, off, flat, op, own=values if inc else None)
            got, cnt = emu.self_form(r, values, op, piece=1000, inc=inc, offset=offset)
            assert same(got, want) and np.array_equal(cnt, lengths(off)), (channels, offset, op)
            assert same(host_self(c.tree, c.p, r, values, op, inc=inc, offset=offset)[0], want)
        want = fold(values, qoff, qflat, "sum")
        got, cnt = emu.within(c.q, c.qradii, values, "sum", perm=c.launch, offset=offset)
        assert same(got, want) and np.array_equal(cnt, lengths(qoff)), (channels, offset, "query")
        assert same(host_within(c.tree, c.p, c.q, c.qradii, values, "sum", offset=offset)[0], want)
    # one column changed: every other column of the result stays
    base = emu.self_form(r, values, "sum")[0]
    for col in sorted({0, channels // 2, channels - 1}):
        other = values.copy()
        other[:, col] = spread_values(c.n, 1, 999)[:, 0]
        got = emu.self_form(r, other, "sum")[0]
        keep = np.arange(channels) != col
        assert same(got[:, keep], base[:, keep]) and not same(got[:, col], base[:, col]), (channels, col)
        assert same(got, fold(other, off, flat, "sum"))


def test_written_bytes_and_repeated_calls(emu_lib):
    """Every entry of `out` is written (the marker check of call()), counts = NULL is accepted, two calls give identical
    bytes."""
    c = case("lidar", "L2Squared")
    emu = Emulated(emu_lib, c.p, c.leaf, "L2Squared")
    values = spread_values(c.n, W + 1, 5)
    off, flat = c.rows("per row", c.radii)
    want = fold(values, off, flat, "sum")
    for run in (lambda **kw: emu.self_form(c.radii, values, "sum", **kw),
                lambda **kw: host_self(c.tree, c.p, c.radii, values, "sum", **kw)):
        a, ca = run()
        b, cb = run(counts=False)
        again, _ = run()
        assert cb is None and same(a, want) and same(b, want) and same(again, a) and np.array_equal(ca, lengths(off))
    qoff, qflat = c.qrows("per row", c.qradii)
    for run in (lambda **kw: emu.within(c.q, c.qradii, values, "max", **kw),
                lambda **kw: host_within(c.tree, c.p, c.q, c.qradii, values, "max", **kw)):
        a, _ = run()
        b, cb = run(counts=False)
        assert cb is None and same(a, fold(values, qoff, qflat, "max")) and same(a, b) and same(run()[0], a)


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_self_kernel_where_the_leaf_scan_changes(emu_lib, L):
    """A tree whose largest leaf has exactly 31 | 32 | 33 and 64 | 65 points (tests/leaf_cases.py)."""
    pts, blob, q, nb, ref, radii = leaf_cases.case(L)
    pts = np.asarray(pts)
    emu = Emulated(emu_lib, pts, L, "L2Squared")
    leaf_cases.assert_leaf(emu.host, L)
    values = spread_values(len(pts), 3, L)
    for r in leaf_cases.self_radii(L, radii):
        off, flat = self_rows(emu.host, pts, r)
        for op in OPS:
            want = fold(values, off, flat, op)
            got, cnt = emu.self_form(F32(r), values, op, piece=1000 if op == "sum" else 0)
            assert same(got, want) and np.array_equal(cnt, lengths(off)), (L, r, op)
        if r == radii[1]:  # (r_all: every blob point's row is the rest of the blob)
            assert np.all(lengths(off)[-L:] >= L - 1)


@pytest.mark.parametrize("depth", [39, 40, 135, 136])
def test_emulated_self_kernel_where_the_stack_class_changes(emu_lib, depth):
    pts = np.asarray(depth_cases.cloud_at_depth(depth, 3, 10)[0])
    emu = Emulated(emu_lib, pts, 10, "L2Squared")
    off, flat = self_rows(emu.host, pts, 0.05)
    assert np.all(lengths(off)[3_000:] == len(pts) - 3_001)
    values = spread_values(len(pts), 2, depth)
    run = depth_cases.Watch(depth, emu_lib)
    got, cnt = run(emu.self_form, F32(0.05), values, "sum", inc=True)
    assert same(got, fold(values, off, flat, "sum", own=values)) and np.array_equal(cnt, lengths(off)), depth
    assert same(host_self(emu.host, pts, 0.05, values, "sum", inc=True)[0], got)


def special_values(n, seed):
    """NaN, +-inf, +-0 and ordinary numbers; column 0 is all signed zeros, column 1 all NaN."""
    rng = np.random.default_rng(seed)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.25, 3e38, -3e38, 1e-45], dtype=np.float32)
    v = pool[rng.integers(0, len(pool), (n, 4))]
    v[:, 0] = np.where(rng.random(n) < 0.5, F32(-0.0), F32(0.0))
    v[:, 1] = np.nan
    return np.ascontiguousarray(v)


def test_special_values(emu_lib):
    """NaN, +-inf and signed zeros fold as the formulas read: a NaN value never replaces an accumulator, of -0 and +0 the
    first seen stays, and a NaN own value with INCLUDE_SELF stays NaN under max and min."""
    c = case("small", "L2Squared")
    emu = Emulated(emu_lib, c.p, c.leaf, "L2Squared")
    values = special_values(c.n, 3)
    name, r = c.sources()[2]
    off, flat = c.rows(name, r)
    busy = lengths(off) >= 2
    assert busy.sum() > 100
    for op in OPS:
        for inc in (False, True):
            want = fold(values, off, flat, op, own=values if inc else None)
            eq = same_numbers if op == "sum" else same
            assert eq(host_self(c.tree, c.p, r, values, op, inc=inc)[0], want), (op, inc)
            assert eq(emu.self_form(r, values, op, inc=inc)[0], want), (op, inc)
            if op != "sum":  # written out, not only through fold()
                assert np.all(np.isnan(want[:, 1]) == inc)  # (all-NaN column: the identity survives; a NaN own value stays)
                first = values[flat["index"][np.asarray(off[:-1], dtype=np.int64)[busy]], 0]
                if not inc:  # the zeros column: the first zero seen stays, whatever its sign
                    assert np.array_equal(np.signbit(want[busy, 0]), np.signbit(first))
                else:
                    assert np.array_equal(np.signbit(want[:, 0]), np.signbit(values[:, 0]))
    qoff, qflat = c.qrows("per row", c.qradii)
    for op in OPS:
        want = fold(values, qoff, qflat, op)
        eq = same_numbers if op == "sum" else same
        assert eq(host_within(c.tree, c.p, c.q, c.qradii, values, op)[0], want)
        assert eq(emu.within(c.q, c.qradii, values, op, perm=c.launch)[0], want)


def test_emulated_per_row_radii_that_pass_no_test(emu_lib):
    """A NaN and a negative radii entry (the _device forms cannot look): the identity -- or the own value -- and count 0,
    every other row unchanged.  Radius 0, +inf and FLT_MAX are valid."""
    c = case("small", "L2Squared")
    emu = Emulated(emu_lib, c.p, c.leaf, "L2Squared")
    values = spread_values(c.n, 3, 9)
    radii = np.full(c.n, 0.02, dtype=np.float32)
    radii[10], radii[20], radii[30] = 0.0, np.inf, FLT_MAX
    off, flat = self_rows(c.tree, c.p, radii)
    assert lengths(off)[10] == 0 and lengths(off)[20] == c.n - 1 and lengths(off)[30] == c.n - 1
    bad = radii.copy()
    bad[100], bad[200] = np.nan, -1.0
    keep = np.ones(c.n, dtype=bool)
    keep[[100, 200]] = False
    assert lengths(off)[100] > 0 and lengths(off)[200] > 0
    for op, identity in (("sum", 0.0), ("min", INF), ("max", -INF)):
        want = fold(values, off, flat, op)
        got, cnt = emu.self_form(radii, values, op)
        assert same(got, want)
        got, cnt = emu.self_form(bad, values, op, piece=256)
        assert same(got[keep], want[keep]) and np.array_equal(cnt[keep], lengths(off)[keep])
        assert same(got[~keep], np.full((2, 3), identity, dtype=np.float32)) and not cnt[~keep].any()
        got, cnt = emu.self_form(bad, values, op, inc=True)
        assert same(got[~keep], values[~keep]) and not cnt[~keep].any()
    qr = np.full(len(c.q), 0.02, dtype=np.float32)
    qoff, qflat = search_rows(c.tree, c.p, c.q, qr)
    qbad = qr.copy()
    qbad[5], qbad[50] = np.nan, -INF
    qkeep = np.ones(len(c.q), dtype=bool)
    qkeep[[5, 50]] = False
    got, cnt = emu.within(c.q, qbad, values, "max", perm=c.launch)
    want = fold(values, qoff, qflat, "max")
    assert same(got[qkeep], want[qkeep]) and np.all(got[~qkeep] == -INF) and not cnt[~qkeep].any()
    # the host-buffer forms and the host loops refuse such an entry by its row
    host_self(c.tree, c.p, bad, values, "sum", status=INVALID)
    assert "radii[100]" in pt._load().ptk_last_error().decode()
    host_within(c.tree, c.p, c.q, qbad, values, "sum", status=INVALID)
    assert "radii[5]" in pt._load().ptk_last_error().decode()


def test_coincident_points_and_the_own_record(emu_lib):
    """Piles of coincident points: the OTHER points of a pile are folded in, the own record is not, and with
    INCLUDE_SELF it is folded in exactly once.  The values are distinct powers of two: a sum names its terms."""
    p = np.repeat(np.array([[0.5, 0.25, -1.0], [3.0, 3.0, 3.0]], dtype=np.float32), [7, 5], axis=0)
    values = np.exp2(np.arange(12, dtype=np.float32))[:, None].copy()
    pile = np.array([values[:7].sum()] * 7 + [values[7:].sum()] * 5, dtype=np.float32)[:, None]
    tree = host_tree(p, 3, "L2Squared")
    emu = Emulated(emu_lib, p, 3, "L2Squared")
    for run in (lambda **kw: host_self(tree, p, 0.01, values, "sum", **kw), lambda **kw: emu.self_form(F32(0.01), values, "sum", **kw)):
        got, cnt = run()
        assert same(got, pile - values) and np.array_equal(cnt, [6] * 7 + [4] * 5)
        got, cnt = run(inc=True)
        assert same(got, pile) and np.array_equal(cnt, [6] * 7 + [4] * 5)
    c = case("ties", "L2Squared")
    name, r = c.sources()[4]
    off, flat = c.rows(name, r)
    assert (flat["distance"] == 0).sum() > 0 and not np.any(flat["index"] == np.repeat(np.arange(c.n), lengths(off)))


@pytest.mark.parametrize("metric", ["L2Squared", "LPInf"])
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_emulated_self_kernel_on_a_stream_that_does_not_belong_to_its_points(emu_lib, metric, move):
    """A tree built over one cloud, searched over a shrunk or shifted copy: a point is often absent from its own row, and
    INCLUDE_SELF does not depend on that."""
    p_tree = ds.uniform_cloud(3_000, 3, 61)
    p = (p_tree * F32(0.5) + F32(0.25)) if move == "shrunk" else (p_tree + F32(0.3))
    p = np.ascontiguousarray(p, dtype=np.float32)
    emu = Emulated(emu_lib, p, 8, metric, tree_points=p_tree)
    values = spread_values(len(p), 2, 13)
    raw_off, raw_flat = search_rows(emu.host, p, p, 0.05)
    own = raw_flat["index"] == np.repeat(np.arange(len(p)), lengths(raw_off))
    assert 0 < own.sum() < len(p)  # (some rows hold their own record, some do not)
    for r in (0.01, 0.05):
        off, flat = self_rows(emu.host, p, r)
        for op, inc in (("sum", True), ("sum", False), ("min", True)):
            want = fold(values, off, flat, op, own=values if inc else None)
            assert same(host_self(emu.host, p, r, values, op, inc=inc)[0], want), (metric, move, r, op, inc)
            got, cnt = emu.self_form(F32(r), values, op, piece=1000, inc=inc)
            assert same(got, want) and np.array_equal(cnt, lengths(off)), (metric, move, r, op, inc)


def test_argument_checks_and_the_python_wrapper_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = host_tree(p, 3, "L2Squared")
    lib = pt._load()
    values = spread_values(9, 2, 1)
    out, cnt = np.zeros((9, 2), dtype=np.float32), np.zeros(9, dtype=np.uint64)
    h, pp, vp, op_, cp = tree._h, p.ctypes.data, values.ctypes.data, out.ctypes.data, cnt.ctypes.data
    q = ds.uniform_cloud(4, 3, 22)
    qp = q.ctypes.data
    ok = np.full(9, 0.1, dtype=np.float32)
    hs, hw = lib.ptk_host_aggregate_within_self, lib.ptk_host_aggregate_within
    ds_, dw = lib.ptk_aggregate_within_self, lib.ptk_aggregate_within
    assert hs(h, pp, F32(0.1), None, vp, 2, 0, op_, cp) == 0 and hs(h, pp, F32(0.1), None, vp, 2, 0, op_, None) == 0
    assert hw(h, pp, qp, 4, F32(0.1), None, vp, 2, 2, op_, cp) == 0
    # every PTK_ERR_INVALID of the contract, from the host loops and from the device forms on this handle alike
    for channels in (0, 1025):
        assert hs(h, pp, F32(0.1), None, vp, channels, 0, op_, cp) == INVALID
        assert "channels" in lib.ptk_last_error().decode()
        assert hw(h, pp, qp, 4, F32(0.1), None, vp, channels, 0, op_, cp) == INVALID
        assert ds_(h, F32(0.1), None, vp, channels, 0, op_, cp) == INVALID
        assert dw(h, qp, 4, F32(0.1), None, vp, channels, 0, op_, cp) == INVALID
    for bad_op in (3, 0xFF, 0x200, 0x103):
        assert hs(h, pp, F32(0.1), None, vp, 2, bad_op, op_, cp) == INVALID
        assert hw(h, pp, qp, 4, F32(0.1), None, vp, 2, bad_op, op_, cp) == INVALID
        assert ds_(h, F32(0.1), None, vp, 2, bad_op, op_, cp) == INVALID
        assert dw(h, qp, 4, F32(0.1), None, vp, 2, bad_op, op_, cp) == INVALID
    for inc_op in (0x100, 0x101, 0x102):  # INCLUDE_SELF belongs to the self forms
        assert hs(h, pp, F32(0.1), None, vp, 2, inc_op, op_, cp) == 0
        assert hw(h, pp, qp, 4, F32(0.1), None, vp, 2, inc_op, op_, cp) == INVALID
        assert dw(h, qp, 4, F32(0.1), None, vp, 2, inc_op, op_, cp) == INVALID
        assert lib.ptk_aggregate_within_device(h, qp, 4, F32(0.1), None, vp, 2, inc_op, op_, cp, None) == INVALID
    for v_, o_ in ((None, op_), (vp, None), (vp, vp)):  # null values, null out, out == values
        assert hs(h, pp, F32(0.1), None, v_, 2, 0, o_, cp) == INVALID
        assert hw(h, pp, qp, 4, F32(0.1), None, v_, 2, 0, o_, cp) == INVALID
        assert ds_(h, F32(0.1), None, v_, 2, 0, o_, cp) == INVALID
        assert dw(h, qp, 4, F32(0.1), None, v_, 2, 0, o_, cp) == INVALID
    assert hw(h, pp, None, 0, F32(0.1), None, None, 2, 0, None, None) == 0  # (no rows to write)
    assert hs(None, pp, F32(0.1), None, vp, 2, 0, op_, cp) == INVALID and hs(h, None, F32(0.1), None, vp, 2, 0, op_, cp) == INVALID
    assert hw(h, pp, None, 4, F32(0.1), None, vp, 2, 0, op_, cp) == INVALID
    assert ds_(None, F32(0.1), None, vp, 2, 0, op_, cp) == INVALID and dw(None, qp, 4, F32(0.1), None, vp, 2, 0, op_, cp) == INVALID
    for bad in (np.nan, -0.5, -INF):
        assert hs(h, pp, F32(bad), None, vp, 2, 0, op_, cp) == INVALID
        assert "radius must be >= 0" in lib.ptk_last_error().decode()
        assert hw(h, pp, qp, 4, F32(bad), None, vp, 2, 0, op_, cp) == INVALID
        assert hs(h, pp, F32(bad), ok.ctypes.data, vp, 2, 0, op_, cp) == 0  # (ignored beside an array)
        assert hw(h, pp, qp, 4, F32(bad), ok.ctypes.data, vp, 2, 0, op_, cp) == 0
    for bad in (np.nan, -1e-3):
        radii = ok.copy()
        radii[2] = radii[3] = bad
        assert hs(h, pp, F32(1), radii.ctypes.data, vp, 2, 0, op_, cp) == INVALID
        assert "radii[2]" in lib.ptk_last_error().decode()
        assert hw(h, pp, qp, 4, F32(1), radii.ctypes.data, vp, 2, 0, op_, cp) == INVALID
        assert "radii[2]" in lib.ptk_last_error().decode()
    # a host-only handle has no device search
    assert ds_(h, F32(0.1), None, vp, 2, 0, op_, cp) == DEVICE
    assert dw(h, qp, 4, F32(0.1), None, vp, 2, 0, op_, cp) == DEVICE
    assert lib.ptk_aggregate_within_self_device(h, F32(0.1), None, vp, 2, 0, op_, cp, None) == DEVICE
    assert lib.ptk_aggregate_within_device(h, qp, 4, F32(0.1), None, vp, 2, 0, op_, cp, None) == DEVICE
    # the host loops serve the topological metrics and dim > 3
    pts5 = ds.uniform_cloud(200, 5, 5)
    t5 = host_tree(pts5, 4, "L2Squared")
    v5 = spread_values(200, 1, 2)
    off, flat = self_rows(t5, pts5, 0.3)
    assert lengths(off).sum() > 0 and same(host_self(t5, pts5, 0.3, v5, "sum")[0], fold(v5, off, flat, "sum"))
    pse2 = np.random.default_rng(12).random((300, 3), dtype=np.float32)
    se2 = host_tree(pse2, 4, "SE2Squared")
    v3 = spread_values(300, 1, 3)
    off, flat = self_rows(se2, pse2, 0.02)
    assert lengths(off).sum() > 0 and same(host_self(se2, pse2, 0.02, v3, "max", inc=True)[0], fold(v3, off, flat, "max", own=v3))
    off, flat = search_rows(se2, pse2, pse2[:50] + F32(0.001), 0.02)
    assert same(host_within(se2, pse2, np.ascontiguousarray(pse2[:50] + F32(0.001)), 0.02, v3, "min")[0], fold(v3, off, flat, "min"))
    # the Python wrapper: refusals of its own, then the library's
    with pytest.raises(pt.PtkError) as no_device:
        tree.aggregate_within_self(0.1, values)
    assert no_device.value.status == DEVICE
    with pytest.raises(pt.PtkError):
        tree.aggregate_within(q, 0.1, values)
    for bad in (values.astype(np.float64), np.zeros((8, 2), dtype=np.float32), np.zeros((9, 2, 1), dtype=np.float32),
                np.zeros((9, 0), dtype=np.float32), np.zeros((9, 1025), dtype=np.float32), np.float32(1.0), "x"):
        with pytest.raises(ValueError):
            tree.aggregate_within_self(0.1, bad)
        with pytest.raises(ValueError):
            tree.aggregate_within(q, 0.1, bad)
    for bad in ("mean", None, 3):
        with pytest.raises(ValueError):
            tree.aggregate_within_self(0.1, values, op=bad)
        with pytest.raises(ValueError):
            tree.aggregate_within(q, 0.1, values, op=bad)
    for bad in (np.zeros(8, dtype=np.float32), np.zeros((9, 1), dtype=np.float32), "x"):
        with pytest.raises(ValueError):
            tree.aggregate_within_self(bad, values)
    with pytest.raises(ValueError):
        tree.aggregate_within(q, np.zeros(3, dtype=np.float32), values)
    with pytest.raises(ValueError):
        tree.aggregate_within(np.zeros((4, 2), dtype=np.float32), 0.1, values)
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    with pytest.raises(pt.PtkError) as f64:
        t64.aggregate_within_self(0.1, values)
    assert "float32" in str(f64.value)
    with pytest.raises(pt.PtkError):
        t64.aggregate_within(q.astype(np.float64), 0.1, values)
    # allow_host_loop does not serve a handle without a device (PTK_ERR_DEVICE is no refusal of the search)
    pt.allow_host_loop(True)
    try:
        with pytest.raises(pt.PtkError):
            tree.aggregate_within_self(0.1, values)
    finally:
        pt.allow_host_loop(False)


def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "aggregate_main.cpp"), "-o", out]
    if host_only:  # (a stand-alone host program: the place for the sanitizers)
        cmd[1:1] = ["-DPICO_TREE_HOST_ONLY", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def check_cpp(exe, d, c, channels):
    """The program's files against the fold over the host loops' rows."""
    values = spread_values(c.n, channels, 77)
    r = c.scalars[2] if c.scalars[2] > 0 else c.scalars[-1]
    for name, a in (("points", c.p), ("queries", c.q), ("radii", c.radii), ("qradii", c.qradii), ("values", values)):
        np.ascontiguousarray(a, dtype=np.float32).tofile(os.path.join(d, name + ".bin"))
    res = subprocess.run([exe, d, repr(float(r)), str(channels), str(c.leaf), _CPP_METRIC[c.metric]], capture_output=True,
                         text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rows = {"self_scalar": (self_rows(c.tree, c.p, r), None), "self_radii": (c.rows("per row", c.radii), values),
            "within_scalar": (search_rows(c.tree, c.p, c.q, r), None), "within_radii": (c.qrows("per row", c.qradii), None)}
    for stem, ((off, flat), own) in rows.items():
        for op in OPS:
            got = np.fromfile(os.path.join(d, f"{stem}_{op}.out"), dtype=np.float32).reshape(-1, channels)
            cnt = np.fromfile(os.path.join(d, f"{stem}_{op}.cnt"), dtype=np.uint64)
            assert same(got, fold(values, off, flat, op, own=own)), (c.kind, c.metric, stem, op)
            assert np.array_equal(cnt.astype(np.int64), lengths(off)), (c.kind, c.metric, stem, op)


@pytest.fixture(scope="module")
def cpp_host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aggregate_cpp") / "aggregate_host")
    _cpp_program(exe, host_only=True)
    return exe


@pytest.mark.parametrize("kind,metric,channels", [("uniform", "L2Squared", 3), ("lidar", "L1", 1), ("ties", "LPInf", W + 1),
                                                  ("small", "LNInf", 4)])
def test_cpp_members_without_a_backend_under_the_sanitizers(cpp_host_exe, tmp_path, kind, metric, channels):
    check_cpp(cpp_host_exe, str(tmp_path), case(kind, metric), channels)


# ---- gpu tier ---------------------------------------------------------------------------------------------------------

def device_placed(torch, dev, shape, offset, fill=None):
    """A float32 CUDA tensor of `shape` at 16 k (+ 4 with `offset`) inside a buffer of marker floats: (buffer, view)."""
    count = int(np.prod(shape))
    buf = torch.full((count + 8,), float(np.frombuffer(bytes([MARK] * 4), dtype=np.float32)[0]), dtype=torch.float32, device=dev)
    at = (-buf.data_ptr() % 16) // 4 + 4 + (1 if offset else 0)
    view = buf[at:at + count].view(*shape)
    assert view.data_ptr() % 16 == (4 if offset else 0) and view.is_contiguous()
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill)))
    return buf, view, at


def device_call(tree, gpu, r, values, op, q=None, inc=False, counts=True, offset=False, stream=None):
    """The _device form (self: q None) on torch buffers placed as asked; returns (out, counts) as numpy."""
    import torch

    dev = torch.device("cuda", gpu)
    lib = pt._load()
    rows = tree.npts if q is None else len(q)
    channels = values.shape[1]
    _, v, _ = device_placed(torch, dev, values.shape, offset, values)
    obuf, out, at = device_placed(torch, dev, (rows, channels), offset)
    cnt = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    scalar = np.ndim(r) == 0
    d_r = None if scalar else torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    tail = (F32(r if scalar else 0), None if scalar else d_r.data_ptr(), v.data_ptr(), channels,
            OPS[op] | (INCLUDE_SELF if inc else 0), out.data_ptr(), cnt.data_ptr() if counts else None, s)
    if q is None:
        rc = lib.ptk_aggregate_within_self_device(tree._h, *tail)
    else:
        d_q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        rc = lib.ptk_aggregate_within_device(tree._h, d_q.data_ptr(), rows, *tail)
    assert rc == 0, lib.ptk_last_error()
    torch.cuda.synchronize(dev)
    whole = obuf.cpu().numpy()
    got = whole[at:at + rows * channels].reshape(rows, channels).copy()
    guard = np.concatenate([whole[:at], whole[at + rows * channels:]])
    assert np.all(bits(guard) == 0xA5A5A5A5), "a write outside the output"
    assert not np.any(bits(got) == 0xA5A5A5A5), "an entry of out was not written"
    c = cnt.cpu().numpy()
    assert not counts or not np.any(c == -1), "a count was not written"
    return got, (c if counts else None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric", METRICS)
def test_device_equals_the_contract(gpu, kind, metric, monkeypatch):
    """Both forms on the device against the fold over the host loops' rows, bit for bit: scalar and per-row radii, the
    three ops, the own value, 1, 5, W and 2 W + 1 channels, aligned and offset buffers, pieces of 1 000 positions, the
    host-buffer forms and the Python wrapper."""
    c = case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    turn = 0
    for name, r in c.sources():
        off, flat = c.rows(name, r)
        for op in OPS:
            for inc in (False, True):
                channels = [1, 5, W, 2 * W + 1][turn % 4]
                offset = (turn // 4) % 2 == 1
                turn += 1
                values = spread_values(c.n, channels, 40 + channels)
                want = fold(values, off, flat, op, own=values if inc else None)
                what = (kind, metric, name, op, inc, channels, offset)
                got, cnt = device_call(tree, gpu, r, values, op, inc=inc, offset=offset)
                assert same(got, want) and np.array_equal(cnt, lengths(off)), what
                assert same(device_call(tree, gpu, r, values, op, inc=inc, offset=not offset, counts=False)[0], want), what
    # every channel count at both placements, on one source
    name, r = c.sources()[2] if kind != "ties" else c.sources()[4]
    off, flat = c.rows(name, r)
    for channels in (1, 5, W, 2 * W + 1):
        values = spread_values(c.n, channels, 60 + channels)
        want = fold(values, off, flat, "sum")
        for offset in (False, True):
            assert same(device_call(tree, gpu, r, values, "sum", offset=offset)[0], want), (kind, metric, channels, offset)
    for name, r in c.qsources():
        off, flat = c.qrows(name, r)
        for op in OPS:
            channels = [1, 5, W, 2 * W + 1][turn % 4]
            offset = (turn // 4) % 2 == 1
            turn += 1
            values = spread_values(c.n, channels, 80 + channels)
            want = fold(values, off, flat, op)
            got, cnt = device_call(tree, gpu, r, values, op, q=c.q, offset=offset)
            assert same(got, want) and np.array_equal(cnt, lengths(off)), (kind, metric, "query", name, op, channels, offset)
            assert same(device_call(tree, gpu, r, values, op, q=c.q, offset=not offset)[0], want)
    # pieces; the host-buffer forms; the wrapper; the counts of the count calls
    values = spread_values(c.n, W + 1, 3)
    off, flat = c.rows("per row", c.radii)
    want = fold(values, off, flat, "sum", own=values)
    monkeypatch.setenv("PTK_MAX_BATCH", "1000")
    got, cnt = device_call(tree, gpu, c.radii, values, "sum", inc=True)
    monkeypatch.delenv("PTK_MAX_BATCH")
    assert same(got, want) and np.array_equal(cnt, lengths(off))
    got, cnt = call(pt._load().ptk_aggregate_within_self, (tree._h,), c.n, c.radii, values, "sum", inc=True)
    assert same(got, want) and np.array_equal(cnt, lengths(off))
    got, cnt = tree.aggregate_within_self(c.radii, values, include_self=True, counts=True)
    assert same(got, want) and np.array_equal(cnt, lengths(off)) and np.array_equal(cnt, tree.count_within_self(c.radii))
    flat1 = tree.aggregate_within_self(c.radii, values[:, 0].copy(), op="max")
    assert flat1.shape == (c.n,) and same(flat1, fold(values[:, :1].copy(), off, flat, "max")[:, 0])
    qoff, qflat = c.qrows("per row", c.qradii)
    want = fold(values, qoff, qflat, "min")
    got, cnt = call(pt._load().ptk_aggregate_within, (tree._h, c.q.ctypes.data, len(c.q)), len(c.q), c.qradii, values, "min")
    assert same(got, want) and np.array_equal(cnt, lengths(qoff))
    got, cnt = tree.aggregate_within(c.q, c.qradii, values, op="min", counts=True)
    assert same(got, want) and np.array_equal(cnt, tree.count_within(c.q, c.qradii))


@pytest.mark.gpu
def test_query_rows_come_back_in_the_callers_order(gpu):
    """A batch large enough to be reordered for the launch (12 000 shuffled rows, each with its own radius): rows are
    compared in the caller's order, so a mix-up between launch position and row index shows."""
    import torch

    p = ds.uniform_cloud(20_000, 3, 71)
    rng = np.random.default_rng(5)
    q = np.ascontiguousarray((p[rng.permutation(len(p))[:12_000]] + (rng.random((12_000, 3)) - 0.5).astype(np.float32) * F32(0.01)))
    radii = (rng.random(12_000) * 0.003).astype(np.float32)  # (squared: up to ~0.055 across)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    values = spread_values(len(p), 5, 21)
    off, flat = search_rows(tree, p, q, radii)
    assert len(np.unique(lengths(off))) > 20
    for op in OPS:
        got, cnt = device_call(tree, gpu, radii, values, op, q=q)
        assert same(got, fold(values, off, flat, op)) and np.array_equal(cnt, lengths(off)), op
    dev = torch.device("cuda", gpu)
    got, cnt = tree.aggregate_within(torch.from_numpy(q).to(dev), torch.from_numpy(radii).to(dev),
                                     torch.from_numpy(values).to(dev), op="sum", counts=True)
    assert same(got.cpu().numpy(), fold(values, off, flat, "sum")) and np.array_equal(cnt.cpu().numpy(), lengths(off))
    one = tree.aggregate_within(torch.from_numpy(q).to(dev), 0.001, torch.from_numpy(values[:, 0].copy()).to(dev), op="max")
    soff, sflat = search_rows(tree, p, q, 0.001)
    assert tuple(one.shape) == (12_000,) and same(one.cpu().numpy(), fold(values[:, :1].copy(), soff, sflat, "max")[:, 0])


@pytest.mark.gpu
def test_device_forms_on_a_side_stream_and_radii_that_pass_no_test(gpu):
    import torch

    c = case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    dev = torch.device("cuda", gpu)
    side = torch.cuda.Stream(device=gpu)
    values = spread_values(c.n, 5, 31)
    bad = c.radii.copy()
    bad[100], bad[2000] = np.nan, -1.0
    qbad = c.qradii.copy()
    qbad[5], qbad[50] = np.nan, -1.0
    with torch.cuda.stream(side):
        dv = torch.from_numpy(values).to(dev)
        d_radii, d_bad = torch.from_numpy(c.radii).to(dev), torch.from_numpy(bad).to(dev)
        dq, d_qbad = torch.from_numpy(c.q).to(dev), torch.from_numpy(qbad).to(dev)
        a, ca = tree.aggregate_within_self(d_radii, dv, counts=True, device=True)
        a2 = tree.aggregate_within_self(d_radii, dv, device=True)
        b, cb = tree.aggregate_within_self(d_bad, dv, op="max", include_self=True, counts=True, device=True)
        s = tree.aggregate_within_self(float(c.scalars[1]), dv, op="min", device=True)
        w, cw = tree.aggregate_within(dq, d_qbad, dv, op="min", counts=True)
    side.synchronize()
    off, flat = c.rows("per row", c.radii)
    assert same(a.cpu().numpy(), fold(values, off, flat, "sum")) and same(a2.cpu().numpy(), a.cpu().numpy())
    assert np.array_equal(ca.cpu().numpy(), lengths(off))
    assert same(s.cpu().numpy(), fold(values, *c.rows("r1", c.scalars[1]), "min"))
    keep = np.ones(c.n, dtype=bool)
    keep[[100, 2000]] = False
    want = fold(values, off, flat, "max", own=values)
    b, cb = b.cpu().numpy(), cb.cpu().numpy()
    assert lengths(off)[100] > 0 and lengths(off)[2000] > 0
    assert same(b[keep], want[keep]) and same(b[~keep], values[~keep]) and not cb[~keep].any()
    qoff, qflat = c.qrows("per row", c.qradii)
    qkeep = np.ones(len(c.q), dtype=bool)
    qkeep[[5, 50]] = False
    w, cw = w.cpu().numpy(), cw.cpu().numpy()
    assert same(w[qkeep], fold(values, qoff, qflat, "min")[qkeep]) and np.all(w[~qkeep] == INF) and not cw[~qkeep].any()
    with pytest.raises(ValueError):
        tree.aggregate_within_self(bad, dv, device=True)  # (host radii are checked before they go up)
    with pytest.raises(ValueError):
        tree.aggregate_within_self(0.1, values, device=True)  # (a device call takes a CUDA tensor)


@pytest.mark.gpu
def test_special_values_on_the_device(gpu):
    c = case("small", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    values = special_values(c.n, 3)
    name, r = c.sources()[2]
    off, flat = c.rows(name, r)
    qoff, qflat = c.qrows("per row", c.qradii)
    for op in OPS:
        eq = same_numbers if op == "sum" else same
        for inc in (False, True):
            for offset in (False, True):
                want = fold(values, off, flat, op, own=values if inc else None)
                assert eq(device_call(tree, gpu, r, values, op, inc=inc, offset=offset)[0], want), (op, inc, offset)
        assert eq(device_call(tree, gpu, c.qradii, values, op, q=c.q)[0], fold(values, qoff, qflat, op)), op
    for name, r in c.sources()[3:-1]:  # 10.0, +inf, FLT_MAX: whole-tree rows
        off, flat = c.rows(name, r)
        assert np.all(lengths(off) == c.n - 1)
        v = spread_values(c.n, 2, 8)
        assert same(device_call(tree, gpu, r, v, "sum")[0], fold(v, off, flat, "sum")), name


@pytest.mark.gpu
def test_the_radius_capture_is_left_alone(gpu):
    """A scalar search_radius count / fill pair with aggregate calls between its halves still copies its captured rows."""
    import torch

    p, q = ds.uniform_cloud(20_000, 3, 71), ds.uniform_cloud(6_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    lib = pt._load()
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    stream = torch.cuda.current_stream(dq.device).cuda_stream
    want = tree.search_radius(q, 0.002)
    counts = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), len(q), F32(0.002), F32(1), counts.data_ptr(),
                                              stream) == 0
    values = spread_values(len(p), 3, 2)
    dv = torch.from_numpy(values).to(dq.device)
    mine = tree.aggregate_within_self(0.001, dv, device=True)
    theirs = tree.aggregate_within(dq, 0.002, dv, op="max")
    offsets = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    offsets[1:] = torch.cumsum(counts[:len(q)], 0)
    out = torch.empty((max(int(offsets[-1].item()), 1), 2), dtype=torch.int32, device=dq.device)
    assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), len(q), F32(0.002), F32(1), offsets.data_ptr(),
                                             out.data_ptr(), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want.offsets)
    rows = np.ascontiguousarray(out.cpu().numpy()).view(pt.NEIGHBOR).reshape(-1)
    assert rows[:len(want.flat)].tobytes() == want.flat.tobytes()
    assert same(mine.cpu().numpy(), fold(values, *self_rows(tree, p, 0.001), "sum"))
    assert same(theirs.cpu().numpy(), fold(values, want.offsets, want.flat, "max"))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [39, 40, 135, 136, 1031])
def test_depths_where_the_stack_class_changes(gpu, depth):
    pts = np.asarray(depth_cases.cloud_at_depth(depth, 3, 10)[0])
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    depth_cases.assert_depth(tree, depth)
    off, flat = self_rows(tree, pts, 0.05)
    assert np.all(lengths(off)[3_000:] == len(pts) - 3_001)  # (the rest of the pile, at offset 0)
    values = spread_values(len(pts), W + 1, depth)
    got, cnt = device_call(tree, gpu, 0.05, values, "sum", inc=True)
    assert same(got, fold(values, off, flat, "sum", own=values)) and np.array_equal(cnt, lengths(off)), depth
    q = np.ascontiguousarray(pts[::7] + F32(0.001))
    qoff, qflat = search_rows(tree, pts, q, 0.05)
    got, cnt = device_call(tree, gpu, 0.05, values, "max", q=q)
    assert same(got, fold(values, qoff, qflat, "max")) and np.array_equal(cnt, lengths(qoff)), depth


@pytest.mark.gpu
def test_refusals(gpu):
    """The deep stack class, dim > 3 and the topological metrics: PTK_ERR_UNSUPPORTED with the host loop named;
    allow_host_loop then serves them with the bytes of the fold."""
    deep = np.asarray(depth_cases.cloud_at_depth(1032, 3, 10)[0])
    cases = [(deep, pt.Metric.L2Squared, 10, 0.01, "tree depth 1032"),
             (ds.uniform_cloud(2_500, 5, 10), pt.Metric.L2Squared, 8, 0.3, "dim > 3"),
             (np.random.default_rng(12).random((2_000, 3), dtype=np.float32), pt.Metric.SE2Squared, 8, 0.01, "topological")]
    for p, metric, leaf, r, why in cases:
        p = np.ascontiguousarray(p, dtype=np.float32)
        tree = pt.KdTree(p, metric, leaf, device=gpu)
        values = spread_values(len(p), 3, 4)
        q = np.ascontiguousarray(p[::5] + F32(0.001))
        with pytest.raises(pt.PtkError) as refused:
            tree.aggregate_within_self(r, values)
        assert refused.value.status == UNSUPPORTED
        assert why in str(refused.value) and "ptk_host_aggregate_within_self" in str(refused.value)
        with pytest.raises(pt.PtkError) as refused:
            tree.aggregate_within(q, r, values)
        assert refused.value.status == UNSUPPORTED
        assert why in str(refused.value) and "(ptk_host_aggregate_within)" in str(refused.value)
        pt.allow_host_loop(True)
        try:
            with warnings.catch_warnings():  # (the host loop warns once per process)
                warnings.simplefilter("ignore")
                got, cnt = tree.aggregate_within_self(r, values, op="max", include_self=True, counts=True)
                qgot, qcnt = tree.aggregate_within(q, r, values, counts=True)
        finally:
            pt.allow_host_loop(False)
        off, flat = self_rows(tree, p, r)
        assert same(got, fold(values, off, flat, "max", own=values)) and np.array_equal(cnt, lengths(off)), why
        qoff, qflat = search_rows(tree, p, q, r)
        assert same(qgot, fold(values, qoff, qflat, "sum")) and np.array_equal(qcnt, lengths(qoff)), why
    small = pt.KdTree(cloud("small")[0], pt.Metric.L2Squared, 5, device=gpu)
    lib = pt._load()
    v = spread_values(small.npts, 2, 1)
    out = np.zeros_like(v)
    bad = np.full(small.npts, 0.1, dtype=np.float32)
    bad[7] = bad[9] = np.nan
    assert lib.ptk_aggregate_within_self(small._h, F32(np.nan), None, v.ctypes.data, 2, 0, out.ctypes.data, None) == INVALID
    assert lib.ptk_aggregate_within_self(small._h, F32(1), bad.ctypes.data, v.ctypes.data, 2, 0, out.ctypes.data, None) == INVALID
    assert "radii[7]" in lib.ptk_last_error().decode()
    assert lib.ptk_aggregate_within_self(small._h, F32(1), None, v.ctypes.data, 2, 0, v.ctypes.data, None) == INVALID
    assert lib.ptk_aggregate_within_self(small._h, F32(1), None, v.ctypes.data, 0, 0, out.ctypes.data, None) == INVALID
    t64 = pt.KdTree(cloud("small")[0].astype(np.float64), pt.Metric.L2Squared, 5, device=gpu)
    with pytest.raises(pt.PtkError):
        t64.aggregate_within_self(0.1, v)


@pytest.mark.gpu
def test_cpp_members_through_the_backend(gpu, tmp_path):
    exe = str(tmp_path / "aggregate_batch")
    _cpp_program(exe, host_only=False)
    check_cpp(exe, str(tmp_path), case("uniform", "L2Squared"), W + 1)
