"""gpu tier: the host-buffer forms whose rows have one size, through the one body that stages them (host_form in
pico_tree_amd/csrc/ptk_backend.hip, host_form64 in ptk_backend_f64.hpp, the layout of ptk_io_parts.hpp).

The shapes are the smallest at which the staging can go wrong, not a workload: 3 000 uniform 3-D points (leaf size 10),
257 queries (four wavefronts and one lane), a 130-point tree for the self forms, and the same trees in float64.  Every
form is compared byte for byte with what its family's tests compare to: the rows of ``oracle.Oracle(.., "port")`` filtered
as tests/test_knn_within.py and tests/test_count_within.py filter them, the numpy fold of tests/test_aggregate_within.py,
the moments, host-loop frames and labels of tests/test_normals_self.py and tests/test_cluster_self.py (imported, not
copied).  Expected values never come from the code under test, except where a test says "the same call on a fresh handle"
or "the serial result": there the subject is the handle's blocks and lock, and the values themselves are checked above.
"""

from __future__ import annotations

import functools
import threading

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import test_aggregate_within as ta
from tests import test_cluster_self as tc
from tests import test_count_within as tcw
from tests import test_knn_self as tks
from tests import test_knn_within as tkw
from tests import test_normals_self as tn
from tests.test_radius_self import without_self

LEAF = 10
NQ, K = 257, 16
VIEW = [0.3, 0.2, 5.0]
UNSUPPORTED = -2


# ---- the data and what is expected of it: no GPU, computed once ----------------------------------------------------------

class Data:
    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        real = self.dtype.type
        scale = real(1.0000001) if self.dtype == np.float64 else real(1)  # (float64: coordinates no float32 holds)
        self.p = np.ascontiguousarray(ds.uniform_cloud(3_000, 3, 71).astype(dtype) * scale)
        self.q = np.ascontiguousarray(ds.uniform_cloud(NQ, 3, 72).astype(dtype) * scale)
        self.s = np.ascontiguousarray(ds.uniform_cloud(130, 3, 73).astype(dtype) * scale)
        self.ref = oracle.Oracle(self.p, LEAF, "port", dtype=dtype)
        self.sref = oracle.Oracle(self.s, LEAF, "port", dtype=dtype)
        # the median distance of a query's 8th neighbour: rows of k = 16 are part hits, part padding
        self.r = real(np.median(self.ref.search_knn(self.q, K)["distance"][:, 7]))
        self.radii = np.array([0, self.r / 2, self.r, 4 * self.r], dtype=dtype)[np.arange(NQ) % 4]
        # ... and of a point's 4th other point in the small tree (column 0 is the point itself)
        self.rs = real(np.median(self.sref.search_knn(self.s, 6)["distance"][:, 4]))
        self.sradii = np.array([self.rs / 2, self.rs, 2 * self.rs, 0], dtype=dtype)[np.arange(130) % 4]


@functools.lru_cache(maxsize=None)
def data(dtype):
    return Data(dtype)


def radius_rows(ref, q, r):
    """(offsets, flat) of the oracle's search_radius; r an array: row i is its row of the run at r[i]."""
    if np.ndim(r) == 0:
        return ref.search_radius(q, r)
    parts = [None] * len(q)
    for v in np.unique(r):
        at = np.flatnonzero(r == v)
        off, flat = ref.search_radius(np.ascontiguousarray(q[at]), v)
        off = np.asarray(off).astype(np.int64)
        for j, i in enumerate(at):
            parts[i] = flat[off[j]:off[j + 1]]
    offsets = np.zeros(len(q) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in parts])
    return offsets, np.concatenate(parts)


def self_rows(ref, p, r):
    return without_self(*radius_rows(ref, p, r))


def knn_rows(ref, q, k, r):
    """tests/test_knn_within.py::expected; r an array: row i is its row at r[i]."""
    if np.ndim(r) == 0:
        return tkw.expected(ref, q, k, r)
    out = np.zeros((len(q), k), dtype=ref.neighbor)
    for v in np.unique(r):
        at = np.flatnonzero(r == v)
        out[at] = tkw.expected(ref, np.ascontiguousarray(q[at]), k, v)
    return out


def counts_of(ref, q, r):
    """tests/test_count_within.py::expected; r an array: the lengths of radius_rows."""
    if np.ndim(r) == 0:
        return tcw.expected(ref, q, r)
    return np.diff(np.asarray(radius_rows(ref, q, r)[0]).astype(np.int64))


def raw(a):
    """The bytes that count: of neighbour records the index and the distance (the padding of the float64 record has a
    test of its own), of anything else all of them; None (an output that was not asked for) stays None."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype.names == ("index", "distance"):
        return np.ascontiguousarray(a["index"]).tobytes() + np.ascontiguousarray(a["distance"]).tobytes()
    return np.ascontiguousarray(a).tobytes()


def same(got, want):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    return len(got) == len(want) and all(raw(g) == raw(w) for g, w in zip(got, want))


def aggregate(tree, q, r, values, counts):
    """ptk_aggregate_within (q given) or ptk_aggregate_within_self through tests/test_aggregate_within.py::call: guarded
    buffers, every entry written."""
    lib = pt._load()
    if q is None:
        return ta.call(lib.ptk_aggregate_within_self, (tree._h,), tree.npts, r, values, "sum", counts=counts)
    return ta.call(lib.ptk_aggregate_within, (tree._h, q.ctypes.data, len(q)), len(q), r, values, "sum", counts=counts)


def cases(dtype):
    """[(name, which tree ("p" or "s"), run(tree) -> result, expected)] of every fixed-row host form of a precision with
    every optional part present and absent."""
    d = data(dtype)
    out = []
    for rname, r, rs in (("scalar radius", d.r, d.rs), ("per-row radii", d.radii, d.sradii)):
        out.append((f"knn_within, {rname}", "p", lambda t, r=r: t.search_knn_within(d.q, K, r), knn_rows(d.ref, d.q, K, r)))
        out.append((f"count_within, {rname}", "p", lambda t, r=r: t.count_within(d.q, r), counts_of(d.ref, d.q, r)))
        off, flat = self_rows(d.sref, d.s, rs)
        lens = np.diff(np.asarray(off).astype(np.int64))
        out.append((f"count_within_self, {rname}", "s", lambda t, rs=rs: t.count_within_self(rs), lens))
        for mn in (0, 3):
            out.append((f"cluster_within_self, {rname}, min_neighbors {mn}", "s",
                        lambda t, rs=rs, mn=mn: tc.device_labels(t, rs, mn), tc.expected_labels(off, flat, mn)))
        if d.dtype == np.float64:
            continue
        host = pt.KdTree(d.s, pt.Metric.L2Squared, LEAF, device=pt.PTK_DEVICE_NONE)
        frames = tn.host_normals(host, rs, 2, VIEW, want="frames")[0]
        moments = tn.expected_moments(d.s, off, flat)
        for want, expected in (("both", (frames, moments)), ("frames", (frames, None)), ("moments", (None, moments))):
            out.append((f"normals_within_self, {rname}, {want}", "s",
                        lambda t, rs=rs, want=want: tn.device_normals(t, rs, 2, VIEW, want=want), expected))
        qoff, qflat = radius_rows(d.ref, d.q, r)
        qlens = np.diff(np.asarray(qoff).astype(np.int64))
        for channels in (1, 9):  # (9: two channel windows)
            v, vs = ta.spread_values(len(d.p), channels, 5 + channels), ta.spread_values(len(d.s), channels, 7 + channels)
            for counts in (True, False):
                what = f"{rname}, {channels} channels, counts {'on' if counts else 'off'}"
                out.append((f"aggregate_within, {what}", "p",
                            lambda t, r=r, v=v, counts=counts: aggregate(t, d.q, r, v, counts),
                            (ta.fold(v, qoff, qflat, "sum"), qlens if counts else None)))
                out.append((f"aggregate_within_self, {what}", "s",
                            lambda t, rs=rs, vs=vs, counts=counts: aggregate(t, None, rs, vs, counts),
                            (ta.fold(vs, off, flat, "sum"), lens if counts else None)))
    out.append(("knn_self", "s", lambda t: t.search_knn_self(5), tks.expected(d.sref, d.s, 5)))
    if d.dtype == np.float64:
        out.append(("search_knn", "p", lambda t: t.search_knn(d.q, K), d.ref.search_knn(d.q, K)))
    return out


def trees(gpu, dtype):
    d = data(dtype)
    return {"p": pt.KdTree(d.p, pt.Metric.L2Squared, LEAF, device=gpu), "s": pt.KdTree(d.s, pt.Metric.L2Squared, LEAF, device=gpu)}


# ---- the tests --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_every_host_form_with_every_optional_part_present_and_absent(gpu, dtype):
    """All calls of a precision on ONE pair of handles, so each finds the blocks as the call before left them."""
    handles = trees(gpu, dtype)
    todo = cases(dtype)
    assert len(todo) == (33 if dtype == "float32" else 12)
    for name, which, run, want in todo:
        assert same(run(handles[which]), want), (dtype, name)
    for name, which, run, want in reversed(todo):  # ... and as the call AFTER it in the list left them
        assert same(run(handles[which]), want), (dtype, name, "second pass")


def reuse_sequence(dtype):
    """[(name, run(tree))]: large, small, large; a self form between two query forms; the other kinds of parts."""
    d = data(dtype)
    large = ("knn_within, 257 queries, k = 16", lambda t: t.search_knn_within(d.q, K, d.r))
    small = ("knn_within, 1 query, k = 1", lambda t: t.search_knn_within(d.q[:1], 1, d.r))
    seq = [large, small, large,
           ("count_within_self", lambda t: t.count_within_self(d.r)),
           ("count_within, per-row radii", lambda t: t.count_within(d.q, d.radii)),
           ("cluster_within_self", lambda t: tc.device_labels(t, d.r, 3))]
    if d.dtype == np.float32:
        v = ta.spread_values(len(d.p), 9, 3)
        seq += [("aggregate_within", lambda t: aggregate(t, d.q, d.radii, v, True)),
                ("normals_within_self", lambda t: tn.device_normals(t, d.r, 2, VIEW)),
                ("aggregate_within, no radii, no counts", lambda t: aggregate(t, d.q, d.r, v, False))]
    else:
        seq += [("search_knn", lambda t: t.search_knn(d.q, K))]
    return seq + [small, ("knn_within, per-row radii", lambda t: t.search_knn_within(d.q, K, d.radii)), large]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_blocks_reused_on_one_handle_give_what_a_fresh_handle_gives(gpu, dtype):
    """A stale offset, a block grown after its pointer was taken, a part read from the wrong block: each shows as a
    difference from the same call on a handle that has served nothing else."""
    d = data(dtype)
    used = pt.KdTree(d.p, pt.Metric.L2Squared, LEAF, device=gpu)
    for step, (name, run) in enumerate(reuse_sequence(dtype)):
        fresh = pt.KdTree(d.p, pt.Metric.L2Squared, LEAF, device=gpu)
        assert same(run(used), run(fresh)), (dtype, step, name)
    # (the values themselves, once: the large call against the oracle)
    assert same(used.search_knn_within(d.q, K, d.r), knn_rows(d.ref, d.q, K, d.r))


@pytest.mark.gpu
def test_float64_record_padding_comes_back_zero(gpu):
    """The four padding bytes of a ptk_neighbor64 record are written by no kernel (tests/test_f64.py: "padding zero --
    whatever the buffer held"): the host form clears them, in rows of hits and in rows of padding entries alike."""
    d = data("float64")
    tree = pt.KdTree(d.p, pt.Metric.L2Squared, LEAF, device=gpu)
    # The output block is dirtied first (a fresh allocation may read as zeros): at radius 0 every point is a cluster of its
    # own, and the labels 0, 1, 2, ... lie where the padding of the first 750 records will.
    assert np.array_equal(tc.device_labels(tree, 0.0, 0), np.arange(len(d.p)))
    for r in (d.r, d.radii):
        nns = np.empty((NQ, K), dtype=pt.NEIGHBOR64)
        nns.view(np.uint8).reshape(-1)[:] = 0xFF
        got = tree.search_knn_within(d.q, K, r, nns)
        assert got is nns and same(got, knn_rows(d.ref, d.q, K, r))
        assert not nns.view(np.uint8).reshape(NQ, K, 16)[:, :, 4:8].any()
    # k beyond the tree (tests/test_f64.py::test_gpu_double_k_larger_than_the_tree): the slots no search writes read
    # {0, DBL_MAX} with zero padding, whatever the block and the caller's array held
    small = pt.KdTree(d.s, pt.Metric.L2Squared, LEAF, device=gpu)
    assert np.array_equal(tc.device_labels(small, 0.0, 0), np.arange(len(d.s)))
    n, k = len(d.s), len(d.s) + 10
    nns = np.empty((NQ, k), dtype=pt.NEIGHBOR64)
    nns.view(np.uint8).reshape(-1)[:] = 0xFF
    got = small.search_knn(d.q, k, nns)
    assert same(got[:, :n], d.sref.search_knn(d.q, n))
    assert np.all(got["distance"][:, n:] == np.finfo(np.float64).max) and np.all(got["index"][:, n:] == 0)
    assert not got.view(np.uint8).reshape(NQ, k, 16)[:, :, 4:8].any()


@pytest.mark.gpu
def test_four_threads_on_one_float32_handle(gpu):
    """Four threads, one handle, a different host form each, ten times: the handle's I/O lock keeps the calls apart, so
    every result is the serial one.  Each thread touches its own arrays only; nothing else is shared."""
    d = data("float32")
    tree = pt.KdTree(d.p, pt.Metric.L2Squared, LEAF, device=gpu)
    v = ta.spread_values(len(d.p), 9, 3)
    forms = [("knn_within", lambda: tree.search_knn_within(d.q, K, d.radii)),
             ("count_within_self", lambda: tree.count_within_self(d.r)),
             ("normals_within_self", lambda: tree.normals_within_self(d.r, viewpoint=VIEW, moments=True)),
             ("aggregate_within", lambda: tree.aggregate_within(d.q, d.radii, v, counts=True))]
    serial = [run() for _, run in forms]
    assert same(serial[0], knn_rows(d.ref, d.q, K, d.radii))
    results = [[] for _ in forms]
    errors = []
    start = threading.Barrier(len(forms))

    def work(i):
        try:
            start.wait()
            for _ in range(10):
                results[i].append(forms[i][1]())
        except BaseException as ex:  # noqa: BLE001 (reported by the assert below)
            errors.append((forms[i][0], repr(ex)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(forms))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i, (name, _) in enumerate(forms):
        assert len(results[i]) == 10
        for turn, got in enumerate(results[i]):
            assert same(got, serial[i]), (name, turn)


@pytest.mark.gpu
def test_a_refused_call_between_two_served_ones(gpu):
    """count_within with per-row radii on a 4-D tree is refused (PTK_ERR_UNSUPPORTED) with the output untouched; the
    calls after it on that handle and on a 3-D handle are served and correct."""
    d = data("float32")
    p4, q4 = ds.uniform_cloud(3_000, 4, 74), ds.uniform_cloud(NQ, 4, 75)
    ref4 = oracle.Oracle(p4, LEAF, "port")
    r4 = np.float32(np.median(ref4.search_knn(q4, 8)["distance"][:, 7]))
    radii4 = np.full(NQ, r4, dtype=np.float32)
    want4 = tcw.expected(ref4, q4, r4)
    assert want4.min() < want4.max()
    tree4 = pt.KdTree(p4, pt.Metric.L2Squared, LEAF, device=gpu)
    tree3 = pt.KdTree(d.p, pt.Metric.L2Squared, LEAF, device=gpu)
    assert np.array_equal(tree4.count_within(q4, r4), want4)
    assert np.array_equal(tree3.count_within(d.q, d.radii), counts_of(d.ref, d.q, d.radii))
    with pytest.raises(pt.PtkError) as refused:
        tree4.count_within(q4, radii4)
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED == UNSUPPORTED
    counts = np.full(NQ, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    lib = pt._load()
    assert lib.ptk_search_count_within_radii(tree4._h, q4.ctypes.data, NQ, radii4.ctypes.data, 0, counts.ctypes.data) == UNSUPPORTED
    assert np.all(counts == 0xA5A5A5A5A5A5A5A5), "a refused call wrote to its output"
    assert np.array_equal(tree4.count_within(q4, r4), want4)
    assert np.array_equal(tree3.count_within(d.q, d.radii), counts_of(d.ref, d.q, d.radii))
    assert same(tree3.search_knn_within(d.q, K, d.r), knn_rows(d.ref, d.q, K, d.r))
