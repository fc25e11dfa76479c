"""What the host forms of the searches with ragged rows promise about ``offsets`` and ``*out`` (ptk.h): the one driver
behind them all (pico_tree_amd/csrc/ptk_rows_out.hpp), through the C ABI, for each of the eight entry points

    ptk_search_radius   ptk_search_radius_radii   ptk_search_radius_self   ptk_search_box     and their ptk_search64_ forms.

A tree of 300 uniform points in 3-D (leaf size 8) and 64 queries or boxes.  Expected rows: the library's host loops
(``ptk_host_search_*`` on a host-only handle) for float32, the oracle for float64 -- what the families' own tests use.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import poison

OK, INVALID, UNSUPPORTED = 0, -1, -2
N_POINTS, N_QUERIES, LEAF = 300, 64, 8
RADIUS = 0.01   # (squared: about 1.3 points of the unit cube's 300 in the ball)
HALF = 0.08     # half the side of a box: about 1.2 points
SENTINEL = 0xDEAD0

KINDS = ["radius", "radii", "self", "box"]
FORMS = [(kind, f64) for f64 in (False, True) for kind in KINDS]
FORM_IDS = [("ptk_search64_" if f64 else "ptk_search_") + ("box" if kind == "box" else "radius" if kind == "radius"
            else "radius_" + kind) for kind, f64 in FORMS]
SORTS = {"radius": (0, 1), "radii": (0, 1), "self": (0, 1), "box": (0,)}


@functools.lru_cache(maxsize=None)
def inputs(f64):
    """The cloud, the queries, one radius per query (a third of them 0) and the boxes; shared and read-only."""
    dtype = np.float64 if f64 else np.float32
    p = np.ascontiguousarray(ds.uniform_cloud(N_POINTS, 3, 41).astype(dtype))
    q = np.ascontiguousarray(ds.uniform_cloud(N_QUERIES, 3, 42).astype(dtype))
    radii = (RADIUS * (np.arange(N_QUERIES) % 3)).astype(dtype)
    lo, hi = np.ascontiguousarray(q - dtype(HALF)), np.ascontiguousarray(q + dtype(HALF))
    for a in (p, q, radii, lo, hi):
        a.flags.writeable = False
    return dict(p=p, q=q, radii=radii, lo=lo, hi=hi, dtype=np.dtype(dtype))


def without_self(off, flat):
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    own = flat["index"] == rows
    out = np.zeros(len(off), dtype=np.uint64)
    out[1:] = np.cumsum(np.diff(off.astype(np.int64)) - np.bincount(rows[own], minlength=len(off) - 1))
    return out, flat[~own]


@functools.lru_cache(maxsize=None)
def expected(kind, f64, sort):
    """(offsets, rows) of the mixed case: computed once and shared."""
    d = inputs(f64)
    if f64:
        ref = oracle.Oracle(d["p"], LEAF, "port", dtype=np.float64)
        if kind == "radius":
            return ref.search_radius(d["q"], RADIUS, sort=bool(sort))
        if kind == "self":
            return without_self(*ref.search_radius(d["p"], RADIUS, sort=bool(sort)))
        if kind == "box":
            return ref.search_box(d["lo"], d["hi"])
        # (one run per row, single-threaded: a call of one query is one OpenMP region, and oversubscribed regions take
        # seconds where this takes none; the thread count found is put back)
        threads = ref.max_threads()
        ref.set_threads(1)
        try:
            per_row = [ref.search_radius(d["q"][i:i + 1], d["radii"][i], sort=bool(sort))[1] for i in range(N_QUERIES)]
        finally:
            ref.set_threads(threads)
        off = np.zeros(N_QUERIES + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in per_row])
        return off, np.concatenate(per_row)
    lib = pt._load()
    host = pt.KdTree(d["p"], pt.Metric.L2Squared, LEAF, device=pt.PTK_DEVICE_NONE)
    n = N_POINTS if kind == "self" else N_QUERIES
    off, rows = np.zeros(n + 1, dtype=np.uint64), ctypes.c_void_p()
    p, q, o, r = d["p"].ctypes.data, d["q"].ctypes.data, off.ctypes.data, ctypes.byref(rows)
    if kind == "radius":
        rc = lib.ptk_host_search_radius(host._h, p, q, N_QUERIES, RADIUS, 1.0, sort, o, r)
    elif kind == "radii":
        rc = lib.ptk_host_search_radius_radii(host._h, p, q, N_QUERIES, d["radii"].ctypes.data, sort, o, r)
    elif kind == "self":
        rc = lib.ptk_host_search_radius_self(host._h, p, RADIUS, None, sort, o, r)
    else:
        rc = lib.ptk_host_search_box(host._h, p, d["lo"].ctypes.data, d["hi"].ctypes.data, N_QUERIES, o, r)
    assert rc == OK, lib.ptk_last_error()
    return off, pt._adopt(lib, rows, int(off[-1]), np.int32 if kind == "box" else pt.NEIGHBOR)


def row_dtype(kind, f64):
    return np.dtype(np.int32) if kind == "box" else np.dtype(pt.NEIGHBOR64 if f64 else pt.NEIGHBOR)


def call(tree, kind, f64, offsets, out, *, sort=0, n=None, q=None, radius=RADIUS, e=1.0, radii=None, lo=None, hi=None):
    """One entry point with the module's inputs unless the caller names others; `offsets` an address or None, `out` a
    c_void_p.  Returns the status."""
    lib, d = pt._load(), inputs(f64)
    fn = getattr(lib, FORM_IDS[FORMS.index((kind, f64))])
    n = N_QUERIES if n is None else n
    ptr = lambda a: a.ctypes.data  # noqa: E731
    if kind == "radius":
        return fn(tree._h, ptr(d["q"] if q is None else q), n, radius, e, sort, offsets, ctypes.byref(out))
    if kind == "radii":
        return fn(tree._h, ptr(d["q"] if q is None else q), n, ptr(d["radii"] if radii is None else radii), sort, offsets,
                  ctypes.byref(out))
    if kind == "self":
        return fn(tree._h, radius, None, sort, offsets, ctypes.byref(out))
    return fn(tree._h, ptr(d["lo"] if lo is None else lo), None if hi is None else ptr(hi), n, offsets, ctypes.byref(out))


def rows_of(out, total, dtype):
    """A copy of the records behind *out as they lie in memory, and the block given back to the library."""
    assert out.value, "*out is NULL after a call that succeeded"
    raw = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8)), (max(total, 1) * dtype.itemsize,))
    rows = raw[:total * dtype.itemsize].copy().view(dtype)
    pt._load().ptk_free(out)
    return rows


@pytest.fixture(scope="module")
def trees(gpu):
    return {f64: pt.KdTree(inputs(f64)["p"], pt.Metric.L2Squared, LEAF, device=gpu) for f64 in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,f64", FORMS, ids=FORM_IDS)
def test_mixed_rows(trees, kind, f64):
    """Rows both empty and not: offsets and rows are those of the reference, byte for byte, in both orders; the padding
    word of every float64 record is zero."""
    d, dtype = inputs(f64), row_dtype(kind, f64)
    n = N_POINTS if kind == "self" else N_QUERIES
    for sort in SORTS[kind]:
        want_off, want = expected(kind, f64, sort)
        lens = np.diff(want_off.astype(np.int64))
        assert (lens == 0).any() and (lens > 0).any(), "the case is not mixed"
        offsets, out = np.full(n + 1, 0xA5A5, dtype=np.uint64), ctypes.c_void_p(SENTINEL)
        hi = d["hi"] if kind == "box" else None
        assert call(trees[f64], kind, f64, offsets.ctypes.data, out, sort=sort, hi=hi) == OK, pt._load().ptk_last_error()
        assert offsets.tobytes() == want_off.tobytes(), (kind, f64, sort)
        got = rows_of(out, int(offsets[-1]), dtype)
        if kind == "box":
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (kind, f64)
            continue
        # (field by field: the oracle's float64 records carry whatever padding their buffer had)
        assert np.array_equal(got["index"], want["index"]), (kind, f64, sort)
        assert np.ascontiguousarray(got["distance"]).tobytes() == np.ascontiguousarray(want["distance"]).tobytes()
        if f64:
            assert not poison.record_bytes(got)[:, 4:8].any(), "the padding word of a record is not zero"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,f64", FORMS, ids=FORM_IDS)
def test_all_rows_empty(trees, kind, f64):
    """A radius of 0, boxes outside the cloud: PTK_OK, every offset 0, and a block ptk_free accepts."""
    d = inputs(f64)
    n = N_POINTS if kind == "self" else N_QUERIES
    offsets, out = np.full(n + 1, 0xA5A5, dtype=np.uint64), ctypes.c_void_p(0)
    zeros = np.zeros(N_QUERIES, dtype=d["dtype"])
    far_lo, far_hi = np.ascontiguousarray(d["lo"] + 10), np.ascontiguousarray(d["hi"] + 10)
    rc = call(trees[f64], kind, f64, offsets.ctypes.data, out, radius=0.0, radii=zeros, lo=far_lo,
              hi=far_hi if kind == "box" else None)
    assert rc == OK, pt._load().ptk_last_error()
    assert not offsets.any()
    assert out.value
    pt._load().ptk_free(out)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,f64", [f for f in FORMS if f[0] != "self"],
                         ids=[i for i, f in zip(FORM_IDS, FORMS) if f[0] != "self"])
def test_empty_batch(trees, kind, f64):
    """nq / nb = 0: PTK_OK, offsets[0] = 0 and no block.  (The self forms have no empty batch on a tree with points.)"""
    offsets, out = np.full(1, 0xA5A5, dtype=np.uint64), ctypes.c_void_p(SENTINEL)
    hi = inputs(f64)["hi"] if kind == "box" else None
    assert call(trees[f64], kind, f64, offsets.ctypes.data, out, n=0, hi=hi) == OK, pt._load().ptk_last_error()
    assert offsets[0] == 0 and out.value is None


@pytest.mark.gpu
@pytest.mark.parametrize("kind,f64", FORMS, ids=FORM_IDS)
def test_a_refused_call_leaves_no_block(trees, gpu, kind, f64):
    """*out preset to a sentinel: after a refusal it is NULL.  Null offsets for every form; e = 0 for the scalar radius
    forms, a 4-D tree for the per-row and the self forms, null maxs for the box forms."""
    d = inputs(f64)
    n = N_POINTS if kind == "self" else N_QUERIES
    hi = d["hi"] if kind == "box" else None
    out = ctypes.c_void_p(SENTINEL)
    assert call(trees[f64], kind, f64, None, out, hi=hi) == INVALID
    assert out.value is None
    offsets, out = np.zeros(n + 1, dtype=np.uint64), ctypes.c_void_p(SENTINEL)
    if kind == "radius":
        assert call(trees[f64], kind, f64, offsets.ctypes.data, out, e=0.0) == INVALID
    elif kind == "box":
        assert call(trees[f64], kind, f64, offsets.ctypes.data, out, hi=None) == INVALID
    else:
        p4 = np.ascontiguousarray(ds.uniform_cloud(N_POINTS, 4, 43).astype(d["dtype"]))
        tree4 = pt.KdTree(p4, pt.Metric.L2Squared, LEAF, device=gpu)
        offsets = np.zeros(N_POINTS + 1, dtype=np.uint64)
        assert call(tree4, kind, f64, offsets.ctypes.data, out, q=p4) == UNSUPPORTED
    assert out.value is None


@pytest.mark.gpu
def test_the_radius_capture_survives_the_per_row_and_the_self_form(trees, gpu):
    """ptk_search_radius_radii and ptk_search_radius_self between the count pass and the fill pass of a device pair on the
    same handle: the pair still gives the rows of the reference."""
    import torch

    lib, tree, d = pt._load(), trees[False], inputs(False)
    dev = f"cuda:{gpu}"
    dq = torch.from_numpy(d["q"].copy()).to(dev)
    stream = torch.cuda.current_stream(dq.device).cuda_stream
    counts = torch.zeros(N_QUERIES, dtype=torch.int64, device=dev)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), N_QUERIES, RADIUS, 1.0, counts.data_ptr(), stream) == OK
    for kind, n in (("radii", N_QUERIES), ("self", N_POINTS)):
        offsets, out = np.zeros(n + 1, dtype=np.uint64), ctypes.c_void_p(0)
        assert call(tree, kind, False, offsets.ctypes.data, out) == OK, lib.ptk_last_error()
        assert offsets.tobytes() == expected(kind, False, 0)[0].tobytes()
        lib.ptk_free(out)
    offsets = torch.zeros(N_QUERIES + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    total = int(offsets[-1])
    rows = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
    assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), N_QUERIES, RADIUS, 1.0, offsets.data_ptr(),
                                             rows.data_ptr(), 0, stream) == OK
    torch.cuda.synchronize()
    want_off, want = expected("radius", False, 0)
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want_off)
    assert np.ascontiguousarray(rows[:total].cpu().numpy()).tobytes() == np.ascontiguousarray(want).tobytes()
