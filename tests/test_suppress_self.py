"""suppress_within_self: greedy radius suppression of a tree's own points -- thinning to an r-separated subset, or
non-maximum suppression under the caller's scores (ptk.h).

Every expected value is a 0/1 array fixed by the contract.  ``expected_keep`` below is the contract written out -- the
keys, then one greedy pass in descending key -- applied to rows obtained independently of the feature: the compiled
reference's ``search_radius`` rows of the tree's own points with the own entry removed (the clouds and ``Case`` of
tests/test_radius_self.py, shared with it), or, on trees the reference cannot build (streams that do not belong to their
points, the constructed cases), the library's host loop ``ptk_host_search_radius``.  The constructed cases carry a second,
hand-written expectation.  Comparison is exact equality of the whole array.

The CPU tier checks the host loop on a host-only handle, the real kernel source in the emulator
(tests/cpp/emulate_suppress.cpp) under two schedules of what a lane sees in another point's cell, the C++ members
(tests/cpp/suppress_self_main.cpp) and the Python wrapper; the gpu tier checks the device rounds, float32 and float64.
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
METRICS = rs.METRICS
POISON8 = 0xA5

needs_reference = rs.needs_reference
needs_reference64 = rs.needs_reference64


# ---- the contract, written out ---------------------------------------------------------------------------------------

def fmix32(i):
    """The 32-bit finaliser of ptk.h over an array of indices."""
    h = np.asarray(i).astype(np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def keys_of(n, scores):
    """key(i) = (ord_i << 32) | (0xFFFFFFFF - i) as uint64; ``scores`` None: ord_i = fmix32(i), else the total-order map
    of the bits of the float32 score."""
    i = np.arange(n, dtype=np.uint64)
    if scores is None:
        ord_ = fmix32(i)
    else:
        b = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
        ord_ = np.where(b & 0x80000000 != 0, b ^ 0xFFFFFFFF, b ^ 0x80000000)
    return (ord_ << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - i)


def expected_keep(off, flat, scores=None):
    """keep of the rows (offsets, flat records with an ``index`` field; own entries already removed): one greedy pass in
    descending key.  keep[i] = 1 iff row i holds no j with key(j) > key(i) and keep[j] == 1."""
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    idx = np.asarray(flat["index"]).astype(np.int64)
    key = keys_of(n, scores)
    assert len(np.unique(key)) == n
    keep = np.zeros(n, dtype=np.uint8)
    for i in np.argsort(key)[::-1].tolist():
        row = idx[off[i]:off[i + 1]]
        keep[i] = 0 if np.any((key[row] > key[i]) & (keep[row] == 1)) else 1
    return keep


SCORE_KINDS = (None, "random", "levels", "special")


@functools.lru_cache(maxsize=None)
def _scores(n, kind):
    rng = np.random.default_rng(4242 + n)
    if kind is None:
        return None
    if kind == "random":
        s = rng.standard_normal(n).astype(np.float32)
    elif kind == "levels":  # four levels: most comparisons are index tie-breaks
        s = rng.integers(0, 4, n).astype(np.float32)
    elif kind == "special":  # both zeros, both infinities, and values on either side of them
        s = np.array([-0.0, 0.0, np.inf, -np.inf, 1.0, -1.0, np.finfo(np.float32).smallest_subnormal,
                      -np.finfo(np.float32).max], dtype=np.float32)[rng.integers(0, 8, n)]
    else:
        raise ValueError(kind)
    s.flags.writeable = False
    return s


def scores_of(n, kind):
    return _scores(int(n), kind)


@functools.lru_cache(maxsize=None)
def _want_scalar(kind, metric, dtype, r, sk):
    c = rs.case(kind, metric, dtype)
    out = expected_keep(*c.want(c.dtype.type(r)), scores_of(c.n, sk))
    out.flags.writeable = False
    return out


def want_scalar(c, r, sk):
    """Expected keep of a Case at the scalar radius r under a kind of scores: computed once, shared by the tiers."""
    return _want_scalar(c.kind, c.metric, c.dtype.name, float(r), sk)


@functools.lru_cache(maxsize=None)
def _want_radii(kind, metric, dtype, sk):
    c = rs.case(kind, metric, dtype)
    out = expected_keep(*c.want_per_row(), scores_of(c.n, sk))
    out.flags.writeable = False
    return out


def want_radii(c, sk):
    return _want_radii(c.kind, c.metric, c.dtype.name, sk)


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


def guarded_cells(n):
    """(whole buffer, the n cells) of a uint8 output between two runs of guard entries, all 0xA5 bytes."""
    return rs.guarded(n, np.uint8)


def written(buf, keep):
    """Every cell holds 0 or 1 (no poison, no "undecided" left behind), nothing was written outside."""
    return rs.guards_intact(buf) and bool(np.all(keep <= 1))


def _ptr(a):
    return None if a is None else a.ctypes.data


def host_keep(tree, r, scores=None, points=None):
    """ptk_host_suppress_within_self into a guarded buffer; r a scalar or an array."""
    lib = pt._load()
    p = tree._pts if points is None else points
    buf, keep = guarded_cells(len(p))
    n_kept = ctypes.c_uint64(12345)
    scalar = np.ndim(r) == 0
    rc = lib.ptk_host_suppress_within_self(tree._h, p.ctypes.data, np.float32(r if scalar else 0),
                                           None if scalar else r.ctypes.data, _ptr(scores), keep.ctypes.data,
                                           ctypes.byref(n_kept))
    assert rc == 0, lib.ptk_last_error()
    assert written(buf, keep), "a cell was not written, or one was written outside"
    assert n_kept.value == int(keep.sum())
    return keep.copy()


def separated_and_maximal(off, flat, keep):
    """Straight from the rows, independent of expected_keep: no kept point has a kept point in its row, and every
    suppressed point has one."""
    off = np.asarray(off).astype(np.int64)
    row, idx = rs.row_ids(off), np.asarray(flat["index"]).astype(np.int64)
    kept = keep.astype(bool)
    kept_in_row = np.bincount(row[kept[idx]], minlength=len(keep))
    return bool(np.all(kept_in_row[kept] == 0)), bool(np.all(kept_in_row[~kept] > 0))


# ---- the contract's own arithmetic -----------------------------------------------------------------------------------

def test_the_keys_of_the_contract():
    """The finaliser on values known from its source (MurmurHash3's fmix32), the order of the score map, the tie-break."""
    assert fmix32(np.array([0, 1, 2, 0xFFFFFFFF])).tolist() == [0, 0x514E28B7, 0x30F4C306, 0x81F16F39]
    assert len(np.unique(fmix32(np.arange(1 << 16)))) == 1 << 16
    s = np.array([-np.inf, -1.0, -0.0, 0.0, np.finfo(np.float32).smallest_subnormal, 1.0, np.inf], dtype=np.float32)
    k = keys_of(len(s), s)
    assert np.all(k[1:] > k[:-1])  # ascending scores, ascending keys: -0.0 below +0.0, the infinities at the ends
    k = keys_of(4, np.zeros(4, dtype=np.float32))
    assert np.all(k[1:] < k[:-1])  # an equal score is decided by the LOWER index
    # the greedy pass on rows written by hand: 0 - 1 - 2 - 3 in a line, each next to its neighbours, scores descending
    off = np.array([0, 1, 3, 5, 6], dtype=np.uint64)
    flat = np.zeros(6, dtype=pt.NEIGHBOR)
    flat["index"] = [1, 0, 2, 1, 3, 2]
    assert expected_keep(off, flat, np.array([4, 3, 2, 1], dtype=np.float32)).tolist() == [1, 0, 1, 0]
    assert expected_keep(off, flat, np.array([1, 2, 3, 4], dtype=np.float32)).tolist() == [0, 1, 0, 1]
    assert expected_keep(off, flat, np.array([1, 4, 3, 2], dtype=np.float32)).tolist() == [0, 1, 0, 1]


# ---- CPU tier: the host loop on a host-only handle -------------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "5d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_equals_the_expected_keep(kind, metric):
    c = rs.case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    for r in own_radii(c):
        for sk in SCORE_KINDS:
            got = host_keep(tree, r, scores_of(c.n, sk))
            assert np.array_equal(got, want_scalar(c, r, sk)), (kind, metric, r, sk)
            if r == 0:
                assert np.all(got == 1)  # (radius 0 keeps everything)
            if metric in ("L2Squared", "L1"):  # symmetric rows: a maximal r-separated subset
                assert separated_and_maximal(*c.want(r), got) == (True, True), (kind, metric, r, sk)
    radii = c.radii()
    for sk in SCORE_KINDS:
        assert np.array_equal(host_keep(tree, radii, scores_of(c.n, sk)), want_radii(c, sk)), (kind, metric, "per row", sk)


@needs_reference
def test_the_expected_keep_tells_the_rules_apart():
    """On the data of this module the pieces of the contract all matter: points are suppressed and kept, the orders
    differ, ties between equal scores occur inside rows, and the per-point radii give asymmetric rows."""
    c = rs.case("lidar", "L2Squared")
    r = own_radii(c)[1]
    off, flat = c.want(r)
    row, idx = rs.row_ids(off), flat["index"].astype(np.int64)
    wants = [want_scalar(c, r, sk) for sk in SCORE_KINDS]
    for w in wants:
        assert 0.05 * c.n < w.sum() < 0.95 * c.n
    for a in range(len(wants)):
        for b in range(a + 1, len(wants)):
            assert not np.array_equal(wants[a], wants[b]), (SCORE_KINDS[a], SCORE_KINDS[b])
    levels = scores_of(c.n, "levels")
    assert np.mean(levels[row] == levels[idx]) > 0.15, "few ties inside rows: the index tie-break is not exercised"
    special = scores_of(c.n, "special")
    zeros = (special[row] == 0) & (special[idx] == 0)
    assert np.any(np.signbit(special[row][zeros]) != np.signbit(special[idx][zeros])), "no -0.0 next to a +0.0"
    # index order in place of the hashed default would give another array
    in_index_order = expected_keep(off, flat, -np.arange(c.n, dtype=np.float32))
    assert not np.array_equal(in_index_order, wants[0])
    off, flat = c.want_per_row()
    row, idx = rs.row_ids(off), flat["index"].astype(np.int64)
    forward = set((row * c.n + idx).tolist())
    assert any((j * c.n + i) not in forward for i, j in zip(row.tolist(), idx.tolist())), "the rows are symmetric"


@needs_reference
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "LPInf"])
def test_exactly_one_point_of_a_pile_is_kept_on_ties(metric):
    """"ties" at the grid step exactly (strict: the grid neighbours stay out): a row holds the coincident points and
    nothing else, so of every pile exactly one point is kept -- the one of highest key."""
    c = rs.case("ties", metric)
    r = c.values()[3]
    off, flat = c.want(r)
    assert np.all(flat["distance"] == 0) and len(flat) > 0
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    _, pile = np.unique(c.p, axis=0, return_inverse=True)
    pile = pile.reshape(-1)
    sizes = np.bincount(pile)
    assert sizes.max() > 3
    for sk in SCORE_KINDS:
        got = host_keep(tree, r, scores_of(c.n, sk))
        assert np.all(np.bincount(pile, weights=got) == 1), (metric, sk)
        key = keys_of(c.n, scores_of(c.n, sk))
        best = np.zeros(len(sizes), dtype=np.uint64)
        np.maximum.at(best, pile, key)
        assert np.array_equal(got == 1, key == best[pile]), (metric, sk)


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
        loop = host_search_rows(tree, p, r)  # (rows from ptk_host_search_radius_self's loop: the same rows)
        assert np.array_equal(rows[0], loop[0]) and np.array_equal(rows[1]["index"], loop[1]["index"])
        for sk in (None, "random", "levels"):
            s = scores_of(len(p), sk)
            assert np.array_equal(host_keep(tree, r, s), expected_keep(*rows, s)), (metric, r, sk)


# ---- the constructed cases -------------------------------------------------------------------------------------------

def chain(n):
    """n collinear points at spacing 1 (1-D); with radius 1.5^2 under L2Squared each point's row is its two neighbours."""
    return np.ascontiguousarray(np.arange(n, dtype=np.float32).reshape(-1, 1))


CHAIN_R = np.float32(1.5 * 1.5)


def pile_cloud():
    """200 coincident points and 50 scattered ones (3-D); point 0 is a scattered one."""
    p = ds.uniform_cloud(250, 3, 44)
    pile = np.arange(250) % 5 != 0  # 200 of them
    p[pile] = np.float32(0.5)
    return np.ascontiguousarray(p), pile


class ByHostLoop:
    """keep(tree, points, r, scores) through ptk_host_suppress_within_self on a host-only handle."""
    chain_n = 600

    def tree(self, p, metric, leaf):
        return pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)

    def keep(self, tree, p, r, scores=None):
        return host_keep(tree, r, scores)


def check_constructed(how):
    """The chain, the pile and the tiny trees through `how` (the host loop, the emulator, the device): against the
    hand-written arrays and against the contract applied to the host loop's rows."""
    # the chain with scores descending along the line: point k waits for point k - 1 -- the even indices, after as many
    # rounds as the bound allows
    n = how.chain_n
    p = chain(n)
    tree = how.tree(p, "L2Squared", 4)
    rows = host_search_rows(tree, p, CHAIN_R)
    assert np.array_equal(np.diff(rows[0].astype(np.int64)), [1] + [2] * (n - 2) + [1])
    descending = np.arange(n, 0, -1).astype(np.float32)
    got = how.keep(tree, p, CHAIN_R, descending)
    assert np.array_equal(got, (np.arange(n) % 2 == 0).astype(np.uint8)), np.flatnonzero(got != (np.arange(n) % 2 == 0))[:5]
    assert np.array_equal(got, expected_keep(*rows, descending))
    rounds = getattr(how, "last_rounds", None)
    if rounds is not None:
        assert 1 <= rounds <= n, rounds
    # ascending: the mirror image (the last point is kept)
    ascending = np.arange(n).astype(np.float32)
    assert np.array_equal(how.keep(tree, p, CHAIN_R, ascending), ((n - 1 - np.arange(n)) % 2 == 0).astype(np.uint8))
    # the default order
    got = how.keep(tree, p, CHAIN_R)
    assert np.array_equal(got, expected_keep(*rows, None))
    assert separated_and_maximal(*rows, got) == (True, True)
    # a radius that reaches nothing (strict: the neighbour AT distance 1 stays out): everything is kept
    assert np.all(how.keep(tree, p, np.float32(1.0), descending) == 1)
    # a pile of coincident points away from everything else: one of it is kept at any r > 0 -- the one of highest key --,
    # all of it at r = 0
    p, pile = pile_cloud()
    tree = how.tree(p, "L2Squared", 3)
    for r in (np.float32(1e-30), np.float32(1e-6), np.finfo(np.float32).smallest_subnormal):
        for s in (None, scores_of(len(p), "levels")):
            got = how.keep(tree, p, r, s)
            key = keys_of(len(p), s)
            best = np.flatnonzero(pile)[np.argmax(key[pile])]
            assert got[pile].sum() == 1 and got[best] == 1 and np.all(got[~pile] == 1), (r, s is None)
    assert np.all(how.keep(tree, p, np.float32(0)) == 1)
    # n = 1, 2, 3
    for n in (1, 2, 3):
        p = ds.uniform_cloud(n, 3, 21)
        tree = how.tree(p, "L2Squared", 3)
        for r in (0.0, 0.05, 10.0, INF):
            rows = host_search_rows(tree, p, np.float32(r))
            for s in (None, np.arange(n, dtype=np.float32), np.zeros(n, dtype=np.float32)):
                assert np.array_equal(how.keep(tree, p, np.float32(r), s), expected_keep(*rows, s)), (n, r)
        # every row holds every other point: the point of highest key alone
        assert how.keep(tree, p, np.float32(INF), np.arange(n, dtype=np.float32)).tolist() == [0] * (n - 1) + [1]
        assert how.keep(tree, p, np.float32(INF), np.zeros(n, dtype=np.float32)).tolist() == [1] + [0] * (n - 1)


def test_constructed_cases_on_the_host_loop():
    check_constructed(ByHostLoop())


def test_a_tree_holds_at_least_one_point():
    """n_points == 0 succeeds in every form (ptk.h) -- and no handle of this library has 0 points: the build refuses."""
    with pytest.raises(pt.PtkError):
        pt.KdTree(np.zeros((0, 3), dtype=np.float32), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)


def test_argument_checks_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    keep = np.zeros(9, dtype=np.uint8)
    ok = np.full(9, 0.1, dtype=np.float32)
    n_kept, n_rounds = ctypes.c_uint64(0), ctypes.c_uint32(0)
    INVALID, DEVICE = -1, -3
    host = lib.ptk_host_suppress_within_self
    assert host(tree._h, p.ctypes.data, np.float32(0.1), None, None, None, None) == INVALID
    assert host(tree._h, None, np.float32(0.1), None, None, keep.ctypes.data, None) == INVALID
    assert host(None, p.ctypes.data, np.float32(0.1), None, None, keep.ctypes.data, None) == INVALID
    assert host(tree._h, p.ctypes.data, np.float32(0.1), None, None, keep.ctypes.data, None) == 0  # (n_kept may be null)
    for bad in (np.nan, -0.5, -INF):
        assert host(tree._h, p.ctypes.data, np.float32(bad), None, None, keep.ctypes.data, None) == INVALID
        assert "radius must be >= 0" in lib.ptk_last_error().decode()
        assert host(tree._h, p.ctypes.data, np.float32(bad), ok.ctypes.data, None, keep.ctypes.data, None) == 0
    for bad in (np.nan, -1e-3):
        radii = ok.copy()
        radii[4] = radii[7] = bad
        assert host(tree._h, p.ctypes.data, np.float32(1), radii.ctypes.data, None, keep.ctypes.data, None) == INVALID
        assert "radii[4]" in lib.ptk_last_error().decode()
    scores = ok.copy()
    scores[3] = scores[8] = np.nan
    assert host(tree._h, p.ctypes.data, np.float32(1), None, scores.ctypes.data, keep.ctypes.data, None) == INVALID
    assert "scores[3]" in lib.ptk_last_error().decode()
    scores[3] = scores[8] = np.inf  # (an infinity is an ordinary value)
    assert host(tree._h, p.ctypes.data, np.float32(1), None, scores.ctypes.data, keep.ctypes.data, None) == 0
    # a host-only handle has no device search: PTK_ERR_DEVICE from every device entry point
    assert lib.ptk_suppress_within_self(tree._h, np.float32(0.1), None, None, keep.ctypes.data, ctypes.byref(n_kept),
                                        ctypes.byref(n_rounds)) == DEVICE
    assert lib.ptk_suppress_within_self_device(tree._h, np.float32(0.1), None, None, keep.ctypes.data, None, None) == DEVICE
    assert lib.ptk_suppress_within_self(None, np.float32(0.1), None, None, keep.ctypes.data, None, None) == INVALID
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    assert lib.ptk_search64_suppress_within_self(t64._h, 0.1, None, None, keep.ctypes.data, None, None) == DEVICE
    assert lib.ptk_search64_suppress_within_self_device(t64._h, 0.1, None, None, keep.ctypes.data, None, None) == DEVICE
    assert lib.ptk_search64_suppress_within_self(None, 0.1, None, None, keep.ctypes.data, None, None) == INVALID
    assert lib.ptk_version() == 101


def test_the_wrapper_checks_its_arguments_and_shapes_its_result(monkeypatch):
    """The Python wrapper's own work: the checks of radius and scores, bool / indices results, last_suppress_rounds (the
    host loop serves a host-only handle here in place of the device form)."""
    p, pile = pile_cloud()
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    n = len(p)
    with pytest.raises(pt.PtkError) as refused:
        tree.suppress_within_self(0.1)
    assert refused.value.status == -3  # PTK_ERR_DEVICE
    for bad in (np.zeros(n - 1, dtype=np.float32), np.zeros((n, 1), dtype=np.float32), "x"):
        with pytest.raises(ValueError):
            tree.suppress_within_self(bad)
        with pytest.raises(ValueError):
            tree.suppress_within_self(0.1, scores=bad)
    nan = np.zeros(n, dtype=np.float32)
    nan[17] = nan[40] = np.nan
    with pytest.raises(ValueError, match=r"scores\[17\]"):
        tree.suppress_within_self(0.1, scores=nan)
    with pytest.raises(ValueError):
        tree.suppress_within_self(0.1, scores=np.full(n, 1e300))  # (does not fit the float32 of the key)
    lib = pt._load()

    class Served:  # the device entry point of a host-only handle, answered by the host loop
        def __getattr__(self, name):
            if name == "ptk_suppress_within_self":
                def served(h, r, rp, sp, keep, n_kept, n_rounds):
                    ctypes.cast(n_rounds, ctypes.POINTER(ctypes.c_uint32))[0] = 7
                    return lib.ptk_host_suppress_within_self(h, p.ctypes.data, r, rp, sp, keep, n_kept)
                return served
            return getattr(lib, name)

    monkeypatch.setattr(pt, "_load", lambda: Served())
    levels = scores_of(n, "levels")
    for r, s in ((1e-6, None), (1e-6, levels), (0.0, None), (0.02, levels), (0.02, levels.astype(np.float64)),
                 (0.02, levels.astype(np.int64).tolist())):
        plain = tree.suppress_within_self(r, scores=s)
        assert plain.dtype == np.bool_ and plain.shape == (n,)
        want = host_keep(tree, np.float32(r), None if s is None else levels)
        assert np.array_equal(plain, want == 1)
        kept = tree.suppress_within_self(r, scores=s, indices=True)
        assert kept.dtype == np.int64 and np.array_equal(kept, np.flatnonzero(want))
        assert tree.last_suppress_rounds == 7
    radii = np.full(n, 1e-6, dtype=np.float32)
    radii[::2] = 0
    assert np.array_equal(tree.suppress_within_self(radii), host_keep(tree, radii) == 1)
    import pico_tree

    assert pico_tree.KdTree.suppress_within_self is pt.KdTree.suppress_within_self


# ---- CPU tier: the C++ members on a host-only build --------------------------------------------------------------------

def _cpp_inputs(d):
    p = ds.uniform_cloud(4_000, 3, 91)
    p[::5] = np.round(p[::5] * 4) / 4 * np.float32(0.999)  # a fifth snapped to a grid: coincident points
    p.tofile(os.path.join(d, "points.bin"))
    r = np.float32(0.004)
    radii = np.full(len(p), r, dtype=np.float32)
    radii[3::50] = 0
    radii[7::90] = np.float32(0.02)
    radii.tofile(os.path.join(d, "radii.bin"))
    scores = np.array(scores_of(len(p), "levels"))
    scores.tofile(os.path.join(d, "scores.bin"))
    return p, r, radii, scores


def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "suppress_self_main.cpp"), "-o", out]
    if host_only:
        cmd.insert(1, "-DPICO_TREE_HOST_ONLY")
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def _check_cpp_output(d, p, r, radii, scores):
    def got(name):
        return np.fromfile(os.path.join(d, name + ".u8"), dtype=np.uint8)

    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=pt.PTK_DEVICE_NONE)
    tree_l1 = pt.KdTree(p, pt.Metric.L1, 10, device=pt.PTK_DEVICE_NONE)
    for name, t in (("l2", tree), ("l1", tree_l1)):
        for rows, form in ((host_search_rows(t, p, r), "scalar"), (host_search_rows(t, p, radii), "radii")):
            assert np.array_equal(got(f"{name}_{form}"), expected_keep(*rows, None)), (name, form)
            scored = "scored" if form == "scalar" else "radii_scored"
            assert np.array_equal(got(f"{name}_{scored}"), expected_keep(*rows, scores)), (name, scored)
    assert 0.3 * len(p) < got("l2_scalar").sum() < len(p)
    if oracle.have_reference64():
        pd = p.astype(np.float64)
        ref = oracle.Oracle(pd, 10, "reference", dtype=np.float64)
        rows = rs.without_self(*ref.search_radius(pd, np.float64(r)))
        assert np.array_equal(got("l2d_scalar"), expected_keep(*rows, None))
        assert np.array_equal(got("l2d_scored"), expected_keep(*rows, scores))


def test_cpp_members_on_a_host_only_tree(tmp_path):
    d = str(tmp_path)
    p, r, radii, scores = _cpp_inputs(d)
    exe = os.path.join(d, "suppress_self_main")
    _cpp_program(exe, host_only=True)
    res = subprocess.run([exe, d, repr(float(r))], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
    _check_cpp_output(d, p, r, radii, scores)


# ---- CPU tier: the real kernel source in the emulator ----------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/cpp/emulate_suppress.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_suppress") / "libptk_emu_suppress.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_suppress.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.emu_create.restype = vp
    lib.emu_create.argtypes = [vp, u64, ctypes.c_uint32, vp, u64, vp]
    lib.emu_destroy.argtypes = [vp]
    lib.emu_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu_suppress_self.argtypes = [vp, u64, ctypes.c_float, vp, vp, ctypes.c_int, vp]
    lib.emu64_create.restype = vp
    lib.emu64_create.argtypes = [vp, u64, ctypes.c_uint32, u64]
    lib.emu64_destroy.argtypes = [vp]
    lib.emu64_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu64_suppress_self.argtypes = [vp, u64, ctypes.c_double, vp, vp, ctypes.c_int, vp]
    return lib


def emu_keep(emu, r, scores=None, piece=64, snapshot=0, rounds=None):
    """The rounds over an rs.Emulated tree into a poisoned, guarded buffer: every cell decided, nothing written outside.
    `rounds`: a list the number of rounds is appended to."""
    buf, keep = guarded_cells(emu.n)
    scalar = np.ndim(r) == 0
    n_rounds = emu.lib.emu_suppress_self(emu.h, piece, np.float32(r if scalar else 0), None if scalar else r.ctypes.data,
                                         _ptr(scores), snapshot, keep.ctypes.data)
    assert 1 <= n_rounds <= emu.n, n_rounds  # (0: the bound of n_points rounds did not end it)
    assert written(buf, keep), "a cell was not decided, or one was written outside"
    if rounds is not None:
        rounds.append(n_rounds)
    return keep.copy()


def emu_both(emu, r, scores=None, piece=64):
    """Both schedules -- cells read live, cells read from a snapshot taken at the start of each round, the stalest view
    the memory model allows -- must give one array; the stale one never needs fewer rounds."""
    rounds = []
    live = emu_keep(emu, r, scores, piece, 0, rounds)
    stale = emu_keep(emu, r, scores, piece, 1, rounds)
    assert np.array_equal(live, stale), "the result depends on what a load happens to see"
    assert rounds[0] <= rounds[1], rounds
    return live


class ByEmulator:
    def __init__(self, lib):
        self.lib = lib
        self.turn = 0
        self.chain_n = 300
        self.last_rounds = None

    def tree(self, p, metric, leaf):
        emu = rs.Emulated(self.lib, p, leaf, metric)
        emu._pts, emu._h = emu.host._pts, emu.host._h  # (host_search_rows takes the host tree of the same points)
        return emu

    def keep(self, emu, p, r, scores=None):
        self.turn += 1  # the pieces take turns
        rounds = []
        got = emu_keep(emu, r, scores, (64, 0, 647)[self.turn % 3], 0, rounds)
        stale = emu_keep(emu, r, scores, (0, 64)[self.turn % 2], 1, rounds)
        assert np.array_equal(got, stale)
        self.last_rounds = rounds[1]
        return got


@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_kernels_equal_the_expected_keep(emu_lib, kind, metric):
    """Scalar and per-row, every kind of scores; pieces of 64 leaf positions (every launch one wavefront, a ragged last
    one), 647 (pieces that end inside a wavefront) and the whole tree; both schedules."""
    c = rs.case(kind, metric)
    emu = rs.Emulated(emu_lib, c.p, c.leaf, metric)
    for r in own_radii(c):
        for sk, piece in ((None, 64), ("random", 647), ("levels", 64), ("special", 0)):
            got = emu_both(emu, r, scores_of(c.n, sk), piece)
            assert np.array_equal(got, want_scalar(c, r, sk)), (kind, metric, r, sk, piece)
    radii = c.radii()
    for sk, piece in ((None, 647), ("levels", 64)):
        assert np.array_equal(emu_both(emu, radii, scores_of(c.n, sk), piece), want_radii(c, sk)), (kind, metric, sk)


@needs_reference
def test_emulated_rounds_are_few_in_the_default_order_and_many_in_index_order(emu_lib):
    """Information, not contract -- but the reason the default order is hashed: on a cloud sorted along an axis the
    index order needs many times the rounds of the hashed one, under the stale schedule above all."""
    c = rs.case("uniform", "L2Squared")
    order = np.argsort(c.p[:, 0], kind="stable")
    p = np.ascontiguousarray(c.p[order])
    emu = rs.Emulated(emu_lib, p, c.leaf, "L2Squared")
    r = own_radii(c)[2]
    rows = host_search_rows(emu.host, p, r)
    hashed, by_index = [], []
    got = emu_keep(emu, r, None, 0, 1, hashed)
    assert np.array_equal(got, expected_keep(*rows, None))
    s = -np.arange(len(p), dtype=np.float32)
    got = emu_keep(emu, r, s, 0, 1, by_index)
    assert np.array_equal(got, expected_keep(*rows, s))
    print("rounds, stale schedule: hashed", hashed[0], "index order", by_index[0])
    assert by_index[0] > hashed[0], (hashed, by_index)


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_kernels_where_the_leaf_scan_changes(emu_lib, L):
    """The CPU half of tests/test_leaf_boundaries.py for this kernel: a tree whose largest leaf has exactly 31 | 32 | 33
    and 64 | 65 points; at the radius that holds the whole leaf exactly one of its points is kept."""
    pts, blob, q, nb, ref, radii = leaf_cases.case(L)
    pts = np.asarray(pts)
    emu = rs.Emulated(emu_lib, pts, L, "L2Squared")
    leaf_cases.assert_leaf(emu.host, L)
    for r in leaf_cases.self_radii(L, radii):
        rows = leaf_cases.self_rows(ref, pts, r)
        for sk, piece in ((None, 64), ("levels", 647)):
            s = scores_of(len(pts), sk)
            got = emu_both(emu, r, s, piece)
            assert np.array_equal(got, expected_keep(*rows, s)), (L, r, sk, piece)
        if r == radii[1]:
            assert got[len(pts) - L:].sum() == 1


@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "ties", "1d"])
@pytest.mark.parametrize("metric", METRICS)
def test_emulated_float64_kernels_equal_the_expected_keep(emu_lib, kind, metric):
    c = rs.case(kind, metric, "float64")
    lib = emu_lib
    h = lib.emu64_create(c.p.ctypes.data, c.n, c.p.shape[1], c.leaf)
    assert h
    try:
        lib.emu64_set_metric(h, rs._EMU_METRIC[metric])

        def keep(r, s, piece, snapshot):
            buf, out = guarded_cells(c.n)
            scalar = np.ndim(r) == 0
            rounds = lib.emu64_suppress_self(h, piece, float(r) if scalar else 0.0, None if scalar else r.ctypes.data,
                                             _ptr(s), snapshot, out.ctypes.data)
            assert 1 <= rounds <= c.n and written(buf, out)
            return out.copy()

        for r in own_radii(c):
            for sk, piece in ((None, 64), ("random", 647), ("levels", 0), ("special", 64)):
                s = scores_of(c.n, sk)
                live = keep(r, s, piece, 0)
                assert np.array_equal(live, keep(r, s, piece, 1)), (kind, metric, r, sk, "schedules")
                assert np.array_equal(live, want_scalar(c, r, sk)), (kind, metric, r, sk)
        radii = c.radii()
        for sk, piece in ((None, 64), ("levels", 647)):
            s = scores_of(c.n, sk)
            live = keep(radii, s, piece, 0)
            assert np.array_equal(live, keep(radii, s, piece, 1))
            assert np.array_equal(live, want_radii(c, sk)), (kind, metric, "per row", sk)
    finally:
        lib.emu64_destroy(h)


def test_emulated_kernels_on_the_constructed_cases(emu_lib):
    how = ByEmulator(emu_lib)
    check_constructed(how)


def test_emulated_chain_takes_every_round_the_bound_allows(emu_lib):
    """The chain with descending scores under the stale schedule: point k is decided in round k + 1 -- n rounds, the
    bound of ptk.h reached."""
    n = 200
    p = chain(n)
    emu = rs.Emulated(emu_lib, p, 4, "L2Squared")
    rounds = []
    got = emu_keep(emu, CHAIN_R, np.arange(n, 0, -1).astype(np.float32), 64, 1, rounds)
    assert np.array_equal(got, (np.arange(n) % 2 == 0).astype(np.uint8)) and rounds == [n]


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
    """The rows of such a stream are asymmetric: a point looks at its OWN row only.  Expected: the contract over the
    host loop's rows of the same tree and points pair; the host loop of the feature on that pair as well."""
    p_tree, p = foreign_stream(move)
    emu = rs.Emulated(emu_lib, p, 8, metric, tree_points=p_tree)
    asym = 0
    for r in (0.01, 0.05, 0.3):
        rows = host_search_rows(emu.host, p, np.float32(r))
        asym += asymmetric_pairs(*rows)
        for sk, piece in ((None, 647), ("levels", 64)):
            s = scores_of(len(p), sk)
            want = expected_keep(*rows, s)
            assert np.array_equal(emu_both(emu, r, s, piece), want), (metric, move, r, sk)
            assert np.array_equal(host_keep(emu.host, r, s, points=p), want), (metric, move, r, sk, "host loop")
    assert asym > 0, "every row is symmetric: the stream tells nothing apart"


def test_emulated_kernels_on_a_stream_with_non_finite_points(emu_lib):
    p_tree, leaf = rs.cloud("uniform")
    p = np.array(p_tree)
    p[700, 1], p[1900, 0] = np.nan, np.inf
    emu = rs.Emulated(emu_lib, p, leaf, "L2Squared", tree_points=p_tree)
    for r in (0.01, 0.1):
        rows = host_search_rows(emu.host, p, np.float32(r))
        for sk, piece in ((None, 0), ("random", 647)):
            s = scores_of(len(p), sk)
            assert np.array_equal(emu_both(emu, r, s, piece), expected_keep(*rows, s)), (r, sk)


def empty_rows(off, flat, rows):
    """(offsets, flat) with the given rows emptied."""
    keep = ~np.isin(rs.row_ids(off), rows)
    lens = np.diff(np.asarray(off).astype(np.int64))
    assert np.all(lens[rows] > 0)
    lens[rows] = 0
    off2 = np.zeros(len(off), dtype=np.uint64)
    off2[1:] = np.cumsum(lens)
    return off2, flat[keep]


def test_emulated_per_row_radii_that_pass_no_test_and_nan_scores(emu_lib):
    """A NaN and a negative radii entry (the _device forms cannot look): the row is empty -- the point is kept -- and the
    point still suppresses others through their rows.  A NaN score takes the place its bits give it under ord."""
    p, leaf = rs.cloud("uniform")
    emu = rs.Emulated(emu_lib, p, leaf, "L2Squared")
    radii = np.full(len(p), 0.01, dtype=np.float32)
    rows = host_search_rows(emu.host, p, radii)
    bad = radii.copy()
    bad[100], bad[2000] = np.nan, -1.0
    scores = np.array(scores_of(len(p), "random"))
    scores[[5, 100, 777]] = np.nan
    scores[888] = -np.nan
    assert np.signbit(scores[888]) and not np.signbit(scores[5])
    key = keys_of(len(p), scores)
    numbers = ~np.isnan(scores)
    assert key[5] > key[numbers].max() and key[888] < key[numbers].min()  # (above +inf's place, below -inf's)
    for s in (None, scores):
        got = emu_both(emu, bad, s, 647)
        assert np.array_equal(got, expected_keep(*empty_rows(*rows, [100, 2000]), s))
        assert got[100] == 1 and got[2000] == 1
    # (still a neighbour: some point of lower key next to point 100 is suppressed by it)
    got = emu_both(emu, bad, scores, 64)
    off, flat = empty_rows(*rows, [100, 2000])
    holders = np.flatnonzero(np.bincount(rs.row_ids(off)[flat["index"] == 100], minlength=len(p)))
    assert len(holders) > 0 and np.all(got[holders] == 0)


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 10, "L2Squared"), (2, 4, "L1")])
def test_emulated_kernels_where_the_stack_class_changes(emu_lib, dim, leaf, metric, depth):
    """Trees of exactly 39 | 40 and 135 | 136 levels (tests/depth_cases.py): the pile of coincident points walks the chain
    of one-point peels.  The record stacks stay within 2 * depth + 2 and within what the host's spill class for the depth
    holds.  At r = 1e4 every row holds every other point: the point of highest key alone is kept."""
    pts, _ = depth_cases.cloud_at_depth(depth, dim, leaf)
    pts = np.asarray(pts)
    ref = oracle.Oracle(pts, leaf, "reference", metric=metric)
    emu = rs.Emulated(emu_lib, pts, leaf, metric)
    run = depth_cases.Watch(depth, emu_lib)
    rows = rs.without_self(*ref.search_radius(pts, np.float32(0.05)))
    n_pile = len(pts) - 3_000
    assert np.all(rs.clamp(rows[0], 0)[3_000:] >= n_pile - 1)
    highs = []
    # (ascending scores: the pile's last point is its best -- every other point of the pile walks to the chain's end)
    for s in (None, np.arange(len(pts), dtype=np.float32)):
        got = run(emu_keep, emu, np.float32(0.05), s, 647)
        highs.append(run.high)
        assert np.array_equal(got, expected_keep(*rows, s)), (depth, s is None)
        assert got[3_000:].sum() <= 1
    for s in (None, np.arange(len(pts), dtype=np.float32)):
        got = run(emu_keep, emu, np.float32(1e4), s, 0, 1)
        highs.append(run.high)
        best = int(np.argmax(keys_of(len(pts), s)))
        assert got.sum() == 1 and got[best] == 1, (depth, s is None)
    assert min(highs) > depth, highs


# ---- gpu tier ---------------------------------------------------------------------------------------------------------

def device_keep(tree, r, scores=None, rounds=None):
    """keep through the host-buffer entry point into a poisoned, guarded buffer."""
    lib = pt._load()
    buf, keep = guarded_cells(tree.npts)
    n_kept, n_rounds = ctypes.c_uint64(12345), ctypes.c_uint32(0)
    scalar = np.ndim(r) == 0
    fn = lib.ptk_search64_suppress_within_self if tree._f64 else lib.ptk_suppress_within_self
    rc = fn(tree._h, tree._real(r if scalar else 0), None if scalar else r.ctypes.data, _ptr(scores), keep.ctypes.data,
            ctypes.byref(n_kept), ctypes.byref(n_rounds))
    assert rc == 0, lib.ptk_last_error()
    assert written(buf, keep), "a cell was not decided, or one was written outside"
    assert n_kept.value == int(keep.sum())
    assert 1 <= n_rounds.value <= tree.npts, n_rounds.value
    if rounds is not None:
        rounds.append(n_rounds.value)
    return keep.copy()


class ByDevice:
    chain_n = 600

    def __init__(self, gpu, dtype=np.float32):
        self.gpu, self.dtype = gpu, dtype
        self.last_rounds = None

    def tree(self, p, metric, leaf):
        t = pt.KdTree(p.astype(self.dtype), getattr(pt.Metric, metric), leaf, device=self.gpu)
        if self.dtype != np.float32:  # (host_search_rows takes the float32 host tree of the same points)
            host = pt.KdTree(p, getattr(pt.Metric, metric), leaf, device=pt.PTK_DEVICE_NONE)
            return _Pair(t, host)
        return t

    def keep(self, tree, p, r, scores=None):
        rounds = []
        got = device_keep(getattr(tree, "device_tree", tree), self.dtype(r) if np.ndim(r) == 0 else r.astype(self.dtype),
                          scores, rounds)
        self.last_rounds = rounds[0]
        return got


class _Pair:
    """A float64 device tree with the float32 host tree whose host loop gives the rows of the constructed cases (their
    numbers are exact in both formats, with a margin from every radius)."""

    def __init__(self, device_tree, host):
        self.device_tree, self._h, self._pts = device_tree, host._h, host._pts
        self._host = host


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_equals_the_expected_keep(gpu, kind, metric, monkeypatch):
    c = rs.case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    for r in own_radii(c):
        for sk in SCORE_KINDS:
            got = device_keep(tree, r, scores_of(c.n, sk))
            assert np.array_equal(got, want_scalar(c, r, sk)), (kind, metric, r, sk)
    radii = c.radii()
    for sk in (None, "levels"):
        assert np.array_equal(device_keep(tree, radii, scores_of(c.n, sk)), want_radii(c, sk)), (kind, metric, "per row", sk)
    r = own_radii(c)[2]
    assert np.array_equal(tree.suppress_within_self(r), want_scalar(c, r, None) == 1)
    assert 1 <= tree.last_suppress_rounds <= c.n
    # pieces of leaf positions that end inside a wavefront: a round spans all of them before the next starts
    monkeypatch.setenv("PTK_MAX_BATCH", "1000")
    for sk in (None, "random"):
        assert np.array_equal(device_keep(tree, r, scores_of(c.n, sk)), want_scalar(c, r, sk)), (kind, metric, "pieces", sk)
    assert np.array_equal(device_keep(tree, radii, scores_of(c.n, "levels")), want_radii(c, "levels"))
    monkeypatch.delenv("PTK_MAX_BATCH")


@pytest.mark.gpu
@needs_reference64
@pytest.mark.parametrize("kind", ["uniform", "ties", "lidar", "2d", "1d", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_float64_trees(gpu, kind, metric, monkeypatch):
    """The kinds and metrics of the float32 test in double (and the 1-D cloud): every instantiation of the float64 round
    kernel behind its dispatch; on "ties" the piles."""
    import torch

    c = rs.case(kind, metric, "float64")
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    for r in own_radii(c):
        for sk in SCORE_KINDS:
            assert np.array_equal(device_keep(tree, r, scores_of(c.n, sk)), want_scalar(c, r, sk)), (kind, metric, r, sk)
    radii = c.radii()
    for sk in (None, "levels"):
        assert np.array_equal(device_keep(tree, radii, scores_of(c.n, sk)), want_radii(c, sk)), (kind, metric, "per row", sk)
    r = own_radii(c)[1]
    dev = tree.suppress_within_self(r, scores=scores_of(c.n, "random"), device=True)
    assert dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), want_scalar(c, r, "random") == 1)


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [False, True])
def test_a_stream_under_capture_is_refused_by_name(gpu, f64):
    """The rounds wait on their stream: a capturing stream gets PTK_ERR_INVALID and the reason before anything is
    enqueued -- the capture itself goes on and ends as it would have."""
    import torch

    p = rs.cloud("small")[0]
    tree = pt.KdTree(p.astype(np.float64) if f64 else p, pt.Metric.L2Squared, 5, device=gpu)
    lib = pt._load()
    fn = lib.ptk_search64_suppress_within_self_device if f64 else lib.ptk_suppress_within_self_device
    keep = torch.zeros(tree.npts, dtype=torch.uint8, device=f"cuda:{gpu}")
    side = torch.cuda.Stream(device=gpu)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        keep.fill_(7)
        rc = fn(tree._h, tree._real(0.01), None, None, keep.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        message = lib.ptk_last_error().decode()
    assert rc == -1 and "captured" in message, (rc, message)
    torch.cuda.synchronize()
    # outside a capture the same call serves
    assert fn(tree._h, tree._real(0.01), None, None, keep.data_ptr(), None, side.cuda_stream) == 0
    side.synchronize()
    assert int(keep.max().item()) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constructed_cases_on_the_device(gpu, dtype):
    """The chain at n = 600 (the even indices, 1 <= n_rounds <= 600), the pile, n = 1, 2, 3."""
    check_constructed(ByDevice(gpu, dtype))


@pytest.mark.gpu
@needs_reference
def test_the_host_buffer_form_with_poisoned_inputs_around(gpu):
    """The host-buffer form reads exactly its n radii and n scores and writes exactly its n cells: the arrays sit inside
    larger ones whose other entries are NaN (a radius or score read from there would be refused or change the order)."""
    c = rs.case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    G = rs.GUARD
    radii_buf = np.full(c.n + 2 * G, np.nan, dtype=np.float32)
    radii_buf[G:G + c.n] = c.radii()
    scores_buf = np.full(c.n + 2 * G, np.nan, dtype=np.float32)
    scores_buf[G:G + c.n] = scores_of(c.n, "levels")
    got = device_keep(tree, radii_buf[G:G + c.n], scores_buf[G:G + c.n])
    assert np.array_equal(got, want_radii(c, "levels"))


@pytest.mark.gpu
@needs_reference
def test_two_calls_give_identical_arrays(gpu):
    c = rs.case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    for r in own_radii(c)[1:]:
        for sk in (None, "levels"):
            s = scores_of(c.n, sk)
            first = device_keep(tree, r, s)
            assert np.array_equal(first, device_keep(tree, r, s)) and np.array_equal(first, want_scalar(c, r, sk))


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
        for sk in (None, "levels"):
            s = scores_of(len(p), sk)
            assert np.array_equal(device_keep(tree, np.float32(r), s), expected_keep(*rows, s)), (metric, move, r, sk)
    assert asym > 0


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
    for s in (None, np.arange(len(pts), dtype=np.float32)):
        assert np.array_equal(device_keep(tree, np.float32(0.05), s), expected_keep(*rows, s)), (depth, s is None)
        got = device_keep(tree, np.float32(1e4), s)  # (every row holds every other point: the highest key alone)
        assert got.sum() == 1 and got[int(np.argmax(keys_of(len(pts), s)))] == 1, (depth, s is None)


@pytest.mark.gpu
@needs_reference
def test_torch_device_forms_on_a_side_stream(gpu):
    """The _device entry point on a side stream into a poisoned, guarded tensor; the wrapper's device form, plain and
    indices; a NaN and a negative d_radii entry and NaN d_scores: empty rows and bit-ordered scores."""
    import torch

    c = rs.case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    lib = pt._load()
    side = torch.cuda.Stream(device=gpu)
    r = own_radii(c)[2]
    radii = c.radii()
    levels = scores_of(c.n, "levels")
    G = rs.GUARD
    n_rounds = ctypes.c_uint32(0)
    bad = radii.copy()
    bad[100], bad[2000] = np.nan, -1.0
    bad_scores = np.array(scores_of(c.n, "random"))
    bad_scores[[5, 100, 777]] = np.nan
    bad_scores[888] = -np.nan
    with torch.cuda.stream(side):
        buf = torch.full((c.n + 2 * G,), POISON8, dtype=torch.uint8, device=f"cuda:{gpu}")
        assert lib.ptk_suppress_within_self_device(tree._h, np.float32(r), None, None, buf[G:].data_ptr(),
                                                   ctypes.byref(n_rounds), side.cuda_stream) == 0
        plain = tree.suppress_within_self(r, device=True)
        rounds = tree.last_suppress_rounds
        kept = tree.suppress_within_self(r, scores=torch.from_numpy(np.array(levels)).to(f"cuda:{gpu}"), indices=True,
                                         device=True)
        from_host = tree.suppress_within_self(r, scores=levels, device=True)
        d_radii = torch.from_numpy(radii).to(f"cuda:{gpu}")
        per_row = tree.suppress_within_self(d_radii, device=True)
        d_bad = torch.from_numpy(bad).to(f"cuda:{gpu}")
        d_bad_scores = torch.from_numpy(bad_scores).to(f"cuda:{gpu}")
        per_row_bad = [tree.suppress_within_self(d_bad, scores=s, device=True) for s in (None, d_bad_scores)]
    side.synchronize()
    raw = buf.cpu().numpy()
    want = want_scalar(c, r, None)
    assert np.all(raw[:G] == POISON8) and np.all(raw[-G:] == POISON8) and np.array_equal(raw[G:-G], want)
    assert 1 <= n_rounds.value <= c.n and 1 <= rounds <= c.n
    assert plain.dtype == torch.bool and np.array_equal(plain.cpu().numpy(), want == 1)
    assert kept.dtype == torch.int64 and np.array_equal(kept.cpu().numpy(), np.flatnonzero(want_scalar(c, r, "levels")))
    assert np.array_equal(from_host.cpu().numpy(), want_scalar(c, r, "levels") == 1)
    assert np.array_equal(per_row.cpu().numpy(), want_radii(c, None) == 1)
    rows = empty_rows(*c.want_per_row(), [100, 2000])
    for s, got in zip((None, bad_scores), per_row_bad):
        got = got.cpu().numpy()
        assert np.array_equal(got, expected_keep(*rows, s) == 1), s is None
        assert got[100] and got[2000]
    for wrong in (d_bad[:5], d_bad.double(), d_bad.reshape(-1, 1)):
        with pytest.raises(ValueError):
            tree.suppress_within_self(wrong, device=True)
        with pytest.raises(ValueError):
            tree.suppress_within_self(r, scores=wrong, device=True)
    with pytest.raises(ValueError):
        tree.suppress_within_self(r, scores=bad_scores, device=True)  # (a host array is checked before it goes up)
    with pytest.raises(ValueError):
        tree.suppress_within_self(r, scores=d_bad_scores)  # (a host call takes a host array)


def _refused(tree, reason, want):
    with pytest.raises(pt.PtkError) as refused:
        tree.suppress_within_self(0.01, scores=scores_of(tree.npts, "levels"))
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
    assert reason in str(refused.value) and "ptk_host_suppress_within_self" in str(refused.value), str(refused.value)
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got = tree.suppress_within_self(0.01, scores=scores_of(tree.npts, "levels"))
    finally:
        pt.allow_host_loop(False)
    assert np.array_equal(got, want == 1), reason


@pytest.mark.gpu
@needs_reference
def test_refused_handles_and_the_host_loop_that_serves_them(gpu):
    c5 = rs.case("5d", "L2Squared")
    _refused(pt.KdTree(c5.p, pt.Metric.L2Squared, c5.leaf, device=gpu), "dim > 3",
             expected_keep(*c5.want(np.float32(0.01)), scores_of(c5.n, "levels")))
    rng = np.random.default_rng(12)
    p1 = rng.random((2_000, 1), dtype=np.float32)
    ref = oracle.Oracle(p1, 8, "reference", metric="SO2")
    _refused(pt.KdTree(p1, pt.Metric.SO2, 8, device=gpu), "topological",
             expected_keep(*rs.without_self(*ref.search_radius(p1, np.float32(0.01))), scores_of(len(p1), "levels")))
    deep, _ = depth_cases.cloud_at_depth(1032, 3, 10)
    deep = np.asarray(deep)
    tree = pt.KdTree(deep, pt.Metric.L2Squared, 10, device=gpu)
    _refused(tree, "tree depth 1032",
             expected_keep(*host_search_rows(tree, deep, np.float32(0.01)), scores_of(len(deep), "levels")))
    # the argument checks of the device entry points
    lib = pt._load()
    small = pt.KdTree(rs.cloud("small")[0], pt.Metric.L2Squared, 5, device=gpu)
    keep = np.zeros(small.npts, dtype=np.uint8)
    bad = np.full(small.npts, 0.1, dtype=np.float32)
    bad[7] = bad[9] = np.nan
    assert lib.ptk_suppress_within_self(small._h, np.float32(0.1), None, None, None, None, None) == -1
    assert lib.ptk_suppress_within_self(small._h, np.float32(np.nan), None, None, keep.ctypes.data, None, None) == -1
    assert lib.ptk_suppress_within_self(small._h, np.float32(-1), None, None, keep.ctypes.data, None, None) == -1
    assert lib.ptk_suppress_within_self(small._h, np.float32(1), bad.ctypes.data, None, keep.ctypes.data, None, None) == -1
    assert "radii[7]" in lib.ptk_last_error().decode()
    assert lib.ptk_suppress_within_self(small._h, np.float32(1), None, bad.ctypes.data, keep.ctypes.data, None, None) == -1
    assert "scores[7]" in lib.ptk_last_error().decode()
    assert lib.ptk_suppress_within_self_device(small._h, np.float32(0.1), None, None, None, None, None) == -1
    assert lib.ptk_suppress_within_self(small._h, np.float32(0.1), None, None, keep.ctypes.data, None, None) == 0
    with pytest.raises(ValueError):
        small.suppress_within_self(bad, device=True)


@pytest.mark.gpu
def test_the_radius_capture_and_the_other_searches_are_left_alone(gpu):
    """A scalar search_radius count / fill pair with suppress calls between its halves still returns its rows;
    count_within_self, search_radius_self and cluster_within_self of the same handle give the bytes they gave before."""
    import torch

    p, q = ds.uniform_cloud(20_000, 3, 71), ds.uniform_cloud(6_000, 3, 72)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)

    def others():
        return [tree.count_within_self(0.001).tobytes(), tree.count_within_self(0.001, max_count=3).tobytes(),
                tree.search_radius_self(0.001).flat.tobytes(), tree.cluster_within_self(0.001, min_neighbors=3).tobytes(),
                tree.search_knn(q, 1).tobytes()]

    before = others()
    lib = pt._load()
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    stream = torch.cuda.current_stream(dq.device).cuda_stream
    want = tree.search_radius(q, 0.002)
    counts = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                              counts.data_ptr(), stream) == 0
    keep = tree.suppress_within_self(0.001, device=True)
    keep_host = tree.suppress_within_self(np.full(len(p), 0.001, dtype=np.float32))
    offsets = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    offsets[1:] = torch.cumsum(counts[:len(q)], 0)
    out = torch.empty((max(int(offsets[-1].item()), 1), 2), dtype=torch.int32, device=dq.device)
    assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), len(q), np.float32(0.002), np.float32(1),
                                             offsets.data_ptr(), out.data_ptr(), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want.offsets)
    assert rs.raw_rows(out)[:len(want.flat)].tobytes() == want.flat.tobytes()
    rows = tree.search_radius_self(0.001)
    assert np.array_equal(keep.cpu().numpy(), expected_keep(rows.offsets, rows.flat, None) == 1)
    assert np.array_equal(keep_host, keep.cpu().numpy())
    assert separated_and_maximal(rows.offsets, rows.flat, keep_host.astype(np.uint8)) == (True, True)
    assert others() == before


@pytest.mark.gpu
def test_cpp_batched_members(gpu, tmp_path):
    d = str(tmp_path)
    p, r, radii, scores = _cpp_inputs(d)
    exe = os.path.join(d, "suppress_self_batch")
    _cpp_program(exe, host_only=False)
    res = subprocess.run([exe, d, repr(float(r))], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
    _check_cpp_output(d, p, r, radii, scores)
