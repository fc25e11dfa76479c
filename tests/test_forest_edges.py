"""The kd-forest search at its edges: every branch of `forest_knn_kernel` (pico_tree_amd/csrc/ptk_forest.hpp) that
tests/test_forest.py's SIFT-like clouds stay away from, its limits, its arguments and non-finite input.

One case table serves both tiers:

* CPU tier (no marker): the kernel source under the lane emulator (`tests.emu.emulated_forest_knn`) against
  `oracle.ForestOracle` over the reflections the emulator drew;
* `gpu` tier: `pt.KdForest` through the C ABI -- host form into a numpy buffer, device form into a caller-made torch
  tensor, both prefilled with 0xA5 bytes so that a slot the kernel did not write cannot pass -- against
  `ForestOracle(pts, leaf, forest.rotations)`.

The k-list of the kernel lives one entry per lane, its ranks come from ballots, its node records from readlane, its
distances from a transposing butterfly: the lane-by-lane emulator cannot see a mistake in any of that, the `gpu` tier
can.

`ForestOracle` shares the product's design decisions (tie order, queue cap, summation tree), so two groups of checks do
not go through it: every listed distance is recomputed here, in numpy, in the kernel's own summation order
(`_kernel_distance`), and exhaustive searches are compared with a float64 brute force and the exact kd_tree oracle
(`test_*_exhaustive_search_is_exact`).
"""

from __future__ import annotations

import functools
import re

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import poison as P
from tests.emu import emulated_forest_knn

FLT_MAX = np.finfo(np.float32).max
PTK_ERR_INVALID, PTK_ERR_UNSUPPORTED = -1, -2  # (ptk.h)
SEED = 11                                      # of the reflections, both tiers
PREFILL = 0xA5


# ---- the case table -------------------------------------------------------------------------------------------------
# name: (dim, n, leaf, trees, k, leaves, nq).  The smallest shapes that reach each branch.
CASES = {
    "seg2": (256, 1200, 32, 2, 5, 4, 24),             # the `segs` loop twice
    "seg3-k64": (384, 900, 20, 2, 64, 6, 16),         # three segments, 16 + 4 row chunks, a full 64-lane list
    "ragged-chunks": (128, 1500, 200, 2, 10, 3, 16),  # up to 13 chunks of 16 rows, the last one ragged
    "dim96": (96, 2000, 8, 2, 7, 5, 32),              # the unrolled 32-wide path 3 times
    "dim160": (160, 2000, 8, 2, 7, 5, 32),            # ... 5 times
    "dim12": (12, 2000, 8, 2, 7, 5, 32),              # the float4 path at a dimension other than 16
    "dim1": (1, 2000, 4, 2, 7, 5, 32),                # the scalar path
    "dim2": (2, 2000, 4, 3, 7, 5, 32),
    "dim3": (3, 2000, 4, 3, 7, 5, 32),
    "leaf100": (16, 3000, 100, 3, 10, 4, 32),         # second pass of the 64-lane leaf loop, partly empty wave
    "n1": (16, 1, 8, 2, 3, 4, 8),
    "root-is-leaf": (16, 5, 8, 2, 8, 4, 8),
    "n2-leaf1": (16, 2, 1, 2, 4, 4, 8),
    "k>n": (128, 40, 4, 3, 64, 100, 8),               # all 40 points, then 24 padding slots
    "one-tree-one-leaf": (16, 3000, 8, 1, 5, 1, 32),
    "zero-leaves": (16, 3000, 8, 1, 5, 0, 32),        # every row all padding
    "lattice3-self": (3, 4096, 4, 3, 8, 20, 111),     # equal queue distances, equal point distances
    "lattice2-centres": (2, 4096, 1, 3, 9, 30, 78),
    "duplicates": (16, 3000, 4, 3, 10, 8, 60),        # copies under different indices
    "deep-90": (3, 90, 1, 2, 3, 200, 8),              # a tree about 89 levels deep (the limit is 95)
}

#: Real (non-padding) entries every row of a case must have, where the shape fixes it: with k >= n the list never fills,
#: max() stays FLT_MAX, every far child is queued, and `leaves` covers every leaf of every tree.
FOUND = {"n1": 1, "root-is-leaf": 5, "n2-leaf1": 2, "k>n": 40, "zero-leaves": 0}


def _line(count):
    """Points (2^-i, 0, 0): every sliding-midpoint split takes one point off, the tree is a chain."""
    pts = np.zeros((count, 3), dtype=np.float32)
    pts[:, 0] = np.exp2(-np.arange(count, dtype=np.float64)).astype(np.float32)
    return pts


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(points, queries) of a case; read-only."""
    dim, n, _, _, _, _, nq = CASES[name]
    if name == "lattice3-self":
        g = np.arange(16, dtype=np.float32)
        pts = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
        q = np.ascontiguousarray(pts[::37])
    elif name == "lattice2-centres":
        g = np.arange(64, dtype=np.float32)
        pts = np.ascontiguousarray(np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2))
        q = np.ascontiguousarray(pts[::53] + np.float32(0.5))
    elif name == "duplicates":
        pts = ds.sift_like_cloud(n, dim, 1, centres=20)
        pts[1::3] = pts[::3]
        q = np.ascontiguousarray(pts[::50])
    elif name == "deep-90":
        pts = _line(90)
        q = np.zeros((nq, 3), dtype=np.float32)
        q[:, 0] = np.float32(0.75) * pts[[0, 1, 5, 20, 40, 60, 80, 89], 0]
        q[1::2, 1] = np.float32(1e-9)
    else:
        pts, q = ds.sift_like_cloud(n, dim, 1, centres=20), ds.sift_like_cloud(nq, dim, 2, centres=20)
    assert pts.shape == (n, dim) and q.shape == (nq, dim) and pts.dtype == q.dtype == np.float32
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


# ---- what every row must satisfy, whoever made it -------------------------------------------------------------------

def _kernel_distance(q, p):
    """Squared distances of the rows of `q` and `p` (m, dim) in float32, added in the kernel's own order: left to right,
    or -- dim % 128 == 0 -- lane l sums elements 2l, 2l + 1 of every 128-float segment, then the 64 partial sums are
    added pairwise by lane bit 5, 4, ... 0.  Plain numpy, independent of the oracle."""
    q, p = np.asarray(q, dtype=np.float32), np.asarray(p, dtype=np.float32)
    diff = q - p
    sq = diff * diff
    m, dim = sq.shape
    if dim % 128:
        acc = np.zeros(m, dtype=np.float32)
        for a in range(dim):
            acc = acc + sq[:, a]
        return acc
    s = np.zeros((m, 64), dtype=np.float32)
    for seg in range(dim // 128):
        part = sq[:, 128 * seg:128 * seg + 128]
        s = s + part[:, 0::2]
        s = s + part[:, 1::2]
    for bit in (32, 16, 8, 4, 2, 1):
        s = s[:, :bit] + s[:, bit:2 * bit]
    assert s.dtype == np.float32
    return s[:, 0]


def _check_rows(got, want, pts, q, what):
    """Byte-equal to the oracle; ascending; distinct indices; padding exactly (-1, FLT_MAX) and only at the end; every
    distance the squared distance to pts[index] in the kernel's summation order."""
    assert got.dtype == pt.NEIGHBOR and got.shape == want.shape, what
    assert P.same_rows(got, want), (what, P.first_difference(got, want))
    real = got["index"] >= 0
    nreal = real.sum(1)
    nq, k = got.shape
    assert np.array_equal(real, np.arange(k)[None, :] < nreal[:, None]), (what, "padding inside a row")
    assert np.all(got["index"][~real] == -1) and np.all(got["distance"][~real] == FLT_MAX), what
    assert np.all(got["index"][real] < len(pts)), what
    for i in range(nq):
        row = got[i, :nreal[i]]
        assert np.all(np.diff(row["distance"]) >= 0), (what, i, "not ascending")
        assert len(set(row["index"].tolist())) == len(row), (what, i, "an index twice")
    r, c = np.nonzero(real)
    if len(r):
        d = _kernel_distance(q[r], pts[got["index"][r, c]])
        assert d.tobytes() == np.ascontiguousarray(got["distance"][r, c]).tobytes(), (what, "distance is not |q - p|^2")


def _check_case_on_the_oracle(name, want):
    """What keeps a case from silently testing nothing, asserted on the oracle's rows alone."""
    real = (want["index"] >= 0).sum(1)
    if name in FOUND:
        assert np.all(real == FOUND[name]), (name, real)
    elif name == "one-tree-one-leaf":  # one leaf of at most 8 points: some rows full, some padded
        assert np.all(real >= 1) and np.any(real < want.shape[1]) and np.any(real == want.shape[1]), (name, real)
    else:
        assert np.all(real == want.shape[1]), (name, "rows of this case are full")
    if name.startswith("lattice"):  # equal point distances inside every row
        assert np.all((np.diff(want["distance"], axis=1) == 0).any(1)), name
    if name == "duplicates":
        # query j is point 50 j, points 3 m and 3 m + 1 coincide: both copies are listed, at distance 0
        for j, row in enumerate(want):
            i = 50 * j
            twins = {i, i + 1} if i % 3 == 0 else {i, i - 1} if i % 3 == 1 else {i}
            zero = set(row["index"][row["distance"] == 0].tolist())
            assert twins <= zero, (name, j, twins, zero)


# ---- engines --------------------------------------------------------------------------------------------------------

def _emulated(pts, leaf, trees, q, k, leaves):
    """(rows, oracle over the same reflections, dropped)."""
    got, rot, dropped = emulated_forest_knn(pts, leaf, trees, SEED, q, k, leaves)
    return got, oracle.ForestOracle(pts, leaf, rot), dropped


def _prefilled(nq, k):
    out = np.empty((nq, max(k, 1)), dtype=pt.NEIGHBOR)
    out.view(np.uint8)[...] = PREFILL
    return out


def _abi_host(forest, q, k, leaves, out=None):
    """ptk_forest_search_knn into a prefilled numpy buffer: (status, buffer)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    out = _prefilled(len(q), k) if out is None else out
    rc = pt._load().ptk_forest_search_knn(forest._h, q.ctypes.data, len(q), k, leaves, out.ctypes.data)
    return rc, out


def _abi_device(forest, q, k, leaves, gpu, stream=None):
    """ptk_forest_search_knn_device into a prefilled, caller-made torch tensor: (status, rows on the host)."""
    import torch

    dev = torch.device("cuda", gpu)
    dq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    fill = int(np.array([PREFILL] * 4, dtype=np.uint8).view(np.int32)[0])
    dout = torch.full((len(q), max(k, 1), 2), fill, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    rc = pt._load().ptk_forest_search_knn_device(forest._h, dq.data_ptr(), len(q), k, leaves, dout.data_ptr(),
                                                 s.cuda_stream)
    s.synchronize()
    rows = np.ascontiguousarray(dout.cpu().numpy()).view(pt.NEIGHBOR).reshape(len(q), max(k, 1))
    return rc, rows


def _device_both_forms(forest, q, k, leaves, gpu, what):
    rc, host = _abi_host(forest, q, k, leaves)
    assert rc == 0, what
    rc, dev = _abi_device(forest, q, k, leaves, gpu)
    assert rc == 0, what
    assert P.same_rows(dev, host), (what, "device form differs from host form", P.first_difference(dev, host))
    return host


# ---- the case table, both tiers -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_emulated_forest_edge_case_equals_oracle(name):
    _, _, leaf, trees, k, leaves, _ = CASES[name]
    pts, q = _cloud(name)
    got, orc, dropped = _emulated(pts, leaf, trees, q, k, leaves)
    want = orc.search_knn(q, k, leaves)
    _check_case_on_the_oracle(name, want)
    assert orc.last_dropped == 0 and dropped == 0
    _check_rows(got, want, pts, q, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_forest_edge_case_equals_oracle(gpu, name):
    _, _, leaf, trees, k, leaves, _ = CASES[name]
    pts, q = _cloud(name)
    forest = pt.KdForest(pts, leaf, trees, seed=SEED, device=gpu)
    orc = oracle.ForestOracle(pts, leaf, forest.rotations)
    want = orc.search_knn(q, k, leaves)
    _check_case_on_the_oracle(name, want)
    got = _device_both_forms(forest, q, k, leaves, gpu, name)
    assert orc.last_dropped == 0 and forest.dropped == 0
    _check_rows(got, want, pts, q, name)
    # the Python wrapper hands out the same rows
    assert P.same_rows(forest.search_knn(q, k, leaves), want), name


# ---- a full queue ---------------------------------------------------------------------------------------------------
FULL_QUEUE = (16, 20_000, 1, 2, 64, 600, 24)  # leaf 1, k = 64: max() stays large, every descent queues its whole path


@functools.lru_cache(maxsize=None)
def _full_queue_cloud():
    dim, n, _, _, _, _, nq = FULL_QUEUE
    pts, q = ds.sift_like_cloud(n, dim, 1, centres=20), ds.sift_like_cloud(nq, dim, 2, centres=20)
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


def test_emulated_forest_full_queue_drops_what_the_oracle_drops():
    _, _, leaf, trees, k, leaves, _ = FULL_QUEUE
    pts, q = _full_queue_cloud()
    got, orc, dropped = _emulated(pts, leaf, trees, q, k, leaves)
    want = orc.search_knn(q, k, leaves)
    assert orc.last_dropped > 0, "the case does not fill the queue: it tests nothing"
    _check_rows(got, want, pts, q, "full queue")
    assert dropped == orc.last_dropped


@pytest.mark.gpu
def test_forest_full_queue_drops_what_the_oracle_drops(gpu):
    """`KdForest.dropped` is cumulative over the life of the handle: two identical calls add twice the oracle's count."""
    _, _, leaf, trees, k, leaves, _ = FULL_QUEUE
    pts, q = _full_queue_cloud()
    forest = pt.KdForest(pts, leaf, trees, seed=SEED, device=gpu)
    orc = oracle.ForestOracle(pts, leaf, forest.rotations)
    want = orc.search_knn(q, k, leaves)
    assert orc.last_dropped > 0, "the case does not fill the queue: it tests nothing"
    before = forest.dropped
    assert before == 0
    rc, first = _abi_host(forest, q, k, leaves)
    assert rc == 0
    after_one = forest.dropped
    rc, second = _abi_device(forest, q, k, leaves, gpu)
    assert rc == 0
    after_two = forest.dropped
    _check_rows(first, want, pts, q, "full queue, host form")
    _check_rows(second, want, pts, q, "full queue, device form")
    assert after_one - before == orc.last_dropped
    assert after_two - before == 2 * orc.last_dropped


# ---- non-finite query rows ------------------------------------------------------------------------------------------
NON_FINITE = {"dim16": (16, 3000, 8, 3, 5, 6), "dim128": (128, 1500, 32, 2, 5, 6)}  # dim, n, leaf, trees, k, leaves


@functools.lru_cache(maxsize=None)
def _non_finite_batch(name):
    """(points, clean queries, poisoned queries, mask of poisoned rows, mask of rows whose poison is NaN, +-Inf, +-MAX)."""
    dim, n = NON_FINITE[name][:2]
    pts, clean = ds.sift_like_cloud(n, dim, 1, centres=20), ds.sift_like_cloud(256, dim, 2, centres=20)
    q, mask = P.poison(clean, seed=5)
    changed = (q != clean) | np.isnan(q)
    assert np.array_equal(changed.any(1), mask) and np.all(changed.sum(1) <= 1)
    with np.errstate(invalid="ignore"):
        lethal = (changed & (~np.isfinite(q) | (np.abs(q) == FLT_MAX))).any(1)
    assert lethal.sum() >= 5 and (mask & ~lethal).sum() >= 3  # every member of the palette is in the batch
    for a in (pts, clean, q):
        a.setflags(write=False)
    return pts, clean, q, mask, lethal


def _check_non_finite(name, search, orc):
    """`search(q)` -> rows of the engine under test."""
    _, _, _, _, k, leaves = NON_FINITE[name]
    pts, clean, q, mask, lethal = _non_finite_batch(name)
    want = orc.search_knn(q, k, leaves)
    # on the oracle first: the finite members of the palette give full, finite rows
    huge = mask & ~lethal
    assert np.all(want["index"][huge] >= 0) and np.all(np.isfinite(want["distance"][huge])), name
    assert np.all(want["distance"][huge] < FLT_MAX) and np.all(want["distance"][huge][:, 0] > 1e36), name
    got = search(q)
    assert P.same_rows(got, want), (name, P.first_difference(got, want, mask))
    assert np.all(got["index"][lethal] == -1) and np.all(got["distance"][lethal] == FLT_MAX), \
        (name, "a NaN / Inf / MAX row is not all padding")
    unpoisoned = search(clean)
    assert P.same_rows(unpoisoned, orc.search_knn(clean, k, leaves)), name
    assert P.same_rows(got[~mask], unpoisoned[~mask]), (name, "a poisoned row changed a clean row")
    assert np.all(unpoisoned["index"] >= 0)
    _check_rows(got[~lethal], want[~lethal], pts, q[~lethal], name)


@pytest.mark.parametrize("name", list(NON_FINITE))
def test_emulated_forest_non_finite_query_rows(name):
    _, _, leaf, trees, k, leaves = NON_FINITE[name]
    pts = _non_finite_batch(name)[0]
    rot = emulated_forest_knn(pts, leaf, trees, SEED, pts[:1], 1, 1)[1]
    _check_non_finite(name, lambda q: emulated_forest_knn(pts, leaf, trees, SEED, q, k, leaves)[0],
                      oracle.ForestOracle(pts, leaf, rot))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NON_FINITE))
def test_forest_non_finite_query_rows(gpu, name):
    _, _, leaf, trees, k, leaves = NON_FINITE[name]
    pts = _non_finite_batch(name)[0]
    forest = pt.KdForest(pts, leaf, trees, seed=SEED, device=gpu)
    _check_non_finite(name, lambda q: _device_both_forms(forest, q, k, leaves, gpu, name),
                      oracle.ForestOracle(pts, leaf, forest.rotations))


# ---- exact answers, not through the restatement ---------------------------------------------------------------------
# (dim, n, nq, k, leaf, trees): `default_rng(dim).random` clouds searched exhaustively (max_leaves_visited = 2^30).
EXACT = [(3, 5000, 200, 16, 4, 3), (5, 4000, 200, 10, 8, 2), (16, 3000, 100, 10, 8, 2), (33, 2000, 64, 64, 10, 1),
         (128, 1000, 40, 5, 16, 2)]
EXHAUSTIVE = 2 ** 30


@functools.lru_cache(maxsize=None)
def _exact_cloud(dim, n, nq):
    """The first n points and nq queries of the cloud of `dim` (the emulator runs a prefix of what the device runs)."""
    full_n, full_nq = next((c[1], c[2]) for c in EXACT if c[0] == dim)
    rng = np.random.default_rng(dim)
    pts, q = rng.random((full_n, dim), dtype=np.float32), rng.random((full_nq, dim), dtype=np.float32)
    pts, q = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(q[:nq])
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


def _check_exact(got, pts, q, k, what):
    """`got` against a float64 brute force (indices) and the exact kd_tree oracle (distance bits).

    The bound: a float32 squared distance -- dim subtractions (2^-24 each, doubled by the squaring), dim squarings
    (2^-24) and dim - 1 additions of non-negative terms (2^-24 each along any path of any summation tree) -- differs from
    the exact one by less than (dim + 2) * 2^-23 of it.  Derived, not measured.  Two float32 distances can therefore
    change places only if the exact ones are closer than twice that."""
    dim = pts.shape[1]
    bound = (dim + 2) * 2.0 ** -23
    d64 = ((q.astype(np.float64)[:, None, :] - pts.astype(np.float64)[None, :, :]) ** 2).sum(2)
    order = np.argsort(d64, axis=1, kind="stable")[:, :k + 1]
    top = np.take_along_axis(d64, order, 1)
    # on the brute force alone: the k-th and the (k + 1)-th neighbour are further apart than float32 can confuse
    assert np.all(top[:, k] - top[:, k - 1] > 2 * bound * top[:, k]), what
    assert np.all(got["index"] >= 0), what
    assert np.array_equal(np.sort(got["index"], axis=1), np.sort(order[:, :k], axis=1)), (what, "not the k nearest")
    # ... and in the same order in every row whose neighbours are ALL that far apart
    clear = np.all(np.diff(top, axis=1) > 2 * bound * top[:, 1:], axis=1)
    assert clear.sum() * 2 >= len(q), what
    assert np.array_equal(got["index"][clear], order[clear, :k]), what
    if dim % 128:
        exact = oracle.Oracle(pts, 10, "port").search_knn(q, k)
        assert np.ascontiguousarray(got["distance"]).tobytes() == np.ascontiguousarray(exact["distance"]).tobytes(), what
    else:
        d = np.take_along_axis(d64, got["index"].astype(np.int64), 1)
        assert np.all(np.abs(got["distance"].astype(np.float64) - d) <= bound * d), what
    _check_rows(got, got, pts, q, what)


@pytest.mark.parametrize("dim,n,nq,k,leaf,trees", EXACT)
def test_forest_oracle_exhaustive_search_is_exact(dim, n, nq, k, leaf, trees):
    """The restatement at the sizes the device runs (the emulator takes minutes there)."""
    pts, q = _exact_cloud(dim, n, nq)
    rot = emulated_forest_knn(pts[:64], leaf, trees, SEED, q[:1], 1, 1)[1]
    orc = oracle.ForestOracle(pts, leaf, rot)
    got = orc.search_knn(q, k, EXHAUSTIVE)
    assert orc.last_dropped == 0
    _check_exact(got, pts, q, k, (dim, n))


@pytest.mark.parametrize("dim,n,nq,k,leaf,trees", [(d, 800, 32, k, leaf, t) for d, _, _, k, leaf, t in EXACT])
def test_emulated_forest_exhaustive_search_is_exact(dim, n, nq, k, leaf, trees):
    pts, q = _exact_cloud(dim, n, nq)
    got, _, dropped = emulated_forest_knn(pts, leaf, trees, SEED, q, k, EXHAUSTIVE)
    assert dropped == 0
    _check_exact(got, pts, q, k, (dim, n))


@pytest.mark.gpu
@pytest.mark.parametrize("dim,n,nq,k,leaf,trees", EXACT)
def test_forest_exhaustive_search_is_exact(gpu, dim, n, nq, k, leaf, trees):
    pts, q = _exact_cloud(dim, n, nq)
    forest = pt.KdForest(pts, leaf, trees, seed=SEED, device=gpu)
    got = _device_both_forms(forest, q, k, EXHAUSTIVE, gpu, (dim, n))
    assert forest.dropped == 0
    _check_exact(got, pts, q, k, (dim, n))


# ---- limits and arguments -------------------------------------------------------------------------------------------

def _bad_cloud(value, row=17, col=3):
    pts = ds.sift_like_cloud(200, 8, 1, centres=20)
    pts[row, col] = value
    return pts


def _overflowing_cloud(value):
    """Two dimensions, point 17 = (value, 0), point 18 = (0, value): a unit vector r has a component beyond 1/2, so
    2 (r . x) overflows for one of the two whatever r is."""
    pts = ds.sift_like_cloud(200, 2, 1, centres=20)
    pts[17], pts[18] = (value, 0), (0, value)
    return pts


def test_forest_create_refuses_a_dimension_beyond_the_lds():
    """2 dim + 2 * 1024 + 2 * 96 floats of LDS: 7072 is the last dimension that fits 64 KiB.  Checked before the device
    lookup, so this needs no GPU."""
    with pytest.raises(pt.PtkError, match="7073") as err:
        pt.KdForest(np.zeros((4, 7073), dtype=np.float32), 2, 1, device=0)
    assert err.value.status == PTK_ERR_UNSUPPORTED


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_forest_create_refuses_non_finite_points(value):
    """As ptk_tree_create_from_points: PTK_ERR_INVALID naming the first offending point, before the device lookup."""
    pts = _bad_cloud(value)
    pts[101, 0] = value
    with pytest.raises(pt.PtkError, match=r"point 17 is not finite \(coordinate 3 ") as err:
        pt.KdForest(pts, 8, 2, device=0)
    assert err.value.status == PTK_ERR_INVALID


@pytest.mark.parametrize("value", [FLT_MAX, -FLT_MAX, np.nan, np.inf])
def test_emulated_forest_build_refuses_a_reflection_that_is_not_finite(value):
    """x - (2 r.x) r overflows (or is inf - inf) for a coordinate at FLT_MAX: an all-finite cloud would hand NaN to
    std::nth_element.  build_forest_tree says so instead."""
    pts = _overflowing_cloud(value)
    with pytest.raises(RuntimeError, match="point 1[78] has no finite reflection"):
        emulated_forest_knn(pts, 8, 2, SEED, pts[:4], 3, 4)


def test_emulated_forest_builds_over_a_huge_finite_coordinate():
    pts = _bad_cloud(np.float32(1e30))
    q = ds.sift_like_cloud(16, 8, 2, centres=20)
    got, orc, dropped = _emulated(pts, 8, 2, q, 3, 4)
    assert dropped == 0
    _check_rows(got, orc.search_knn(q, 3, 4), pts, q, "1e30")
    assert np.all(got["index"] >= 0) and not np.any(got["index"] == 17)


DEPTH = r"forest tree is (\d+) levels deep \(limit 95\)"


def _too_deep():
    return {"line-120": (_line(120), 1), "coincident-500": (np.full((500, 3), 7.0, dtype=np.float32), 4)}


@pytest.mark.parametrize("name", ["line-120", "coincident-500"])
def test_emulated_forest_build_refuses_a_tree_beyond_the_depth_limit(name):
    pts, leaf = _too_deep()[name]
    with pytest.raises(RuntimeError, match=DEPTH) as err:
        emulated_forest_knn(pts, leaf, 2, SEED, pts[:2], 1, 4)
    depth = int(re.search(DEPTH, str(err.value)).group(1))
    assert depth >= 96 and (name != "coincident-500" or depth == 496)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["line-120", "coincident-500"])
def test_forest_create_refuses_a_tree_beyond_the_depth_limit(gpu, name):
    pts, leaf = _too_deep()[name]
    with pytest.raises(pt.PtkError, match=r"tree 0: " + DEPTH) as err:
        pt.KdForest(pts, leaf, 2, seed=SEED, device=gpu)
    assert err.value.status == PTK_ERR_UNSUPPORTED
    depth = int(re.search(DEPTH, str(err.value)).group(1))
    assert depth >= 96 and (name != "coincident-500" or depth == 496)


@pytest.mark.gpu
def test_forest_create_refuses_an_overflowing_reflection_and_builds_over_1e30(gpu):
    with pytest.raises(pt.PtkError, match=r"tree 0: point 1[78] has no finite reflection") as err:
        pt.KdForest(_overflowing_cloud(FLT_MAX), 8, 2, seed=SEED, device=gpu)
    assert err.value.status == PTK_ERR_UNSUPPORTED
    pts = _bad_cloud(np.float32(1e30))
    q = ds.sift_like_cloud(16, 8, 2, centres=20)
    forest = pt.KdForest(pts, 8, 2, seed=SEED, device=gpu)
    got = _device_both_forms(forest, q, 3, 4, gpu, "1e30")
    _check_rows(got, oracle.ForestOracle(pts, 8, forest.rotations).search_knn(q, 3, 4), pts, q, "1e30")
    assert np.all(got["index"] >= 0) and not np.any(got["index"] == 17)


@pytest.mark.gpu
def test_forest_largest_dimension_that_fits_the_lds(gpu):
    """dim 7072: the kernel's dynamic LDS is exactly 64 KiB."""
    dim, n, leaf, trees, k, leaves, nq = 7072, 300, 8, 1, 3, 2, 4
    pts, q = ds.sift_like_cloud(n, dim, 1, centres=20), ds.sift_like_cloud(nq, dim, 2, centres=20)
    forest = pt.KdForest(pts, leaf, trees, seed=SEED, device=gpu)
    got = _device_both_forms(forest, q, k, leaves, gpu, "dim 7072")
    want = oracle.ForestOracle(pts, leaf, forest.rotations).search_knn(q, k, leaves)
    assert np.all(want["index"] >= 0)
    _check_rows(got, want, pts, q, "dim 7072")


@pytest.fixture(scope="module")
def small_forest(gpu):
    pts, q = ds.sift_like_cloud(500, 16, 1, centres=20), ds.sift_like_cloud(8, 16, 2, centres=20)
    return pt.KdForest(pts, 8, 2, seed=SEED, device=gpu), pts, q


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 65])
def test_forest_search_refuses_k_outside_1_to_64_and_writes_nothing(gpu, small_forest, k):
    import torch

    forest, _, q = small_forest
    untouched = _prefilled(len(q), 65)
    rc, out = _abi_host(forest, q, k, 4, out=_prefilled(len(q), 65))
    assert rc == PTK_ERR_INVALID and out.tobytes() == untouched.tobytes()
    dev = torch.device("cuda", gpu)
    dq = torch.from_numpy(q).to(dev)
    dout = torch.from_numpy(untouched.view(np.int32).reshape(len(q), 65, 2).copy()).to(dev)
    rc = pt._load().ptk_forest_search_knn_device(forest._h, dq.data_ptr(), len(q), k, 4, dout.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert rc == PTK_ERR_INVALID and dout.cpu().numpy().tobytes() == untouched.tobytes()
    with pytest.raises(pt.PtkError, match=r"k must be in 1\.\.64"):
        forest.search_knn(q, k, 4)


@pytest.mark.gpu
def test_forest_search_arguments(gpu, small_forest):
    import torch

    forest, pts, q = small_forest
    dev = torch.device("cuda", gpu)
    want = oracle.ForestOracle(pts, 8, forest.rotations).search_knn(q, 5, 4)
    # no queries: an empty (0, k) result, host and device form
    empty = forest.search_knn(np.empty((0, 16), dtype=np.float32), 5, 4)
    assert empty.shape == (0, 5) and empty.dtype == pt.NEIGHBOR
    assert forest.search_knn(torch.empty((0, 16), dtype=torch.float32, device=dev), 5, 4).numpy().shape == (0, 5)
    # what the wrapper refuses
    with pytest.raises(ValueError):
        forest.search_knn(np.zeros((4, 15), dtype=np.float32), 5, 4)
    with pytest.raises(ValueError):
        forest.search_knn(torch.zeros((4, 15), dtype=torch.float32, device=dev), 5, 4)
    with pytest.raises(ValueError):
        forest.search_knn(torch.zeros((4, 32), dtype=torch.float32, device=dev)[:, ::2], 5, 4)
    with pytest.raises(ValueError):
        forest.search_knn(torch.zeros((4, 16), dtype=torch.float64, device=dev), 5, 4)
    # the device form on a stream of the caller's equals the host form
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = forest.search_knn(torch.from_numpy(q).to(dev), 5, 4)
    side.synchronize()
    assert P.same_rows(got.numpy(), want)
    rc, rows = _abi_device(forest, q, 5, 4, gpu, stream=side)
    assert rc == 0 and P.same_rows(rows, want)
    rc, host = _abi_host(forest, q, 5, 4)
    assert rc == 0 and P.same_rows(host, want)
    _check_rows(host, want, pts, q, "arguments")
