"""GPU tier: every value of every launch ladder, once, on the smallest input that reaches it.

The launch wrappers of pico_tree_amd/csrc pick their kernel instantiation through the helpers of ptk_dispatch.hpp: the
k-list size (4 / 8 / 16 / 32 / 64 slots; 1 / 4 / 8 / 16 / 32 in the capped float64 search), the metric, and the boolean
pairs (one radius or one per row, count or fill, exact or approximate, the leaf-list form, the compressing find, the
topological box).  A forgotten or swapped arm of one of them returns wrong rows for ONE k, metric or flag: here every arm
runs on one small cloud per precision and dimension -- 3 000 uniform points, leaf size 10, 257 queries (four full
wavefronts and one lane), 130 points for the searches of the tree's own points -- against ``oracle.Oracle(.., "port")``,
compared as the tests of each family compare (index and distance bits; the filtered rows for the bounded searches).  The
topological metrics are outside the restatement: they compare against the compiled reference, as their own tests do.

tests/cpp/dispatch_main.cpp checks the helpers themselves on the host."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import test_normals_self as ns
from tests import test_radius_self as rs
from tests.test_cluster_self import expected_labels
from tests.test_f64 import _topological_case
from tests.test_knn_within import same_rows

pytestmark = pytest.mark.gpu

N, NQ, N_SELF, LEAF = 3_000, 257, 130, 10
KS = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 81)  # each list size at both ends; 65 / 81: the list in LDS / in the row
KS_SELF = (3, 4, 7, 8, 15, 16, 31, 32, 63)           # k + 1 at each boundary
KS_CAPPED = (1, 4, 5, 16, 17, 32)
EUCLID = ("L2Squared", "L1", "LPInf", "LNInf")
CONFIGS = [("float32", 3), ("float32", 5), ("float64", 3), ("float64", 5)]
# (the uncapped ladders: a batch of 257 queries is capped by the rule, and the capped forms have a test of their own)
UNCAPPED = {"knn_cap": 0, "knn64_cap": 0, "radius_cap": 0, "radius64_cap": 0}


class Case:
    """Points, queries and the restatement's tree; its k-NN rows are computed once per k and shared."""

    def __init__(self, dtype, dim, metric, n, leaf):
        self.dtype, self.dim, self.metric, self.leaf = np.dtype(dtype), dim, metric, leaf
        scale = 1.0000001 if self.dtype == np.float64 else 1  # (double coordinates that are no float32 numbers)
        self.p = np.ascontiguousarray(ds.uniform_cloud(n, dim, 1).astype(dtype) * self.dtype.type(scale))
        self.q = np.ascontiguousarray(ds.uniform_cloud(NQ, dim, 2).astype(dtype) * self.dtype.type(scale))
        self.ref = oracle.Oracle(self.p, leaf, "port", metric, dtype=dtype)
        self._knn = {}

    def knn(self, k):
        if k not in self._knn:
            self._knn[k] = self.ref.search_knn(self.q, k)
            self._knn[k].setflags(write=False)
        return self._knn[k]

    def tree(self, gpu):
        return pt.KdTree(self.p, pt.Metric[self.metric], self.leaf, device=gpu)

    def radius(self, nth=5):
        """The median distance of the nth neighbour: rows of the bounded searches end inside the list."""
        return self.dtype.type(np.median(self.knn(16)["distance"][:, nth - 1]))

    def radii(self, n=NQ):
        """One radius per row: none, half and four times radius(), in turn."""
        r = np.empty(n, dtype=self.dtype)
        r[0::3], r[1::3], r[2::3] = 0, self.radius() / 2, self.radius() * 4
        return r

    def within(self, k, r):
        """search_knn_within's rows from the restatement's search_knn rows: entries below the radius, the pad behind."""
        rows = self.knn(k)
        r = np.broadcast_to(np.asarray(r, dtype=self.dtype), (len(rows),))[:, None]
        out = np.zeros(rows.shape, dtype=rows.dtype)
        out["index"], out["distance"] = -1, r
        keep = rows["distance"] < r
        out[keep] = rows[keep]
        return out

    def radius_rows(self, q, r, e=None):
        """(offsets, flat) of search_radius with a scalar radius or one per row (one run per distinct radius)."""
        if np.ndim(r) == 0:
            return self.ref.search_radius(q, r, e=e)
        off, parts = np.zeros(len(q) + 1, dtype=np.uint64), [None] * len(q)
        for v in np.unique(r):
            at = np.flatnonzero(r == v)
            o, flat = self.ref.search_radius(np.ascontiguousarray(q[at]), v)
            for j, i in enumerate(at):
                parts[i] = flat[int(o[j]):int(o[j + 1])]
        off[1:] = np.cumsum([len(x) for x in parts])
        return off, np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def case(dtype, dim, metric="L2Squared", n=N, leaf=LEAF):
    return Case(dtype, dim, metric, n, leaf)


def knobs(**values):
    """Context manager: the test hooks set for its body, removed after it."""
    class _Knobs:
        def __enter__(self):
            pt.set_test_knobs(**values)

        def __exit__(self, *exc):
            pt.set_test_knobs(**{name: None for name in values})
    return _Knobs()


def same_radius(got, want, what):
    off, flat = want
    assert np.array_equal(got.offsets, off), what
    assert same_rows(got.flat, flat), what


def check_knn_forms(c, tree, k, what):
    """search_knn, search_knn_within with one radius and with one per row, at one k."""
    assert same_rows(tree.search_knn(c.q, k), c.knn(k)), (what, k, "search_knn")
    assert same_rows(tree.search_knn_within(c.q, k, c.radius()), c.within(k, c.radius())), (what, k, "within")
    assert same_rows(tree.search_knn_within(c.q, k, c.radii()), c.within(k, c.radii())), (what, k, "within, per row")


# ---- the k ladders -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dim", CONFIGS)
def test_k_ladders(gpu, dtype, dim):
    """float32: knn_reg_kernel / knn_reg_within(_radii)_kernel, their dim 5 forms, knn_kernel beyond 64.  float64: the
    register kernels to 64 slots at dim 3, to 32 at dim 5 -- k = 33 .. 64 there is the row kernel's."""
    c = case(dtype, dim)
    tree = c.tree(gpu)
    with knobs(**UNCAPPED):
        for k in KS:
            check_knn_forms(c, tree, k, (dtype, dim))


def self_rows(ref, p, k):
    """search_knn_self from the (k + 1)-rows: without the first entry whose index is the row's, else without the last."""
    rows = ref.search_knn(p, k + 1)
    hit = rows["index"] == np.arange(len(p))[:, None]
    keep = np.ones(hit.shape, dtype=bool)
    keep[np.arange(len(p)), np.where(hit.any(1), hit.argmax(1), k)] = False
    return rows[keep].reshape(len(p), k)


def test_knn_self_ladder(gpu):
    c = case("float32", 3, n=N_SELF)
    tree = c.tree(gpu)
    for k in KS_SELF:
        assert tree.self_route(k) == 1  # (the direct kernel)
        assert same_rows(tree.search_knn_self(k), self_rows(c.ref, c.p, k)), k


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_capped_forms(gpu, dtype):
    """The capped launch, the cooperative search and the redo kernel at each of their list sizes (float32: 4 .. 32 of the
    five; float64: 1 / 4 / 8 / 16 / 32), under the two metrics that are capped; a cap of 1 hands nearly every query over."""
    cap = "knn_cap" if dtype == "float32" else "knn64_cap"
    with knobs(**{cap: 1, "knn_cap_min_nq": 1}):
        # (float32 has a capped kernel of 64 slots as well: k = 33 .. 56)
        for metric, ks in (("L2Squared", KS_CAPPED + ((33,) if dtype == "float32" else ())), ("L1", (5,))):
            c = case(dtype, 3, metric)
            tree = c.tree(gpu)
            for k in ks:
                assert same_rows(tree.search_knn(c.q, k), c.knn(k)), (dtype, metric, k)
                if dtype == "float64" or k > 1:  # (float32 k = 1 is the two-phase search: never capped)
                    assert tree.knn_coop_counts()["cooperative"] > 0, (dtype, metric, k)


# ---- the metrics -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dim", CONFIGS)
def test_euclidean_metrics(gpu, dtype, dim):
    """The three metrics beside the default on one k of each ladder, and on the count and radius searches with one radius
    and one per row (the float64 ones pick their metric in the count unit)."""
    for metric in EUCLID[1:]:
        c = case(dtype, dim, metric)
        tree = c.tree(gpu)
        with knobs(**UNCAPPED):
            check_knn_forms(c, tree, 5, (dtype, dim, metric))
            check_knn_forms(c, tree, 70, (dtype, dim, metric))
        for r in (c.radius(), c.radii()) if dim == 3 else (c.radius(),):  # (a radius per row: 3-D trees)
            want = c.radius_rows(c.q, r)
            same_radius(tree.search_radius(c.q, r), want, (dtype, dim, metric, np.ndim(r)))
            if dim == 3:  # (count_within is a search of 3-D trees)
                assert np.array_equal(tree.count_within(c.q, r), np.diff(want[0].astype(np.int64))), (dtype, metric, np.ndim(r))


def test_knn_self_metrics(gpu):
    for metric in EUCLID[1:]:
        c = case("float32", 3, metric, n=N_SELF)
        assert same_rows(c.tree(gpu).search_knn_self(7), self_rows(c.ref, c.p, 7)), metric


@pytest.mark.skipif(not (oracle.have_reference() and oracle.have_reference64()), reason="compiled reference not present")
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_topological_metrics(gpu, dtype, metric):
    """knn_topo_reg_kernel / knn_topo_kernel and knn64_(reg_)kernel<Topo64..> at every list size, the radius search (count
    and fill) and the box search (count and fill, the four-bound tests)."""
    pts, q, radius, mins, maxs, _ = _topological_case(metric, N, NQ, 93)
    pts, q, mins, maxs = (np.ascontiguousarray(a.astype(dtype)) for a in (pts, q, mins, maxs))
    tree = pt.KdTree(pts, pt.Metric[metric], LEAF, device=gpu)
    ref = oracle.Oracle(pts, LEAF, "reference", metric, dtype=dtype)
    for k in KS:
        assert same_rows(tree.search_knn(q, k), ref.search_knn(q, k)), (dtype, metric, k)
    want = ref.search_radius(q, float(radius))
    assert want[0][-1] > NQ
    same_radius(tree.search_radius(q, float(radius)), want, (dtype, metric, "radius"))
    boxes = np.empty((2 * len(mins), pts.shape[1]), dtype=dtype)
    boxes[0::2], boxes[1::2] = mins, maxs
    got, (off, flat) = tree.search_box(boxes), ref.search_box(mins, maxs)
    assert off[-1] > 0 and np.array_equal(got.offsets, off) and np.array_equal(got.flat, flat), (dtype, metric, "box")


# ---- the boolean pairs -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_self_searches_with_one_radius_and_one_per_row(gpu, dtype):
    """count_within_self, search_radius_self, cluster_within_self with and without the compressing find, and (float32)
    normals_within_self: each kernel's PER_ROW pair, the link kernel's PER_ROW x COMPRESS."""
    c = case(dtype, 3, n=N_SELF)
    tree = c.tree(gpu)
    one = c.radius(2)  # (130 points: a radius at which the clusters are a dozen, with border points and noise)
    for r in (one, np.resize(np.array([0, one / 2, one * 2], dtype=dtype), N_SELF)):
        per_row = np.ndim(r) != 0
        want = rs.without_self(*c.radius_rows(c.p, r))
        assert np.array_equal(tree.count_within_self(r), np.diff(want[0].astype(np.int64))), (dtype, per_row)
        same_radius(tree.search_radius_self(r), want, (dtype, per_row))
        labels = expected_labels(*want, 2)
        core = np.diff(want[0].astype(np.int64)) >= 2
        assert len(np.unique(labels[core])) > 4 and (labels[~core] >= 0).any() and (labels < 0).any()  # clusters, border, noise
        for compress in (1, 0):
            with knobs(cluster_compress=compress):
                assert np.array_equal(tree.cluster_within_self(r, min_neighbors=2), labels), (dtype, per_row, compress)
        if dtype == "float32":
            host = pt.KdTree(c.p, pt.Metric.L2Squared, LEAF, device=pt.PTK_DEVICE_NONE)
            frames, moments = tree.normals_within_self(r, moments=True)
            assert moments.tobytes() == ns.expected_moments(c.p, *want).tobytes(), per_row
            assert frames.tobytes() == ns.host_normals(host, r, want="frames")[0].tobytes(), per_row


@pytest.mark.parametrize("leaf", [LEAF, 40])
def test_radius_lists_exact_and_approximate(gpu, leaf):
    """radius_list_kernel<BIG, EXACT, CAPPED> and radius_coop_count_kernel<EXACT>: leaves of 40 points need the BIG form
    of the leaf lists; e = 1.25 is the approximate search; a cap of 1 hands nearly every query to the cooperative count."""
    import torch

    c = case("float32", 3, leaf=leaf)
    tree = c.tree(gpu)
    r = c.radius(16)
    dq = torch.from_numpy(c.q).to(f"cuda:{gpu}")
    for e in (None, 1.25):
        off, flat = c.radius_rows(c.q, r, e=e)
        for cap in (0, 1):
            with knobs(radius_cap=cap):
                same_radius(tree.search_radius(c.q, r) if e is None else tree.search_radius(c.q, r, e), (off, flat), (leaf, e, cap))
                # (the counters are those of a device-buffer count pass: the host entry has finished both passes)
                d_off, raw = tree.search_radius_device(dq, r, e=e or 1.0)
                torch.cuda.synchronize()
                assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), off), (leaf, e, cap)
                assert raw.cpu().numpy().tobytes() == flat.tobytes(), (leaf, e, cap)
                assert (tree.radius_coop_counts()["cooperative"] > 0) == (cap == 1), (leaf, e, cap)


@pytest.mark.parametrize("dtype,dim", CONFIGS[1:])
def test_radius_count_and_fill_of_the_other_families(gpu, dtype, dim):
    """radius_nd_kernel<FILL>, radius64_kernel<M, FILL, D3> at dim 3 and 5, the capped float64 pair."""
    c = case(dtype, dim)
    tree = c.tree(gpu)
    r = c.radius(16)
    for e in (None, 1.25):
        want = c.radius_rows(c.q, r, e=e)
        for cap in (0, 1):
            with knobs(radius64_cap=cap):
                same_radius(tree.search_radius(c.q, r) if e is None else tree.search_radius(c.q, r, e), want, (dtype, dim, e, cap))
                if dtype == "float64" and dim == 3:
                    assert (tree.knn_coop_counts()["cooperative"] > 0) == (cap == 1), (e, cap)


@pytest.mark.parametrize("dtype,dim", CONFIGS)
def test_box_count_and_fill(gpu, dtype, dim):
    """box_kernel / box_nd_kernel / box64_kernel<FILL, false>: search_box is a count pass and a fill pass."""
    c = case(dtype, dim)
    rng = np.random.default_rng(7)
    mins = rng.random((NQ, dim)).astype(dtype) * c.dtype.type(0.8)
    maxs = mins + c.dtype.type(0.35 if dim == 5 else 0.15)
    boxes = np.empty((2 * NQ, dim), dtype=dtype)
    boxes[0::2], boxes[1::2] = mins, maxs
    got, (off, flat) = c.tree(gpu).search_box(boxes), c.ref.search_box(mins, maxs)
    assert off[-1] > NQ and np.array_equal(got.offsets, off) and np.array_equal(got.flat, flat), (dtype, dim)
