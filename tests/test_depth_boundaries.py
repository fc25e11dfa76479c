"""Every search family at the tree depths where its dispatch changes ("Depth boundaries").

    39 | 40, 135 | 136   the private spill class of the record stacks: 64 / 256 / 2048 records (ovf_class_of)
    1031 | 1032          the record stacks spill to HBM, the batch runs in pieces (deep_tree, deep_plan); the
                         topological metrics refuse
    51 | 52              the keys of the cooperative radius finish have bits for 51 branches (radius_cap, radius64_cap)
    1024 | 1025          the float64 search_knn_within starts unseeded (ptk_backend_f64.hpp)

tests/depth_cases.py builds a tree of exactly the wanted depth and the queries that fill its record stacks.  The CPU
tier runs the kernel source in the emulator with a counter in ``Stack::push`` / ``Stack64::push``: rows byte-equal to
the oracle, no stack ever above ``2 * depth + 2`` records (the invariant the class table rests on) nor above what the
HOST's class for that depth holds, and the corner queries within 8 records of the invariant (the bounded k-NN and the
count kernels: tests/test_knn_within.py and tests/test_count_within.py, where their emulators are built).  The gpu
tier runs the same trees through every entry point of the library, rows byte-compared with the oracle.
"""

from __future__ import annotations

import warnings

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from tests import depth_cases as dc
from tests.emu import EmulatedTree, EmulatedTree64, ovf_capacity
from tests.depth_cases import EUCLID_CASES, Watch, need
from tests.test_count_within import expected as count_expected
from tests.test_knn_within import expected as within_expected
from tests.test_knn_within import same_rows

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")


# ---- CPU tier: the class table ---------------------------------------------------------------------------------------

def test_the_class_of_every_depth_holds_what_the_invariant_allows():
    """The host's table (ovf_class_of / kOvfSlots, through the emulator's export): the class of a depth holds
    2 * depth + 2 records in a ring of 16, classes change exactly at 39 | 40 and 135 | 136, and 1032 is the first depth of
    the deep class.  (The emulator itself runs every kernel with 2048 spill slots: this, and the high-water checks
    below against ovf_capacity, are what ties the table to the kernels on the CPU.)"""
    for depth in range(1, 1032):
        cap = ovf_capacity(depth)
        assert cap is not None and cap >= need(depth), (depth, cap)
    assert [ovf_capacity(d) for d in (39, 40, 135, 136, 1031)] == [80, 272, 272, 2064, 2064]
    assert ovf_capacity(1032) is None
    # (every launch of the library runs a ring of 16 with this class, but one: the capped phase 2 of the k = 1 search,
    # a ring of 12 -- kP2Ring of ptk_backend_core.hpp says why that holds, test_capped_phase_2_... measures it)


# ---- CPU tier: the kernels in the emulator ---------------------------------------------------------------------------

def _same_radius(got, want, what):
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes(), what


@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", EUCLID_CASES)
def test_emulated_kernels_at_the_class_boundaries(dim, leaf, metric, depth):
    pts, pile = dc.cloud_at_depth(depth, dim, leaf)
    q, nc = dc.queries(pts, pile)
    emu = EmulatedTree(pts, leaf, pt.Metric[metric])
    assert emu.max_depth() == depth
    ref = oracle.Oracle(pts, leaf, "port", metric)
    run = Watch(depth)
    fill = dc.FILL[("euclid", dim, leaf)]
    # (the cooperative finishes run as 64 fibers per wavefront in the emulator, seconds per hundred queries: they get the
    # corner queries, the pile and its neighbours, and a few of the others)
    few, fewer = q[:nc + 24], q[:nc + 3]
    for k in (1, 5, 40, 80):
        want = ref.search_knn(q, k)
        assert run(emu.search_knn, q, k).tobytes() == want.tobytes(), k
        if k <= 40 and metric in ("L2Squared", "L1"):
            # The corner queries alone: the stacks really fill (the measured value, and the bar of 8).  Under the two
            # max / min metrics a k-NN search prunes the chain after a few levels -- the box distance it compares with
            # is a SUM over the axes, the distance to the pile is not --, and only the radius searches below fill.
            run(emu.search_knn, q[:nc], k)
            assert need(depth) - run.high == fill and fill <= 8, (k, run.high, need(depth))
    assert run(emu.search_knn, q, 6, e=1.25).tobytes() == ref.search_knn(q, 6, e=1.25).tobytes()
    for r in (0.05, 1e4):
        want = ref.search_radius(q, r)
        _same_radius(run(emu.search_radius, q, r), want, r)
        if r > 1:  # the corner queries again: a radius that holds the whole tree fills the stacks, under every metric
            run(emu.search_radius, q[:nc], r)
            assert need(depth) - run.high == fill and fill <= 8, (r, run.high)
        if metric == "L2Squared":
            _same_radius(run(emu.search_radius_captured, q, r)[:2], want, (r, "capture"))
        if metric in ("L2Squared", "L1") and dim <= 3:
            _same_radius(run(emu.search_radius_lists, q, r)[:2], want, (r, "lists"))
            for cap in (1, 8) if depth <= 51 else ():  # (radius_cap(): deeper trees run uncapped)
                sub = few if r < 1 else fewer
                off, rows, stats = run(emu.search_radius_lists_capped, sub, r, cap)
                _same_radius((off, rows), ref.search_radius(sub, r), (r, "lists capped", cap))
                assert stats["handed_over"] > 0
    got = run(emu.search_radius, q, 0.05, sort=True)
    want = ref.search_radius(q, 0.05, sort=True)
    assert np.array_equal(got[0], want[0]) and got[1]["distance"].tobytes() == want[1]["distance"].tobytes()
    if metric in ("L2Squared", "L1") and dim <= 3:  # the capped k > 1 search with its cooperative finish
        for k, sub in ((5, few), (40, fewer)):
            want = ref.search_knn(sub, k)
            for cap in (1, 8):
                rows, handed, _ = run(emu.search_knn_capped, sub, k, cap)
                assert rows.tobytes() == want.tobytes(), (k, cap)
                assert handed > 0
    if metric == "L2Squared":
        lo, hi = q - np.float32(0.02), q + np.float32(0.02)
        lo = np.concatenate([lo, pts.min(0)[None, :] - np.float32(1)])
        hi = np.concatenate([hi, pts.max(0)[None, :] + np.float32(1)])
        want = ref.search_box(lo, hi)
        got = run(emu.search_box, lo, hi)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert int(np.diff(want[0])[-1]) == len(pts)


@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("dim,leaf,metric", [(3, 1, "L2Squared"), (3, 10, "L2Squared"), (3, 10, "L1"), (2, 4, "L2Squared"),
                                             (2, 4, "L1")])
def test_emulated_two_phase_k1_search_at_the_class_boundaries(dim, leaf, metric, depth):
    """k = 1 as the backend runs it for metric_l2_squared and metric_l1: phase 1, the class order, phase 2 uncapped
    (variant 3: ring 16) and capped with the cooperative finish (variants 5 and 8: ring 12), on the tree itself and on
    its view without the piles (what the device searches when the tree has piles; its depth is the base cloud's)."""
    pts, pile = dc.cloud_at_depth(depth, dim, leaf)
    q, _ = dc.queries(pts, pile)
    ref = oracle.Oracle(pts, leaf, "port", metric)
    want = ref.search_knn(q, 1)
    for view in (False, True):
        if view and metric != "L2Squared":
            continue  # (the view is the default metric's)
        emu = EmulatedTree(pts, leaf, pt.Metric[metric])
        d = depth
        if view:
            assert emu.use_pile_view() > 0
            d = emu.max_depth()
            assert d < depth
        run = Watch(d)
        for variant in (3, 5, 8):
            rows, _ = run(emu.two_phase_knn1, q, variant=variant)
            assert rows.tobytes() == want.tobytes(), (view, variant)


@pytest.mark.parametrize("leaf", [1, 10])
def test_emulated_radius_finish_at_the_last_depth_its_keys_cover(leaf):
    """51 levels: every path bit of the keys of the cooperative radius finish is in use (kRcMaxDepth); the rows come back
    in the reference's order.  (At 52 the backend runs uncapped: radius_cap().)"""
    pts, pile = dc.cloud_at_depth(51, 3, leaf)
    q, nc = dc.queries(pts, pile)
    emu, ref = EmulatedTree(pts, leaf), oracle.Oracle(pts, leaf, "port")
    run = Watch(51)
    for r, sub in ((0.05, q[:nc + 56]), (1e4, q[:nc + 3])):  # (fibers: seconds per hundred queries)
        for cap in (1, 8):
            off, rows, stats = run(emu.search_radius_lists_capped, sub, r, cap)
            _same_radius((off, rows), ref.search_radius(sub, r), (r, cap))
            assert stats["handed_over"] > 0


@pytest.mark.parametrize("depth", [39, 40, 135, 136])
def test_capped_phase_2_never_holds_more_than_depth_plus_cap_records(depth):
    """The capped phase 2 runs a ring of 12 with the spill class of a ring of 16 (kP2Ring, ptk_backend_core.hpp): at
    the top of a class -- 39, 135, 1031 levels -- that is four records short of 2 * depth + 2.  What saves it is the cap:
    a level costs two records only once its far child has been entered, and a capped traversal enters at most `cap`
    of them, so it holds at most depth + min(cap, depth) records -- within 12 + OVF for every cap up to kP2CapMax = 32,
    which phase2_cap() enforces on the test hook.  Measured on the 2-D tree of leaf size 4, whose two-phase search does
    use its stack (half the need with the cap lifted), with the cap raised as far as the emulator's hook goes."""
    pts, pile = dc.cloud_at_depth(depth, 2, 4)
    q, _ = dc.queries(pts, pile)
    want = oracle.Oracle(pts, 4, "port").search_knn(q, 1)
    emu = EmulatedTree(pts, 4)
    run = Watch(depth)
    highs = {}
    for cap in (1, 2, 8, 24, 32, 1000):
        rows, _ = run(emu.two_phase_knn1, q, variant=5, p2_cap=cap)
        assert rows.tobytes() == want.tobytes(), cap
        highs[cap] = emu.last_p2_high_water
        assert highs[cap] <= depth + min(cap, depth), (cap, highs)
        if cap <= 32:  # every cap the backend lets through: within the ring that runs plus the class it runs with
            assert highs[cap] <= ovf_capacity(depth, 16) - 4, (cap, highs)
    assert highs[1000] >= depth, highs  # (this tree's phase 2 does use its stack)


@needs_reference
@pytest.mark.parametrize("depth", [39, 40, 135, 136])
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_emulated_topological_kernels_at_the_class_boundaries(metric, depth):
    """The trees of depth_cases.chain_at_depth: a chain of distinct points, whose one-point leaves are the NEARER child of
    the fill queries on every level, so that a radius search over the whole tree holds two undo records per level (a
    pile of coincident points leaves these stacks half empty: depth_cases.TOPO)."""
    dim, leaf, fill = dc.TOPO[metric]
    pts, n_chain = dc.chain_at_depth(depth, metric)
    q, nf = dc.chain_queries(pts, metric)
    emu = EmulatedTree(pts, leaf, pt.Metric[metric])
    assert emu.max_depth() == depth
    ref = oracle.Oracle(pts, leaf, "reference", metric)
    run = Watch(depth)
    for k in (1, 7, 40):
        assert run(emu.search_knn, q, k).tobytes() == ref.search_knn(q, k).tobytes(), k
    for r in (0.05, 1e4):
        _same_radius(run(emu.search_radius, q, r), ref.search_radius(q, r), r)
    run(emu.search_radius, q[:nf], 1e4)
    assert need(depth) - run.high == fill and fill <= 8, run.high  # the measured value, and the bar
    if depth <= 40:  # (k = 40 takes the whole chain of these: the k-NN kernels fill as well)
        run(emu.search_knn, q[:nf], 40)
        assert need(depth) - run.high <= 8, run.high


@pytest.mark.parametrize("depth,dim", [(51, 3), (52, 3), (135, 3), (135, 5), (1024, 3), (1025, 5)])
def test_emulated_float64_kernels_at_their_boundaries(depth, dim):
    """The double kernels allocate 2 * depth + 4 slots per lane exactly, so an over-long stack lands in the next lane's
    column: knn (registers and the row), radius plain and capped (the cooperative finish: keys of 51 branches), box."""
    leaf = 10 if dim == 3 else 1
    pts, pile = dc.cloud_at_depth(depth, dim, leaf, np.float64)
    q, nc = dc.queries(pts, pile)
    emu = EmulatedTree64(pts, leaf)
    assert emu.max_depth() == depth
    ref = oracle.Oracle(pts, leaf, "port", dtype=np.float64)
    run = Watch(depth)
    run.cap = None  # (no classes on this side: the invariant alone)
    for k in (1, 8, 32, 40):
        assert same_rows(run(emu.search_knn, q, k), ref.search_knn(q, k)), k
    run(emu.search_knn, q[:nc], 8)
    assert need(depth) - run.high <= 8, run.high
    for r in (0.05, 1e4):
        want = ref.search_radius(q, r)
        off, flat = run(emu.search_radius, q, r)
        assert np.array_equal(off, want[0]) and same_rows(flat, want[1]), r
        if depth == 51:  # (the keys of the finish have bits for 51 branches; radius64_cap() runs deeper trees uncapped)
            sub = q[:nc + 56] if r < 1 else q[:nc + 3]  # (fibers: seconds per hundred queries)
            sub_want = ref.search_radius(sub, r)
            for cap in (1, 8):
                off, flat, handed, _ = run(emu.search_radius_capped, sub, r, cap)
                assert np.array_equal(off, sub_want[0]) and same_rows(flat, sub_want[1]), (r, cap)
                assert handed > 0
    lo, hi = q - 0.02, q + 0.02
    got, want = run(emu.search_box, lo, hi), ref.search_box(lo, hi)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- gpu tier ----------------------------------------------------------------------------------------------------------

F32_DEPTHS = (39, 40, 135, 136, 1031, 1032)


def _prefilled(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).reshape(-1)[:] = 0xA5
    return a


def _knn(tree, ref, q, k, e=None):
    nns = _prefilled((len(q),) if k == 1 else (len(q), k), tree.dtype_neighbor)
    got = tree.search_knn(q, k, nns) if e is None else tree.search_knn(q, k, float(e), nns)
    want = ref.search_knn(q, k, e=e)
    assert same_rows(got, want[:, 0] if k == 1 else want), ("search_knn", k, e)


def _radius(tree, ref, q, r, sort=False):
    got = tree.search_radius(q, r, sort=sort)
    off, flat = ref.search_radius(q, r, sort=sort)
    assert np.array_equal(got.offsets, off), ("search_radius offsets", r, sort)
    if sort:
        # Equal distances may come in either order of their indices (the reference sorts by distance alone): the
        # distances bit for bit, and the same SET of indices in every run of equal distances of a row.
        dist = np.ascontiguousarray(flat["distance"])
        assert np.ascontiguousarray(got.flat["distance"]).tobytes() == dist.tobytes(), r
        if len(dist):
            row = np.repeat(np.arange(len(q)), np.diff(off).astype(np.int64))
            new_run = np.r_[True, (row[1:] != row[:-1]) | (dist[1:] != dist[:-1])]
            key = np.cumsum(new_run).astype(np.int64) << 32
            assert np.array_equal(np.sort(key | got.flat["index"].astype(np.int64)),
                                  np.sort(key | flat["index"].astype(np.int64))), ("sorted rows: index sets", r)
    else:
        assert same_rows(got.flat, flat), ("search_radius rows", r)


def _box(tree, ref, pts, q, half=0.02):
    real = pts.dtype.type
    lo = np.concatenate([q - real(half), pts.min(0)[None, :] - real(1)])
    hi = np.concatenate([q + real(half), pts.max(0)[None, :] + real(1)])
    boxes = np.empty((2 * len(lo), pts.shape[1]), dtype=pts.dtype)
    boxes[0::2], boxes[1::2] = lo, hi
    got = tree.search_box(boxes)
    off, flat = ref.search_box(lo, hi)
    assert np.array_equal(got.offsets, off) and np.array_equal(got.flat, flat), "search_box"
    assert int(np.diff(off)[-1]) == len(pts)  # the box that holds the whole tree


def _within(tree, ref, q, ks, radii):
    for r in radii:
        for k in ks:
            got = tree.search_knn_within(q, k, r, _prefilled((len(q), k), tree.dtype_neighbor))
            assert same_rows(got, within_expected(ref, q, k, r)), ("search_knn_within", k, r)


def _count(tree, ref, q, radii, n_pile, sums=True):
    at_corner = []
    for r in radii:
        want = count_expected(ref, q, r)
        at_corner.append(int(want[0]))
        for mc in (0, 16):
            assert np.array_equal(tree.count_within(q, r, mc), np.minimum(want, mc) if mc else want), ("count_within", r, mc)
    # (the pile is out at r and in at the next number above it -- under the sum metrics: the max and min metrics prune
    # by a SUM over the axes, in the reference as here, and lose most of the pile)
    assert not sums or at_corner[:3] == [0, n_pile, 0], at_corner
    assert at_corner[3] == ref.n  # (the radius that holds the whole tree)


def _euclid_case(gpu, dim, leaf, metric, depth, dtype=np.float32):
    pts, pile = dc.cloud_at_depth(depth, dim, leaf, dtype)
    q, _ = dc.queries(pts, pile)
    tree = pt.KdTree(np.asarray(pts), pt.Metric[metric], leaf, device=gpu)
    dc.assert_depth(tree, depth)
    ref = oracle.Oracle(pts, leaf, "port", metric, dtype=dtype)
    return pts, q, tree, ref


def _all_entry_points(pts, q, tree, ref, ks, full):
    for k in ks:
        _knn(tree, ref, q, k)
    if full:  # the uncapped phase 2 (ring 16) and the approximate visitors
        _knn(tree, ref, q, 1, e=1.25)
        _knn(tree, ref, q, 6, e=1.25)
    for r in (0.05, 1e4):
        _radius(tree, ref, q, r)
    _radius(tree, ref, q, 0.05, sort=True)
    _radius(tree, ref, q, 1e4, sort=True)
    if full:
        _box(tree, ref, pts, q)
    radii = dc.edge_radii(ref, q)
    _within(tree, ref, q, (5, 80), radii)
    _count(tree, ref, q, radii, len(pts) - 3_000, sums=ref.metric in ("L2Squared", "L1"))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", F32_DEPTHS)
@pytest.mark.parametrize("leaf", [1, 10])
def test_3d_default_metric_at_every_boundary(gpu, leaf, depth):
    pts, q, tree, ref = _euclid_case(gpu, 3, leaf, "L2Squared", depth)
    _all_entry_points(pts, q, tree, ref, (1, 5, 40, 80), full=True)
    # k = 1 of a tree with piles runs on its view without them, a shallow tree.  With the view off (test hook) the
    # two-phase search itself meets the depth: its class (dispatch_knn1_of), the capped phase 2 with its ring of 12,
    # and at 1032 levels the deep path.
    pt.set_test_knobs(pile_view=0)
    whole = pt.KdTree(np.asarray(pts), pt.Metric.L2Squared, leaf, device=gpu)
    dc.assert_depth(whole, depth)
    assert whole.piles()["piles"] == 0 and tree.piles()["piles"] > 0
    _knn(whole, ref, q, 1)
    _knn(whole, ref, q, 1, e=1.25)
    # (the hook for the cap of phase 2 is held at kP2CapMax = 32, what its ring of 12 is sized for: phase2_cap())
    pt.set_test_knobs(pile_view=0, p2_cap=1000)
    _knn(whole, ref, q, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", F32_DEPTHS)
@pytest.mark.parametrize("metric", ["L1", "LPInf", "LNInf"])
def test_3d_other_metrics_at_every_boundary(gpu, metric, depth):
    """The "any k, any metric" claim of the deep path, and the same classes below it."""
    pts, q, tree, ref = _euclid_case(gpu, 3, 10, metric, depth)
    _all_entry_points(pts, q, tree, ref, (1, 5, 40), full=False)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", F32_DEPTHS)
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
@pytest.mark.parametrize("dim,leaf", [(2, 4), (5, 1)])
def test_2d_and_5d_at_every_boundary(gpu, dim, leaf, metric, depth):
    """5-D at 1032: knn_nd_deep, knn_nd_within_deep, radius_nd_deep and the deep box pass of the any-dimension kernels."""
    pts, q, tree, ref = _euclid_case(gpu, dim, leaf, metric, depth)
    _all_entry_points(pts, q, tree, ref, (1, 5, 40, 80), full=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,leaf", [(3, 10), (5, 1)])
def test_deep_tree_in_pieces_of_64_queries(gpu, monkeypatch, dim, leaf):
    """PTK_DEEP_SPILL_MB=1: deep_plan clamps to its smallest piece, 64 queries, so the batch of about 400 runs as seven
    launches with a ragged last one; the rows are those of the default run (one piece) and the oracle's."""
    pts, q, tree, ref = _euclid_case(gpu, dim, leaf, "L2Squared", 1032)
    q = np.ascontiguousarray(np.concatenate([q, q[:60]]))  # (a seventh, ragged piece)
    assert 6 * 64 < len(q) < 7 * 64
    radii = dc.edge_radii(ref, q)

    def rows():
        return [tree.search_knn(q, 1).tobytes(), tree.search_knn(q, 40).tobytes(), tree.search_radius(q, 0.05).flat.tobytes(),
                tree.search_knn_within(q, 5, radii[1]).tobytes(), tree.count_within(q, radii[1]).tobytes()]

    whole = rows()
    assert tree.deep_pieces() == 1
    monkeypatch.setenv("PTK_DEEP_SPILL_MB", "1")
    assert rows() == whole
    assert tree.deep_pieces() == 7
    _all_entry_points(pts, q, tree, ref, (1, 5, 40, 80), full=True)


def _seam_boxes(q, axis, half=0.03):
    """Boxes q +- half whose interval on the circle axis wraps through the seam 0 ~ 1 where it leaves [0, 1]."""
    lo, hi = (q - np.float32(half)).astype(np.float32), (q + np.float32(half)).astype(np.float32)
    wrap = (lo[:, axis] < 0) | (hi[:, axis] > 1)
    lo[lo[:, axis] < 0, axis] += np.float32(1)
    hi[hi[:, axis] > 1, axis] -= np.float32(1)
    return lo, hi, wrap


def _topo_case(gpu, metric, depth):
    dim, leaf, _ = dc.TOPO[metric]
    if depth <= 136:  # a chain of distinct points: the stacks fill (depth_cases.TOPO)
        pts, _ = dc.chain_at_depth(depth, metric)
        q, _ = dc.chain_queries(pts, metric)
    else:  # (no room in float32 for a chain of a thousand halvings: the coincident pile)
        pts, pile = dc.cloud_at_depth(depth, dim, leaf, space=metric)
        q, _ = dc.queries(pts, pile, metric)
    tree = pt.KdTree(np.asarray(pts), pt.Metric[metric], leaf, device=gpu)
    dc.assert_depth(tree, depth)
    return pts, q, tree, oracle.Oracle(pts, leaf, "reference", metric)


def _topo_searches(pts, q, tree, ref):
    for k in (1, 7, 40):
        _knn(tree, ref, q, k)
    for r in (0.05, 1e4):
        _radius(tree, ref, q, r)
    lo, hi, wrap = _seam_boxes(q, pts.shape[1] - 1)
    boxes = np.empty((2 * len(q), pts.shape[1]), dtype=np.float32)
    boxes[0::2], boxes[1::2] = lo, hi
    got = tree.search_box(boxes)
    off, flat = ref.search_box(lo, hi)
    assert np.array_equal(got.offsets, off) and np.array_equal(got.flat, flat), "search_box"
    assert wrap.sum() > 0 and np.diff(off)[wrap].sum() > 0  # the boxes through the seam do find points
    return wrap


@needs_reference
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [39, 40, 135, 136, 1031])
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_topological_metrics_at_every_boundary(gpu, metric, depth):
    pts, q, tree, ref = _topo_case(gpu, metric, depth)
    _topo_searches(pts, q, tree, ref)
    for r in (0.05, 1e4, 0.0):
        for mc in (0, 16):
            want = count_expected(ref, q, np.float32(r), mc)
            assert np.array_equal(tree.count_within(q, r, mc), want), ("count_within", r, mc)


@needs_reference
@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_topological_metrics_refuse_the_first_deep_tree(gpu, metric):
    """1032 levels: the topological kernels have no HBM spill, the device refuses ("too deep"); after allow_host_loop the
    library's host loop answers as the reference does."""
    pts, q, tree, ref = _topo_case(gpu, metric, 1032)
    boxes = np.empty((2 * len(q), pts.shape[1]), dtype=np.float32)
    boxes[0::2], boxes[1::2] = q - np.float32(0.02), q + np.float32(0.02)
    for search in (lambda: tree.search_knn(q, 1), lambda: tree.search_knn(q, 7), lambda: tree.search_radius(q, 0.05),
                   lambda: tree.search_box(boxes)):
        with pytest.raises(pt.PtkError, match="too deep"):
            search()
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (one per process: it may or may not come here)
            _topo_searches(pts, q, tree, ref)
    finally:
        pt.allow_host_loop(False)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [51, 52])
@pytest.mark.parametrize("leaf", [1, 10])
def test_radius_finish_at_the_last_depth_its_keys_cover(gpu, leaf, depth):
    """radius_cap(): a key of the cooperative radius finish has bits for 51 branches.  With a cap of 1 (test hook) nearly
    every query is handed to a wavefront at 51 levels -- every path bit of the keys in use, rows in the reference's
    order --, and none at 52, where the batch must run uncapped."""
    import torch

    pts, q, tree, ref = _euclid_case(gpu, 3, leaf, "L2Squared", depth)
    pt.set_test_knobs(radius_cap=1)
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    handed = 0
    for r in (0.05, 1e4):
        want_off, want = ref.search_radius(q, np.float32(r))
        off, raw = tree.search_radius_device(dq, np.float32(r))  # (the counters are those of a device-buffer count pass)
        torch.cuda.synchronize()
        assert np.array_equal(off.cpu().numpy().astype(np.uint64), want_off) and raw.cpu().numpy().tobytes() == want.tobytes(), r
        handed += tree.radius_coop_counts()["cooperative"]
        _radius(tree, ref, q, r)
    assert (handed > 0) if depth == 51 else (handed == 0), handed


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [51, 52])
@pytest.mark.parametrize("leaf", [1, 10])
def test_float64_radius_finish_at_the_last_depth_its_keys_cover(gpu, leaf, depth):
    pts, q, tree, ref = _euclid_case(gpu, 3, leaf, "L2Squared", depth, np.float64)
    pt.set_test_knobs(radius64_cap=1)
    handed = 0
    for r in (0.05, 1e4):
        _radius(tree, ref, q, r)
        handed += tree.knn_coop_counts()["cooperative"]
    assert (handed > 0) if depth == 51 else (handed == 0), handed


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1024, 1025])
@pytest.mark.parametrize("metric", ["L2Squared", "L1"])
def test_float64_knn_within_where_the_seed_is_dropped(gpu, metric, depth):
    """ptk_search64_knn_within_device seeds its list at radius * (1 + 2^-10) up to 1024 levels and starts unseeded above."""
    pts, q, tree, ref = _euclid_case(gpu, 3, 10, metric, depth, np.float64)
    _within(tree, ref, q, (5, 80), dc.edge_radii(ref, q))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [135, 1032])
@pytest.mark.parametrize("dim,leaf", [(3, 10), (5, 1)])
def test_float64_searches_at_the_depths_of_the_float32_classes(gpu, dim, leaf, depth):
    """2 * depth + 4 slots are allocated per lane exactly: an over-long stack would land in the next lane's column."""
    pts, q, tree, ref = _euclid_case(gpu, dim, leaf, "L2Squared", depth, np.float64)
    for k in (1, 8, 32, 40):
        _knn(tree, ref, q, k)
    for r in (0.05, 1e4):
        _radius(tree, ref, q, r)
    _box(tree, ref, pts, q)
    _count(tree, ref, q, dc.edge_radii(ref, q), len(pts) - 3_000)
