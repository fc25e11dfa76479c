"""Every search family at the leaf sizes where its leaf scan changes ("Leaf-size boundaries").

    n = L                 the tree is one leaf: the root reference is a leaf, no branch, the encoders emit a dummy node
    31 | 32               the count bits of the leaf reference go 5 -> 6; radius_list_kernel<BIG> on; at 32 a piece of the
                          leaf list closes exactly at the leaf's end
    32 | 33               a listed leaf is two pieces (RadiusListPolicy::visit, both cooperative radius finishes)
    63 | 64 | 65          count bits 6 -> 7; two full pieces, then a third
    2047 | 2048 | 2049    64 pieces: every piece number of a finish's sort key; above 2048 the capped radius searches are off
    12 + 19 bits | 20     every bit of the leaf reference in use; one point more and the encoders refuse the tree

tests/leaf_cases.py builds a tree with a leaf of exactly L points and the queries that scan it, with radii at which the
expected rows take some pieces of that leaf and leave others.  The CPU tier runs the kernel source in the emulator, the
gpu tier runs the same trees through every entry point of the library; rows byte-compared with the oracle, and every
handle asserts the size of its largest leaf.  (The kernels of count_within, search_knn_within and the self searches
decode a leaf reference of their own: their CPU halves are in tests/test_count_within.py, test_knn_within.py,
test_knn_self.py, test_radius_self.py, test_cluster_self.py and test_normals_self.py, where their emulators are built.)
"""

from __future__ import annotations

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from tests import leaf_cases as lc
from tests import test_cluster_self as cs
from tests import test_knn_self as ks
from tests import test_normals_self as ns
from tests import test_radius_self as rs
from tests.emu import EmulatedTree, EmulatedTree64
from tests.test_count_within import expected as count_expected
from tests.test_depth_boundaries import _knn, _prefilled, _radius
from tests.test_knn_within import same_rows

needs_reference64 = pytest.mark.skipif(not (oracle.have_reference() and oracle.have_reference64()),
                                       reason="compiled reference not present")

#: The one-leaf tree: n = L = 100 points, a leaf of three pieces and four points (k = 80 still fits the tree).
ONE_LEAF = 100


def _same_radius(got, want, what):
    assert np.array_equal(np.asarray(got[0]).astype(np.uint64), want[0]), what
    assert same_rows(np.asarray(got[1]), want[1]), what


def _case(L, dim=3, dtype=np.float32, metric="L2Squared"):
    """lc.case; ``L = ONE_LEAF`` is the blob alone.  Where the family lists its leaves, the inputs do what the case is
    for -- from the reference's rows alone: at r_part a row of a blob query has points of two pieces of the blob leaf
    (L >= 33), one leaves a piece out between two it has points of (L >= 65), none holds the whole blob; at r_all every
    one does."""
    c = lc.case(L, dim, dtype, metric, n=0 if L == ONE_LEAF else None)
    pts, blob, q, nb, ref, radii = c
    if lc.listed(ref):
        off, flat = ref.search_radius(q[:nb], radii[0])
        hit = lc.pieces_hit(ref, L, off, flat, nb)
        assert L <= lc.PIECE or lc.spans_two(hit), (L, hit)
        assert L <= 2 * lc.PIECE or lc.has_gap(hit), (L, hit)
        in_blob = np.bincount(rs.row_ids(off)[flat["index"] >= ref.n - L], minlength=nb)
        assert in_blob.max() < L, (L, "r_part holds the whole blob")
    off, flat = ref.search_radius(q[:nb], radii[1])
    assert np.all(np.diff(off.astype(np.int64)) >= L), (L, "r_all does not hold the whole blob")
    return c


def _boxes(pts, q):
    """Boxes that cut the blob (q +- 0.004), boxes that hold it (q +- 0.02) and the box of the whole tree."""
    real = pts.dtype.type
    lo = np.concatenate([q - real(0.004), q - real(0.02), pts.min(0)[None, :] - real(1)])
    hi = np.concatenate([q + real(0.004), q + real(0.02), pts.max(0)[None, :] + real(1)])
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def _same_box(got, want, n):
    assert np.array_equal(np.asarray(got[0]).astype(np.uint64), want[0]) and np.array_equal(got[1], want[1]), "search_box"
    assert int(np.diff(want[0].astype(np.int64))[-1]) == n  # (the box that holds the whole tree)


# ---- CPU tier: the kernels in the emulator ---------------------------------------------------------------------------

@pytest.mark.parametrize("L", lc.LEAVES + (ONE_LEAF,))
def test_emulated_float32_kernels_at_the_leaf_boundaries(L):
    pts, blob, q, nb, ref, radii = _case(L)
    emu = EmulatedTree(pts, L)
    lc.assert_leaf(emu, L)
    lc.assert_leaf(emu.host, L)
    # (the cooperative finishes run as 64 fibers per wavefront in the emulator, and under the large leaves a radius of 1e4
    # is 22 000 rows per query: those runs get 30 queries, the blob's among them)
    few = q[:30] if L >= 2047 else q
    for k in (1, 5, 40, 80):
        assert emu.search_knn(q, k).tobytes() == ref.search_knn(q, k).tobytes(), k
    for variant in (3, 5):  # k = 1 as the backend runs it: both phases decode a leaf reference of their own
        rows, _ = emu.two_phase_knn1(q, variant=variant)
        assert rows.tobytes() == ref.search_knn(q, 1).tobytes(), ("two-phase", variant)
    rows, handed, _ = emu.search_knn_capped(q, 5, 1)
    assert rows.tobytes() == ref.search_knn(q, 5).tobytes()
    assert handed > 0 or L == ONE_LEAF  # (a tree of one leaf has no far child to hand over at)
    handed = 0
    for r in radii:
        want = ref.search_radius(q, r)
        _same_radius(emu.search_radius(q, r), want, r)
        _same_radius(emu.search_radius_lists(q, r)[:2], want, (r, "lists"))
        if L <= 2048:  # (radius_cap(): a leaf of more than 64 pieces runs uncapped)
            off, rows, stats = emu.search_radius_lists_capped(few, r, 1)
            _same_radius((off, rows), ref.search_radius(few, r), (r, "lists capped"))
            handed += stats["handed_over"]
    assert handed > 0 or L in (2049, ONE_LEAF)
    if L in (2047, 2048):
        # The piece numbers above 31: at 1e4 a row has more leaf pieces than a finish keeps (512) and is searched again
        # from the root, and a blob query's own launch scans the blob leaf before it hands anything over.  The side query's
        # row holds all 64 pieces of the blob leaf and few enough others, and the finish is what scans them.
        qs, r = lc.side_query(ref, L)
        off, rows, stats = emu.search_radius_lists_capped(qs, r, 1)
        _same_radius((off, rows), ref.search_radius(qs, r), "side query")
        assert stats == {"handed_over": 1, "recounted": 0, "refilled": 0}, stats
    lo, hi = _boxes(pts, q)
    _same_box(emu.search_box(lo, hi), ref.search_box(lo, hi), len(pts))


@pytest.mark.parametrize("L", lc.LEAVES + (ONE_LEAF,))
def test_emulated_float64_kernels_at_the_leaf_boundaries(L):
    pts, blob, q, nb, ref, radii = _case(L, dtype=np.float64)
    emu = EmulatedTree64(pts, L)
    lc.assert_leaf(emu, L)
    few = q[:30] if L >= 2047 else q
    for k in (1, 5, 40, 80):
        assert same_rows(emu.search_knn(q, k), ref.search_knn(q, k)), k
    rows, handed, _ = emu.search_knn_capped(q, 5, 1)
    assert same_rows(rows, ref.search_knn(q, 5))
    assert handed > 0 or L == ONE_LEAF
    handed = 0
    for r in radii:
        _same_radius(emu.search_radius(q, r), ref.search_radius(q, r), r)
        if L <= 2048:  # (radius64_cap())
            off, flat, n, _ = emu.search_radius_capped(few, r, 1)
            _same_radius((off, flat), ref.search_radius(few, r), (r, "capped"))
            handed += n
    assert handed > 0 or L in (2049, ONE_LEAF)
    if L in (2047, 2048):
        # The side query of the float32 test: the double finish scans all 64 pieces of the blob leaf and keeps the row.  (The
        # row is some 380 sorted entries.  The emulator's entry block is 192 per hand-over it has room for; 64 of them is
        # the block the library gives a batch of one row, radius64_entry_cap().)
        qs, r = lc.side_query(ref, L)
        off, flat, n, redone = emu.search_radius_capped(qs, r, 1, max_heavy=64)
        _same_radius((off, flat), ref.search_radius(qs, r), "side query")
        assert (n, redone) == (1, 0), (n, redone)
    lo, hi = _boxes(pts, q)
    _same_box(emu.search_box(lo, hi), ref.search_box(lo, hi), len(pts))


def test_emulated_kernels_with_every_bit_of_the_leaf_reference_in_use():
    """12 count bits and 19 position bits: the blob leaf's reference has its highest position bits set and a count of all
    ones.  One point more needs 20 position bits, and the encoder refuses the tree."""
    pts, blob, q, nb, ref, radii = lc.case(lc.EDGE_LEAF, n=lc.EDGE_N - lc.EDGE_LEAF)
    assert len(pts) == lc.EDGE_N
    emu = EmulatedTree(pts, lc.EDGE_LEAF)
    lc.assert_leaf(emu, lc.EDGE_LEAF)
    sub = q[:40]
    for k in (1, 5, 40):
        assert emu.search_knn(sub, k).tobytes() == ref.search_knn(sub, k).tobytes(), k
    for r in radii[:3]:
        _same_radius(emu.search_radius_lists(sub, r)[:2], ref.search_radius(sub, r), r)
    more = np.ascontiguousarray(np.concatenate([pts[:1], pts]))
    with pytest.raises(RuntimeError, match=lc.REFUSAL):
        EmulatedTree(more, lc.EDGE_LEAF)
    host = pt.KdTree(more, pt.Metric.L2Squared, lc.EDGE_LEAF, device=pt.PTK_DEVICE_NONE)
    lc.assert_leaf(host, lc.EDGE_LEAF)  # (the same leaf: the position bits alone went over)


# ---- gpu tier ----------------------------------------------------------------------------------------------------------

def _within_rows(ref, q, k, r):
    """search_knn_within's rows from the reference's search_knn rows, r one radius or one per row: the entries below the
    radius, the pad (-1, r) behind them."""
    kk = min(k, ref.n)
    rows = ref.search_knn(q, kk)
    r = np.broadcast_to(np.asarray(r, dtype=ref.dtype), (len(q),))[:, None]
    out = np.zeros((len(q), k), dtype=rows.dtype)
    out["index"], out["distance"] = -1, r
    keep = rows["distance"] < r
    out[:, :kk][keep] = rows[keep]
    return out


def _radius_rows(ref, q, r):
    """(offsets, flat) of the reference with one radius per row: one run per distinct radius."""
    off, parts = np.zeros(len(q) + 1, dtype=np.uint64), [None] * len(q)
    for v in np.unique(r):
        at = np.flatnonzero(r == v)
        o, flat = ref.search_radius(np.ascontiguousarray(q[at]), v)
        for j, i in enumerate(at):
            parts[i] = flat[int(o[j]):int(o[j + 1])]
    off[1:] = np.cumsum([len(x) for x in parts])
    return off, np.concatenate(parts)


def _tree(gpu, pts, L, metric="L2Squared"):
    tree = pt.KdTree(np.asarray(pts), pt.Metric[metric], L, device=gpu)
    lc.assert_leaf(tree, L)
    return tree


def _query_searches(tree, ref, pts, q, radii, ks_, full=True):
    """What _all_entry_points of tests/test_depth_boundaries.py runs, at the radii of the leaf case."""
    for k in ks_:
        _knn(tree, ref, q, k)
    if full:
        _knn(tree, ref, q, 1, e=1.25)
        _knn(tree, ref, q, 6, e=1.25)
    for r in radii:
        _radius(tree, ref, q, r)
    for r in (radii[0], radii[1], radii[3]):
        _radius(tree, ref, q, r, sort=True)
    if full:
        lo, hi = _boxes(pts, q)
        boxes = np.empty((2 * len(lo), pts.shape[1]), dtype=pts.dtype)
        boxes[0::2], boxes[1::2] = lo, hi
        got = tree.search_box(boxes)
        _same_box((got.offsets, got.flat), ref.search_box(lo, hi), len(pts))
    for r in radii:
        for k in (5, 80):
            got = tree.search_knn_within(q, k, r, _prefilled((len(q), k), tree.dtype_neighbor))
            assert same_rows(got, _within_rows(ref, q, k, r)), ("search_knn_within", k, r)
        want = count_expected(ref, q, r)
        for mc in (0, 16):
            assert np.array_equal(tree.count_within(q, r, mc), np.minimum(want, mc) if mc else want), ("count_within", r, mc)


@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.LEAVES + (ONE_LEAF,))
def test_3d_default_metric_at_every_leaf_boundary(gpu, L):
    pts, blob, q, nb, ref, radii = _case(L)
    tree = _tree(gpu, pts, L)
    _query_searches(tree, ref, pts, q, radii, (1, 5, 40, 80))
    # k = 1 with the view without piles off (test hook): the two-phase search on the tree as it was built
    pt.set_test_knobs(pile_view=0)
    whole = _tree(gpu, pts, L)
    _knn(whole, ref, q, 1)
    _knn(whole, ref, q, 1, e=1.25)


@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.LEAVES + (ONE_LEAF,))
def test_3d_radii_per_row_and_device_buffers_at_every_leaf_boundary(gpu, L):
    import torch

    pts, blob, q, nb, ref, radii = _case(L)
    tree = _tree(gpu, pts, L)
    per_row = np.resize(np.array(radii, dtype=np.float32), len(q))  # r_part, r_all, 0 and 1e4 in turn
    for k in (5, 80):
        got = tree.search_knn_within(q, k, per_row, _prefilled((len(q), k), tree.dtype_neighbor))
        assert same_rows(got, _within_rows(ref, q, k, per_row)), ("search_knn_within, per row", k)
    want = _radius_rows(ref, q, per_row)
    counts = np.diff(want[0].astype(np.int64))
    for mc in (0, 16):
        assert np.array_equal(tree.count_within(q, per_row, mc), np.minimum(counts, mc) if mc else counts), ("count_within, per row", mc)
    got = tree.search_radius(q, per_row)
    _same_radius((got.offsets, got.flat), want, "search_radius, per row")
    dq = torch.from_numpy(np.array(q)).to(f"cuda:{gpu}")
    for r in radii:
        want = ref.search_radius(q, r)
        off, raw = tree.search_radius_device(dq, np.float32(r))
        torch.cuda.synchronize()
        assert np.array_equal(off.cpu().numpy().astype(np.uint64), want[0]) and raw.cpu().numpy().tobytes() == want[1].tobytes(), r


@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.LEAVES + (ONE_LEAF,))
def test_3d_self_searches_at_every_leaf_boundary(gpu, L):
    pts, blob, q, nb, ref, radii = _case(L)
    pts = np.asarray(pts)
    tree = _tree(gpu, pts, L)
    host = pt.KdTree(pts, pt.Metric.L2Squared, L, device=pt.PTK_DEVICE_NONE)
    lc.assert_leaf(host, L)
    want7 = ks.expected(ref, pts, 7)
    assert tree.self_route(7) == 1 and same_rows(tree.search_knn_self(7), want7), "search_knn_self (direct)"
    pt.set_test_knobs(self_route=2)
    assert same_rows(tree.search_knn_self(7), want7), "search_knn_self (staged)"
    pt.set_test_knobs(self_route=None)
    for r in lc.self_radii(L, radii):
        want = lc.self_rows(ref, pts, r)
        counts = rs.clamp(want[0], 0)
        assert r != radii[1] or np.all(counts[len(pts) - L:] == L - 1)  # (r_all: every blob point's row is the blob)
        for mc in (0, 7):
            assert np.array_equal(tree.count_within_self(r, mc), np.minimum(counts, mc) if mc else counts), ("count_within_self", r, mc)
        got = tree.search_radius_self(r)
        _same_radius((got.offsets, got.flat), want, ("search_radius_self", r))
        assert np.array_equal(tree.cluster_within_self(r, min_neighbors=2), cs.expected_labels(*want, 2)), ("cluster", r)
        frames, moments = tree.normals_within_self(r, moments=True)
        want_m = ns.expected_moments(pts, *want)
        assert moments.tobytes() == want_m.tobytes(), ("moments", r)
        assert frames.tobytes() == ns.host_normals(host, r, want="frames")[0].tobytes(), ("frames", r)
        ns.check_frames(frames, want_m, pts, None, 2, ("normals", L, r))


@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.SMALL_LEAVES)
@pytest.mark.parametrize("metric", ["L1", "LPInf", "LNInf"])
def test_3d_other_metrics_at_the_leaf_boundaries(gpu, metric, L):
    pts, blob, q, nb, ref, radii = _case(L, metric=metric)
    _query_searches(_tree(gpu, pts, L, metric), ref, pts, q, radii, (1, 5, 40), full=False)


@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.SMALL_LEAVES)
@pytest.mark.parametrize("dim", [2, 5])
def test_2d_and_5d_at_the_leaf_boundaries(gpu, dim, L):
    pts, blob, q, nb, ref, radii = _case(L, dim)
    _query_searches(_tree(gpu, pts, L), ref, pts, q, radii, (1, 5, 40, 80))


@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.SMALL_LEAVES)
@pytest.mark.parametrize("dim", [3, 5])
def test_float64_at_the_leaf_boundaries(gpu, dim, L):
    pts, blob, q, nb, ref, radii = _case(L, dim, np.float64)
    tree = _tree(gpu, pts, L)
    for k in (1, 8, 32, 40, 80):
        _knn(tree, ref, q, k)
    for r in radii:
        _radius(tree, ref, q, r)
        want = count_expected(ref, q, r)
        for mc in (0, 16):
            assert np.array_equal(tree.count_within(q, r, mc), np.minimum(want, mc) if mc else want), ("count_within", r, mc)
        if dim == 3:
            got = tree.search_knn_within(q, 5, r, _prefilled((len(q), 5), tree.dtype_neighbor))
            assert same_rows(got, _within_rows(ref, q, 5, r)), ("search_knn_within", r)
    _radius(tree, ref, q, radii[0], sort=True)
    lo, hi = _boxes(pts, q)
    boxes = np.empty((2 * len(lo), dim), dtype=np.float64)
    boxes[0::2], boxes[1::2] = lo, hi
    got = tree.search_box(boxes)
    _same_box((got.offsets, got.flat), ref.search_box(lo, hi), len(pts))


@needs_reference64
@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.SMALL_LEAVES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("metric", ["SO2", "SE2Squared"])
def test_topological_metrics_at_the_leaf_boundaries(gpu, metric, dtype, L):
    dim = 1 if metric == "SO2" else 3
    pts, blob, q, nb, ref, radii = _case(L, dim, np.dtype(dtype), metric)
    tree = _tree(gpu, pts, L, metric)
    for k in (1, 7, 40):
        _knn(tree, ref, q, k)
    for r in radii:
        _radius(tree, ref, q, r)
        if dtype == "float32":
            for mc in (0, 16):
                assert np.array_equal(tree.count_within(q, r, mc), count_expected(ref, q, r, mc)), ("count_within", r, mc)
    real = np.dtype(dtype).type
    lo, hi = (q - real(0.004)).astype(dtype), (q + real(0.004)).astype(dtype)  # (boxes that cut the blob; none wraps)
    keep = (lo[:, dim - 1] >= 0) & (hi[:, dim - 1] <= 1)
    lo, hi = np.ascontiguousarray(lo[keep]), np.ascontiguousarray(hi[keep])
    boxes = np.empty((2 * len(lo), dim), dtype=dtype)
    boxes[0::2], boxes[1::2] = lo, hi
    got = tree.search_box(boxes)
    off, flat = ref.search_box(lo, hi)
    assert np.array_equal(got.offsets, off) and np.array_equal(got.flat, flat), "search_box"
    assert np.diff(off.astype(np.int64))[:nb].max() >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("L", lc.LEAVES)
def test_forced_caps_at_every_leaf_boundary(gpu, L):
    """A cap of 1 (test hooks) hands nearly every query to the cooperative finishes: the k-NN ones at every leaf size, the
    radius ones up to 2048 points -- 64 pieces, every piece number of their keys -- and not at 2049, whatever the hook
    says (radius_cap(), radius64_cap())."""
    import torch

    pts, blob, q, nb, ref, radii = _case(L)
    tree = _tree(gpu, pts, L)
    pt.set_test_knobs(knn_cap=1, knn_cap_min_nq=1, radius_cap=1)
    for k in (5, 40):
        _knn(tree, ref, q, k)
        assert tree.knn_coop_counts()["cooperative"] > 0, k
    dq = torch.from_numpy(np.array(q)).to(f"cuda:{gpu}")
    handed = 0
    for r in radii:
        want = ref.search_radius(q, r)
        off, raw = tree.search_radius_device(dq, np.float32(r))  # (the counters are those of a device-buffer count pass)
        torch.cuda.synchronize()
        assert np.array_equal(off.cpu().numpy().astype(np.uint64), want[0]) and raw.cpu().numpy().tobytes() == want[1].tobytes(), r
        handed += tree.radius_coop_counts()["cooperative"]
        _radius(tree, ref, q, r)
    assert (handed > 0) if L <= 2048 else (handed == 0), handed
    if L in (2047, 2048):  # the side query: the finish scans all 64 pieces of the blob leaf and keeps the row
        qs, r = lc.side_query(ref, L)
        want = ref.search_radius(qs, r)
        off, raw = tree.search_radius_device(torch.from_numpy(qs).to(f"cuda:{gpu}"), np.float32(r))
        torch.cuda.synchronize()
        assert np.array_equal(off.cpu().numpy().astype(np.uint64), want[0]) and raw.cpu().numpy().tobytes() == want[1].tobytes()
        counts = tree.radius_coop_counts()
        assert counts["cooperative"] == 1 and counts["recounted"] == 0, counts
        _radius(tree, ref, qs, r)
    pt.set_test_knobs()

    pts, blob, q, nb, ref, radii = _case(L, dtype=np.float64)
    tree = _tree(gpu, pts, L)
    pt.set_test_knobs(knn64_cap=1, knn_cap_min_nq=1, radius64_cap=1)
    for k in (5, 32):
        _knn(tree, ref, q, k)
        assert tree.knn_coop_counts()["cooperative"] > 0, k
    handed = 0
    for r in radii:
        _radius(tree, ref, q, r)
        handed += tree.knn_coop_counts()["cooperative"]
    assert (handed > 0) if L <= 2048 else (handed == 0), handed
    if L in (2047, 2048):
        qs, r = lc.side_query(ref, L)
        _radius(tree, ref, qs, r)
        counts = tree.knn_coop_counts()
        assert counts["cooperative"] == 1 and counts["redone"] == 0, counts  # (handed over, and not searched again)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_every_bit_of_the_leaf_reference_in_use(gpu, dtype):
    """2^19 - 1 points with a leaf of 4095: 19 position bits and 12 count bits.  The query-based searches only."""
    pts, blob, q, nb, ref, radii = lc.case(lc.EDGE_LEAF, dtype=np.dtype(dtype), n=lc.EDGE_N - lc.EDGE_LEAF)
    assert len(pts) == lc.EDGE_N
    tree = _tree(gpu, pts, lc.EDGE_LEAF)
    sub = np.ascontiguousarray(q[:56])
    for k in (1, 5, 40, 80):
        _knn(tree, ref, sub, k)
    for r in radii[:3]:
        _radius(tree, ref, sub, r)
        got = tree.search_knn_within(sub, 5, r)
        assert same_rows(got, _within_rows(ref, sub, 5, r)), ("search_knn_within", r)
        assert np.array_equal(tree.count_within(sub, r), count_expected(ref, sub, r)), ("count_within", r)
    _radius(tree, ref, sub[:4], radii[3])  # (the whole tree: four rows of half a million entries)
    lo, hi = sub - pts.dtype.type(0.004), sub + pts.dtype.type(0.004)
    boxes = np.empty((2 * len(lo), 3), dtype=pts.dtype)
    boxes[0::2], boxes[1::2] = lo, hi
    got = tree.search_box(boxes)
    off, flat = ref.search_box(lo, hi)
    assert np.array_equal(got.offsets, off) and np.array_equal(got.flat, flat), "search_box"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_one_point_more_than_the_leaf_reference_holds_is_refused(gpu, dtype):
    pts, _ = lc.cloud_with_leaf(lc.EDGE_LEAF, dtype=np.dtype(dtype), n=lc.EDGE_N - lc.EDGE_LEAF)
    more = np.ascontiguousarray(np.concatenate([pts[:1], pts]))
    assert len(more) == 1 << 19
    with pytest.raises(pt.PtkError, match=lc.REFUSAL) as err:
        pt.KdTree(more, pt.Metric.L2Squared, lc.EDGE_LEAF, device=gpu)
    assert err.value.status == -2  # PTK_ERR_UNSUPPORTED
