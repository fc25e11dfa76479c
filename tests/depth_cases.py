"""Trees of an exact depth, and the queries that fill their record stacks (tests/test_depth_boundaries.py).

Almost every launch decision of the library is made from ``max_depth`` ("Depth boundaries"): the private spill
class of the record stack (39 | 40, 135 | 136 levels), the HBM spill of a deep tree (1031 | 1032), the keys of the
cooperative radius finish (51 | 52) and the seed of the float64 ``search_knn_within`` (1024 | 1025).  A cloud of
coincident points peels one level per point under the sliding-midpoint rule, so the depth of a tree is controllable to
the level: 3 000 uniform points plus a pile of ``c`` coincident ones.

Where the pile sits decides how full the stacks get.  Far outside the cloud -- at the end of the longest side of the
root box -- the chain of one-point peels starts at level 1, and a query next to the pile, off it by the same small step
on every axis, enters the far child on nearly every level of the chain: two undo records per level, ``2 * depth + 2``
in the limit (``ptk_backend_core.hpp``, "Stack geometry").  The high-water marks these queries reach in the CPU
emulator are in ``FILL`` below.
"""

from __future__ import annotations

import functools

import numpy as np

import pico_tree_amd as pt
from pico_tree_amd import datasets as ds

#: Step of the corner queries off the pile, per axis.
STEP = 1e-2

#: Records on the fullest stack of the corner queries through the generic kernels, as ``need - high water`` with
#: ``need = 2 * depth + 2``, measured in the CPU emulator (tests/emu.py ``stack_high_water``) at depths 39 and 135 --
#: the same at both, for k = 1 / 5 / 40 and radius 1e4 (a radius that leaves the cloud out, 0.05, holds one record
#: fewer: the root's pending one).
#: tests/test_depth_boundaries.py asserts each of them again: at most 8 below the need is the bar of a case that really
#: fills its stacks.
#:   (space, dim, leaf) -> need - high water
FILL = {("euclid", 3, 1): 6, ("euclid", 3, 10): 6, ("euclid", 2, 4): 5, ("euclid", 5, 1): 8}

#: The topological trees.  A pile of coincident points cannot fill their stacks: below its first levels the box of a
#: pile is a single point, both child intervals of a branch are that point, the interval distances of a query to them
#: are equal and the topological descent (``d1 < d2``, traverse_topo) goes right on every level, where the measurements
#: say the chain is -- the far child is the one-point leaf, whose two undo records are gone again before the next
#: level: high water depth + 1 (SO2) and depth + 4 (SE2Squared), half the need.  So up to 136 levels these trees are
#: built from a chain of DISTINCT points instead, ``x_i = 0.3 * 2^-i`` (``chain_at_depth``): every level splits the one
#: point nearest the cloud off the rest, a query between the chain and the cloud finds that one-point leaf the nearer
#: child on every level, and a radius search that holds the whole tree (1e4) pays two undo records per level.  The
#: coincident pile stays for 1031 | 1032 only: float32 has no room for a chain of a thousand halvings (the chain of 136
#: levels already ends among the subnormal numbers on the circle, whose axis is [0, 1]), and those cases check parity
#: and the invariant, not the fill.
#:   space -> (dim, leaf, need - high water of search_radius(1e4) on the fill queries, measured at all four depths)
TOPO = {"SO2": (1, 1, 2), "SE2Squared": (3, 4, 5)}


#: (dim, leaf, metric) of the euclidean families
EUCLID_CASES = [(3, 1, "L2Squared"), (3, 10, "L2Squared"), (3, 10, "L1"), (3, 10, "LPInf"), (3, 10, "LNInf"),
                (2, 4, "L2Squared"), (2, 4, "L1"), (5, 1, "L2Squared"), (5, 1, "L1")]


def need(depth):
    """Records a traversal of a tree of that depth may hold (ptk_kernels.hpp, "The host's choice of OVF")."""
    return 2 * depth + 2


class Watch:
    """Runs one emulated search at a time and checks the high-water mark of its record stacks: never above the
    invariant, never above what the host's spill class for this depth holds.  ``lib``: the emulator library the search
    runs in, if not tests/cpp/libptk_emu.so."""

    def __init__(self, depth, lib=None):
        from tests.emu import ovf_capacity

        self.depth, self.lib, self.high = depth, lib, 0
        self.cap = ovf_capacity(depth)

    def __call__(self, search, *args, **kw):
        from tests.emu import stack_high_water

        stack_high_water(lib=self.lib)
        got = search(*args, **kw)
        self.high = stack_high_water(lib=self.lib)
        assert self.high <= need(self.depth), ("more records than 2 * depth + 2", self.high, self.depth)
        assert self.cap is None or self.high <= self.cap, ("more records than the host's class holds", self.high, self.cap)
        return got


def edge_radii(ref, q):
    """r exactly the (metric) distance of the first corner query to the pile -- the test of the bounded searches is
    strict: the pile is out --, the next number above it -- the pile is in --, 0, and 1e4: the whole tree, the cloud
    included, so that the root's pending record is on the stack as well and the stacks fill as the plain searches' do."""
    d = ref.search_knn(q[:1], 1)["distance"][0, 0]
    return [d, np.nextafter(d, d.dtype.type(np.inf)), d.dtype.type(0), d.dtype.type(1e4)]


def _base(space, dim):
    """3 000 uniform points; (pile, axes the corner queries step along)."""
    u = ds.uniform_cloud(3_000, dim, 31)
    pile = np.zeros(dim, dtype=np.float32)
    if space == "SO2":  # the circle [0, 1]: the cloud on its lower half, the pile at the far end of the box
        return u * np.float32(0.5), np.array([0.98], dtype=np.float32)
    if space == "SE2Squared":  # x, y on the line, the angle in [0, 1): the pile at the end of the x side, mid-circle
        u[:, :2] -= np.float32(0.5)
        pile[0], pile[2] = -50.0, 0.5
        return u, pile
    pile[0] = -50.0
    return u - np.float32(0.5), pile


def _host_depth(pts, leaf):
    return pt.KdTree(pts, pt.Metric.L2Squared, leaf, device=pt.PTK_DEVICE_NONE).info()["max_depth"]


@functools.lru_cache(maxsize=None)
def _cloud(depth, dim, leaf, dtype, space):
    base, pile = _base(space, dim)
    base, pile = base.astype(dtype), pile.astype(dtype)

    def cloud(c):
        return np.ascontiguousarray(np.concatenate([base, np.repeat(pile[None, :], c, axis=0)]))

    # (one level per point of the pile: two builds find the size, the third confirms that it is the smallest)
    c = max(depth, 2)
    for _ in range(4):
        d = _host_depth(cloud(c), leaf)
        if d == depth:
            break
        c += depth - d
        assert c >= 1, (depth, dim, leaf, "the base cloud alone is deeper than that")
    pts = cloud(c)
    assert _host_depth(pts, leaf) == depth and _host_depth(cloud(c - 1), leaf) == depth - 1, (depth, dim, leaf, c)
    pts.flags.writeable = False
    pile.flags.writeable = False
    return pts, pile


def cloud_at_depth(depth, dim, leaf, dtype=np.float32, space="euclid"):
    """(points, pile): the base cloud plus the smallest pile whose host-built tree has ``max_depth == depth``.  The
    arrays are shared between the tests and read-only."""
    return _cloud(int(depth), int(dim), int(leaf), np.dtype(dtype), space)


def assert_depth(tree, depth):
    """The handle under test has exactly that depth (the device replica is encoded from the same host tree)."""
    assert tree.info()["max_depth"] == depth, (tree.info()["max_depth"], depth)


def corner_queries(pile):
    """The 2^dim points ``pile +- STEP`` (32 of them with seeded signs beyond 5 dimensions)."""
    dim = len(pile)
    if dim <= 5:
        signs = np.array([[1.0 if (i >> a) & 1 else -1.0 for a in range(dim)] for i in range(1 << dim)])
    else:
        signs = np.where(np.random.default_rng(33).random((32, dim)) < 0.5, -1.0, 1.0)
    return np.ascontiguousarray((pile[None, :] + signs * STEP).astype(pile.dtype))


def queries(pts, pile, space="euclid"):
    """At most about 450 queries: the corners, the pile itself, its neighbours in the number format along axis 0, 300
    uniform queries over the cloud and 50 points of the tree (zero distances).  The corners come first."""
    dim, dtype = len(pile), pile.dtype
    corners = corner_queries(pile)
    near = np.repeat(pile[None, :], 3, axis=0)
    near[1, 0] = np.nextafter(pile[0], dtype.type(np.inf))
    near[2, 0] = np.nextafter(pile[0], dtype.type(-np.inf))
    uni = ds.uniform_cloud(300, dim, 32)
    if space == "SO2":
        uni = uni * np.float32(0.5)
    elif space == "SE2Squared":
        uni[:, :2] -= np.float32(0.5)
    else:
        uni = uni - np.float32(0.5)
    own = pts[:: max(1, 3_000 // 50)][:50]
    q = np.ascontiguousarray(np.concatenate([corners, near, uni.astype(dtype), own]).astype(dtype))
    if space == "SO2":
        q = np.clip(q, 0.0, 1.0).astype(dtype)
    return q, len(corners)


# ---- the topological trees up to 136 levels: a chain of distinct points ----------------------------------------------

def _chain_base(space):
    """3 000 uniform points right of the chain: x in [0.5, 1) on the circle, [0.5, 1.5) on the line."""
    if space == "SO2":
        return ds.uniform_cloud(3_000, 1, 31) * np.float32(0.5) + np.float32(0.5)
    u = ds.uniform_cloud(3_000, 3, 31)
    u[:, 0] += np.float32(0.5)
    u[:, 1] -= np.float32(0.5)
    return u


@functools.lru_cache(maxsize=None)
def _chain(depth, space):
    dim, leaf, _ = TOPO[space]
    base = _chain_base(space)

    def cloud(c):
        chain = np.zeros((c, dim), dtype=np.float32)
        chain[:, 0] = np.float32(0.3) * np.exp2(-np.arange(c, dtype=np.float64)).astype(np.float32)
        if dim == 3:
            chain[:, 2] = 0.5
        return np.ascontiguousarray(np.concatenate([base, chain]))

    c = depth
    for _ in range(6):
        d = _host_depth(cloud(c), leaf)
        if d == depth:
            break
        c += depth - d
        assert 1 <= c <= 147, (depth, space, c)  # (0.3 * 2^-147 is the last positive float32 of the chain)
    pts = cloud(c)
    assert _host_depth(pts, leaf) == depth and _host_depth(cloud(c - 1), leaf) == depth - 1, (depth, space, c)
    assert len(np.unique(pts[3_000:, 0])) == c
    pts.flags.writeable = False
    return pts, c


def chain_at_depth(depth, space):
    """(points, chain length): the base cloud plus the shortest chain ``0.3 * 2^-i`` (y = 0, angle 0.5 for SE2Squared) whose
    host-built tree has ``max_depth == depth``; dim and leaf size are TOPO[space]'s.  Shared and read-only."""
    return _chain(int(depth), space)


def chain_queries(pts, space):
    """(queries, n): n fill queries first -- between the head of the chain (0.3) and the cloud (0.5), on the chain's
    line and next to it --, then the head of the chain and its neighbours in float32, 300 uniform queries over the circle
    / the cloud's box (the ones next to 1 reach the tail of the chain through the seam), 30 points of the cloud and 20
    of the chain (zero distances)."""
    dim = pts.shape[1]
    xs = np.array([0.45, 0.4, 0.35, 0.31], dtype=np.float32)
    if dim == 1:
        fill = xs[:, None]
    else:
        fill = np.array([[x, y, a] for y, a in ((0, 0.5), (0.01, 0.51), (-0.01, 0.49)) for x in xs], dtype=np.float32)
    head = np.repeat(pts[3_000][None, :], 3, axis=0)
    head[1, 0] = np.nextafter(head[0, 0], np.float32(np.inf))
    head[2, 0] = np.nextafter(head[0, 0], np.float32(-np.inf))
    uni = ds.uniform_cloud(300, dim, 32)
    if dim == 3:
        uni[:, 0] *= np.float32(1.5)
        uni[:, 1] -= np.float32(0.5)
    own = np.concatenate([pts[:3_000:100], pts[3_000:][:: max(1, (len(pts) - 3_000) // 20)][:20]])
    return np.ascontiguousarray(np.concatenate([fill, head, uni, own]).astype(np.float32)), len(fill)
