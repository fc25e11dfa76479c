"""Non-finite and overflowing inputs, and k beyond the register lists, on every search path.

The contract (include/ptk.h, "Non-finite and overflowing inputs"): a query row or box corner with NaN, +-Inf or any
finite value gets what the reference gives it, for every entry the reference writes; no row changes another row's
result; a k-NN slot the reference's search never writes holds {0, FLT_MAX} ({0, DBL_MAX}, padding zero) on every path;
a tree is not built from points that are NaN or +-Inf.

Everything is compared with the COMPILED reference (oracle/_ref) through tests/poison.py: `poison()` makes the batch,
`written_by_reference()` finds the entries the reference writes, `expect_rows()` puts the documented filler into the
rest, and the comparison is byte for byte on the whole batch.

CPU tier (no marker): the product's kernel source under the lane emulator (tests/emu.py), the library's host loop on a
host-only handle, tree creation.  GPU tier (`gpu` marker): the Python wrapper -> C ABI -> device, host arrays and torch
tensors.  The emulator replaces `ds_min_u32` on float bits, `v_med3_f32` and the float -> uint conversions of the Morton
keys with host code: what those do with a NaN is shown by the GPU tier only.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import poison as P
from tests.emu import EmulatedTree, EmulatedTree64

needs_reference = pytest.mark.skipif(not (oracle.have_reference() and oracle.have_reference64()),
                                     reason="compiled reference not present")

FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
LEAF = 10
PTK_ERR_INVALID = -1  # (ptk.h)


# ---- clouds ---------------------------------------------------------------------------------------------------------

def _lattice(n, seed, cells, dim=3):
    return np.ascontiguousarray(np.round(ds.uniform_cloud(n, dim, seed) * cells) / cells, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _cloud(name, n, nq):
    """(points, clean queries) -- float32; the double tests scale them by 1.0000001 as smoke() does."""
    if name == "lidar":
        return ds.lidar_cloud(n, seed=71), ds.lidar_cloud(nq, seed=72, pose=(3.0, 1.5))
    if name == "ties":  # a lattice: equal distances everywhere, queries on and between the points
        return _lattice(n, 73, 8), _lattice(nq, 74, 16)
    if name == "dim2":
        return ds.uniform_cloud(n, 2, 75), ds.uniform_cloud(nq, 2, 76)
    if name == "dim5":
        return ds.uniform_cloud(n, 5, 77), ds.uniform_cloud(nq, 5, 78)
    if name == "uniform":
        return ds.uniform_cloud(n, 3, 79), ds.uniform_cloud(nq, 3, 80)
    raise KeyError(name)


def _as64(a):
    return np.ascontiguousarray(a.astype(np.float64) * 1.0000001)


class _Case:
    """A cloud, its poisoned batch and the compiled reference over it; expected k-NN rows are made once per (k, e)."""

    def __init__(self, name, n, nq, metric="L2Squared", dtype=np.float32, seed=5, pts=None, q=None):
        p, c = _cloud(name, n, nq) if pts is None else (pts, q)
        self.name, self.metric, self.dtype = name, metric, np.dtype(dtype)
        self.pts = p if self.dtype == np.float32 else _as64(p)
        self.clean = c if self.dtype == np.float32 else _as64(c)
        self.q, self.mask = P.poison(self.clean, seed)
        self.ref = oracle.Oracle(self.pts, LEAF, "reference", metric, dtype=dtype)
        self.ref.set_threads(self.ref.max_threads())
        self._want = {}

    def want(self, k, e=None):
        if (k, e) not in self._want:
            rows, written = P.written_by_reference(self.ref, self.q, k, self.mask, e=e)
            self._want[(k, e)] = P.expect_rows(rows, written)
        return self._want[(k, e)]

    def check(self, got, k, e=None, what=""):
        want = self.want(k, e)
        assert P.same_rows(got, want), (self.name, self.metric, k, what, P.first_difference(got, want, self.mask))

    def radii(self):
        """A median nearest distance of the clean batch, 25 x it, the largest finite scalar, +inf."""
        nearest = self.ref.search_knn(self.clean, 1)["distance"][:, 0]
        med = self.dtype.type(np.median(nearest[nearest > 0]))
        return med, self.dtype.type(25) * med, np.finfo(self.dtype).max, self.dtype.type(np.inf)


@functools.lru_cache(maxsize=None)
def _case(name, n, nq, metric="L2Squared", dtype=np.float32):
    return _Case(name, n, nq, metric, dtype)


def _same_radius(got, want, what, sort=False):
    goff, grows = got[0], got[1]
    woff, wrows = want
    assert np.array_equal(np.asarray(goff).astype(np.uint64), woff), what
    if sort:  # (std::sort is unstable: the order among equal distances is unspecified on both sides)
        assert np.array_equal(np.ascontiguousarray(grows["distance"]).view(np.uint8),
                              np.ascontiguousarray(wrows["distance"]).view(np.uint8)), what
    else:  # (field by field: the padding bytes of the reference's double records are whatever its vectors held)
        assert np.array_equal(grows["index"], wrows["index"]), what
        assert np.ascontiguousarray(grows["distance"]).tobytes() == np.ascontiguousarray(wrows["distance"]).tobytes(), what


# ---- the helper itself ----------------------------------------------------------------------------------------------

def test_poison_makes_the_batch_the_issue_describes():
    for dtype in (np.float32, np.float64):
        q = np.zeros((5_000, 3), dtype=dtype) + dtype(1.5)
        p, mask = P.poison(q, 9)
        assert mask[0] and mask[-1] and 250 <= mask.sum() <= 250 + P.EXTRA_ROWS
        assert ((p != q) | np.isnan(p)).sum(axis=1)[mask].tolist() == [1] * int(mask.sum())  # one coordinate per row
        assert np.array_equal(p[~mask], q[~mask])
        runs = [s for s in range(0, 5_000, 64) if mask[s:s + 64].all()]
        assert runs, "no whole wavefront of poisoned rows"
        vals = p[mask][(p[mask] != 1.5)]
        pal = P.palette(dtype)
        assert np.isnan(vals).any() and all((vals == v).any() for v in pal[1:])
        with np.errstate(over="ignore"):
            assert np.isfinite(pal[5:] * pal[5:]).all() and not np.isfinite(pal[3] * pal[3])
        again, mask2 = P.poison(q, 9)
        assert np.array_equal(mask, mask2) and again.tobytes() == p.tobytes()


@needs_reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_leaves_rows_it_does_not_fill_as_it_found_them(dtype):
    """What `written_by_reference()` rests on: a NaN / +-Inf / +-MAX row accepts nothing and the reference writes the
    distance of slot k - 1 only; a huge finite row has a full list; clean rows are always full."""
    c = _case("lidar", 2_000, 384, dtype=dtype)
    rows, written = P.written_by_reference(c.ref, c.q, 5, c.mask)
    bad = ~np.isfinite(c.q).all(axis=1) | (np.abs(c.q) == np.finfo(dtype).max).any(axis=1)
    assert bad.any() and (bad <= c.mask).all()
    assert not written[bad][:, :, 0].any() and not written[bad][:, :4, 1].any() and written[bad][:, 4, 1].all()
    assert (rows["distance"][bad, 4] == np.finfo(dtype).max).all()
    assert written[~bad].all()
    want = P.expect_rows(rows, written)
    assert (want["index"][bad] == 0).all() and (want["distance"][bad] == np.finfo(dtype).max).all()


# ---- emulator: k-NN -------------------------------------------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("name", ["lidar", "ties", "dim2", "dim5"])
def test_emulated_knn_with_poisoned_rows(name):
    """knn_kernel / knn_reg_kernel / the any-dimension kernels: k-list in the row, in LDS and in registers, the small
    stack, Morton and identity launch order, exact and approximate."""
    c = _case(name, 2_000, 384)
    emu = EmulatedTree(c.pts, LEAF)
    perm = emu.morton_permutation(c.q)[0] if c.pts.shape[1] <= 3 else None
    for k in (1, 4, 16, 40, 80):
        for small in (False, True):
            for lds in (False, True, 2):
                if lds == 2 and k > 32:
                    continue
                p = perm if small else None
                c.check(emu.search_knn(c.q, k, perm=p, small_stack=small, list_in_lds=lds), k, what=(small, lds))
    c.check(emu.search_knn(c.q, 8, e=1.3), 8, e=1.3, what="approximate")
    c.check(emu.search_knn(c.q, 1, e=1.3), 1, e=1.3, what="approximate")


@needs_reference
@pytest.mark.parametrize("name", ["lidar", "ties", "dim2"])
def test_emulated_two_phase_knn1_with_poisoned_rows(name):
    """The two-phase k = 1 search: uncapped (3, 4), capped with the cooperative search and the redo pass (5 - 8), the
    ranked classes straight to the cooperative search (9); and on the view without the piles for the lattice."""
    c = _case(name, 2_000, 384)
    emu = EmulatedTree(c.pts, LEAF)
    perm, _ = emu.morton_permutation(c.q)
    for variant in (3, 4, 5, 6, 7, 8, 9):
        for p in ((None, perm) if variant in (3, 5) else (perm,)):
            got, _ = emu.two_phase_knn1(c.q, perm=p, variant=variant)
            c.check(got, 1, what=("variant", variant))
            if variant >= 5:
                redo = emu.last_coop()[1]
                emu.two_phase_knn1(c.clean, perm=p, variant=variant)
                assert redo <= int(c.mask.sum()) + emu.last_coop()[1], (name, variant, redo)
    got, _ = emu.two_phase_knn1(c.q, e=1.4, perm=perm, variant=3)
    c.check(got, 1, e=1.4, what="approximate")
    if name == "ties":  # subtrees of coincident points: the k = 1 search on the view without them (ptk_piles.hpp)
        pts = c.pts.copy()
        pts[:300] = pts[0]
        piles = _Case("piles", 0, 0, pts=pts, q=c.clean)
        view = EmulatedTree(piles.pts, LEAF)
        assert view.use_pile_view() > 0
        for variant in (5, 3, 9):
            got, _ = view.two_phase_knn1(piles.q, perm=perm, variant=variant)
            piles.check(got, 1, what=("pile view", variant))


@needs_reference
@pytest.mark.parametrize("name,metric", [("lidar", "L2Squared"), ("ties", "L2Squared"), ("lidar", "L1")])
def test_emulated_capped_knn_with_poisoned_rows(name, metric):
    """The general kernel capped at 4 far children, knn_coop_kernel for what it hands over (a small pool too), the
    reference search of what that cannot certify.  A poisoned row may cost a redo; it costs no more than that."""
    c = _case(name, 2_000, 128, metric)  # (two wavefronts, one of them poisoned rows only)
    emu = EmulatedTree(c.pts, LEAF, pt.Metric[metric])
    perm, _ = emu.morton_permutation(c.q)
    for k, p, small in ((4, None, False), (16, perm, True), (40, None, True)):
        got, heavy, redo = emu.search_knn_capped(c.q, k, 4, perm=p, pool_small=small)
        c.check(got, k, what=("cap 4", small))
        _, _, clean_redo = emu.search_knn_capped(c.clean, k, 4, perm=p, pool_small=small)
        assert heavy > 0 and redo <= int(c.mask.sum()) + clean_redo, (name, k, heavy, redo, clean_redo)


@needs_reference
@pytest.mark.parametrize("name", ["lidar", "ties"])
def test_emulated_double_knn_with_poisoned_rows(name):
    c = _case(name, 2_000, 192, dtype=np.float64)
    emu = EmulatedTree64(c.pts, LEAF)
    for k in (1, 16, 40, 80):
        for reg in (True, False):
            c.check(emu.search_knn(c.q, k, list_in_registers=reg), k, what=("registers", reg))
    c.check(emu.search_knn(c.q, 4, e=1.3), 4, e=1.3, what="approximate")
    for k in (4, 16):
        got, heavy, redo = emu.search_knn_capped(c.q, k, 4)
        c.check(got, k, what="cap 4")
        _, _, clean_redo = emu.search_knn_capped(c.clean, k, 4)
        assert heavy > 0 and redo <= int(c.mask.sum()) + clean_redo, (name, k, heavy, redo, clean_redo)


@needs_reference
@pytest.mark.parametrize("name", ["ties", "lidar"])
def test_emulated_knn_beyond_the_register_lists(name):
    """k = 57 ... 200 at size: the kernel with the k-list in LDS and in the output row, on a lattice of equal
    distances and a LiDAR-like cloud, clean and poisoned rows."""
    c = _case(name, 6_000, 192)
    emu = EmulatedTree(c.pts, LEAF)
    for k in (57, 63, 64, 65, 100, 200):
        for lds in (False, True):
            c.check(emu.search_knn(c.q, k, list_in_lds=lds), k, what=("list in LDS", lds))
    clean = c.ref.search_knn(c.clean, 200)
    assert emu.search_knn(c.clean, 200, list_in_lds=False).tobytes() == clean.tobytes()


@needs_reference
@pytest.mark.parametrize("metric", ["L1", "LPInf", "LNInf", "SO2", "SE2Squared"])
def test_emulated_other_metrics_with_poisoned_rows(metric):
    if metric == "SO2":
        pts, q = ds.uniform_cloud(3_000, 1, 81), ds.uniform_cloud(600, 1, 82)
    else:
        pts, q = ds.uniform_cloud(4_000, 3, 83), ds.uniform_cloud(600, 3, 84)
    c = _Case(metric, 0, 0, metric, pts=pts, q=q)
    emu = EmulatedTree(c.pts, LEAF, pt.Metric[metric])
    for k in (1, 5):
        for small in (False, True):
            c.check(emu.search_knn(c.q, k, small_stack=small), k, what=small)
    radius = np.float32(0.05 if metric != "LNInf" else 0.0005)
    _same_radius(emu.search_radius(c.q, radius), c.ref.search_radius(c.q, radius), metric)


# ---- emulator: radius -----------------------------------------------------------------------------------------------

@needs_reference
@pytest.mark.parametrize("name", ["lidar", "ties", "dim5"])
def test_emulated_radius_with_poisoned_rows(name):
    """The two passes, the capture (ample pool, none, one that runs dry), the leaf lists, the lists capped at 4 far
    children with the cooperative finish, sorted rows -- at a median nearest distance, 25 x it, FLT_MAX and +inf."""
    c = _case(name, 2_000, 384)
    emu = EmulatedTree(c.pts, LEAF)
    nd = c.pts.shape[1] > 3
    perm = None if nd else emu.morton_permutation(c.q)[0]
    small, huge = c.radii()[:2], c.radii()[2:]
    for r in small + huge:
        # (every row holds every point at the two huge radii: a part of the batch with its poisoned wavefront)
        q = c.q if r in small else np.ascontiguousarray(c.q[np.flatnonzero(c.mask)[:96].tolist() + list(range(1, 65))])
        want = c.ref.search_radius(q, r)
        pm = None if (nd or len(q) != len(c.q)) else perm
        _same_radius(emu.search_radius(q, r, perm=pm), want, (name, r, "two passes"))
        for sub_cap in (1024, 0, 1):
            _same_radius(emu.search_radius_captured(q, r, perm=pm, sub_cap=sub_cap), want, (name, r, "capture", sub_cap))
        if not nd:
            _same_radius(emu.search_radius_lists(q, r, perm=pm, sub_cap=1024), want, (name, r, "lists"))
            _same_radius(emu.search_radius_lists(q, r, sub_cap=0), want, (name, r, "lists, static chunk"))
            _same_radius(emu.search_radius_lists_capped(q, r, 4, perm=pm), want, (name, r, "capped lists"))
        if r in small:
            _same_radius(emu.search_radius(q, r, sort=True), c.ref.search_radius(q, r, sort=True), (name, r, "sorted"),
                         sort=True)
    assert c.ref.search_radius(c.q, small[1])[0][-1] > len(c.q)


@needs_reference
def test_emulated_double_radius_with_poisoned_rows():
    c = _case("lidar", 2_000, 384, dtype=np.float64)
    emu = EmulatedTree64(c.pts, LEAF)
    for i, r in enumerate(c.radii()):
        q = c.q if i < 2 else np.ascontiguousarray(c.q[np.flatnonzero(c.mask)[:96].tolist() + list(range(1, 100))])
        want = c.ref.search_radius(q, r)
        _same_radius(emu.search_radius(q, r), want, (r, "plain"))
        off, rows, heavy, _ = emu.search_radius_capped(q, r, 4)
        _same_radius((off, rows), want, (r, "capped"))
        if i == 1:
            assert heavy > 0
            _same_radius(emu.search_radius(q, r, sort=True), c.ref.search_radius(q, r, sort=True), (r, "sorted"), sort=True)


# ---- emulator: box --------------------------------------------------------------------------------------------------

def _boxes(c, seed=3):
    """Boxes around the clean queries; corners poisoned per side; inverted boxes; the all-space box; boxes with a NaN
    in EVERY coordinate of one corner.  Returns (mins, maxs, rows with a NaN corner coordinate)."""
    rng = np.random.default_rng(seed)
    span = (c.pts.max(0) - c.pts.min(0)).astype(c.dtype)
    h = (rng.uniform(0.02, 0.3, size=c.clean.shape) * span).astype(c.dtype)
    lo, hi = (c.clean - h).astype(c.dtype), (c.clean + h).astype(c.dtype)
    lo, hi, mask = P.poison_corners(lo, hi, seed + 1, share=0.3)
    clean = np.flatnonzero(~mask)
    inv = clean[:20]
    lo[inv], hi[inv] = hi[inv].copy(), lo[inv].copy()         # inverted boxes
    lo[clean[20]], hi[clean[20]] = -np.inf, np.inf            # all of space
    lo[clean[21]], hi[clean[21]] = -np.finfo(c.dtype).max, np.finfo(c.dtype).max
    lo[clean[22]] = np.nan                                    # a min corner that bounds nothing
    hi[clean[23]] = np.nan
    lo[clean[24]], hi[clean[24]] = np.nan, np.nan             # neither corner bounds anything
    nan = np.isnan(lo).any(axis=1) | np.isnan(hi).any(axis=1)
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi), nan


def _on_the_circle(lo, hi):
    """Boxes for a tree under metric_se2_squared, within the preconditions the reference asserts for a metric_box_map
    query (segment.hpp:29: `min <= max` on a plane axis; angles in [0, 1] on the circle axis, where min > max wraps):
    a plane axis that is inverted or holds a NaN becomes [-FLT_MAX, +inf]; +-Inf and +-FLT_MAX corners stay."""
    lo, hi = lo.copy(), hi.copy()
    for a in (lo, hi):
        a[:, 2] = np.clip(np.nan_to_num(a[:, 2], nan=0.25, posinf=1.0, neginf=0.0), 0.0, 1.0)
    bad = ~(lo[:, :2] <= hi[:, :2])
    lo[:, :2][bad], hi[:, :2][bad] = -FLT_MAX, np.inf
    return lo, hi


@needs_reference
@pytest.mark.parametrize("name,dtype", [("lidar", np.float32), ("ties", np.float32), ("dim2", np.float32),
                                        ("dim5", np.float32), ("lidar", np.float64), ("dim5", np.float64)])
def test_emulated_box_search_with_poisoned_corners(name, dtype):
    """box_kernel, box_nd_kernel, box64_kernel.  The reference's box test is `min > x || max < x -> outside`
    (box.hpp:31-40): a NaN corner coordinate bounds nothing on its side, it does not empty the box."""
    c = _case(name, 2_000, 384, dtype=dtype)
    lo, hi, nan = _boxes(c)
    emu = EmulatedTree(c.pts, LEAF) if dtype == np.float32 else EmulatedTree64(c.pts, LEAF)
    woff, wflat = c.ref.search_box(lo, hi)
    goff, gflat = emu.search_box(lo, hi)
    counts = np.diff(woff.astype(np.int64))
    assert nan.sum() >= 20 and counts[nan].sum() > 0, "no NaN-cornered box holds a point: the case shows nothing"
    bad = np.flatnonzero(np.diff(goff.astype(np.int64)) != counts)
    assert len(bad) == 0, (name, f"{len(bad)} boxes differ in size, {int(nan[bad].sum())} of them with a NaN corner; "
                                 f"first: box {bad[0]} [{lo[bad[0]]}, {hi[bad[0]]}]: {np.diff(goff.astype(np.int64))[bad[0]]} "
                                 f"points, reference {counts[bad[0]]}")
    assert np.array_equal(gflat, wflat)


# ---- the host loop --------------------------------------------------------------------------------------------------

def _prefilled(shape, dtype):
    out = np.empty(shape, dtype=dtype)
    out.view(np.uint8).reshape(-1)[:] = 0xA5
    return out


@needs_reference
@pytest.mark.parametrize("metric", ["L2Squared", "L1", "SE2Squared"])
def test_host_loop_with_poisoned_rows(metric):
    """ptk_host_search_* on a host-only handle, into prefilled buffers: no slot of a k-NN row is left as it was."""
    lib = pt._load()
    c = _Case("uniform", 0, 0, metric, pts=ds.uniform_cloud(4_000, 3, 85), q=ds.uniform_cloud(1_200, 3, 86))
    tree = pt.KdTree(c.pts, pt.Metric[metric], LEAF, device=pt.PTK_DEVICE_NONE)
    nq = len(c.q)
    for k, e in ((1, None), (5, None), (16, None), (80, None), (5, 1.3)):
        out = _prefilled((nq, k), pt.NEIGHBOR)
        assert lib.ptk_host_search_knn(tree._h, c.pts.ctypes.data, c.q.ctypes.data, nq, k, e or 1.0, out.ctypes.data) == 0
        c.check(out, k, e, what="host loop")
    # k > n_points: the slots between the last neighbour and the sentinel hold the filler too
    few = pt.KdTree(c.pts[:7].copy(), pt.Metric[metric], 3, device=pt.PTK_DEVICE_NONE)
    out = _prefilled((nq, 12), pt.NEIGHBOR)
    assert lib.ptk_host_search_knn(few._h, few._pts.ctypes.data, c.q.ctypes.data, nq, 12, 1.0, out.ctypes.data) == 0
    short = oracle.Oracle(few._pts, 3, "reference", metric)
    rows, written = P.written_by_reference(short, c.q, 7, c.mask)
    assert out[:, :7].tobytes() == P.expect_rows(rows, written).tobytes()
    assert (out["index"][:, 7:] == 0).all() and (out["distance"][:, 7:] == FLT_MAX).all()

    med, wide = c.radii()[:2]
    for k in (1, 16):  # search_knn_within: the entries the reference wrote, below the radius; {-1, radius} behind them
        rows, written = P.written_by_reference(c.ref, c.q, k, c.mask)
        for r in (med, wide, INF):
            keep = written.all(axis=2) & (rows["distance"] < r)
            assert (np.diff(keep.astype(np.int8), axis=1) <= 0).all()  # a prefix of each row
            want = np.empty((nq, k), dtype=pt.NEIGHBOR)
            want["index"], want["distance"] = np.where(keep, rows["index"], -1), np.where(keep, rows["distance"], r)
            out = _prefilled((nq, k), pt.NEIGHBOR)
            assert lib.ptk_host_search_knn_within(tree._h, c.pts.ctypes.data, c.q.ctypes.data, nq, k, r, out.ctypes.data) == 0
            assert P.same_rows(out, want), (metric, k, r, P.first_difference(out, want, c.mask))
    for r in (med, wide, np.float32(FLT_MAX), INF):
        woff, wflat = c.ref.search_radius(c.q, r)
        counts = _prefilled((nq,), np.uint64)
        assert lib.ptk_host_search_count_within(tree._h, c.pts.ctypes.data, c.q.ctypes.data, nq, r, 0, counts.ctypes.data) == 0
        assert np.array_equal(counts, np.diff(woff)), (metric, r)
        if r == INF:
            continue
        off, rows = _prefilled((nq + 1,), np.uint64), ctypes.c_void_p()
        assert lib.ptk_host_search_radius(tree._h, c.pts.ctypes.data, c.q.ctypes.data, nq, r, 1.0, 0, off.ctypes.data,
                                          ctypes.byref(rows)) == 0
        got = pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR)
        _same_radius((off, got), (woff, wflat), (metric, r, "host loop"))
    lo, hi, nan = _boxes(c)
    if metric == "SE2Squared":
        lo, hi = _on_the_circle(lo, hi)
    off, rows = _prefilled((nq + 1,), np.uint64), ctypes.c_void_p()
    assert lib.ptk_host_search_box(tree._h, c.pts.ctypes.data, lo.ctypes.data, hi.ctypes.data, nq, off.ctypes.data,
                                   ctypes.byref(rows)) == 0
    got = pt._adopt(lib, rows, int(off[-1]), np.int32)
    woff, wflat = c.ref.search_box(lo, hi)
    assert np.array_equal(off, woff) and np.array_equal(got, wflat), metric


# ---- creation -------------------------------------------------------------------------------------------------------

def _create_cases():
    for dtype in (np.float32, np.float64):
        for value in (np.nan, np.inf, -np.inf):
            for where in ("first", "middle", "last"):
                yield dtype, value, where


def _check_creation_refuses_non_finite_points(device, n):
    for dtype, value, where in _create_cases():
        pts = ds.uniform_cloud(n, 3, 91).astype(dtype)
        row = {"first": 0, "middle": n // 2 + 1, "last": n - 1}[where]
        pts[row, (row + 1) % 3] = value
        with pytest.raises(pt.PtkError) as err:
            pt.KdTree(pts, pt.Metric.L2Squared, LEAF, device=device)
        assert err.value.status == PTK_ERR_INVALID and f"point {row} " in str(err.value), (dtype, value, where, str(err.value))
    # two offenders: the message names the first
    pts = ds.uniform_cloud(n, 3, 91)
    pts[n - 2, 0], pts[17, 2] = np.nan, np.inf
    with pytest.raises(pt.PtkError, match="point 17 "):
        pt.KdTree(pts, pt.Metric.L2Squared, LEAF, device=device)
    # the C entry leaves no handle behind
    handle = ctypes.c_void_p(0xDEAD)
    lib = pt._load()
    assert lib.ptk_tree_create_from_points(pts.ctypes.data, n, 3, LEAF, device, ctypes.byref(handle)) == PTK_ERR_INVALID
    assert not handle.value


def test_creation_refuses_non_finite_points():
    """ptk_tree_create_from_points / ptk_tree64_create_from_points: PTK_ERR_INVALID naming the first offending point
    (the builder partitions with `<` through std::nth_element, which a NaN makes undefined)."""
    _check_creation_refuses_non_finite_points(pt.PTK_DEVICE_NONE, 3_000)
    _check_creation_refuses_non_finite_points(pt.PTK_DEVICE_NONE, 300_000)  # (checked on several threads)


@needs_reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_points_at_the_largest_finite_scalar_are_accepted(dtype):
    """+-FLT_MAX / +-DBL_MAX are finite: such a tree is built and searched as the reference's (box extents and
    distances overflow to +inf on both sides)."""
    mx = np.finfo(dtype).max
    pts = ds.uniform_cloud(2_000, 3, 92).astype(dtype)
    pts[5, 0], pts[900, 1], pts[1_999, 2], pts[1_000, 0] = mx, -mx, mx, -mx
    q = ds.uniform_cloud(500, 3, 93).astype(dtype)
    ref = oracle.Oracle(pts, LEAF, "reference", dtype=dtype)
    if dtype == np.float32:
        host = pt.KdTree(pts, pt.Metric.L2Squared, LEAF, device=pt.PTK_DEVICE_NONE)
        assert host._serialize() == ref.save_bytes()
        emu = EmulatedTree(pts, LEAF)
    else:
        emu = EmulatedTree64(pts, LEAF)
        assert oracle.canonical_stream64(emu.save_bytes()) == oracle.canonical_stream64(ref.save_bytes())
    for k in (1, 8):
        got, want = emu.search_knn(q, k), ref.search_knn(q, k)
        assert np.array_equal(got["index"], want["index"]), k
        assert np.ascontiguousarray(got["distance"]).tobytes() == np.ascontiguousarray(want["distance"]).tobytes(), k
    _same_radius(emu.search_radius(q, dtype(0.01)), ref.search_radius(q, dtype(0.01)), "radius")


# =====================================================================================================================
# GPU tier: the Python wrapper -> C ABI -> device, against the compiled reference.  Every k-NN output buffer is
# prefilled with 0xA5 bytes (host form: `nns`; device form: the caller's tensor), so an unwritten slot cannot pass.
# =====================================================================================================================

GPU_POINTS = {"lidar": 50_000, "ties": 60_000}
GPU_QUERIES = 100_000
GPU_LARGE_K_QUERIES = 20_000   # (k >= 57: 200 slots of 16 bytes per row in double)
GPU_RADIUS_QUERIES = 30_000    # (a few hundred hits per row at 25 x the median nearest distance on the lattice)


def _gpu_cloud(name, nq):
    if name == "lidar":
        return ds.lidar_cloud(GPU_POINTS[name], seed=171), ds.lidar_cloud(nq, seed=172, pose=(3.0, 1.5))
    # a lattice of 25^3 positions under 60 000 points: equal distances everywhere and piles of coincident points
    return _lattice(GPU_POINTS[name], 173, 24), _lattice(nq, 174, 48)


class _GpuCase(_Case):
    def __init__(self, name, nq, dtype, device, metric="L2Squared", pts=None, q=None):
        p, c = _gpu_cloud(name, nq) if pts is None else (pts, q)
        super().__init__(name, 0, 0, metric, dtype, pts=p, q=c)
        self.device = device
        self.tree = pt.KdTree(self.pts, pt.Metric[metric], LEAF, device=device)
        self._dq = self._dclean = None

    def dq(self, clean=False):
        import torch
        if self._dq is None:
            self._dq = torch.from_numpy(self.q).to(f"cuda:{self.device}")
            self._dclean = torch.from_numpy(self.clean).to(f"cuda:{self.device}")
        return self._dclean if clean else self._dq

    def host_rows(self, k, e=None, clean=False, tree=None):
        nns = _prefilled((len(self.q),) if k == 1 else (len(self.q), k), self.ref.neighbor)
        args = (e, nns) if e is not None else (nns,)
        got = (tree or self.tree).search_knn(self.clean if clean else self.q, k, *args)
        assert got is nns
        return got

    def device_rows(self, k, e=None, clean=False, tree=None):
        import torch
        f64 = self.dtype == np.float64
        out = torch.full((len(self.q), k, 2), -6510615555426900571 if f64 else -1515870811,
                         dtype=torch.int64 if f64 else torch.int32, device=f"cuda:{self.device}")
        args = (e, out) if e is not None else (out,)
        got = (tree or self.tree).search_knn(self.dq(clean), k, *args).numpy()
        torch.cuda.synchronize()
        return got

    def check_isolated(self, got, clean_rows, what):
        """The poisoned batch and its clean twin: byte-equal rows wherever no row was poisoned, whatever the reference
        says."""
        a = P.record_bytes(got).reshape(len(self.q), -1)[~self.mask]
        b = P.record_bytes(clean_rows).reshape(len(self.q), -1)[~self.mask]
        assert np.array_equal(a, b), (self.name, what, "a poisoned row changed the row of a neighbour")


@pytest.fixture(scope="module")
def gcases(gpu):
    cache = {}

    def get(name, dtype, nq=GPU_QUERIES, metric="L2Squared"):
        key = (name, np.dtype(dtype).name, nq, metric)
        if key not in cache:
            cache[key] = _GpuCase(name, nq, dtype, gpu, metric)
        return cache[key]

    yield get
    cache.clear()


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["lidar", "ties"])
def test_gpu_knn_with_poisoned_rows(gcases, name, dtype):
    """search_knn through the host form and the device form: the two-phase k = 1 search, the register lists with the
    batch's own cap (k <= 56), exact and approximate; the isolation property against the clean twin."""
    c = gcases(name, dtype)
    for k in (1, 4, 16, 32, 40):
        c.check(c.host_rows(k), k, what="host form")
        got = c.device_rows(k)
        c.check(got, k, what="device form")
        if k in (1, 16):
            c.check_isolated(got, c.device_rows(k, clean=True), k)
    for k in (1, 8):
        c.check(c.device_rows(k, e=1.3), k, e=1.3, what="approximate")


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["lidar", "ties"])
def test_gpu_knn_beyond_the_register_lists(gcases, name, dtype):
    """k = 57 ... 64 (the register list of 64 slots, never capped) and k = 65 ... 200 (the k-list in the output row / in
    LDS) at size, on clean and poisoned rows of a lattice of equal distances and a LiDAR-like cloud."""
    c = gcases(name, dtype, GPU_LARGE_K_QUERIES)
    for k in (57, 64, 65, 80, 100, 200):
        got = c.device_rows(k)
        c.check(got, k, what="device form")
        if k in (64, 80):
            c.check(c.host_rows(k), k, what="host form")
            c.check_isolated(got, c.device_rows(k, clean=True), k)
    rows, written = P.written_by_reference(c.ref, c.clean, 200)
    assert written.all() and P.same_rows(c.device_rows(200, clean=True), P.expect_rows(rows, written))


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["lidar", "ties"])
def test_gpu_capped_knn_with_poisoned_rows(gcases, name, dtype):
    """The cap on and low (test hooks), so that nearly every query is handed to the cooperative search: its shared
    bound (`ds_min` on the bits of a float), the merge, the redo list.  The counters say the path ran, and that a
    poisoned row costs at most a redo."""
    c = gcases(name, dtype)
    f64 = c.dtype == np.float64
    knobs = {"knn64_cap": 4, "knn_cap_min_nq": 1} if f64 else {"knn_cap": 4, "knn_cap_min_nq": 1}
    pt.set_test_knobs(**knobs)
    try:
        for k in ((4, 16, 32) if f64 else (4, 16, 32, 40)):
            got = c.device_rows(k)
            counts = c.tree.knn_coop_counts()
            c.check(got, k, what=("capped", counts))
            c.device_rows(k, clean=True)
            clean = c.tree.knn_coop_counts()
            assert counts["cooperative"] > 0, (name, k, counts)
            assert counts["redone"] <= int(c.mask.sum()) + clean["redone"], (name, k, counts, clean, int(c.mask.sum()))
    finally:
        pt.set_test_knobs()


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("direct", [0, 2])
@pytest.mark.parametrize("name", ["lidar", "ties"])
def test_gpu_capped_two_phase_knn1_with_poisoned_rows(gpu, gcases, name, direct):
    """k = 1 with a cap of 1 or 2 far children in phase 2 (nearly every continuation goes to the cooperative search),
    through phase 2 first and straight from phase 1; the lattice on the full tree (pile_view=0) as well."""
    base = gcases(name, np.float32)
    pt.set_test_knobs(coop_direct=direct)
    if name == "ties":
        pt.set_test_knobs(pile_view=0)
    tree = pt.KdTree(base.pts, pt.Metric.L2Squared, LEAF, device=gpu)  # (the view is chosen when the tree is made)
    try:
        for cap in (1, 2):
            pt.set_test_knobs(p2_cap=cap)
            got = base.device_rows(1, tree=tree)
            counts = tree.knn1_counts()
            base.check(got, 1, what=("p2_cap", cap, counts))
            clean_rows = base.device_rows(1, clean=True, tree=tree)
            clean = tree.knn1_counts()
            base.check_isolated(got, clean_rows, ("p2_cap", cap))
            assert counts["cooperative"] > 0, (name, cap, counts)
            assert counts["redone"] <= int(base.mask.sum()) + clean["redone"], (name, cap, counts, clean)
    finally:
        pt.set_test_knobs()
        tree.close()


@pytest.mark.gpu
@needs_reference
def test_gpu_knn_reorder_metrics_and_dimensions_with_poisoned_rows(gpu, gcases):
    """Batch order ON / OFF / AUTO (the Morton keys are cut from float -> uint conversions of the rows), metric_l1 /
    metric_lpinf / metric_lninf at k = 1 and 16, a 2-D and a 5-D tree."""
    c = gcases("lidar", np.float32)
    for mode in (pt.REORDER_ON, pt.REORDER_OFF, pt.REORDER_AUTO):
        c.tree.set_reorder(mode)
        for k in (1, 16):
            c.check(c.device_rows(k), k, what=("reorder", mode))
    for metric in ("L1", "LPInf", "LNInf"):
        m = gcases("lidar", np.float32, 30_000, metric)
        for k in (1, 16):
            m.check(m.device_rows(k), k, what="device form")
            m.check(m.host_rows(k), k, what="host form")
    for dim in (2, 5):
        d = _GpuCase(f"dim{dim}", 0, np.float32, gpu, pts=ds.uniform_cloud(40_000, dim, 175),
                     q=ds.uniform_cloud(30_000, dim, 176))
        for k in (1, 16, 80):
            d.check(d.device_rows(k), k, what="device form")
        r = np.float32(4) * d.radii()[0]  # (25 x would hold a third of a 5-D cloud in every row)
        _same_radius(_radius_rows(d.tree.search_radius(d.q, r)), d.ref.search_radius(d.q, r), (dim, "radius"))


def _radius_rows(darray):
    return darray.offsets, darray.flat


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["lidar", "ties"])
def test_gpu_knn_within_with_poisoned_rows(gcases, name, dtype):
    """search_knn_within keeps its own padding {-1, radius}: the entries the reference wrote, below the radius."""
    c = gcases(name, dtype, GPU_LARGE_K_QUERIES)
    med = c.radii()[0]
    for k in (1, 16, 80):
        rows, written = P.written_by_reference(c.ref, c.q, k, c.mask)
        for r in (med, c.dtype.type(np.inf)):
            keep = written.all(axis=2) & (rows["distance"] < r)
            want = np.zeros((len(c.q), k), dtype=c.ref.neighbor)
            want["index"], want["distance"] = np.where(keep, rows["index"], -1), np.where(keep, rows["distance"], r)
            nns = _prefilled((len(c.q),) if k == 1 else (len(c.q), k), c.ref.neighbor)
            got = c.tree.search_knn_within(c.q, k, r, nns)
            assert P.same_rows(got, want), (name, k, r, "host form", P.first_difference(got, want, c.mask))
            got = c.tree.search_knn_within(c.dq(), k, r).numpy()
            assert P.same_rows(got, want), (name, k, r, "device form", P.first_difference(got, want, c.mask))


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("env", [{}, {"radius_cap": 4}, {"radius_capture_chunks": 0}, {"radius_capture_chunks": 1},
                                 {"PTK_RADIUS_CAPTURE_MB": "0"}, {"PTK_RADIUS_CAPTURE_MB": "2"}],
                         ids=["default", "cap-4", "static-chunk-only", "pool-runs-dry", "capture-off", "budget-too-small"])
@pytest.mark.parametrize("name", ["lidar", "ties"])
def test_gpu_radius_with_poisoned_rows(gcases, monkeypatch, name, env):
    """search_radius, host form and the device count / fill pair, at a median nearest distance, 25 x it, FLT_MAX and
    +inf; the list pass capped at 4 far children; every capture regime; sorted rows."""
    import torch
    for key, value in env.items():
        if key.startswith("PTK_"):
            monkeypatch.setenv(key, value)
        else:
            pt.set_test_knobs(**{key: value})
    c = gcases(name, np.float32, GPU_RADIUS_QUERIES)
    small, huge = c.radii()[:2], c.radii()[2:]
    try:
        for r in small + huge:
            # (every row holds every point at the two huge radii: three poisoned wavefronts and one clean one)
            rows = slice(None) if r in small else np.r_[np.flatnonzero(c.mask)[:192], np.flatnonzero(~c.mask)[:64]]
            q = np.ascontiguousarray(c.q[rows])
            want = c.ref.search_radius(q, r)
            _same_radius(_radius_rows(c.tree.search_radius(q, r)), want, (name, r, env, "host form"))
            off, raw = c.tree.search_radius_device(torch.from_numpy(q).to(f"cuda:{c.device}"), r)
            torch.cuda.synchronize()
            _same_radius((off.cpu().numpy(), raw.cpu().numpy().view(pt.NEIGHBOR)[:, 0]), want, (name, r, env, "device pair"))
            if env.get("radius_cap") and r == small[1]:
                counts = c.tree.radius_coop_counts()
                assert counts["cooperative"] > 0, (name, counts)
                c.tree.search_radius_device(c.dq(clean=True), r)
                clean = c.tree.radius_coop_counts()
                assert counts["recounted"] <= int(c.mask.sum()) + clean["recounted"], (name, counts, clean)
        _same_radius(_radius_rows(c.tree.search_radius(c.q, small[1], sort=True)),
                     c.ref.search_radius(c.q, small[1], sort=True), (name, env, "sorted"), sort=True)
    finally:
        pt.set_test_knobs()


@pytest.mark.gpu
@needs_reference
def test_gpu_double_radius_with_poisoned_rows(gcases):
    c = gcases("lidar", np.float64, GPU_RADIUS_QUERIES)
    for knobs in ({}, {"radius64_cap": 4}):
        pt.set_test_knobs(**knobs) if knobs else None
        try:
            for i, r in enumerate(c.radii()):
                rows = slice(None) if i < 2 else np.r_[np.flatnonzero(c.mask)[:192], np.flatnonzero(~c.mask)[:64]]
                q = np.ascontiguousarray(c.q[rows])
                _same_radius(_radius_rows(c.tree.search_radius(q, r)), c.ref.search_radius(q, r), (r, knobs))
                if knobs and i == 1:
                    assert c.tree.knn_coop_counts()["cooperative"] > 0
        finally:
            pt.set_test_knobs()


@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["3d", "5d", "double", "SE2Squared"])
def test_gpu_box_search_with_poisoned_corners(gpu, gcases, kind):
    """search_box through host buffers and device buffers: NaN / +-Inf / +-MAX corners, inverted boxes, all of space."""
    import torch
    if kind == "3d":
        c = gcases("lidar", np.float32)
    elif kind == "double":
        c = gcases("lidar", np.float64)
    elif kind == "5d":
        c = _GpuCase("dim5", 0, np.float32, gpu, pts=ds.uniform_cloud(40_000, 5, 177), q=ds.uniform_cloud(20_000, 5, 178))
    else:
        c = _GpuCase("se2", 0, np.float32, gpu, "SE2Squared", pts=ds.uniform_cloud(40_000, 3, 179),
                     q=ds.uniform_cloud(20_000, 3, 180))
    n = 20_000
    sub = _Case.__new__(_Case)
    sub.pts, sub.clean, sub.dtype = c.pts, c.clean[:n], c.dtype
    lo, hi, nan = _boxes(sub)
    if kind == "SE2Squared":
        lo, hi = _on_the_circle(lo, hi)
        nan = np.isnan(lo).any(axis=1) | np.isnan(hi).any(axis=1)
    woff, wflat = c.ref.search_box(lo, hi)
    assert kind == "SE2Squared" or np.diff(woff.astype(np.int64))[nan].sum() > 0
    boxes = np.empty((2 * n, c.pts.shape[1]), dtype=c.dtype)
    boxes[0::2], boxes[1::2] = lo, hi
    got = c.tree.search_box(boxes)
    assert np.array_equal(got.offsets, woff) and np.array_equal(got.flat, wflat), (kind, "host buffers")
    if c.dtype == np.float32:
        dev = f"cuda:{gpu}"
        off, flat = c.tree.search_box_device(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))
        torch.cuda.synchronize()
        assert np.array_equal(off.cpu().numpy().astype(np.uint64), woff) and np.array_equal(flat.cpu().numpy(), wflat), \
            (kind, "device buffers")


@pytest.mark.gpu
def test_gpu_creation_refuses_non_finite_points(gpu):
    _check_creation_refuses_non_finite_points(gpu, 3_000)
    _check_creation_refuses_non_finite_points(gpu, 300_000)  # (the size the top levels are partitioned on the device at)
