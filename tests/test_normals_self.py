"""normals_within_self: PCA normals and curvature of a tree's own points (ptk.h).

Expected MOMENTS are the contract in numpy float32 (``expected_moments``: vectorised over rows, sequential over the rank
inside a row) applied to rows obtained independently of the feature: the compiled reference's rows with the own entry
removed (``Case.want`` / ``Case.want_per_row`` of tests/test_radius_self.py), or, where the reference cannot build the
tree, the library's host loop ``ptk_host_search_radius`` / ``_radii``.  They are compared byte for byte, pad words
included.

FRAMES are checked three ways: (a) byte equality of the host loop, the emulated kernel, the device and the C++ member;
(b) properties against ``expected_covariance`` in float64 -- the eigen-residuals against a bound that is 32 x the
largest residual numpy's float32 ``eigh`` leaves on the same matrices, relative to the Frobenius norm, computed at run
time; unit length; ascending non-negative eigenvalues; the curvature recomputed bit for bit -- and (c) the sign rule.

The CPU tier runs the host loop on a host-only handle, the real kernel source in the emulator
(tests/cpp/emulate_frames.cpp), the C++ member (tests/cpp/normals_self_main.cpp, -DPICO_TREE_HOST_ONLY) and the Python
wrapper's refusals; the gpu tier the device forms.
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
from tests import depth_cases, leaf_cases, poison
from tests.test_radius_self import Case, case, cloud, guarded, guards_intact, row_ids, without_self  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")
METRICS = ["L2Squared", "L1", "LPInf", "LNInf"]
_EMU_METRIC = {"L2Squared": 0, "L1": 1, "LPInf": 2, "LNInf": 3}
_CPP_METRIC = {"L2Squared": "l2", "L1": "l1", "LPInf": "lpinf", "LNInf": "lninf"}
NAN_BITS = 0x7FC00000
F32 = np.float32
VIEW = np.array([0.3, -2.0, 5.0], dtype=np.float32)

needs_reference = pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference not present")


# ---- the contract in numpy ------------------------------------------------------------------------------------------------

def expected_moments(p, off, flat):
    """ptk_moments of every row: accumulators from +0, the offsets u = p_i - p_j (float32, query first) in row order."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    cnt = np.diff(off)
    m = np.zeros(n, dtype=pt.MOMENTS)
    s = np.zeros((n, 3), dtype=np.float32)
    o = np.zeros((n, 6), dtype=np.float32)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    idx = np.asarray(flat["index"]).astype(np.int64)
    with np.errstate(all="ignore"):
        for t in range(int(cnt.max(initial=0))):
            rows = np.flatnonzero(cnt > t)
            u = p[rows] - p[idx[off[rows] + t]]
            assert u.dtype == np.float32
            s[rows] = s[rows] + u
            for k, (a, b) in enumerate(pairs):
                o[rows, k] = o[rows, k] + u[:, a] * u[:, b]
    m["sum"], m["outer"], m["count"] = s, o, cnt
    return m


def expected_covariance(m):
    """C (n, 6: xx, xy, xz, yy, yz, zz) of moments: the three lines of the contract in float32."""
    with np.errstate(all="ignore"):
        inv = F32(1) / (m["count"].astype(np.float32) + F32(1))  # (count + 1 is exact in float32 below 2^24)
        assert inv.dtype == np.float32
        mean = m["sum"] * inv[:, None]
        c = np.empty((len(m), 6), dtype=np.float32)
        for k, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
            c[:, k] = m["outer"][:, k] * inv - mean[:, a] * mean[:, b]
    return c


def full(c):
    """(n, 3, 3) symmetric matrices of (n, 6)."""
    out = np.empty((len(c), 3, 3), dtype=c.dtype)
    for k, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        out[:, a, b] = out[:, b, a] = c[:, k]
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_frames(frames, moments, p, view, min_neighbors, what):
    """Checks (b) and (c) and the NaN rule of `frames` against `moments` (already known to be the contract's); returns
    (largest relative residual of the frames, the same of numpy's float32 eigh) on the rows that have a frame."""
    c = expected_covariance(moments)
    cnt = moments["count"]
    assert np.array_equal(frames["count"], cnt), what
    nan = (cnt < max(min_neighbors, 2)) | ~np.isfinite(c).all(1)
    fb = np.concatenate([bits(frames["normal"]), bits(frames["curvature"])[:, None], bits(frames["eigenvalues"])], axis=1)
    assert np.all(fb[nan] == NAN_BITS), what
    ok = ~nan
    assert np.isfinite(frames["normal"][ok]).all() and np.isfinite(frames["eigenvalues"][ok]).all(), what
    if not ok.any():
        return 0.0, 0.0
    f, c32 = frames[ok], full(c[ok])
    c64 = c32.astype(np.float64)
    norm = np.sqrt((c64 ** 2).sum((1, 2)))
    # the yardstick: numpy's float32 eigh on the same matrices, its residuals in float64
    w, v = np.linalg.eigh(c32)
    assert w.dtype == np.float32
    res_np = np.linalg.norm(np.einsum("nij,njk->nik", c64, v.astype(np.float64)) - v.astype(np.float64) * w.astype(np.float64)[:, None, :], axis=1)
    some = norm > 0
    worst_np = float((res_np[some] / norm[some][:, None]).max(initial=0.0))
    bound = 32.0 * worst_np
    n64, l64 = f["normal"].astype(np.float64), f["eigenvalues"].astype(np.float64)
    res = np.linalg.norm(np.einsum("nij,nj->ni", c64, n64) - l64[:, :1] * n64, axis=1)
    rel = np.where(some, res / np.where(some, norm, 1.0), 0.0)
    worst = float(rel.max(initial=0.0))
    print(f"{what}: residual {worst:.3e} (eigh float32 {worst_np:.3e}, bound {bound:.3e}) on {int(ok.sum())} rows")
    assert np.all(res[~some] == 0), what  # (a zero matrix: zero eigenvalues, any unit vector)
    assert worst <= bound, (what, worst, bound)
    # the other two pairs through the trace and the Frobenius norm: each eigenvalue within bound * |C|_F of a true one
    # gives |sum l - tr C| <= 3 bound |C|_F and | |l|_2 - |C|_F | <= sqrt(3) bound |C|_F
    tr = c64[:, 0, 0] + c64[:, 1, 1] + c64[:, 2, 2]
    assert np.all(np.abs(l64.sum(1) - tr) <= 3 * bound * norm), what
    assert np.all(np.abs(np.sqrt((l64 ** 2).sum(1)) - norm) <= np.sqrt(3.0) * bound * norm), what
    assert np.all(np.abs((n64 ** 2).sum(1) - 1.0) <= 8 * 2.0 ** -24), what
    lam = f["eigenvalues"]
    assert np.all(lam[:, 0] <= lam[:, 1]) and np.all(lam[:, 1] <= lam[:, 2]) and np.all(lam >= 0), what
    assert not np.any(np.signbit(lam)), what  # (clamped below at +0)
    with np.errstate(all="ignore"):
        total = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
        curv = np.where(total == 0, F32(0), lam[:, 0] / np.where(total == 0, F32(1), total)).astype(np.float32)
    assert np.array_equal(bits(curv), bits(f["curvature"])), what
    # (c) the sign rule
    nrm = f["normal"]
    if view is not None:
        w3 = np.asarray(view, dtype=np.float32)[None, :] - np.asarray(p, dtype=np.float32)[ok]
        dot = (nrm[:, 0] * w3[:, 0] + nrm[:, 1] * w3[:, 1]) + nrm[:, 2] * w3[:, 2]
        assert dot.dtype == np.float32 and np.all(dot >= 0), what
    else:
        a = np.abs(nrm)
        lead = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), nrm[:, 0], np.where(a[:, 1] >= a[:, 2], nrm[:, 1], nrm[:, 2]))
        assert np.all(lead >= 0), what
    return worst, worst_np


def all_written(records):
    raw = records.view(np.uint8).reshape(len(records), -1)
    return not np.any((raw == 0xA5).all(1))


def _call(fn, lead, r, mn, view, n, want):
    """fn(*lead, radius, radii, min_neighbors, viewpoint, frames, moments) into guarded 0xA5 buffers; `want`: "both",
    "frames" or "moments".  Returns (frames or None, moments or None)."""
    fbuf, frames = guarded(n, pt.FRAME)
    mbuf, moments = guarded(n, pt.MOMENTS)
    scalar = np.ndim(r) == 0
    radii = None if scalar else np.ascontiguousarray(r, dtype=np.float32)
    v = None if view is None else np.ascontiguousarray(view, dtype=np.float32)
    rc = fn(*lead, F32(r if scalar else 0), None if scalar else radii.ctypes.data, mn, None if v is None else v.ctypes.data,
            frames.ctypes.data if want != "moments" else None, moments.ctypes.data if want != "frames" else None)
    assert rc == 0, pt._load().ptk_last_error()
    assert guards_intact(fbuf) and guards_intact(mbuf)
    if want != "moments":
        assert all_written(frames), "a frame was not written"
    if want != "frames":
        assert all_written(moments), "a moments record was not written"
        assert not moments["pad_"].any(), "the pad words are not zero"
    return (frames.copy() if want != "moments" else None), (moments.copy() if want != "frames" else None)


def host_normals(tree, r, mn=2, view=None, points=None, want="both"):
    p = tree._pts if points is None else points
    return _call(pt._load().ptk_host_normals_within_self, (tree._h, p.ctypes.data), r, mn, view, len(p), want)


def device_normals(tree, r, mn=2, view=None, want="both"):
    return _call(pt._load().ptk_normals_within_self, (tree._h,), r, mn, view, tree.npts, want)


def host_search_rows(tree, p, r):
    """(offsets, flat) of ptk_host_search_radius / _radii over the points themselves, the own entries removed."""
    lib = pt._load()
    p = np.ascontiguousarray(p, dtype=np.float32)
    off = np.zeros(len(p) + 1, dtype=np.uint64)
    rows = ctypes.c_void_p()
    if np.ndim(r) == 0:
        rc = lib.ptk_host_search_radius(tree._h, p.ctypes.data, p.ctypes.data, len(p), F32(r), F32(1), 0, off.ctypes.data,
                                        ctypes.byref(rows))
    else:
        r = np.ascontiguousarray(r, dtype=np.float32)
        rc = lib.ptk_host_search_radius_radii(tree._h, p.ctypes.data, p.ctypes.data, len(p), r.ctypes.data, 0,
                                              off.ctypes.data, ctypes.byref(rows))
    assert rc == 0, lib.ptk_last_error()
    return without_self(off, pt._adopt(lib, rows, int(off[-1]), pt.NEIGHBOR))


def radii_of(c):
    """The scalar radii of a case: Case.values(); on "small" a whole-tree radius as well."""
    v = [F32(x) for x in c.values()]
    return v + [F32(10.0)] if c.kind == "small" else v


@functools.lru_cache(maxsize=None)
def want_moments(kind, metric, which):
    """The contract's moments on the reference's rows: `which` an index into radii_of(), or "per row"."""
    c = case(kind, metric)
    rows = c.want_per_row() if which == "per row" else c.want(radii_of(c)[which])
    m = expected_moments(c.p, *rows)
    m.setflags(write=False)
    return m


def same(a, b):
    return a.tobytes() == b.tobytes()


# ---- CPU tier ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/cpp/emulate_frames.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_frames") / "libptk_emu_frames.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "cpp"),
        os.path.join(ROOT, "tests", "cpp", "emulate_frames.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.emu_create.restype = vp
    lib.emu_create.argtypes = [vp, u64, ctypes.c_uint32, vp, u64, vp]
    lib.emu_destroy.argtypes = [vp]
    lib.emu_set_metric.argtypes = [vp, ctypes.c_int]
    lib.emu_frames_self.argtypes = [vp, u64, ctypes.c_float, vp, u64, vp, vp, vp]
    return lib


class Emulated:
    """frames_self_kernel over a tree built by the product's host builder over `tree_points` (default: the points)."""

    def __init__(self, lib, p, leaf, metric, tree_points=None):
        self.lib, self.p = lib, np.ascontiguousarray(p, dtype=np.float32)
        self.host = pt.KdTree(self.p if tree_points is None else tree_points, getattr(pt.Metric, metric), leaf,
                              device=pt.PTK_DEVICE_NONE)
        nodes, self.idx, _, _ = self.host.flat()
        self.n = len(self.p)
        self.h = lib.emu_create(self.p.ctypes.data, self.n, 3, nodes.ctypes.data, len(nodes), self.idx.ctypes.data)
        assert self.h
        lib.emu_set_metric(self.h, _EMU_METRIC[metric])

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.emu_destroy(self.h)
            self.h = None

    def normals(self, r, mn=2, view=None, piece=0, want="both"):
        return _call(self.lib.emu_frames_self, (self.h, piece), r, mn, view, self.n, want)


@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_loop_and_emulated_kernel(emu_lib, kind, metric):
    """The host loop on a host-only handle and the real kernel source lane by lane, pieces of 1 000 and the whole tree,
    scalar and per-row radii: the contract's moments on the reference's rows, identical frames, checks (b) and (c)."""
    c = case(kind, metric)
    emu = Emulated(emu_lib, c.p, c.leaf, metric)
    todo = [(i, r) for i, r in enumerate(radii_of(c))] + [("per row", c.radii())]
    framed = 0
    for turn, (which, r) in enumerate(todo):
        want = want_moments(kind, metric, which)
        view = VIEW if turn % 2 else None
        what = (kind, metric, which)
        hf, hm = host_normals(emu.host, r, 2, view)
        assert same(hm, want), what
        ef, em = emu.normals(r, 2, view, piece=1000 if turn % 2 else 0)
        assert same(em, want) and same(ef, hf), what
        ef2, em2 = emu.normals(r, 2, view, piece=0 if turn % 2 else 1000)
        assert same(em2, want) and same(ef2, hf), what
        check_frames(hf, want, c.p, view, 2, what)
        framed += int(np.isfinite(hf["curvature"]).sum())
        if np.ndim(r) == 0 and r == 0:
            assert not want["count"].any() and not want["sum"].any() and np.all(bits(hf["curvature"]) == NAN_BITS)
    assert framed > 0
    # either output alone, and a larger min_neighbors
    which, r = todo[1]
    want = want_moments(kind, metric, which)
    hf, _ = host_normals(emu.host, r, 12, VIEW)
    assert np.any(want["count"] < 12) or kind == "ties"
    check_frames(hf, want, c.p, VIEW, 12, (kind, metric, "min_neighbors 12"))
    assert same(emu.normals(r, 12, VIEW, want="frames")[0], hf) and same(emu.normals(r, 12, VIEW, want="moments")[1], want)
    assert same(host_normals(emu.host, r, 12, VIEW, want="frames")[0], hf)
    assert same(host_normals(emu.host, r, 12, VIEW, want="moments")[1], want)


@pytest.mark.parametrize("L", leaf_cases.SMALL_LEAVES)
def test_emulated_kernel_where_the_leaf_scan_changes(emu_lib, L):
    """The CPU half of tests/test_leaf_boundaries.py for this kernel: a tree whose largest leaf has exactly 31 | 32 | 33
    and 64 | 65 points; the contract's moments on the reference's rows, the host loop's frames, checks (b) and (c)."""
    pts, blob, q, nb, ref, radii = leaf_cases.case(L)
    pts = np.asarray(pts)
    emu = Emulated(emu_lib, pts, L, "L2Squared")
    leaf_cases.assert_leaf(emu.host, L)
    for r in leaf_cases.self_radii(L, radii):
        want = expected_moments(pts, *leaf_cases.self_rows(ref, pts, r))
        hf, hm = host_normals(emu.host, r, 2, VIEW)
        assert same(hm, want), (L, r)
        for piece in (0, 1000):
            ef, em = emu.normals(r, 2, VIEW, piece=piece)
            assert same(em, want) and same(ef, hf), (L, r, piece)
        check_frames(hf, want, pts, VIEW, 2, ("leaf", L, r))
        if r == 0:  # (no neighbours: no frame anywhere)
            assert not np.isfinite(hf["curvature"]).any(), L
        if r == radii[1]:  # (r_all: every blob point's row is the rest of the blob, and it has a frame)
            assert np.isfinite(ef["curvature"][-L:]).all(), L


def test_ties_give_zero_offsets_and_zero_covariances():
    """Coincident points: rows of zero offsets give a zero covariance, whose frame is zero eigenvalues, curvature +0 and
    the x axis (no rotation runs, equal eigenvalues keep their columns)."""
    p = np.repeat(np.array([[0.5, 0.25, -1.0], [3.0, 3.0, 3.0]], dtype=np.float32), [7, 5], axis=0)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    f, m = host_normals(tree, 0.01)
    assert np.array_equal(m["count"], np.repeat([6, 4], [7, 5])) and not m["sum"].any() and not m["outer"].any()
    assert np.array_equal(f["normal"], np.tile(np.array([1, 0, 0], dtype=np.float32), (12, 1)))
    assert not bits(f["eigenvalues"]).any() and not bits(f["curvature"]).any()


def grid():
    x, y = np.meshgrid(np.arange(5, dtype=np.float32), np.arange(5, dtype=np.float32))
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), np.full(25, 2.0, dtype=np.float32)], axis=1))


def check_grid(normals):
    """`normals(r, mn, view)` -> frames of the 5 x 5 grid at z = 2: the zero row and column of C make the two z
    rotations skip, so the z eigenvector stays the unit axis."""
    up = normals(100.0, 2, np.array([0, 0, 10], dtype=np.float32))
    assert np.array_equal(up["normal"], np.tile(np.array([0, 0, 1], dtype=np.float32), (25, 1)))
    assert not bits(up["curvature"]).any() and np.all(up["count"] == 24) and not bits(up["eigenvalues"][:, 0]).any()
    down = normals(100.0, 2, np.array([0, 0, -10], dtype=np.float32))
    assert np.array_equal(down["normal"], np.tile(np.array([0, 0, -1], dtype=np.float32), (25, 1)))
    assert not bits(down["curvature"]).any()
    none = normals(100.0, 30, None)
    raw = none.view(np.uint32).reshape(25, 8)
    assert np.all(raw[:, :7] == NAN_BITS) and np.all(none["count"] == 24)


def check_tiny(normals_of):
    """`normals_of(points)` -> (frames, moments) at a radius that holds everything: n_points = 1 and 2 give NaN frames with
    counts 0 and 1; 3 points spanning a triangle have a normal perpendicular to it within (b)."""
    for n in (1, 2):
        f, m = normals_of(ds.uniform_cloud(n, 3, 21))
        assert np.all(f.view(np.uint32).reshape(n, 8)[:, :7] == NAN_BITS) and np.all(f["count"] == n - 1)
        assert np.all(m["count"] == n - 1)
    p = ds.uniform_cloud(3, 3, 21)
    f, m = normals_of(p)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    want = expected_moments(p, *host_search_rows(tree, p, 10.0))
    assert same(m, want) and np.all(f["count"] == 2)
    worst, worst_np = check_frames(f, want, p, None, 2, "triangle")
    # The points are coplanar, so the smallest true eigenvalue is 0 up to the rounding of C; a unit vector whose residual
    # is within bound * |C|_F makes an angle with the true eigenvector of at most that over the gap l1 - l0.
    c64 = full(expected_covariance(want)).astype(np.float64)
    norm = np.sqrt((c64 ** 2).sum((1, 2)))
    lam = f["eigenvalues"].astype(np.float64)
    true = np.cross(p[1].astype(np.float64) - p[0], p[2].astype(np.float64) - p[0])
    true /= np.linalg.norm(true)
    sin = np.linalg.norm(np.cross(f["normal"].astype(np.float64), true[None, :]), axis=1)
    slack = 2 * (32 * max(worst_np, 2.0 ** -24) * norm + 8 * 2.0 ** -24 * norm) / (lam[:, 1] - lam[:, 0])
    assert np.all(sin <= slack), (sin, slack)


def test_hand_written_cases_on_the_host_loop(emu_lib):
    p = grid()
    tree = pt.KdTree(p, pt.Metric.L2Squared, 4, device=pt.PTK_DEVICE_NONE)
    check_grid(lambda r, mn, view: host_normals(tree, r, mn, view)[0])
    emu = Emulated(emu_lib, p, 4, "L2Squared")
    check_grid(lambda r, mn, view: emu.normals(r, mn, view)[0])

    def tiny(q):
        return host_normals(pt.KdTree(q, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE), 10.0)

    check_tiny(tiny)


def test_emulated_per_row_radii_that_pass_no_test(emu_lib):
    """A NaN and a negative radii entry (the _device form cannot look): the empty result, every other row unchanged."""
    p, leaf = cloud("uniform")
    emu = Emulated(emu_lib, p, leaf, "L2Squared")
    radii = np.full(len(p), 0.01, dtype=np.float32)
    cf, cm = emu.normals(radii)
    radii[100], radii[2000] = np.nan, -1.0
    f, m = emu.normals(radii, piece=1000)
    keep = np.ones(len(p), dtype=bool)
    keep[[100, 2000]] = False
    assert same(f[keep], cf[keep]) and same(m[keep], cm[keep]) and cm["count"][100] > 0 and cm["count"][2000] > 0
    assert not m[~keep].view(np.uint8).any()
    assert np.all(f[~keep].view(np.uint32).reshape(2, 8)[:, :7] == NAN_BITS) and not f["count"][~keep].any()


@pytest.mark.parametrize("metric", ["L2Squared", "LPInf"])
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_emulated_kernel_on_a_stream_that_does_not_belong_to_its_points(emu_lib, metric, move):
    """A tree built over one cloud, searched over a shrunk or shifted copy: a point is often absent from its own row and
    still belongs to its neighbourhood (m = c + 1 either way)."""
    p_tree = ds.uniform_cloud(3_000, 3, 61)
    p = (p_tree * F32(0.5) + F32(0.25)) if move == "shrunk" else (p_tree + F32(0.3))
    p = np.ascontiguousarray(p, dtype=np.float32)
    emu = Emulated(emu_lib, p, 8, metric, tree_points=p_tree)
    for r in (0.01, 0.05):
        want = expected_moments(p, *host_search_rows(emu.host, p, r))
        hf, hm = host_normals(emu.host, r, points=p)
        ef, em = emu.normals(r, piece=1000)
        assert same(hm, want) and same(em, want) and same(ef, hf), (metric, move, r)
        check_frames(hf, want, p, None, 2, (metric, move, r))


@pytest.mark.parametrize("depth", [39, 40, 135, 136])
def test_emulated_kernel_where_the_stack_class_changes(emu_lib, depth):
    pts = np.asarray(depth_cases.cloud_at_depth(depth, 3, 10)[0])
    emu = Emulated(emu_lib, pts, 10, "L2Squared")
    want = expected_moments(pts, *host_search_rows(emu.host, pts, 0.05))
    assert np.all(want["count"][3_000:] == len(pts) - 3_001)
    run = depth_cases.Watch(depth, emu_lib)
    ef, em = run(emu.normals, F32(0.05))
    hf, hm = host_normals(emu.host, 0.05)
    assert same(em, want) and same(hm, want) and same(ef, hf), depth
    check_frames(hf, want, pts, None, 2, ("depth", depth))


def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "normals_self_main.cpp"), "-o", out]
    if host_only:
        cmd.insert(1, "-DPICO_TREE_HOST_ONLY")
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def check_cpp(exe, d, tree, p, leaf, metric, r, radii, mn, view):
    """The program's four files against the host loop of `tree` (a handle over the same points and leaf size)."""
    p.tofile(os.path.join(d, "points.bin"))
    radii.tofile(os.path.join(d, "radii.bin"))
    args = [exe, d, repr(float(r)), str(mn), str(leaf), _CPP_METRIC[metric]]
    if view is not None:
        args += [repr(float(x)) for x in view]
    res = subprocess.run(args, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    for name, rr in (("scalar", r), ("radii", radii)):
        hf, hm = host_normals(tree, rr, mn, view, points=p)
        assert np.fromfile(os.path.join(d, name + ".frm"), dtype=pt.FRAME).tobytes() == hf.tobytes(), (metric, name)
        assert np.fromfile(os.path.join(d, name + ".mom"), dtype=pt.MOMENTS).tobytes() == hm.tobytes(), (metric, name)


@needs_reference
@pytest.mark.parametrize("kind,metric,view", [("uniform", "L2Squared", None), ("lidar", "L1", VIEW), ("ties", "LPInf", VIEW),
                                              ("small", "LNInf", None)])
def test_cpp_member_without_a_backend(tmp_path, kind, metric, view):
    c = case(kind, metric)
    exe = str(tmp_path / "normals_self_host")
    _cpp_program(exe, host_only=True)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=pt.PTK_DEVICE_NONE)
    check_cpp(exe, str(tmp_path), tree, c.p, c.leaf, metric, radii_of(c)[2], c.radii(), 3, view)


def test_argument_checks_and_the_python_wrapper_on_a_host_only_handle():
    p = ds.uniform_cloud(9, 3, 21)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    lib = pt._load()
    frames, moments = np.zeros(9, dtype=pt.FRAME), np.zeros(9, dtype=pt.MOMENTS)
    fp, mp = frames.ctypes.data, moments.ctypes.data
    ok = np.full(9, 0.1, dtype=np.float32)
    INVALID, DEVICE = -1, -3
    assert pt.FRAME.itemsize == 32 and pt.MOMENTS.itemsize == 48
    host = lib.ptk_host_normals_within_self
    assert host(tree._h, p.ctypes.data, F32(0.1), None, 2, None, None, None) == INVALID
    assert host(tree._h, None, F32(0.1), None, 2, None, fp, mp) == INVALID
    assert host(None, p.ctypes.data, F32(0.1), None, 2, None, fp, mp) == INVALID
    assert host(tree._h, p.ctypes.data, F32(0.1), None, 2, None, fp, None) == 0
    assert host(tree._h, p.ctypes.data, F32(0.1), None, 2, None, None, mp) == 0
    for bad in (np.nan, -0.5, -INF):
        assert host(tree._h, p.ctypes.data, F32(bad), None, 2, None, fp, mp) == INVALID
        assert "radius must be >= 0" in lib.ptk_last_error().decode()
        assert host(tree._h, p.ctypes.data, F32(bad), ok.ctypes.data, 2, None, fp, mp) == 0  # (ignored beside an array)
    for bad in (np.nan, -1e-3):
        radii = ok.copy()
        radii[4] = radii[7] = bad
        assert host(tree._h, p.ctypes.data, F32(1), radii.ctypes.data, 2, None, fp, mp) == INVALID
        assert "radii[4]" in lib.ptk_last_error().decode()
    # a normal is defined for Euclidean 3-D points: the host loop refuses the rest as the device forms do
    for dim in (2, 5):
        q = ds.uniform_cloud(50, dim, 5)
        t = pt.KdTree(q, pt.Metric.L2Squared, 4, device=pt.PTK_DEVICE_NONE)
        assert host(t._h, q.ctypes.data, F32(0.1), None, 2, None, fp, mp) == INVALID
        assert "3-D" in lib.ptk_last_error().decode()
        assert lib.ptk_normals_within_self(t._h, F32(0.1), None, 2, None, fp, mp) == INVALID
    q = np.random.default_rng(12).random((50, 3), dtype=np.float32)
    se2 = pt.KdTree(q, pt.Metric.SE2Squared, 4, device=pt.PTK_DEVICE_NONE)
    assert host(se2._h, q.ctypes.data, F32(0.1), None, 2, None, fp, mp) == INVALID
    assert "topological" in lib.ptk_last_error().decode()
    assert lib.ptk_normals_within_self(se2._h, F32(0.1), None, 2, None, fp, mp) == INVALID
    # a host-only handle has no device search
    assert lib.ptk_normals_within_self(tree._h, F32(0.1), None, 2, None, fp, mp) == DEVICE
    assert lib.ptk_normals_within_self_device(tree._h, F32(0.1), None, 2, None, fp, mp, None) == DEVICE
    assert lib.ptk_normals_within_self(None, F32(0.1), None, 2, None, fp, mp) == INVALID
    assert lib.ptk_version() == 101
    with pytest.raises(pt.PtkError):
        tree.normals_within_self(0.1)
    for bad in (np.zeros(8, dtype=np.float32), np.zeros((9, 1), dtype=np.float32), "x"):
        with pytest.raises(ValueError):
            tree.normals_within_self(bad)
    with pytest.raises(ValueError):
        tree.normals_within_self(0.1, min_neighbors=-1)
    for bad in ([1.0, 2.0], "x", np.zeros((3, 1))):
        with pytest.raises(ValueError):
            tree.normals_within_self(0.1, viewpoint=bad)
    t64 = pt.KdTree(p.astype(np.float64), pt.Metric.L2Squared, 3, device=pt.PTK_DEVICE_NONE)
    with pytest.raises(pt.PtkError):
        t64.normals_within_self(0.1)


# ---- gpu tier ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@needs_reference
@pytest.mark.parametrize("kind", ["uniform", "lidar", "ties", "small"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_equals_the_contract(gpu, kind, metric, monkeypatch):
    c = case(kind, metric)
    tree = pt.KdTree(c.p, getattr(pt.Metric, metric), c.leaf, device=gpu)
    todo = [(i, r) for i, r in enumerate(radii_of(c))] + [("per row", c.radii())]
    for turn, (which, r) in enumerate(todo):
        want = want_moments(kind, metric, which)
        view = VIEW if turn % 2 else None
        what = (kind, metric, which)
        f, m = device_normals(tree, r, 2, view)
        assert same(m, want), what
        hf, hm = host_normals(tree, r, 2, view, points=c.p)
        assert same(hm, want) and same(f, hf), what
        check_frames(f, want, c.p, view, 2, what)
        # frames only and moments only agree with the run that asks for both; two calls give identical bytes
        assert same(device_normals(tree, r, 2, view, want="frames")[0], f), what
        assert same(device_normals(tree, r, 2, view, want="moments")[1], m), what
    which, r = todo[2]
    monkeypatch.setenv("PTK_MAX_BATCH", "1000")
    f, m = device_normals(tree, r, 5, VIEW)
    monkeypatch.delenv("PTK_MAX_BATCH")
    f1, m1 = device_normals(tree, r, 5, VIEW)
    assert same(f, f1) and same(m, m1) and same(m, want_moments(kind, metric, which)), (kind, metric, "pieces")
    check_frames(f, m, c.p, VIEW, 5, (kind, metric, "pieces"))
    # the Python wrapper
    got, gm = tree.normals_within_self(r, min_neighbors=5, viewpoint=VIEW, moments=True)
    assert got.dtype == pt.FRAME and same(got, f) and same(gm, m)
    assert same(tree.normals_within_self(c.radii()), device_normals(tree, c.radii(), 2, None, want="frames")[0])


def records(t, dtype):
    return np.ascontiguousarray(t.cpu().numpy()).view(dtype).reshape(-1)


@pytest.mark.gpu
@needs_reference
def test_device_form_on_a_side_stream_and_radii_that_pass_no_test(gpu):
    import torch

    c = case("lidar", "L2Squared")
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    radii = c.radii()
    bad = radii.copy()
    bad[100], bad[2000] = np.nan, -1.0
    with torch.cuda.stream(side):
        d_radii = torch.from_numpy(radii).to(f"cuda:{gpu}")
        d_bad = torch.from_numpy(bad).to(f"cuda:{gpu}")
        f, m = tree.normals_within_self(d_radii, viewpoint=VIEW, moments=True, device=True)
        f2, m2 = tree.normals_within_self(d_radii, viewpoint=VIEW, moments=True, device=True)
        fb, mb = tree.normals_within_self(d_bad, viewpoint=VIEW, moments=True, device=True)
        fs = tree.normals_within_self(float(c.values()[1]), device=True)
    side.synchronize()
    want = want_moments("lidar", "L2Squared", "per row")
    f, m, f2, m2 = records(f, pt.FRAME), records(m, pt.MOMENTS), records(f2, pt.FRAME), records(m2, pt.MOMENTS)
    assert same(m, want) and same(f, f2) and same(m, m2)
    assert same(f, host_normals(tree, radii, 2, VIEW, points=c.p)[0])
    assert same(records(fs, pt.FRAME), host_normals(tree, c.values()[1], points=c.p)[0])
    fb, mb = records(fb, pt.FRAME), records(mb, pt.MOMENTS)
    keep = np.ones(c.n, dtype=bool)
    keep[[100, 2000]] = False
    assert want["count"][100] > 0 and want["count"][2000] > 0
    assert same(fb[keep], f[keep]) and same(mb[keep], m[keep]) and not mb[~keep].view(np.uint8).any()
    assert np.all(fb[~keep].view(np.uint32).reshape(2, 8)[:, :7] == NAN_BITS) and not fb["count"][~keep].any()
    with pytest.raises(ValueError):
        tree.normals_within_self(bad, device=True)  # (host radii are checked before they go up)


@pytest.mark.gpu
def test_the_radius_capture_is_left_alone(gpu):
    """A scalar search_radius count / fill pair with a normals call between its halves still copies its captured rows."""
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
    frames = tree.normals_within_self(0.001, device=True)
    again = tree.normals_within_self(np.full(len(p), 0.001, dtype=np.float32))
    offsets = torch.zeros(len(q) + 1, dtype=torch.int64, device=dq.device)
    offsets[1:] = torch.cumsum(counts[:len(q)], 0)
    out = torch.empty((max(int(offsets[-1].item()), 1), 2), dtype=torch.int32, device=dq.device)
    assert lib.ptk_search_radius_fill_device(tree._h, dq.data_ptr(), len(q), F32(0.002), F32(1), offsets.data_ptr(),
                                             out.data_ptr(), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want.offsets)
    rows = np.ascontiguousarray(out.cpu().numpy()).view(pt.NEIGHBOR).reshape(-1)
    assert rows[:len(want.flat)].tobytes() == want.flat.tobytes()
    assert same(records(frames, pt.FRAME), again)
    assert np.array_equal(again["count"], tree.count_within_self(0.001))


@pytest.mark.gpu
def test_hand_written_cases_on_the_device(gpu):
    tree = pt.KdTree(grid(), pt.Metric.L2Squared, 4, device=gpu)
    check_grid(lambda r, mn, view: device_normals(tree, r, mn, view)[0])
    check_tiny(lambda q: device_normals(pt.KdTree(q, pt.Metric.L2Squared, 3, device=gpu), 10.0))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [39, 40, 135, 136, 1031])
def test_depths_where_the_stack_class_changes(gpu, depth):
    pts = np.asarray(depth_cases.cloud_at_depth(depth, 3, 10)[0])
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    depth_cases.assert_depth(tree, depth)
    want = expected_moments(pts, *host_search_rows(tree, pts, 0.05))
    assert np.all(want["count"][3_000:] == len(pts) - 3_001)  # (the rest of the pile, at offset 0)
    f, m = device_normals(tree, 0.05)
    assert same(m, want) and same(f, host_normals(tree, 0.05, points=pts)[0]), depth
    check_frames(f, want, pts, None, 2, ("depth", depth))


@pytest.mark.gpu
def test_refusals(gpu):
    lib = pt._load()
    deep = np.asarray(depth_cases.cloud_at_depth(1032, 3, 10)[0])
    tree = pt.KdTree(deep, pt.Metric.L2Squared, 10, device=gpu)
    with pytest.raises(pt.PtkError) as refused:
        tree.normals_within_self(0.01)
    assert refused.value.status == pt.PTK_ERR_UNSUPPORTED
    assert "tree depth 1032" in str(refused.value) and "ptk_host_normals_within_self" in str(refused.value)
    pt.allow_host_loop(True)
    try:
        with warnings.catch_warnings():  # (the host loop warns once per process)
            warnings.simplefilter("ignore")
            got, gm = tree.normals_within_self(0.01, viewpoint=VIEW, moments=True)
    finally:
        pt.allow_host_loop(False)
    hf, hm = host_normals(tree, 0.01, 2, VIEW, points=deep)
    assert same(got, hf) and same(gm, hm)
    frames, moments = np.zeros(3_000, dtype=pt.FRAME), np.zeros(3_000, dtype=pt.MOMENTS)
    fp, mp = frames.ctypes.data, moments.ctypes.data
    for q, metric in ((ds.uniform_cloud(2_500, 2, 8), pt.Metric.L2Squared), (ds.uniform_cloud(2_500, 5, 10), pt.Metric.L2Squared),
                      (np.random.default_rng(12).random((2_000, 3), dtype=np.float32), pt.Metric.SE2Squared)):
        t = pt.KdTree(q, metric, 8, device=gpu)
        assert lib.ptk_normals_within_self(t._h, F32(0.01), None, 2, None, fp, mp) == -1
        assert lib.ptk_normals_within_self_device(t._h, F32(0.01), None, 2, None, fp, mp, None) == -1
        assert lib.ptk_host_normals_within_self(t._h, q.ctypes.data, F32(0.01), None, 2, None, fp, mp) == -1
        with pytest.raises(pt.PtkError) as invalid:
            t.normals_within_self(0.01)
        assert invalid.value.status == -1
    small = pt.KdTree(cloud("small")[0], pt.Metric.L2Squared, 5, device=gpu)
    bad = np.full(small.npts, 0.1, dtype=np.float32)
    bad[7] = bad[9] = np.nan
    assert lib.ptk_normals_within_self(small._h, F32(0.1), None, 2, None, None, None) == -1
    assert lib.ptk_normals_within_self_device(small._h, F32(0.1), None, 2, None, None, None, None) == -1
    assert lib.ptk_normals_within_self(small._h, F32(np.nan), None, 2, None, fp, mp) == -1
    assert lib.ptk_normals_within_self(small._h, F32(-1), None, 2, None, fp, mp) == -1
    assert lib.ptk_normals_within_self(small._h, F32(1), bad.ctypes.data, 2, None, fp, mp) == -1
    assert "radii[7]" in lib.ptk_last_error().decode()
    t64 = pt.KdTree(cloud("small")[0].astype(np.float64), pt.Metric.L2Squared, 5, device=gpu)
    with pytest.raises(pt.PtkError):
        t64.normals_within_self(0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["L2Squared", "LPInf"])
@pytest.mark.parametrize("move", ["shrunk", "shifted"])
def test_streams_that_do_not_belong_to_their_points(gpu, tmp_path, metric, move):
    p_tree = ds.uniform_cloud(3_000, 3, 61)
    p = (p_tree * F32(0.5) + F32(0.25)) if move == "shrunk" else (p_tree + F32(0.3))
    p = np.ascontiguousarray(p, dtype=np.float32)
    fn = str(tmp_path / "tree.bin")
    pt.save_kd_tree(pt.KdTree(p_tree, getattr(pt.Metric, metric), 8, device=pt.PTK_DEVICE_NONE), fn)
    tree = pt.load_kd_tree(p, fn, device=gpu)
    for r in (0.01, 0.05):
        want = expected_moments(p, *host_search_rows(tree, p, r))
        f, m = device_normals(tree, r, 2, VIEW)
        assert same(m, want) and same(f, host_normals(tree, r, 2, VIEW, points=p)[0]), (metric, move, r)
        check_frames(f, want, p, VIEW, 2, (metric, move, r))


@pytest.mark.gpu
@needs_reference
def test_cpp_member_through_the_backend(gpu, tmp_path):
    c = case("uniform", "L2Squared")
    exe = str(tmp_path / "normals_self_batch")
    _cpp_program(exe, host_only=False)
    tree = pt.KdTree(c.p, pt.Metric.L2Squared, c.leaf, device=pt.PTK_DEVICE_NONE)
    check_cpp(exe, str(tmp_path), tree, c.p, c.leaf, "L2Squared", radii_of(c)[2], c.radii(), 3, VIEW)
