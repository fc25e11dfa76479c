"""align_step: the normal equations of one ICP iteration, reduced on the device (ptk.h).

Expected values are the contract restated in numpy (``restate``): the pose in float32, one operation at a time; the
terms in float64; every sum as the fixed tree written with reshapes -- per level four sequential adds from +0, then six
halving steps.  The rows the restatement sums over are ``ptk_host_search_knn`` rows of the numpy-posed queries, which the
project already trusts; nothing expected comes from the code under test.  Records are compared byte for byte.

The CPU tier runs the host loop (``ptk_host_align_step``) on host-only handles, the real source of the K22 kernels in the
emulator (tests/cpp/emulate_align.cpp: the wavefronts as 64 fibers meeting at every shuffle), the C++ member
(tests/cpp/align_main.cpp, -DPICO_TREE_HOST_ONLY under -fsanitize=address,undefined), the argument checks and
``AlignSums.solve``; the gpu tier the device form and the host-buffer form.
"""

from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import pico_tree_amd as pt
from pico_tree_amd import datasets as ds
from tests import depth_cases, poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")
FLT_MAX = F32(np.finfo(np.float32).max)
INVALID, UNSUPPORTED, DEVICE = -1, -2, -3
#: block and level edges: 65 536 rows are 256 blocks and two levels, 65 537 are 257 -> 2 -> 1, three levels
NQ = [0, 1, 63, 64, 65, 255, 256, 257, 65536, 65537]
MODES = ["point", "plane"]
POINT_FIELDS = ["sum_distance", "sum_q", "sum_p", "sum_qp", "sum_qq", "sum_pp"]
PLANE_FIELDS = ["sum_distance", "jtj", "jtr", "sum_rr"]
N_TARGET = 5000


# ---- the contract in numpy ------------------------------------------------------------------------------------------------

def pose32(T, q):
    """q' = ((R_a0*x + R_a1*y) + R_a2*z) + t_a, every operation a float32 operation.  T: (3, 4) float32 or None."""
    if T is None:
        return q
    T = np.asarray(T, dtype=np.float32).reshape(3, 4)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    out = np.empty_like(q)
    with np.errstate(all="ignore"):
        for a in range(3):
            v = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
            assert v.dtype == np.float32
            out[:, a] = v
    return out


def host_rows(tree, p, qp):
    """ptk_host_search_knn(q', k = 1, e = 1): the rows the contract names."""
    out = np.zeros(len(qp), dtype=pt.NEIGHBOR)
    qp = np.ascontiguousarray(qp)
    rc = pt._load().ptk_host_search_knn(tree._h, p.ctypes.data, qp.ctypes.data, len(qp), 1, F32(1), out.ctypes.data)
    assert rc == 0, pt._load().ptk_last_error()
    return out


def terms_of(p, qp, rows, max_distance, normals):
    """(terms float64 [nq, T] in the order of the record's fields of the mode, accepted mask).  A rejected row is +0."""
    nq = len(qp)
    d = rows["distance"]
    with np.errstate(invalid="ignore"):
        ok = (d < F32(max_distance)) & (d < FLT_MAX)
    idx = np.where(ok, rows["index"], 0)
    q = qp.astype(np.float64)
    m = p[idx].astype(np.float64)
    dist = d.astype(np.float64)
    return _terms(nq, ok, q, m, dist, idx, normals)


@np.errstate(all="ignore")  # (a rejected row's arithmetic may be anything: its terms are replaced by +0 below)
def _terms(nq, ok, q, m, dist, idx, normals):
    if normals is None:
        cols = [dist] + [q[:, a] for a in range(3)] + [m[:, a] for a in range(3)]
        cols += [q[:, a] * m[:, b] for a in range(3) for b in range(3)]
        cols.append((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        cols.append((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    else:
        nf = normals[idx]
        ok = ok & np.isfinite(nf).all(axis=1)
        n = np.where(ok[:, None], nf, F32(0)).astype(np.float64)
        e = [q[:, a] - m[:, a] for a in range(3)]
        r = ((e[0] * n[:, 0]) + (e[1] * n[:, 1])) + (e[2] * n[:, 2])
        J = [(q[:, 1] * n[:, 2]) - (q[:, 2] * n[:, 1]), (q[:, 2] * n[:, 0]) - (q[:, 0] * n[:, 2]),
             (q[:, 0] * n[:, 1]) - (q[:, 1] * n[:, 0]), n[:, 0], n[:, 1], n[:, 2]]
        cols = [dist] + [J[u] * J[v] for u in range(6) for v in range(u, 6)] + [J[u] * r for u in range(6)] + [r * r]
    with np.errstate(all="ignore"):
        t = np.stack(cols, axis=1) if nq else np.zeros((0, len(cols)))
    t = np.where(ok[:, None], t, 0.0)  # (+0.0, whatever the unaccepted row's arithmetic gave)
    return np.ascontiguousarray(t, dtype=np.float64), ok


def tree_sum(x):
    """The fixed tree over axis 0 of x [n, T], n > 0: levels of blocks of 256, four sequential adds, six halvings."""
    x = np.asarray(x, dtype=np.float64)
    levels = 0
    while True:
        n, t = x.shape
        nb = (n + 255) // 256
        pad = np.zeros((nb * 256, t))
        pad[:n] = x
        b = pad.reshape(nb, 4, 64, t)  # entry l + 64 j of a block at [j, l]
        v = (((0.0 + b[:, 0]) + b[:, 1]) + b[:, 2]) + b[:, 3]
        s = 32
        while s >= 1:
            v = v[:, :s] + v[:, s:2 * s]
            s //= 2
        x = v[:, 0]
        levels += 1
        if nb == 1:
            return x[0], levels


def record_of(plane, count, rows, sums):
    rec = np.zeros((1,), dtype=pt.ALIGN_SUMS)
    rec["count"], rec["rows"] = count, rows
    if sums is not None:
        names = PLANE_FIELDS if plane else POINT_FIELDS
        at = 0
        for name in names:
            w = int(np.prod(pt.ALIGN_SUMS[name].shape, dtype=np.int64)) if pt.ALIGN_SUMS[name].shape else 1
            rec[name] = sums[at:at + w] if w > 1 else sums[at]
            at += w
        assert at == len(sums)
    return rec


def restate(tree, p, q, T, max_distance, normals):
    """(record, rows, q') of the contract."""
    qp = pose32(T, q)
    rows = host_rows(tree, p, qp)
    if len(q) == 0:
        return record_of(normals is not None, 0, 0, None), rows, qp
    t, ok = terms_of(p, qp, rows, max_distance, normals)
    sums, _ = tree_sum(t)
    return record_of(normals is not None, int(ok.sum()), len(q), sums), rows, qp


# ---- data -------------------------------------------------------------------------------------------------------------------

def host_tree(p, leaf=10, metric=pt.Metric.L2Squared):
    return pt.KdTree(np.ascontiguousarray(p), metric, leaf, device=pt.PTK_DEVICE_NONE)


def unit_normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return np.ascontiguousarray((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))


def rigid(angle, axis, t):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)
    m[:3, 3] = t
    return m


POSE = np.ascontiguousarray(rigid(0.03, [0.2, -0.1, 1.0], [0.4, -0.3, 0.1])[:3, :], dtype=np.float32)


class Target:
    """The 5 000-point tree of the issue, its normals, and a query cloud of which every batch is a prefix."""

    def __init__(self):
        self.p = ds.lidar_cloud(N_TARGET, seed=1)
        self.tree = host_tree(self.p)
        self.normals = unit_normals(N_TARGET, 5)
        self.q = ds.lidar_cloud(max(NQ), seed=2, pose=(3.0, 1.5))
        d = host_rows(self.tree, self.p, pose32(POSE, self.q[:4096]))["distance"]
        self.split = F32(np.median(d))  # a rejection distance that splits a batch

    def normals_of(self, mode):
        return self.normals if mode == "plane" else None


@functools.lru_cache(maxsize=None)
def target():
    return Target()


@functools.lru_cache(maxsize=None)
def expected(mode, nq):
    """The restated record of the standard call at nq rows: computed once, shared by the tiers."""
    c = target()
    rec, rows, qp = restate(c.tree, c.p, c.q[:nq], POSE, c.split, c.normals_of(mode))
    return rec.tobytes(), rows, qp


def host_step(tree, q, T, max_distance, normals, rows=False):
    return tree.align_step(np.ascontiguousarray(q), T, max_distance, normals, rows=rows, host_loop=True)


# ---- CPU tier: the host loop against the restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("nq", NQ)
@pytest.mark.parametrize("mode", MODES)
def test_host_loop_equals_the_restatement(mode, nq):
    c = target()
    want, want_rows, _ = expected(mode, nq)
    sums, rows = host_step(c.tree, c.q[:nq], POSE, c.split, c.normals_of(mode), rows=True)
    assert sums.tobytes() == want
    assert rows.tobytes() == want_rows.tobytes()
    assert sums.rows == nq and (nq < 64 or 0 < sums.count < nq)
    # (without the rows: the same record; a second call: the same record)
    assert host_step(c.tree, c.q[:nq], POSE, c.split, c.normals_of(mode)).tobytes() == want
    other = PLANE_FIELDS if mode == "point" else POINT_FIELDS
    for name in other[1:]:
        assert not np.asarray(sums.record[name]).view(np.uint64).any(), name  # +0, not -0


@pytest.mark.parametrize("mode", MODES)
def test_sums_against_exact_sums(mode):
    """|sum - exact| <= 64 * 2^-53 * sum |term|.  Derivation: a path from a term to the root of the tree passes, per
    level, at most 4 adds in its lane and 6 halving adds: 10 roundings per level, 10 * levels <= 40 for levels <= 4.
    A term has at most 4 roundings of its own, so no more than 44 <= 64 relative perturbations of 2^-53 touch any term's
    contribution, and (1 + u)^44 - 1 < 64 u.  ``exact`` is math.fsum of the same terms: the terms as the contract rounds
    them (the differences in a point-to-plane term cancel, so its own roundings are not relative to the term; they are
    common to both sides here, and the 4 stay in the bound as slack)."""
    c = target()
    nq = 65537
    qp = pose32(POSE, c.q[:nq])
    rows = host_rows(c.tree, c.p, qp)
    t, _ = terms_of(c.p, qp, rows, INF, c.normals_of(mode))
    got, levels = tree_sum(t)
    assert levels == 3 <= 4
    sums = host_step(c.tree, c.q[:nq], POSE, INF, c.normals_of(mode))
    flat = np.concatenate([np.atleast_1d(sums.record[name][0]).ravel() for name in (PLANE_FIELDS if mode == "plane" else POINT_FIELDS)])
    assert flat.tobytes() == got.tobytes()
    for j in range(t.shape[1]):
        exact = math.fsum(t[:, j])
        bound = 64 * 2.0 ** -53 * math.fsum(np.abs(t[:, j]))
        assert abs(flat[j] - exact) <= bound, (j, flat[j], exact, bound)


# ---- CPU tier: the kernels in the emulator ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/cpp/emulate_align.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_align") / "libptk_emu_align.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "cpp"),
        os.path.join(ROOT, "tests", "cpp", "emulate_align.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    lib.emu_create.restype = vp
    lib.emu_create.argtypes = [vp, u64, u32, vp, u64, vp]
    lib.emu_destroy.argtypes = [vp]
    lib.emu_align_step.argtypes = [vp, vp, u64, vp, ctypes.c_float, vp, vp, vp, vp]
    return lib


def emulated(lib, tree, p, q, T, max_distance, normals, rows):
    """(record bytes, q') of the K22 kernels over `rows`."""
    nodes, idx, _, _ = tree.flat()
    h = lib.emu_create(p.ctypes.data, len(p), 3, nodes.ctypes.data, len(nodes), idx.ctypes.data)
    assert h
    try:
        q = np.ascontiguousarray(q)
        rec = np.full((1,), 0, dtype=pt.ALIGN_SUMS)
        rec.view(np.uint8)[:] = 0xA5
        posed = np.zeros((len(q), 3), dtype=np.float32)
        Tm = None if T is None else np.ascontiguousarray(T, dtype=np.float32)
        rc = lib.emu_align_step(h, q.ctypes.data, len(q), None if Tm is None else Tm.ctypes.data, F32(max_distance),
                                None if normals is None else normals.ctypes.data, rows.ctypes.data, rec.ctypes.data,
                                posed.ctypes.data)
        assert rc == 0
        return rec.tobytes(), posed
    finally:
        lib.emu_destroy(h)


#: (every edge in point-to-point; the three-level batch in point-to-plane, whose records are the wider ones)
@pytest.mark.parametrize("mode,nq", [("point", n) for n in NQ[:-1]] + [("plane", n) for n in NQ[:-2] + [NQ[-1]]])
def test_emulated_kernels_equal_the_host_loop(emu_lib, mode, nq):
    c = target()
    want, rows, qp = expected(mode, nq)
    got, posed = emulated(emu_lib, c.tree, c.p, c.q[:nq], POSE, c.split, c.normals_of(mode), rows)
    assert got == want
    assert posed.tobytes() == qp.tobytes()


# ---- CPU tier: the C++ member -------------------------------------------------------------------------------------------------

def _cpp_program(out, host_only):
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "align_main.cpp"), "-o", out]
    if host_only:  # (a stand-alone host program: the place for the sanitizers)
        cmd[1:1] = ["-DPICO_TREE_HOST_ONLY", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    else:
        libdir = os.path.join(ROOT, "pico_tree_amd", "csrc")
        cmd += ["-L" + libdir, "-lptk", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)


def check_cpp(exe, d, nq):
    c = target()
    for name, a in (("points", c.p), ("queries", c.q[:nq]), ("normals", c.normals), ("transform", POSE)):
        np.ascontiguousarray(a, dtype=np.float32).tofile(os.path.join(d, name + ".bin"))
    res = subprocess.run([exe, d, repr(float(c.split)), "10"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    read = lambda name: open(os.path.join(d, name), "rb").read()
    want, rows, _ = expected("point", nq)
    assert read("point.sums") == want and read("point.rows") == rows.tobytes()
    assert read("plane.sums") == expected("plane", nq)[0]
    assert read("point_identity.sums") == restate(c.tree, c.p, c.q[:nq], None, c.split, None)[0].tobytes()


@pytest.mark.parametrize("nq", [257, 65537])
def test_cpp_member_without_a_backend_under_the_sanitizers(tmp_path_factory, tmp_path, nq):
    exe = str(tmp_path_factory.getbasetemp() / "align_host")
    if not os.path.exists(exe):
        _cpp_program(exe, host_only=True)
    check_cpp(exe, str(tmp_path), nq)


# ---- CPU tier: acceptance ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_rejection_distances(mode):
    c = target()
    q, normals = c.q[:1000], c.normals_of(mode)
    none = host_step(c.tree, q, POSE, 0.0, normals)
    assert none.count == 0 and none.rows == 1000
    assert none.tobytes() == record_of(mode == "plane", 0, 1000, None).tobytes()  # every sum +0
    some = host_step(c.tree, q, POSE, c.split, normals)
    every = host_step(c.tree, q, POSE, INF, normals)
    assert 0 < some.count < every.count == 1000
    for md, got in ((c.split, some), (INF, every)):
        assert got.tobytes() == restate(c.tree, c.p, q, POSE, md, normals)[0].tobytes()
    # strict: a rejection distance equal to a row's distance rejects that row, the next number above it accepts it
    rows = host_rows(c.tree, c.p, pose32(POSE, q))
    d = np.sort(rows["distance"])[500]
    at, above = host_step(c.tree, q, POSE, d, normals), host_step(c.tree, q, POSE, np.nextafter(d, F32(np.inf)), normals)
    assert at.count == int((rows["distance"] < d).sum()) < above.count == int((rows["distance"] <= d).sum())


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_and_overflowing_queries_are_rejected_and_change_nothing_else(mode):
    c = target()
    clean, normals = c.q[:2000], c.normals_of(mode)
    bad, mask = poison.poison(clean, seed=3)
    assert mask.sum() > 100
    sums, rows = host_step(c.tree, bad, None, INF, normals, rows=True)
    want, want_rows, _ = restate(c.tree, c.p, bad, None, INF, normals)
    assert sums.tobytes() == want.tobytes() and rows.tobytes() == want_rows.tobytes()
    pad = ~(rows["distance"] < FLT_MAX)
    assert pad.any() and (rows["index"][pad] == 0).all() and (rows["distance"][pad] == FLT_MAX).all()
    assert sums.count == 2000 - int(pad.sum())
    # every other row's contribution unchanged: the terms of the rows that were left alone are those of the clean batch,
    # bit for bit, and a rejected row's terms are all +0
    t_bad, ok_bad = terms_of(c.p, bad, rows, INF, normals)
    t_clean, _ = terms_of(c.p, clean, host_rows(c.tree, c.p, clean), INF, normals)
    same_query = ~mask
    assert np.array_equal(t_bad[same_query].view(np.uint64), t_clean[same_query].view(np.uint64))
    assert not t_bad[~ok_bad].view(np.uint64).any()
    # under a pose the non-finite rows stay rejected (NaN and inf go through the float32 arithmetic as IEEE has it)
    posed = host_step(c.tree, bad, POSE, INF, normals)
    assert posed.tobytes() == restate(c.tree, c.p, bad, POSE, INF, normals)[0].tobytes()


def test_a_row_without_a_neighbour_gives_the_pad_and_is_rejected():
    """k = 1 never exceeds n_points (a tree holds a point); the row no search fills is the one whose every distance
    overflows: on a one-point tree it is the pad {0, FLT_MAX}, rejected even by max_distance = +inf."""
    p = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    tree = host_tree(p)
    q = np.array([[1.5, 2.0, 3.0], [3e38, 0, 0], [-3e38, 3e38, 0]], dtype=np.float32)
    sums, rows = host_step(tree, q, None, INF, None, rows=True)
    assert rows["index"].tolist() == [0, 0, 0] and rows["distance"].tolist() == [0.25, FLT_MAX, FLT_MAX]
    assert sums.count == 1 and sums.rows == 3 and sums.sum_distance == 0.25
    assert sums.tobytes() == restate(tree, p, q, None, INF, None)[0].tobytes()


def test_a_non_finite_normal_rejects_its_rows():
    c = target()
    q = c.q[:3000]
    rows = host_rows(c.tree, c.p, pose32(POSE, q))
    normals = c.normals.copy()
    hit = np.unique(rows["index"])[::7]
    normals[hit[0::3], 0] = np.nan
    normals[hit[1::3], 1] = np.inf
    normals[hit[2::3], 2] = -np.inf
    sums = host_step(c.tree, q, POSE, INF, normals)
    rejected = int(np.isin(rows["index"], hit).sum())
    assert rejected > 0 and sums.count == 3000 - rejected
    assert sums.tobytes() == restate(c.tree, c.p, q, POSE, INF, normals)[0].tobytes()
    # (point-to-point does not look at the normals)
    assert host_step(c.tree, q, POSE, INF, None).count == 3000


@pytest.mark.parametrize("mode", MODES)
def test_no_transform_and_the_identity_give_the_same_bytes(mode):
    """1*x + 0*y + 0*z + 0 is exact for finite x, so the identity matrix poses every finite query onto itself and the
    record is that of transform = None.  A -0 coordinate becomes +0 under the identity (-0 + 0 = +0): q' differs in
    that sign bit, which no sum sees -- every sum starts at +0 and the distance squares the difference."""
    c = target()
    normals = c.normals_of(mode)
    eye = np.eye(4)[:3]
    q = c.q[:1500].copy()
    a, b = host_step(c.tree, q, None, c.split, normals), host_step(c.tree, q, eye, c.split, normals)
    assert a.tobytes() == b.tobytes() and pose32(eye, q).tobytes() == q.tobytes()
    q[::5, 0] = F32(-0.0)
    q[1::5, 2] = F32(-0.0)
    a, b = host_step(c.tree, q, None, c.split, normals), host_step(c.tree, q, eye, c.split, normals)
    assert a.tobytes() == b.tobytes() and a.count > 0
    assert pose32(eye, q).tobytes() != q.tobytes() and np.array_equal(pose32(eye, q), q)


# ---- CPU tier: refusals -------------------------------------------------------------------------------------------------------

def _raw_host(tree, p, q, T, md, normals, out, rows=None):
    lib = pt._load()
    rc = lib.ptk_host_align_step(tree._h, p.ctypes.data, None if q is None else q.ctypes.data, 0 if q is None else len(q),
                                 None if T is None else T.ctypes.data, F32(md),
                                 None if normals is None else normals.ctypes.data, out, rows)
    return rc, lib.ptk_last_error().decode()


def _raw_device(tree, q_ptr, nq, md, out, ws, ws_bytes):
    lib = pt._load()
    rc = lib.ptk_align_step_device(tree._h, q_ptr, nq, None, F32(md), None, out, None, ws, ws_bytes, None)
    return rc, lib.ptk_last_error().decode()


def test_refusals_on_host_only_handles():
    lib = pt._load()
    rec = np.zeros(1, dtype=pt.ALIGN_SUMS)
    out = rec.ctypes.data
    rng = np.random.default_rng(0)
    # dim 2 and dim 5: PTK_ERR_INVALID from every form, the host loop included
    for dim in (2, 5):
        p = rng.random((200, dim)).astype(np.float32)
        tree = host_tree(p)
        q = p[:10].copy()
        rc, why = _raw_host(tree, p, q, None, 1.0, None, out)
        assert rc == INVALID and "3-D" in why
        assert lib.ptk_align_step(tree._h, q.ctypes.data, 10, None, F32(1), None, out, None) == INVALID
        assert _raw_device(tree, q.ctypes.data, 10, 1.0, out, out, 1 << 20)[0] == INVALID
        with pytest.raises(pt.PtkError):
            tree.align_step(q, host_loop=True)
    # every metric but L2Squared
    p3 = rng.random((200, 3)).astype(np.float32)
    q3 = p3[:10].copy()
    for metric in pt.Metric:
        if metric.name in ("L2Squared", "SO2"):  # (SO2 is one-dimensional: refused by its dimension, below)
            continue
        tree = host_tree(p3, metric=metric)
        rc, why = _raw_host(tree, p3, q3, None, 1.0, None, out)
        assert rc == INVALID and "metric_l2_squared" in why, metric
        assert lib.ptk_align_step(tree._h, q3.ctypes.data, 10, None, F32(1), None, out, None) == INVALID, metric
        assert _raw_device(tree, q3.ctypes.data, 10, 1.0, out, out, 1 << 20)[0] == INVALID, metric
    p1 = rng.random((200, 1)).astype(np.float32)
    assert _raw_host(host_tree(p1, metric=pt.Metric.SO2), p1, p1[:5].copy(), None, 1.0, None, out)[0] == INVALID
    # NaN and negative max_distance; null pointers
    tree = host_tree(p3)
    for md in (float("nan"), -1.0, -0.5):
        rc, why = _raw_host(tree, p3, q3, None, md, None, out)
        assert rc == INVALID and "max_distance" in why
        assert lib.ptk_align_step(tree._h, q3.ctypes.data, 10, None, F32(md), None, out, None) == INVALID
        assert _raw_device(tree, q3.ctypes.data, 10, md, out, out, 1 << 20)[0] == INVALID
        with pytest.raises(pt.PtkError):
            tree.align_step(q3, max_distance=md, host_loop=True)
    assert _raw_host(tree, p3, q3, None, 1.0, None, None)[0] == INVALID          # null record
    assert lib.ptk_host_align_step(tree._h, p3.ctypes.data, None, 10, None, F32(1), None, out, None) == INVALID  # null queries
    assert lib.ptk_host_align_step(tree._h, None, q3.ctypes.data, 10, None, F32(1), None, out, None) == INVALID  # null points
    assert lib.ptk_host_align_step(None, p3.ctypes.data, q3.ctypes.data, 10, None, F32(1), None, out, None) == INVALID
    assert lib.ptk_align_step(tree._h, q3.ctypes.data, 10, None, F32(1), None, None, None) == INVALID
    assert lib.ptk_align_step(tree._h, None, 10, None, F32(1), None, out, None) == INVALID
    assert _raw_device(tree, q3.ctypes.data, 10, 1.0, None, out, 1 << 20)[0] == INVALID
    # a host-only handle: PTK_ERR_DEVICE from the device forms once the arguments are good; the host loop serves it
    assert lib.ptk_align_step(tree._h, q3.ctypes.data, 10, None, F32(1), None, out, None) == DEVICE
    assert _raw_device(tree, q3.ctypes.data, 10, 1.0, out, out, 1 << 20)[0] == DEVICE
    with pytest.raises(pt.PtkError):
        tree.align_step(q3)
    assert _raw_host(tree, p3, q3, None, 1.0, None, out)[0] == 0 and rec["rows"][0] == 10
    # the workspace size: 0 for an empty batch, growing with the rows
    need = ctypes.c_uint64(7)
    assert lib.ptk_align_step_workspace(tree._h, 0, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.ptk_align_step_workspace(tree._h, 1000, ctypes.byref(need)) == 0 and need.value >= 1000 * 20
    assert lib.ptk_align_step_workspace(tree._h, 1000, None) == INVALID
    # float64 trees and the wrapper's own checks
    with pytest.raises(pt.PtkError):
        pt.KdTree(p3.astype(np.float64), device=pt.PTK_DEVICE_NONE).align_step(q3.astype(np.float64), host_loop=True)
    with pytest.raises(ValueError):
        tree.align_step(q3, transform=np.eye(3), host_loop=True)
    with pytest.raises(ValueError):
        tree.align_step(q3, normals=np.zeros((5, 3), dtype=np.float32), host_loop=True)


# ---- CPU tier: solve() --------------------------------------------------------------------------------------------------------

def exact_record(p, q, rows, normals):
    """(the record with every sum replaced by math.fsum of its terms, the bound 64 * 2^-53 * sum |term| of each sum)."""
    t, ok = terms_of(p, q, rows, INF, normals)
    sums = np.array([math.fsum(t[:, j]) for j in range(t.shape[1])])
    bound = np.array([64 * 2.0 ** -53 * math.fsum(np.abs(t[:, j])) for j in range(t.shape[1])])
    plane = normals is not None
    return record_of(plane, int(ok.sum()), len(q), sums)[0], record_of(plane, 0, 0, bound)[0]


def separated_subset(c, motion_bound):
    """Points of the target whose nearest other point is more than 4 x `motion_bound` away: a source point moved by
    less than `motion_bound` still has its own original as its nearest neighbour."""
    out = np.zeros((N_TARGET, 1), dtype=pt.NEIGHBOR)
    assert pt._load().ptk_host_search_knn_self(c.tree._h, c.p.ctypes.data, 1, out.ctypes.data) == 0
    return np.flatnonzero(out["distance"][:, 0] > F32((4 * motion_bound) ** 2))


def test_solve_point_to_point_returns_the_motion():
    """A source made by the inverse of a known rigid motion M of a subset of the target, the motion small against the
    spacing of the subset so that every correspondence is the identity: solve() returns M.

    Tolerance 1: against the same numpy solve of fsum-exact sums.  The sums differ from the exact ones by at most
    B = 64 * 2^-53 * sum |term| each (test_sums_against_exact_sums).  Propagated: H = sum_qp - sum_q sum_p^T / n moves by
    dH <= B_qp + (B_q |sum_p| + |sum_q| B_p) / n entrywise; the orthogonal polar factor of H moves by at most
    2 |dH|_F / (s2 + s3) (Li 1995, perturbation of the polar factor; s: singular values of H); t = mean_p - R mean_q by
    at most |B_p| / n + |dR| |mean_q| + |B_q| / n.  Both solves also pay numpy's own rounding in a 3 x 3 SVD and three
    3 x 3 products, each backward stable to a few units of 2^-53 of its operands: 64 * 2^-52 * (1 + |t| + |mean|).
    Tolerance 2: against M itself, by the same propagation of the one other error there is, the rounding of the source
    to float32: each source point is off by at most e = sqrt(3) * 2^-24 * max |q|, so dH <= e sqrt(n) |P_c|_F."""
    c = target()
    M = rigid(0.002, [0.3, 1.0, -0.4], [0.010, -0.020, 0.005])
    reach = float(np.abs(c.p).max()) * math.sqrt(3)
    moved = 0.002 * reach + 0.03  # (no point moves further)
    sel = separated_subset(c, moved)
    assert len(sel) > 300
    S = c.p[sel].astype(np.float64)
    inv = np.linalg.inv(M)
    q = np.ascontiguousarray((S @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    sums, rows = host_step(c.tree, q, None, INF, None, rows=True)
    assert np.array_equal(rows["index"], sel) and sums.count == len(sel)
    got = sums.solve()
    exact, B = exact_record(c.p, q, rows, None)
    want = pt.solve_align_sums(exact, False)
    n = float(len(sel))
    sq, sp = exact["sum_q"], exact["sum_p"]
    dH = B["sum_qp"].reshape(3, 3) + (np.outer(B["sum_q"], np.abs(sp)) + np.outer(np.abs(sq), B["sum_p"])) / n
    H = exact["sum_qp"].reshape(3, 3) - np.outer(sq, sp) / n
    s = np.linalg.svd(H, compute_uv=False)
    mean = max(np.linalg.norm(sq / n), np.linalg.norm(sp / n))
    own = 64 * 2.0 ** -52 * (1 + np.linalg.norm(want[:3, 3]) + mean)
    dR = 2 * np.linalg.norm(dH) / (s[1] + s[2])
    dt = np.linalg.norm(B["sum_p"]) / n + dR * mean + np.linalg.norm(B["sum_q"]) / n
    assert np.linalg.norm(got[:3, :3] - want[:3, :3]) <= dR + own, (np.linalg.norm(got[:3, :3] - want[:3, :3]), dR, own)
    assert np.linalg.norm(got[:3, 3] - want[:3, 3]) <= dt + own
    assert np.array_equal(got[3], [0, 0, 0, 1]) and abs(np.linalg.det(got[:3, :3]) - 1) < 1e-12
    # against the motion itself
    e = math.sqrt(3) * 2.0 ** -24 * float(np.abs(q).max())
    Pc = S - S.mean(axis=0)
    dR2 = 2 * e * math.sqrt(n) * np.linalg.norm(Pc) / (s[1] + s[2])
    assert np.linalg.norm(got[:3, :3] - M[:3, :3]) <= dR2 + dR + own
    assert np.linalg.norm(got[:3, 3] - M[:3, 3]) <= e + dR2 * mean + dt + own
    assert sums.rms <= moved
    with pytest.raises(ValueError):
        host_step(c.tree, q[:2], None, INF, None).solve()
    assert host_step(c.tree, q[:3], None, INF, None).solve().shape == (4, 4)


def test_solve_point_to_plane_against_exact_sums():
    """The same source with the target's normals: solve() is jtj x = -jtr and the exponential map.  Tolerance: the same
    numpy solve of fsum-exact sums.  With A = jtj, b = jtr moved by dA, db (|.| <= the bound B of each sum):
    |dx| <= |A^-1| (|db| + |dA| |x|) / (1 - |A^-1| |dA|); the rotation is exp of the skew matrix of x[:3], 1-Lipschitz, so
    it moves by at most sqrt(2) |dx| in the Frobenius norm, the translation by |dx|.  numpy's own solve is backward stable:
    64 * 2^-52 * cond(A) * |x| on either side.  (Against M itself the linearisation is second order in the angle: the
    increment is M only to about angle^2 * |q|, which is why the loop iterates; checked as such.)"""
    c = target()
    M = rigid(0.002, [0.3, 1.0, -0.4], [0.010, -0.020, 0.005])
    reach = float(np.abs(c.p).max()) * math.sqrt(3)
    sel = separated_subset(c, 0.002 * reach + 0.03)
    S = c.p[sel].astype(np.float64)
    inv = np.linalg.inv(M)
    q = np.ascontiguousarray((S @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    sums, rows = host_step(c.tree, q, None, INF, c.normals, rows=True)
    assert np.array_equal(rows["index"], sel) and sums.count == len(sel)
    got = sums.solve()
    exact, B = exact_record(c.p, q, rows, c.normals)
    want = pt.solve_align_sums(exact, True)

    def sym(tri):
        a = np.zeros((6, 6))
        a[np.triu_indices(6)] = tri
        return a + np.triu(a, 1).T

    A, dA = sym(exact["jtj"]), np.linalg.norm(sym(B["jtj"]))
    x = np.linalg.solve(A, -exact["jtr"])
    ainv = np.linalg.norm(np.linalg.inv(A), 2)
    assert ainv * dA < 0.5
    dx = ainv * (np.linalg.norm(B["jtr"]) + dA * np.linalg.norm(x)) / (1 - ainv * dA)
    own = 64 * 2.0 ** -52 * np.linalg.cond(A) * np.linalg.norm(x)
    assert np.linalg.norm(got[:3, :3] - want[:3, :3]) <= math.sqrt(2) * (dx + own)
    assert np.linalg.norm(got[:3, 3] - want[:3, 3]) <= dx + own
    assert np.allclose(sums.normal_matrix, sym(sums.jtj)) and np.array_equal(sums.normal_matrix, sums.normal_matrix.T)
    second_order = 0.002 ** 2 * reach + 2 * 0.002 * 0.03
    assert np.abs(got - M).max() <= 8 * second_order + 1e-6
    with pytest.raises(ValueError):
        host_step(c.tree, q[:5], None, INF, c.normals).solve()


def test_icp_on_the_host_loop_recovers_a_motion():
    c = target()
    M = rigid(0.01, [0.1, 0.2, 1.0], [0.15, -0.1, 0.05])
    sel = separated_subset(c, 0.3)
    inv = np.linalg.inv(M)
    q = np.ascontiguousarray((c.p[sel].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    before = q.copy()
    res = pt.icp(c.tree, q, 4.0, iterations=10, step=lambda T: host_step(c.tree, q, T, 4.0, None))
    assert q.tobytes() == before.tobytes()
    assert res.iterations <= 10 and res.rms[-1] < res.rms[0]
    assert np.abs(res.transform - M).max() < 1e-4
    assert all(pose.dtype == np.float64 for pose in res.poses)


# ---- gpu tier -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gpu_target(gpu):
    c = target()
    return pt.KdTree(c.p, pt.Metric.L2Squared, 10, device=gpu)


def device_step(tree, gpu, q, T, max_distance, normals, rows=False, stream=None):
    import torch
    dev = f"cuda:{gpu}"
    dq = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    dn = None if normals is None else torch.from_numpy(normals).to(dev)
    if stream is None:
        return tree.align_step(dq, T, max_distance, dn, rows=rows)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        return tree.align_step(dq, T, max_distance, dn, rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQ)
@pytest.mark.parametrize("mode", MODES)
def test_device_and_host_forms_equal_the_host_loop(gpu, mode, nq):
    c, tree = target(), gpu_target(gpu)
    want, want_rows, qp = expected(mode, nq)
    sums, rows = device_step(tree, gpu, c.q[:nq], POSE, c.split, c.normals_of(mode), rows=True)
    assert sums.tobytes() == want
    assert rows.numpy().tobytes() == want_rows.tobytes()
    # the rows are search_knn(q', 1); without d_rows the record is the same
    import torch
    if nq:
        again = tree.search_knn(torch.from_numpy(np.ascontiguousarray(qp)).to(f"cuda:{gpu}"), 1).numpy()
        assert again.tobytes() == want_rows.tobytes()
    assert device_step(tree, gpu, c.q[:nq], POSE, c.split, c.normals_of(mode)).tobytes() == want
    # the host-buffer form
    hs, hrows = tree.align_step(np.ascontiguousarray(c.q[:nq]), POSE, c.split, c.normals_of(mode), rows=True)
    assert hs.tobytes() == want and hrows.tobytes() == want_rows.tobytes()
    assert tree.align_step(np.ascontiguousarray(c.q[:nq]), POSE, c.split, c.normals_of(mode)).tobytes() == want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_tree_with_piles(gpu, mode):
    """A grid cloud: twenty coincident points per site, subtrees of one point many times over (the k = 1 search runs on
    the view without them)."""
    p = np.ascontiguousarray(np.floor(ds.uniform_cloud(20000, 3, seed=4, scale=10.0)), dtype=np.float32)
    q = np.ascontiguousarray(ds.uniform_cloud(3001, 3, seed=5, scale=10.0) + F32(0.25))
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    assert tree.piles()["piles"] > 0
    host = host_tree(p)
    normals = unit_normals(len(p), 9) if mode == "plane" else None
    want, want_rows = host_step(host, q, POSE, 2.0, normals, rows=True)
    got, rows = device_step(tree, gpu, q, POSE, 2.0, normals, rows=True)
    assert rows.numpy().tobytes() == want_rows.tobytes() and got.tobytes() == want.tobytes()
    assert 0 < got.count < len(q)
    assert tree.align_step(q, POSE, 2.0, normals).tobytes() == want.tobytes()


@pytest.mark.gpu
def test_a_tree_of_the_deep_stack_class(gpu):
    pt.set_test_knobs(pile_view=0)  # (with the view the k = 1 search of this cloud is shallow)
    p, pile = depth_cases.cloud_at_depth(1032, 3, 10)
    p = np.ascontiguousarray(p)
    tree = pt.KdTree(p, pt.Metric.L2Squared, 10, device=gpu)
    depth_cases.assert_depth(tree, 1032)
    assert tree.piles()["piles"] == 0
    q = np.ascontiguousarray(depth_cases.queries(p, pile)[0])
    host = host_tree(p)
    normals = unit_normals(len(p), 10)
    for nm in (None, normals):
        want, want_rows = host_step(host, q, None, INF, nm, rows=True)
        got, rows = device_step(tree, gpu, q, None, INF, nm, rows=True)
        assert rows.numpy().tobytes() == want_rows.tobytes() and got.tobytes() == want.tobytes()
        assert tree.align_step(q, None, INF, nm).tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_batch_pieces_that_are_no_multiple_of_the_block(gpu, mode, monkeypatch):
    c, tree = target(), gpu_target(gpu)
    nq = 4099
    want = host_step(c.tree, c.q[:nq], POSE, c.split, c.normals_of(mode)).tobytes()
    monkeypatch.setenv("PTK_MAX_BATCH", "1000")
    assert device_step(tree, gpu, c.q[:nq], POSE, c.split, c.normals_of(mode)).tobytes() == want
    assert tree.align_step(np.ascontiguousarray(c.q[:nq]), POSE, c.split, c.normals_of(mode)).tobytes() == want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_sorted_and_shuffled_batches_follow_their_own_order(gpu, mode):
    c, tree = target(), gpu_target(gpu)
    base = c.q[:65537]
    by_morton = np.ascontiguousarray(base[ds.morton_order(base)])
    shuffled = np.ascontiguousarray(base[np.random.default_rng(8).permutation(len(base))])
    records = []
    for q in (by_morton, shuffled):
        want = host_step(c.tree, q, POSE, c.split, c.normals_of(mode))
        got = device_step(tree, gpu, q, POSE, c.split, c.normals_of(mode))
        assert got.tobytes() == want.tobytes()
        records.append(got)
    # (the same rows in another order: the same count, and sums that agree to rounding but not to the bit)
    assert records[0].count == records[1].count
    assert records[0].tobytes() != records[1].tobytes()


@pytest.mark.gpu
def test_two_calls_on_two_streams(gpu):
    import torch
    c, tree = target(), gpu_target(gpu)
    nq = 65537
    want = expected("plane", nq)[0]
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    a = device_step(tree, gpu, c.q[:nq], POSE, c.split, c.normals, stream=s1)
    b = device_step(tree, gpu, c.q[:nq], POSE, c.split, c.normals, stream=s2)
    assert a.tobytes() == b.tobytes() == want
    s1.synchronize(), s2.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_every_byte_of_the_record_is_written_and_nothing_past_the_workspace(gpu, mode):
    """The device form with a workspace of exactly the size asked for inside a poisoned buffer, and a poisoned record:
    two fills (0xA5, 0x5A) give the host loop's bytes -- a byte the call left alone would keep its fill --, and the
    guards on either side of both keep theirs."""
    import torch
    c, tree = target(), gpu_target(gpu)
    lib = pt._load()
    dev = f"cuda:{gpu}"
    normals = None if mode == "point" else torch.from_numpy(c.normals).to(dev)
    guard = 4096
    for nq in (0, 257, 65537):
        want = expected(mode, nq)[0]
        dq = torch.from_numpy(np.ascontiguousarray(c.q[:max(nq, 1)])).to(dev)
        need = ctypes.c_uint64()
        assert lib.ptk_align_step_workspace(tree._h, nq, ctypes.byref(need)) == 0
        T = np.ascontiguousarray(POSE)
        for fill in (0xA5, 0x5A):
            ws = torch.full((guard + need.value + guard,), fill, dtype=torch.uint8, device=dev)
            out = torch.full((guard + 384 + guard,), fill, dtype=torch.uint8, device=dev)
            rc = lib.ptk_align_step_device(tree._h, dq.data_ptr(), nq, T.ctypes.data, c.split,
                                           None if normals is None else normals.data_ptr(), out.data_ptr() + guard, None,
                                           ws.data_ptr() + guard if need.value else None, need.value,
                                           torch.cuda.current_stream(dev).cuda_stream)
            assert rc == 0, lib.ptk_last_error()
            torch.cuda.synchronize()
            o, w = out.cpu().numpy(), ws.cpu().numpy()
            assert o[guard:guard + 384].tobytes() == want, (nq, fill)
            assert (o[:guard] == fill).all() and (o[guard + 384:] == fill).all()
            assert (w[:guard] == fill).all() and (w[guard + need.value:] == fill).all()
    # a workspace one byte short: PTK_ERR_INVALID, and the message gives both sizes
    assert lib.ptk_align_step_workspace(tree._h, 257, ctypes.byref(need)) == 0
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
    out = torch.empty((384,), dtype=torch.uint8, device=dev)
    rc = lib.ptk_align_step_device(tree._h, dq.data_ptr(), 257, None, F32(1), None, out.data_ptr(), None, ws.data_ptr(),
                                   need.value - 1, None)
    why = lib.ptk_last_error().decode()
    assert rc == INVALID and str(need.value) in why and str(need.value - 1) in why
    assert lib.ptk_align_step_device(tree._h, dq.data_ptr(), 257, None, F32(1), None, out.data_ptr(), None, None,
                                     need.value, None) == INVALID
    assert lib.ptk_align_step_device(tree._h, None, 257, None, F32(1), None, out.data_ptr(), None, ws.data_ptr(),
                                     need.value, None) == INVALID
    assert lib.ptk_align_step_device(tree._h, dq.data_ptr(), 257, None, F32(1), None, None, None, ws.data_ptr(),
                                     need.value, None) == INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_icp_driven_by_the_device_and_by_the_host_loop(gpu, mode):
    import torch
    c, tree = target(), gpu_target(gpu)
    M = rigid(0.01, [0.1, 0.2, 1.0], [0.15, -0.1, 0.05])
    sel = separated_subset(c, 0.3)
    inv = np.linalg.inv(M)
    q = np.ascontiguousarray((c.p[sel].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    normals = c.normals_of(mode)
    dq = torch.from_numpy(q).to(f"cuda:{gpu}")
    dn = None if normals is None else torch.from_numpy(normals).to(f"cuda:{gpu}")
    on_device = pt.icp(tree, dq, 4.0, normals=dn, iterations=6, min_delta=0.0)
    on_host = pt.icp(c.tree, q, 4.0, iterations=6, min_delta=0.0, step=lambda T: host_step(c.tree, q, T, 4.0, normals))
    assert on_device.iterations == on_host.iterations == 6
    for a, b in zip(on_device.poses, on_host.poses):
        assert a.tobytes() == b.tobytes()
    assert on_device.rms == on_host.rms and on_device.rms[-1] < on_device.rms[0]
    assert torch.equal(dq.cpu(), torch.from_numpy(q))
    by_host_form = pt.icp(tree, q, 4.0, normals=normals, iterations=6, min_delta=0.0)
    assert by_host_form.transform.tobytes() == on_device.transform.tobytes()


@pytest.mark.gpu
def test_cpp_member_through_the_backend(gpu, tmp_path):
    exe = str(tmp_path / "align_backend")
    _cpp_program(exe, host_only=False)
    check_cpp(exe, str(tmp_path), 65537)
