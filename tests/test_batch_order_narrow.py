"""The block passes of the batch order on narrow streams (pico_tree_amd/csrc/ptk_sort.hpp: radix_key_hist_kernel,
radix_digit_hist_kernel, radix_narrow_scatter_kernel).

The permutation must be exactly the one a stable sort of the order keys gives.  The CPU tier runs the kernels' source
lane by lane (tests/cpp/emulate_batch_order_narrow.cpp, the pass loop of make_permutation) against
``numpy.argsort(keys, kind="stable")``; the gpu tier compares the device's order with the new passes on (the default)
against the passes of r04 forced through the test hook ``sort_block=1``, and the k = 1 rows of the two.
"""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import pico_tree_amd as pt
from pico_tree_amd import datasets as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096

# sort_narrow: 1 = digit stream, + 2 = packed 4-byte items into the last pass, + 4 = the key kernel's rows through LDS
ALL = 7
WIDE_ITEMS = 5  # the layout of a batch above 2^24 rows: 8-byte pairs all the way
BITS = {(3, 16): (6, 5, 5), (3, 24): (8, 8, 8), (2, 16): (8, 8, 0), (2, 24): (12, 12, 0)}


@pytest.fixture(scope="module")
def emu_narrow(tmp_path_factory):
    """tests/cpp/emulate_batch_order_narrow.cpp, compiled with the emulator's g++ line and HIP stand-in."""
    out = str(tmp_path_factory.mktemp("emu_narrow") / "libptk_emu_narrow.so")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w",
        "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "emulate_batch_order_narrow.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_radix_sort_narrow.restype = ctypes.c_int
    lib.emu_radix_sort_narrow.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_morton.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def rows_at(q, offset_bytes):
    """A copy of the rows of `q` whose first byte lies `offset_bytes` past a 16-byte boundary."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    raw = np.zeros(q.nbytes + 64, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + offset_bytes
    out = raw[start:start + q.nbytes].view(np.float32).reshape(q.shape)
    out[...] = q
    assert out.ctypes.data % 16 == offset_bytes % 16
    return out


def grid_of(q, bits):
    """lo, inv of the key grid over the box of the rows (as make_permutation derives them from the root box)."""
    d = q.shape[1]
    lo = np.zeros(3, dtype=np.float32)
    inv = np.zeros(3, dtype=np.float32)
    lo[:d] = q.min(0)
    ext = (q.max(0) - q.min(0)).astype(np.float32)
    b = np.asarray(bits, dtype=np.uint32)
    inv[:d] = np.where(ext > 0, np.exp2(b[:d]).astype(np.float32) / np.where(ext > 0, ext, 1), 0).astype(np.float32)
    return lo, inv, b


def run(lib, q, bits, narrow):
    """(permutation, keys, rows went through LDS) of the emulated passes; the keys also checked against morton_kernel."""
    nq, d = q.shape
    lo, inv, b = grid_of(q, bits)
    keys = np.zeros(nq, dtype=np.uint32)
    perm = np.zeros(nq, dtype=np.uint32)
    rc = lib.emu_radix_sort_narrow(q.ctypes.data, d, nq, lo.ctypes.data, inv.ctypes.data, b.ctypes.data, int(b.sum()),
                                   narrow, keys.ctypes.data, perm.ctypes.data)
    assert rc >= 0
    want_keys = np.zeros(nq, dtype=np.uint32)
    ids = np.zeros(nq, dtype=np.uint32)
    lib.emu_morton(q.ctypes.data, d, nq, lo.ctypes.data, inv.ctypes.data, b.ctypes.data, want_keys.ctypes.data,
                   ids.ctypes.data)
    assert np.array_equal(keys, want_keys)
    return perm, keys, rc == 1


def check(lib, q, bits, narrow, staged):
    perm, keys, went_staged = run(lib, q, bits, narrow)
    assert went_staged == staged
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32))
    return keys


@pytest.mark.parametrize("dim,key_bits", sorted(BITS))
@pytest.mark.parametrize("nq", [4_095, 4_096, 4_097, 8_193, 3 * 4_096 + 17])
def test_emulated_passes_give_the_stable_sort(emu_narrow, nq, dim, key_bits):
    """Every size around a tile and its last, partly filled one; 16-bit keys (two passes: keys -> packed -> rows) and
    24-bit keys (keys -> pairs -> packed -> rows); dim 3 takes its rows through LDS, dim 2 keeps load_query."""
    q = rows_at(ds.uniform_cloud(nq, dim, 100 + nq % 97 + dim), 0)
    keys = check(emu_narrow, q, BITS[dim, key_bits], ALL, staged=dim == 3)
    assert int(keys.max()) >> (key_bits - 8) == 255 and len(np.unique(keys)) > nq // 40  # (the keys use their width)


@pytest.mark.parametrize("narrow", [ALL, WIDE_ITEMS])
@pytest.mark.parametrize("key_bits", [16, 24])
def test_emulated_passes_on_equal_keys_and_on_every_top_digit(emu_narrow, key_bits, narrow):
    """One point 4 113 times: every key equal, one digit run per pass, the order is the identity.  A lattice that puts
    rows into all 256 values of the top digit, first in descending key order: every pass moves every row.
    WIDE_ITEMS is the item layout of a batch above 2^24 rows (8-byte pairs into the last pass) forced at a small size."""
    bits = BITS[3, key_bits]
    same = rows_at(np.tile(np.array([[0.25, -3.0, 7.5]], dtype=np.float32), (TILE + 17, 1)), 0)
    perm, keys, _ = run(emu_narrow, same, bits, narrow)
    assert len(np.unique(keys)) == 1 and np.array_equal(perm, np.arange(len(same), dtype=np.uint32))
    g = (np.arange(16, dtype=np.float32) + 0.5) / 16
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)  # 4 096 rows
    corners = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.float32)
    lattice = rows_at(np.concatenate([corners, cells[::-1], cells[:37], cells]), 0)
    keys = check(emu_narrow, lattice, bits, narrow, staged=True)
    assert len(np.unique(keys >> (key_bits - 8))) == 256


@pytest.mark.parametrize("offset_rows,staged", [(0, True), (1, False), (4, True)])
@pytest.mark.parametrize("key_bits", [16, 24])
def test_emulated_passes_from_a_view_at_a_row_offset(emu_narrow, key_bits, offset_rows, staged):
    """The rows of a view that begins `offset_rows` rows into a 16-byte aligned buffer: one row further the base is 12
    bytes past the boundary and the key kernel keeps load_query; four rows further it is aligned again.  The last tile
    is partly filled either way, and the buffer ends with the batch (nothing past the last row is the batch's)."""
    whole = rows_at(ds.uniform_cloud(2 * TILE + 301 + offset_rows, 3, 7), 0)
    q = whole[offset_rows:]
    assert (q.ctypes.data % 16 == 0) == staged
    check(emu_narrow, q, BITS[3, key_bits], ALL, staged)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dim,key_bits", sorted(BITS))
def test_emulated_keys_with_a_cell_table(emu_narrow, dim, key_bits, mode):
    """The key kernel computes the keys of a thread's eight rows side by side (order_keys); with a table of cell classes
    (mode 1 = kCellsEmptyFirst: k nearest neighbours, 2 = kCellsDenseFirst: radius search) they are the keys order_key
    gives row by row in morton_kernel -- every class byte 0 .. 13 in the table, a last tile that is partly filled."""
    q = rows_at(ds.uniform_cloud(TILE + 333, dim, 21), 0)
    lo, inv, b = grid_of(q, BITS[dim, key_bits])
    cell_bits = np.array([3, 2, 2] if dim == 3 else [4, 3, 0], dtype=np.uint32)
    _, cell_inv, _ = grid_of(q, cell_bits)
    occ = (np.arange(1 << int(cell_bits.sum()), dtype=np.uint32) * 5 % 14).astype(np.uint8)
    tile, row = np.zeros(len(q), dtype=np.uint32), np.zeros(len(q), dtype=np.uint32)
    fn = emu_narrow.emu_keys_with_cells
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + \
                  [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 2
    fn(q.ctypes.data, dim, len(q), lo.ctypes.data, inv.ctypes.data, b.ctypes.data, key_bits, occ.ctypes.data,
       cell_inv.ctypes.data, cell_bits.ctypes.data, mode, tile.ctypes.data, row.ctypes.data)
    assert np.array_equal(tile, row)
    assert len(np.unique(row >> (key_bits - mode))) == 2 * mode  # (the class bits are in the keys)


# ---- gpu tier ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device_tree(gpu):
    return pt.KdTree(ds.uniform_cloud(60_000, 3, 11), pt.Metric.L2Squared, 10, device=gpu)


def _queries(kind, nq):
    q = ds.uniform_cloud(nq, 3, 12)
    return q if kind == "uniform" else (np.round(q * 10) / 10).astype(np.float32)  # a lattice: 11^3 distinct rows


def _orders(tree, dq):
    """The batch order of the device rows `dq`: (narrow passes -- the default --, the r04 block passes)."""
    pt.set_test_knobs()
    new = tree.batch_permutation(dq).cpu().numpy()
    pt.set_test_knobs(sort_block=1)
    try:
        old = tree.batch_permutation(dq).cpu().numpy()
    finally:
        pt.set_test_knobs()
    return new, old


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "lattice"])
@pytest.mark.parametrize("nq", [786_432, 786_433, 1_048_576, 1_048_577])
def test_device_order_equals_the_r04_block_passes(gpu, device_tree, nq, kind):
    """Where the block form begins (16-bit keys: keys -> packed -> rows), one row more, where the keys become 24 bits
    (keys -> pairs -> packed -> rows), one row more."""
    import torch

    dq = torch.from_numpy(_queries(kind, nq)).to(f"cuda:{gpu}")
    new, old = _orders(device_tree, dq)
    assert np.array_equal(np.sort(new[:: nq // 4096]), np.unique(new[:: nq // 4096])) and int(new.max()) == nq - 1
    assert np.array_equal(new, old)


@pytest.mark.gpu
def test_device_order_of_a_view_and_of_wide_items(gpu, device_tree):
    """A torch view one row into its buffer (not 16-byte aligned: load_query) and four rows in (aligned: through LDS);
    the item layout of a batch above 2^24 rows (sort_narrow=5: no packed items) at a size that fits a test."""
    import torch

    nq = 1_048_577
    whole = torch.from_numpy(_queries("uniform", nq + 4)).to(f"cuda:{gpu}")
    for first in (1, 4):
        dq = whole[first:first + nq]
        assert (dq.data_ptr() % 16 == 0) == (first == 4)
        new, old = _orders(device_tree, dq)
        assert np.array_equal(new, old)
    pt.set_test_knobs(sort_narrow=WIDE_ITEMS)
    wide = device_tree.batch_permutation(whole[:nq]).cpu().numpy()
    pt.set_test_knobs()
    assert np.array_equal(wide, _orders(device_tree, whole[:nq])[1])


@pytest.mark.gpu
def test_device_knn1_rows_equal_between_the_two_forms(gpu, device_tree):
    import torch

    dq = torch.from_numpy(_queries("uniform", 1_048_577)).to(f"cuda:{gpu}")
    new = device_tree.search_knn(dq, 1).numpy()
    pt.set_test_knobs(sort_block=1)
    old = device_tree.search_knn(dq, 1).numpy()
    pt.set_test_knobs()
    assert new.tobytes() == old.tobytes()
