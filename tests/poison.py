"""Query batches with non-finite and overflowing rows, and what the reference makes of them -- shared by the CPU and
the GPU tier of tests/test_non_finite.py.  TEST INFRASTRUCTURE (a plain module, not a conftest).

The contract under test (include/ptk.h, "Non-finite and overflowing inputs"):

* a query row with NaN, +-Inf or any finite value gets what the reference gives it, for every entry the reference
  writes; no row changes another row's result;
* a k-NN slot the reference's search never writes holds ``{index 0, distance MAX}`` (padding zero for double).

`poison()` makes the batch, `written_by_reference()` finds out which entries the reference writes (two runs into
buffers prefilled with different bytes: an entry both runs agree on was written), `expect_rows()` substitutes the
documented filler for the rest.  The comparison is then byte for byte on the whole batch: nothing is masked out.
"""

from __future__ import annotations

import numpy as np

#: Rows `poison()` adds to the drawn share: a whole wavefront in caller order, row 0 and the last row.
EXTRA_ROWS = 66


def palette(dtype) -> np.ndarray:
    """NaN, +-Inf, +-MAX, +-0.8 sqrt(MAX), 0.1 sqrt(MAX) of `dtype`.  The last three are finite and so is their squared
    distance to any ordinary point: such rows have a full, huge-valued, defined k-list -- they drive huge bit patterns
    through the bounds the lanes of a wavefront share."""
    dtype = np.dtype(dtype)
    mx = np.finfo(dtype).max
    root = np.sqrt(mx, dtype=dtype)
    return np.array([np.nan, np.inf, -np.inf, mx, -mx, dtype.type(0.8) * root, dtype.type(-0.8) * root,
                     dtype.type(0.1) * root], dtype=dtype)


def poison(q: np.ndarray, seed: int, share: float = 0.05):
    """A copy of `q` with one coordinate of `share` of the rows (drawn at random), of one run of 64 consecutive rows
    starting at a multiple of 64, of row 0 and of the last row replaced by a value drawn from `palette()`.
    Returns (batch, mask of the poisoned rows)."""
    q = np.array(q, copy=True, order="C")
    n, dim = q.shape
    rng = np.random.default_rng(seed)
    mask = np.zeros(n, dtype=bool)
    mask[rng.choice(n, int(round(share * n)), replace=False)] = True
    if n >= 64:
        start = 64 * int(rng.integers(0, n // 64))
        mask[start:start + 64] = True
    mask[0] = mask[n - 1] = True
    rows = np.flatnonzero(mask)
    pal = palette(q.dtype)
    # (every value of the palette at least once where the rows allow it, the rest drawn)
    vals = pal[rng.integers(0, len(pal), len(rows))]
    if len(rows) >= len(pal):
        vals[rng.choice(len(rows), len(pal), replace=False)] = pal
    q[rows, rng.integers(0, dim, len(rows))] = vals
    assert mask.sum() <= int(round(share * n)) + EXTRA_ROWS
    return q, mask


def poison_corners(lo: np.ndarray, hi: np.ndarray, seed: int, share: float = 0.05):
    """Box corners poisoned per side: (lo', hi', mask) -- a poisoned box has one coordinate of its min corner OR of its
    max corner replaced (`poison()` on each side with half the share, so some boxes get both)."""
    lo2, m_lo = poison(lo, seed, share / 2)
    hi2, m_hi = poison(hi, seed + 1, share / 2)
    return lo2, hi2, m_lo | m_hi


def filler(neighbor_dtype) -> tuple:
    """(index, distance) of a k-NN slot no search wrote."""
    return 0, np.finfo(np.dtype(neighbor_dtype)["distance"]).max


def written_by_reference(ref, q: np.ndarray, k: int, mask: np.ndarray | None = None, share: float = 0.05,
                         e: float | None = None):
    """The compiled reference's search_knn rows of `q` and which of their entries it WROTE: (rows, written), `written`
    a bool array (nq, k, 2) over {index, distance}.  The search runs twice into buffers prefilled with two different
    byte patterns; where both runs agree the entry was written (0xA5A5A5A5 / 0x5A5A5A5A are no index of a tree, and as
    floating-point numbers the one is negative and the other is not the other's value).

    Asserts, on the reference alone, what keeps a comparison through `expect_rows()` from hiding a failure: every
    entry of a clean row is written; the poisoned rows are at most `share` of the batch + 66; at least a quarter of
    them is fully written (the finite members of the palette)."""
    assert ref.kind == "reference"
    q = np.ascontiguousarray(q, dtype=ref.dtype)
    runs = []
    for byte in (0xA5, 0x5A):
        out = np.empty((len(q), k), dtype=ref.neighbor)
        out.view(np.uint8).reshape(-1)[:] = byte
        runs.append(ref.search_knn(q, k, e=e, out=out))
    a, b = runs
    written = np.empty((len(q), k, 2), dtype=bool)
    for f, name in enumerate(("index", "distance")):
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        raw = np.dtype(f"u{x.dtype.itemsize}")
        written[:, :, f] = x.view(raw) == y.view(raw)
    full = written.all(axis=(1, 2))
    if mask is None:
        assert full.all(), "the reference left entries of a clean batch unwritten"
    else:
        assert full[~mask].all(), "the reference left entries of a clean row unwritten"
        assert mask.sum() <= int(round(share * len(q))) + EXTRA_ROWS
        assert 4 * int(full[mask].sum()) >= int(mask.sum()), (int(full[mask].sum()), int(mask.sum()))
    return a, written


def expect_rows(rows: np.ndarray, written: np.ndarray) -> np.ndarray:
    """The rows the library must give: the reference's entry where it wrote one, the documented filler elsewhere
    (padding bytes of the double record zero)."""
    want = np.zeros(rows.shape, dtype=rows.dtype)
    idx, dist = filler(rows.dtype)
    want["index"] = np.where(written[:, :, 0], rows["index"], idx)
    want["distance"] = np.where(written[:, :, 1], rows["distance"], dist)
    return want


def record_bytes(a: np.ndarray) -> np.ndarray:
    """The records of `a` as they lie in memory, padding included: uint8 (records, itemsize).  (numpy copies a
    structured array with padding field by field and leaves the padding of the copy as it finds it, so a strided view
    -- `DeviceNeighbors.numpy()` -- is copied as opaque records here.)"""
    a = np.asarray(a)
    opaque = np.ascontiguousarray(a.view(np.dtype((np.void, a.dtype.itemsize))))
    return opaque.view(np.uint8).reshape(-1, a.dtype.itemsize)


def same_rows(got: np.ndarray, want: np.ndarray) -> bool:
    """Byte equality of two row arrays of one neighbor dtype (index, padding and the bits of every distance)."""
    return got.dtype == want.dtype and got.size == want.size and np.array_equal(record_bytes(got), record_bytes(want))


def first_difference(got: np.ndarray, want: np.ndarray, mask: np.ndarray | None = None) -> str:
    """For an assertion message: the first row that differs."""
    if got.size != want.size:
        return f"shapes {got.shape} and {want.shape}"
    g, w = record_bytes(got).reshape(len(want), -1), record_bytes(want).reshape(len(want), -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    if len(bad) == 0:
        return "no difference"
    i = int(bad[0])
    got, want = np.asarray(got).reshape(len(want), -1), np.asarray(want).reshape(len(want), -1)
    clean = "" if mask is None else f", {int((~mask[bad]).sum())} of them clean rows"
    return f"{len(bad)} rows differ{clean}; first: row {i}: got {got[i]!r}, want {want[i]!r}"
