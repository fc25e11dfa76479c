#!/usr/bin/env python3
"""normals_within_self on cloud L (BASELINE config 2's tree points) against the rows route a caller had before (one
MI355X, device buffers).

The radius is the median 8th-neighbour distance of the cloud (search_knn_self(8)) and 4 x it (metric units: squared
radii).  Forms:

  frames            ptk_normals_within_self_device, frames only
  frames_moments    ... frames and moments
  rows_route        ptk_search_count_within_self_device (max_count = 0), torch.cumsum and
                    ptk_search_radius_self_fill_device at the same radius: the rows a caller would then gather points by
                    and feed to an eigen-solver -- no covariance work is counted
  fill_only         ptk_search_radius_self_fill_device alone, on the offsets of the rows route

Milliseconds per call, host clock around the call and a device synchronisation; `reps` repetitions with the forms
alternating, after one warm-up round; median, min and max per form, the ratios of the medians and the run-to-run spread
of the rows route, (max - min) / median.  Also the largest eigen-residual |C n - l0 n| / |C|_F of the frames on a sample
of rows beside the one numpy's float32 eigh leaves on the same matrices (C from the moments, residuals in float64).
Writes profiles/frames_self_bench.json (or the path given with --out) and prints each row.

  python tools/bench_frames_self.py [--reps N] [--out PATH] [--small-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = np.array(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3)}


def residuals(frames, moments):
    """(largest relative residual of the frames, of numpy's float32 eigh) over the rows that have a frame."""
    ok = np.isfinite(frames["curvature"])
    f, m = frames[ok], moments[ok]
    inv = np.float32(1) / (m["count"].astype(np.float32) + np.float32(1))
    mean = m["sum"] * inv[:, None]
    c = np.empty((len(m), 3, 3), dtype=np.float32)
    for k, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        c[:, a, b] = c[:, b, a] = m["outer"][:, k] * inv - mean[:, a] * mean[:, b]
    c64 = c.astype(np.float64)
    norm = np.sqrt((c64 ** 2).sum((1, 2)))
    some = norm > 0
    n64, l0 = f["normal"].astype(np.float64), f["eigenvalues"][:, 0].astype(np.float64)
    mine = np.linalg.norm(np.einsum("nij,nj->ni", c64, n64) - l0[:, None] * n64, axis=1)
    w, v = np.linalg.eigh(c)
    v64 = v.astype(np.float64)
    theirs = np.linalg.norm(np.einsum("nij,njk->nik", c64, v64) - v64 * w.astype(np.float64)[:, None, :], axis=1).max(1)
    return float((mine[some] / norm[some]).max(initial=0.0)), float((theirs[some] / norm[some]).max(initial=0.0)), int(ok.sum())


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_self_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="150 k points only (a quick look)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_self.py needs a GPU")

    lib = pt._load()
    full, _ = ds.config2_clouds("L", nq=1)
    name, pts = ("150k", np.ascontiguousarray(full[::51][:150_000])) if args.small_only else ("7.73M", full)
    n = len(pts)
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    med = np.float32(np.median(tree.search_knn_self(8)["distance"][:, 7]))
    frames = torch.empty((n, pt.FRAME.itemsize), dtype=torch.uint8, device="cuda")
    moments = torch.empty((n, pt.MOMENTS.itemsize), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rows = []
    for mult in (1, 4):
        rr = np.float32(mult) * med

        def normals(with_moments):
            def call():
                assert lib.ptk_normals_within_self_device(tree._h, rr, None, 2, None, frames.data_ptr(),
                                                          moments.data_ptr() if with_moments else None, stream) == 0
            return call

        def count():
            assert lib.ptk_search_count_within_self_device(tree._h, rr, None, 0, counts.data_ptr(), stream) == 0

        count()
        torch.cuda.synchronize()
        total = int(counts[:n].sum().item())
        out = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")

        def fill_only():
            assert lib.ptk_search_radius_self_fill_device(tree._h, rr, None, offsets.data_ptr(), out.data_ptr(), 0,
                                                          stream) == 0

        def rows_route():
            count()
            offsets[1:] = torch.cumsum(counts[:n], 0)
            fill_only()

        rows_route()  # (the offsets fill_only reads)
        forms = (("frames", normals(False)), ("frames_moments", normals(True)), ("rows_route", rows_route),
                 ("fill_only", fill_only))
        ms = {f: [] for f, _ in forms}
        for rep in range(args.reps + 1):  # (round 0 warms every form up)
            for f, fn in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep > 0:
                    ms[f].append((time.perf_counter() - t0) * 1e3)
        row = {"tree": name, "n_points": n, "r": float(rr), "r_over_median_8th": mult,
               "neighbours_per_point": round(total / n, 2), **{f: stats(v) for f, v in ms.items()}}
        base, fill = row["rows_route"], row["fill_only"]
        for f in ("frames", "frames_moments"):
            row[f + "_over_rows_route"] = round(row[f]["median_ms"] / base["median_ms"], 3)
            row[f + "_over_fill_only"] = round(row[f]["median_ms"] / fill["median_ms"], 3)
        row["rows_route_spread"] = round((base["max_ms"] - base["min_ms"]) / base["median_ms"], 3)
        # the counts of the frames are those of the count pass, and the residuals on every 40th row
        normals(True)()
        torch.cuda.synchronize()
        fr = np.ascontiguousarray(frames.cpu().numpy()).view(pt.FRAME).reshape(-1)
        mo = np.ascontiguousarray(moments.cpu().numpy()).view(pt.MOMENTS).reshape(-1)
        assert np.array_equal(fr["count"], counts[:n].cpu().numpy()), "counts differ from count_within_self"
        step = 1 if n <= 200_000 else 40
        mine, theirs, sampled = residuals(fr[::step], mo[::step])
        row["residual_over_frobenius"] = {"jacobi_6_sweeps": mine, "numpy_eigh_float32": theirs, "rows": sampled}
        row["rows_with_a_frame"] = int(np.isfinite(fr["curvature"]).sum())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps,
           "clock": "host clock around the call and a device synchronisation", "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
