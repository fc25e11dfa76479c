#!/usr/bin/env python3
"""count_within_self / search_radius_self on cloud L (BASELINE config 2's tree points) against what a caller could do
without them (one MI355X, device buffers).

For each tree size (7.73 M points; 150 k points, every 51st of them) and r in {0.25, 1.0, 4.0} (metric units: squared
radii, the three of profiles/count_within_bench.json), four forms:

  self_count     ptk_search_count_within_self_device (scalar radius, max_count = 0)
  caller_count   ptk_search_count_within_device on a device copy of the tree's points in their original order -- the call
                 a user had before; subtracting one from every count is NOT counted
  self_rows      the self count, torch.cumsum and ptk_search_radius_self_fill_device
  caller_rows    ptk_search_count_within_radii_device with a constant radii array on the same query buffer, torch.cumsum
                 and ptk_search_radius_radii_fill_device -- the only count / fill pair of the library that leaves the
                 handle's capture alone, as the self form does; stripping the own entry from every row is NOT counted

Milliseconds per call, host clock around the call and a device synchronisation; `reps` repetitions with the forms
alternating, after one warm-up round; median, min and max per form, the ratio self / caller of the medians and the
run-to-run spread of the caller's form, (max - min) / median.  The trees are built from their own points, so every
point is in its own row: the tool asserts counts == caller's counts - 1 before it times anything.  Writes
profiles/radius_self_bench.json (or the path given with --out) and prints each row.

  python tools/bench_radius_self.py [--reps N] [--out PATH] [--small-only]
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


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_self_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="the 150 k tree only (a quick look)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_radius_self.py needs a GPU")

    lib = pt._load()
    full, _ = ds.config2_clouds("L", nq=1)
    clouds = [("150k", np.ascontiguousarray(full[::51][:150_000]))]
    if not args.small_only:
        clouds.insert(0, ("7.73M", full))
    rows = []
    for name, pts in clouds:
        n = len(pts)
        tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
        dp = torch.from_numpy(pts).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        counts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        counts_c = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        for r in (0.25, 1.0, 4.0):
            rr = np.float32(r)
            radii = torch.full((n,), float(r), dtype=torch.float32, device="cuda")

            def self_count():
                assert lib.ptk_search_count_within_self_device(tree._h, rr, None, 0, counts.data_ptr(), stream) == 0

            def caller_count():
                assert lib.ptk_search_count_within_device(tree._h, dp.data_ptr(), n, rr, 0, counts_c.data_ptr(), stream) == 0

            # (the first calls: the side table, the warm-up of every kernel; the check that both forms count the same)
            self_count()
            caller_count()
            torch.cuda.synchronize()
            assert torch.equal(counts[:n] + 1, counts_c[:n]), "self counts are not the caller's counts minus one"
            total_self = int(counts[:n].sum().item())
            total_caller = int(counts_c[:n].sum().item())
            out = torch.empty((max(total_caller, 1), 2), dtype=torch.int32, device="cuda")

            def self_rows():
                self_count()
                offsets[1:] = torch.cumsum(counts[:n], 0)
                assert lib.ptk_search_radius_self_fill_device(tree._h, rr, None, offsets.data_ptr(), out.data_ptr(), 0,
                                                              stream) == 0

            def caller_rows():
                assert lib.ptk_search_count_within_radii_device(tree._h, dp.data_ptr(), n, radii.data_ptr(), 0,
                                                                counts_c.data_ptr(), stream) == 0
                offsets[1:] = torch.cumsum(counts_c[:n], 0)
                assert lib.ptk_search_radius_radii_fill_device(tree._h, dp.data_ptr(), n, radii.data_ptr(),
                                                               offsets.data_ptr(), out.data_ptr(), 0, stream) == 0

            forms = (("self_count", self_count), ("caller_count", caller_count), ("self_rows", self_rows),
                     ("caller_rows", caller_rows))
            ms = {f: [] for f, _ in forms}
            for rep in range(args.reps + 1):  # (round 0 warms every form up)
                for f, fn in forms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep > 0:
                        ms[f].append((time.perf_counter() - t0) * 1e3)
            row = {"tree": name, "n_points": n, "r": r, "neighbours_per_point": round(total_self / n, 2),
                   **{f: stats(v) for f, v in ms.items()}}
            for what in ("count", "rows"):
                s, c = row["self_" + what], row["caller_" + what]
                row[what + "_self_over_caller"] = round(s["median_ms"] / c["median_ms"], 3)
                row["caller_" + what + "_spread"] = round((c["max_ms"] - c["min_ms"]) / c["median_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out, radii
        del tree, dp, counts, counts_c, offsets
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps,
           "clock": "host clock around the call and a device synchronisation", "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
