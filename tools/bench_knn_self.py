#!/usr/bin/env python3
"""search_knn_self on cloud L (BASELINE config 2's tree points): the direct kernel against the staged route and against
what a caller could do without the call (one MI355X, device buffers).

For each tree size (7.73 M points; 150 k points, every 51st of them) and k in {1, 7, 15, 16}, three forms:

  direct   search_knn_self through knn_self_kernel
  staged   search_knn_self through the staged route (test hook self_route = 2)
  caller   search_knn of a device copy of the tree's points with k + 1 -- the call a user had before; stripping the
           point itself from the rows is NOT counted

Milliseconds per call, host clock around the call and a device synchronisation (the staged route allocates and waits, so
device events alone would flatter it); `reps` repetitions with the forms alternating, after one warm-up round; median,
min and max per form, and the run-to-run spread of `caller`, (max - min) / median.  Writes
profiles/knn_self_bench.json (or the path given with --out) and prints each row.

  python tools/bench_knn_self.py [--reps N] [--out PATH] [--small-only]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_self_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="the 150 k tree only (a quick look)")
    args = ap.parse_args()

    full, _ = ds.config2_clouds("L", nq=1)
    clouds = [("150k", np.ascontiguousarray(full[::51][:150_000]))]
    if not args.small_only:
        clouds.insert(0, ("7.73M", full))
    rows = []
    for name, pts in clouds:
        n = len(pts)
        tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
        dp = torch.from_numpy(pts).cuda()
        for k in (1, 7, 15, 16):
            out = torch.empty((n, k, 2), dtype=torch.int32, device="cuda")
            out1 = torch.empty((n, k + 1, 2), dtype=torch.int32, device="cuda")

            def direct():
                pt.set_test_knobs(self_route=None)
                tree.search_knn_self(k, out)

            def staged():
                pt.set_test_knobs(self_route=2)
                tree.search_knn_self(k, out)
                pt.set_test_knobs(self_route=None)

            def caller():
                tree.search_knn(dp, k + 1, out1)

            assert tree.self_route(k) == 1
            forms = (("direct", direct), ("staged", staged), ("caller", caller))
            ms = {f: [] for f, _ in forms}
            for rep in range(args.reps + 1):  # (round 0 warms every form up)
                for f, fn in forms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep > 0:
                        ms[f].append((time.perf_counter() - t0) * 1e3)
            row = {"tree": name, "n_points": n, "k": k, **{f: stats(v) for f, v in ms.items()}}
            c = row["caller"]
            row["caller_spread"] = round((c["max_ms"] - c["min_ms"]) / c["median_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out, out1
        del tree, dp
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
