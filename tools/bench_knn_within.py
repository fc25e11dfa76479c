#!/usr/bin/env python3
"""search_knn_within against search_knn and the radius search on the LiDAR clouds of BASELINE configs 2 and 3
(7.73 M points, 7.20 M queries, one MI355X, device buffers).

For k = 1 and k = 16 at r in {0.25, 1.0, 4.0} (metric units: squared radii): device-event milliseconds per call
(warmed; median, min and max of the steps), the fraction of filled slots; beside them search_knn of the same k and
the radius search (count pass + scan + fill pass, the device forms) with its hits per query.  Writes
profiles/knn_within_bench.json (or the path given with --out) and prints it.

  python tools/bench_knn_within.py [--steps N] [--out PATH] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup=2):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3)}


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_within_bench.json"))
    ap.add_argument("--quick", action="store_true", help="one radius and k = 16 only (a profiler run)")
    args = ap.parse_args()

    pts, q = ds.config2_clouds("L")
    nq = len(q)
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
    dq = torch.from_numpy(q).cuda()
    rows = []
    ks = (16,) if args.quick else (1, 16)
    rs = (1.0,) if args.quick else (0.25, 1.0, 4.0)
    for k in ks:
        out = torch.empty((nq, k, 2), dtype=torch.int32, device="cuda")
        knn = timed(lambda: tree.search_knn(dq, k, out), args.steps)
        for r in rs:
            within = timed(lambda: tree.search_knn_within(dq, k, r, out), args.steps)
            filled = float((out[..., 0] >= 0).float().mean().item())
            row = {"k": k, "r": r, "nq": nq, "knn_within": within, "filled_frac": round(filled, 4), "knn": knn}
            if not args.quick:
                holder = {}

                def radius():
                    holder["res"] = tree.search_radius_device(dq, r)

                row["radius"] = timed(radius, args.steps)
                offsets = holder.pop("res")[0]
                row["radius_hits_per_query"] = round(float(offsets[-1].item()) / nq, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del out
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L", "steps": args.steps, "rows": rows}
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
