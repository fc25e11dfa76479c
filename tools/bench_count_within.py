#!/usr/bin/env python3
"""count_within against the radius count pass on the LiDAR clouds of BASELINE config 3 (7.73 M points, 7.20 M
queries, cloud L, one MI355X, device buffers).

At r in {0.25, 1.0, 4.0} (metric units: squared radii), in one process with the forms ALTERNATING repetition by
repetition: ptk_search_radius_count_device, count_within, count_within with the test knob count_shortcut=0 (both
shortcuts off), count_within with max_count = 16; and the float64 tree at r = 1.0 (count_within only).  Device-event
milliseconds per call (median, min and max of the repetitions), the mean count per query, whether every form gave the
radius count pass's counts (clamped for max_count), and the side table's build time and size.  Writes
profiles/count_within_bench.json (or --out) and prints it.

  python tools/bench_count_within.py [--reps N] [--out PATH] [--quick]
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


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    ms = np.array(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3), "reps": len(ms)}


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_within_bench.json"))
    ap.add_argument("--quick", action="store_true", help="r = 1.0, count_within only (a profiler run)")
    args = ap.parse_args()

    lib = pt._load()
    pts, q = ds.config2_clouds("L")
    nq = len(q)
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
    dq = torch.from_numpy(q).cuda()
    info0 = tree.info()["device_bytes"] if hasattr(tree, "info") else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = tree.count_within(dq[:64], 1.0)  # (the first count on the handle builds the side table)
    torch.cuda.synchronize()
    table_ms = (time.perf_counter() - t0) * 1e3
    info1 = tree.info()["device_bytes"] if hasattr(tree, "info") else None
    del first
    stream = torch.cuda.current_stream().cuda_stream
    counts = torch.empty(nq, dtype=torch.int64, device="cuda")

    def radius_count(r):
        assert lib.ptk_search_radius_count_device(tree._h, dq.data_ptr(), nq, np.float32(r), np.float32(1.0),
                                                  counts.data_ptr(), stream) == 0

    def knob(on):
        if on:
            os.environ["PTK_TEST_KNOBS"] = "count_shortcut=0"
        else:
            os.environ.pop("PTK_TEST_KNOBS", None)

    rows = []
    for r in ((1.0,) if args.quick else (0.25, 1.0, 4.0)):
        forms = {
            "radius_count_device": lambda: radius_count(r),
            "count_within": lambda: tree.count_within(dq, r),
        }
        if not args.quick:
            forms["count_within_shortcut_off"] = lambda: (knob(True), tree.count_within(dq, r), knob(False))
            forms["count_within_max16"] = lambda: tree.count_within(dq, r, 16)
        for fn in forms.values():  # warm-up
            fn()
        ms = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, fn in forms.items():
                ms[name].append(event_ms(fn))
        radius_count(r)
        want = counts.clone()
        same = {"count_within": bool(torch.equal(tree.count_within(dq, r), want))}
        if not args.quick:
            knob(True)
            same["count_within_shortcut_off"] = bool(torch.equal(tree.count_within(dq, r), want))
            knob(False)
            same["count_within_max16"] = bool(torch.equal(tree.count_within(dq, r, 16), torch.clamp(want, max=16)))
        row = {"r": r, "nq": nq, "hits_per_query": round(float(want.sum().item()) / nq, 2), "equal_counts": same}
        for name in forms:
            row[name] = summary(ms[name])
        row["speedup_vs_radius_count"] = round(row["radius_count_device"]["median_ms"] / row["count_within"]["median_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config3 L (7.73 M points, 7.20 M queries)",
           "reps": args.reps, "order": "forms alternate repetition by repetition", "rows": rows,
           "side_table": {"first_call_ms": round(table_ms, 2), "bytes": (info1 - info0) if info0 is not None else None}}
    if not args.quick:
        p64, q64 = pts.astype(np.float64), q.astype(np.float64)
        t64 = pt.KdTree(p64, pt.Metric.L2Squared, 10, device=0)
        dq64 = torch.from_numpy(q64).cuda()
        t64.count_within(dq64, 1.0)
        res["float64_r1"] = summary([event_ms(lambda: t64.count_within(dq64, 1.0)) for _ in range(args.reps)])
        print(json.dumps({"float64_r1": res["float64_r1"]}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
