#!/usr/bin/env python3
"""search_radius with a radius per query row against the scalar radius search on the LiDAR clouds of BASELINE config 3
(7.73 M points, cloud L, one MI355X, device buffers), at 7.20 M queries and at the first 150 k of them.

In one process, the forms of a comparison ALTERNATING repetition by repetition, device-event milliseconds per call
(median, min and max of the repetitions).  A "call" is the whole two-pass search as a caller of the C ABI runs it: the
count pass, a cumulative sum of the counts (torch) with the read-back of the total, the allocation of the rows, the fill
pass.

  constant   the per-row form (ptk_search_count_within_radii_device with max_count = 0, then
             ptk_search_radius_radii_fill_device) with a CONSTANT radii array against the scalar
             ptk_search_radius_count_device + ptk_search_radius_fill_device at the same radius, r = 0.25 and 1.0.  The
             scalar form captures its rows in the count pass (leaf lists, the cooperative search for the long rows) and
             replays them in the fill pass; the per-row form traverses twice and captures nothing, so it is expected to
             lose.  Reported: the ratio of the medians, the run-to-run spread of the scalar form ((max - min) / median)
             beside it, and whether the two forms gave the same bytes.
  adaptive   radii[i] proportional to the range of query i from the sensor of the query scan, scaled to a median of 1.0
             and clipped at --clip (default 4.0), against the only thing a caller without the per-row form can do: the
             scalar search at max(radii) (whose rows would then still have to be filtered).  The scalar form is left
             out where its rows would not fit --max-records (the count of its rows is reported instead).

Writes profiles/radius_radii_bench.json (or --out) and prints it.

  python tools/bench_radius_radii.py [--reps N] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

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


def alternate(forms, reps):
    """{name: summary} of the forms, one warm-up each, then alternating repetition by repetition."""
    for fn in forms.values():
        fn()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(event_ms(fn))
    return {name: summary(v) for name, v in ms.items()}


def spread(s):
    return round((s["max_ms"] - s["min_ms"]) / s["median_ms"], 3)


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clip", type=float, default=4.0)
    ap.add_argument("--max-records", type=float, default=2e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_radii_bench.json"))
    args = ap.parse_args()

    pts, q_all = ds.config2_clouds("L")
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
    tree.count_within(torch.from_numpy(q_all[:64]).cuda(), 1.0)  # (the first count builds the side table)
    sensor = np.array([3.0, 1.5, 2.0], dtype=np.float64) * 20.0  # (datasets.config2_clouds: the pose of the query scan)
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config3 L (7.73 M points)", "reps": args.reps,
           "order": "forms alternate repetition by repetition",
           "call": "count pass + cumsum + read-back of the total + allocation + fill pass", "batches": []}
    for nq in (150_000, len(q_all)):
        q = np.ascontiguousarray(q_all[:nq])
        dq = torch.from_numpy(q).cuda()
        batch = {"nq": nq, "constant": [], "adaptive": None}

        def scalar(r):
            return tree.search_radius_device(dq, r)

        def per_row(dr):
            return tree.search_radius_device(dq, dr)

        for r in (0.25, 1.0):
            dr = torch.full((nq,), r, dtype=torch.float32, device="cuda")
            t = alternate({"scalar": lambda: scalar(r), "radii": lambda: per_row(dr)}, args.reps)
            (o1, f1), (o2, f2) = scalar(r), per_row(dr)
            row = {"r": r, **t, "records": int(o1[-1]), "same_bytes": bool(torch.equal(o1, o2) and torch.equal(f1, f2)),
                   "ratio_radii_to_scalar": round(t["radii"]["median_ms"] / t["scalar"]["median_ms"], 3),
                   "scalar_spread": spread(t["scalar"])}
            del o1, f1, o2, f2
            batch["constant"].append(row)
            print(json.dumps(row), flush=True)

        rng = np.sqrt(((q.astype(np.float64) - sensor) ** 2).sum(1))
        radii = np.minimum(rng / np.median(rng), args.clip).astype(np.float32)
        dr = torch.from_numpy(radii).cuda()
        r_max = float(radii.max())
        at_max = int(tree.count_within(dq, r_max).sum())
        forms = {"radii": lambda: per_row(dr)}
        if at_max <= args.max_records:
            forms["scalar_at_max_radius"] = lambda: scalar(r_max)
        t = alternate(forms, args.reps)
        ad = {"radii": "range from the sensor / its median, clipped at %g" % args.clip, **t,
              "median_radius": round(float(np.median(radii)), 4), "max_radius": round(r_max, 4),
              "records_radii": int(per_row(dr)[0][-1]), "records_scalar_at_max": at_max}
        if "scalar_at_max_radius" in t:
            ad["ratio_radii_to_scalar_at_max"] = round(t["radii"]["median_ms"] / t["scalar_at_max_radius"]["median_ms"], 3)
            ad["scalar_spread"] = spread(t["scalar_at_max_radius"])
        else:
            ad["scalar_at_max_radius"] = "not run: its rows exceed --max-records"
        batch["adaptive"] = ad
        print(json.dumps(ad), flush=True)
        res["batches"].append(batch)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # (after every batch: a run that is cut short keeps what it measured)
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
