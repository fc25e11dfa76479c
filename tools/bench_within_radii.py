#!/usr/bin/env python3
"""The per-row forms of search_knn_within / count_within against their scalar forms on the LiDAR clouds of BASELINE
config 3 (7.73 M points, cloud L, one MI355X, device buffers), at 7.20 M queries and at the first 150 k of them.  (The
clouds come from datasets.config2_clouds("L"): configs 2 and 3 of BASELINE share cloud L and differ in k only.)

In one process, the forms of a comparison ALTERNATING repetition by repetition, device-event milliseconds per call
(median, min and max of the repetitions):

  constant   the _radii forms with a CONSTANT radii array against the scalar forms at the same radius: search_knn_within
             k = 1 and k = 16 at r = 1.0, count_within at r = 0.25 / 1.0 / 4.0 (the radii of
             profiles/count_within_bench.json).  The scalar forms are the yardstick; the per-row form adds one load per
             query.  Reported: the ratio of the medians, the run-to-run spread of the scalar form ((max - min) / median)
             beside it, and whether the two forms gave the same bytes.
  warm       the ICP warm start, k = 1: radii[i] is just above the distance from q_i to the neighbour that a copy of the
             batch displaced by a small rigid motion (0.5 degrees about z, 5 cm / 2 cm) found -- the bound iteration
             n + 1 of a registration has from iteration n.  Against search_knn k = 1 and against the scalar bounded
             search at max(radii); the share of rows whose neighbour is search_knn's is reported.

Writes profiles/within_radii_bench.json (or --out) and prints it.

  python tools/bench_within_radii.py [--reps N] [--out PATH]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "within_radii_bench.json"))
    args = ap.parse_args()

    pts, q_all = ds.config2_clouds("L")
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
    dp = torch.from_numpy(pts).cuda()
    tree.count_within(torch.from_numpy(q_all[:64]).cuda(), 1.0)  # (the first count builds the side table)
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config3 L (7.73 M points)", "reps": args.reps,
           "order": "forms alternate repetition by repetition", "batches": []}
    for nq in (len(q_all), 150_000):
        q = np.ascontiguousarray(q_all[:nq])
        dq = torch.from_numpy(q).cuda()
        batch = {"nq": nq, "constant": [], "warm_start": None}

        def const(r):
            return torch.full((nq,), r, dtype=torch.float32, device="cuda")

        for k in (1, 16):
            r, dr = 1.0, const(1.0)
            t = alternate({"scalar": lambda: tree.search_knn_within(dq, k, r),
                           "radii": lambda: tree.search_knn_within(dq, k, dr)}, args.reps)
            same = bool(torch.equal(tree.search_knn_within(dq, k, r).raw, tree.search_knn_within(dq, k, dr).raw))
            row = {"form": "search_knn_within", "k": k, "r": r, **t, "same_bytes": same,
                   "ratio_radii_to_scalar": round(t["radii"]["median_ms"] / t["scalar"]["median_ms"], 3),
                   "scalar_spread": spread(t["scalar"])}
            batch["constant"].append(row)
            print(json.dumps(row), flush=True)
        for r in (0.25, 1.0, 4.0):
            dr = const(r)
            t = alternate({"scalar": lambda: tree.count_within(dq, r),
                           "radii": lambda: tree.count_within(dq, dr)}, args.reps)
            same = bool(torch.equal(tree.count_within(dq, r), tree.count_within(dq, dr)))
            row = {"form": "count_within", "r": r, **t, "same_bytes": same,
                   "ratio_radii_to_scalar": round(t["radii"]["median_ms"] / t["scalar"]["median_ms"], 3),
                   "scalar_spread": spread(t["scalar"])}
            batch["constant"].append(row)
            print(json.dumps(row), flush=True)

        # the warm start: the neighbours of the batch displaced by a small rigid motion bound this batch's rows
        a = np.deg2rad(0.5)
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]],
                           dtype=torch.float32, device="cuda")
        moved = (dq @ rot.T + torch.tensor([0.05, 0.02, 0.0], device="cuda")).contiguous()
        prev = tree.search_knn(moved, 1).raw[:, 0, 0].long()
        d = ((dq - dp[prev]) ** 2).sum(1)
        radii = torch.nextafter(d * 1.000001, torch.full_like(d, float("inf"))).contiguous()
        r_max = float(radii.max().item())
        t = alternate({"search_knn": lambda: tree.search_knn(dq, 1),
                       "scalar_at_max_radius": lambda: tree.search_knn_within(dq, 1, r_max),
                       "radii": lambda: tree.search_knn_within(dq, 1, radii)}, args.reps)
        nn = tree.search_knn(dq, 1).raw
        got = tree.search_knn_within(dq, 1, radii).raw
        batch["warm_start"] = {
            "k": 1, "motion": "0.5 deg about z, (0.05, 0.02, 0)", **t,
            "median_radius": round(float(radii.median().item()), 5), "max_radius": round(r_max, 3),
            "rows_equal_search_knn": round(float((got[:, 0, 0] == nn[:, 0, 0]).float().mean().item()), 6),
            "ratio_radii_to_search_knn": round(t["radii"]["median_ms"] / t["search_knn"]["median_ms"], 3),
            "ratio_radii_to_scalar_at_max": round(t["radii"]["median_ms"] / t["scalar_at_max_radius"]["median_ms"], 3)}
        print(json.dumps(batch["warm_start"]), flush=True)
        res["batches"].append(batch)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # (after every batch: a run that is cut short keeps what it measured)
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
