#!/usr/bin/env python3
"""cluster_within_self on cloud L (BASELINE config 2's tree points) against the only route a caller had to the same
answer before, up to the point where the host takes over (one MI355X, device buffers).

For each tree size (7.73 M points; 150 k points, every 51st of them: the shapes of tools/bench_radius_self.py) and r in
{0.25, 1.0, 4.0} (metric units: squared radii), these forms:

  cluster_mn0       ptk_cluster_within_self_device, min_neighbors = 0: init, link, flatten
  cluster_mn4       ... min_neighbors = 4: mark, link, flatten, border, decode
  cluster_mn0_plain / cluster_mn4_plain   the same with find NOT halving its paths (test hook cluster_compress = 0)
  rows_route        ptk_search_count_within_self_device (max_count = 0), torch.cumsum and
                    ptk_search_radius_self_fill_device at the same radius: the rows a caller would then pull down and
                    feed to a union-find on the host -- neither the download nor that union-find is counted

Milliseconds per call, host clock around the call and a device synchronisation; `reps` repetitions with the forms
alternating, after one warm-up round; median, min and max per form, the ratio cluster / rows_route of the medians and
the run-to-run spread of the rows route, (max - min) / median.  The per-pass split comes from ptk_profile_* in a run of
its own per form: mark + border (search_ms - search_tail_ms), link (search_tail_ms), the elementwise passes (other_ms).
Before it times anything the tool checks the labels of the 150 k tree against a union-find over the rows on the host.
Writes profiles/cluster_self_bench.json (or the path given with --out) and prints each row.

  python tools/bench_cluster_self.py [--reps N] [--out PATH] [--small-only]
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


def host_components(offsets, index):
    """Labels of plain connected components over rows, by a sequential union-find on the host."""
    n = len(offsets) - 1
    row = np.repeat(np.arange(n), np.diff(offsets))
    lo, hi = np.minimum(row, index), np.maximum(row, index)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for key in np.unique(lo.astype(np.int64) * n + hi).tolist():
        a, b = find(key // n), find(key % n)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_self_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="the 150 k tree only (a quick look)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster_self.py needs a GPU")

    lib = pt._load()
    full, _ = ds.config2_clouds("L", nq=1)
    clouds = [("150k", np.ascontiguousarray(full[::51][:150_000]))]
    if not args.small_only:
        clouds.insert(0, ("7.73M", full))
    rows = []
    for name, pts in clouds:
        n = len(pts)
        tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
        stream = torch.cuda.current_stream().cuda_stream
        labels = torch.zeros(n, dtype=torch.int32, device="cuda")
        counts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        for r in (0.25, 1.0, 4.0):
            rr = np.float32(r)

            def cluster(mn, compress):
                def call():
                    pt.set_test_knobs(cluster_compress=compress)
                    assert lib.ptk_cluster_within_self_device(tree._h, rr, None, mn, labels.data_ptr(), stream) == 0
                return call

            def count():
                assert lib.ptk_search_count_within_self_device(tree._h, rr, None, 0, counts.data_ptr(), stream) == 0

            count()
            torch.cuda.synchronize()
            total = int(counts[:n].sum().item())
            out = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")

            def rows_route():
                count()
                offsets[1:] = torch.cumsum(counts[:n], 0)
                assert lib.ptk_search_radius_self_fill_device(tree._h, rr, None, offsets.data_ptr(), out.data_ptr(), 0,
                                                              stream) == 0

            forms = (("cluster_mn0", cluster(0, 1)), ("cluster_mn4", cluster(4, 1)), ("cluster_mn0_plain", cluster(0, 0)),
                     ("cluster_mn4_plain", cluster(4, 0)), ("rows_route", rows_route))
            if name == "150k":  # the answer, once per radius, against the host's union-find over the rows
                rows_route()
                cluster(0, 1)()
                torch.cuda.synchronize()
                want = host_components(offsets.cpu().numpy(), out[:total, 0].cpu().numpy().astype(np.int64))
                assert np.array_equal(labels.cpu().numpy(), want), "labels differ from the host's union-find"
            ms = {f: [] for f, _ in forms}
            for rep in range(args.reps + 1):  # (round 0 warms every form up)
                for f, fn in forms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep > 0:
                        ms[f].append((time.perf_counter() - t0) * 1e3)
            row = {"tree": name, "n_points": n, "r": r, "neighbours_per_point": round(total / n, 2),
                   **{f: stats(v) for f, v in ms.items()}}
            base = row["rows_route"]
            for f, _ in forms[:-1]:
                row[f + "_over_rows_route"] = round(row[f]["median_ms"] / base["median_ms"], 3)
            row["rows_route_spread"] = round((base["max_ms"] - base["min_ms"]) / base["median_ms"], 3)
            # the per-pass split: a run of its own per form, the events of the handle's profile
            for f, fn in forms[:-1]:
                tree.profile(enable=True, reset=True)
                fn()
                torch.cuda.synchronize()
                p = tree.profile(enable=False, reset=True)
                row[f + "_passes_ms"] = {"mark_border": round(p["search_ms"] - p["search_tail_ms"], 3),
                                         "link": round(p["search_tail_ms"], 3), "elementwise": round(p["other_ms"], 3)}
            cluster(0, 1)()
            torch.cuda.synchronize()
            got = labels.cpu().numpy()
            row["clusters_mn0"] = int((got == np.arange(n)).sum())
            row["largest_cluster_mn0"] = int(np.bincount(got).max())
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out
        pt.set_test_knobs(cluster_compress=None)
        del tree, labels, counts, offsets
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps,
           "clock": "host clock around the call and a device synchronisation", "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
