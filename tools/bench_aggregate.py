#!/usr/bin/env python3
"""aggregate_within_self on cloud L (BASELINE config 2's tree points) against the rows route a caller had before and
against normals_within_self (one MI355X, device buffers).

The radius is the median 8th-neighbour distance of the cloud (search_knn_self(8)) and 4 x it (metric units: squared
radii), as in tools/bench_frames_self.py.  Forms:

  agg_<op>_c<channels>   ptk_aggregate_within_self_device with counts, op in sum, max, channels in 1, 4, W, 4 W and 64
                         (W = 8 accumulators per lane: a call of more channels traverses once per window of W)
  rows_<op>_c<channels>  the rows route: ptk_search_count_within_self_device (max_count = 0), torch.cumsum,
                         ptk_search_radius_self_fill_device, then an index-select of `values` by the rows' indices and a
                         segmented reduce in torch (torch.segment_reduce).  Skipped, and said so, where the gathered
                         [rows, channels] block alone would pass --gather-limit-gib
  rows_only              the count, the scan and the fill alone (what every rows_* form starts with)
  moments                ptk_normals_within_self_device, moments only: a traversal that accumulates nine floats

Milliseconds per call, host clock around the call and a device synchronisation; `reps` repetitions with the forms
alternating, after one warm-up round; median, min and max per form, the ratios of the medians and the run-to-run spread
of rows_only, (max - min) / median.  The results on 4 channels are checked against a fold on the host over a sample of
2 000 rows of the fill pass (max exactly; a sum within the float32 bound of a sum in another order); how many of those
rows the rows route's own reduce agrees on is reported beside it.  Writes profiles/aggregate_bench.json (or --out) and prints each row.

  python tools/bench_aggregate.py [--reps N] [--out PATH] [--small-only] [--gather-limit-gib G]
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

W = 8  # kAggWidth (pico_tree_amd/csrc/ptk_kernels_aggregate.hpp)
OPS = {"sum": 0, "max": 2}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="150 k points only (a quick look)")
    ap.add_argument("--gather-limit-gib", type=float, default=24.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_aggregate.py needs a GPU")

    lib = pt._load()
    full, _ = ds.config2_clouds("L", nq=1)
    name, pts = ("150k", np.ascontiguousarray(full[::51][:150_000])) if args.small_only else ("7.73M", full)
    n = len(pts)
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    med = np.float32(np.median(tree.search_knn_self(8)["distance"][:, 7]))
    channel_counts = [1, 4, W, 4 * W, 64]
    gen = torch.Generator(device="cuda").manual_seed(1)
    values = {c: torch.rand((n, c), dtype=torch.float32, device="cuda", generator=gen) - 0.5 for c in channel_counts}
    outs = {c: torch.empty((n, c), dtype=torch.float32, device="cuda") for c in channel_counts}
    agg_counts = torch.zeros(n, dtype=torch.int64, device="cuda")
    moments = torch.empty((n, pt.MOMENTS.itemsize), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rows = []
    for mult in (1, 4):
        rr = np.float32(mult) * med

        def aggregate(op, c):
            def call():
                assert lib.ptk_aggregate_within_self_device(tree._h, rr, None, values[c].data_ptr(), c, OPS[op],
                                                            outs[c].data_ptr(), agg_counts.data_ptr(), stream) == 0
            return call

        def normals_moments():
            assert lib.ptk_normals_within_self_device(tree._h, rr, None, 2, None, None, moments.data_ptr(), stream) == 0

        def count():
            assert lib.ptk_search_count_within_self_device(tree._h, rr, None, 0, counts.data_ptr(), stream) == 0

        count()
        torch.cuda.synchronize()
        total = int(counts[:n].sum().item())
        out = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")

        def rows_only():
            count()
            offsets[1:] = torch.cumsum(counts[:n], 0)
            assert lib.ptk_search_radius_self_fill_device(tree._h, rr, None, offsets.data_ptr(), out.data_ptr(), 0,
                                                          stream) == 0

        def rows_route(op, c):
            def call():
                rows_only()
                gathered = values[c].index_select(0, out[:total, 0].to(torch.int64))
                return torch.segment_reduce(gathered, op, lengths=counts[:n], axis=0, unsafe=True)
            return call

        forms = [("moments", normals_moments), ("rows_only", rows_only)]
        skipped = {}
        for op in OPS:
            for c in channel_counts:
                forms.append((f"agg_{op}_c{c}", aggregate(op, c)))
                gib = total * c * 4 / 2 ** 30
                if gib <= args.gather_limit_gib:
                    forms.append((f"rows_{op}_c{c}", rows_route(op, c)))
                else:
                    skipped[f"rows_{op}_c{c}"] = f"the gathered block alone is {gib:.1f} GiB"
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
        if skipped:
            row["skipped"] = skipped
        for op in OPS:
            for c in channel_counts:
                a = row[f"agg_{op}_c{c}"]["median_ms"]
                row[f"agg_{op}_c{c}_over_moments"] = round(a / row["moments"]["median_ms"], 3)
                if f"rows_{op}_c{c}" in row:
                    row[f"agg_{op}_c{c}_over_rows_route"] = round(a / row[f"rows_{op}_c{c}"]["median_ms"], 3)
                row[f"agg_{op}_c{c}_over_rows_only"] = round(a / row["rows_only"]["median_ms"], 3)
        base = row["rows_only"]
        row["rows_only_spread"] = round((base["max_ms"] - base["min_ms"]) / base["median_ms"], 3)
        # the results on 4 channels against a fold on the host over a sample of the rows the fill pass wrote: the counts, max
        # exactly, sum within the bound of a float32 sum of c terms in another order (2 c eps sum |v|); the rows route's own
        # results on the same sample are reported beside them, not asserted (they are torch's)
        torch_max, torch_sum = rows_route("max", 4)(), rows_route("sum", 4)()
        aggregate("max", 4)()
        torch.cuda.synchronize()
        assert torch.equal(agg_counts, counts[:n]), "counts differ from count_within_self"
        got_max = outs[4].cpu().numpy().copy()
        aggregate("sum", 4)()
        torch.cuda.synchronize()
        got_sum = outs[4].cpu().numpy()
        h_off, h_val = offsets.cpu().numpy(), values[4].cpu().numpy()
        sample = np.random.default_rng(3).choice(np.flatnonzero(np.diff(h_off) > 0), 2000, replace=False)
        agree = {"torch_max": 0, "torch_sum": 0}
        t_max, t_sum = torch_max.cpu().numpy(), torch_sum.cpu().numpy()
        for i in sample:
            v = h_val[out[int(h_off[i]):int(h_off[i + 1]), 0].cpu().numpy()].astype(np.float64)
            bound = 2.0 * len(v) * 2.0 ** -24 * np.abs(v).sum(0)
            assert np.array_equal(got_max[i], v.max(0).astype(np.float32)), ("max differs from the rows", int(i))
            assert np.all(np.abs(got_sum[i] - v.sum(0)) <= bound), ("sum differs from the rows", int(i))
            agree["torch_max"] += int(np.array_equal(t_max[i], v.max(0).astype(np.float32)))
            agree["torch_sum"] += int(np.all(np.abs(t_sum[i] - v.sum(0)) <= bound))
        row["checked_rows"] = {"sample": len(sample), "aggregate_agrees": len(sample), "rows_route_max_agrees": agree["torch_max"],
                               "rows_route_sum_agrees": agree["torch_sum"]}
        del torch_max, torch_sum
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps,
           "accumulators_per_lane": W, "clock": "host clock around the call and a device synchronisation", "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
