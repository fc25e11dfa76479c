#!/usr/bin/env python3
"""suppress_within_self on cloud L (BASELINE config 2's tree points, 7.73 M) against the only route a caller had to the
same answer before: the rows of search_radius_self on the device and the same rounds written in torch over the flat rows
(one MI355X, device buffers).

For each radius (squared, metric units; chosen to give about 8 and about 30 neighbours per row) and each order --
``scores`` None (the hashed default) and the curvature of normals_within_self at the same radius -- these forms:

  suppress      ptk_suppress_within_self_device: init, then rounds until none is undecided (one 4-byte read-back each)
  rows_route    ptk_search_count_within_self_device (max_count = 0), torch.cumsum, ptk_search_radius_self_fill_device,
                then the rounds in torch over (row, index) of the flat rows: per round a scatter-reduce of "a kept
                neighbour of higher key" and "an undecided one" per row.  Where the rows and the temporaries of those
                rounds do not fit the device's free memory the size is reported as "rows do not fit"; the 150 k tree,
                which always fits, is measured in every run.

Milliseconds per call, host clock around the call and a device synchronisation; `reps` repetitions with the forms
alternating, after one warm-up round; median, min and max per form; the rounds launched; the first round alone (a run
of its own with the handle's profile events: search_ms - search_tail_ms) and the later rounds together; the bytes of rows
the call does without.
Before it times anything the tool checks the device result against the torch rounds over the rows on the 150 k tree.
Writes profiles/suppress_within_self_bench.json (or the path given with --out) and prints each row.

  python tools/bench_suppress.py [--reps N] [--out PATH] [--small-only]
"""
from __future__ import annotations

import argparse
import ctypes
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


def torch_keys(torch, n, scores, device):
    """key(i) of the contract as int64 that compares like the uint64: (ord_i << 31 | (0x7FFFFFFF - i)) needs n < 2^31;
    ord_i: fmix32(i) or the total-order map of the score's bits."""
    i = torch.arange(n, dtype=torch.int64, device=device)
    if scores is None:
        h = i.clone()
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
        ord_ = h
    else:
        b = scores.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        ord_ = torch.where((b & 0x80000000) != 0, b ^ 0xFFFFFFFF, b ^ 0x80000000)
    return (ord_ << 31) | (0x7FFFFFFF - i)


def torch_rounds(torch, n, row, idx, key):
    """The rounds over flat rows: (keep as uint8, rounds)."""
    state = torch.full((n,), 2, dtype=torch.uint8, device=row.device)
    higher = key[idx] > key[row]
    row_h, idx_h = row[higher], idx[higher]
    rounds = 0
    while True:
        rounds += 1
        s = state[idx_h]
        kept = torch.zeros(n, dtype=torch.bool, device=row.device).index_put_((row_h[s == 1],), torch.tensor(True, device=row.device))
        open_ = torch.zeros(n, dtype=torch.bool, device=row.device).index_put_((row_h[s == 2],), torch.tensor(True, device=row.device))
        undecided = state == 2
        state = torch.where(undecided & kept, torch.zeros_like(state), state)
        state = torch.where(undecided & ~kept & ~open_, torch.ones_like(state), state)
        if not bool((state == 2).any().item()):
            return state, rounds


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suppress_within_self_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="the 150 k tree only (a quick look)")
    ap.add_argument("--radii", default="0.065,0.15", help="squared radii at 7.73 M points")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_suppress.py needs a GPU")

    lib = pt._load()
    full, _ = ds.config2_clouds("L", nq=1)
    radii_full = [float(x) for x in args.radii.split(",")]
    # (the 150 k tree is every 51st point: the same neighbour counts need 51 times the squared radius on a surface)
    clouds = [("150k", np.ascontiguousarray(full[::51][:150_000]), [r * 51 for r in radii_full])]
    if not args.small_only:
        clouds.insert(0, ("7.73M", full, radii_full))
    rows_out = []
    for name, pts, radii in clouds:
        n = len(pts)
        tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.current_stream().cuda_stream
        keep = torch.zeros(n, dtype=torch.uint8, device=dev)
        counts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        n_rounds = ctypes.c_uint32(0)
        for r in radii:
            rr = np.float32(r)
            # the curvature of every point at the same radius (a row too short for a normal: below every real curvature)
            frames = tree.normals_within_self(r, device=True).view(torch.float32).reshape(n, pt.FRAME.itemsize // 4)
            curvature = torch.nan_to_num(frames[:, pt.FRAME.fields["curvature"][1] // 4], nan=-1.0).contiguous()
            del frames
            assert lib.ptk_search_count_within_self_device(tree._h, rr, None, 0, counts.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            total = int(counts[:n].sum().item())
            row_bytes = total * 8
            free, _ = torch.cuda.mem_get_info()
            # the torch rounds hold the rows, (row, index) as int64 and a few masks of that length: about 8 x the rows
            fits = row_bytes * 8 < free
            for order, scores in (("hashed", None), ("curvature", curvature)):
                sp = scores.data_ptr() if scores is not None else None

                def suppress():
                    assert lib.ptk_suppress_within_self_device(tree._h, rr, None, sp, keep.data_ptr(),
                                                               ctypes.byref(n_rounds), stream) == 0

                out = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev) if fits else None
                key = torch_keys(torch, n, scores, dev)
                route_rounds = [0]

                def rows_route():
                    assert lib.ptk_search_count_within_self_device(tree._h, rr, None, 0, counts.data_ptr(), stream) == 0
                    offsets[1:] = torch.cumsum(counts[:n], 0)
                    assert lib.ptk_search_radius_self_fill_device(tree._h, rr, None, offsets.data_ptr(), out.data_ptr(), 0,
                                                                  stream) == 0
                    row = torch.repeat_interleave(torch.arange(n, device=dev), counts[:n])
                    state, route_rounds[0] = torch_rounds(torch, n, row, out[:total, 0].to(torch.int64), key)
                    return state

                forms = [("suppress", suppress)] + ([("rows_route", rows_route)] if fits else [])
                if fits and name == "150k":  # the answer, once, against the torch rounds over the rows
                    suppress()
                    want = rows_route()
                    torch.cuda.synchronize()
                    assert torch.equal(keep, want), "keep differs from the rounds over the rows"
                ms = {f: [] for f, _ in forms}
                for rep in range(args.reps + 1):  # (round 0 warms every form up)
                    for f, fn in forms:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        if rep > 0:
                            ms[f].append((time.perf_counter() - t0) * 1e3)
                row = {"tree": name, "n_points": n, "r": r, "order": order,
                       "neighbours_per_point": round(total / n, 2), "row_bytes_avoided": row_bytes,
                       "rounds": int(n_rounds.value), "kept": int(keep.sum().item()),
                       **{f: stats(v) for f, v in ms.items()}}
                if fits:
                    row["rows_route_rounds"] = route_rounds[0]
                    row["suppress_over_rows_route"] = round(row["suppress"]["median_ms"] / row["rows_route"]["median_ms"], 3)
                else:
                    row["rows_route"] = "rows do not fit"
                # the first round alone and the later rounds together: the handle's profile events, a run of its own
                tree.profile(enable=True, reset=True)
                suppress()
                torch.cuda.synchronize()
                p = tree.profile(enable=False, reset=True)
                row["first_round_ms"] = round(p["search_ms"] - p["search_tail_ms"], 3)
                row["later_rounds_ms"] = round(p["search_tail_ms"], 3)
                rows_out.append(row)
                print(json.dumps(row), flush=True)
                del out
        del tree, keep, counts, offsets
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps,
           "clock": "host clock around the call and a device synchronisation", "rows": rows_out}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
