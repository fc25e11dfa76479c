#!/usr/bin/env python3
"""mst_within_self on cloud L (BASELINE config 2's tree points, 7.73 M), on a 1 M subsample and on every 51st point
(150 k), one MI355X, device buffers.  Two radii per cloud: +inf (the Euclidean minimum spanning tree) and 4 x the median
8th-neighbour distance (squared under L2Squared: 16 x the median of spacing_knn_self's kth).  Per cloud and radius:

  mst          ptk_mst_within_self_device as it is: every branch tested against the component table: total time, rounds,
               time per round
  mst_far      the same with only the root and the far children tested against the table (mst_skip=1)
  mst_noskip   the same without the table (mst_skip=0): the A/B that justifies it.  Its cost grows with the square of
               the component sizes at radius inf, so a run is made only where the run one size below predicts less than
               --limit seconds (quadratic in n at inf, linear at the finite radius); otherwise the prediction is recorded
  knn1_self    search_knn_self(k = 1) on the device: the floor of a first round
  host_loop    ptk_host_mst_within_self at the finite radius, where its rows fit (--host-max points): what a caller has
               without the feature

Milliseconds per call, host clock around the call and a device synchronisation, median of `reps` after one warm-up.
Before it times a form the tool checks its edges against the default form's (same set).  The file is rewritten after
every row, so a run that is cut short leaves what it measured.

  python tools/bench_mst.py [--reps N] [--out PATH] [--sizes 150k,1M,7.73M] [--limit SECONDS] [--host-max N]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mst_within_self_bench.json"))
    ap.add_argument("--sizes", default="150k,1M,7.73M")
    ap.add_argument("--limit", type=float, default=20.0, help="seconds a run without the table may be predicted to take")
    ap.add_argument("--host-max", type=int, default=200_000, help="points up to which the host loop is run")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)

    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    if not torch.cuda.is_available():
        raise SystemExit("bench_mst.py needs a GPU")
    lib = pt._load()
    full, _ = ds.config2_clouds("L", nq=1)
    table = {"150k": np.ascontiguousarray(full[::51][:150_000]), "1M": np.ascontiguousarray(full[::7][:1_000_000]),
             "7.73M": full}
    dev = torch.device("cuda", 0)
    rows_out = []
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps,
           "clock": "host clock around the call and a device synchronisation", "rows": rows_out}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    last_noskip = {}  # radius kind -> (n, seconds) of the largest run made without the table
    for name in args.sizes.split(","):
        pts = table[name]
        n = len(pts)
        tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
        stream = torch.cuda.current_stream().cuda_stream
        need = ctypes.c_uint64(0)
        assert lib.ptk_mst_within_self_workspace(tree._h, ctypes.byref(need)) == 0
        ws = torch.zeros(int(need.value), dtype=torch.uint8, device=dev)
        edges = torch.zeros((n - 1, 3), dtype=torch.int32, device=dev)
        raw1 = torch.empty((n, 1, 2), dtype=torch.int32, device=dev)
        _, kth = tree.spacing_knn_self(8, sqrt=False, kth=True)
        finite = np.float32(16) * np.float32(np.median(kth))

        def timed(fn, reps):
            ms = []
            for rep in range(reps + 1):  # (round 0 warms up)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if rep > 0 or reps == 0:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(ms)), 3), out

        def mst(radius, skip):
            if skip is None:
                os.environ.pop("PTK_TEST_KNOBS", None)
            else:
                os.environ["PTK_TEST_KNOBS"] = f"mst_skip={skip}"
            count, rounds = ctypes.c_uint64(0), ctypes.c_uint32(0)
            rc = lib.ptk_mst_within_self_device(tree._h, ctypes.c_float(radius), None, edges.data_ptr(), None, ws.data_ptr(),
                                                int(need.value), ctypes.byref(count), ctypes.byref(rounds), stream)
            os.environ.pop("PTK_TEST_KNOBS", None)
            assert rc == 0, lib.ptk_last_error()
            return int(count.value), int(rounds.value)

        def edge_set(count):
            e = edges[:count]
            key = (e[:, 0].to(torch.int64) << 32) | e[:, 1].to(torch.int64)
            order = torch.argsort(key)
            return key[order], e[:, 2][order].clone()

        row = {"tree": name, "n_points": n}
        ms, _ = timed(lambda: tree.search_knn_self(1, raw1), args.reps)
        row["knn1_self_ms"] = ms
        for kind, radius in (("inf", float("inf")), ("4x_median_8th", float(finite))):
            cell = {"radius": radius}
            ms, (count, rounds) = timed(lambda: mst(radius, None), args.reps)
            cell["mst"] = {"total_ms": ms, "rounds": rounds, "ms_per_round": round(ms / max(rounds, 1), 3), "n_edges": count}
            want = edge_set(count)
            ms, (count2, rounds2) = timed(lambda: mst(radius, 1), args.reps)
            got = edge_set(count2)
            assert count2 == count and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "mst_skip=1 differs"
            cell["mst_far"] = {"total_ms": ms, "rounds": rounds2, "ms_per_round": round(ms / max(rounds2, 1), 3)}
            predicted = None
            if kind in last_noskip:
                n0, s0 = last_noskip[kind]
                predicted = s0 * ((n / n0) ** 2 if kind == "inf" else n / n0)
            if predicted is not None and predicted > args.limit:
                cell["mst_noskip"] = {"not_run": f"predicted {predicted:.0f} s from the {last_noskip[kind][0]}-point run "
                                      f"({'quadratic' if kind == 'inf' else 'linear'} in n): it merely needs too long"}
            else:
                ms, (count0, rounds0) = timed(lambda: mst(radius, 0), 0)  # (one run, no warm-up: it is the long one)
                got = edge_set(count0)
                assert count0 == count and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "mst_skip=0 differs"
                cell["mst_noskip"] = {"total_ms": ms, "rounds": rounds0, "ms_per_round": round(ms / max(rounds0, 1), 3)}
                last_noskip[kind] = (n, ms / 1e3)
            if kind != "inf" and n <= args.host_max:
                host = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=pt.PTK_DEVICE_NONE)
                out = np.zeros(n - 1, dtype=pt.MST_EDGE)
                n_e = ctypes.c_uint64(0)
                t0 = time.perf_counter()
                assert lib.ptk_host_mst_within_self(host._h, pts.ctypes.data, ctypes.c_float(radius), None, out.ctypes.data,
                                                    ctypes.byref(n_e), None) == 0
                cell["host_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                assert n_e.value == count
            elif kind != "inf":
                cell["host_loop_ms"] = "not run: the host loop keeps every row at once, which does not fit at this size"
            row[kind] = cell
            print(json.dumps({"tree": name, kind: cell}), flush=True)
            rows_out.append({"tree": name, "n_points": n, "knn1_self_ms": row["knn1_self_ms"], "kind": kind, **cell})
            save()
        del tree, ws, edges, raw1
    save()


if __name__ == "__main__":
    main()
