#!/usr/bin/env python3
"""spacing_knn_self on cloud L (BASELINE config 2's tree points, 7.73 M) and on every 51st of them (150 k) against the
route a caller had to the same numbers before: the rows of search_knn_self on the device, reduced in torch (one MI355X,
device buffers).  For k = 8, 16 and 30 these forms:

  A_mean     ptk_spacing_knn_self_device, mean only (route 1: the direct kernel with the reducing exit)
  A_all      the same with kth, keep and the record (the statistics kernels on the same stream)
  B_rows     search_knn_self(device=True), then torch: sqrt, mean over the row, mean / std over the cloud, the mask
  C_rows     search_knn_self(device=True) alone -- the traversal A runs, with its 8 k bytes per point stored

Milliseconds per call, host clock around the call and a device synchronisation; `reps` repetitions with the forms
alternating, after one warm-up round; median, min and max per form.  Before it times anything the tool checks A's mask
against B's wherever the two decisions are not within rounding of each other.

``--root PATH`` measures the package of another checkout (C_rows on the parent commit: ``--root <parent> --forms C_rows``).
Writes profiles/spacing_knn_self_bench.json (or the path given with --out) and prints each row.

  python tools/bench_spacing.py [--reps N] [--out PATH] [--small-only] [--forms A_mean,A_all,B_rows,C_rows] [--root PATH]
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


def stats(ms):
    ms = np.array(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spacing_knn_self_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="the 150 k tree only (a quick look)")
    ap.add_argument("--ks", default="8,16,30")
    ap.add_argument("--forms", default="A_mean,A_all,B_rows,C_rows")
    ap.add_argument("--root", default=ROOT, help="the checkout whose pico_tree_amd is measured")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    if not torch.cuda.is_available():
        raise SystemExit("bench_spacing.py needs a GPU")
    wanted = args.forms.split(",")
    lib = pt._load()
    full, _ = ds.config2_clouds("L", nq=1)
    clouds = [("150k", np.ascontiguousarray(full[::51][:150_000]))]
    if not args.small_only:
        clouds.insert(0, ("7.73M", full))
    F32 = ctypes.c_float
    rows_out = []
    for name, pts in clouds:
        n = len(pts)
        tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.current_stream().cuda_stream
        have_a = "A_mean" in wanted or "A_all" in wanted
        if have_a:
            mean = torch.zeros(n, dtype=torch.float32, device=dev)
            kth = torch.zeros(n, dtype=torch.float32, device=dev)
            keep = torch.zeros(n, dtype=torch.uint8, device=dev)
            rec = torch.zeros(64, dtype=torch.uint8, device=dev)
            need = ctypes.c_uint64(0)
            assert lib.ptk_spacing_knn_self_workspace(tree._h, ctypes.byref(need)) == 0
            ws = torch.zeros(int(need.value), dtype=torch.uint8, device=dev)
        for k in [int(x) for x in args.ks.split(",")]:
            assert tree.self_route(k) == 1
            raw = torch.empty((n, k, 2), dtype=torch.int32, device=dev)

            def a_mean():
                assert lib.ptk_spacing_knn_self_device(tree._h, k, 1, F32(2.0), mean.data_ptr(), None, None, None, None, 0,
                                                       stream) == 0

            def a_all():
                assert lib.ptk_spacing_knn_self_device(tree._h, k, 1, F32(2.0), mean.data_ptr(), kth.data_ptr(), keep.data_ptr(),
                                                       rec.data_ptr(), ws.data_ptr(), int(need.value), stream) == 0

            def c_rows():
                tree.search_knn_self(k, raw)

            def b_rows():
                tree.search_knn_self(k, raw)
                d = raw[:, :, 1].view(torch.float32)
                m = torch.sqrt(d).mean(dim=1)
                mu, sigma = m.double().mean(), m.double().std()
                return m, m.double() <= mu + 2.0 * sigma, mu, sigma

            table = {"A_mean": a_mean, "A_all": a_all, "B_rows": b_rows, "C_rows": c_rows}
            forms = [(f, table[f]) for f in wanted]
            if "A_all" in wanted and "B_rows" in wanted:  # the answer, once
                a_all()
                m, mask, mu, sigma = b_rows()
                torch.cuda.synchronize()
                clear = (m.double() - (mu + 2.0 * sigma)).abs() > 1e-6 * (mu + 2.0 * sigma)
                assert torch.equal(keep.bool()[clear], mask[clear]), "keep differs from the mask over the rows"
            ms = {f: [] for f, _ in forms}
            for rep in range(args.reps + 1):  # (round 0 warms every form up)
                for f, fn in forms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep > 0:
                        ms[f].append((time.perf_counter() - t0) * 1e3)
            row = {"tree": name, "n_points": n, "k": k, "row_bytes_avoided": n * k * 8, **{f: stats(v) for f, v in ms.items()}}
            if have_a and "A_all" in wanted:
                row["kept"] = int(keep.sum().item())
            if "A_mean" in ms and "C_rows" in ms:
                row["A_mean_over_C_rows"] = round(row["A_mean"]["median_ms"] / row["C_rows"]["median_ms"], 3)
            if "A_all" in ms and "B_rows" in ms:
                row["A_all_over_B_rows"] = round(row["A_all"]["median_ms"] / row["B_rows"]["median_ms"], 3)
            rows_out.append(row)
            print(json.dumps(row), flush=True)
            del raw
        del tree
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L (tree points)", "reps": args.reps,
           "package": "this checkout" if os.path.abspath(args.root) == ROOT else "another checkout (--root)", "clock": "host clock around the call and a device synchronisation",
           "rows": rows_out}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
