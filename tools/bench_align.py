#!/usr/bin/env python3
"""align_step on the headline cloud (BASELINE config 2: 7.73 M tree points, 7.2 M queries; one MI355X) against the routes
a caller had before it.

Forms (device buffers unless said otherwise; the pose is a small rigid motion, the rejection distance the median squared
distance of the batch, the normals of the plane forms random unit vectors -- the cost of a step does not depend on
them):

  step_point / step_plane        ptk_align_step_device: pose kernel, k = 1 search, the summation tree; 384 bytes stay on
                                 the device
  knn1                           ptk_search_knn_device(k = 1) of the same posed queries alone: the share of a step that
                                 is the search
  rows_torch_point / _plane      the route of the parent commit on the device: q' = q R^T + t in torch, search_knn rows,
                                 a gather of the matched tree points (the caller's own device copy, by original index)
                                 and of the normals, the masked sums in float64 with torch (whose order nobody defines)
  host_step_point                ptk_align_step with host buffers: the queries go up, 384 bytes come down
  host_rows_numpy_point          the host-buffer route of the parent commit: search_knn with host buffers (the rows come
                                 down), the pose, the gather and the sums in numpy

Milliseconds per call, host clock around the call and a device synchronisation; `reps` passes with the forms
alternating after one warm-up pass; median, min and max per form and the ratios of the medians.  The sums of the step
are checked against the torch route's (relative difference of every sum, reported).  Writes
profiles/align_step_bench.json (or --out) and prints the row.

  python tools/bench_align.py [--reps N] [--out PATH] [--small-only]
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


def main():
    import torch

    import pico_tree_amd as pt
    from pico_tree_amd import datasets as ds

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_step_bench.json"))
    ap.add_argument("--small-only", action="store_true", help="150 k points and queries only (a quick look)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py needs a GPU")
    if args.reps < 5:
        raise SystemExit("medians of at least 5 passes")

    lib = pt._load()
    pts, q = ds.config2_clouds("L")
    name = "7.73M / 7.2M"
    if args.small_only:
        name, pts, q = "150k / 150k", np.ascontiguousarray(pts[::51][:150_000]), np.ascontiguousarray(q[::48][:150_000])
    n, nq = len(pts), len(q)
    tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    dq = torch.from_numpy(q).cuda()
    dpts = torch.from_numpy(pts).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    dnormals = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=gen), dim=1).contiguous()
    c, s = np.cos(0.01), np.sin(0.01)
    pose = np.array([[c, -s, 0, 0.05], [s, c, 0, -0.03], [0, 0, 1, 0.02]], dtype=np.float32)
    dR, dt = torch.from_numpy(pose[:, :3].copy()).cuda(), torch.from_numpy(pose[:, 3].copy()).cuda()

    need = ctypes.c_uint64()
    assert lib.ptk_align_step_workspace(tree._h, nq, ctypes.byref(need)) == 0
    ws = torch.empty((need.value,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((pt.ALIGN_SUMS.itemsize,), dtype=torch.uint8, device="cuda")
    rows = torch.empty((nq, 1, 2), dtype=torch.int32, device="cuda")
    posed = (dq @ dR.T + dt).contiguous()
    assert lib.ptk_search_knn_device(tree._h, posed.data_ptr(), nq, 1, np.float32(1), rows.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    max_distance = np.float32(rows[:, 0, 1].view(torch.float32).median().item())

    def step(normals, already_posed=False):
        def call():
            src, m = (posed, None) if already_posed else (dq, pose.ctypes.data)
            assert lib.ptk_align_step_device(tree._h, src.data_ptr(), nq, m, max_distance,
                                             normals.data_ptr() if normals is not None else None, out.data_ptr(), None,
                                             ws.data_ptr(), need.value, stream) == 0
        return call

    def knn1():
        assert lib.ptk_search_knn_device(tree._h, posed.data_ptr(), nq, 1, np.float32(1), rows.data_ptr(), stream) == 0

    def rows_torch(plane, already_posed=False):
        def call():
            qp = posed if already_posed else (dq @ dR.T + dt).contiguous()
            assert lib.ptk_search_knn_device(tree._h, qp.data_ptr(), nq, 1, np.float32(1), rows.data_ptr(), stream) == 0
            idx = rows[:, 0, 0].to(torch.int64)
            dist = rows[:, 0, 1].view(torch.float32)
            keep = ((dist < float(max_distance)) & (dist < 3.0e38)).to(torch.float64).unsqueeze(1)
            p64, q64 = dpts.index_select(0, idx).to(torch.float64), qp.to(torch.float64)
            res = {"count": keep.sum(), "sum_distance": (dist.to(torch.float64) * keep[:, 0]).sum()}
            if not plane:
                qm, pm = q64 * keep, p64 * keep
                # (broadcast products and column sums: a float64 matmul of two [nq, 3] blocks is an order slower here)
                res.update(sum_q=qm.sum(0), sum_p=pm.sum(0), sum_qp=(qm.unsqueeze(2) * p64.unsqueeze(1)).sum(0).reshape(9),
                           sum_qq=(qm * q64).sum(), sum_pp=(pm * p64).sum())
            else:
                n64 = dnormals.index_select(0, idx).to(torch.float64)
                r = ((q64 - p64) * n64).sum(1, keepdim=True)
                J = torch.cat([torch.linalg.cross(q64, n64), n64], dim=1) * keep
                jtj = (J.unsqueeze(2) * J.unsqueeze(1)).sum(0)
                res.update(jtj=jtj[torch.triu_indices(6, 6)[0], torch.triu_indices(6, 6)[1]], jtr=(J * r).sum(0),
                           sum_rr=(r * r * keep).sum())
            return res
        return call

    def host_step():
        tree.align_step(q, pose, max_distance).count

    def host_rows_numpy():
        R, t = pose[:, :3], pose[:, 3]
        qp = np.ascontiguousarray(q @ R.T + t, dtype=np.float32)
        found = tree.search_knn(qp, 1)
        keep = found["distance"] < max_distance
        p64, q64 = pts[found["index"][keep]].astype(np.float64), qp[keep].astype(np.float64)
        return q64.sum(0), p64.sum(0), q64.T @ p64, (q64 * q64).sum(), (p64 * p64).sum(), found["distance"][keep].sum(dtype=np.float64)

    forms = [("step_point", step(None)), ("step_plane", step(dnormals)), ("knn1", knn1),
             ("rows_torch_point", rows_torch(False)), ("rows_torch_plane", rows_torch(True)), ("host_step_point", host_step),
             ("host_rows_numpy_point", host_rows_numpy)]
    ms = {f: [] for f, _ in forms}
    for rep in range(args.reps + 1):  # (pass 0 warms every form up)
        for f, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep > 0:
                ms[f].append((time.perf_counter() - t0) * 1e3)
    row = {"cloud": name, "n_points": n, "nq": nq, "max_distance": float(max_distance), "workspace_bytes": int(need.value),
           **{f: stats(v) for f, v in ms.items()}}
    med = {f: row[f]["median_ms"] for f in ms}
    row["search_share_of_step_point"] = round(med["knn1"] / med["step_point"], 3)
    row["search_share_of_step_plane"] = round(med["knn1"] / med["step_plane"], 3)
    row["step_point_over_rows_torch_point"] = round(med["step_point"] / med["rows_torch_point"], 3)
    row["step_plane_over_rows_torch_plane"] = round(med["step_plane"] / med["rows_torch_plane"], 3)
    row["host_step_point_over_host_rows_numpy_point"] = round(med["host_step_point"] / med["host_rows_numpy_point"], 3)
    row["knn1_spread"] = round((row["knn1"]["max_ms"] - row["knn1"]["min_ms"]) / med["knn1"], 3)
    # the sums of the step against the torch route's, both over the same posed queries (torch's pose arithmetic is not
    # the contract's: a row at the rejection distance would flip): every sum, relative to the largest magnitude of its field
    worst = {}
    for plane, normals in ((False, None), (True, dnormals)):
        step(normals, already_posed=True)()
        torch.cuda.synchronize()
        rec = np.ascontiguousarray(out.cpu().numpy()).view(pt.ALIGN_SUMS)[0]
        ref = {k: np.atleast_1d(v.cpu().numpy()) for k, v in rows_torch(plane, already_posed=True)().items()}
        assert int(rec["count"]) == int(ref.pop("count")[0]) and int(rec["rows"]) == nq
        for k, v in ref.items():
            got = np.atleast_1d(rec[k]).ravel()
            worst[("plane_" if plane else "point_") + k] = float(np.abs(got - v).max() / max(np.abs(v).max(), 1e-300))
        row["accepted_rows"] = int(rec["count"])
    row["largest_relative_difference_to_the_torch_route"] = max(worst.values())
    assert row["largest_relative_difference_to_the_torch_route"] < 1e-6, worst  # (float64 sums in two orders)
    print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "cloud": "config2 L", "reps": args.reps,
           "clock": "host clock around the call and a device synchronisation", "rows": [row]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
