#!/usr/bin/env python3
"""ms per call of the host forms with ragged rows, through the C ABI: ptk_search_radius (r^2 = 0.25), ptk_search64_radius
(the same) and ptk_search_box (side 1) at 2 000 and 900 000 queries of BASELINE config 2's cloud L.  One JSON line of
medians; PTK_LIBRARY picks the build, so two builds are compared by running this in alternating processes."""
import ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds

pts, q = ds.config2_clouds("L")
lib = pt._load()
tree = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=0)
tree64 = pt.KdTree(pts.astype(np.float64), pt.Metric.L2Squared, 10, device=0)


def med(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


out = {}
for nq, reps in ((2_000, 15), (900_000, 5)):
    q32 = np.ascontiguousarray(q[:: len(q) // nq][:nq])
    q64 = q32.astype(np.float64)
    lo, hi = q32 - np.float32(0.5), q32 + np.float32(0.5)
    off = np.zeros(nq + 1, dtype=np.uint64)

    def call(fn, *args):
        rows = ctypes.c_void_p()
        assert fn(*args, off.ctypes.data, ctypes.byref(rows)) == 0, lib.ptk_last_error()
        lib.ptk_free(rows)

    out[f"radius_{nq}"] = med(lambda: call(lib.ptk_search_radius, tree._h, q32.ctypes.data, nq, 0.25, 1.0, 0), reps)
    out[f"radius64_{nq}"] = med(lambda: call(lib.ptk_search64_radius, tree64._h, q64.ctypes.data, nq, 0.25, 1.0, 0), reps)
    out[f"box_{nq}"] = med(lambda: call(lib.ptk_search_box, tree._h, lo.ctypes.data, hi.ctypes.data, nq), reps)
    out[f"rows_{nq}"] = int(off[-1])
print(json.dumps(out), flush=True)
