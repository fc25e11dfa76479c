"""pico_tree_amd -- Python host side of the MI355X batched k-NN backend.

Mirrors the reference's Python module (``pico_tree.KdTree``,
``/root/reference/src/pyco_tree/pico_tree/_pyco_tree/def_kd_tree.cpp:14-195``):
same constructor arguments, ``search_knn`` / ``search_radius`` overloads, result
dtype ``[('index','<i4'),('distance','<f4')]`` and output shapes
(``(npts,)`` for k == 1, ``(npts, k)`` otherwise;
``_pyco_tree/kd_tree.hpp:362-378``).  Every search runs on the GPU through the
C ABI of ``include/ptk.h`` (``pico_tree_amd/csrc/libptk.so``); there is no CPU
search path here and no fallback: if the library or a device is missing the
call raises.

Two kinds of buffers are accepted:

* numpy arrays (host): copied to the device and back by the backend;
* torch CUDA tensors (device): used in place on the current torch stream, the
  result is a :class:`DeviceNeighbors` holding an ``int32`` tensor of shape
  ``(nq, k, 2)`` whose last axis is ``(index, bits of the float32 distance)``.
"""

from __future__ import annotations

import ctypes
import enum
import os
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32,
                    c_uint32, c_uint64, c_void_p)

import numpy as np

from . import datasets  # noqa: F401  (re-export)

__all__ = ["KdTree", "KdForest", "save_kd_tree", "load_kd_tree", "Metric", "NEIGHBOR", "NEIGHBOR64", "FRAME", "MOMENTS", "DArray", "DeviceNeighbors", "PtkError",
           "library_path", "device_count", "datasets", "trim_pinned_pool", "registered", "empty_pinned",
           "ALIGN_SUMS", "AlignSums", "IcpResult", "icp", "SPACING_STATS", "MST_EDGE"]

_HERE = os.path.dirname(os.path.abspath(__file__))
#: (PTK_LIBRARY: another build of the same library -- the experiment builds of tools/)
_LIB_PATH = os.environ.get("PTK_LIBRARY") or os.path.join(_HERE, "csrc", "libptk.so")

#: Result record; identical to the reference binding's neighbor dtype.
NEIGHBOR = np.dtype([("index", "<i4"), ("distance", "<f4")])
#: ptk_frame / ptk_moments (ptk.h): the records of KdTree.normals_within_self
FRAME = np.dtype([("normal", "<f4", (3,)), ("curvature", "<f4"), ("eigenvalues", "<f4", (3,)), ("count", "<u4")])
MOMENTS = np.dtype([("sum", "<f4", (3,)), ("count", "<u4"), ("outer", "<f4", (6,)), ("pad_", "<u4", (2,))])
#: PTK_AGG_* (ptk.h): the ops of KdTree.aggregate_within_self / aggregate_within
PTK_AGG_SUM, PTK_AGG_MIN, PTK_AGG_MAX, PTK_AGG_INCLUDE_SELF = 0, 1, 2, 0x100
_AGGREGATE_OPS = {"sum": PTK_AGG_SUM, "min": PTK_AGG_MIN, "max": PTK_AGG_MAX}
#: ptk_align_sums (ptk.h): the record of KdTree.align_step, 384 bytes
ALIGN_SUMS = np.dtype([("count", "<u8"), ("rows", "<u8"), ("sum_distance", "<f8"), ("sum_q", "<f8", (3,)),
                       ("sum_p", "<f8", (3,)), ("sum_qp", "<f8", (9,)), ("sum_qq", "<f8"), ("sum_pp", "<f8"),
                       ("jtj", "<f8", (21,)), ("jtr", "<f8", (6,)), ("sum_rr", "<f8")])
assert ALIGN_SUMS.itemsize == 384
#: ptk_spacing_stats (ptk.h): the record of KdTree.outliers_knn_self, 64 bytes; PTK_SPACING_SQRT: the flag of the call
SPACING_STATS = np.dtype([("count", "<u8"), ("rows", "<u8"), ("sum", "<f8"), ("mean", "<f8"), ("ssd", "<f8"),
                          ("variance", "<f8"), ("ratio_squared", "<f8"), ("reserved", "<f8")])
assert SPACING_STATS.itemsize == 64
PTK_SPACING_SQRT = 1
#: The same record of a tree over float64 points: ``neighbor<int, double>`` is 16 bytes with the
#: distance at offset 8, which is what the reference binding's PYBIND11_NUMPY_DTYPE yields for it
#: (_pyco_tree/def_core.hpp:17-18).
NEIGHBOR64 = np.dtype({"names": ["index", "distance"], "formats": ["<i4", "<f8"], "offsets": [0, 8],
                       "itemsize": 16})

#: One edge of :meth:`KdTree.mst_within_self` (``ptk_mst_edge``): 12 bytes.
MST_EDGE = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("w", "<f4")])

PTK_OK = 0
PTK_DEVICE_CURRENT = -1
PTK_DEVICE_NONE = -2
REORDER_AUTO, REORDER_ON, REORDER_OFF = 0, 1, 2


class PtkError(RuntimeError):
    """A non-zero status from libptk (message from ``ptk_last_error``)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"libptk status {status}: {message}")
        self.status = status


class _Info(Structure):
    _fields_ = [("dim", c_uint32), ("n_points", c_uint64), ("n_nodes", c_uint64),
                ("n_leaves", c_uint64), ("max_depth", c_uint32), ("max_leaf_count", c_uint32),
                ("device_bytes", c_uint64), ("device", c_int32)]


class _Profile(Structure):
    _fields_ = [("search_ms", c_double), ("reorder_ms", c_double), ("other_ms", c_double),
                ("launches", c_uint64), ("queries", c_uint64), ("search_tail_ms", c_double)]


_lib = None

_SIGNATURES = {
    "ptk_version": (c_int, []),
    "ptk_last_error": (c_char_p, []),
    "ptk_device_count": (c_int, []),
    "ptk_warmup": (c_int, [c_int32]),
    "ptk_tree_create_from_points": (c_int, [c_void_p, c_uint64, c_uint32, c_uint64, c_int32,
                                            POINTER(c_void_p)]),
    "ptk_tree_create": (c_int, [c_void_p, POINTER(c_void_p)]),
    "ptk_tree_destroy": (None, [c_void_p]),
    "ptk_tree_get_info": (c_int, [c_void_p, POINTER(_Info)]),
    "ptk_tree_get_flat": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_tree_set_reorder": (c_int, [c_void_p, c_int]),
    "ptk_tree_set_metric": (c_int, [c_void_p, c_int]),
    "ptk_tree_set_outer_bounds": (c_int, [c_void_p, c_void_p, c_uint64]),
    "ptk_tree_get_outer_bounds": (c_int, [c_void_p, c_void_p]),
    "ptk_tree_serialize": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]),
    "ptk_tree_create_from_stream": (c_int, [c_void_p, c_uint64, c_uint32, c_void_p, c_uint64, c_int32,
                                            POINTER(c_void_p)]),
    "ptk_tree_create_from_topological_stream": (c_int, [c_void_p, c_uint64, c_uint32, c_void_p, c_uint64, c_int32,
                                                        POINTER(c_void_p)]),
    "ptk_tree_serialize_topological": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]),
    "ptk_search_knn": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p]),
    "ptk_search_knn_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p,
                                      c_void_p]),
    "ptk_search_knn_self": (c_int, [c_void_p, c_uint32, c_void_p]),
    "ptk_search_knn_self_device": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p]),
    "ptk_cluster_within_self": (c_int, [c_void_p, c_float, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_cluster_within_self_device": (c_int, [c_void_p, c_float, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_normals_within_self": (c_int, [c_void_p, c_float, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "ptk_normals_within_self_device": (c_int, [c_void_p, c_float, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p,
                                               c_void_p]),
    "ptk_aggregate_within_self": (c_int, [c_void_p, c_float, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p]),
    "ptk_aggregate_within_self_device": (c_int, [c_void_p, c_float, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p,
                                                 c_void_p]),
    "ptk_aggregate_within": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p,
                                     c_void_p]),
    "ptk_aggregate_within_device": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_void_p, c_void_p, c_uint32, c_uint32,
                                            c_void_p, c_void_p, c_void_p]),
    "ptk_align_step_workspace": (c_int, [c_void_p, c_uint64, POINTER(c_uint64)]),
    "ptk_align_step_device": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_uint64, c_void_p]),
    "ptk_align_step": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "ptk_host_align_step": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "ptk_spacing_knn_self": (c_int, [c_void_p, c_uint32, c_uint32, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_spacing_knn_self_device": (c_int, [c_void_p, c_uint32, c_uint32, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_uint64, c_void_p]),
    "ptk_spacing_knn_self_workspace": (c_int, [c_void_p, POINTER(c_uint64)]),
    "ptk_mst_within_self": (c_int, [c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_mst_within_self_device": (c_int, [c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p,
                                           c_void_p, c_void_p]),
    "ptk_mst_within_self_workspace": (c_int, [c_void_p, POINTER(c_uint64)]),
    "ptk_host_mst_within_self": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_suppress_within_self": (c_int, [c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_suppress_within_self_device": (c_int, [c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_search_count_within_self": (c_int, [c_void_p, c_float, c_void_p, c_uint64, c_void_p]),
    "ptk_search_count_within_self_device": (c_int, [c_void_p, c_float, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_search_radius_self": (c_int, [c_void_p, c_float, c_void_p, c_int, c_void_p, POINTER(c_void_p)]),
    "ptk_search_radius_self_fill_device": (c_int, [c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ptk_search_knn_within": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p]),
    "ptk_search_knn_within_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p, c_void_p]),
    "ptk_search_count_within": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_uint64, c_void_p]),
    "ptk_search_count_within_device": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_uint64, c_void_p, c_void_p]),
    "ptk_search_knn_within_radii": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p]),
    "ptk_search_knn_within_radii_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]),
    "ptk_search_count_within_radii": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p]),
    "ptk_search_count_within_radii_device": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_search_radius_radii_fill_device": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ptk_search_radius_radii": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_int, c_void_p, POINTER(c_void_p)]),
    "ptk_search_radius_count": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_float, c_void_p]),
    "ptk_search_radius_fill": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_float, c_void_p,
                                       c_void_p, c_int]),
    "ptk_search_radius_count_device": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_float,
                                               c_void_p, c_void_p]),
    "ptk_search_radius_fill_device": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_float,
                                              c_void_p, c_void_p, c_int, c_void_p]),
    "ptk_search_radius": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_float, c_int, c_void_p,
                                  POINTER(c_void_p)]),
    "ptk_search_box": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p,
                               POINTER(c_void_p)]),
    "ptk_search_box_count_device": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_search_box_fill_device": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "ptk_free": (None, [c_void_p]),
    "ptk_host_search_knn": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p]),
    "ptk_host_search_knn_within": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p]),
    "ptk_host_search_knn_self": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
    "ptk_host_cluster_within_self": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_host_normals_within_self": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_uint64, c_void_p, c_void_p,
                                             c_void_p]),
    "ptk_host_aggregate_within_self": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p,
                                               c_void_p]),
    "ptk_host_aggregate_within": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_float, c_void_p, c_void_p, c_uint32,
                                          c_uint32, c_void_p, c_void_p]),
    "ptk_host_suppress_within_self": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_host_spacing_knn_self": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_float, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    "ptk_host_search_count_within_self": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_uint64, c_void_p]),
    "ptk_host_search_radius_self": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p, POINTER(c_void_p)]),
    "ptk_host_search_count_within": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_float, c_uint64, c_void_p]),
    "ptk_host_search_knn_within_radii": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p]),
    "ptk_host_search_count_within_radii": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p]),
    "ptk_host_search_radius_radii": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_int, c_void_p, POINTER(c_void_p)]),
    "ptk_host_search_radius": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_float, c_float, c_int,
                                       c_void_p, POINTER(c_void_p)]),
    "ptk_host_search_box": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, POINTER(c_void_p)]),
    "ptk_host_alloc": (c_int, [c_uint64, POINTER(c_void_p)]),
    "ptk_host_free": (None, [c_void_p]),
    "ptk_host_register": (c_int, [c_void_p, c_uint64]),
    "ptk_host_unregister": (c_int, [c_void_p]),
    "ptk_tree64_create_from_points": (c_int, [c_void_p, c_uint64, c_uint32, c_uint64, c_int32, POINTER(c_void_p)]),
    "ptk_tree64_create_from_stream": (c_int, [c_void_p, c_uint64, c_uint32, c_void_p, c_uint64, c_int32,
                                              POINTER(c_void_p)]),
    "ptk_tree64_destroy": (None, [c_void_p]),
    "ptk_tree64_get_info": (c_int, [c_void_p, POINTER(_Info)]),
    "ptk_tree64_set_metric": (c_int, [c_void_p, c_int]),
    "ptk_tree64_serialize": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]),
    "ptk_tree64_serialize_topological": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]),
    "ptk_tree64_create_from_topological_stream": (c_int, [c_void_p, c_uint64, c_uint32, c_void_p, c_uint64, c_int32,
                                                          POINTER(c_void_p)]),
    "ptk_search64_knn": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_double, c_void_p]),
    "ptk_search64_knn_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_double, c_void_p, c_void_p]),
    "ptk_search64_knn_self": (c_int, [c_void_p, c_uint32, c_void_p]),
    "ptk_search64_knn_self_device": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p]),
    "ptk_search64_cluster_within_self": (c_int, [c_void_p, c_double, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_search64_cluster_within_self_device": (c_int, [c_void_p, c_double, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_search64_spacing_knn_self": (c_int, [c_void_p, c_uint32, c_uint32, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_search64_spacing_knn_self_device": (c_int, [c_void_p, c_uint32, c_uint32, c_float, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_uint64, c_void_p]),
    "ptk_search64_spacing_knn_self_workspace": (c_int, [c_void_p, POINTER(c_uint64)]),
    "ptk_search64_suppress_within_self": (c_int, [c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ptk_search64_suppress_within_self_device": (c_int, [c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                                         c_void_p]),
    "ptk_search64_count_within_self": (c_int, [c_void_p, c_double, c_void_p, c_uint64, c_void_p]),
    "ptk_search64_count_within_self_device": (c_int, [c_void_p, c_double, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_search64_radius_self": (c_int, [c_void_p, c_double, c_void_p, c_int, c_void_p, POINTER(c_void_p)]),
    "ptk_search64_knn_within": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_double, c_void_p]),
    "ptk_search64_knn_within_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_double, c_void_p, c_void_p]),
    "ptk_search64_count_within": (c_int, [c_void_p, c_void_p, c_uint64, c_double, c_uint64, c_void_p]),
    "ptk_search64_count_within_device": (c_int, [c_void_p, c_void_p, c_uint64, c_double, c_uint64, c_void_p, c_void_p]),
    "ptk_search64_knn_within_radii": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p]),
    "ptk_search64_knn_within_radii_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]),
    "ptk_search64_count_within_radii": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p]),
    "ptk_search64_count_within_radii_device": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p]),
    "ptk_search64_radius_radii": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_int, c_void_p, POINTER(c_void_p)]),
    "ptk_search64_radius": (c_int, [c_void_p, c_void_p, c_uint64, c_double, c_double, c_int, c_void_p,
                                    POINTER(c_void_p)]),
    "ptk_search64_box": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, POINTER(c_void_p)]),
    "ptk_forest_create": (c_int, [c_void_p, c_uint64, c_uint32, c_uint64, c_uint32, c_uint64, c_int32,
                                  POINTER(c_void_p)]),
    "ptk_forest_destroy": (None, [c_void_p]),
    "ptk_forest_get_rotations": (c_int, [c_void_p, c_void_p]),
    "ptk_forest_get_dropped": (c_int, [c_void_p, POINTER(c_uint64)]),
    "ptk_forest_search_knn": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_uint64, c_void_p]),
    "ptk_forest_search_knn_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_uint64, c_void_p,
                                             c_void_p]),
    "ptk_profile_enable": (c_int, [c_void_p, c_int]),
    "ptk_profile_get": (c_int, [c_void_p, POINTER(_Profile), c_int]),
    "ptk_profile_get_sized": (c_int, [c_void_p, c_void_p, c_uint64, c_int]),
    "ptk_debug_knn1_counts": (c_int, [c_void_p, POINTER(c_uint32)]),
    "ptk_debug_piles": (c_int, [c_void_p, POINTER(ctypes.c_uint64)]),
    "ptk_debug_batch_permutation": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p]),
    "ptk_debug_create_phases": (c_int, [c_void_p, POINTER(c_double)]),
    "ptk_debug_create_route": (c_int, [c_void_p, POINTER(ctypes.c_uint64), POINTER(ctypes.c_char_p)]),
    "ptk_debug_key_bits": (c_int, [c_void_p, c_uint64, POINTER(c_uint32)]),
    "ptk_debug_batch_order": (c_int, [c_void_p, POINTER(c_int)]),
    "ptk_debug_deep_pieces": (c_int, [c_void_p, POINTER(c_uint32)]),
    "ptk_debug_self_route": (c_int, [c_void_p, c_uint32, POINTER(c_int)]),
    "ptk_debug_knn_coop_counts": (c_int, [c_void_p, POINTER(c_uint32)]),
    "ptk_debug_radius_coop_counts": (c_int, [c_void_p, POINTER(c_uint32)]),
    "ptk_tree64_debug_knn_coop_counts": (c_int, [c_void_p, POINTER(c_uint32)]),
    "ptk_debug_knn_cap": (c_int, [c_uint64, c_uint32, c_float, POINTER(c_uint32), POINTER(c_uint64)]),
    "ptk_multi_create_from_points": (c_int, [c_void_p, c_uint64, c_uint32, c_uint64, c_void_p, c_uint32,
                                             POINTER(c_void_p)]),
    "ptk_multi_create": (c_int, [c_void_p, c_void_p, c_uint32, POINTER(c_void_p)]),
    "ptk_multi_destroy": (None, [c_void_p]),
    "ptk_multi_device_count": (c_int, [c_void_p]),
    "ptk_multi_get_tree": (c_int, [c_void_p, c_uint32, POINTER(c_void_p)]),
    "ptk_multi_set_metric": (c_int, [c_void_p, c_int]),
    "ptk_multi_search_knn": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p]),
    "ptk_multi_search_radius": (c_int, [c_void_p, c_void_p, c_uint64, c_float, c_float, c_int, c_void_p,
                                        POINTER(c_void_p)]),
    "ptk_multi_search_knn_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_float, c_void_p, c_void_p]),
}

#: Every symbol include/ptk.h declares; tests check the library exports them all.
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def library_path() -> str:
    return _LIB_PATH


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                f"{_LIB_PATH} is missing: build it with `python -m pico_tree_amd.build` "
                "(there is no CPU fallback)")
        # PyTorch bundles its own HIP runtime under the same SONAME as the system one
        # (libamdhip64.so.7).  Import it first so that libptk binds to the runtime that
        # torch tensors and streams live in, whatever the import order of the caller.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


PTK_ERR_UNSUPPORTED = -2
_host_loop_warned = False
_host_loop_allowed = False


def allow_host_loop(on: bool = True) -> None:
    """Off by default: a batched search the DEVICE refuses for a valid tree (``PTK_ERR_UNSUPPORTED`` -- a topological
    tree deeper than the device stack, a dimension beyond the LDS staging) raises :class:`PtkError`, like every other
    failure of the backend: the batched path has no CPU fallback.  ``allow_host_loop(True)`` lets the wrapper serve such a
    call with the library's host loop (``ptk_host_search_*``: the reference's own batch loop over the per-query search)
    after one ``RuntimeWarning``.  Process-wide."""
    global _host_loop_allowed
    _host_loop_allowed = bool(on)


def _warn_host_loop(why: str) -> None:
    """One warning per process when a call the device search refuses is served by the host loop instead."""
    global _host_loop_warned
    if not _host_loop_warned:
        _host_loop_warned = True
        import warnings
        warnings.warn("pico_tree_amd: the device search refused this call (" + why + "); it runs as a loop of "
                      "per-query host searches over the rows instead, as the reference's module does for every call "
                      "(further refusals are served the same way without this message)", RuntimeWarning, stacklevel=4)


def _check(status: int) -> None:
    if status != PTK_OK:
        raise PtkError(status, _load().ptk_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    return int(_load().ptk_device_count())


def warmup(device: int = -1) -> None:
    """Starts loading the library's device code for ``device`` (default: the current one) in the background, so that
    the first :class:`KdTree` for it does not wait for the load (``ptk_warmup``).  Optional."""
    _check(_load().ptk_warmup(int(device)))


class _PinnedBlock:
    """One block of page-locked host memory out of :class:`_PinnedPool`; numpy arrays made from it keep it alive
    (``__array_interface__``), and the block goes back to the pool when the last of them is gone."""

    def __init__(self, pool, ptr: int, capacity: int, nbytes: int):
        self._pool, self._ptr, self._capacity = pool, ptr, capacity
        self.__array_interface__ = {"data": (ptr, False), "shape": (nbytes,), "typestr": "|u1", "version": 3}

    def __del__(self):
        pool, self._pool = self._pool, None
        if pool is not None:
            pool._give(self._ptr, self._capacity)


class _PinnedPool:
    """Result arrays of the host-buffer searches.  The reference's module returns a NEW array from every
    ``search_knn(pts, k)`` (def_kd_tree.cpp:73-82); a fresh 58 MB numpy array costs its first touch on every call
    (2-19 ms on the hosts of the GPU pool, profiles/r03_notes.txt item 24) and a staging copy on the way.  Here the
    rows land in page-locked blocks (``ptk_host_alloc``) that the device writes directly and that are handed out again
    once the array built on them has been garbage-collected.  ``PTK_PINNED_POOL_MB`` (default 2048) bounds what the
    pool holds, in use and free; beyond it -- or for small results -- plain numpy arrays are returned.  A request is
    served from the smallest idle block that holds it (within a factor of two: a workload whose batch sizes vary reuses
    its blocks instead of pinning one per size), and when the budget is spent the idle blocks of other sizes are freed
    before a pageable array is given out.  ``pico_tree_amd.trim_pinned_pool()`` frees every idle block."""

    MIN_BYTES = 1 << 20

    def __init__(self):
        import threading
        # (re-entrant: a block's __del__ may run -- cyclic garbage collection -- on the thread that holds the lock)
        self._lock = threading.RLock()
        self._free = {}   # capacity -> [ptr, ...]
        self._held = 0    # bytes allocated (in use + free)

    def _budget(self) -> int:
        return int(os.environ.get("PTK_PINNED_POOL_MB", "2048")) << 20

    def empty(self, shape, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < self.MIN_BYTES:
            return np.empty(shape, dtype=dtype)
        capacity = (nbytes + (1 << 20) - 1) & ~((1 << 20) - 1)
        ptr = None
        evict = []
        with self._lock:
            # the smallest idle block that holds the request, if it is not more than twice as large
            # (snapshots of the dict: a block's __del__ may re-enter _give() on this thread -- garbage collection inside
            # the loop -- and add a capacity key: 'dictionary changed size during iteration')
            fits = sorted(c for c, stock in list(self._free.items()) if stock and capacity <= c <= 2 * capacity)
            if fits:
                capacity = fits[0]
                ptr = self._free[capacity].pop()
            else:
                if self._held + capacity > self._budget():  # idle blocks of other sizes make room first
                    for c in sorted(list(self._free), reverse=True):
                        while self._free[c] and self._held + capacity > self._budget():
                            evict.append(self._free[c].pop())
                            self._held -= c
                if self._held + capacity <= self._budget():
                    self._held += capacity
                    ptr = 0  # allocate outside the lock
        if evict:
            lib = _load()
            for p in evict:
                lib.ptk_host_free(p)
        if ptr is None:
            return np.empty(shape, dtype=dtype)
        if ptr == 0:
            out = c_void_p()
            if _load().ptk_host_alloc(capacity, byref(out)) != PTK_OK or not out.value:
                with self._lock:
                    self._held -= capacity
                return np.empty(shape, dtype=dtype)
            ptr = out.value
        block = _PinnedBlock(self, ptr, capacity, nbytes)
        return np.asarray(block).view(dtype).reshape(shape)

    def _give(self, ptr: int, capacity: int) -> None:
        try:
            with self._lock:
                self._free.setdefault(capacity, []).append(ptr)
        except Exception:  # (interpreter shutdown)
            pass

    def trim(self) -> None:
        """Frees the blocks that are not in use."""
        with self._lock:
            free, self._free = self._free, {}
            for capacity, stock in list(free.items()):
                self._held -= capacity * len(stock)
        lib = _load()
        for stock in free.values():
            for ptr in stock:
                lib.ptk_host_free(ptr)


_pinned_pool = _PinnedPool()


def set_test_knobs(**knobs) -> None:
    """Test hooks of libptk.so: ``set_test_knobs(knn_cap=4, knn_cap_min_nq=1)`` writes ``name=value`` pairs into the
    environment variable ``PTK_TEST_KNOBS`` (the library reads it on every call); ``name=None`` removes one,
    ``set_test_knobs()`` with no arguments removes all.  The hooks force a path a test wants to see taken (a cap on every
    batch, one of the two sorts, the hand-over list of a small batch ...); DESIGN.md section 11 lists them."""
    if not knobs:
        os.environ.pop("PTK_TEST_KNOBS", None)
        return
    have = dict(item.split("=", 1) for item in os.environ.get("PTK_TEST_KNOBS", "").split(",") if "=" in item)
    for name, value in knobs.items():
        if value is None:
            have.pop(name, None)
        else:
            have[name] = str(int(value))
    if have:
        os.environ["PTK_TEST_KNOBS"] = ",".join(f"{k}={v}" for k, v in have.items())
    else:
        os.environ.pop("PTK_TEST_KNOBS", None)


def trim_pinned_pool() -> None:
    """Frees the page-locked result blocks that no array uses any more (the pool keeps them for the next call)."""
    _pinned_pool.trim()


class registered:
    """``with pico_tree_amd.registered(arr): ...`` page-locks a numpy array the caller owns for the duration of the
    block (``ptk_host_register`` / ``ptk_host_unregister``): searches inside move it without a staging copy.  For arrays
    that live long -- the buffers of a stream of scans; registering costs more than one staged copy."""

    def __init__(self, arr: np.ndarray):
        if not isinstance(arr, np.ndarray) or not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("a C-contiguous numpy array is required")
        self._arr = arr
        self._on = False

    def __enter__(self):
        _check(_load().ptk_host_register(self._arr.ctypes.data, self._arr.nbytes))
        self._on = True
        return self._arr

    def __exit__(self, *exc):
        if self._on:
            self._on = False
            _check(_load().ptk_host_unregister(self._arr.ctypes.data))
        return False


def empty_pinned(shape, dtype=np.float32) -> np.ndarray:
    """An uninitialised numpy array in page-locked host memory (``ptk_host_alloc``): query arrays kept in one are
    uploaded without staging.  Small arrays (< 1 MiB) are ordinary numpy arrays."""
    return _pinned_pool.empty(shape, dtype)


class Metric(enum.Enum):
    """Metrics of the reference binding (``def_kd_tree.cpp:14-17``) plus ``LNInf``, which the reference
    has in C++ only (``metric_lninf``, metric.hpp:157-186).  ``L2Squared`` takes the tuned kernels; the
    others run the generic kernels with the metric swapped in."""
    L1 = 1
    L2Squared = 2
    LPInf = 3
    LNInf = 4
    #: the reference's topological metrics (C++ only there, metric.hpp:186-257): points on the circle
    #: [0, 1] / 0 ~ 1 (1-D), and planar poses x, y, angle (3-D).  float32; knn and radius searches.
    SO2 = 5
    SE2Squared = 6


_PTK_METRIC = {Metric.L2Squared: 0, Metric.L1: 1, Metric.LPInf: 2, Metric.LNInf: 3, Metric.SO2: 4,
               Metric.SE2Squared: 5}  # PTK_METRIC_* of ptk.h


class _LibraryBuffer:
    """Owner of a result buffer malloc'ed by libptk: frees it (``ptk_free``) when the last numpy view
    of it is gone."""

    def __init__(self, lib, ptr):
        self._lib, self._ptr = lib, ptr

    def __del__(self):
        try:
            self._lib.ptk_free(self._ptr)
        except Exception:
            pass


def _adopt(lib, ptr: c_void_p, count: int, dtype) -> np.ndarray:
    """The library's ragged result as a numpy array WITHOUT copying it (a radius batch of BASELINE
    config 3 is 6 GB of rows): the array keeps the buffer alive through a ``_LibraryBuffer``."""
    dtype = np.dtype(dtype)
    if count == 0 or not ptr.value:
        lib.ptk_free(ptr)
        return np.empty(0, dtype=dtype)
    raw = (ctypes.c_char * (count * dtype.itemsize)).from_address(ptr.value)
    raw._owner = _LibraryBuffer(lib, ptr)  # the ctypes object is the base of the array below
    return np.frombuffer(raw, dtype=dtype, count=count)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _is_scalar_radius(radius) -> bool:
    """One radius for the batch (a number, a 0-d array or tensor) rather than an array of one per query."""
    if _is_torch(radius):
        return radius.dim() == 0
    return np.ndim(radius) == 0


class DArray:
    """Ragged result of a radius (or box) search: a sequence of numpy arrays.

    Same role and constructor as the reference's ``DArray``
    (``_pyco_tree/darray.hpp:31-288``, ``def_darray.cpp``): ``DArray(dtype)`` makes an
    empty one to be filled by ``search_radius(..., nns)``; it is a sequence (``len``,
    indexing incl. negative indices and slices, iteration, truthiness).  Stored flat:
    row ``i`` is ``flat[offsets[i]:offsets[i + 1]]`` (a view, no copy).
    """

    def __init__(self, dtype=None, flat=None, *, offsets=None):
        if isinstance(dtype, np.ndarray) and isinstance(flat, np.ndarray):
            offsets, dtype = dtype, None  # DArray(offsets, flat): the internal form
        if flat is None:
            dt = np.dtype(dtype if dtype is not None else NEIGHBOR)
            if dt != NEIGHBOR and dt != NEIGHBOR64 and dt != np.dtype(np.int32):
                raise ValueError("unexpected dtype for DArray")
            flat = np.empty(0, dtype=dt)
            offsets = np.zeros(1, dtype=np.uint64)
        self.offsets = offsets
        self.flat = flat

    @property
    def dtype(self):
        return self.flat.dtype

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def __bool__(self) -> bool:
        return len(self) > 0

    def __getitem__(self, i):
        n = len(self)
        if isinstance(i, slice):
            rows = [self[j] for j in range(*i.indices(n))]
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            if rows:
                off[1:] = np.cumsum([len(r) for r in rows])
            flat = np.concatenate(rows) if rows else np.empty(0, dtype=self.dtype)
            return DArray(off, flat.astype(self.dtype, copy=False))
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return self.flat[int(self.offsets[i]):int(self.offsets[i + 1])]

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def _assign(self, offsets: np.ndarray, flat: np.ndarray) -> None:
        """Takes a new result; storage is kept when the total size is unchanged (the
        reference re-uses each row's memory when its size allows, darray.hpp)."""
        if flat.dtype != self.flat.dtype:
            raise ValueError("unexpected dtype_neighbor for data")
        if len(flat) == len(self.flat) and len(flat) > 0:
            np.copyto(self.flat, flat)
        else:
            self.flat = flat
        self.offsets = offsets


class DeviceNeighbors:
    """k-NN result resident on the device: ``raw`` is int32 ``(nq, k, 2)`` -- (index, bits of the
    float32 distance) -- for a float32 tree and int64 ``(nq, k, 2)`` -- (index, bits of the float64
    distance) -- for a float64 tree (the 16-byte ``neighbor<int, double>`` record)."""

    def __init__(self, raw):
        self.raw = raw

    @property
    def index(self):
        return self.raw[..., 0]

    @property
    def distance(self):
        import torch
        return self.raw[..., 1].view(torch.float64 if self.raw.dtype == torch.int64 else torch.float32)

    def numpy(self) -> np.ndarray:
        """Host copy with the :data:`NEIGHBOR` (or :data:`NEIGHBOR64`) dtype, shape ``(nq,)`` or ``(nq, k)``."""
        a = self.raw.cpu().numpy()
        out = np.ascontiguousarray(a).view(NEIGHBOR64 if a.dtype == np.int64 else NEIGHBOR)[..., 0]
        return out[:, 0] if out.shape[1] == 1 else out


class KdTree:
    """A kd-tree over float32 or float64 points, searched on the MI355X.

    ``KdTree(pts, Metric.L2Squared, max_leaf_size)`` as in the reference.  ``pts``
    is ``(npts, sdim)`` C-contiguous (an F-contiguous ``(sdim, npts)`` array is the
    same memory and accepted like the reference does); its dtype selects the
    instantiation like the reference's dispatch does (_pyco_tree/kd_tree.hpp:383-445):
    float32 -> the tuned kernels (``ptk_*``), float64 -> the double-precision
    kernels (``ptk_tree64_*`` / ``ptk_search64_*``, results ``NEIGHBOR64``).  The tree
    is built on the host with the sliding-midpoint rule and uploaded once.

    The points must be finite: a NaN or +-Inf coordinate raises :class:`PtkError` (``PTK_ERR_INVALID``, the message
    names the first offending point); +-FLT_MAX is accepted.  ``load_kd_tree`` does not look at the points.
    """

    def __init__(self, pts, metric: Metric = Metric.L2Squared, max_leaf_size: int = 10,
                 device: int | None = None, _stream: bytes | None = None):
        if not isinstance(metric, Metric):
            raise TypeError("metric must be a pico_tree_amd.Metric")
        self._metric = metric
        if isinstance(pts, np.ndarray) and pts.dtype == np.float64:
            self._dtype, self._neighbor, self._f64 = np.dtype(np.float64), NEIGHBOR64, True
        else:
            self._dtype, self._neighbor, self._f64 = np.dtype(np.float32), NEIGHBOR, False
        self._real = np.float64 if self._f64 else np.float32
        self._given = pts  # in the caller's own layout (row- or column-major), for __array__
        pts = self._as_matrix(pts, None, "pts", self._dtype)
        if int(max_leaf_size) <= 0:
            raise ValueError("max_leaf_size must be positive")
        self._pts = pts  # keep alive, like py::keep_alive<1, 2>
        self._npts, self._sdim = pts.shape
        self._max_leaf_size = int(max_leaf_size)
        lib = _load()
        handle = c_void_p()
        dev = PTK_DEVICE_CURRENT if device is None else int(device)
        self._fn = (lambda name: getattr(lib, name.replace("ptk_tree_", "ptk_tree64_").replace("ptk_search_", "ptk_search64_"))) \
            if self._f64 else (lambda name: getattr(lib, name))
        if _stream is None:
            _check(self._fn("ptk_tree_create_from_points")(pts.ctypes.data, self._npts, self._sdim,
                                                           self._max_leaf_size, dev, byref(handle)))
        else:  # load_kd_tree: the tree comes from a saved stream
            buf = ctypes.create_string_buffer(_stream, len(_stream))
            # (a tree over a topological space is written with four bounds per branch, kd_tree_node.hpp:52-67)
            entry = "ptk_tree_create_from_topological_stream" if self._topological() else "ptk_tree_create_from_stream"
            _check(self._fn(entry)(pts.ctypes.data, self._npts, self._sdim, buf, len(_stream), dev, byref(handle)))
        self._h = handle
        if metric is not Metric.L2Squared:
            _check(self._fn("ptk_tree_set_metric")(handle, _PTK_METRIC[metric]))

    def __array__(self, dtype=None, copy=None):
        """The tree as a read-only view of its points, shaped as they were given -- ``(npts, sdim)`` for
        row-major input, ``(sdim, npts)`` for column-major input: the reference exposes exactly this
        through the buffer protocol (``def_kd_tree.cpp:30-33``, ``_pyco_tree/kd_tree.hpp:292-315``) to
        show how the data is interpreted.  ``np.asarray(tree)`` does not copy."""
        v = self._given.view()
        v.flags.writeable = False
        if dtype is not None and np.dtype(dtype) != v.dtype:
            return v.astype(dtype)
        return v.copy() if copy else v

    @property
    def metric_string(self) -> str:  # core.hpp:24-38
        return self._metric.name

    def _topological(self) -> bool:
        return self._metric.name in ("SO2", "SE2Squared")

    def _serialize(self) -> bytes:
        entry = "ptk_tree_serialize_topological" if self._topological() else "ptk_tree_serialize"
        size = c_uint64()
        _check(self._fn(entry)(self._h, None, 0, byref(size)))
        buf = ctypes.create_string_buffer(size.value)
        _check(self._fn(entry)(self._h, buf, size.value, byref(size)))
        return buf.raw[:size.value]

    # -- helpers ---------------------------------------------------------------
    @staticmethod
    def _as_matrix(a, sdim, what, dtype=np.float32):
        """Validates like py_array_map.hpp:37-62 and returns a C-order view."""
        if not isinstance(a, np.ndarray):
            raise ValueError(f"{what} must be a numpy array")
        if a.dtype != dtype:
            raise ValueError("unexpected dtype_scalar for data")
        if a.ndim != 2:
            raise ValueError(f"{what} must have 2 dimensions")
        if a.flags.c_contiguous:
            m = a
        elif a.flags.f_contiguous:
            m = a.T  # (sdim, npts) column-major is (npts, sdim) row-major memory
        else:
            raise ValueError(f"{what} must be contiguous")
        if sdim is not None and m.shape[1] != sdim:
            raise ValueError(f"{what} has spatial dimension {m.shape[1]}, tree has {sdim}")
        return m

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._fn("ptk_tree_destroy")(h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self) -> str:  # _pyco_tree/kd_tree.hpp:321-326
        return f"KdTree(metric={self._metric.name}, dtype={self._dtype.name}, sdim={self._sdim}, npts={self._npts})"

    # -- properties (names of the reference binding) ----------------------------------
    @property
    def npts(self) -> int:
        return self._npts

    @property
    def sdim(self) -> int:
        return self._sdim

    @property
    def dtype_index(self):
        return np.dtype(np.int32)

    @property
    def dtype_scalar(self):
        return self._dtype

    @property
    def dtype_neighbor(self):
        return self._neighbor

    def metric(self, scalar: float) -> float:
        """The metric's one-dimensional form in the tree's scalar type: ``x * x`` for L2Squared, ``|x|``
        for L1 and LPInf (metric.hpp:95-98, :120-123, :147-150)."""
        x = self._real(scalar)
        return float(x * x) if self._metric in (Metric.L2Squared, Metric.SE2Squared) else float(abs(x))

    def info(self) -> dict:
        inf = _Info()
        _check(self._fn("ptk_tree_get_info")(self._h, byref(inf)))
        return {name: getattr(inf, name) for name, _ in _Info._fields_}

    def _float32_only(self, what):
        if self._f64:
            raise PtkError(-2, f"{what} is available for float32 trees only")

    def flat(self):
        """(nodes uint32[n_nodes, 4], indices int32[npts], root_min, root_max)."""
        self._float32_only("flat()")
        inf = self.info()
        nodes = np.empty((inf["n_nodes"], 4), dtype=np.uint32)
        indices = np.empty(self._npts, dtype=np.int32)
        rmin = np.empty(self._sdim, dtype=np.float32)
        rmax = np.empty(self._sdim, dtype=np.float32)
        _check(_load().ptk_tree_get_flat(self._h, nodes.ctypes.data, indices.ctypes.data,
                                         rmin.ctypes.data, rmax.ctypes.data))
        return nodes, indices, rmin, rmax

    def set_reorder(self, mode: int) -> None:
        if self._f64:
            return  # the double-precision kernels take the batch in the caller's order
        _check(_load().ptk_tree_set_reorder(self._h, int(mode)))

    def profile(self, enable: bool | None = None, reset: bool = False) -> dict:
        self._float32_only("profile()")
        lib = _load()
        if enable is not None:
            _check(lib.ptk_profile_enable(self._h, int(enable)))
        p = _Profile()
        _check(lib.ptk_profile_get_sized(self._h, byref(p), ctypes.sizeof(p), int(reset)))
        return {name: getattr(p, name) for name, _ in _Profile._fields_}

    def create_phases(self) -> dict:
        """Where the creation of the handle went, in seconds (``ptk_debug_create_phases``)."""
        self._float32_only("create_phases()")
        ms = (c_double * 3)()
        _check(_load().ptk_debug_create_phases(self._h, ms))
        return {"host_build_s": ms[0] / 1e3, "encode_s": ms[1] / 1e3, "upload_s": ms[2] / 1e3}

    def create_route(self) -> dict:
        """How the tree of the handle was built (``ptk_debug_create_route``): ``on_device`` = 1 when the partitions of
        the top levels were made on the device, else ``why`` names what sent the build to the host; the counters of
        the device build (levels, branches of the top, subtrees below it, planes that slid and where)."""
        self._float32_only("create_route()")
        c = (ctypes.c_uint64 * 8)()
        why = ctypes.c_char_p()
        _check(_load().ptk_debug_create_route(self._h, c, byref(why)))
        names = ("on_device", "threshold", "levels", "top_branches", "subtrees", "slides", "slide_rounds_device",
                 "slides_host_whole")
        route = {name: int(v) for name, v in zip(names, c)}
        route["why"] = (why.value or b"").decode("utf-8", "replace")
        return route

    def knn1_counts(self) -> dict:
        """Counters of the last two-phase k = 1 search (``ptk_debug_knn1_counts``)."""
        self._float32_only("knn1_counts()")
        c = (c_uint32 * 4)()
        _check(_load().ptk_debug_knn1_counts(self._h, c))
        return {"phase2": int(c[0]), "cooperative": int(c[1]), "redone": int(c[2]), "dealt": int(c[3])}

    def knn_coop_counts(self) -> dict:
        """After a search with 1 < k <= 56: queries the general kernel handed to the cooperative search, queries that
        search sent to the redo list and why (``ptk_debug_knn_coop_counts``)."""
        c = (c_uint32 * 7)()
        if self._f64:
            _check(_load().ptk_tree64_debug_knn_coop_counts(self._h, c))
        else:
            _check(_load().ptk_debug_knn_coop_counts(self._h, c))
        return {"cooperative": int(c[0]), "redone": int(c[1]), "pool": int(c[2]), "ties": int(c[3]), "box": int(c[4]),
                "range": int(c[5]), "tie_sweeps": int(c[6])}

    def radius_coop_counts(self) -> dict:
        """After a radius count pass on the device (``search_radius_device`` / the count half of ``search_radius``):
        queries the list pass handed to a wavefront, rows recounted from the root, leaf entries kept for the fill pass
        (``ptk_debug_radius_coop_counts``)."""
        self._float32_only("radius_coop_counts()")
        c = (c_uint32 * 3)()
        _check(_load().ptk_debug_radius_coop_counts(self._h, c))
        return {"cooperative": int(c[0]), "recounted": int(c[1]), "entries": int(c[2])}

    def piles(self) -> dict:
        """Subtrees of coincident points of the device replica (``ptk_debug_piles``): how many, the points they hold,
        the depth of what a k = 1 search of the default metric traverses."""
        self._float32_only("piles()")
        c = (ctypes.c_uint64 * 3)()
        _check(_load().ptk_debug_piles(self._h, c))
        return {"piles": int(c[0]), "points": int(c[1]), "knn1_depth": int(c[2])}

    def batch_permutation(self, q):
        """The order the rows of a device batch would be searched in (``ptk_debug_batch_permutation``): a uint32 torch
        tensor, entry i = the row searched i-th."""
        import torch

        self._float32_only("batch_permutation()")
        perm = torch.empty((q.shape[0],), dtype=torch.int32, device=q.device)
        _check(_load().ptk_debug_batch_permutation(self._h, q.data_ptr(), q.shape[0], perm.data_ptr()))
        return perm

    def batch_order(self) -> int:
        """What the last search did with the order of its batch: 0 as it came, 1 sorted on the device, 2 found
        coherent and left alone (``ptk_debug_batch_order``)."""
        self._float32_only("batch_order()")
        how = c_int(0)
        _check(_load().ptk_debug_batch_order(self._h, byref(how)))
        return int(how.value)

    def deep_pieces(self) -> int:
        """Launches of the last pass of a search on a tree deeper than the private stack classes, whose batch runs in
        pieces (``ptk_debug_deep_pieces``); 0 if there was none."""
        self._float32_only("deep_pieces()")
        n = c_uint32(0)
        _check(_load().ptk_debug_deep_pieces(self._h, byref(n)))
        return int(n.value)

    def key_bits(self, nq: int) -> tuple:
        """Bits of the Morton key per axis for a batch of ``nq`` queries (``ptk_debug_key_bits``)."""
        self._float32_only("key_bits()")
        b = (c_uint32 * 3)()
        _check(_load().ptk_debug_key_bits(self._h, int(nq), b))
        return int(b[0]), int(b[1]), int(b[2])

    # -- k nearest neighbours ------------------------------------------------------------
    def search_knn(self, pts, k: int, *args):
        """``search_knn(pts, k[, e][, nns])`` -- the four reference overloads.

        Host arrays return (or fill) a numpy array of :data:`NEIGHBOR`; a torch
        CUDA tensor returns a :class:`DeviceNeighbors` (``nns`` may be a
        preallocated int32 ``(nq, k, 2)`` tensor).

        A query row with NaN, +-Inf or any finite value (one whose distances overflow included) gets what the
        reference gives it, for every entry the reference writes, and changes no other row.  A slot the reference's
        search never writes -- ``k > npts``; a row that accepts fewer than ``k`` points (a NaN or +-Inf row accepts
        none) -- holds ``(index 0, distance FLT_MAX)`` (``DBL_MAX`` for float64): no slot of the result is left
        unwritten, whatever ``nns`` held.
        """
        e, nns = self._split_optional(args)
        k = int(k)
        if _is_torch(pts):
            return self._search_knn_device(pts, k, e, nns)
        q = self._as_matrix(pts, self._sdim, "pts", self._dtype)
        nq = q.shape[0]
        shape = (nq,) if k == 1 else ((nq, k) if pts.flags.c_contiguous else (k, nq))
        NB = self._neighbor
        if nns is None:
            # (float64 records carry 4 bytes of padding, zeroed; float32 rows land in a page-locked block of the pool)
            nns = np.zeros(shape, dtype=NB) if self._f64 else _pinned_pool.empty(shape, NB)
        elif not isinstance(nns, np.ndarray) or nns.dtype != NB:
            raise ValueError("unexpected dtype_neighbor for data")
        elif nns.size != nq * k or not nns.flags.c_contiguous:
            # Resized like ensure_size() of the reference (kd_tree.hpp:362-378).
            try:
                nns.resize(shape, refcheck=False)
            except ValueError:
                nns = np.empty(shape, dtype=NB)
        search = self._fn("ptk_search_knn")
        if k > 1 and not pts.flags.c_contiguous:
            # Column-major callers get the transposed (k, npts) layout of the reference
            # (kd_tree.hpp:362-378): row i of the search is column i of the output.
            tmp = np.empty((nq, k), dtype=NB)
            self._served(search(self._h, q.ctypes.data, nq, k, self._real(e), tmp.ctypes.data),
                         lambda lib: lib.ptk_host_search_knn(self._h, self._pts.ctypes.data, q.ctypes.data, nq, k,
                                                             np.float32(e), tmp.ctypes.data))
            nns.reshape(-1)[:] = tmp.reshape(-1)
            return nns
        self._served(search(self._h, q.ctypes.data, nq, k, self._real(e), nns.ctypes.data),
                     lambda lib: lib.ptk_host_search_knn(self._h, self._pts.ctypes.data, q.ctypes.data, nq, k,
                                                         np.float32(e), nns.ctypes.data))
        return nns

    def search_knn_within(self, pts, k: int, radius: float, nns=None):
        """``search_knn_within(pts, k, radius[, nns])`` -- the k nearest points closer than ``radius``.

        Row i is :meth:`search_knn`'s row of ``min(k, npts)`` entries, keeping only the entries with
        distance ``< radius`` (metric units: squared for L2 squared), padded to k entries with
        ``(index -1, distance radius)`` (``ptk_search_knn_within`` / ``ptk_search64_knn_within``).  Exact;
        float32 and float64 trees.  Layouts as :meth:`search_knn`: host arrays give numpy rows (``(k, nq)`` for
        column-major queries), a torch CUDA tensor gives a :class:`DeviceNeighbors`.

        ``radius`` may also be a 1-D array of ``nq`` radii, one per query row (``ptk_search_knn_within_radii``): row i
        is then the row the scalar call gives with ``radius[i]``.  Host queries take any array-like (converted to the
        tree's dtype; a NaN or negative entry raises); torch CUDA queries take a contiguous CUDA tensor of the tree's
        dtype on the same device (not inspected: a row whose radius is NaN or negative is all padding).
        """
        k = int(k)
        radii = None if _is_scalar_radius(radius) else radius
        r = self._real(radius) if radii is None else None
        NB = self._neighbor
        if _is_torch(pts):
            import torch
            tq, traw = (torch.float64, torch.int64) if self._f64 else (torch.float32, torch.int32)
            if pts.dtype != tq or pts.dim() != 2 or pts.shape[1] != self._sdim:
                raise ValueError(f"queries must be a {self._dtype.name} (nq, sdim) tensor")
            if not pts.is_cuda or not pts.is_contiguous():
                raise ValueError("queries must be a contiguous CUDA tensor")
            nq = pts.shape[0]
            out = nns.raw if isinstance(nns, DeviceNeighbors) else nns
            if out is None:
                # (float64: the records carry 4 bytes of padding, zeroed so that index reads as an int64)
                out = (torch.zeros if self._f64 else torch.empty)((nq, k, 2), dtype=traw, device=pts.device)
            if out.dtype != traw or tuple(out.shape) != (nq, k, 2) or not out.is_contiguous():
                raise ValueError(f"nns must be a contiguous {traw} (nq, k, 2) tensor")
            if radii is not None:
                radii = self._device_radii(radii, pts, nq)
            stream = torch.cuda.current_stream(pts.device).cuda_stream
            if radii is not None:
                _check(self._fn("ptk_search_knn_within_radii_device")(self._h, pts.data_ptr(), nq, k, radii.data_ptr(),
                                                                     out.data_ptr(), stream))
                return DeviceNeighbors(out)
            _check(self._fn("ptk_search_knn_within_device")(self._h, pts.data_ptr(), nq, k, r, out.data_ptr(), stream))
            return DeviceNeighbors(out)
        q = self._as_matrix(pts, self._sdim, "pts", self._dtype)
        nq = q.shape[0]
        if radii is not None:
            radii = self._host_radii(radii, nq)
        shape = (nq,) if k == 1 else ((nq, k) if pts.flags.c_contiguous else (k, nq))
        if nns is None:
            nns = np.zeros(shape, dtype=NB) if self._f64 else np.empty(shape, dtype=NB)
        elif not isinstance(nns, np.ndarray) or nns.dtype != NB:
            raise ValueError("unexpected dtype_neighbor for data")
        elif nns.size != nq * k or not nns.flags.c_contiguous:
            try:
                nns.resize(shape, refcheck=False)
            except ValueError:
                nns = np.zeros(shape, dtype=NB)
        # (column-major callers: row i of the search is column i of the output, as search_knn)
        rows = nns if k == 1 or pts.flags.c_contiguous else np.zeros((nq, k), dtype=NB)
        if radii is not None:
            self._served(self._fn("ptk_search_knn_within_radii")(self._h, q.ctypes.data, nq, k, radii.ctypes.data,
                                                                rows.ctypes.data),
                         lambda lib: lib.ptk_host_search_knn_within_radii(self._h, self._pts.ctypes.data, q.ctypes.data,
                                                                          nq, k, radii.ctypes.data, rows.ctypes.data))
        else:
            self._served(self._fn("ptk_search_knn_within")(self._h, q.ctypes.data, nq, k, r, rows.ctypes.data),
                         lambda lib: lib.ptk_host_search_knn_within(self._h, self._pts.ctypes.data, q.ctypes.data, nq, k,
                                                                    np.float32(radius), rows.ctypes.data))
        if rows is not nns:
            nns.reshape(-1)[:] = rows.reshape(-1)
        return nns

    def self_route(self, k: int) -> int:
        """Which route :meth:`search_knn_self` takes for ``k`` on this tree: 1 the direct kernel, 2 the staged route
        (``ptk_debug_self_route``; a float64 tree always takes the staged route)."""
        if self._f64:
            return 2
        route = c_int(0)
        _check(_load().ptk_debug_self_route(self._h, int(k), byref(route)))
        return int(route.value)

    def search_knn_self(self, k: int, nns=None, device: bool = False):
        """``search_knn_self(k[, nns], device=False)`` -- each tree point's k nearest OTHER points.

        Row i belongs to point i of the tree.  It is :meth:`search_knn`'s row of ``min(k + 1, npts)`` entries for that
        point with one entry removed -- the first whose index is i, else (``k + 1`` or more other points coincide with
        it and come first) the last --, padded to k entries with ``(index -1, distance FLT_MAX)`` (``DBL_MAX`` for
        float64).  Exact; float32 and float64 trees; no query array: the tree holds its points on the device
        (``ptk_search_knn_self`` / ``ptk_search64_knn_self``).

        Returns numpy rows of :attr:`dtype_neighbor`, ``(npts, k)`` or ``(npts,)`` for ``k == 1``.  With
        ``device=True``, or a torch CUDA tensor / :class:`DeviceNeighbors` as ``nns``, the rows stay on the device
        (a :class:`DeviceNeighbors`, on the current torch stream).  :meth:`self_route` says whether the call only
        enqueues (1) or allocates and waits (2).
        """
        k = int(k)
        n = self._npts
        NB = self._neighbor
        if device or isinstance(nns, DeviceNeighbors) or _is_torch(nns):
            import torch
            traw = torch.int64 if self._f64 else torch.int32
            out = nns.raw if isinstance(nns, DeviceNeighbors) else nns
            if out is None:
                dev = torch.device("cuda", int(self.info()["device"]))
                out = (torch.zeros if self._f64 else torch.empty)((n, max(k, 0), 2), dtype=traw, device=dev)
            if not out.is_cuda or out.dtype != traw or tuple(out.shape) != (n, k, 2) or not out.is_contiguous():
                raise ValueError(f"nns must be a contiguous CUDA {traw} (npts, k, 2) tensor")
            stream = torch.cuda.current_stream(out.device).cuda_stream
            _check(self._fn("ptk_search_knn_self_device")(self._h, k, out.data_ptr(), stream))
            return DeviceNeighbors(out)
        shape = (n,) if k == 1 else (n, max(k, 0))
        if nns is None:
            nns = np.zeros(shape, dtype=NB) if self._f64 else np.empty(shape, dtype=NB)
        elif not isinstance(nns, np.ndarray) or nns.dtype != NB:
            raise ValueError("unexpected dtype_neighbor for data")
        elif nns.size != n * k or not nns.flags.c_contiguous:
            try:
                nns.resize(shape, refcheck=False)
            except ValueError:
                nns = np.zeros(shape, dtype=NB)
        self._served(self._fn("ptk_search_knn_self")(self._h, k, nns.ctypes.data),
                     lambda lib: lib.ptk_host_search_knn_self(self._h, self._pts.ctypes.data, k, nns.ctypes.data))
        return nns

    def count_within(self, pts, radius: float, max_count: int = 0):
        """``count_within(pts, radius, max_count=0)`` -- how many points lie closer than ``radius`` to each query.

        ``counts[i]`` is the length of :meth:`search_radius`'s row i (distance ``< radius``, metric units: squared for
        L2 squared), clamped to ``max_count`` when that is > 0 (``ptk_search_count_within`` /
        ``ptk_search64_count_within``).  Exact; the rows are never built.  Host arrays (row- or column-major, the
        tree's dtype) give an ``int64[nq]`` array; a torch CUDA tensor gives an ``int64`` tensor on its device, enqueued
        on the current stream.

        ``radius`` may also be a 1-D array of ``nq`` radii, one per query row (``ptk_search_count_within_radii``), as for
        :meth:`search_knn_within`; ``max_count`` stays one value.  The device serves that form for trees of up to three
        dimensions and the four non-topological metrics; the rest is refused (``allow_host_loop`` serves float32 trees).
        """
        radii = None if _is_scalar_radius(radius) else radius
        r = self._real(radius) if radii is None else None
        max_count = int(max_count)
        if max_count < 0:
            raise ValueError("max_count must be >= 0")
        if _is_torch(pts):
            import torch
            tq = torch.float64 if self._f64 else torch.float32
            if pts.dtype != tq or pts.dim() != 2 or pts.shape[1] != self._sdim:
                raise ValueError(f"queries must be a {self._dtype.name} (nq, sdim) tensor")
            if not pts.is_cuda or not pts.is_contiguous():
                raise ValueError("queries must be a contiguous CUDA tensor")
            nq = pts.shape[0]
            out = torch.empty((nq,), dtype=torch.int64, device=pts.device)
            if radii is not None:
                radii = self._device_radii(radii, pts, nq)
            stream = torch.cuda.current_stream(pts.device).cuda_stream
            if radii is not None:
                _check(self._fn("ptk_search_count_within_radii_device")(self._h, pts.data_ptr(), nq, radii.data_ptr(),
                                                                       max_count, out.data_ptr(), stream))
                return out
            _check(self._fn("ptk_search_count_within_device")(self._h, pts.data_ptr(), nq, r, max_count, out.data_ptr(),
                                                             stream))
            return out
        q = self._as_matrix(pts, self._sdim, "pts", self._dtype)
        nq = q.shape[0]
        counts = np.zeros((nq,), dtype=np.int64)
        if radii is not None:
            radii = self._host_radii(radii, nq)
            self._served(self._fn("ptk_search_count_within_radii")(self._h, q.ctypes.data, nq, radii.ctypes.data, max_count,
                                                                  counts.ctypes.data),
                         lambda lib: lib.ptk_host_search_count_within_radii(self._h, self._pts.ctypes.data, q.ctypes.data,
                                                                            nq, radii.ctypes.data, max_count,
                                                                            counts.ctypes.data))
            return counts
        self._served(self._fn("ptk_search_count_within")(self._h, q.ctypes.data, nq, r, max_count, counts.ctypes.data),
                     lambda lib: lib.ptk_host_search_count_within(self._h, self._pts.ctypes.data, q.ctypes.data, nq,
                                                                  np.float32(radius), max_count, counts.ctypes.data))
        return counts

    def _self_radii(self, radius, device: bool):
        """(scalar, radii) of a self search: one radius (radii None), or one per tree point by original index -- a host
        array of the tree's dtype, or with ``device`` a contiguous CUDA tensor on the tree's device (a host array-like
        is checked for NaN / negative entries here and uploaded)."""
        if _is_scalar_radius(radius):
            return self._real(radius), None
        n = self._npts
        if not device:
            return self._real(0), self._host_radii(radius, n)
        import torch
        dev = torch.device("cuda", int(self.info()["device"]))
        if not (_is_torch(radius) and radius.is_cuda):
            host = self._host_radii(radius, n)
            bad = np.flatnonzero(~(host >= 0))
            if len(bad):
                raise ValueError(f"radius[{int(bad[0])}] must be >= 0 (and not NaN)")
            return self._real(0), torch.from_numpy(host).to(dev)
        tq = torch.float64 if self._f64 else torch.float32
        if radius.device != dev:
            raise ValueError(f"radius must be on the tree's device ({dev}), not on {radius.device}")
        if radius.dtype != tq:
            raise ValueError(f"radius must be a {self._dtype.name} tensor, not {radius.dtype}")
        if radius.dim() != 1 or radius.shape[0] != n:
            raise ValueError(f"radius must be a scalar or a 1-D tensor of {n} radii, one per tree point")
        if not radius.is_contiguous():
            raise ValueError("radius must be a contiguous tensor")
        return self._real(0), radius

    def count_within_self(self, radius, max_count: int = 0, device: bool = False):
        """``count_within_self(radius, max_count=0, device=False)`` -- how many OTHER tree points lie closer than
        ``radius`` to each tree point.

        ``counts[i]`` is the length of :meth:`search_radius_self`'s row i, clamped to ``max_count`` when that is > 0
        (the clamp applies after the point itself has left).  ``radius`` is a scalar or an array of ``npts`` radii
        indexed by original point index.  No query array: the tree holds its points on the device
        (``ptk_search_count_within_self`` / ``ptk_search64_count_within_self``).  Returns an ``int64[npts]`` array;
        with ``device=True`` an ``int64`` CUDA tensor on the tree's device, enqueued on the current torch stream (a
        CUDA tensor of radii is taken as it is: a NaN or negative entry gives count 0).  Served where
        :meth:`count_within` with an array is; the rest is refused (``allow_host_loop`` serves float32 trees)."""
        max_count = int(max_count)
        if max_count < 0:
            raise ValueError("max_count must be >= 0")
        r, radii = self._self_radii(radius, device)
        n = self._npts
        if device:
            import torch
            dev = torch.device("cuda", int(self.info()["device"]))
            out = torch.empty((n,), dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(self._fn("ptk_search_count_within_self_device")(
                self._h, r, radii.data_ptr() if radii is not None else None, max_count, out.data_ptr(), stream))
            return out
        counts = np.zeros((n,), dtype=np.int64)
        rp = radii.ctypes.data if radii is not None else None
        self._served(self._fn("ptk_search_count_within_self")(self._h, r, rp, max_count, counts.ctypes.data),
                     lambda lib: lib.ptk_host_search_count_within_self(self._h, self._pts.ctypes.data, r, rp, max_count,
                                                                       counts.ctypes.data))
        return counts

    def search_radius_self(self, radius, sort: bool = False, device: bool = False):
        """``search_radius_self(radius, sort=False, device=False)`` -- each tree point's neighbours within ``radius``
        among the OTHER points of the tree.

        Row i is :meth:`search_radius`'s row for point i (exact, strict ``distance < radius``) without the entry whose
        index is i, if there is one; the other entries keep their order (traversal order, or ascending distance with
        ``sort``); coincident other points stay at distance 0.  ``radius`` is a scalar or an array of ``npts`` radii
        indexed by original point index; a NaN or negative value is refused (by its row).  No query array
        (``ptk_search_radius_self`` / ``ptk_search64_radius_self``).  Returns a :class:`DArray`; with ``device=True``
        (float32 trees) ``(offsets int64 tensor [npts + 1], raw int32 tensor [total, 2])`` on the current torch stream,
        as :meth:`search_radius_device` (a NaN or negative entry of a CUDA tensor of radii gives an empty row).  Served
        where :meth:`count_within_self` is."""
        r, radii = self._self_radii(radius, device)
        n = self._npts
        lib = _load()
        if device:
            import torch
            self._float32_only("search_radius_self(device=True)")
            dev = torch.device("cuda", int(self.info()["device"]))
            stream = torch.cuda.current_stream(dev).cuda_stream
            rp = radii.data_ptr() if radii is not None else None
            counts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            _check(lib.ptk_search_count_within_self_device(self._h, r, rp, 0, counts.data_ptr(), stream))
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            offsets[1:] = torch.cumsum(counts[:n], 0)
            total = int(offsets[-1].item())
            out = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
            _check(lib.ptk_search_radius_self_fill_device(self._h, r, rp, offsets.data_ptr(), out.data_ptr(),
                                                          int(bool(sort)), stream))
            return offsets, out[:total]
        offsets = np.zeros(n + 1, dtype=np.uint64)
        rows = c_void_p()
        rp = radii.ctypes.data if radii is not None else None
        self._served(self._fn("ptk_search_radius_self")(self._h, r, rp, int(bool(sort)), offsets.ctypes.data, byref(rows)),
                     lambda lib: lib.ptk_host_search_radius_self(self._h, self._pts.ctypes.data, r, rp, int(bool(sort)),
                                                                 offsets.ctypes.data, byref(rows)))
        return DArray(offsets, _adopt(lib, rows, int(offsets[-1]), self._neighbor))

    def cluster_within_self(self, radius, min_neighbors: int = 0, compact: bool = False, device: bool = False):
        """``cluster_within_self(radius, min_neighbors=0, compact=False, device=False)`` -- the clusters of the tree's
        points: the connected components of the fixed-radius graph, with DBSCAN's core-point rule.

        With row i being :meth:`search_radius_self`'s row i: point i is *core* iff that row has at least
        ``min_neighbors`` entries (0: every point; DBSCAN's ``min_samples`` is ``min_neighbors + 1``); core points i and
        j are joined whenever j is in row i or i in row j.  A core point's label is the smallest original index among
        the core points of its component; a non-core point takes the smallest label among the core points of its own
        row, ``-1`` (noise) without one, and passes nothing on.  ``radius`` is a scalar or an array of ``npts`` radii
        indexed by original point index.  No rows are written (``ptk_cluster_within_self`` /
        ``ptk_search64_cluster_within_self``).  Returns an ``int32[npts]`` array; with ``device=True`` an ``int32`` CUDA
        tensor on the tree's device, enqueued on the current torch stream.  ``compact=True`` renumbers the clusters
        ``0..C-1`` in ascending order of their representative index; noise stays ``-1``.  Served where
        :meth:`count_within_self` is; the rest is refused (``allow_host_loop`` serves float32 trees)."""
        min_neighbors = int(min_neighbors)
        if min_neighbors < 0:
            raise ValueError("min_neighbors must be >= 0")
        r, radii = self._self_radii(radius, device)
        n = self._npts
        lib = _load()
        if device:
            import torch
            dev = torch.device("cuda", int(self.info()["device"]))
            out = torch.empty((n,), dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            fn = lib.ptk_search64_cluster_within_self_device if self._f64 else lib.ptk_cluster_within_self_device
            _check(fn(self._h, r, radii.data_ptr() if radii is not None else None, min_neighbors, out.data_ptr(), stream))
            if compact:
                _, inverse = torch.unique(out, sorted=True, return_inverse=True)
                # (the values ascend: a leading -1, if there is noise, takes rank 0)
                out = (inverse - (out.min() < 0).to(inverse.dtype)).to(torch.int32) if n else out
            return out
        labels = np.zeros((n,), dtype=np.int32)
        rp = radii.ctypes.data if radii is not None else None
        fn = lib.ptk_search64_cluster_within_self if self._f64 else lib.ptk_cluster_within_self
        self._served(fn(self._h, r, rp, min_neighbors, labels.ctypes.data, None),
                     lambda lib: lib.ptk_host_cluster_within_self(self._h, self._pts.ctypes.data, r, rp, min_neighbors,
                                                                  labels.ctypes.data, None))
        if compact and n:
            values, inverse = np.unique(labels, return_inverse=True)
            labels = (inverse.reshape(-1) - (1 if values[0] < 0 else 0)).astype(np.int32)
        return labels

    def normals_within_self(self, radius, min_neighbors: int = 2, viewpoint=None, moments: bool = False,
                            device: bool = False):
        """``normals_within_self(radius, min_neighbors=2, viewpoint=None, moments=False, device=False)`` -- the surface
        normal, curvature and covariance eigenvalues of every tree point's neighbourhood (PCA normals).

        The neighbourhood of point i is :meth:`search_radius_self`'s row i plus the point itself; its covariance is
        accumulated inside the traversal, no rows are written (``ptk_normals_within_self``).  Returns a structured
        array of dtype :data:`FRAME` by original point index: ``normal`` (unit length, the eigenvector of the smallest
        eigenvalue), ``curvature`` = l0 / (l0 + l1 + l2), ``eigenvalues`` (ascending) and ``count`` (the row's
        length).  A row shorter than ``max(min_neighbors, 2)`` gives NaN.  ``viewpoint`` (3 numbers) turns every normal
        towards it; without one the component of largest magnitude is positive.  ``radius`` is a scalar or an array
        of ``npts`` radii indexed by original point index.  With ``moments=True`` returns ``(frames, moments)``, the
        second of dtype :data:`MOMENTS`: the sums the covariance was made from.  With ``device=True`` the records are
        ``uint8`` CUDA tensors ``[npts, 32]`` / ``[npts, 48]`` on the tree's device, enqueued on the current torch
        stream.  float32 trees with three dimensions and a non-topological metric; served where
        :meth:`count_within_self` is, the rest is refused (``allow_host_loop`` serves deep trees)."""
        self._float32_only("normals_within_self")
        min_neighbors = int(min_neighbors)
        if min_neighbors < 0:
            raise ValueError("min_neighbors must be >= 0")
        view = None
        if viewpoint is not None:
            try:
                view = np.ascontiguousarray(viewpoint, dtype=np.float32)
            except (TypeError, ValueError) as ex:
                raise ValueError(f"viewpoint: not an array of numbers ({ex})") from None
            if view.shape != (3,):
                raise ValueError("viewpoint must hold 3 numbers")
        vp = view.ctypes.data if view is not None else None
        r, radii = self._self_radii(radius, device)
        n = self._npts
        lib = _load()
        if device:
            import torch
            dev = torch.device("cuda", int(self.info()["device"]))
            frames = torch.empty((n, FRAME.itemsize), dtype=torch.uint8, device=dev)
            mom = torch.empty((n, MOMENTS.itemsize), dtype=torch.uint8, device=dev) if moments else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib.ptk_normals_within_self_device(self._h, r, radii.data_ptr() if radii is not None else None,
                                                      min_neighbors, vp, frames.data_ptr(),
                                                      mom.data_ptr() if moments else None, stream))
            return (frames, mom) if moments else frames
        frames = np.zeros((n,), dtype=FRAME)
        mom = np.zeros((n,), dtype=MOMENTS) if moments else None
        mp = mom.ctypes.data if moments else None
        rp = radii.ctypes.data if radii is not None else None
        self._served(lib.ptk_normals_within_self(self._h, r, rp, min_neighbors, vp, frames.ctypes.data, mp),
                     lambda lib: lib.ptk_host_normals_within_self(self._h, self._pts.ctypes.data, r, rp, min_neighbors, vp,
                                                                  frames.ctypes.data, mp))
        return (frames, mom) if moments else frames

    def _aggregate_op(self, op, include_self: bool = False) -> int:
        try:
            code = _AGGREGATE_OPS[op]
        except (KeyError, TypeError):
            raise ValueError(f"op must be one of {sorted(_AGGREGATE_OPS)}, not {op!r}") from None
        return code | (PTK_AGG_INCLUDE_SELF if include_self else 0)

    def _aggregate_values(self, values, device):
        """(values as a contiguous float32 [npts, channels] array or CUDA tensor, channels, was it 1-D).  ``device``: None
        for a host call, else the torch device the tensor must live on."""
        n = self._npts
        if device is not None:
            import torch
            if not (_is_torch(values) and values.is_cuda):
                raise ValueError("values must be a CUDA tensor for a device call")
            if values.device != device:
                raise ValueError(f"values must be on {device}, not on {values.device}")
            if values.dtype != torch.float32:
                raise ValueError(f"values must be a float32 tensor, not {values.dtype}")
            if not values.is_contiguous():
                raise ValueError("values must be a contiguous tensor")
            shape = tuple(values.shape)
        else:
            if _is_torch(values):
                if values.is_cuda:
                    raise ValueError("values: a host call takes a host array, not a CUDA tensor")
                values = values.numpy()
            values = np.asarray(values)
            if values.dtype != np.float32:
                raise ValueError(f"values must be a float32 array, not {values.dtype}")
            values = np.ascontiguousarray(values)
            shape = values.shape
        if len(shape) not in (1, 2) or shape[0] != n:
            raise ValueError(f"values must have shape ({n},) or ({n}, channels), not {tuple(shape)}")
        flat = len(shape) == 1
        channels = 1 if flat else int(shape[1])
        if not 1 <= channels <= 1024:
            raise ValueError(f"values must hold 1 .. 1024 channels, not {channels}")
        return values, channels, flat

    def aggregate_within_self(self, radius, values, op: str = "sum", include_self: bool = False, counts: bool = False,
                              device: bool = False):
        """``aggregate_within_self(radius, values, op="sum", include_self=False, counts=False, device=False)`` -- the sum,
        minimum or maximum of a per-point value over every tree point's neighbourhood.

        The neighbourhood of point i is :meth:`search_radius_self`'s row i (unsorted: the other points closer than
        ``radius``); ``values`` is ``(npts,)`` or ``(npts, channels)`` float32 by original point index, and row i of the
        result folds ``values[j]`` over the row, channel by channel, in row order (``ptk_aggregate_within_self``: the
        exact float32 formulas are in ``ptk.h``).  No rows are written.  ``op`` is ``"sum"``, ``"min"`` or ``"max"``; an
        empty row gives 0, +inf or -inf.  With ``include_self`` the fold starts at the point's own value instead.
        ``radius`` is a scalar or an array of ``npts`` radii by original point index.  A 1-D ``values`` gives a 1-D
        result.  With ``counts=True`` returns ``(out, counts)``, ``counts`` the ``int64`` row lengths (mean = sum /
        count).  With ``device=True`` ``values`` is a contiguous CUDA tensor on the tree's device and the results are
        CUDA tensors, enqueued on the current torch stream.  float32 trees; served where :meth:`count_within_self` is,
        the rest is refused (``allow_host_loop`` serves every float32 tree)."""
        self._float32_only("aggregate_within_self")
        code = self._aggregate_op(op, include_self)
        n = self._npts
        lib = _load()
        if device:
            import torch
            dev = torch.device("cuda", int(self.info()["device"]))
            values, channels, flat = self._aggregate_values(values, dev)
            r, radii = self._self_radii(radius, True)
            out = torch.empty((n, channels), dtype=torch.float32, device=dev)
            cnt = torch.empty((n,), dtype=torch.int64, device=dev) if counts else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib.ptk_aggregate_within_self_device(self._h, r, radii.data_ptr() if radii is not None else None,
                                                        values.data_ptr(), channels, code, out.data_ptr(),
                                                        cnt.data_ptr() if counts else None, stream))
        else:
            values, channels, flat = self._aggregate_values(values, None)
            r, radii = self._self_radii(radius, False)
            out = np.zeros((n, channels), dtype=np.float32)
            cnt = np.zeros((n,), dtype=np.int64) if counts else None
            rp = radii.ctypes.data if radii is not None else None
            cp = cnt.ctypes.data if counts else None
            self._served(lib.ptk_aggregate_within_self(self._h, r, rp, values.ctypes.data, channels, code, out.ctypes.data, cp),
                         lambda lib: lib.ptk_host_aggregate_within_self(self._h, self._pts.ctypes.data, r, rp,
                                                                        values.ctypes.data, channels, code,
                                                                        out.ctypes.data, cp))
        if flat:
            out = out.reshape(n)
        return (out, cnt) if counts else out

    def aggregate_within(self, pts, radius, values, op: str = "sum", counts: bool = False):
        """``aggregate_within(pts, radius, values, op="sum", counts=False)`` -- the sum, minimum or maximum of a per-point
        value over the neighbourhood of each query.

        Row i of the result folds ``values[j]`` over :meth:`search_radius`'s unsorted row i of ``pts`` (``e = 1``), as
        :meth:`aggregate_within_self` does over the tree's own rows -- a query has no own point, so this is also the
        form for a subset of the tree's points (``ptk_aggregate_within``).  ``radius`` is a scalar or one radius per
        query.  Host ``pts`` take a float32 numpy ``values`` and return numpy arrays; a contiguous CUDA ``pts`` tensor
        takes a CUDA ``values`` tensor on the same device, is enqueued on the current torch stream and returns tensors.
        float32 trees; served where :meth:`search_radius` with per-row radii is, the rest is refused
        (``allow_host_loop`` serves every float32 tree)."""
        self._float32_only("aggregate_within")
        code = self._aggregate_op(op)
        radii = None if _is_scalar_radius(radius) else radius
        r = self._real(radius) if radii is None else self._real(0)
        lib = _load()
        if _is_torch(pts):
            import torch
            if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != self._sdim:
                raise ValueError("queries must be a float32 (nq, sdim) tensor")
            if not pts.is_cuda or not pts.is_contiguous():
                raise ValueError("queries must be a contiguous CUDA tensor")
            nq = pts.shape[0]
            values, channels, flat = self._aggregate_values(values, pts.device)
            if radii is not None:
                radii = self._device_radii(radii, pts, nq)
            out = torch.empty((nq, channels), dtype=torch.float32, device=pts.device)
            cnt = torch.empty((nq,), dtype=torch.int64, device=pts.device) if counts else None
            stream = torch.cuda.current_stream(pts.device).cuda_stream
            _check(lib.ptk_aggregate_within_device(self._h, pts.data_ptr(), nq, r,
                                                   radii.data_ptr() if radii is not None else None, values.data_ptr(),
                                                   channels, code, out.data_ptr(), cnt.data_ptr() if counts else None,
                                                   stream))
        else:
            q = self._as_matrix(pts, self._sdim, "pts", self._dtype)
            nq = q.shape[0]
            values, channels, flat = self._aggregate_values(values, None)
            if radii is not None:
                radii = self._host_radii(radii, nq)
            out = np.zeros((nq, channels), dtype=np.float32)
            cnt = np.zeros((nq,), dtype=np.int64) if counts else None
            rp = radii.ctypes.data if radii is not None else None
            cp = cnt.ctypes.data if counts else None
            self._served(lib.ptk_aggregate_within(self._h, q.ctypes.data, nq, r, rp, values.ctypes.data, channels, code,
                                                  out.ctypes.data, cp),
                         lambda lib: lib.ptk_host_aggregate_within(self._h, self._pts.ctypes.data, q.ctypes.data, nq, r, rp,
                                                                   values.ctypes.data, channels, code, out.ctypes.data, cp))
        if flat:
            out = out.reshape(nq)
        return (out, cnt) if counts else out

    @staticmethod
    def _align_transform(transform):
        """None, or the pose as 12 contiguous float32 values, row-major [R|t]: from a (3, 4) or (4, 4) matrix or 12 values."""
        if transform is None:
            return None
        m = np.asarray(transform)
        if m.shape == (4, 4):
            m = m[:3, :]
        if m.shape not in ((3, 4), (12,)):
            raise ValueError(f"transform must be a (3, 4) or (4, 4) matrix or 12 values, not {m.shape}")
        return np.ascontiguousarray(m, dtype=np.float32).reshape(12)

    def align_step(self, pts, transform=None, max_distance=np.inf, normals=None, rows: bool = False,
                   host_loop: bool = False):
        """``align_step(pts, transform=None, max_distance=inf, normals=None, rows=False)`` -- the normal equations of one
        ICP iteration, reduced on the device.

        The source points ``pts`` are posed by ``transform`` (a (3, 4) or (4, 4) matrix ``[R|t]``, applied in float32;
        ``None``: as they are), matched to their nearest tree point (``search_knn(q', 1)``), rejected where the squared
        distance is not below ``max_distance``, and the sums of the accepted rows are returned as an :class:`AlignSums`
        (``ptk_align_step``: the exact terms and the fixed order of the sums are in ``ptk.h``; every form gives the same
        bytes).  Without ``normals`` the sums are those of point-to-point alignment; with ``normals`` -- float32
        ``(npts, 3)`` by original point index, e.g. from :meth:`normals_within_self` -- those of point-to-plane.
        :meth:`AlignSums.solve` turns them into the rigid increment.  ``pts`` is never rewritten.  With ``rows=True``
        returns ``(sums, rows)``, ``rows`` being the unfiltered result of the search.  Host ``pts`` take host
        ``normals``; a contiguous CUDA ``pts`` tensor takes a CUDA ``normals`` tensor on the same device, is enqueued on
        the current torch stream (the workspace is the wrapper's) and the record is read when a field is first looked
        at.  ``host_loop=True`` runs the library's host loop instead (``ptk_host_align_step``: no device needed).
        float32 trees with three dimensions under ``Metric.L2Squared``."""
        self._float32_only("align_step")
        m = self._align_transform(transform)
        mp = m.ctypes.data if m is not None else None
        md = np.float32(max_distance)
        lib = _load()
        if _is_torch(pts):
            import torch
            if host_loop:
                raise ValueError("host_loop=True takes host arrays")
            if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != self._sdim:
                raise ValueError("queries must be a float32 (nq, sdim) tensor")
            if not pts.is_cuda or not pts.is_contiguous():
                raise ValueError("queries must be a contiguous CUDA tensor")
            nq = pts.shape[0]
            if normals is not None:
                if not (_is_torch(normals) and normals.is_cuda and normals.device == pts.device):
                    raise ValueError(f"normals must be a CUDA tensor on {pts.device} for a device call")
                if normals.dtype != torch.float32 or tuple(normals.shape) != (self._npts, 3) or not normals.is_contiguous():
                    raise ValueError(f"normals must be a contiguous float32 ({self._npts}, 3) tensor")
            need = c_uint64()
            _check(lib.ptk_align_step_workspace(self._h, nq, byref(need)))
            stream = torch.cuda.current_stream(pts.device)
            # (a workspace per stream: calls on two streams must not share their temporaries)
            cache = self.__dict__.setdefault("_align_ws", {})
            key = (pts.device.index, stream.cuda_stream)
            ws = cache.get(key)
            if ws is None or ws.numel() < need.value:
                ws = cache[key] = torch.empty((max(int(need.value), 256),), dtype=torch.uint8, device=pts.device)
            out = torch.empty((ALIGN_SUMS.itemsize,), dtype=torch.uint8, device=pts.device)
            raw = torch.empty((nq, 1, 2), dtype=torch.int32, device=pts.device) if rows else None
            _check(lib.ptk_align_step_device(self._h, pts.data_ptr(), nq, mp, md,
                                             normals.data_ptr() if normals is not None else None, out.data_ptr(),
                                             raw.data_ptr() if rows else None, ws.data_ptr(), ws.numel(),
                                             stream.cuda_stream))
            done = torch.cuda.Event()
            done.record(stream)
            sums = AlignSums(None, normals is not None, _pending=(out, done))
            return (sums, DeviceNeighbors(raw)) if rows else sums
        q = self._as_matrix(pts, self._sdim, "pts", self._dtype)
        nq = q.shape[0]
        if normals is not None:
            if _is_torch(normals):
                if normals.is_cuda:
                    raise ValueError("normals: a host call takes a host array, not a CUDA tensor")
                normals = normals.numpy()
            normals = np.asarray(normals)
            if normals.dtype != np.float32 or normals.shape != (self._npts, 3):
                raise ValueError(f"normals must be a float32 ({self._npts}, 3) array")
            normals = np.ascontiguousarray(normals)
        np_ = normals.ctypes.data if normals is not None else None
        rec = np.zeros((1,), dtype=ALIGN_SUMS)
        found = np.zeros((nq,), dtype=NEIGHBOR) if rows else None
        fp = found.ctypes.data if rows else None
        if host_loop:
            _check(lib.ptk_host_align_step(self._h, self._pts.ctypes.data, q.ctypes.data, nq, mp, md, np_, rec.ctypes.data, fp))
        else:
            self._served(lib.ptk_align_step(self._h, q.ctypes.data, nq, mp, md, np_, rec.ctypes.data, fp),
                         lambda lib: lib.ptk_host_align_step(self._h, self._pts.ctypes.data, q.ctypes.data, nq, mp, md, np_,
                                                             rec.ctypes.data, fp))
        sums = AlignSums(rec, normals is not None)
        return (sums, found) if rows else sums

    def _suppress_scores(self, scores, device):
        """The scores of :meth:`suppress_within_self`: None, a contiguous float32 host array of ``npts`` entries without a
        NaN, or -- ``device``: the torch device of a device call -- a contiguous float32 CUDA tensor on it, taken as it is
        (a host array-like is checked and uploaded)."""
        if scores is None:
            return None
        n = self._npts
        if device is not None and _is_torch(scores) and scores.is_cuda:
            import torch
            if scores.device != device:
                raise ValueError(f"scores must be on the tree's device ({device}), not on {scores.device}")
            if scores.dtype != torch.float32:
                raise ValueError(f"scores must be a float32 tensor, not {scores.dtype}")
            if scores.dim() != 1 or scores.shape[0] != n:
                raise ValueError(f"scores must be a 1-D tensor of {n} scores, one per tree point")
            if not scores.is_contiguous():
                raise ValueError("scores must be a contiguous tensor")
            return scores
        if _is_torch(scores):
            if scores.is_cuda:
                raise ValueError("scores: a host call takes a host array, not a CUDA tensor")
            scores = scores.numpy()
        try:
            host = np.asarray(scores)
            if host.dtype.kind not in "fiub":
                raise TypeError
            wide = host
            with np.errstate(over="ignore"):  # (a value that does not fit is refused below)
                host = np.ascontiguousarray(host, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"scores must be None or an array of {n} numbers") from None
        if host.ndim != 1 or host.shape[0] != n:
            raise ValueError(f"scores must be a 1-D array of {n} scores, one per tree point, not {tuple(host.shape)}")
        if wide.dtype.kind == "f" and wide.dtype.itemsize > 4 and np.any(np.isinf(host) & ~np.isinf(wide)):
            raise ValueError("scores: a value does not fit float32 (the key holds a float32 score)")
        bad = np.flatnonzero(np.isnan(host))
        if len(bad):
            raise ValueError(f"scores[{int(bad[0])}] must not be NaN")
        if device is not None:
            import torch
            return torch.from_numpy(host if host.flags.writeable else host.copy()).to(device)
        return host

    def suppress_within_self(self, radius, scores=None, indices: bool = False, device: bool = False):
        """``suppress_within_self(radius, scores=None, indices=False, device=False)`` -- greedy radius suppression of the
        tree's points: thinning to an r-separated subset (Poisson-disk / spatial subsampling), or with ``scores``
        non-maximum suppression ("keep the points whose score is a local maximum within r").

        With row i being :meth:`search_radius_self`'s row i (the other points j with ``distance(i, j) < radius_i``,
        strict, in the metric's own unit -- squared under ``L2Squared``) and
        ``key(i) = (ord_i << 32) | (0xFFFFFFFF - i)``: ``keep[i]`` is True iff row i holds no j with
        ``key(j) > key(i)`` and ``keep[j]`` True -- the greedy pass over the points in descending key.  With ``scores``
        (``npts`` float32 values by original point index, no NaN) ``ord_i`` is the total-order map of the score's bits
        (``b ^ 0xFFFFFFFF`` if the sign bit is set, else ``b ^ 0x80000000``): a higher score wins, an equal score is
        decided by the lower index, ``-0.0`` lies below ``+0.0``, infinities are ordinary values.  Without,
        ``ord_i = fmix32(i)`` (the 32-bit finaliser written out in ``ptk.h``): a fixed pseudo-random order.  With a
        scalar radius under ``L2Squared`` or ``L1`` the kept set is a maximal r-separated subset; of a pile of
        coincident points exactly one is kept for any r > 0 (the one of highest key -- unless a kept point outside the
        pile, of higher key still, lies within r and suppresses all of it); radius 0 keeps everything.  ``radius`` is a scalar or an
        array of ``npts`` radii by original point index.  No rows are written (``ptk_suppress_within_self`` /
        ``ptk_search64_suppress_within_self``).

        Returns a ``bool[npts]`` array; with ``indices=True`` the kept original indices ascending (``int64``).  With
        ``device=True`` the result is a CUDA tensor on the tree's device and the work is enqueued on the current torch
        stream; ``scores`` may then be a contiguous float32 CUDA tensor, taken as it is (a NaN takes the place its bits
        give it, a NaN or negative radius entry gives an empty row: the point is kept).  Unlike the other device forms
        this call WAITS on that stream once per round (it reads a 4-byte counter back) and cannot be captured into a
        graph (a capturing stream raises).  ``tree.last_suppress_rounds`` holds the number of rounds launched (information only).  Served where
        :meth:`count_within_self` is; the rest is refused (``allow_host_loop`` serves float32 trees)."""
        n = self._npts
        lib = _load()
        rounds = ctypes.c_uint32(0)
        if device:
            import torch
            dev = torch.device("cuda", int(self.info()["device"]))
            r, radii = self._self_radii(radius, True)
            d_scores = self._suppress_scores(scores, dev)
            out = torch.empty((n,), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            fn = lib.ptk_search64_suppress_within_self_device if self._f64 else lib.ptk_suppress_within_self_device
            _check(fn(self._h, r, radii.data_ptr() if radii is not None else None,
                      d_scores.data_ptr() if d_scores is not None else None, out.data_ptr(), byref(rounds), stream))
            self.last_suppress_rounds = int(rounds.value)
            keep = out.to(torch.bool)
            return torch.nonzero(keep).reshape(-1) if indices else keep
        r, radii = self._self_radii(radius, False)
        host = self._suppress_scores(scores, None)
        keep = np.zeros((n,), dtype=np.uint8)
        rp = radii.ctypes.data if radii is not None else None
        sp = host.ctypes.data if host is not None else None
        fn = lib.ptk_search64_suppress_within_self if self._f64 else lib.ptk_suppress_within_self
        self._served(fn(self._h, r, rp, sp, keep.ctypes.data, None, byref(rounds)),
                     lambda lib: lib.ptk_host_suppress_within_self(self._h, self._pts.ctypes.data, r, rp, sp,
                                                                   keep.ctypes.data, None))
        self.last_suppress_rounds = int(rounds.value)
        keep = keep.astype(bool)
        return np.flatnonzero(keep).astype(np.int64) if indices else keep

    def _spacing(self, k, sqrt, ratio, want_kth, want_keep, want_stats, device):
        """One call of ``ptk_spacing_knn_self`` (its float64 / ``_device`` forms): ``(mean, kth, keep, record)``, the
        outputs that were not asked for None; ``record`` a ``SPACING_STATS`` numpy record."""
        k = int(k)
        n = self._npts
        lib = _load()
        if sqrt is None:
            sqrt = self._metric in (Metric.L2Squared, Metric.SE2Squared)
        flags = PTK_SPACING_SQRT if sqrt else 0
        ratio = float(ratio)
        reduce_ = want_keep or want_stats
        if reduce_ and not 0.0 <= ratio <= float(np.finfo(np.float32).max):  # (the C ABI takes a float)
            raise ValueError("std_ratio must be finite (as a float32) and >= 0")
        if device:
            import torch
            dev = torch.device("cuda", int(self.info()["device"]))
            treal = torch.float64 if self._f64 else torch.float32
            mean = torch.empty((n,), dtype=treal, device=dev)
            kth = torch.empty((n,), dtype=treal, device=dev) if want_kth else None
            keep = torch.empty((n,), dtype=torch.uint8, device=dev) if want_keep else None
            rec = torch.empty((64,), dtype=torch.uint8, device=dev) if want_stats else None
            need = ctypes.c_uint64(0)
            ws = None
            if reduce_:
                fn = lib.ptk_search64_spacing_knn_self_workspace if self._f64 else lib.ptk_spacing_knn_self_workspace
                _check(fn(self._h, byref(need)))
                ws = torch.empty((max(int(need.value), 1),), dtype=torch.uint8, device=dev)
            ptr = lambda t: t.data_ptr() if t is not None else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            fn = lib.ptk_search64_spacing_knn_self_device if self._f64 else lib.ptk_spacing_knn_self_device
            _check(fn(self._h, k, flags, ratio, ptr(mean), ptr(kth), ptr(keep), ptr(rec), ptr(ws), int(need.value), stream))
            if ws is not None:
                ws.record_stream(torch.cuda.current_stream(dev))
            record = None
            if rec is not None:  # (the record is read on the host: the one wait of this form, only where it is asked for)
                record = np.frombuffer(rec.cpu().numpy().tobytes(), dtype=SPACING_STATS)[0]
            return mean, kth, keep, record
        mean = np.empty((n,), dtype=self._real)
        kth = np.empty((n,), dtype=self._real) if want_kth else None
        keep = np.empty((n,), dtype=np.uint8) if want_keep else None
        rec = np.zeros((1,), dtype=SPACING_STATS) if want_stats else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        fn = lib.ptk_search64_spacing_knn_self if self._f64 else lib.ptk_spacing_knn_self
        self._served(fn(self._h, k, flags, ratio, ptr(mean), ptr(kth), ptr(keep), ptr(rec)),
                     lambda lib: lib.ptk_host_spacing_knn_self(self._h, self._pts.ctypes.data, k, flags, ratio, ptr(mean),
                                                               ptr(kth), ptr(keep), ptr(rec)))
        return mean, kth, keep, rec[0] if rec is not None else None

    def spacing_knn_self(self, k: int, sqrt=None, kth: bool = False, device: bool = False):
        """``spacing_knn_self(k, sqrt=None, kth=False, device=False)`` -- the mean distance from each tree point to its k
        nearest OTHER points, and with ``kth=True`` the distance to the k-th of them, without the rows.

        Row i is :meth:`search_knn_self`'s row i; with ``m`` its entries below ``FLT_MAX`` (``DBL_MAX``),
        ``mean[i] = (((0 + d_0) + d_1) + ...) / m`` and ``kth[i] = d_{m-1}`` in the tree's dtype, one rounding per
        operation in that order; a point with no neighbour (``npts == 1``) gets ``FLT_MAX`` (``DBL_MAX``) for both.
        ``sqrt``: take the square root of every distance first (``PTK_SPACING_SQRT``); ``None`` means on iff the metric
        is ``L2Squared`` or ``SE2Squared``, so that the result is a length.  (``ptk_spacing_knn_self`` /
        ``ptk_search64_spacing_knn_self``.)

        Returns ``mean`` or ``(mean, kth)``: numpy arrays of the tree's dtype, or with ``device=True`` CUDA tensors on
        the tree's device, enqueued on the current torch stream.  :meth:`self_route` says whether the call only
        enqueues (1) or allocates and waits (2).  ``allow_host_loop`` serves float32 trees the device refuses."""
        mean, kd, _, _ = self._spacing(k, sqrt, 0.0, kth, False, False, device)
        return (mean, kd) if kth else mean

    def outliers_knn_self(self, k: int, std_ratio: float = 2.0, sqrt=None, indices: bool = False, stats: bool = False,
                          device: bool = False):
        """``outliers_knn_self(k, std_ratio=2.0, sqrt=None, indices=False, stats=False, device=False)`` -- statistical
        outlier removal (PCL's ``StatisticalOutlierRemoval``, Open3D's ``remove_statistical_outlier``): keep the points
        whose mean distance to their k nearest other points is at most ``mean + std_ratio * stddev`` of those means.

        The means are :meth:`spacing_knn_self`'s.  A point is valid when it has a neighbour and its mean is finite;
        ``mean`` and ``variance`` (the sample variance) are taken over the valid points in float64 on a fixed summation
        tree, and ``keep[i] = valid_i and (e <= 0 or e * e <= std_ratio**2 * variance)`` with ``e = mean_i - mean`` --
        the decision uses no square root and is the same bits on host and device (``ptk.h``).  ``std_ratio`` must be
        finite and >= 0.

        Returns the ``bool[npts]`` mask, or with ``indices=True`` the kept original indices ascending (``int64``); with
        ``stats=True`` additionally a dict of the record (``count``, ``rows``, ``sum``, ``mean``, ``ssd``, ``variance``,
        ``ratio_squared``) plus ``stddev = sqrt(variance)`` and ``threshold = mean + std_ratio * stddev`` (information
        only), and ``record``, the 64 bytes themselves.  With ``device=True`` the mask is a CUDA tensor, enqueued on the
        current torch stream; asking for ``stats`` reads 64 bytes back and waits for them."""
        _, _, keep, rec = self._spacing(k, sqrt, std_ratio, False, True, stats, device)
        if device:
            import torch
            mask = keep.to(torch.bool)
            out = torch.nonzero(mask).reshape(-1) if indices else mask
        else:
            mask = keep.astype(bool)
            out = np.flatnonzero(mask).astype(np.int64) if indices else mask
        if not stats:
            return out
        info = {name: rec[name].item() for name in SPACING_STATS.names if name != "reserved"}
        info["stddev"] = float(np.sqrt(info["variance"]))
        info["threshold"] = info["mean"] + float(np.float32(std_ratio)) * info["stddev"]
        info["record"] = rec.tobytes()
        return out, info

    def _mst_core(self, core, device):
        """The core distances of :meth:`mst_within_self`: None, a contiguous float32 host array of ``npts`` entries, none
        NaN or negative, or -- ``device``: the torch device of a device call -- a contiguous float32 CUDA tensor on it,
        taken as it is (a host array-like is checked and uploaded)."""
        if core is None:
            return None
        n = self._npts
        if device is not None and _is_torch(core) and core.is_cuda:
            import torch
            if core.device != device:
                raise ValueError(f"core must be on the tree's device ({device}), not on {core.device}")
            if core.dtype != torch.float32 or core.dim() != 1 or core.shape[0] != n or not core.is_contiguous():
                raise ValueError(f"core must be a contiguous 1-D float32 tensor of {n} entries, one per tree point")
            return core
        if _is_torch(core):
            if core.is_cuda:
                raise ValueError("core: a host call takes a host array, not a CUDA tensor")
            core = core.numpy()
        try:
            host = np.ascontiguousarray(core, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"core must be None or an array of {n} numbers") from None
        if host.ndim != 1 or host.shape[0] != n:
            raise ValueError(f"core must be a 1-D array of {n} entries, one per tree point, not {tuple(host.shape)}")
        bad = np.flatnonzero(~(host >= 0))
        if len(bad):
            raise ValueError(f"core[{int(bad[0])}] must be >= 0 (and not NaN)")
        if device is not None:
            import torch
            return torch.from_numpy(host if host.flags.writeable else host.copy()).to(device)
        return host

    def mst_within_self(self, radius=np.inf, core=None, labels: bool = False, device: bool = False):
        """``mst_within_self(radius=inf, core=None, labels=False, device=False)`` -- the minimum spanning forest of the
        fixed-radius graph over the tree's points: the single-linkage dendrogram for every radius up to ``radius`` at once,
        and with ``core`` HDBSCAN's mutual-reachability tree.

        With row i being :meth:`search_radius_self`'s row i at ``radius`` (strict, the metric's own unit -- squared under
        ``L2Squared``), ``{i, j}`` is an edge iff j is in row i or i in row j.  Its weight is the row's distance, or with
        ``core`` (``npts`` float32 values by original index, in the same unit: :meth:`spacing_knn_self`'s ``kth`` with
        ``sqrt=False``) ``max(d, core[i], core[j])``, and the edge then exists only if that is below ``radius`` too.  Edges
        are ordered by ``(bits(w), lo, hi)`` with ``lo < hi`` the two indices: the triples are distinct, so the forest is
        unique, and ties are decided by this rule alone.  Cutting the forest at any ``r' <= radius`` (keep ``w < r'``)
        gives the components of ``cluster_within_self(r', 0)``.  ``radius=inf`` gives the Euclidean minimum spanning
        tree of the cloud.  (``ptk_mst_within_self``.)

        Returns a structured array (:data:`MST_EDGE`: ``lo``, ``hi`` uint32, ``w`` float32) of ``npts`` minus the number
        of components records, ascending in that order; with ``labels=True`` also ``int32[npts]``, the smallest index
        of each point's component.  With ``device=True`` the edges are three CUDA tensors ``(lo, hi, w)`` (int32, int32,
        float32) in the same order, ``core`` may be a float32 CUDA tensor (a NaN or negative entry then gives a point
        without edges), and the rounds run on the current torch stream; like :meth:`suppress_within_self` the call
        waits on that stream once per round and cannot be captured into a graph.  ``tree.last_mst_rounds`` holds the
        rounds launched (information only).  Served for float32 trees with ``sdim <= 3`` under ``L2Squared`` and ``L1``;
        the rest is refused (``allow_host_loop`` serves float32 trees under those two metrics)."""
        n = self._npts
        lib = _load()
        if self._f64:
            raise PtkError(PTK_ERR_UNSUPPORTED, "mst_within_self: float64 trees are not served (the host loop, "
                           "ptk_host_mst_within_self, serves float32 trees)")
        r = np.float32(radius)
        rounds = ctypes.c_uint32(0)
        count = c_uint64(0)
        cap = max(n - 1, 1)
        if device:
            import torch
            dev = torch.device("cuda", int(self.info()["device"]))
            d_core = self._mst_core(core, dev)
            need = c_uint64(0)
            _check(lib.ptk_mst_within_self_workspace(self._h, byref(need)))
            ws = torch.empty((int(need.value),), dtype=torch.uint8, device=dev)
            raw = torch.empty((cap, 3), dtype=torch.int32, device=dev)
            lab = torch.empty((n,), dtype=torch.int32, device=dev) if labels else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib.ptk_mst_within_self_device(self._h, r, d_core.data_ptr() if d_core is not None else None,
                                                  raw.data_ptr(), lab.data_ptr() if labels else None, ws.data_ptr(),
                                                  need, byref(count), byref(rounds), stream))
            self.last_mst_rounds = int(rounds.value)
            raw = raw[:int(count.value)]
            # (the _device form writes the set in no order: three stable sorts give (bits(w), lo, hi) ascending)
            for col in (1, 0, 2):
                raw = raw[torch.argsort(raw[:, col], stable=True)]
            edges = (raw[:, 0].contiguous(), raw[:, 1].contiguous(), raw[:, 2].contiguous().view(torch.float32))
            return (edges, lab) if labels else edges
        host = self._mst_core(core, None)
        edges = np.zeros((cap,), dtype=MST_EDGE)
        lab = np.empty((n,), dtype=np.int32) if labels else None
        cp = host.ctypes.data if host is not None else None
        lp = lab.ctypes.data if labels else None
        self._served(lib.ptk_mst_within_self(self._h, r, cp, edges.ctypes.data, byref(count), lp, byref(rounds)),
                     lambda lib: lib.ptk_host_mst_within_self(self._h, self._pts.ctypes.data, r, cp, edges.ctypes.data,
                                                              byref(count), lp))
        self.last_mst_rounds = int(rounds.value)
        edges = edges[:int(count.value)].copy()
        return (edges, lab) if labels else edges

    def _host_radii(self, radii, nq: int):
        """The per-row radii of a host batch: any 1-D array-like of nq values, as a contiguous array of the tree's dtype."""
        if _is_torch(radii):
            if radii.is_cuda:
                raise ValueError("radius: host queries take host radii, not a CUDA tensor")
            radii = radii.numpy()
        try:
            radii = np.ascontiguousarray(radii, dtype=self._dtype)
        except (TypeError, ValueError) as ex:
            raise ValueError(f"radius: not an array of numbers ({ex})") from None
        if radii.ndim != 1:
            raise ValueError(f"radius must be a scalar or a 1-D array of one radius per query, not {radii.ndim}-D")
        if radii.shape[0] != nq:
            raise ValueError(f"radius holds {radii.shape[0]} entries for {nq} queries")
        return radii

    def _device_radii(self, radii, pts, nq: int):
        """The per-row radii of a torch CUDA batch: a contiguous 1-D CUDA tensor of the tree's dtype on the queries'
        device, taken as it is (no copy, no look at the values)."""
        if not _is_torch(radii):
            raise ValueError("radius: CUDA queries take a scalar or a CUDA tensor of one radius per query")
        if not radii.is_cuda or radii.device != pts.device:
            raise ValueError(f"radius must be on the queries' device ({pts.device}), not on {radii.device}")
        if radii.dtype != pts.dtype:
            raise ValueError(f"radius must be a {self._dtype.name} tensor, not {radii.dtype}")
        if radii.dim() != 1:
            raise ValueError(f"radius must be a scalar or a 1-D tensor of one radius per query, not {radii.dim()}-D")
        if radii.shape[0] != nq:
            raise ValueError(f"radius holds {radii.shape[0]} entries for {nq} queries")
        if not radii.is_contiguous():
            raise ValueError("radius must be a contiguous tensor")
        return radii

    def _served(self, status: int, host_loop) -> None:
        """``_check``: every failure raises.  Only after ``allow_host_loop(True)`` is a search the DEVICE refuses for a
        valid tree (PTK_ERR_UNSUPPORTED) served by the host loop of the library (``ptk_host_search_*``: the reference's
        own batch loop) with one warning; a missing device or a HIP error raises regardless."""
        if status == PTK_ERR_UNSUPPORTED and not self._f64 and _host_loop_allowed:
            lib = _load()
            _warn_host_loop(lib.ptk_last_error().decode("utf-8", "replace"))
            status = host_loop(lib)
        _check(status)

    def _search_knn_device(self, q, k, e, out):
        import torch
        tq, traw = (torch.float64, torch.int64) if self._f64 else (torch.float32, torch.int32)
        if q.dtype != tq or q.dim() != 2 or q.shape[1] != self._sdim:
            raise ValueError(f"queries must be a {self._dtype.name} (nq, sdim) tensor")
        if not q.is_cuda or not q.is_contiguous():
            raise ValueError("queries must be a contiguous CUDA tensor")
        nq = q.shape[0]
        if out is None:
            # float64: the records carry 4 bytes of padding, zeroed so that index reads as an int64
            out = (torch.zeros if self._f64 else torch.empty)((nq, k, 2), dtype=traw, device=q.device)
        elif isinstance(out, DeviceNeighbors):
            out = out.raw
        if out.dtype != traw or tuple(out.shape) != (nq, k, 2) or not out.is_contiguous():
            raise ValueError(f"nns must be a contiguous {traw} (nq, k, 2) tensor")
        stream = torch.cuda.current_stream(q.device).cuda_stream
        _check(self._fn("ptk_search_knn_device")(self._h, q.data_ptr(), nq, k, self._real(e),
                                                 out.data_ptr(), stream))
        return DeviceNeighbors(out)

    # -- radius ---------------------------------------------------------------------------
    def search_radius(self, pts, radius: float, *args, sort: bool = False):
        """``search_radius(pts, radius[, e][, nns], sort=False)`` -> :class:`DArray`.

        A query row with NaN, +-Inf or any finite value gets the row the reference gives it (a NaN or +-Inf row
        under the sum metrics: an empty one -- ``radius > distance`` is false) and changes no other row; ``radius``
        may be ``FLT_MAX`` or ``+inf``.

        ``radius`` may also be a 1-D array of ``nq`` radii, one per query row (``ptk_search_radius_radii`` /
        ``ptk_search64_radius_radii``): row i is the scalar call's row i at ``radius[i]``.  That form is exact -- ``e``
        may not be given -- and a NaN or negative entry is refused by its row.  The device serves it where it serves
        :meth:`count_within` with an array; the rest is refused (``allow_host_loop`` serves float32 trees)."""
        radii = None if _is_scalar_radius(radius) else radius
        if radii is not None and any(isinstance(a, (int, float, np.floating)) and not isinstance(a, bool) for a in args):
            raise ValueError("search_radius with one radius per query is exact: e may not be given")
        e, nns, sort = self._split_optional_radius(args, sort)
        q = self._as_matrix(pts, self._sdim, "pts", self._dtype)
        nq = q.shape[0]
        if nns is not None and (not isinstance(nns, DArray) or nns.dtype != self._neighbor):
            raise ValueError("unexpected dtype_neighbor for data")
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        rows = c_void_p()
        lib = _load()
        if radii is not None:
            radii = self._host_radii(radii, nq)
            self._served(self._fn("ptk_search_radius_radii")(self._h, q.ctypes.data, nq, radii.ctypes.data,
                                                             int(bool(sort)), offsets.ctypes.data, byref(rows)),
                         lambda lib: lib.ptk_host_search_radius_radii(self._h, self._pts.ctypes.data, q.ctypes.data, nq,
                                                                      radii.ctypes.data, int(bool(sort)),
                                                                      offsets.ctypes.data, byref(rows)))
            flat = _adopt(lib, rows, int(offsets[-1]), self._neighbor)
            if nns is None:
                return DArray(offsets, flat)
            nns._assign(offsets, flat)
            return nns
        self._served(self._fn("ptk_search_radius")(self._h, q.ctypes.data, nq, self._real(radius),
                                                   self._real(e), int(bool(sort)), offsets.ctypes.data, byref(rows)),
                     lambda lib: lib.ptk_host_search_radius(self._h, self._pts.ctypes.data, q.ctypes.data, nq,
                                                            np.float32(radius), np.float32(e), int(bool(sort)),
                                                            offsets.ctypes.data, byref(rows)))
        flat = _adopt(lib, rows, int(offsets[-1]), self._neighbor)
        if nns is None:
            return DArray(offsets, flat)
        nns._assign(offsets, flat)
        return nns

    # -- box ------------------------------------------------------------------------------
    def search_box(self, boxes, nns=None):
        """``search_box(boxes[, nns])`` -> :class:`DArray` of int32 index arrays.

        ``boxes`` is ``(2 * nbox, sdim)``: rows ``2 i`` and ``2 i + 1`` are the min and max corner
        of box ``i`` (``_pyco_tree/kd_tree.hpp:245-268``).  Row ``i`` of the result lists the points
        inside the closed box in the reference's traversal order.

        A corner with NaN, +-Inf or any finite value gets what the reference gives it: its test is
        ``min > x or max < x -> outside`` (``box.hpp:31-40``), so a NaN corner coordinate does not bound its side of
        the axis (it does not empty the box), and an inverted box is empty."""
        b = self._as_matrix(boxes, self._sdim, "boxes", self._dtype)
        if b.shape[0] % 2 != 0:
            raise ValueError("query min and max don't have equal size")
        nb = b.shape[0] // 2
        mins = np.ascontiguousarray(b[0::2])
        maxs = np.ascontiguousarray(b[1::2])
        if nns is not None and (not isinstance(nns, DArray) or nns.dtype != np.dtype(np.int32)):
            raise ValueError("unexpected dtype_index for data")
        offsets = np.zeros(nb + 1, dtype=np.uint64)
        rows = c_void_p()
        lib = _load()
        self._served(self._fn("ptk_search_box")(self._h, mins.ctypes.data, maxs.ctypes.data, nb, offsets.ctypes.data,
                                                byref(rows)),
                     lambda lib: lib.ptk_host_search_box(self._h, self._pts.ctypes.data, mins.ctypes.data,
                                                         maxs.ctypes.data, nb, offsets.ctypes.data, byref(rows)))
        flat = _adopt(lib, rows, int(offsets[-1]), np.int32)
        if nns is None:
            return DArray(offsets, flat)
        nns._assign(offsets, flat)
        return nns

    def search_box_device(self, mins, maxs):
        """Device form of :meth:`search_box`: ``mins`` / ``maxs`` are float32 ``(nbox, sdim)`` CUDA tensors; returns
        (offsets int64 tensor [nbox + 1], indices int32 tensor [total]) on the current torch stream."""
        import torch
        self._float32_only("search_box_device()")
        for a in (mins, maxs):
            if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != self._sdim or not a.is_cuda \
                    or not a.is_contiguous():
                raise ValueError("mins / maxs must be contiguous float32 (nbox, sdim) CUDA tensors")
        if mins.shape != maxs.shape:
            raise ValueError("query min and max don't have equal size")
        nb = mins.shape[0]
        lib = _load()
        stream = torch.cuda.current_stream(mins.device).cuda_stream
        counts = torch.zeros(nb + 1, dtype=torch.int64, device=mins.device)
        _check(lib.ptk_search_box_count_device(self._h, mins.data_ptr(), maxs.data_ptr(), nb, counts.data_ptr(), stream))
        offsets = torch.zeros(nb + 1, dtype=torch.int64, device=mins.device)
        offsets[1:] = torch.cumsum(counts[:nb], 0)
        total = int(offsets[-1].item())
        out = torch.empty(max(total, 1), dtype=torch.int32, device=mins.device)
        _check(lib.ptk_search_box_fill_device(self._h, mins.data_ptr(), maxs.data_ptr(), nb, offsets.data_ptr(),
                                              out.data_ptr(), stream))
        return offsets, out[:total]

    def search_radius_device(self, q, radius: float, e: float | None = None, sort: bool = False):
        """Device form: returns (offsets int64 tensor [nq + 1], raw int32 tensor [total, 2]).

        ``radius`` may also be a float32 CUDA tensor of ``nq`` radii, one per query row: the per-row count
        (``ptk_search_count_within_radii_device`` with ``max_count = 0``), ``torch.cumsum`` and
        ``ptk_search_radius_radii_fill_device`` on the current stream.  That form is exact (``e`` may not be given) and
        only enqueues: a row whose radius is NaN or negative is empty."""
        import torch
        self._float32_only("search_radius_device()")
        if q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != self._sdim:
            raise ValueError("queries must be a float32 (nq, sdim) tensor")
        if not q.is_cuda or not q.is_contiguous():
            raise ValueError("queries must be a contiguous CUDA tensor")
        nq = q.shape[0]
        lib = _load()
        stream = torch.cuda.current_stream(q.device).cuda_stream
        counts = torch.zeros(nq + 1, dtype=torch.int64, device=q.device)
        if not _is_scalar_radius(radius):
            if e is not None:
                raise ValueError("search_radius_device with one radius per query is exact: e may not be given")
            radii = self._device_radii(radius, q, nq)
            _check(lib.ptk_search_count_within_radii_device(self._h, q.data_ptr(), nq, radii.data_ptr(), 0,
                                                            counts.data_ptr(), stream))
            offsets = torch.zeros(nq + 1, dtype=torch.int64, device=q.device)
            offsets[1:] = torch.cumsum(counts[:nq], 0)
            total = int(offsets[-1].item())
            out = torch.empty((max(total, 1), 2), dtype=torch.int32, device=q.device)
            _check(lib.ptk_search_radius_radii_fill_device(self._h, q.data_ptr(), nq, radii.data_ptr(), offsets.data_ptr(),
                                                           out.data_ptr(), int(bool(sort)), stream))
            return offsets, out[:total]
        e = 1.0 if e is None else e
        _check(lib.ptk_search_radius_count_device(self._h, q.data_ptr(), nq, np.float32(radius),
                                                  np.float32(e), counts.data_ptr(), stream))
        offsets = torch.zeros(nq + 1, dtype=torch.int64, device=q.device)
        offsets[1:] = torch.cumsum(counts[:nq], 0)
        total = int(offsets[-1].item())
        out = torch.empty((max(total, 1), 2), dtype=torch.int32, device=q.device)
        _check(lib.ptk_search_radius_fill_device(self._h, q.data_ptr(), nq, np.float32(radius),
                                                 np.float32(e), offsets.data_ptr(), out.data_ptr(),
                                                 int(bool(sort)), stream))
        return offsets, out[:total]

    # -- argument plumbing for the overload sets ------------------------------------------------
    @staticmethod
    def _split_optional(args):
        e, nns = 1.0, None
        for a in args:
            if isinstance(a, (int, float, np.floating)) and not isinstance(a, bool):
                e = float(a)
            else:
                nns = a
        if len(args) > 2:
            raise TypeError("search_knn(pts, k[, e][, nns])")
        if not e > 0:
            raise ValueError("e must be positive")
        return e, nns

    @staticmethod
    def _split_optional_radius(args, sort):
        e, nns = 1.0, None
        for a in args:
            if isinstance(a, bool):
                sort = a
            elif isinstance(a, (int, float, np.floating)):
                e = float(a)
            else:
                nns = a
        if len(args) > 3:
            raise TypeError("search_radius(pts, radius[, e][, nns][, sort])")
        if not e > 0:
            raise ValueError("e must be positive")
        return e, nns, sort


class MultiKdTree:
    """One kd-tree replicated on several GPUs of this node, single process (``ptk_multi_*``).

    A batch is cut into ``len(devices)`` contiguous row ranges, range ``r`` searched on
    ``devices[r]``; rows come back in the caller's order and are bit-identical to a single-device
    :class:`KdTree`.  Host arrays move range by range (no inter-GPU traffic); with torch tensors on
    ``devices[0]`` the ranges and the (index, distance) rows travel over xGMI through RCCL."""

    def __init__(self, pts, max_leaf_size: int = 10, devices=None):
        p = np.ascontiguousarray(pts, dtype=np.float32)
        if p.ndim != 2:
            raise ValueError("pts must be (n, sdim)")
        if devices is None:
            devices = list(range(device_count()))
        self._devices = np.ascontiguousarray(devices, dtype=np.int32)
        self._sdim = p.shape[1]
        self._h = c_void_p()
        _check(_load().ptk_multi_create_from_points(p.ctypes.data, p.shape[0], p.shape[1], int(max_leaf_size),
                                                     self._devices.ctypes.data, len(self._devices), byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _load().ptk_multi_destroy(self._h)
            self._h = None

    @property
    def devices(self):
        return [int(d) for d in self._devices]

    def _queries(self, q):
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self._sdim:
            raise ValueError("pts must be (nq, sdim)")
        return q

    def search_knn(self, pts, k: int, e: float | None = None):
        """Host arrays: ``(nq,)`` (k = 1) or ``(nq, k)`` :data:`NEIGHBOR` records; a torch tensor on
        ``devices[0]``: :class:`DeviceNeighbors` (asynchronous on the current torch stream)."""
        k = int(k)
        if _is_torch(pts):
            import torch

            if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != self._sdim or not pts.is_contiguous():
                raise ValueError("pts must be a contiguous float32 (nq, sdim) tensor")
            if pts.device.index != int(self._devices[0]):
                raise ValueError("pts must live on devices[0]")
            out = torch.empty((pts.shape[0], k, 2), dtype=torch.int32, device=pts.device)
            stream = torch.cuda.current_stream(pts.device).cuda_stream
            _check(_load().ptk_multi_search_knn_device(self._h, pts.data_ptr(), pts.shape[0], k,
                                                       np.float32(1.0 if e is None else e), out.data_ptr(), stream))
            return DeviceNeighbors(out)
        q = self._queries(pts)
        out = np.empty((q.shape[0],) if k == 1 else (q.shape[0], k), dtype=NEIGHBOR)
        _check(_load().ptk_multi_search_knn(self._h, q.ctypes.data, q.shape[0], k, np.float32(1.0 if e is None else e),
                                            out.ctypes.data))
        return out

    def search_radius(self, pts, radius: float, e: float | None = None, sort: bool = False) -> "DArray":
        q = self._queries(pts)
        offsets = np.zeros(q.shape[0] + 1, dtype=np.uint64)
        rows = c_void_p()
        lib = _load()
        _check(lib.ptk_multi_search_radius(self._h, q.ctypes.data, q.shape[0], np.float32(radius),
                                           np.float32(1.0 if e is None else e), int(bool(sort)), offsets.ctypes.data,
                                           byref(rows)))
        return DArray(offsets, _adopt(lib, rows, int(offsets[-1]), NEIGHBOR))


class KdForest:
    """Randomised kd-forest for approximate nearest neighbours in high dimensions, searched on
    the MI355X (one query per wavefront; ``pico_tree_amd/csrc/ptk_forest.hpp``).

    Mirrors ``pico_tree::kd_forest`` of the reference's pico_understory
    (``/root/reference/examples/pico_understory/pico_understory/kd_forest.hpp:42-85``):
    ``KdForest(pts, max_leaf_size, forest_size)``, ``search_nn(pts, max_leaves_visited)`` and, for
    k > 1, ``search_knn(pts, k, max_leaves_visited)`` (the reference's generic
    ``search_nearest`` with a k-list visitor, de-duplicated by index here).  ``seed`` fixes the
    Householder reflections, which the reference draws from ``std::random_device``.

    Limits (``include/ptk.h``, forest section): ``k <= 64``, ``sdim <= 7072``, trees at most 95 levels deep (several
    hundred coincident points under a small ``max_leaf_size`` are refused).  The points must be finite, and so must
    their reflections: :class:`PtkError` otherwise.  A query row that is not finite, or whose distances overflow, comes
    back all padding ``(-1, FLT_MAX)`` and changes no other row.
    """

    def __init__(self, pts, max_leaf_size: int, forest_size: int, seed: int = 0, device: int | None = None):
        pts = KdTree._as_matrix(pts, None, "pts")
        if int(max_leaf_size) <= 0 or int(forest_size) <= 0:
            raise ValueError("max_leaf_size and forest_size must be positive")
        self._pts = pts
        self._npts, self._sdim = pts.shape
        self._forest_size = int(forest_size)
        handle = c_void_p()
        dev = PTK_DEVICE_CURRENT if device is None else int(device)
        _check(_load().ptk_forest_create(pts.ctypes.data, self._npts, self._sdim, int(max_leaf_size),
                                         self._forest_size, int(seed), dev, byref(handle)))
        self._h = handle

    @property
    def npts(self) -> int:
        return self._npts

    @property
    def sdim(self) -> int:
        return self._sdim

    @property
    def rotations(self) -> np.ndarray:
        """The unit reflection vectors, ``(forest_size, sdim)``."""
        out = np.empty((self._forest_size, self._sdim), dtype=np.float32)
        _check(_load().ptk_forest_get_rotations(self._h, out.ctypes.data))
        return out

    def search_knn(self, pts, k: int, max_leaves_visited: int):
        """Host array -> ``(nq, k)`` :data:`NEIGHBOR` array; torch CUDA tensor -> :class:`DeviceNeighbors`.
        Rows are ascending; slots beyond the distinct points found hold ``(-1, FLT_MAX)``."""
        k = int(k)
        if _is_torch(pts):
            import torch
            if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != self._sdim \
                    or not pts.is_cuda or not pts.is_contiguous():
                raise ValueError("queries must be a contiguous float32 (nq, sdim) CUDA tensor")
            out = torch.empty((pts.shape[0], k, 2), dtype=torch.int32, device=pts.device)
            stream = torch.cuda.current_stream(pts.device).cuda_stream
            _check(_load().ptk_forest_search_knn_device(self._h, pts.data_ptr(), pts.shape[0], k,
                                                        int(max_leaves_visited), out.data_ptr(), stream))
            return DeviceNeighbors(out)
        q = KdTree._as_matrix(pts, self._sdim, "pts")
        out = np.empty((q.shape[0], k), dtype=NEIGHBOR)
        _check(_load().ptk_forest_search_knn(self._h, q.ctypes.data, q.shape[0], k, int(max_leaves_visited),
                                             out.ctypes.data))
        return out

    @property
    def dropped(self) -> int:
        """Queue entries dropped so far because a per-tree queue was full (0 in normal use).  Cumulative over the life
        of the handle: every search adds what it dropped."""
        v = c_uint64()
        _check(_load().ptk_forest_get_dropped(self._h, byref(v)))
        return int(v.value)

    def search_nn(self, pts, max_leaves_visited: int):
        """``(nq,)`` nearest neighbours (kd_forest.hpp:78-85)."""
        res = self.search_knn(pts, 1, max_leaves_visited)
        return res if isinstance(res, DeviceNeighbors) else res[:, 0]

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _load().ptk_forest_destroy(h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- registration: the sums of KdTree.align_step and the loop around them ------------------------
class AlignSums:
    """The record of :meth:`KdTree.align_step` (``ptk_align_sums``): ``count``, ``rows``, ``sum_distance`` and the sums of
    the mode -- ``sum_q``, ``sum_p``, ``sum_qp`` (3 x 3), ``sum_qq``, ``sum_pp`` for point-to-point, ``jtj`` (the 21
    entries of the upper triangle), ``jtr``, ``sum_rr`` for point-to-plane -- as float64.  ``record`` is the 384-byte
    numpy record itself (``tobytes()`` compares two results bit for bit)."""

    def __init__(self, record, plane: bool, _pending=None):
        self._record = record
        self._pending = _pending
        self.plane = bool(plane)

    @property
    def record(self) -> np.ndarray:
        if self._record is None:  # a device call: wait for it, bring the 384 bytes down
            out, done = self._pending
            done.synchronize()
            self._record = np.ascontiguousarray(out.cpu().numpy()).view(ALIGN_SUMS)
            self._pending = None
        return self._record

    def tobytes(self) -> bytes:
        return self.record.tobytes()

    def __getattr__(self, name):
        if name in ALIGN_SUMS.names:
            v = self.record[name][0]
            if name in ("count", "rows"):
                return int(v)
            if name == "sum_qp":
                return v.reshape(3, 3)
            return float(v) if v.ndim == 0 else v
        raise AttributeError(name)

    def __repr__(self) -> str:
        return f"AlignSums({'point-to-plane' if self.plane else 'point-to-point'}, count={self.count}, rows={self.rows})"

    @property
    def normal_matrix(self) -> np.ndarray:
        """The symmetric 6 x 6 matrix J^T J of the point-to-plane sums."""
        a = np.zeros((6, 6))
        a[np.triu_indices(6)] = self.jtj
        return a + np.triu(a, 1).T

    @property
    def rms(self) -> float:
        """Root mean square of what the mode minimises over the accepted rows: the point distance (the square root of the
        mean squared distance) for point-to-point, the distance to the tangent plane for point-to-plane; NaN when no
        row was accepted."""
        if self.count == 0:
            return float("nan")
        return float(np.sqrt((self.sum_rr if self.plane else self.sum_distance) / self.count))

    def solve(self) -> np.ndarray:
        """The rigid increment as a 4 x 4 float64 matrix: applied AFTER the pose the sums were taken at.  Point-to-point:
        Kabsch -- H = sum_qp - sum_q sum_p^T / count, its SVD with the determinant fix, t = mean_p - R mean_q.
        Point-to-plane: jtj x = -jtr, the exponential map of the rotation part.  Raises below 3 (6) accepted rows."""
        need = 6 if self.plane else 3
        if self.count < need:
            raise ValueError(f"align_step accepted {self.count} rows; the {'point-to-plane' if self.plane else 'point-to-point'} "
                             f"solve needs at least {need}")
        return solve_align_sums(self.record[0], self.plane)


def solve_align_sums(rec, plane: bool) -> np.ndarray:
    """:meth:`AlignSums.solve` on anything with the fields of :data:`ALIGN_SUMS` (the tests hand in exact sums)."""
    inc = np.eye(4)
    if plane:
        a = np.zeros((6, 6))
        a[np.triu_indices(6)] = np.asarray(rec["jtj"], dtype=np.float64)
        a = a + np.triu(a, 1).T
        x = np.linalg.solve(a, -np.asarray(rec["jtr"], dtype=np.float64))
        w, angle = x[:3], float(np.linalg.norm(x[:3]))
        k = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        if angle < 1e-12:
            rot = np.eye(3) + k
        else:  # Rodrigues
            rot = np.eye(3) + (np.sin(angle) / angle) * k + ((1.0 - np.cos(angle)) / (angle * angle)) * (k @ k)
        inc[:3, :3], inc[:3, 3] = rot, x[3:]
        return inc
    n = float(rec["count"])
    sq, sp = np.asarray(rec["sum_q"], dtype=np.float64), np.asarray(rec["sum_p"], dtype=np.float64)
    h = np.asarray(rec["sum_qp"], dtype=np.float64).reshape(3, 3) - np.outer(sq, sp) / n
    u, _, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    rot = vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T
    inc[:3, :3], inc[:3, 3] = rot, sp / n - rot @ (sq / n)
    return inc


class IcpResult:
    """What :func:`icp` returns: ``transform`` (4 x 4 float64, source -> target), ``poses`` (the pose after every
    iteration), ``rms`` (of every iteration's sums, taken BEFORE its increment), ``sums`` (the last :class:`AlignSums`),
    ``converged``."""

    def __init__(self, transform, poses, rms, sums, converged):
        self.transform, self.poses, self.rms, self.sums, self.converged = transform, poses, rms, sums, converged

    @property
    def iterations(self) -> int:
        return len(self.poses)


def icp(tree: KdTree, source, max_distance, normals=None, init=None, iterations: int = 30, min_delta: float = 1e-9,
        step=None) -> IcpResult:
    """Iterative closest point of ``source`` against the points of ``tree``: ``iterations`` times at most,
    :meth:`KdTree.align_step` at the current pose and the increment of :meth:`AlignSums.solve`.

    The pose is composed in float64 on the host; each call receives it rounded to float32 and ``source`` is never
    rewritten.  ``init``: the starting pose, a (4, 4) matrix (identity by default).  The loop ends early when no entry
    of an increment differs from the identity by ``min_delta`` or more.  ``normals``: the target's normals for
    point-to-plane steps.  ``step(pose32)`` -- ``pose32`` the (3, 4) float32 pose -- may replace the call that returns
    the :class:`AlignSums` of an iteration (the tests drive the loop through the library's host loop with it)."""
    pose = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    if pose.shape != (4, 4):
        raise ValueError("init must be a (4, 4) matrix")
    if step is None:
        def step(pose32):
            return tree.align_step(source, pose32, max_distance, normals)
    poses, rms, sums, converged = [], [], None, False
    for _ in range(int(iterations)):
        sums = step(np.ascontiguousarray(pose[:3, :], dtype=np.float32))
        rms.append(sums.rms)
        inc = sums.solve()
        pose = inc @ pose
        poses.append(pose.copy())
        if np.max(np.abs(inc - np.eye(4))) < min_delta:
            converged = True
            break
    return IcpResult(pose, poses, rms, sums, converged)


# ---- file I/O (the reference's PKD container, _pyco_tree/kd_tree.hpp:546-614) -------------------
_PKD_SIGNATURE = b"\x89PKD"
_PKD_VERSION = 1


def save_kd_tree(tree: KdTree, filename: str) -> None:
    """``pico_tree.save_kd_tree``: PKD header (signature, version, metric string) followed by the
    tree in the reference's kd_tree::save format.  The points are not stored."""
    metric = tree.metric_string.encode("ascii")
    with open(filename, "wb") as f:
        f.write(_PKD_SIGNATURE)
        f.write(np.uint32(_PKD_VERSION).tobytes())
        f.write(np.uint64(len(metric)).tobytes())
        f.write(metric)
        f.write(tree._serialize())


def load_kd_tree(pts, filename: str, device: int | None = None) -> KdTree:
    """``pico_tree.load_kd_tree``: rebuilds a :class:`KdTree` over ``pts`` from a file written by
    :func:`save_kd_tree` or by the reference's own ``save_kd_tree`` (any of its metrics; the dtype of
    ``pts`` -- float32 or float64 -- must be the one the tree was built over)."""
    with open(filename, "rb") as f:
        data = f.read()
    if data[:4] != _PKD_SIGNATURE:
        raise RuntimeError("unexpected header signature")
    if int(np.frombuffer(data, dtype=np.uint32, count=1, offset=4)[0]) != _PKD_VERSION:
        raise RuntimeError("unsupported header version")
    n = int(np.frombuffer(data, dtype=np.uint64, count=1, offset=8)[0])
    metric = data[16:16 + n].decode("ascii", "replace")
    if metric not in Metric.__members__:  # kd_tree.hpp:588-598
        raise RuntimeError("unexpected metric string")
    return KdTree(pts, Metric[metric], 1, device=device, _stream=data[16 + n:])
