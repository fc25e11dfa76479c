"""The top levels of ptk_tree_create_from_points built on the device (pico_tree_amd/csrc/ptk_build.hpp): the tree
must be the one the host builder makes -- nodes, permutation, outer bounds -- and therefore the reference's
(tests/test_oracle.py pins the host builder to the compiled reference node for node).

device_top_build answers every difficulty with "build it on the host", and the two trees are then identical by
construction: every comparison here goes with the record of how the handle was built (``KdTree.create_route()``,
ptk_debug_create_route), so that a build that never ran on the device fails the test instead of passing it."""
import numpy as np
import pytest

import oracle
import pico_tree_amd as pt
from pico_tree_amd import datasets as ds

pytestmark = pytest.mark.gpu

N0 = 1 << 18  # the smallest cloud whose top levels are built on the device
TOO_MANY = "too many sliding planes in the top levels"


def outer_bounds(tree):
    out = np.empty((tree.info()["n_nodes"], 2), dtype=np.float32)
    assert pt._load().ptk_tree_get_outer_bounds(tree._h, out.ctypes.data) == 0
    return out


def assert_same_tree(host, other, what=""):
    for x, y in zip(host.flat(), other.flat()):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), what
    assert other.info() == host.info(), what
    assert outer_bounds(other).tobytes() == outer_bounds(host).tobytes(), what


def assert_on_device(tree, what=""):
    route = tree.create_route()
    assert route["on_device"] == 1, (what, "built on the host: " + route["why"], route)
    assert route["why"] == "" and route["levels"] >= 1 and route["subtrees"] == route["top_branches"] + 1, (what, route)
    return route


def assert_on_host(tree, why, what=""):
    route = tree.create_route()
    assert route["on_device"] == 0 and route["why"] == why, (what, route)
    return route


def build_pair(pts, leaf, gpu, monkeypatch, threads="64"):
    """(the PTK_DEVICE_BUILD=0 handle, the PTK_DEVICE_BUILD=1 handle) of the same points."""
    monkeypatch.setenv("PTK_BUILD_THREADS", threads)
    monkeypatch.setenv("PTK_DEVICE_BUILD", "0")
    host = pt.KdTree(pts, pt.Metric.L2Squared, leaf, device=gpu)
    assert_on_host(host, "PTK_DEVICE_BUILD=0" if len(pts) >= N0 else "fewer than 2^18 points")
    monkeypatch.setenv("PTK_DEVICE_BUILD", "1")
    return host, pt.KdTree(pts, pt.Metric.L2Squared, leaf, device=gpu)


def _clouds():
    rng = np.random.default_rng(5)
    yield "uniform", ds.uniform_cloud(700_000, 3, 11)
    pts, _ = ds.config2_clouds("L", 1_200_000, 10)
    yield "lidar", pts
    sheets = ds.uniform_cloud(600_000, 3, 12)
    sheets[::3, 2] *= np.float32(1e-4)  # a dense sheet: lopsided splits, many levels above the threshold
    sheets[1::7] = sheets[::7][: len(sheets[1::7])]  # exact duplicates (ties on every plane they touch)
    yield "sheets+duplicates", sheets
    yield "2-d", np.ascontiguousarray(ds.uniform_cloud(500_000, 3, 13)[:, :2])
    yield "5-d", rng.random((400_000, 5), dtype=np.float32)
    quant = np.round(ds.uniform_cloud(600_000, 3, 14) / np.float32(0.01)) * np.float32(0.01)  # points ON the planes
    yield "quantised", quant.astype(np.float32)


@pytest.mark.parametrize("threads", ["3", "64"])
def test_device_built_tree_is_the_host_built_tree(gpu, monkeypatch, threads):
    monkeypatch.setenv("PTK_BUILD_THREADS", threads)
    for name, pts in _clouds():
        monkeypatch.setenv("PTK_DEVICE_BUILD", "0")
        host = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
        assert_on_host(host, "PTK_DEVICE_BUILD=0", name)
        monkeypatch.setenv("PTK_DEVICE_BUILD", "1")
        dev = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
        assert_on_device(dev, name)
        assert outer_bounds(dev).tobytes() == outer_bounds(host).tobytes(), name
        a, b = host.flat(), dev.flat()
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), name
        assert dev.info() == host.info(), name
        q = np.ascontiguousarray(pts[:: max(1, len(pts) // 2000)])
        if pts.shape[1] <= 3:
            assert dev.search_knn(q, 4).tobytes() == host.search_knn(q, 4).tobytes(), name


@pytest.mark.parametrize("case", ["far-max", "far-min", "far-max-quantised", "far-min-duplicates"])
def test_planes_that_slide_in_the_top_levels(gpu, monkeypatch, case):
    """Most of the root box empty along its longest side: the first partitions leave one side empty and the builder
    slides the plane (std::nth_element).  The first rounds of libstdc++'s introselect run on the device (the Hoare
    partitions of ptk_build.hpp: pairing of left and right stops by rank), the rest of the same call on the host:
    the permutation -- and with it the tree -- must be the host's to the last index.  Far point beyond the maximum
    (nth = last - 1: the ranges shrink from the left) and below the minimum (nth = first + 1: from the right);
    coordinates on a grid (thousands of elements EQUAL to the pivot: both kinds of stop at once) and exact duplicates."""
    pts = ds.uniform_cloud(1_500_000, 3, 21)
    pts[:, 0] *= np.float32(0.2)
    if "quantised" in case:
        pts[:, 0] = np.round(pts[:, 0] / np.float32(0.002)) * np.float32(0.002)
    if "duplicates" in case:
        pts[1::5] = pts[::5][: len(pts[1::5])]
    pts[0, 0] = np.float32(50.0) if "max" in case else np.float32(-50.0)  # the box is long in x, the cloud at one end
    monkeypatch.setenv("PTK_DEVICE_BUILD", "0")
    host = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    assert_on_host(host, "PTK_DEVICE_BUILD=0")
    monkeypatch.setenv("PTK_DEVICE_BUILD", "1")
    dev = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    route = assert_on_device(dev)
    assert route["slides"] >= 1 and route["slide_rounds_device"] >= 1, route
    for x, y in zip(host.flat(), dev.flat()):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert_same_tree(host, dev)
    pt.set_test_knobs(device_slide_off=1)  # (the round trip to the host for the whole range: the same tree)
    dev2 = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    route = assert_on_device(dev2)
    assert route["slide_rounds_device"] == 0 and route["slides_host_whole"] >= 1 and route["slides"] >= 1, route
    for x, y in zip(host.flat(), dev2.flat()):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert_same_tree(host, dev2)


# ---- the smallest shapes the device build accepts ------------------------------------------------------------------
# A build of 2^18 points takes tens of milliseconds.  Every case compares flat(), info() and the outer bounds with the
# PTK_DEVICE_BUILD=0 handle and asserts the route it expects.

@pytest.mark.parametrize("n", [N0 - 1, N0, N0 + 1, N0 + 255, N0 + 256, N0 + 257])
def test_the_boundary_between_the_host_and_the_device_build(gpu, monkeypatch, n):
    """2^18 points: the grid of the position kernels is (n + 256) / 256 blocks and position n is written."""
    host, dev = build_pair(ds.uniform_cloud(n, 3, 31), 10, gpu, monkeypatch)
    if n < N0:
        assert_on_host(dev, "fewer than 2^18 points")
    else:
        route = assert_on_device(dev)
        assert route["threshold"] == 16384 and route["levels"] >= 4, route
    assert_same_tree(host, dev)


@pytest.mark.parametrize("dim", [1, 4, 8, 9])
def test_dimensions_up_to_the_limit_and_one_beyond(gpu, monkeypatch, dim):
    rng = np.random.default_rng(40 + dim)
    host, dev = build_pair(rng.random((N0, dim), dtype=np.float32), 10, gpu, monkeypatch)
    if dim <= 8:
        assert_on_device(dev)
    else:
        assert_on_host(dev, "shape not supported")
    assert_same_tree(host, dev)


@pytest.mark.parametrize("leaf", [1, 4095])
def test_leaf_sizes(gpu, monkeypatch, leaf):
    """4 095 is the largest leaf a device handle of 2^18 points takes (19 + 12 bits of a leaf reference), so on such a
    handle the threshold never is the leaf size: that branch of the rule runs on the CPU tier only
    (tests/test_build_emulation.py takes the threshold as a parameter)."""
    host, dev = build_pair(ds.uniform_cloud(N0 + 3, 3, 33), leaf, gpu, monkeypatch)
    assert assert_on_device(dev)["threshold"] == 16384
    assert_same_tree(host, dev)


def test_a_leaf_size_the_device_handle_refuses(gpu, monkeypatch):
    """Leaf 20 000: the device build runs (threshold 20 000), the handle cannot encode the leaves: the same refusal
    from both settings."""
    pts = ds.uniform_cloud(N0 + 3, 3, 33)
    monkeypatch.setenv("PTK_BUILD_THREADS", "64")
    errors = []
    for setting in ("0", "1"):
        monkeypatch.setenv("PTK_DEVICE_BUILD", setting)
        with pytest.raises(pt.PtkError) as err:
            pt.KdTree(pts, pt.Metric.L2Squared, 20_000, device=gpu)
        errors.append(str(err.value))
    assert errors[0] == errors[1] and "leaf reference" in errors[0], errors


@pytest.mark.parametrize("threads,threshold,levels", [("1", (N0 + 5) // 8, 4), ("64", 16384, 5)])
def test_thresholds_from_the_number_of_build_threads(gpu, monkeypatch, threads, threshold, levels):
    """One thread: the threshold is n / 8, three levels of halving bring the nodes to about that, and those of the eight
    that are still above it make a fourth (counted by tests/cpp/emulate_build_main.cpp on this cloud, as the five of the
    threshold of 16 384)."""
    host, dev = build_pair(ds.uniform_cloud(N0 + 5, 3, 34), 10, gpu, monkeypatch, threads)
    route = assert_on_device(dev)
    assert route["threshold"] == threshold and route["levels"] == levels, route
    assert_same_tree(host, dev)


@pytest.mark.parametrize("order", ["ascending", "descending", "uniform"])
def test_input_orders(gpu, monkeypatch, order):
    """Sorted along x: the first partition swaps nothing; sorted the other way: it swaps every pair."""
    pts = ds.uniform_cloud(N0 + 77, 3, 35)
    pts[:, 0] *= np.float32(2)  # (x is the axis of the root)
    if order != "uniform":
        pts = np.ascontiguousarray(pts[np.argsort(pts[:, 0] if order == "ascending" else -pts[:, 0], kind="stable")])
    host, dev = build_pair(pts, 10, gpu, monkeypatch)
    assert_on_device(dev)
    assert_same_tree(host, dev)


def cluster_cloud():
    """A cluster of 22 000 points in a ball of radius 1e-4 around (3, 0.5, 0.5) beside a uniform unit cube (2^18 points
    in all): the cluster is the right child of the root -- above the threshold of 16 384, below the 32 768 a slide needs
    for its device rounds -- and its box is empty along x but for its far end, so its plane slides (nth = 1) and the host
    takes the range whole.  tests/cpp/emulate_build_main.cpp says so with the driver's thresholds: 1 slide, taken whole."""
    rng = np.random.default_rng(36)
    d = rng.normal(size=(22_000, 3))
    d *= (rng.random((22_000, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True) * 1e-4
    ball = (np.array([3, 0.5, 0.5]) + d).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([ds.uniform_cloud(N0 - 22_000, 3, 36), ball]))


def test_a_slide_the_host_takes_whole(gpu, monkeypatch):
    host, dev = build_pair(cluster_cloud(), 10, gpu, monkeypatch)
    route = assert_on_device(dev)
    assert route["slides_host_whole"] >= 1, route
    assert_same_tree(host, dev)


def ladder_cloud(rungs_x, rungs_y):
    """2^18 uniform points, some of them moved out to x = 8, 64, 512 ... and others to y = 8, 64 ...: once the largest is
    split off, the box of the rest reaches to half of it and the next one lies below a quarter -- nothing on the right of
    the middle, the plane slides (nth = len - 1, on all of the cloud: device rounds) and peels that one off.  A rung, a
    slide.  (A pile of coincident points above the threshold of 16 384 would do the same, but the 8 192 levels of the
    builder and the 4 095 points of a device handle's leaf do not leave room for one.)"""
    pts = ds.uniform_cloud(N0, 3, 37)
    pts[1000:1000 + rungs_x, 0] = np.float32(8) ** np.arange(1, rungs_x + 1, dtype=np.float32)
    pts[5000:5000 + rungs_y, 1] = np.float32(8) ** np.arange(1, rungs_y + 1, dtype=np.float32)
    return pts


@pytest.mark.parametrize("rungs_y,slides", [(23, 64), (24, None)])
def test_the_limit_of_64_sliding_planes(gpu, monkeypatch, rungs_y, slides):
    """Counted by tests/cpp/emulate_build_main.cpp with the driver's thresholds first: 41 + 23 rungs are 64 slides, the
    last the build accepts; with one more it gives up at the 65th."""
    host, dev = build_pair(ladder_cloud(41, rungs_y), 10, gpu, monkeypatch)
    if slides is not None:
        route = assert_on_device(dev)
        assert route["slides"] == slides and route["slides"] >= 40 and route["slide_rounds_device"] >= slides, route
    else:
        assert assert_on_host(dev, TOO_MANY)["slides"] == 65
    assert_same_tree(host, dev)


# (Not here: 2^18 copies of one point.  Both settings end in the host builder's refusal of a tree deeper than 8 192
# levels -- the device build gives up at its 65th sliding plane first -- but the host builder alone takes some twelve
# seconds to get there: std::nth_element over the whole cloud, 8 192 times.  tests/test_cabi.py has the refusal on a
# small cloud, the limit of 64 is above.)


@pytest.mark.parametrize("cloud", ["uniform", "sliding"])
def test_the_stream_of_a_device_built_tree_is_the_reference_s(gpu, monkeypatch, cloud):
    pts = ds.uniform_cloud(N0, 3, 38)
    if cloud == "sliding":  # (the cloud of test_planes_that_slide_in_the_top_levels, at 2^18 points)
        pts[:, 0] *= np.float32(0.2)
        pts[0, 0] = np.float32(50.0)
    monkeypatch.setenv("PTK_BUILD_THREADS", "64")
    monkeypatch.setenv("PTK_DEVICE_BUILD", "1")
    dev = pt.KdTree(pts, pt.Metric.L2Squared, 10, device=gpu)
    route = assert_on_device(dev)
    if cloud == "sliding":
        assert route["slides"] >= 1 and route["slide_rounds_device"] >= 1, route
    kind = "reference" if oracle.have_reference() else "port"
    assert dev._serialize() == oracle.Oracle(pts, 10, kind).save_bytes(), kind
