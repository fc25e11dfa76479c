"""CPU tier: the kernels of the device tree build (pico_tree_amd/csrc/ptk_kernels_build.hpp) run lane by lane in
tests/cpp/emulate_build_main.cpp, in the launch sequence of ptk::device_top_build, and are checked inside that program
against the standard library on a copy of the same input: std::partition after every level, std::nth_element after
every slide, the host builder's tree at the end, a plain loop for the root box.  The program exits non-zero on the first
difference and names the level and the segment; here are the clouds -- the shapes where rank arithmetic breaks: ranges
that end on a block edge, nodes with no swap and with every position swapped, levels whose segments no longer cover the
permutation, pivots with thousands of equals -- and what a sweep has to have seen to count.

The program is built twice, the second time with -fsanitize=address,undefined as an executable of its own (nothing
sanitized is loaded into this process): its buffers have exactly the sizes the driver allocates, so a rank that lands
one past an end is a report, not a silent write."""
from __future__ import annotations

import concurrent.futures
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 255, 256, 257, 511, 512, 513, 1_000, 5_000)  # the grid is (n + 256) / 256 blocks: position n is written
FAMILIES = ("uniform", "ints", "ascending", "descending", "outlier-above", "outlier-below", "equal-but-one")
TOO_MANY = "too many sliding planes in the top levels"
WORKERS = max(1, min(8, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(plain, sanitized): tests/cpp/emulate_build_main.cpp compiled with the emulator's g++ line (__graft_entry__.build),
    and once more with the sanitizers; the two compilations run side by side."""
    d = tmp_path_factory.mktemp("emu_build")
    base = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-w",
            "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "emulate_build_main.cpp")]
    plain, sanitized = str(d / "emulate_build"), str(d / "emulate_build_san")
    jobs = [subprocess.Popen(base + ["-o", plain]),
            subprocess.Popen(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", sanitized])]
    assert [j.wait() for j in jobs] == [0, 0]
    return plain, sanitized


# ---- clouds ----------------------------------------------------------------------------------------------------------

def family_cloud(family, n, dim, seed):
    """(n, dim) float32; axis 0 is the longest side of the box, the one the root splits."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, dim), dtype=np.float32)
    p[:, 0] *= np.float32(2)
    if family == "ints":  # small integers 0 .. 3: ties, points on the planes
        p = rng.integers(0, 4, (n, dim)).astype(np.float32)
    elif family == "ascending":  # along the split axis: no swap
        p = p[np.argsort(p[:, 0], kind="stable")]
    elif family == "descending":  # every pair swaps
        p = p[np.argsort(-p[:, 0], kind="stable")]
    elif family == "outlier-above":  # nth = len - 1
        p[n // 2, 0] = np.float32(50)
    elif family == "outlier-below":  # nth = 1
        p[n // 2, 0] = np.float32(-50)
    elif family == "equal-but-one":
        p[:, 0] = np.float32(1)
        p[n // 3, 0] = np.float32(3)
    return np.ascontiguousarray(p, dtype=np.float32)


def structured_cases():
    """(name, points, leaf, threshold, host_below, box_blocks)."""
    for i_n, n in enumerate(SIZES):
        for dim in range(1, 9):
            for i_f, family in enumerate(FAMILIES):
                leaf = 10 if (i_n + dim) % 2 else 1
                # one node per level (only the root is above the threshold) | a few | as many as the leaf size allows
                threshold = (max(leaf, n - 1), max(leaf, n // 3), max(leaf, 16))[(i_n + dim + i_f) % 3]
                yield (f"{family}-n{n}-d{dim}-t{threshold}", family_cloud(family, n, dim, 1000 * i_n + 10 * dim + i_f), leaf,
                       threshold, 8, 3)
    for dim in (1, 3, 8):  # hundreds of nodes in a level: build_cut_kernel's grid of 64 has several blocks
        yield f"wide-d{dim}", family_cloud("uniform", 5_000, dim, 77 + dim), 10, 16, 8, 3
    yield "wide-full-box-grid", family_cloud("uniform", 5_000, 3, 99), 10, 16, 8, 1024  # (the driver's grid of build_box_kernel)
    rng = np.random.default_rng(5)
    for dim in (2, 3):  # lopsided: nine tenths of the points in a small clump, ranges reach the frontier at different levels
        p = rng.random((5_000, dim), dtype=np.float32)
        p[500:] = np.float32(0.9) + p[500:] * np.float32(0.01)
        yield f"lopsided-d{dim}", rng.permutation(p), 10, 64, 8, 3


SLIDE_LENGTHS = (9, 10, 33, 256, 257, 2_000)
SLIDE_PATTERNS = ("distinct", "all-equal", "two-values", "equal-to-pivot", "ascending", "descending", "organ-pipe")


def slide_cloud(pattern, length, side, seed):
    """A 2-d cloud whose second partition leaves one side empty: `length` values of the pattern in [1, 2] along axis 0,
    in this order, and one point far above them (placed last: nth = len - 1) or far below (placed first: nth = 1), so
    that the partition of the root moves nothing and the plane of the node of `length` points has to slide."""
    rng = np.random.default_rng(seed)
    v = np.float32(1) + rng.permutation(length).astype(np.float32) / np.float32(length)
    if pattern == "all-equal":
        v[:] = np.float32(1.5)
    elif pattern == "two-values":
        v = np.where(rng.random(length) < 0.5, np.float32(1.25), np.float32(1.75)).astype(np.float32)
    elif pattern == "equal-to-pivot":  # three quarters of the range ARE the pivot, whichever of the three is picked
        v[rng.random(length) < 0.75] = np.float32(1.5)
    elif pattern == "ascending":
        v = np.sort(v)
    elif pattern == "descending":
        v = np.sort(v)[::-1]
    elif pattern == "organ-pipe":
        s = np.sort(v)
        v = np.concatenate([s[::2], s[1::2][::-1]])
    p = np.empty((length + 1, 2), dtype=np.float32)
    p[:, 1] = rng.random(length + 1, dtype=np.float32) * np.float32(1e-3)
    if side == "above":
        p[:length, 0], p[length, 0] = v, np.float32(100)
    else:
        p[1:, 0], p[0, 0] = v, np.float32(-100)
    return p


def slide_cases():
    for i_l, length in enumerate(SLIDE_LENGTHS):
        for i_p, pattern in enumerate(SLIDE_PATTERNS):
            for side in ("above", "below"):
                yield (f"slide-{pattern}-{length}-{side}", slide_cloud(pattern, length, side, 100 * i_l + i_p), 4,
                       max(4, length // 4), 8, 3)


def random_cases(count=150):
    rng = np.random.default_rng(2024)
    for i in range(count):
        n, dim = int(rng.integers(2, 600)), int(rng.integers(1, 9))
        family = FAMILIES[int(rng.integers(len(FAMILIES)))]
        leaf = int(rng.integers(1, 12))
        threshold = max(leaf, int(rng.integers(1, max(2, n // 2))))
        p = family_cloud(family, n, dim, 50_000 + i)
        if rng.random() < 0.3:  # coordinates on a coarse grid as well
            p = (np.round(p * np.float32(8)) / np.float32(8)).astype(np.float32)
        yield f"random-{i}-{family}-n{n}-d{dim}-t{threshold}", p, leaf, threshold, int(rng.integers(3, 40)), 2


# ---- running ---------------------------------------------------------------------------------------------------------

def run_cases(exe, cases, directory):
    """{name: counters}; fails with the program's own message on the first case that differs."""
    def one(item):
        i, (name, p, leaf, threshold, host_below, box_blocks) = item
        path = os.path.join(directory, f"{os.path.basename(exe)}_{i}.bin")
        p.tofile(path)
        res = subprocess.run([exe, path, str(p.shape[0]), str(p.shape[1]), str(leaf), str(threshold), str(host_below),
                              str(box_blocks)], capture_output=True, text=True)
        os.remove(path)
        return name, res

    out = {}
    with concurrent.futures.ThreadPoolExecutor(WORKERS) as pool:
        for name, res in pool.map(one, enumerate(cases)):
            assert res.returncode == 0, (name, res.returncode, res.stderr[-2000:])
            out[name] = json.loads(res.stdout)
    return out


def check_refusals(results):
    """The one refusal these clouds may meet is the driver's 64-slide limit, on the clouds of coincident coordinates."""
    for name, r in results.items():
        if r["on_device"] != 1:
            assert r["why"] == TOO_MANY and ("ints" in name or "equal-but-one" in name), (name, r)
            assert r["slides"] == 65, (name, r)
        else:
            assert r["why"] == "" and r["subtrees"] == r["top_branches"] + 1, (name, r)


@pytest.fixture(scope="module")
def structured(programs, tmp_path_factory):
    return run_cases(programs[0], list(structured_cases()), str(tmp_path_factory.mktemp("structured")))


@pytest.fixture(scope="module")
def slides(programs, tmp_path_factory):
    return run_cases(programs[0], list(slide_cases()), str(tmp_path_factory.mktemp("slides")))


def test_structured_cases_equal_the_standard_library(structured):
    assert len(structured) == len(SIZES) * 8 * len(FAMILIES) + 6
    check_refusals(structured)
    built = [r for r in structured.values() if r["on_device"] == 1]
    assert len(built) >= 0.9 * len(structured)
    for family in FAMILIES:  # every family is built to the end in every dimension
        for dim in range(1, 9):
            assert any(r["on_device"] == 1 for name, r in structured.items() if name.startswith(family) and f"-d{dim}-" in name), (family, dim)
    pick = lambda prefix: [r for name, r in structured.items() if name.startswith(prefix)]
    assert sum(r["segments_no_swap"] for r in pick("ascending")) >= 80  # (the root of every such cloud, at the least)
    assert sum(r["segments_all_swap"] for r in pick("descending")) >= 80
    for prefix in ("outlier-above", "outlier-below", "equal-but-one", "ints"):
        assert sum(r["slides"] for r in pick(prefix)) >= 20, prefix
        assert sum(r["slide_rounds_device"] for r in pick(prefix)) >= 20, prefix
    for r in pick("wide"):
        assert r["max_level_segments"] > 64 and r["on_device"] == 1, r
    for r in pick("lopsided"):
        assert r["on_device"] == 1 and r["levels"] >= 6 and r["max_level_unsegmented"] >= 500 and r["max_level_segments"] >= 2, r
    # one node per level, and a level of one node that is the whole permutation
    assert any(r["levels"] == 1 and r["max_level_unsegmented"] == 0 for r in structured.values())


def test_slides_equal_nth_element(slides):
    assert len(slides) == len(SLIDE_LENGTHS) * len(SLIDE_PATTERNS) * 2
    for name, r in slides.items():
        assert r["on_device"] == 1 and r["why"] == "", (name, r)
        assert r["slides"] >= 1, (name, r)
        if not r["introselect_checked"]:
            continue
        assert r["slide_rounds_device"] >= 1 and r["slides_host_whole"] < r["slides"], (name, r)
        if "equal-to-pivot-2000" in name:
            assert r["max_round_equal_to_pivot"] >= 1_000, (name, r)
        if "all-equal-2000" in name:
            assert r["max_round_equal_to_pivot"] >= 1_998, (name, r)


def test_every_outcome_of_the_median_of_three_occurs(structured, slides):
    if not all(r["introselect_checked"] for r in slides.values()):
        pytest.skip("the device rounds of a slide follow libstdc++'s introselect (releases 9 to 15): another standard library here")
    outcomes = np.zeros(6, dtype=np.int64)
    for r in list(structured.values()) + list(slides.values()):
        outcomes += np.asarray(r["pivot_outcomes"], dtype=np.int64)
    print("median of three, per outcome:", outcomes.tolist())
    assert (outcomes > 0).all(), outcomes.tolist()


def test_sanitized_program_on_the_structured_cases(programs, tmp_path):
    got = run_cases(programs[1], list(structured_cases()) + list(slide_cases()), str(tmp_path))
    check_refusals(got)


def test_random_sweep(programs, tmp_path):
    check_refusals(run_cases(programs[0], list(random_cases()), str(tmp_path)))


def test_arguments_out_of_range_are_refused(programs, tmp_path):
    path = str(tmp_path / "p.bin")
    np.zeros((4, 9), dtype=np.float32).tofile(path)
    for args in (("4", "9", "1", "1", "8"), ("1", "3", "1", "1", "8"), ("4", "3", "10", "2", "8"), ("400", "3", "1", "1", "8")):
        assert subprocess.run([programs[0], path, *args], capture_output=True).returncode == 2, args
