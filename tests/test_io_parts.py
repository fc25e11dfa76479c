"""CPU tier: where the parts of a host-buffer call lie inside a device block (pico_tree_amd/csrc/ptk_io_parts.hpp) in
tests/cpp/io_parts_main.cpp, a stand-alone host program built with -fsanitize=address,undefined (nothing sanitized is
loaded into this process): the part lists of every fixed-row host entry point, sizes of 0 / 1 / 15 / 16 / 17 bytes, every
subset of the optional parts absent -- offsets on 16-byte boundaries, no overlap, a null pointer for an absent part that
moves no other part, and the total the blocks are grown to.  The program exits non-zero on the first difference and names
it."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_io_parts_layout(tmp_path):
    exe = str(tmp_path / "io_parts_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "io_parts_main.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "io_parts OK", (res.returncode, res.stdout, res.stderr[-2000:])
