"""CPU tier: the dispatch helpers of the launch layer (pico_tree_amd/csrc/ptk_dispatch.hpp) in tests/cpp/dispatch_main.cpp,
a stand-alone host program built with -fsanitize=address,undefined (nothing sanitized is loaded into this process): the
slot ladders for k = 0 .. 200, the boolean tags, the spill classes and the four metric sets against the ladders, macros
and switches they replaced.  The program exits non-zero on the first difference and names it."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_helpers_pick_what_the_ladders_picked(tmp_path):
    exe = str(tmp_path / "dispatch_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "pico_tree_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "dispatch_main.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "dispatch OK", (res.returncode, res.stdout, res.stderr[-2000:])
