#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel symbol between two builds of libptk (no GPU needed).

  python tools/diff_kernel_disasm.py OLD_OBJ_DIR NEW_OBJ_DIR

Each directory is a pico_tree_amd/csrc/_obj of a build.  The device code object of every unit is taken out of the
object's .hip_fatbin section (clang-offload-bundler), disassembled (llvm-objdump) and split per symbol; branch-target
comments are dropped.  Prints, per unit, the symbols of the old build that are missing in the new one, those only in
the new one, and every symbol whose instructions differ, and closes each unit with the size (instructions) and one
SHA-256 over the old build's symbols as each build has them.  Exit status 1 if a symbol of the old build is missing or
differs.
"""
from __future__ import annotations

import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def disassemble(obj: str, work: str) -> dict:
    fat = os.path.join(work, os.path.basename(obj) + ".fatbin")
    co = os.path.join(work, os.path.basename(obj) + ".co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    targets = subprocess.check_output([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o",
                                       "--input=" + fat], text=True).split()
    target = next(t for t in targets if "gfx950" in t)
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=" + target, "--input=" + fat, "--output=" + co])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn",
                                    "--no-leading-addr", co], text=True)
    funcs, cur = {}, None
    for line in text.splitlines():
        if line and not line[0].isspace() and line.rstrip().endswith(">:"):
            cur = line.split("<", 1)[1].rstrip()[:-2]
            funcs[cur] = []
        elif cur is not None:
            line = re.sub(r"// [0-9A-Fa-f]+:.*", "", line).rstrip()
            if line and line.strip() != "...":  # (alignment fill after the last function of a section)
                funcs[cur].append(line)
    return funcs


def main() -> int:
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    bad = 0
    with tempfile.TemporaryDirectory() as work:
        for old in sorted(glob.glob(os.path.join(old_dir, "*.o"))):
            unit = os.path.basename(old)
            new = os.path.join(new_dir, unit)
            os.makedirs(os.path.join(work, "a"), exist_ok=True)
            os.makedirs(os.path.join(work, "b"), exist_ok=True)
            a, b = disassemble(old, os.path.join(work, "a")), disassemble(new, os.path.join(work, "b"))
            missing = [s for s in a if s not in b]
            differ = [s for s in a if s in b and a[s] != b[s]]
            print(f"{unit}: {len(a)} symbols, {len(missing)} missing, {len(differ)} differ, "
                  f"{len([s for s in b if s not in a])} new")
            for s in missing + differ:
                print("  ", "missing" if s in missing else "differs", s)
            for name, funcs in (("old", a), ("new", b)):
                h, n = hashlib.sha256(), 0
                for sym in sorted(a):
                    body = funcs.get(sym, [])
                    n += len(body)
                    h.update(sym.encode() + b"\0" + "\n".join(body).encode() + b"\0")
                print(f"   {name}: {n} instructions in these symbols, sha256 {h.hexdigest()[:32]}")
            bad += len(missing) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
