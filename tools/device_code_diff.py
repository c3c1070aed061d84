#!/usr/bin/env python3
"""Is the device code of two builds the same?  For every object file of the library in either of two build directories: take the
gfx950 code object out of the fat binary, disassemble it and compare -- the whole listing (addresses and encodings included), and
the kernels' names and register / scratch / LDS figures from the code object's metadata.  An object that only one build has (a
renamed or split host file) counts as one without device code there: it compares equal iff the other side has none either.  Runs
without a GPU.

    python tools/device_code_diff.py OTHER_TREE/warpsense_amd/build warpsense_amd/build [--json out.json]

Both trees are built with the same flags (python -m warpsense_amd.build --force).  Exit status 1 if any file differs."""
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIGURES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True).stdout


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    if not os.path.exists(obj) or ".hip_fatbin" not in run(os.path.join(LLVM, "llvm-objdump"), "-h", obj):
        return [], {}  # not in this build, or host code only (the api_*.hip files have no kernels)
    run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}", f"--output={co}")
    listing = run(os.path.join(LLVM, "llvm-objdump"), "-d", co).split("\n")[2:]  # (the first lines name the file)
    kernels, cur = {}, None
    for ln in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).split("\n"):
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", ln)
        if not m:
            continue
        if m.group(1) == "name" and m.group(2).startswith("_Z"):
            cur = kernels.setdefault(m.group(2), {})
        elif m.group(1) in FIGURES and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return listing, kernels


def instructions(listing):
    return sum(1 for ln in listing if ln.startswith("\t"))


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    report, differ = {}, False
    for name in sorted({f for d in (a_dir, b_dir) for f in os.listdir(d) if f.endswith(".o")}):
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            la, ka = code_object(os.path.join(a_dir, name), ta)
            lb, kb = code_object(os.path.join(b_dir, name), tb)
        same = la == lb and ka == kb
        entry = {"identical": same, "kernels": max(len(ka), len(kb)), "instructions": max(instructions(la), instructions(lb))}
        missing = [side for side, d in (("a", a_dir), ("b", b_dir)) if not os.path.exists(os.path.join(d, name))]
        if missing:
            entry["only_in"] = "b" if missing == ["a"] else "a"
        if not same:
            differ = True
            entry["kernels_a"], entry["kernels_b"] = ka, kb
            entry["diff"] = [d for d in difflib.unified_diff(la, lb, "a", "b", lineterm="", n=0)][:200]
        report[name] = entry
        print(f"{name:<24} {'identical' if same else 'DIFFERENT'}  {entry['kernels']} kernels, {entry['instructions']} instructions")
        if not same:
            print("\n".join(entry["diff"][:40]))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(report, f, indent=1)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
