#!/usr/bin/env python3
"""Is the device code of two builds the same?  For every object file of the library in either of two build directories: take the
gfx950 code object out of the fat binary, disassemble it and compare -- the whole listing (addresses and encodings included), and
the kernels' names and register / scratch / LDS figures from the code object's metadata.  An object that only one build has (a
renamed or split host file) counts as one without device code there: it compares equal iff the other side has none either.  Runs
without a GPU.

    python tools/device_code_diff.py OTHER_TREE/warpsense_amd/build warpsense_amd/build [--json out.json]

--by-kernel compares kernel by kernel instead, in whatever object a kernel lies (kernels that moved between files): the same four
figures, and the kernel's own instructions -- offset from the kernel's first instruction, text, encoding, and a branch's target as an
offset from the same start -- so that neither the object's name nor the kernel's place in it counts.  A kernel that only one build
has, or that one build has twice, is a difference.

Both trees are built with the same flags (python -m warpsense_amd.build --force).  Exit status 1 if any file (any kernel) differs."""
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


def code_object(obj, tmp, sizes=None):
    """(listing, {kernel: figures}) of the object's gfx950 code; `sizes`, if given, is filled with {function symbol: bytes of code}"""
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    if not os.path.exists(obj) or ".hip_fatbin" not in run(os.path.join(LLVM, "llvm-objdump"), "-h", obj):
        return [], {}  # not in this build, or host code only (the api_*.hip files have no kernels)
    run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}", f"--output={co}")
    listing = run(os.path.join(LLVM, "llvm-objdump"), "-d", co).split("\n")[2:]  # (the first lines name the file)
    kernels, cur = {}, {}
    for ln in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).split("\n"):
        # the fields of one kernel: an item of amdhsa.kernels, in alphabetical order (its arguments' fields are indented further)
        m = re.match(r"(  - |    )\.(\w+):\s+(\S+)", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if m.group(2) == "name":
            kernels[m.group(3)] = cur
        elif m.group(2) in FIGURES:
            cur[m.group(2)] = int(m.group(3))
    if sizes is not None:
        for ln in run(os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", co).split("\n"):
            f = ln.split()
            if len(f) == 8 and f[3] == "FUNC":
                sizes[f[7]] = int(f[2], 0)
    return listing, kernels


def by_symbol(listing, sizes):
    """{symbol: its instructions as 'offset: text // encoding <symbol+target>'} -- nothing in a line depends on where the symbol lies;
    the padding between two symbols belongs to neither"""
    out, cur, base = {}, None, 0
    for ln in listing:
        m = re.match(r"([0-9a-f]+) <(.+)>:$", ln)
        if m:
            base, cur = int(m.group(1), 16), out.setdefault(m.group(2), [])
            size = sizes.get(m.group(2), 1 << 62)
            continue
        m = re.match(r"\t(.*?)\s*// ([0-9A-Fa-f]+): (.*)$", ln)
        if m and cur is not None and int(m.group(2), 16) - base < size:
            cur.append(f"{int(m.group(2), 16) - base:#x}: {m.group(1)} // {m.group(3)}")
    return out


def kernels_of(build_dir):
    """{kernel: {"object", "figures", "listing"}} over every object of a build, and the kernels that more than one object defines"""
    found, twice = {}, []
    for name in sorted(f for f in os.listdir(build_dir) if f.endswith(".o")):
        sizes = {}
        with tempfile.TemporaryDirectory() as tmp:
            listing, kernels = code_object(os.path.join(build_dir, name), tmp, sizes)
        code = by_symbol(listing, sizes)
        for k, figures in kernels.items():
            if k in found:
                twice.append(k)
            found[k] = {"object": name, "figures": figures, "listing": code.get(k, [])}
    return found, twice


def main_by_kernel(a_dir, b_dir):
    (ka, twice_a), (kb, twice_b) = kernels_of(a_dir), kernels_of(b_dir)
    report, differ = {}, False
    for k in sorted(set(ka) | set(kb)):
        a, b = ka.get(k), kb.get(k)
        entry = {"object_a": a and a["object"], "object_b": b and b["object"]}
        if a is None or b is None:
            entry["identical"], entry["only_in"] = False, "a" if b is None else "b"
        else:
            entry["identical"] = a["figures"] == b["figures"] and a["listing"] == b["listing"] and len(a["listing"]) > 0 and k not in twice_a + twice_b
            entry["instructions"] = max(len(a["listing"]), len(b["listing"]))
            entry["figures"] = a["figures"]
            if not entry["identical"]:
                entry["figures_b"] = b["figures"]
                entry["diff"] = [d for d in difflib.unified_diff(a["listing"], b["listing"], "a", "b", lineterm="", n=0)][:200]
        if k in twice_a + twice_b:
            entry["defined_twice_in"] = [side for side, t in (("a", twice_a), ("b", twice_b)) if k in t]
        differ |= not entry["identical"]
        report[k] = entry
        where = entry["object_a"] if entry["object_a"] == entry["object_b"] else f"{entry['object_a']} -> {entry['object_b']}"
        print(f"{'identical' if entry['identical'] else 'DIFFERENT'}  {entry.get('instructions', 0):>6} instructions  {where:<36} {k}")
        if not entry["identical"]:
            print("\n".join(entry.get("diff", [])[:40]))
    return report, differ


def instructions(listing):
    return sum(1 for ln in listing if ln.startswith("\t"))


def main_by_file(a_dir, b_dir):
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
    return report, differ


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    report, differ = (main_by_kernel if "--by-kernel" in sys.argv else main_by_file)(a_dir, b_dir)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(report, f, indent=1)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
