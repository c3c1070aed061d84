"""The integer rules of ws_store_fuse (ws_fuse.h) held to plain uint64 / int64 / __int128 arithmetic on the GPU itself
(tests/cpp/fuse_units.hip).  The whole-call tests reach these helpers only through whole maps, at four resolutions and with values
from the middle of their domains.

fuse_div with make_fuse_div: for every res in 1 .. 1024 the quotient boundaries of res^3 over fuse_sample's whole numerator range
[0, 2^16 res^3); and the routine's own claim (n < 2^47, d <= 2^30) at powers of two, their neighbours and 4096 random divisors.
Both shift branches (k < 64, k >= 64) must have been taken by some divisor.
fuse_pull against a true floor in __int128 at rot entries +-2^30, the ends of base, sums within +-2 of a multiple of 2^30 on both
signs and pivots at the ends of int32; fuse_dead on both sides of +-2^30.
fuse_integrate: all 2^32 pairs (ev, nv) of int16 values for each of twelve weight triples (ew, nw, max_weight), not thinned (stride
1), and 2^24 random quintuples.
fuse_sample on seven chunks around the origin with the eighth absent, found through store_ray_table_fill's table and two segments:
cells whose corners all hold -32768, all 32767, a mix, random values, a zero or a negative weight or lie in an absent chunk (at
least 1000 of each, and of the cells whose shifted numerator is 0 and at its maximum), at ten resolutions, b on both sides of every
chunk face, edge and corner, f from {0, 1, res / 2, res - 1} and random.

Every line must report `mismatches 0` and exactly the number of cases derived here."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def claim_cases():
    """the cases of the `fuse_div claim` line: per divisor j d - 1 and j d for j = 1 .. 1024 and for the last 1024 multiples below
    2^47 (each j once, and only those that exist), the largest n, and 2^16 random n"""
    divs = [(1 << e) + o for e in range(31) for o in (-1, 0, 1) if 1 <= (1 << e) + o <= 1 << 30]
    for t in range(4096):
        h = mix64(0xD1D + t)
        divs.append(1 + ((h % (1 << 30)) >> (mix64(h) % 30 if t & 1 else 0)))
    assert len(divs) == 91 + 4096 and min(divs) == 1 and max(divs) == 1 << 30
    total = 0
    for d in divs:
        jmax = ((1 << 47) - 1) // d
        total += 2 * (min(1024, jmax) + min(1024, max(jmax - 1024, 0))) + 1 + (1 << 16)
    return total


def expected_counts():
    return {"fuse_div res^3": 1024 * 262144 - 1,
            "fuse_div claim": claim_cases(),
            "fuse_pull": 7 * 5 * 5 * (2 + 64 * 5 + (1 << 14)),
            "fuse_dead": 11,
            "fuse_integrate pairs": 12 << 32,
            "fuse_integrate random": 1 << 24,
            "fuse_sample": 10 * (15 ** 3 * 64 + (1 << 20))}


def test_fuse_helpers_match_plain_integer_arithmetic(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "fuse_units"
    # the library's own compiler flags: division and contraction are those of the kernels
    subprocess.check_call([B.hipcc(), *B.flags(), os.path.join(ROOT, "tests", "cpp", "fuse_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "mismatches" in ln]
    want = expected_counts()
    assert len(lines) == len(want) and all(ln.rstrip().endswith("mismatches 0") for ln in lines), out.stdout
    checked = {ln.split("checked")[0].strip(): int(ln.split("checked")[1].split()[0]) for ln in lines}
    assert checked == want, (checked, want)
    # both shift branches of fuse_div were taken
    branches = re.findall(r"^fuse_div branches\s+k < 64: (\d+) divisors\s+k >= 64: (\d+) divisors$", out.stdout, re.M)
    assert len(branches) == 1 and int(branches[0][0]) > 0 and int(branches[0][1]) > 0, out.stdout
