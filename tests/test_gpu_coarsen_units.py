"""The rule of ws_store_coarsen (ws_coarsen.h) run on the GPU itself and held to a plain restatement on the host of the same program
(tests/cpp/coarsen_units.hip).  The whole-call tests reach the rule only through whole chunks, with sums from the middle of its domain.

coarsen_div: every S in -262144 .. 262136 (eight int16 values) for every n in 1 .. 8 against the built-in division with an explicit
floor.
coarsen_add and coarsen_entry: eight children, every assignment of the weights {-5, 0, 1, 32767} (4^8), every min_observed in
1 .. 8, and sixteen sets of values: all -32768, all 32767, S = -1, and thirteen drawn from the ends of int16, +-1 and random.

Every line must report `mismatches 0` and exactly the number of cases derived here."""
import math
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected_counts():
    return {"coarsen_div": 8 * (262136 + 262144 + 1), "coarsen_entry": 16 * 8 * 4 ** 8}


def expected_fill():
    """the cases whose entry is fill: of the 4^8 weight assignments C(8, n) 2^8 have n observed children (two of the four weights
    are > 0); fill iff n < min_observed"""
    with_n = [math.comb(8, n) * 256 for n in range(9)]
    assert sum(with_n) == 4 ** 8
    return 16 * sum(sum(with_n[:m]) for m in range(1, 9))


def test_coarsen_rule_matches_plain_integer_arithmetic(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "coarsen_units"
    # the library's own compiler flags: the multiply-shift is that of the kernel
    subprocess.check_call([B.hipcc(), *B.flags(), os.path.join(ROOT, "tests", "cpp", "coarsen_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "mismatches" in ln]
    want = expected_counts()
    assert len(lines) == len(want) and all(ln.rstrip().endswith("mismatches 0") for ln in lines), out.stdout
    checked = {ln.split("checked")[0].strip(): int(ln.split("checked")[1].split()[0]) for ln in lines}
    assert checked == want, (checked, want)
    kinds = re.findall(r"^coarsen_entry kinds\s+fill: (\d+)\s+value: (\d+)$", out.stdout, re.M)
    assert len(kinds) == 1 and int(kinds[0][0]) == expected_fill() and int(kinds[0][1]) == want["coarsen_entry"] - expected_fill(), out.stdout
