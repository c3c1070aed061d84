"""The rules of the ground layer (ws_ground.h) run on the GPU itself and held to a plain restatement on the host of the same program
(tests/cpp/ground_units.hip): ground_levels and ground_pick for every H in 1 .. 64 with the deciding bit at every position of the
current and of the carried word, and on random words; ground_frac over the edges of the value domain; the small helpers.

Every line must report `mismatches 0` and exactly the number of cases derived here."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ground_rules_match_their_plain_restatement(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "ground_units"
    subprocess.check_call([B.hipcc(), *B.flags(), f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "cpp", "ground_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {ln.split()[0]: ln for ln in out.stdout.splitlines() if "mismatches" in ln}
    cases = 64 * 64 * 65
    small = 8 * 8 + 14 ** 3 + 14 * 14 + 4 * 5 * 5 + 4
    for name, n in (("ground_levels", cases), ("ground_small", small)):
        assert lines[name].rstrip().endswith("mismatches 0") and int(lines[name].split("checked")[1].split()[0]) == n, out.stdout
    # per H and level bit: the full headroom and H cases with one voxel of it missing; only the first is a level
    planted = sum(64 * (1 + H) for H in range(1, 65))
    m = re.search(r"^ground_levels cases\s+planted: (\d+)\s+planted levels: (\d+)\s+random with a level: (\d+)$", out.stdout, re.M)
    assert m and int(m.group(1)) == planted and int(m.group(2)) == 64 * 64 and int(m.group(3)) > 1000, out.stdout
