"""The rules of the clearance (ws_clearance.h) run on the GPU itself and held to a plain restatement on the host of the same program
(tests/cpp/clearance_units.hip): the margin, whose floor square root starts from a float estimate on the device, for every d2 in
0 .. 65025 at the five resolutions and both ends of the radius; the rotated offset and its voxel at the ends of the domains of
rotation, offset, position and resolution, and where the rounding turns; the penalty and the (margin, index) key.

Every line must report `mismatches 0` and exactly the number of cases derived here."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clearance_rules_match_their_plain_restatement(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "clearance_units"
    subprocess.check_call([B.hipcc(), *B.flags(), f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "cpp", "clearance_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {ln.split()[0]: ln for ln in out.stdout.splitlines() if "mismatches" in ln}
    for name, n in (("clear_margin", 5 * 65026 * 2), ("clear_centre", 1 << 19), ("clear_small", 64 * 64)):
        assert lines[name].rstrip().endswith("mismatches 0") and int(lines[name].split("checked")[1].split()[0]) == n, out.stdout
    # d2 res^2 is a perfect square iff d2 is one: 256 values of d2, five resolutions, two radii -- the root itself is the edge of the floor
    m = re.search(r"^clear_margin cases\s+perfect squares: (\d+)$", out.stdout, re.M)
    assert m and int(m.group(1)) == 256 * 5 * 2, out.stdout
    # the cases reach what they are there for: sums exactly at the rounding's turn, negative centres, and a sum near 3 * 2^50
    m = re.search(r"^clear_centre cases\s+exact halves: (\d+)\s+negative centres: (\d+)\s+widest sum: (\d+)$", out.stdout, re.M)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 100000 and int(m.group(3)) > 2 * 2 ** 50, out.stdout
