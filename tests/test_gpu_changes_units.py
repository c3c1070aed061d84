"""The rule of ws_store_changes (ws_changes.h) run on the GPU itself and held to a plain restatement on the host of the same program
(tests/cpp/changes_units.hip): changes_verdict and changes_word over ev and nv in {-32768, -band, -band + 1, 0, band - 1, band,
free - 1, free, 32767}, ew and nw in {-5, 0, min_weight - 1, min_weight, 32767}, valid / not valid, and three parameter sets.

The line must report `mismatches 0` and exactly the number of cases derived here; the kinds are counted from the rule."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [(64, 600, 1), (1, 1, 1), (32767, 32767, 32767)]


def expected_kinds():
    """(unknown, new, same, appeared, vanished) over the grid, from the sentences of the header"""
    out = [0] * 5
    for band, free, mw in SETS:
        values = [-32768, -band, -band + 1, 0, band - 1, band, free - 1, free, 32767]
        weights = [-5, 0, mw - 1, mw, 32767]
        for ev in values:
            for nv in values:
                for ew in weights:
                    for nw in weights:
                        for valid in (False, True):
                            cur, ref = ew >= mw, valid and nw >= mw
                            app = abs(ev) < band and nv >= free
                            van = ev >= free and abs(nv) < band
                            out[0 if not cur else 1 if not ref else 4 if van else 3 if app else 2] += 1
    return out


def test_changes_rule_matches_its_plain_restatement(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "changes_units"
    subprocess.check_call([B.hipcc(), *B.flags(), f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "cpp", "changes_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "mismatches" in ln]
    cases = len(SETS) * 9 * 9 * 5 * 5 * 2
    assert len(lines) == 1 and lines[0].rstrip().endswith("mismatches 0") and int(lines[0].split("checked")[1].split()[0]) == cases, out.stdout
    kinds = re.findall(r"^changes_verdict kinds\s+unknown: (\d+)\s+new: (\d+)\s+same: (\d+)\s+appeared: (\d+)\s+vanished: (\d+)$", out.stdout, re.M)
    want = expected_kinds()
    assert len(kinds) == 1 and [int(v) for v in kinds[0]] == want and sum(want) == cases and min(want) > 0, (kinds, want)
