"""tools/replay_stream.py --rollouts-csv: the path from arc_rollouts through TSDFMapping.score_trajectories to the file, on a short
stream through a small window.  One line per update of the map, the fan's size in every line, and a best trajectory that is one of the
fan, has no hit and carries the speed and yaw rate of its index."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollouts_csv_has_one_scored_fan_per_update(tmp_path):
    out_csv = tmp_path / "rollouts.csv"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay_stream.py"), "--map", "128", "--scans", "4", "--rollouts-csv", str(out_csv)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    doc = json.loads(run.stdout.strip().splitlines()[-1])
    rows = list(csv.DictReader(open(out_csv)))
    speeds, rates = np.linspace(0.25, 1.5, 6), np.linspace(-0.8, 0.8, 17)
    assert len(rows) >= 1 and doc["rollouts_csv"]["lines"] == len(rows) and doc["rollouts_csv"]["trajectories"] == len(speeds) * len(rates)
    for row in rows:
        b = int(row["best"])
        assert int(row["trajectories"]) == len(speeds) * len(rates) and 0 <= int(row["hit_trajectories"]) <= len(speeds) * len(rates) and -1 <= b < len(speeds) * len(rates)
        if b >= 0:
            assert int(row["min_margin_mm"]) >= 0 and int(row["hit_trajectories"]) < len(speeds) * len(rates)
            assert abs(float(row["speed_mps"]) - speeds[b // len(rates)]) < 1e-3 and abs(float(row["yaw_rate_rps"]) - rates[b % len(rates)]) < 1e-3
    assert doc["rollouts_csv"]["with_a_best"] == sum(int(r["best"]) >= 0 for r in rows)
