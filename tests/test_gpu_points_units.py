"""Device unit tests of the two upper layers of the registration kernels.  tests/points_cases.py builds the case table from fixed
seeds (tests/test_points_cases_host.py holds it to its claims on the CPU); the two programs include the library's headers and are
compiled with the library's own flags.

tests/cpp/points_units.hip (reg_points.h): central_gradient and point_terms against registration.cu:217-250 restated on int64 in
the same thread; the 29 sums of synthetic workgroups on both routes -- consume_point + wave_reduce32_add, and mfma_consume +
mfma_flush + mfma_finalize -- against plain uint64 sums of the host: the same extreme limb in all 64 lanes of a wave, a single
non-zero lane at every lane position for every row of J, alternating extremes, random values, waves of 0, 1, 63, 64 points, 1, 2,
4, 8 waves, every pattern twice in one launch, and the 32 + 8 words read straight after mfma_finalize; gather_point,
gather_point<true> and gather_point_loop on windows A .. E of tests/reg_cases.py over a sequence of poses with the voxel caches
kept, per point against the oracle.

tests/cpp/exchange_units.hip (reg_exchange.h): counted_add, counted_poll, counted_fold, counted_publish<false>, counted_collect
and peer_exchange by one wave that performs every addition itself, on accumulator words preset to zero, all ones, a carry into
the count at the first addition and in mid-exchange, a count byte that wraps, and random; and the bounded poll giving up.

Every line must report `mismatches 0` and exactly the number of cases that Python derives from the table.

Run time on one MI355X, measured: 5.5 s for the module -- 1.9 s the first test and 1.3 s the second (the compile is most of
either; both programs together run in 1.6 s, process start included), the rest is the import and the case table."""
import os
import subprocess

import pytest

import points_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name, want, *args):
    from warpsense_amd import build as B
    exe = tmp_path / name
    # the library's own compiler flags: division and contraction are those of the kernels
    subprocess.check_call([B.hipcc(), *B.flags(), os.path.join(ROOT, "tests", "cpp", name + ".hip"), "-o", str(exe)])
    out = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "mismatches" in ln]
    assert len(lines) == len(want) and all(ln.rstrip().endswith("mismatches 0") for ln in lines), out.stdout
    checked = {ln.split("checked")[0].strip(): int(ln.split("checked")[1].split()[0]) for ln in lines}
    assert checked == want, (checked, want)


def test_point_terms_sums_and_gathers_on_the_device(tmp_path):
    case_file = tmp_path / "points_cases.bin"
    P.write_case_file(str(case_file))
    _run(tmp_path, "points_units", P.expected_counts()[0], str(case_file))


def test_counted_exchange_on_the_device(tmp_path):
    _run(tmp_path, "exchange_units", P.expected_counts()[1])
