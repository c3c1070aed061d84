"""The device's fixed-point helpers (ws_device.h, ws_march.h) held to plain int64 / double arithmetic over the domains their
exactness arguments state, evaluated on the GPU itself (tests/cpp/device_units.hip): make_fastdiv_dev, div_trunc, div_res,
div_res_b with ring_b / ring_m, trunc15_biased, the three forms of the weight ramp, integrate_entry, the sqrt of l2norm_i /
l2norm_l and div_trunc_i64 -- on random operands, and on the ones its argument is about: numerators within one of a multiple of the
divisor, at 2^53 where it switches between the double and the plain division.  The whole suite scans only reach these through whole
maps.  The helpers of the map queries have a program of their own: tests/cpp/query_units.hip, tests/test_gpu_query_units.py; both
programs share tests/cpp/unit_report.hpp."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_helpers_match_plain_integer_arithmetic(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "device_units"
    # the library's own compiler flags: the helpers must be exact as the kernels are built (correctly rounded sqrt, no contraction)
    subprocess.check_call([B.hipcc(), *B.flags(), os.path.join(ROOT, "tests", "cpp", "device_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)  # (about 3 s on one MI355X)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "mismatches" in ln]
    assert len(lines) == 13 and all(ln.rstrip().endswith("mismatches 0") for ln in lines), out.stdout
