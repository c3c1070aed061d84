"""The integer helpers of the four map queries held to plain int64 / uint64 arithmetic over the domains their exactness comments
state, evaluated on the GPU itself (tests/cpp/query_units.hip): floor_div, isqrt_u64, ray_cell_fill / ray_cell_T / ray_cell_signs,
RayWalk (start, advance, seed, sample, first_at, first_voxel) and ray_crossing of ws_raycast.h; sample_floor_T and sample_class of
ws_sample.h; crossing, mesh_vertex and block_scan_256 of ws_mesh.h; scan_block_totals of ws_device.h on both sides of its one-piece-
per-thread limit.  The whole-query tests reach these only through whole maps, with inputs from the middle of those domains."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_helpers_match_plain_integer_arithmetic(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "query_units"
    # the library's own compiler flags: the helpers must be exact as the kernels are built (correctly rounded sqrt and division, no contraction)
    subprocess.check_call([B.hipcc(), *B.flags(), os.path.join(ROOT, "tests", "cpp", "query_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)  # (about 0.6 s on one MI355X)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "mismatches" in ln]
    assert len(lines) == 11 and all(ln.rstrip().endswith("mismatches 0") for ln in lines), out.stdout
