"""The two scans of ws_store_pack / ws_store_unpack (ws_pack.h) run on the GPU on their own and held to serial loops on the host of
the same program (tests/cpp/pack_units.hip), which includes the header the library's kernels include:

    pack_brick_offsets: the 512 brick offsets of a class map, for the edge maps listed here and 4096 maps drawn from mix64
    pack_scan: the first payload word of n headers and the three sums, for n around the ends of a wave (64) and of a round (1024),
        the 5780 chunks of the replayed run, and 20 000 chunks of 512 dense bricks, whose offsets pass 2^32 words

Each line must report `mismatches 0` and exactly the number of cases derived here from these lists."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_ENDS = [0, 127, 128, 255, 256, 511]  # two codes per thread: a wave of pack_brick_offsets holds 128 bricks
EDGE_MAPS = (["all default", "all uniform", "all dense"]
             + [f"period 2: {a}, {b}" for a in range(3) for b in range(3) if a != b]
             + [f"period 3, phase {p}" for p in range(3)]
             + [f"one dense brick at {b}" for b in WAVE_ENDS]
             + [f"all dense but a {kind} brick at {b}" for kind in ("default", "uniform") for b in WAVE_ENDS])
RANDOM_MAPS = 4096
SCAN_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 5780]
SCAN_LONG = 20000  # x 512 dense bricks x 512 words = 5 242 880 000 words


def test_the_scans_match_their_serial_restatements(tmp_path):
    from warpsense_amd import build as B
    exe = tmp_path / "pack_units"
    subprocess.check_call([B.hipcc(), *B.flags(), f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "cpp", "pack_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {ln.split()[0]: ln for ln in out.stdout.splitlines() if "mismatches" in ln}
    want = {"pack_brick_offsets": (len(EDGE_MAPS) + RANDOM_MAPS) * 512, "pack_scan": sum(SCAN_N) + SCAN_LONG}
    assert sorted(lines) == sorted(want) and len([ln for ln in out.stdout.splitlines() if "mismatches" in ln]) == 2, out.stdout
    for name, cases in want.items():
        assert lines[name].rstrip().endswith("mismatches 0") and int(lines[name].split("checked")[1].split()[0]) == cases, out.stdout
    maps = re.findall(r"^pack_brick_offsets maps\s+edge: (\d+)\s+random: (\d+)$", out.stdout, re.M)
    assert maps == [(str(len(EDGE_MAPS)), str(RANDOM_MAPS))], out.stdout
    long = re.findall(r"^pack_scan long\s+chunks: (\d+)\s+words: (\d+)\s+last hi: (\d+)$", out.stdout, re.M)
    words = SCAN_LONG * 512 * 512
    assert words > 2 ** 32 and (SCAN_LONG - 1) * 512 * 512 >> 32 == 1 and long == [(str(SCAN_LONG), str(words), "1")], out.stdout
