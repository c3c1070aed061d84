"""The Gauss-Newton update on synthetic sums, on every device route.  tests/gn_cases.py builds a few thousand sequences of sums
backwards from the step each update is to take -- rotations on both sides of gn_step's 0.25 rad branch, at it and a few ulp beside
it, zero and tiny ones, c == 0, singular systems, damping alone, pivoting in one step only, sums beyond 2^53, e and c as the low
words of larger totals, the convergence test at epsilon, max_iterations under the sequence (tests/test_gn_cases_host.py holds the
table to its claims on the CPU) -- and records the state the oracle (wso_gn_begin / wso_gn_update) leaves after every update.

tests/cpp/gn_units.hip includes the library's headers and runs the three forms of the update (gn_update_terms, gn_update,
gn_update_total set up as the resident loop sets it up) on every sequence, comparing T, alpha, prev, iterations and finished with
the oracle's as bit patterns after every update, and holds the reductions below them (wave_reduce32, wave_reduce32_add,
block_reduce32, sum_partials, expand_sums) to plain uint64 sums.  Two routes of the C ABI then take a subset with every class in it:
ws_reg_solve_dev (reg_solve_kernel) and the apply path of ws_reg_iterate_shard_dev (reg_pass_kernel<false>) on an empty shard.
Every comparison is for equality of bits, the sincos branch (theta >= 0.25) included.

Run time on one MI355X, measured: 6.1 s for the module -- 3.8 s the first test (the compile of the unit program and the case table are
most of it; the program itself, twelve launches and the host's sums, runs in under half a second), 0.21 s ws_reg_solve_dev on 280
sequences, 0.04 s the apply path."""
import os
import subprocess

import numpy as np
import pytest

import gn_cases as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# cases per line of the unit program that do not depend on the case file: patterns x groups x 32 slots, with 48 + 2 + units patterns
REDUCTION_CASES = {"wave_reduce32": 562 * 8 * 32, "wave_reduce32_add": 562 * 32, "block_reduce32": 562 * 32, "block_reduce32<1>": 114 * 32,
                   "block_reduce32<2>": 178 * 32, "block_reduce32<4>": 306 * 32, "sum_partials<false>": 306 * 32, "sum_partials<true>": 306 * 32}


def test_every_form_of_the_update_equals_the_oracle_bit_for_bit(tmp_path):
    from warpsense_amd import build as B
    exe, case_file = tmp_path / "gn_units", tmp_path / "gn_cases.bin"
    total = G.write_case_file(str(case_file), G.sequences())
    assert total == sum(len(s.updates) for s in G.sequences()) > 7000
    # the library's own compiler flags: division, sqrt and contraction are those of the kernels
    subprocess.check_call([B.hipcc(), *B.flags(), os.path.join(ROOT, "tests", "cpp", "gn_units.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if "mismatches" in ln]
    assert len(lines) == 12 and all(ln.rstrip().endswith("mismatches 0") for ln in lines), out.stdout
    checked = {ln.split("checked")[0].strip(): int(ln.split("checked")[1].split()[0]) for ln in lines}
    want = dict(REDUCTION_CASES, gn_update_terms=total, gn_update=total, gn_update_total=total, expand_sums=44 * total)
    assert checked == want, (checked, want)


def _expected(u):
    """what ws_reg_poll reports after update u, from the oracle's state: (finished or out of iterations, iterations, pose bits)"""
    return int(u.after[22]), int(u.after[21]), u.after[:16].reshape(4, 4).T


def _run_route(seqs, backend, update):
    """begin -> update per set of sums -> poll, compared with the oracle after every update; returns (updates compared, mismatches)"""
    import torch
    bad, n = [], 0
    for i, s in enumerate(seqs):
        backend.begin(s.pose(), s.max_iterations, float(s.it_weight_gradient), float(s.epsilon))
        for k, u in enumerate(s.updates):
            backend.sums.copy_(torch.from_numpy(u.words))
            update(backend)
            fin, it, T = backend.poll()
            fin_o, it_o, T_o = _expected(u)
            if fin != bool(fin_o or it_o >= s.max_iterations) or it != it_o or not np.array_equal(T.view(np.uint32), T_o):
                bad.append((s.cls, i, k, fin, it, it_o, np.argwhere(T.view(np.uint32) != T_o).tolist()[:4]))
            n += 1
    return n, bad


def _subset():
    seqs = G.subset()
    assert sorted({s.cls for s in seqs}) == sorted(G.CLASSES) and len(seqs) <= 400
    return seqs


def test_reg_solve_kernel_on_the_cases():
    """ws_reg_begin -> ws_reg_solve_dev per update -> ws_reg_poll on a RegistrationCuda without a map"""
    import warpsense_amd as W
    from warpsense_amd.dist import HipGnBackend
    rc = W.RegistrationCuda()
    b = HipGnBackend(rc, None, 50)
    seqs = _subset()
    n, bad = _run_route(seqs, b, lambda b: b.solve(b.sums))
    rc.close()
    assert n == sum(len(s.updates) for s in seqs) and not bad, (len(bad), bad[:8])


def test_reg_pass_kernel_apply_path_on_the_cases():
    """the update at the head of ws_reg_iterate_shard_dev (reg_pass_kernel<false>, apply_previous = 1) on a tiny map with an empty
    shard: the launch applies the sums it is given and accumulates nothing"""
    import warpsense_amd as W
    from warpsense_amd.dist import HipGnBackend
    res, tau = 50, 1000
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=10, size=tuple(16 * res / 1000.0 for _ in range(3))))
    reg = W.TSDFRegistration(params, W.LocalMap(16, 16, 16, tau, 0))
    b = HipGnBackend(reg.reg_, reg.tsdf(), res)

    def update(b):
        b._pending = True  # the sums in place are those of a previous iteration: apply them
        own = b.iterate(0, 0)
        assert own is b.sums

    seqs = _subset()
    n, bad = _run_route(seqs, b, update)
    assert n == sum(len(s.updates) for s in seqs) and not bad, (len(bad), bad[:8])
    # what an empty shard adds: nothing (the launch behind the last update of a live sequence left its own sums, all zero)
    live = next(s for s in seqs if s.cls == "history")
    b.begin(live.pose(), live.max_iterations, float(live.it_weight_gradient), float(live.epsilon))
    import torch
    b.sums.copy_(torch.from_numpy(live.updates[0].words))
    update(b)
    assert not b.sums.cpu().numpy().any()
