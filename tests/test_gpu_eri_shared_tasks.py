"""GPU tests of the integral stage's treatment of shared blocks (launch_eri, kern_eri.hip): the task launches of the
shared entries on their one stream with the copy of the shared blocks behind them, next to the dense launches.

Entry under test: stages.coulomb_batch(cc.SPD, frags, D) in full mode (mqc_hip_coulomb_batch: launch_eri with the share
plan, then the in-core J/K over the batch); fragments of 40 functions.

  1. representative counts around a wave: atoms H and C are bit-identical across the batch in r distinct geometries,
     r in {1, 2, 63, 64, 65}; atom N repeats with another count r2, so one class launch holds sets of different
     representative counts.  A set is shared when 6 r <= nfrag: nfrag = max(16, 6 r) rounded up to a multiple of r.
  2. a batch where nothing is shared (20 jittered fragments): the share plan is off, every fragment against the oracle.
  3. both operators: a range-separated SCF batch (CAM-B3LYP, STO-3G, 18 water dimers whose first water repeats in two
     geometries) against the same call without block sharing.

The one-stream placement is the default from 1024 fragments on; MQC_HIP_ERI_TASK_STREAM_MIN=0 switches it on for every
batch with a share plan.  That switch and MQC_HIP_NO_BLOCK_SHARING are read once per process, so the runs that need them
are child processes (the pattern of test_routes_match_the_references).

References: for 1, J of EVERY fragment -- with the one-stream placement (child) and with the placement this process
takes by default -- against J from a child under MQC_HIP_NO_BLOCK_SHARING=1, and a sample of 8 fragments per case of
the one-stream run against the oracle through check_batch.  The integrals of the runs are the same numbers; only the
summation order of the J/K kernels differs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import integral_class_cases as cc
from tests import stages
from tests.helpers import fragment_bohr
from tests.test_gpu_integral_classes import TOL, batch_densities, check_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# r -> r2: distinct geometries of the (H, C) group and of N
REPEATS = {1: 2, 2: 1, 63: 2, 64: 3, 65: 2}

# What two runs of the build BEFORE the one-stream placement (sharing on in both, one process each) differ by on these
# inputs, max |dJ| over all fragments, measured on one MI355X: r = 1 and 2 (16 fragments) 0; r = 63, 64, 65 (378, 384, 390
# fragments, jk_tri_kernel's LDS atomics) 2.22e-16 each, with max |J| = 2.8.  Two unshared runs of that build: 0, 0, 2.22e-16,
# 2.22e-16, 1.11e-16; its shared against its unshared run: 2.22e-16 in all five.
PARENT_RUN_TO_RUN = 2.220446049250313e-16
# bound of the shared / unshared comparison: four times that (8.9e-16; check_batch's TOL * sum |D| is at least 2e-11)
UNSHARED_BOUND = 4.0 * PARENT_RUN_TO_RUN
TASK_STREAM = {"MQC_HIP_ERI_TASK_STREAM_MIN": "0"}


def batch_size(r: int) -> int:
    m = max(16, 6 * r)
    return (m + r - 1) // r * r


def repeat_batch(r: int):
    """cc.sharing_batch's construction with two groups: one rigid frame (cc.jitter_xyz(100)); fragment f takes H and C
    from geometry f % r of the first group and N from geometry f % r2 of the second, copied bit for bit; O moves in
    every fragment.  All displacements are at most 0.05 Bohr per coordinate."""
    r2 = REPEATS[r]
    base = cc.jitter_xyz(100)
    hc = [base[:2] + np.random.default_rng(7300 + g).uniform(-0.05, 0.05, size=(2, 3)) for g in range(r)]
    nn = [base[2] + np.random.default_rng(7400 + g).uniform(-0.05, 0.05, size=3) for g in range(r2)]
    frags = []
    for f in range(batch_size(r)):
        xyz = base.copy()
        xyz[:2] = hc[f % r]
        xyz[2] = nn[f % r2]
        xyz[3] += np.random.default_rng(7500 + f).uniform(-0.05, 0.05, size=3)
        frags.append(fragment_bohr(cc.ELEMENTS, xyz))
    return frags


def oracle_sample(r: int):
    """8 fragments: fragment 0 (a representative of every set), the last representative of each group, a
    non-representative of each group, the last fragment (a non-representative of every shared set), the rest drawn
    from a fixed seed."""
    m, r2 = batch_size(r), REPEATS[r]
    which = {0, r - 1, r, r2 - 1, r2, m - 1}
    rng = np.random.default_rng(8800 + r)
    while len(which) < 8:
        which.add(int(rng.integers(m)))
    return sorted(which)


_UNSHARED_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import integral_class_cases as cc, stages
from tests.test_gpu_eri_shared_tasks import repeat_batch
from tests.test_gpu_integral_classes import batch_densities
frags = repeat_batch(int(sys.argv[3]))
np.save(sys.argv[2], stages.coulomb_batch(cc.SPD, frags, batch_densities(40, len(frags))))
"""


def coulomb_in_child(r, out, env_extra):
    # a child forms at most 390 tensors of 40 functions and one J/K pass: seconds; the limit leaves room for a cold start
    subprocess.run([sys.executable, "-c", _UNSHARED_CHILD, ROOT, out, str(r)], env={**os.environ, **env_extra}, check=True, timeout=180)
    return np.load(out)


@pytest.fixture(autouse=True)
def probe_dir(tmp_path, monkeypatch):
    cc.write_basis_files(tmp_path)
    monkeypatch.setenv("MQC_BASIS_PATH", str(tmp_path))
    return tmp_path


@pytest.mark.parametrize("r", sorted(REPEATS))
def test_representative_counts_around_a_wave(r, probe_dir):
    """16 .. 390 fragments; the (H, C) sets have r representatives, the N set REPEATS[r].  Every fragment's J, from
    the one-stream placement (child) and from this process's default placement, is compared with the run without block
    sharing (child); bound: four times what two runs of the parent differ by on these inputs (PARENT_RUN_TO_RUN,
    measured 2.22e-16).  8 fragments (oracle_sample) of the one-stream run are compared with the oracle through
    check_batch; the other fragments are compared with the unshared run only."""
    frags = repeat_batch(r)
    m = len(frags)
    assert m == batch_size(r) and m % r == 0 and 6 * r <= m
    D = batch_densities(40, m)
    assert UNSHARED_BOUND < TOL * np.min(np.sum(np.abs(D), axis=(1, 2)))
    Ju = coulomb_in_child(r, str(probe_dir / "unshared.npy"), {"MQC_HIP_NO_BLOCK_SHARING": "1"})
    Jt = coulomb_in_child(r, str(probe_dir / "task_stream.npy"), TASK_STREAM)
    Jd = stages.coulomb_batch(cc.SPD, frags, D)
    for J, what in ((Jt, "one task stream"), (Jd, "default placement")):
        assert J.shape == (m, 40, 40) and not np.any(np.isnan(J)), what
        per_fragment = np.max(np.abs(J - Ju), axis=(1, 2))
        assert per_fragment.shape == (m,)                  # no fragment left uncompared
        worst = int(np.argmax(per_fragment))
        print("r = %d, %d fragments, %s against unshared: worst |dJ| %.3e (fragment %d), bound %.3e" % (r, m, what, per_fragment[worst], worst, UNSHARED_BOUND))
        assert per_fragment[worst] <= UNSHARED_BOUND, (what, r, worst, per_fragment[worst])
    check_batch(cc.SPD, frags, Jt, oracle_sample(r), "shared tasks r = %d" % r)


def test_nothing_shared():
    """20 fragments of cc.jitter(k): no atom repeats, the share plan is off and the stage takes the route it took before
    the task stream existed.  Every fragment against the oracle."""
    frags = [cc.jitter(k) for k in range(20)]
    J = stages.coulomb_batch(cc.SPD, frags, batch_densities(40, 20))
    check_batch(cc.SPD, frags, J, range(20), "coulomb_batch, nothing shared")


_RSH_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_eri_shared_tasks import run_rsh_batch
np.save(sys.argv[2], run_rsh_batch())
"""


def rsh_dimers():
    """18 water dimers: the first water is bit-identical in two geometries (even / odd fragments), the second differs
    in every fragment."""
    from tests.helpers import water_at
    rng = np.random.default_rng(311)
    first = [water_at(rng, [0.0, 0.0, 0.0]) for _ in range(2)]
    return [fragment_bohr([8, 1, 1, 8, 1, 1], np.vstack([first[i % 2], water_at(rng, [5.2 + 0.05 * i, 0.4, -0.3])])) for i in range(18)]


def run_rsh_batch():
    from metalquicha_amd import methods
    st = methods.ScfSettings(basis_set="sto-3g", functional="cam-b3lyp", energy_tol=1e-10, density_tol=1e-8, guess="gwh", schwarz_tol=1e-12)
    res = methods.run_hip_scf_batch(st, rsh_dimers())
    assert not any(q.has_error for q in res), [q.error_message for q in res if q.has_error]
    return np.array([[q.energy.scf, q.scf_iterations] for q in res])


def test_both_operators_in_a_range_separated_batch(tmp_path):
    """CAM-B3LYP builds the Coulomb tensor and the erf-attenuated one with two launch_eri calls on the same streams: the
    second call's tasks and copy must wait for the first call and work on the second tensor.  The batch in a child with
    the one-stream placement and in a child without block sharing: equal iteration counts, energies to 1e-10 (the
    convergence threshold of both runs; the tensors hold the same numbers, so nothing but summation order separates
    the two)."""
    got = []
    for k, env in enumerate((TASK_STREAM, {"MQC_HIP_NO_BLOCK_SHARING": "1"})):
        out = str(tmp_path / ("rsh_%d.npy" % k))
        # 18 STO-3G dimers, about 15 iterations of a small quadrature: seconds
        subprocess.run([sys.executable, "-c", _RSH_CHILD, ROOT, out], env={**os.environ, **env}, check=True, timeout=180)
        got.append(np.load(out))
    here, other = got
    print("range-separated batch: max |dE| %.3e" % np.max(np.abs(here[:, 0] - other[:, 0])))
    assert np.array_equal(here[:, 1], other[:, 1])
    assert np.max(np.abs(here[:, 0] - other[:, 0])) < 1e-10
