"""GPU tests of the deferred small groups of a batch call (scf_run_batch_impl, engine.cpp): when one topology group of a
call is large, the other groups wait on the host until its integral stage is done and then run next to its SCF loop.

  1. (H2O)6 MBE-2 RHF/cc-pVDZ (the first six waters of the bench generator at side 2: 6 monomers + 15 dimers, two topology
     groups) in ONE batch call, run three ways: deferral forced on (MQC_HIP_DEFER_SMALL_GROUPS_MIN=1: the dimers are the
     large group, the monomers hold 1/40 of their stored integrals), deferral off (=0), and the groups one after the other
     (MQC_HIP_CONCURRENT_GROUPS=0).  Same iteration counts; per-fragment energies within ENERGY_BOUND.
  2. a call whose largest group is refused by validation (water pentamers, 120 functions, on the in-core exact-ERI path
     that stops at 116: MQC_HIP_ERR_UNSUPPORTED) next to one water monomer, deferral on: the call returns, the monomer has
     its energy, the pentamers carry the refusal.  The refused batch never reaches the point where it would let the waiting
     group go; it must do so on its way out.

The switches are read once per process, so every run is a child process.

ENERGY_BOUND: what two runs (one process each) of the build BEFORE the deferral differ by on input 1, max |dE| over the
21 fragments, measured on one MI355X (profiles/r05_d_deferred_groups_parent_spread.log: 1.137e-13, four ulp; the same
build's concurrent run against its one-group-at-a-time run: 2.842e-13): PARENT_RUN_TO_RUN below; floored at one ulp of the
largest energy (a dimer's, -152 Eh: 2.84e-14), times four.  Each child prints a line per call that defers
(MQC_HIP_DEFER_SMALL_GROUPS_TRACE=1), so a run that was meant to defer and did not fails."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_RUN_TO_RUN = 1.1368683772161603e-13          # measured (four ulp of a dimer's energy); see the module docstring
ENERGY_ULP = float(np.spacing(152.0))
ENERGY_BOUND = 4.0 * max(PARENT_RUN_TO_RUN, ENERGY_ULP)

_CLUSTER_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from metalquicha_amd import mbe
from tests.test_gpu_deferred_groups import bench_settings, six_waters
system = six_waters()
run = mbe.run_mbe(system, bench_settings(), level=2)
assert not run.errors, run.errors
print(json.dumps({"terms": [list(t) for t in run.terms], "e": run.energies.tolist(), "it": run.iterations.tolist()}))
"""

_REFUSAL_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_deferred_groups import run_refused_next_to_valid
print(json.dumps(run_refused_next_to_valid()))
"""


def bench_settings(**kw):
    from metalquicha_amd import methods
    return methods.ScfSettings(basis_set="cc-pvdz", guess="gwh", energy_tol=1e-8, density_tol=1e-6, schwarz_tol=1e-12, **kw)


def six_waters():
    from metalquicha_amd import mbe
    from metalquicha_amd.basis import SYMBOLS
    full = mbe.water_cluster(2)
    sym = [SYMBOLS[int(z)] for z in full.element_numbers[:18]]
    return mbe.system_from_xyz(sym, full.coordinates.T[:18] * mbe.BOHR_TO_ANGSTROM, [[3 * m, 3 * m + 1, 3 * m + 2] for m in range(6)])


def run_refused_next_to_valid():
    """Two water pentamers (refused: in-core exact ERIs stop at 116 functions) and one monomer in one call."""
    from metalquicha_amd import methods
    from tests.helpers import water_at
    rng = np.random.default_rng(512)
    waters = [water_at(rng, [5.8 * k, 0.3 * k, -0.2 * k]) for k in range(5)]
    penta = np.stack([np.vstack(waters), np.vstack(waters) + 0.01])
    groups = [methods.FragmentGroup(np.array([8, 1, 1] * 5, dtype=np.int32), penta, np.zeros(2, dtype=np.int32)),
              methods.FragmentGroup(np.array([8, 1, 1], dtype=np.int32), waters[0][None], np.zeros(1, dtype=np.int32))]
    status = []
    recs = methods.run_hip_scf_groups(bench_settings(eri_mode="incore"), groups, status_out=status)
    text = lambda m: bytes(m).split(b"\0", 1)[0].decode(errors="replace")
    return {"status": status[0],
            "penta_error": [int(x) for x in recs[0]["has_error"]], "penta_message": [text(m) for m in recs[0]["message"]],
            "mono_error": int(recs[1]["has_error"][0]), "mono_energy": float(recs[1]["e_total"][0]),
            "mono_status": int(recs[1]["scf_status"][0])}


def child(script, env_extra, limit):
    """The child's last line of output as JSON, plus how many calls of it said that they deferred their small groups."""
    done = subprocess.run([sys.executable, "-c", script, ROOT], env={**os.environ, "MQC_HIP_DEFER_SMALL_GROUPS_TRACE": "1", **env_extra},
                          check=True, capture_output=True, text=True, timeout=limit)
    got = json.loads(done.stdout.strip().splitlines()[-1])
    got["deferring_calls"] = sum("small groups deferred behind a group of" in line for line in done.stderr.splitlines())
    return got


@pytest.fixture(scope="module")
def three_ways():
    # 21 fragments of at most 48 functions: a second of GPU work per child; the limit leaves room for a cold start
    return {name: child(_CLUSTER_CHILD, env, 60) for name, env in (("deferred", {"MQC_HIP_DEFER_SMALL_GROUPS_MIN": "1"}),
                                                                    ("not deferred", {"MQC_HIP_DEFER_SMALL_GROUPS_MIN": "0"}),
                                                                    ("one group at a time", {"MQC_HIP_CONCURRENT_GROUPS": "0"}))}


@pytest.mark.parametrize("other", ["not deferred", "one group at a time"])
def test_deferred_groups_give_the_same_fragments(three_ways, other):
    """6 monomers + 15 dimers: identical iteration counts, energies within ENERGY_BOUND of the run that defers nothing
    and of the run that takes the groups one after the other."""
    a, b = three_ways["deferred"], three_ways[other]
    assert a["deferring_calls"] == 1 and b["deferring_calls"] == 0          # the one engine call of run_mbe
    assert a["terms"] == b["terms"] and sorted(len(t) for t in a["terms"]) == [1] * 6 + [2] * 15
    ea, eb = np.array(a["e"]), np.array(b["e"])
    assert np.all(np.isfinite(ea)) and np.all(ea < -75.0)
    diff = np.abs(ea - eb)
    worst = int(np.argmax(diff))
    print("deferred against %s: worst |dE| %.3e (term %s), bound %.3e" % (other, diff[worst], a["terms"][worst], ENERGY_BOUND))
    assert a["it"] == b["it"]
    assert diff[worst] <= ENERGY_BOUND, (other, a["terms"][worst], diff[worst])


def test_refused_large_group_lets_the_small_group_run():
    """The pentamers are refused before anything of theirs is enqueued; the monomer, which waits for them, runs and
    converges.  A refusal is an ordinary return: the child (half a second here) gets ten."""
    from metalquicha_amd import capi
    got = child(_REFUSAL_CHILD, {"MQC_HIP_DEFER_SMALL_GROUPS_MIN": "1"}, 10)
    assert got["deferring_calls"] == 1
    assert got["status"] == capi.ERR_UNSUPPORTED
    assert got["penta_error"] == [1, 1]
    assert all("in-core" in m for m in got["penta_message"]), got["penta_message"]
    assert got["mono_error"] == 0 and got["mono_status"] == capi.SCF_CONVERGED
    assert -76.1 < got["mono_energy"] < -75.9          # RHF/cc-pVDZ water: -76.027
