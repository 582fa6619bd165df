"""GPU tests of the integral stage's dispatcher (launch_eri, kern_eri.hip; rule in eri_dispatch.hpp): the dense class
launches handed, heaviest first, to whichever stream of the slot drains first, the task stream (behind the copy of the
shared blocks) and the chain stream included.  Only the stream of a launch changes, so the tensor holds the same numbers.

Entry under test: stages.coulomb_batch(cc.SPD, frags, D), fragments of 40 functions: s, p and d shells give more class
launches than depth x streams, so the dispatcher has to wait for streams at these sizes.

The dispatcher is on by default from 1024 fragments; MQC_HIP_ERI_DISPATCH_MIN=0 switches it on for every spread batch,
a negative value off; MQC_HIP_ERI_DISPATCH_DEPTH sets the launches in flight per stream.  The switches are read once per
process, so every run is a child process under its own time limit (the pattern of tests/test_gpu_eri_shared_tasks.py).
MQC_HIP_ERI_DISPATCH_TRACE=1 makes a dispatching call say so on stderr; the tests read that line.

References: J of EVERY fragment against J from a child with MQC_HIP_NO_BLOCK_SHARING=1 and the dispatcher off, bound
UNSHARED_BOUND of test_gpu_eri_shared_tasks (four times what two runs of the parent differ by on these inputs, 2.22e-16);
then oracle_sample's 8 fragments per case (the nothing-shared batch: all 20) against the oracle through check_batch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import integral_class_cases as cc
from tests.test_gpu_eri_shared_tasks import UNSHARED_BOUND, batch_size, oracle_sample, repeat_batch
from tests.test_gpu_integral_classes import TOL, batch_densities, check_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DISPATCH = {"MQC_HIP_ERI_DISPATCH_MIN": "0", "MQC_HIP_ERI_TASK_STREAM_MIN": "0", "MQC_HIP_ERI_DISPATCH_TRACE": "1"}
REFERENCE = {"MQC_HIP_NO_BLOCK_SHARING": "1", "MQC_HIP_ERI_DISPATCH_MIN": "-1", "MQC_HIP_ERI_DISPATCH_TRACE": "1"}
TRACE = re.compile(r"mqc_hip: eri dispatch: (\d+) of (\d+) dense launches placed over (\d+) streams, depth (\d+), (\d+) waits")

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import integral_class_cases as cc, stages
from tests.test_gpu_eri_dispatch import batch_of
from tests.test_gpu_integral_classes import batch_densities
frags = batch_of(sys.argv[3])
np.save(sys.argv[2], stages.coulomb_batch(cc.SPD, frags, batch_densities(40, len(frags))))
"""


def batch_of(case: str):
    """'repeat:r': repeat_batch(r) of test_gpu_eri_shared_tasks; 'jitter': the 20 fragments of its test_nothing_shared."""
    if case == "jitter":
        return [cc.jitter(k) for k in range(20)]
    return repeat_batch(int(case.split(":")[1]))


def coulomb_in_child(case, out, env_extra):
    # a child forms at most 384 tensors of 40 functions and one J/K pass: seconds; the limit leaves room for a cold start
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out, case], env={**os.environ, **env_extra}, stderr=subprocess.PIPE, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-4000:]
    return np.load(out), [tuple(int(x) for x in m.groups()) for m in TRACE.finditer(r.stderr)]


_reference = {}


def reference(case, tmp_path):
    """J without block sharing and without the dispatcher, once per batch"""
    if case not in _reference:
        J, traces = coulomb_in_child(case, str(tmp_path / "reference.npy"), REFERENCE)
        assert traces == [], "the dispatcher ran in the reference child"
        _reference[case] = J
    return _reference[case]


@pytest.fixture(autouse=True)
def probe_dir(tmp_path, monkeypatch):
    cc.write_basis_files(tmp_path)
    monkeypatch.setenv("MQC_BASIS_PATH", str(tmp_path))
    return tmp_path


@pytest.mark.parametrize("case, depth", [("repeat:2", None), ("repeat:64", None), ("repeat:64", 1), ("jitter", None)])
def test_dispatched_batch_matches_static_unshared(case, depth, probe_dir):
    """16 fragments with shared sets; 384 fragments where one class launch holds sets of different representative counts,
    at the default depth and at depth 1; 20 fragments that share nothing (no task stream, no copy).  Every fragment's J
    from the dispatching child against the child without sharing and without the dispatcher, bound UNSHARED_BOUND; the
    oracle on oracle_sample's 8 fragments, on all 20 of the nothing-shared batch."""
    frags = batch_of(case)
    m = len(frags)
    assert m == (20 if case == "jitter" else batch_size(int(case.split(":")[1])))
    D = batch_densities(40, m)
    assert UNSHARED_BOUND < TOL * np.min(np.sum(np.abs(D), axis=(1, 2)))
    Ju = reference(case, probe_dir)
    env = dict(DISPATCH)
    if depth is not None:
        env["MQC_HIP_ERI_DISPATCH_DEPTH"] = str(depth)
    Jd, traces = coulomb_in_child(case, str(probe_dir / "dispatched.npy"), env)
    print("%s: dispatcher (placed, dense launches, streams, depth, waits): %s" % (case, traces))
    assert len(traces) == 1, "one launch_eri call, one dispatching call expected"
    placed, dense, streams, used_depth, _waits = traces[0]
    assert placed == dense, "dynamic placement ended early: a poll failed"
    assert streams >= 2 and used_depth == (2 if depth is None else depth)
    if streams <= 4:        # the default of four hardware queues: more launches than depth x streams, so the host has to wait
        assert dense > used_depth * streams, "fewer launches than depth x streams: the dispatcher never has to wait"
    assert Jd.shape == Ju.shape == (m, 40, 40) and not np.any(np.isnan(Jd))
    per_fragment = np.max(np.abs(Jd - Ju), axis=(1, 2))
    assert per_fragment.shape == (m,)                  # no fragment left uncompared
    worst = int(np.argmax(per_fragment))
    print("%s, %d fragments, dispatched against static unshared: worst |dJ| %.3e (fragment %d), bound %.3e" % (case, m, per_fragment[worst], worst, UNSHARED_BOUND))
    assert per_fragment[worst] <= UNSHARED_BOUND, (case, worst, per_fragment[worst])
    sample = range(20) if case == "jitter" else oracle_sample(int(case.split(":")[1]))
    check_batch(cc.SPD, frags, Jd, sample, "dispatched %s" % case)


UNSPREAD = {"MQC_HIP_ERI_SPREAD_MAX": "0", "MQC_HIP_ERI_DISPATCH_TRACE": "1"}
ONE_SIDE_STREAM = {**DISPATCH, "MQC_HIP_ERI_STREAMS": "1"}


@pytest.mark.parametrize("name, env", [("unspread", UNSPREAD), ("one_side_stream", ONE_SIDE_STREAM)])
def test_shared_batch_on_the_narrow_paths(name, env, probe_dir):
    """repeat:2 (16 fragments, the smallest batch that gets a share plan) on the two paths no other test takes: shared
    blocks without spread (every dense launch on the caller's stream, task launches round-robin over the side streams,
    the copy after the join), and a single side stream with the task stream and the dispatcher on, where the task
    stream and the chain stream are one and the dispatcher has two streams.  Every fragment's J against the child
    without sharing and without the dispatcher, bound UNSHARED_BOUND; the oracle on oracle_sample's fragments."""
    case = "repeat:2"
    frags = batch_of(case)
    m = len(frags)
    assert m == batch_size(2) == 16
    Ju = reference(case, probe_dir)
    Jn, traces = coulomb_in_child(case, str(probe_dir / (name + ".npy")), env)
    print("%s: dispatcher (placed, dense launches, streams, depth, waits): %s" % (name, traces))
    if name == "unspread":
        assert traces == [], "the dispatcher ran on an unspread batch"
    else:
        assert len(traces) == 1, "one launch_eri call, one dispatching call expected"
        placed, dense, streams, _depth, _waits = traces[0]
        assert placed == dense, "dynamic placement ended early: a poll failed"
        assert streams == 2
    assert Jn.shape == Ju.shape == (m, 40, 40) and not np.any(np.isnan(Jn))
    per_fragment = np.max(np.abs(Jn - Ju), axis=(1, 2))
    assert per_fragment.shape == (m,)                  # no fragment left uncompared
    worst = int(np.argmax(per_fragment))
    print("%s, %d fragments, against static unshared: worst |dJ| %.3e (fragment %d), bound %.3e" % (name, m, per_fragment[worst], worst, UNSHARED_BOUND))
    assert per_fragment[worst] <= UNSHARED_BOUND, (name, worst, per_fragment[worst])
    check_batch(cc.SPD, frags, Jn, oracle_sample(2), "%s %s" % (name, case))


_RSH_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_eri_shared_tasks import run_rsh_batch
np.save(sys.argv[2], run_rsh_batch())
"""


def test_both_operators_with_the_dispatcher(tmp_path):
    """CAM-B3LYP on 18 STO-3G dimers: two launch_eri calls back to back on the same streams, the second call's launches
    behind the first call's by stream order.  With the dispatcher on against the same batch without block sharing and
    without the dispatcher: equal iteration counts, energies to 1e-10 (the convergence threshold of both runs)."""
    got = []
    for k, env in enumerate((DISPATCH, REFERENCE)):
        out = str(tmp_path / ("rsh_%d.npy" % k))
        # 18 STO-3G dimers, about 15 iterations of a small quadrature: seconds
        r = subprocess.run([sys.executable, "-c", _RSH_CHILD, ROOT, out], env={**os.environ, **env}, stderr=subprocess.PIPE, text=True, timeout=180)
        assert r.returncode == 0, r.stderr[-4000:]
        traces = TRACE.findall(r.stderr)
        print("range-separated batch, child %d: %d dispatching calls" % (k, len(traces)))
        assert len(traces) == (2 if k == 0 else 0)
        got.append(np.load(out))
    here, other = got
    print("range-separated batch: max |dE| %.3e" % np.max(np.abs(here[:, 0] - other[:, 0])))
    assert np.array_equal(here[:, 1], other[:, 1])
    assert np.max(np.abs(here[:, 0] - other[:, 0])) < 1e-10
