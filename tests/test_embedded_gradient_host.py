"""The host assembler of fmo.run_eembe_fixed_charges, no GPU: an analytic toy energy with known derivatives on the
fragment's atoms and on the charges' sites stands in for the engine, and the assembled gradient must be the exact total
derivative of the assembled energy; a two-rank gloo split must equal one rank."""
import itertools
import os
import subprocess
import sys

import numpy as np

from metalquicha_amd import fmo
from metalquicha_amd.methods import ScfSettings
from tests.helpers import w3_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHARGES = np.array([-0.8, 0.4, 0.4, -0.7, 0.3, 0.4, -0.9, 0.5, 0.4])
K_IN, K_FIELD = 0.2, 0.05


def _toy_job_energy(z, xyz, atoms, out, q):
    """e_total of the toy: a pair term inside the fragment and an 'electronic' coupling to every charge (works on
    complex coordinates: squared distances only)."""
    e = 0.0
    for a, b in itertools.combinations(atoms, 2):
        e = e + 0.1 * z[a] * z[b] * np.exp(-K_IN * np.sum((xyz[a] - xyz[b]) ** 2))
    for a in atoms:
        for g, qg in zip(out, q):
            e = e + qg * z[a] * np.exp(-K_FIELD * np.sum((xyz[a] - xyz[g]) ** 2))
    return e


def toy_solver(system):
    """fmo.GradientSolver with hand-written derivatives of _toy_job_energy."""
    z = np.asarray(system.element_numbers, dtype=float)
    xyz = np.ascontiguousarray(system.coordinates.T)

    def solve(jobs, want_gradient):
        res = []
        for job in jobs:
            atoms = [int(a) for a in job.atoms]; out = [int(g) for g in job.field_atoms]
            ga = np.zeros((len(atoms), 3)); gs = np.zeros((len(out), 3))
            for (i, a), (j, b) in itertools.combinations(enumerate(atoms), 2):
                d = xyz[a] - xyz[b]
                v = -2.0 * K_IN * d * 0.1 * z[a] * z[b] * np.exp(-K_IN * (d @ d))
                ga[i] += v; ga[j] -= v
            for i, a in enumerate(atoms):
                for s, g in enumerate(out):
                    d = xyz[a] - xyz[g]
                    v = -2.0 * K_FIELD * d * job.field_charges[s] * z[a] * np.exp(-K_FIELD * (d @ d))
                    ga[i] += v; gs[s] -= v
            e = float(_toy_job_energy(z, xyz, atoms, out, job.field_charges))
            res.append(fmo.EmbeddedGradient(e, ga if want_gradient else None, gs if want_gradient else None, 1))
        return res
    return solve


def _total_energy(system, xyz, charges):
    """E = sum E'_I + sum (E'_IJ - E'_I - E'_J) written out on its own, for real or complex coordinates (n_atoms, 3)."""
    z = np.asarray(system.element_numbers, dtype=float)
    frags = [[int(a) for a in m] for m in system.monomers]
    n = len(z)

    def embedded(atoms):
        out = [g for g in range(n) if g not in atoms]
        e = _toy_job_energy(z, xyz, atoms, out, charges[out])
        for a in atoms:
            for g in out:
                e = e + z[a] * charges[g] / np.sqrt(np.sum((xyz[a] - xyz[g]) ** 2))
        return e
    mono = [embedded(f) for f in frags]
    e = sum(mono)
    for i, j in itertools.combinations(range(len(frags)), 2):
        e = e + embedded(frags[i] + frags[j]) - mono[i] - mono[j]
    return e


def test_assembled_gradient_is_the_total_derivative_of_the_assembled_energy():
    system = w3_system()
    run = fmo.run_eembe_fixed_charges(system, ScfSettings(), CHARGES, solver=toy_solver(system))
    assert not run.errors and run.gradient.shape == (3, 9)
    xyz = np.ascontiguousarray(system.coordinates.T)
    assert abs(run.energy - float(_total_energy(system, xyz, CHARGES))) < 1e-12
    # complex-step derivative of the closed form: exact to rounding
    exact = np.zeros((9, 3))
    for a in range(9):
        for c in range(3):
            x = xyz.astype(complex); x[a, c] += 1e-30j
            exact[a, c] = _total_energy(system, x, CHARGES).imag / 1e-30
    assert np.max(np.abs(run.gradient.T - exact)) < 1e-12, np.max(np.abs(run.gradient.T - exact))
    assert np.max(np.abs(run.gradient.sum(axis=1))) < 1e-12
    assert set(run.pair_corrections) == {(0, 1), (0, 2), (1, 2)}
    assert abs(run.energy - (run.monomer_energy.sum() + sum(run.pair_corrections.values()))) < 1e-12
    energy_only = fmo.run_eembe_fixed_charges(system, ScfSettings(), CHARGES, want_gradient=False, solver=toy_solver(system))
    assert energy_only.gradient is None and energy_only.energy == run.energy


def test_a_failed_job_gives_no_total():
    system = w3_system()
    inner = toy_solver(system)

    def solver(jobs, want_gradient):
        res = inner(jobs, want_gradient)
        if len(jobs[0].atoms) == 6:
            res[1].error = "made to fail"
        return res
    run = fmo.run_eembe_fixed_charges(system, ScfSettings(), CHARGES, solver=solver)
    assert np.isnan(run.energy) and run.gradient is None and "made to fail" in run.errors[0]


def test_two_rank_gloo_split_equals_one_rank(tmp_path):
    """world_size = 2 over gloo: monomers and dimers round-robin over the ranks, one all-reduce at the end."""
    script = tmp_path / "rank.py"
    script.write_text(
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np, torch, torch.distributed as dist\n"
        "from metalquicha_amd import fmo\n"
        "from metalquicha_amd.methods import ScfSettings\n"
        "from tests.helpers import w3_system\n"
        "from tests.test_embedded_gradient_host import CHARGES, toy_solver\n"
        "dist.init_process_group('gloo', init_method='env://')\n"
        "r, w = dist.get_rank(), dist.get_world_size()\n"
        "def allreduce(a):\n"
        "    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy()); dist.all_reduce(t); return t.numpy()\n"
        "system = w3_system(); solver = toy_solver(system)\n"
        "par = fmo.run_eembe_fixed_charges(system, ScfSettings(), CHARGES, rank=r, world=w, allreduce=allreduce, solver=solver)\n"
        "ser = fmo.run_eembe_fixed_charges(system, ScfSettings(), CHARGES, solver=solver)\n"
        "assert not par.errors and abs(par.energy - ser.energy) < 1e-12, (par.energy, ser.energy)\n"
        "assert np.max(np.abs(par.gradient - ser.gradient)) < 1e-12\n"
        "assert np.max(np.abs(par.monomer_energy - ser.monomer_energy)) < 1e-12 and par.scf_iterations == ser.scf_iterations\n"
        "print('rank', r, 'ok')\n"
        "dist.destroy_process_group()\n" % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29541", str(script)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok") == 2
