"""The CPU reference of the restart (tests/restart_reference.py) and the inputs of the GPU restart tests
(tests/restart_cases.py): what the projection guarantees, and that every case the GPU tests use really does start
closer than GWH -- a condition on the inputs, checked here so that the GPU tests can compare iteration counts with the
reference instead of carrying numbers written down by hand."""
import numpy as np
import pytest

from oracle import scf_oracle as so
from tests import restart_cases as rc
from tests import restart_reference as rr
from tests.helpers import fragment_bohr, oracle_mol


def _metric(kind, basis):
    frag = {"water": rc.water, "dimer": rc.dimer}[kind]()
    mol = oracle_mol(basis, frag)
    S, _, _ = so.int1e(mol)
    return mol, S, so.build_orthogonalizer(S), frag


def test_projection_returns_an_idempotent_density():
    mol, S, X, frag = _metric("water", "cc-pvdz")
    D = rc.reference_scf("water", "cc-pvdz").D
    assert np.max(np.abs(rr.project_density(S, X, D, 5) - D)) < 1e-12
    # the orbitals come with their occupations: minus 2 five times, then zeros
    _, occ = rr.project_orbitals(S, X, D)
    assert np.max(np.abs(occ[:5] + 2.0)) < 1e-12 and np.max(np.abs(occ[5:])) < 1e-12


def test_projection_of_two_monomers_is_an_scf_state_of_the_dimer():
    mol, S, X, frag = _metric("dimer", "6-31g")
    D0 = rc.case_start("dimer-631g")
    n_el = int(frag.nelec)
    assert abs(np.sum(D0 * S) - n_el) > 1e-6 or np.max(np.abs(D0 @ S @ D0 - 2.0 * D0)) > 1e-6     # the input is NOT one
    D = rr.project_density(S, X, D0, n_el // 2)
    assert np.max(np.abs(D @ S @ D - 2.0 * D)) < 1e-10
    assert abs(np.sum(D * S) - n_el) < 1e-10


def test_projection_of_poor_densities_is_still_an_scf_state():
    mol, S, X, frag = _metric("water", "cc-pvdz")
    D = rc.reference_scf("water", "cc-pvdz").D
    assert np.max(np.abs(rr.project_density(S, X, 0.5 * D, 5) - D)) < 1e-12       # the trace does not matter
    Z = rr.project_density(S, X, np.zeros_like(D), 5)
    assert np.max(np.abs(Z @ S @ Z - 2.0 * Z)) < 1e-10 and abs(np.sum(Z * S) - 10.0) < 1e-10


def test_restart_from_the_converged_density_takes_two_iterations():
    mol, S, X, frag = _metric("water", "cc-pvdz")
    ref = rc.reference_scf("water", "cc-pvdz")
    r = rr.run_rhf_restart(mol, 10, ref.D, max_iter=100, e_tol=rc.E_TOL, d_tol=rc.D_TOL)
    assert r.converged and r.iterations == 2
    assert abs(r.energy - ref.energy) < 1e-10


def test_unrestricted_restart_from_the_converged_spin_densities_takes_two_iterations():
    frag = fragment_bohr([8, 1], [[0.0, 0.0, 0.0], [0.0, 0.0, 1.8324]], multiplicity=2)
    mol = oracle_mol("6-31g", frag)
    ref = so.run_uhf(mol, 9, 2, 100, rc.E_TOL, rc.D_TOL)
    assert ref.converged
    r = rr.run_uhf_restart(mol, 9, 2, ref.Da, ref.Db, 100, rc.E_TOL, rc.D_TOL)
    assert r.converged and r.iterations == 2
    assert abs(r.energy - ref.energy) < 1e-10


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_every_gpu_case_starts_closer_than_gwh(name):
    restarted, plain = rc.reference_restart(name)
    print("%s: reference iterations %d restarted, %d from GWH; |dE| = %.2e" % (name, restarted.iterations, plain.iterations,
                                                                            abs(restarted.energy - plain.energy)))
    assert plain.converged and restarted.converged
    assert restarted.iterations < plain.iterations
    assert abs(restarted.energy - plain.energy) < 1e-9
