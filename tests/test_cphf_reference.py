"""The numpy polarizability reference (tests/cphf_reference.py) held against the oracle: its overlap against
so.int1e's, its CPHF tensor against finite differences of the oracle's SCF in a uniform field; and the host side of
mbe.run_mbe_polarizability on synthetic tensors.  No GPU."""
import functools

import numpy as np
import pytest

from metalquicha_amd import mbe
from metalquicha_amd.methods import ScfSettings
from oracle import scf_oracle as so
from tests import cphf_reference as cr
from tests.helpers import fragment_bohr, oracle_mol, w3_system

WATER = ([8, 1, 1], [[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])
BASES = ["sto-3g", "6-31g", "cc-pvdz"]


@functools.lru_cache(maxsize=None)
def _water(basis):
    mol = oracle_mol(basis, fragment_bohr(*WATER))
    eri = so.eri4(mol)
    alpha, _ = cr.polarizability(mol, 10, 1e-13, 1e-11, eri=eri)
    return mol, eri, alpha


@pytest.mark.parametrize("basis", BASES)
def test_overlap_matches_oracle(basis):
    mol = _water(basis)[0]
    S, R = cr.dipole_integrals(mol)
    assert np.max(np.abs(S - so.int1e(mol)[0])) < 1e-13
    assert np.max(np.abs(R - R.transpose(0, 2, 1))) < 1e-14


@pytest.mark.parametrize("basis", BASES)
def test_alpha_matches_finite_field(basis):
    mol, eri, alpha = _water(basis)
    ff = cr.finite_field(mol, 10, 2e-3, 1e-13, 1e-11, eri=eri)
    print("alpha vs finite field:", np.max(np.abs(alpha - ff)), "asymmetry:", np.max(np.abs(alpha - alpha.T)), np.diag(alpha))
    assert np.max(np.abs(alpha - ff)) < 1e-7
    assert np.max(np.abs(alpha - alpha.T)) < 1e-12


def test_alpha_of_cc_pvdz_water():
    assert np.allclose(np.diag(_water("cc-pvdz")[2]), [3.0280, 7.5289, 5.7294], atol=5e-5)


def test_origin_drops_out():
    """The first-order density is traceless with S, so moving the molecule moves no element of alpha."""
    Z, xyz = WATER
    mol = oracle_mol("6-31g", fragment_bohr(Z, np.asarray(xyz) + [3.0, -2.0, 5.0]))
    assert np.max(np.abs(cr.polarizability(mol, 10, 1e-13, 1e-11)[0] - _water("6-31g")[2])) < 1e-9


# ---- the MBE assembly, host side ------------------------------------------------------------------------------------
def _synthetic_solver(system, one, two, fail=()):
    """alpha of a term = sum of its monomers' tensors + sum of its pairs' tensors; energies likewise from scalars."""
    from metalquicha_amd.methods import _RES_DTYPE

    def solve(groups):
        recs, al, it, dn = [], [], [], []
        for g in groups:
            m = g.xyz.shape[0]
            rec = np.zeros(m, dtype=_RES_DTYPE)
            a = np.zeros((m, 3, 3))
            done = np.ones(m, dtype=np.int32)
            for k in range(m):
                # which monomers: match the first atom of every monomer
                mons = [i for i, atoms in enumerate(system.monomers)
                        if any(np.allclose(g.xyz[k, j], system.coordinates[:, atoms[0]]) for j in range(g.xyz.shape[1]))]
                a[k] = sum(one[i] for i in mons) + sum(two[(i, j)] for i in mons for j in mons if i < j)
                rec["e_total"][k] = float(np.trace(a[k]))
                rec["iterations"][k] = 7
                if tuple(mons) in fail:
                    done[k] = 0; a[k] = 0.0
            recs.append(rec); al.append(a); it.append(np.full(m, 5, dtype=np.int32)); dn.append(done)
        return recs, al, it, dn
    return solve


def _tensors(n, seed=11):
    rng = np.random.default_rng(seed)
    sym = lambda x: x + x.T
    one = [sym(rng.normal(size=(3, 3))) for _ in range(n)]
    two = {(i, j): sym(rng.normal(size=(3, 3))) * 0.1 for i in range(n) for j in range(i + 1, n)}
    return one, two


def test_mbe_polarizability_is_additive():
    system = w3_system()
    one, two = _tensors(3)
    run = mbe.run_mbe_polarizability(system, ScfSettings(), level=2, solver=_synthetic_solver(system, one, two))
    assert not run.errors
    assert np.max(np.abs(run.polarizability - (sum(one) + sum(two.values())))) < 1e-13
    # the coefficients are the energy's: the same assembly, component by component, through compute_mbe
    for c in range(3):
        for d in range(3):
            assert abs(mbe.compute_mbe(run.terms, run.polarizabilities[:, c, d])[0] - run.polarizability[c, d]) < 1e-13
    coef = mbe.compute_mbe_coefficients(run.terms)
    assert abs(float(coef @ run.energies) - mbe.compute_mbe(run.terms, run.energies)[0]) < 1e-12
    assert np.all(run.cphf_iterations == 5) and np.all(run.iterations == 7)
    # level 1: the monomers alone
    run1 = mbe.run_mbe_polarizability(system, ScfSettings(), level=1, solver=_synthetic_solver(system, one, two))
    assert np.max(np.abs(run1.polarizability - sum(one))) < 1e-13


def test_mbe_polarizability_reports_failed_terms_and_splits_over_ranks():
    system = w3_system()
    one, two = _tensors(3, seed=5)
    run = mbe.run_mbe_polarizability(system, ScfSettings(), level=2, solver=_synthetic_solver(system, one, two, fail=((0, 2),)))
    assert len(run.errors) == 1 and "(0, 2)" in run.errors[0]
    assert np.all(run.polarizabilities[run.terms.index((0, 2))] == 0.0)
    parts = [mbe.run_mbe_polarizability(system, ScfSettings(), level=2, rank=r, world=2, solver=_synthetic_solver(system, one, two))
             for r in range(2)]
    assert np.max(np.abs(parts[0].polarizability + parts[1].polarizability - (sum(one) + sum(two.values())))) < 1e-13
