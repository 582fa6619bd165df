"""The numpy C-PCM reference (tests/pcm_reference.py) against the properties of the model, CPU only: the cavity matrix
is positive definite, the charges obey Gauss's law, V_pcm is the derivative of E_pcm, epsilon = 1 is the vacuum, an
isolated sphere has its whole area, and an SCF in the continuum converges like the one in the vacuum."""
import math

import numpy as np
import pytest

from metalquicha_amd.basis import ANGSTROM_TO_BOHR
from oracle import scf_oracle as so
from tests import pcm_reference as pr
from tests.helpers import fragment_bohr, oracle_mol, synthetic_density, water_at

WATER = np.array([[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])     # Bohr


def dimer_xyz():
    rng = np.random.default_rng(5)
    return np.concatenate([water_at(rng, [0.0, 0.0, 0.0]), water_at(rng, [5.4, 0.3, -0.2])])


@pytest.fixture(scope="module")
def water_pcm():
    frag = fragment_bohr([8, 1, 1], WATER)
    mol = oracle_mol("6-31g", frag)
    return mol, pr.Pcm(mol, [8, 1, 1], 78.39, 110)


def test_isolated_sphere_has_its_whole_area():
    for pts in (50, 110, 302):
        t, a, _ = pr.cavity([10], [[0.3, -0.2, 0.1]], pts)
        rho = 1.2 * 1.54 * ANGSTROM_TO_BOHR
        assert len(a) == pts
        assert abs(a.sum() - 4.0 * math.pi * rho ** 2) < 1e-12 * a.sum()
        assert np.allclose(np.linalg.norm(t - np.array([0.3, -0.2, 0.1]), axis=1), rho, rtol=0, atol=1e-13)


def test_counts_of_the_issue_cases():
    assert len(pr.cavity([8, 1, 1], WATER, 110)[1]) == 163
    assert len(pr.cavity([8, 1, 1], WATER, 110, ghost=[0, 1, 1])[1]) == 110      # ghosts carry no sphere and cut nothing


@pytest.mark.parametrize("numbers,xyz,pts", [([8, 1, 1], WATER, 110), ([8, 1, 1], WATER, 194), ([8, 1, 1], WATER, 50),
                                              ([1, 1], [[0, 0, 0], [0, 0, 1.4]], 110), ([1, 1], [[0, 0, 0], [0, 0, 1.4]], 302),
                                              ([8, 1, 1] * 2, dimer_xyz(), 50)])
def test_cavity_matrix_is_positive_definite(numbers, xyz, pts):
    t, a, _ = pr.cavity(numbers, xyz, pts)
    S = pr.cavity_matrix(t, a)
    assert np.allclose(S, S.T, rtol=0, atol=0)
    assert np.linalg.eigvalsh(S)[0] > 0.0


def test_gauss_law_for_the_nuclei(water_pcm):
    mol, p = water_pcm
    q = -p.f * np.linalg.solve(p.S, p.v_nuc)
    assert abs(q.sum() + p.f * mol.z.sum()) < 0.01 * p.f * mol.z.sum()


def test_potential_is_the_derivative_of_the_energy(water_pcm):
    mol, p = water_pcm
    D = synthetic_density(mol.nao)
    _, _, _, V = p.response(D)
    h = 1e-4
    for (i, j) in [(0, 0), (3, 1), (8, 8), (12, 5)]:
        E = np.zeros_like(D); E[i, j] += 0.5; E[j, i] += 0.5       # a symmetric direction
        num = (p.response(D + h * E)[2] - p.response(D - h * E)[2]) / (2 * h)
        assert abs(num - np.sum(V * E)) < 1e-9      # E_pcm is quadratic in D: central differences are exact to rounding


def test_epsilon_one_is_the_vacuum():
    frag = fragment_bohr([8, 1, 1], WATER)
    mol = oracle_mol("6-31g", frag)
    vac = so.run_rhf(mol, 10, 100, 1e-10, 1e-8)
    p = pr.Pcm(mol, [8, 1, 1], 1.0, 110)
    r = so.run_rhf(mol, 10, 100, 1e-10, 1e-8, xc=p)
    assert r.iterations == vac.iterations and abs(r.energy - vac.energy) < 1e-12 and p.e_pcm == 0.0


def test_water_in_water_converges_like_the_vacuum():
    frag = fragment_bohr([8, 1, 1], WATER)
    mol = oracle_mol("cc-pvdz", frag)
    vac = so.run_rhf(mol, 10, 100, 1e-8, 1e-6)
    p = pr.Pcm(mol, [8, 1, 1], 78.39, 110)
    r = so.run_rhf(mol, 10, 100, 1e-8, 1e-6, xc=p)
    assert r.converged and abs(r.iterations - vac.iterations) <= 1
    assert len(p.areas) == 163
    # recorded when the model was fixed: E_pcm = -0.010399 Eh, the total moves by -0.009391 Eh (the solute pays 0.001 to polarise)
    assert abs(p.e_pcm + 0.010399) < 2e-6 and abs(r.energy - vac.energy + 0.009391) < 2e-6
    assert abs(r.exc - p.e_pcm) < 1e-14       # the oracle's "E_xc" slot carries E_pcm here
