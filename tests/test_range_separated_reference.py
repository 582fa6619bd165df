"""CPU tests of the wB97X reference (tests/range_separated_reference.py): the attenuated integrals against the oracle's
Coulomb integrals in the omega -> infinity limit, the attenuation function against mpmath across its series switch,
the functional's derivatives by finite differences, and the whole reference SCF against the manifest's two wB97X
goldens.  No GPU."""
import json
import os

import mpmath
import numpy as np
import pytest

from metalquicha_amd.basis import ANGSTROM_TO_BOHR
from metalquicha_amd.methods import SYMBOL_TO_Z
from oracle import scf_oracle as so
from tests import range_separated_reference as rr
from tests.helpers import W1_ANGSTROM, fragment_bohr, oracle_mol

_CASES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "manifest_subset.json")))["cases"]
WB97X_CASES = [c for c in _CASES if c["functional"] == "wb97x"]


def _water(basis):
    return oracle_mol(basis, fragment_bohr([8, 1, 1], np.array(W1_ANGSTROM) * ANGSTROM_TO_BOHR))


@pytest.mark.parametrize("basis", ["6-31g", "cc-pvdz"])
def test_attenuated_integrals_reach_the_coulomb_limit(basis):
    """erf(w r)/r -> 1/r as w grows: at w = 1e7 the short-range remainder is ~1e-12 of the tightest pair; the plain
    Coulomb form of the same routine equals the oracle's C integrals to rounding."""
    mol = _water(basis)
    ref = so.eri4(mol)
    assert np.abs(rr.eri4_erf(mol, None) - ref).max() < 1e-12
    assert np.abs(rr.eri4_erf(mol, 1e7) - ref).max() < 1e-10


def test_attenuated_integrals_are_bounded_by_the_coulomb_ones():
    """erf(w r)/r is positive definite with a Fourier transform below that of 1/r: (ab|ab)_w <= (ab|ab) for every
    diagonal element, the argument behind reusing the Coulomb Schwarz bounds; the attenuated tensor keeps the 8-fold
    symmetry."""
    mol = _water("cc-pvdz")
    full, att = so.eri4(mol), rr.eri4_erf(mol, 0.3)
    n = mol.nao
    d_full = np.einsum("ijij->ij", full).reshape(-1)
    d_att = np.einsum("ijij->ij", att).reshape(-1)
    assert np.all(d_att >= 0.0) and np.all(d_att <= d_full + 1e-14)
    assert np.abs(att - att.transpose(1, 0, 2, 3)).max() < 1e-14
    assert np.abs(att - att.transpose(2, 3, 0, 1)).max() < 1e-14
    M = att.reshape(n * n, n * n)
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > -1e-12


def test_attenuation_series_meets_the_closed_form():
    """F(a) through the series (a >= 1) and the closed form (a < 1) against 50-digit mpmath on both sides of the
    switch, value and derivative."""
    mpmath.mp.dps = 50

    def exact(a):
        a = mpmath.mpf(a)
        return 1 - mpmath.mpf(8) / 3 * a * (mpmath.sqrt(mpmath.pi) * mpmath.erf(1 / (2 * a))
                                            + (2 * a - 4 * a ** 3) * mpmath.exp(-1 / (4 * a * a)) - 3 * a + 4 * a ** 3)
    a = np.array([0.05, 0.3, 0.7, 0.999, 1.0, 1.001, 1.5, 4.0, 30.0, 1e3])
    F = rr.attenuation_erf(rr.DualN.var(a, 0, 1))
    for i, x in enumerate(a):
        v = float(exact(x))
        dv = float(mpmath.diff(exact, mpmath.mpf(x)))
        assert abs(F.v[i] - v) <= 2e-13 * abs(v) + 1e-17, (x, F.v[i], v)
        assert abs(F.d[0][i] - dv) <= 1e-11 * abs(dv) + 1e-17, (x, F.d[0][i], dv)


def test_wb97x_derivatives_by_finite_differences():
    """v_rho_s and v_sigma_ss' of the polarised form against central differences; the restricted form equals the
    polarised one at equal spins."""
    rng = np.random.default_rng(7)
    x = [rng.uniform(0.02, 2.0, 6), rng.uniform(0.02, 2.0, 6)]
    x += [rng.uniform(0.0, 1.0, 6) * x[0] ** (8 / 3), np.zeros(6), rng.uniform(0.0, 1.0, 6) * x[1] ** (8 / 3)]
    x[3] = 0.5 * np.sqrt(x[2] * x[4])
    f, d = rr.eval_wb97x_pol(*x)
    for k in (0, 1, 2, 4):
        h = 1e-6 * x[k]
        xp = list(x); xm = list(x)
        xp[k] = x[k] + h; xm[k] = x[k] - h
        fd = (rr.eval_wb97x_pol(*xp)[0] - rr.eval_wb97x_pol(*xm)[0]) / (2 * h)
        assert np.allclose(d[k], fd, rtol=1e-5, atol=1e-9), k
    rho, sig = x[0], x[2]
    fr, vr, vs = rr.eval_wb97x(rho, sig)
    fp, dp = rr.eval_wb97x_pol(0.5 * rho, 0.5 * rho, 0.25 * sig, 0.25 * sig, 0.25 * sig)
    assert np.allclose(fr, fp, rtol=1e-15)
    # the restricted derivatives the GPU's restricted path forms from the polarised ones, and by central differences
    assert np.allclose(vr, 0.5 * (dp[0] + dp[1]), rtol=1e-15)
    assert np.allclose(vs, 0.25 * (dp[2] + dp[3] + dp[4]), rtol=1e-15)
    for k, v in ((0, vr), (1, vs)):
        args = [rho, sig]
        h = 1e-6 * args[k]
        ap = list(args); am = list(args)
        ap[k] = args[k] + h; am[k] = args[k] - h
        fd = (rr.eval_wb97x(*ap)[0] - rr.eval_wb97x(*am)[0]) / (2 * h)
        assert np.allclose(v, fd, rtol=1e-5, atol=1e-9), k


@pytest.mark.parametrize("case", WB97X_CASES, ids=[c["name"] for c in WB97X_CASES])
def test_reference_scf_meets_the_wb97x_goldens(case):
    """The reference composes with the oracle's RHF / UHF unchanged and lands on the manifest's energies to 1e-10:
    original PW92 parameters in both correlation terms, F(a) with k_F of the spin density, spin-scaled exchange."""
    z = [SYMBOL_TO_Z[s.lower()] for s in case["symbols"]]
    frag = fragment_bohr(z, np.array(case["xyz_angstrom"]) * ANGSTROM_TO_BOHR, multiplicity=case["multiplicity"])
    mol = oracle_mol(case["basis"], frag)
    xc = rr.WB97X(mol, case["grid_level"])
    if case["unrestricted"]:
        o = so.run_uhf(mol, int(frag.nelec), case["multiplicity"], case["maxiter"], 1e-10, 1e-7, xc=xc)
    else:
        o = so.run_rhf(mol, int(frag.nelec), case["maxiter"], 1e-10, 1e-8, xc=xc)
    assert o.converged
    assert abs(o.energy - case["expected_energy"]) < 1e-10
