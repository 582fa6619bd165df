"""CPU tests of the CAM-B3LYP reference (tests/cam_b3lyp_reference.py): the functional's derivatives by finite
differences on both sides of the attenuation function's series switch, the omega -> 0 and omega -> infinity limits of
ITYH, and the whole reference SCF against the manifest's CAM-B3LYP golden, restricted and through the unrestricted
driver.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

from metalquicha_amd.basis import ANGSTROM_TO_BOHR
from metalquicha_amd.methods import SYMBOL_TO_Z
from oracle import scf_oracle as so
from tests import cam_b3lyp_reference as cr
from tests.helpers import fragment_bohr, oracle_mol

_CASES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "manifest_subset.json")))["cases"]
CAM_CASE = [c for c in _CASES if c["functional"] == "cam-b3lyp"][0]


def _points(seed=11):
    """Spin densities from 1e-7 to 2 (the attenuation argument a_s runs from ~0.1 to ~10), the two spins of a point
    within a factor of two of each other (a central difference in one spin is not drowned by the other's rounding),
    reduced gradients up to x_s ~ 3, and sigma_ab of two non-parallel gradients."""
    rng = np.random.default_rng(seed)
    m = 24
    ra = 10.0 ** rng.uniform(-7.0, 0.3, m)
    rb = ra * rng.uniform(0.5, 2.0, m)
    saa = rng.uniform(0.0, 9.0, m) * ra ** (8 / 3)
    sbb = rng.uniform(0.0, 9.0, m) * rb ** (8 / 3)
    sab = 0.3 * np.sqrt(saa * sbb)
    return [ra, rb, saa, sab, sbb]


def _attenuation_argument(r, s, omega=cr.CAM_OMEGA):
    x = np.sqrt(s) / r ** (4 / 3)
    F = 1.0 + (cr.B88_BETA / cr.C_X) * x * x / (1.0 + 6.0 * cr.B88_BETA * x * np.arcsinh(x))
    return omega * np.sqrt(F) / (2.0 * (6.0 * math.pi ** 2 * r) ** (1 / 3))


@pytest.mark.parametrize("which", ["ityh", "cam-b3lyp"])
def test_derivatives_by_finite_differences(which):
    """v_rho_s, v_sigma_ss and v_sigma_ab of the polarised forms against central differences, at points on both sides
    of the series switch (a_s = 1); the restricted form equals the polarised one at equal spins, and its two
    derivatives match central differences too."""
    ev = cr.eval_ityh_pol if which == "ityh" else cr.eval_cam_b3lyp_pol
    x = _points()
    a = _attenuation_argument(x[0], x[2])
    assert np.any(a < 0.5) and np.any(a > 2.0)
    f, d = ev(*x)
    # a relative step of 1e-4: the sigma terms are small beside the density terms at small reduced gradients, so a
    # shorter step drowns their difference in the value's rounding (the truncation error here is ~1e-8 relative)
    # (sigma_ab may be tiny beside the spins' own scale, rho_a^(4/3) rho_b^(4/3): the step in it is measured in that)
    for k in range(5):
        h = 1e-4 * (x[k] + (x[0] * x[1]) ** (4 / 3) if k == 3 else x[k])
        xp = list(x); xm = list(x)
        xp[k] = x[k] + h; xm[k] = x[k] - h
        fd = (ev(*xp)[0] - ev(*xm)[0]) / (2 * h)
        # a central difference is good to its truncation error and to the value's rounding over the step, ~eps |f| / h
        assert np.all(np.abs(d[k] - fd) <= 2e-6 * np.abs(fd) + 1e-13 * np.abs(f) / h), (k, np.abs(d[k] - fd).max())
    if which == "ityh":
        assert np.all(d[3] == 0.0)
    rest = cr.restricted(ev)
    rho, sig = 2.0 * x[0], 4.0 * x[2]
    fr, vr, vs = rest(rho, sig)
    fp, dp = ev(x[0], x[0], x[2], x[2], x[2])
    assert np.allclose(fr, fp, rtol=1e-15)
    assert np.allclose(vr, 0.5 * (dp[0] + dp[1]), rtol=1e-15)
    assert np.allclose(vs, 0.25 * (dp[2] + dp[3] + dp[4]), rtol=1e-15)
    for k, v in ((0, vr), (1, vs)):
        args = [rho, sig]
        h = 1e-4 * args[k]
        ap = list(args); am = list(args)
        ap[k] = args[k] + h; am[k] = args[k] - h
        fd = (rest(*ap)[0] - rest(*am)[0]) / (2 * h)
        assert np.all(np.abs(v - fd) <= 2e-6 * np.abs(fd) + 1e-13 * np.abs(fr) / h), k


def test_ityh_limits():
    """omega -> 0: F_att -> 1 and ITYH is B88, value and derivatives; omega -> infinity: F_att ~ 1/(36 a^2) and ITYH
    vanishes."""
    x = _points(5)
    fb, db = cr.eval_b88_pol(*x)
    f0, d0 = cr.eval_ityh_pol(*x, omega=1e-12)
    assert np.allclose(f0, fb, rtol=1e-8, atol=0.0)
    for k in (0, 1, 2, 4):
        assert np.allclose(d0[k], db[k], rtol=1e-8, atol=0.0), k
    fi, di = cr.eval_ityh_pol(*x, omega=1e7)
    assert np.all(np.abs(fi) <= 1e-12 * np.abs(fb))
    for k in (0, 1, 2, 4):
        assert np.all(np.abs(di[k]) <= 1e-12 * np.abs(db[k]) + 1e-300), k


@pytest.fixture(scope="module")
def water():
    z = [SYMBOL_TO_Z[s.lower()] for s in CAM_CASE["symbols"]]
    frag = fragment_bohr(z, np.array(CAM_CASE["xyz_angstrom"]) * ANGSTROM_TO_BOHR)
    mol = oracle_mol(CAM_CASE["basis"], frag)
    xc = cr.CAMB3LYP(mol, CAM_CASE["grid_level"])
    rhf = so.run_rhf(mol, int(frag.nelec), CAM_CASE["maxiter"], 1e-10, 1e-8, xc=xc)
    return frag, mol, xc, rhf


def test_reference_scf_meets_the_cam_b3lyp_golden(water):
    """B88 0.35 + ITYH 0.46 + VWN5 0.19 + LYP 0.81, exx 0.19, exx_lr 0.46 at omega 0.33 on the oracle's RHF: the
    manifest energy to 1e-10."""
    _, _, _, o = water
    assert o.converged
    assert abs(o.energy - CAM_CASE["expected_energy"]) < 1e-10


def test_reference_unrestricted_equals_restricted_on_closed_shell(water):
    """The per-spin path (potential_uks: both spin densities through the polarised functional, K_lr per spin) on the
    closed-shell water lands on the restricted energy."""
    frag, mol, xc, rhf = water
    o = so.run_uhf(mol, int(frag.nelec), 1, CAM_CASE["maxiter"], 1e-10, 1e-7, xc=xc)
    assert o.converged
    assert abs(o.energy - rhf.energy) < 1e-9
