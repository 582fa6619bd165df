"""Inputs of the restart tests, shared by tests/test_restart_reference.py (CPU) and tests/test_gpu_restart.py: the
displaced-geometry and dimer-from-monomers cases, and their reference runs, computed once per process.

Every case is (fragment the SCF runs on, the density it starts from).  The starting densities are the reference's own
converged densities (of the undisplaced geometry, or of the two monomers), so that the GPU tests compare an engine
restart with a reference restart from the same numbers."""
import functools

import numpy as np

from oracle import scf_oracle as so
from tests import restart_reference as rr
from tests.helpers import fragment_bohr, oracle_mol, water_at

E_TOL, D_TOL = 1e-11, 1e-9
WATER = np.array([[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])   # check_rhf.f90:112-116
MAX_SHIFT = 0.05      # Bohr, per coordinate


def water():
    return fragment_bohr([8, 1, 1], WATER)


def displaced_water():
    rng = np.random.default_rng(20261018)
    return fragment_bohr([8, 1, 1], WATER + rng.uniform(-MAX_SHIFT, MAX_SHIFT, size=WATER.shape))


def dimer_waters():
    rng = np.random.default_rng(5)
    return [water_at(rng, c) for c in ([0.0, 0.0, 0.0], [5.4, 0.3, -0.4])]


def dimer():
    return fragment_bohr([8, 1, 1, 8, 1, 1], np.vstack(dimer_waters()))


def dimer_monomers():
    return [fragment_bohr([8, 1, 1], w) for w in dimer_waters()]


def _xc(mol, functional):
    if not functional:
        return None
    from oracle import xc_oracle
    return xc_oracle.XCOracle(mol, functional, 3)


@functools.lru_cache(maxsize=None)
def reference_scf(kind, basis, functional=""):
    """The reference at tight settings.  kind: "water", "displaced", "dimer", "monomer0", "monomer1" -> ScfResult (GWH)."""
    frag = {"water": water, "displaced": displaced_water, "dimer": dimer,
            "monomer0": lambda: dimer_monomers()[0], "monomer1": lambda: dimer_monomers()[1]}[kind]()
    mol = oracle_mol(basis, frag)
    return so.run_rhf(mol, int(frag.nelec), 100, E_TOL, D_TOL, xc=_xc(mol, functional))


# name -> (kind of the fragment that runs, basis, functional, kinds whose densities make the start)
CASES = {
    "displaced-rhf": ("displaced", "cc-pvdz", "", ("water",)),
    "displaced-b3lyp": ("displaced", "cc-pvdz", "b3lyp", ("water",)),
    "dimer-ccpvdz": ("dimer", "cc-pvdz", "", ("monomer0", "monomer1")),
    "dimer-631g": ("dimer", "6-31g", "", ("monomer0", "monomer1")),
}


def case_fragment(name):
    kind = CASES[name][0]
    return displaced_water() if kind == "displaced" else dimer()


def case_start(name):
    """The density the case starts from: the reference's converged density of the sources, block-diagonal."""
    _, basis, functional, sources = CASES[name]
    return rr.block_diagonal([reference_scf(s, basis, functional).D for s in sources])


@functools.lru_cache(maxsize=None)
def reference_restart(name):
    """-> (restarted ScfResult, GWH-started ScfResult) of the reference on the case's fragment."""
    kind, basis, functional, _ = CASES[name]
    frag = case_fragment(name)
    mol = oracle_mol(basis, frag)
    r = rr.run_rhf_restart(mol, int(frag.nelec), case_start(name), max_iter=100, e_tol=E_TOL, d_tol=D_TOL, xc=_xc(mol, functional))
    return r, reference_scf(kind, basis, functional)
