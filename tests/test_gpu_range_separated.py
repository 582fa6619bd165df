"""GPU tests of range-separated wB97X: the erf-attenuated ERI stage (mqc_hip_eri_packed_attenuated) against the numpy
McMurchie-Davidson reference of tests/range_separated_reference.py through every class route a cc-pVDZ or def2-TZVP
fragment takes (register and pass kernels, twin and twin-wave kernels, the LDS general kernel for f shells); the
manifest's two wB97X goldens through methods.run_hip_scf; batches against one fragment per call over the twin-wave,
triangular and chunked routes; the refusals outside the in-core path."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi, methods
from metalquicha_amd.basis import ANGSTROM_TO_BOHR, SYMBOL_TO_Z
from oracle import scf_oracle as so
from tests import range_separated_reference as rr
from tests import stages
from tests.helpers import fragment_bohr, oracle_mol, water_at
from tests.stages import eri_packed_attenuated

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER = ([8, 1, 1], [[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])
OMEGA = rr.WB97X_OMEGA


@pytest.mark.parametrize("basis", ["6-31g", "cc-pvdz"])
def test_attenuated_tensor_matches_reference(basis):
    """omega = 0.3 (wB97X) on water: every element to 1e-11 of the numpy reference; the stage poisons the tensor
    first, so a NaN-free result means every element was written."""
    frag = fragment_bohr(*WATER)
    M = eri_packed_attenuated(basis, frag, OMEGA)
    ref = stages.pack_eri(rr.eri4_erf(oracle_mol(basis, frag), OMEGA))
    assert not np.any(np.isnan(M))
    assert np.max(np.abs(M - ref)) < 1e-11
    assert np.max(np.abs(M - M.T)) == 0.0
    # the Coulomb tensor of the same call sequence is untouched by the operator switch
    full = stages.eri_packed(basis, frag)
    assert np.max(np.abs(full - stages.pack_eri(rr.eri4_erf(oracle_mol(basis, frag), None)))) < 1e-11


def test_attenuated_tensor_at_large_omega_is_the_coulomb_tensor():
    """omega = 1e4 on cc-pVDZ water against the reference at the same omega (the short-range remainder is ~1e-6
    there, so this pins the finite-omega arithmetic), and omega = 1e8 against mqc_hip_eri_packed itself on a
    def2-TZVP water: the f-shell classes go through the LDS general kernel."""
    frag = fragment_bohr(*WATER)
    M = eri_packed_attenuated("cc-pvdz", frag, 1e4)
    ref = stages.pack_eri(rr.eri4_erf(oracle_mol("cc-pvdz", frag), 1e4))
    assert np.max(np.abs(M - ref)) < 1e-11
    Mt = eri_packed_attenuated("def2-tzvp", frag, 1e8)
    full = stages.eri_packed("def2-tzvp", frag)
    assert not np.any(np.isnan(Mt))
    assert np.max(np.abs(Mt - full)) < 1e-10


def test_attenuated_f_shells_match_reference():
    """def2-TZVP OH (an f shell on O) at omega = 0.3: the general kernel's attenuated mode against the reference."""
    frag = fragment_bohr([8, 1], [[0.0, 0.0, 0.0], [0.0, 0.0, 1.83]])
    mol = oracle_mol("def2-tzvp", frag)
    assert int(np.max(mol.sh_l)) == 3
    M = eri_packed_attenuated("def2-tzvp", frag, OMEGA)
    ref = stages.pack_eri(rr.eri4_erf(mol, OMEGA))
    assert not np.any(np.isnan(M))
    assert np.max(np.abs(M - ref)) < 1e-11


_ROUTE_PROBE = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_range_separated import WATER, OMEGA, eri_packed_attenuated
from tests.helpers import fragment_bohr
M = eri_packed_attenuated("cc-pvdz", fragment_bohr(*WATER), OMEGA)
np.save(sys.argv[2], M)
"""


def test_attenuated_routes_agree(tmp_path):
    """The same tensor through the other routes, each in a fresh process (the route switches are read once): the
    twin entries through the lane-per-entry kernel instead of the wave-per-entry one (MQC_HIP_TWIN_WAVE_MAX=0), and
    every pass class through the LDS general kernel (MQC_HIP_ERI_GENERAL=4)."""
    frag = fragment_bohr(*WATER)
    ref = stages.pack_eri(rr.eri4_erf(oracle_mol("cc-pvdz", frag), OMEGA))
    for k, env in enumerate(({"MQC_HIP_TWIN_WAVE_MAX": "0"}, {"MQC_HIP_ERI_GENERAL": "4"})):
        out = str(tmp_path / ("route%d.npy" % k))
        subprocess.run([sys.executable, "-c", _ROUTE_PROBE, ROOT, out], env={**os.environ, **env}, check=True, timeout=300)
        M = np.load(out)
        assert not np.any(np.isnan(M)), env
        assert np.max(np.abs(M - ref)) < 1e-11, env


def test_attenuated_screening_only_drops_small():
    """The Coulomb Schwarz bounds screen the attenuated tensor: on two distant waters the screened and unscreened
    builds differ by less than the threshold, and the screened one skips blocks."""
    rng = np.random.default_rng(3)
    xyz = np.vstack([water_at(rng, [0, 0, 0]), water_at(rng, [12.0, 0, 0])])
    frag = fragment_bohr([8, 1, 1, 8, 1, 1], xyz)
    full = eri_packed_attenuated("sto-3g", frag, OMEGA)
    scr = eri_packed_attenuated("sto-3g", frag, OMEGA, schwarz_tol=1e-9)
    assert np.max(np.abs(full - scr)) < 1e-9
    assert np.count_nonzero(scr) < np.count_nonzero(full)


@pytest.mark.parametrize("omega", [0.0, -1.0, float("inf")])
def test_attenuated_stage_refuses_bad_omega(omega):
    with pytest.raises(capi.HipBackendError) as e:
        eri_packed_attenuated("sto-3g", fragment_bohr(*WATER), omega)
    assert e.value.code == capi.ERR_VALIDATION
    assert "omega" in str(e.value)


# ---- the functional through the SCF ------------------------------------------------------------------------------------
_CASES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "manifest_subset.json")))["cases"]
WB97X_CASES = [c for c in _CASES if c["functional"] == "wb97x"]


@pytest.mark.parametrize("case", WB97X_CASES, ids=[c["name"] for c in WB97X_CASES])
def test_wb97x_goldens(case):
    """RKS H2O and UKS CH3, wB97X/cc-pVDZ, grid 3: the manifest energy to 1e-8 and the CPU reference (the same SCF with
    the numpy functional and K_lr) to 1e-9 with equal iteration counts."""
    z = [SYMBOL_TO_Z[s.lower()] for s in case["symbols"]]
    frag = fragment_bohr(z, np.array(case["xyz_angstrom"]) * ANGSTROM_TO_BOHR, multiplicity=case["multiplicity"])
    st = methods.ScfSettings(basis_set=case["basis"], functional="wB97X", grid_level=case["grid_level"],
                             energy_tol=1e-10, density_tol=1e-8 if not case["unrestricted"] else 1e-7, guess="gwh",
                             max_iter=case["maxiter"])
    r = methods.run_hip_scf(st, frag)
    assert not r.has_error, r.error_message
    assert r.scf_status == methods.SCF_CONVERGED
    assert abs(r.energy.scf - case["expected_energy"]) < 1e-8
    mol = oracle_mol(case["basis"], frag)
    xc = rr.WB97X(mol, case["grid_level"])
    if case["unrestricted"]:
        o = so.run_uhf(mol, int(frag.nelec), case["multiplicity"], case["maxiter"], 1e-10, 1e-7, xc=xc)
    else:
        o = so.run_rhf(mol, int(frag.nelec), case["maxiter"], 1e-10, 1e-8, xc=xc)
    assert abs(r.energy.scf - o.energy) < 1e-9
    assert r.scf_iterations == o.iterations


def _dimers(k, seed=97):
    rng = np.random.default_rng(seed)
    frags = []
    for i in range(k):
        a = water_at(rng, [0.0, 0.0, 0.0])
        b = water_at(rng, [5.2 + 0.05 * i, 0.4, -0.3])
        frags.append(fragment_bohr([8, 1, 1, 8, 1, 1], np.vstack([a, b])))
    return frags


_BATCH_PROBE = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from metalquicha_amd import methods
from tests.test_gpu_range_separated import _dimers, _SETTINGS
r = methods.run_hip_scf_batch(_SETTINGS, _dimers(int(sys.argv[3])))
assert not any(q.has_error for q in r), [q.error_message for q in r if q.has_error]
np.save(sys.argv[2], np.array([[q.energy.scf, q.scf_iterations] for q in r]))
"""
_SETTINGS = methods.ScfSettings(basis_set="cc-pvdz", functional="wb97x", energy_tol=1e-10, density_tol=1e-8, guess="gwh",
                                schwarz_tol=1e-12)


def test_wb97x_batch_equals_one_per_call(tmp_path):
    """64 water dimers (n = 48) in one call take the triangular tensor layout and the lane-per-entry twin kernels; the
    same dimers one per call take the square layout and the wave-per-entry twin kernels; a third run in a fresh
    process with a 0.4 GB HBM budget cuts the batch into chunks on the two alternating slots.  Energies to 1e-10, equal
    iteration counts."""
    frags = _dimers(64)
    batch = methods.run_hip_scf_batch(_SETTINGS, frags)
    assert not any(q.has_error for q in batch), [q.error_message for q in batch if q.has_error]
    for f, q in zip(frags[:6], batch[:6]):
        one = methods.run_hip_scf(_SETTINGS, f)
        assert not one.has_error, one.error_message
        assert abs(one.energy.scf - q.energy.scf) < 1e-10
        assert one.scf_iterations == q.scf_iterations
    out = str(tmp_path / "chunked.npy")
    subprocess.run([sys.executable, "-c", _BATCH_PROBE, ROOT, out, "64"], env={**os.environ, "MQC_HIP_HBM_BUDGET_GB": "0.4"},
                   check=True, timeout=600)
    ch = np.load(out)
    assert np.max(np.abs(ch[:, 0] - np.array([q.energy.scf for q in batch]))) < 1e-10
    assert np.array_equal(ch[:, 1], np.array([q.scf_iterations for q in batch]))


@pytest.mark.parametrize("what", ["direct", "density_fitting", "large", "gradient"])
def test_wb97x_refusals(what):
    """Outside the in-core exact-ERI path the functional is refused with MQC_HIP_ERR_UNSUPPORTED, a message naming
    what is missing, and no energy."""
    frag = fragment_bohr(*WATER)
    kw = dict(basis_set="cc-pvdz", functional="wb97x")
    if what == "direct":
        kw["eri_mode"] = "direct"
    elif what == "density_fitting":
        kw.update(density_fitting=True, aux_basis_set="mqc-even-tempered-jkfit")
    elif what == "large":
        rng = np.random.default_rng(5)
        frag = fragment_bohr([8, 1, 1] * 5, np.vstack([water_at(rng, [5.5 * i, 0.0, 0.0]) for i in range(5)]))   # n = 120
    st = methods.ScfSettings(**kw)
    grad = what == "gradient"
    r = methods.run_hip_scf(st, frag, want_gradient=grad)
    assert r.has_error and not r.has_energy
    assert "range-separated" in r.error_message
    # the status of the C call itself (the Python result reports per-fragment failures as the driver does, generically)
    fb = methods._flat_basis(st.basis_set, frag)
    aux = methods._flat_basis(st.aux_basis_set, frag) if st.density_fitting else None
    m = methods._Marshalled(frag, fb, aux)
    res = capi.ScfResult()
    eps = np.zeros(fb.nao)
    res.orbital_energies = capi.dptr(eps)
    res.orbital_energies_beta = capi.dptr(eps)
    g = np.zeros((frag.n_atoms, 3))
    if grad:
        res.gradient = capi.dptr(g)
    rc = capi.load_library().mqc_hip_scf_run(capi.get_context(), C.byref(m.mol), C.byref(m.bas),
                                             C.byref(m.aux_bas) if aux is not None else None,
                                             C.byref(methods._options(st, grad)), C.byref(res))
    assert rc == capi.ERR_UNSUPPORTED and res.has_error
    assert {"direct": "direct", "density_fitting": "density fitting", "large": "n_ao <= 116",
            "gradient": "gradients"}[what] in r.error_message
