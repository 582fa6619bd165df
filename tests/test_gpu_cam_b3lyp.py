"""GPU tests of range-separated CAM-B3LYP: the manifest's golden through methods.run_hip_scf and against the CPU reference
of tests/cam_b3lyp_reference.py, restricted and unrestricted; the erf-attenuated ERI stage at CAM-B3LYP's omega; the
quadrature routes that have a range-separated instantiation; batches against one fragment per call over the twin-wave,
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
from tests import cam_b3lyp_reference as cr
from tests import range_separated_reference as rr
from tests import stages
from tests.helpers import fragment_bohr, oracle_mol, water_at
from tests.test_gpu_range_separated import eri_packed_attenuated

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER = ([8, 1, 1], [[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])
_CASES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "manifest_subset.json")))["cases"]
CAM_CASE = [c for c in _CASES if c["functional"] == "cam-b3lyp"][0]
# the manifest has no CAM-B3LYP UKS row: CH3 at the geometry of its UKS rows, against the CPU reference only
CH3_CASE = [c for c in _CASES if c["functional"] == "wb97x" and c["unrestricted"]][0]


def _frag(case):
    z = [SYMBOL_TO_Z[s.lower()] for s in case["symbols"]]
    return fragment_bohr(z, np.array(case["xyz_angstrom"]) * ANGSTROM_TO_BOHR, multiplicity=case["multiplicity"])


def _run(case, functional, frag):
    unrestricted = case["multiplicity"] != 1
    st = methods.ScfSettings(basis_set=case["basis"], functional=functional, grid_level=case["grid_level"],
                             energy_tol=1e-10, density_tol=1e-7 if unrestricted else 1e-8, guess="gwh",
                             max_iter=case["maxiter"])
    r = methods.run_hip_scf(st, frag)
    assert not r.has_error, r.error_message
    assert r.scf_status == methods.SCF_CONVERGED
    mol = oracle_mol(case["basis"], frag)
    xc = cr.CAMB3LYP(mol, case["grid_level"])
    if unrestricted:
        o = so.run_uhf(mol, int(frag.nelec), case["multiplicity"], case["maxiter"], 1e-10, 1e-7, xc=xc)
    else:
        o = so.run_rhf(mol, int(frag.nelec), case["maxiter"], 1e-10, 1e-8, xc=xc)
    assert o.converged
    return r, o


def test_cam_b3lyp_golden():
    """RKS H2O, CAM-B3LYP/cc-pVDZ, grid 3: the manifest energy to 1e-8 and the CPU reference (the same SCF with the numpy
    functional and K_lr at omega = 0.33) to 1e-9 with equal iteration counts.  The name goes in mixed case: matching
    is case-insensitive."""
    frag = _frag(CAM_CASE)
    r, o = _run(CAM_CASE, "CAM-B3LYP", frag)
    assert abs(r.energy.scf - CAM_CASE["expected_energy"]) < 1e-8
    assert abs(r.energy.scf - o.energy) < 1e-9
    assert r.scf_iterations == o.iterations
    # the alias
    ra = methods.run_hip_scf(methods.ScfSettings(basis_set="cc-pvdz", functional="camb3lyp", energy_tol=1e-10,
                                                 density_tol=1e-8, guess="gwh"), frag)
    assert not ra.has_error, ra.error_message
    assert abs(ra.energy.scf - r.energy.scf) < 1e-10


def test_cam_b3lyp_uks_ch3():
    """UKS CH3 (doublet), cc-pVDZ: the polarised ITYH, VWN5 and LYP and K_lr per spin against the CPU reference's
    run_uhf to 1e-9 with equal iteration counts."""
    frag = _frag(CH3_CASE)
    r, o = _run(CH3_CASE, "cam-b3lyp", frag)
    assert abs(r.energy.scf - o.energy) < 1e-9
    assert r.scf_iterations == o.iterations


def test_attenuated_tensor_at_cam_omega():
    """omega = 0.33 on cc-pVDZ water: every element of the packed erf tensor to 1e-11 of the numpy reference."""
    frag = fragment_bohr(*WATER)
    M = eri_packed_attenuated("cc-pvdz", frag, cr.CAM_OMEGA)
    ref = stages.pack_eri(rr.eri4_erf(oracle_mol("cc-pvdz", frag), cr.CAM_OMEGA))
    assert not np.any(np.isnan(M))
    assert np.max(np.abs(M - ref)) < 1e-11


_XC_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from metalquicha_amd import methods
from tests.helpers import fragment_bohr, water_at
rng = np.random.default_rng(4)
ws = [water_at(rng, c) for c in ([0, 0, 0], [5.5, 0.2, -0.3], [0.3, 5.6, 0.4])]
frags = [fragment_bohr([8, 1, 1], ws[0]), fragment_bohr([8, 1, 1, 8, 1, 1], np.vstack(ws[:2])), fragment_bohr([8, 1, 1] * 3, np.vstack(ws))]
st = methods.ScfSettings(basis_set="cc-pvdz", functional="cam-b3lyp", energy_tol=1e-10, density_tol=1e-8, guess="gwh")
res = methods.run_hip_scf_batch(st, frags)
print(json.dumps({"e": [r.energy.scf for r in res], "it": [r.scf_iterations for r in res], "err": [r.error_message for r in res if r.has_error]}))
"""


def test_xc_routes_agree():
    """Restricted CAM-B3LYP at n = 24, 48, 72 (cc-pVDZ water, dimer, trimer), each run in a fresh process because the
    switches are read once.  The default for n <= 96 is the split quadrature with the range-separated functional kernel.
    MQC_HIP_XC_SPLIT=0 takes the range-separated 16-point tile kernel, whose one functional wave walks the components.
    MQC_HIP_XC_PIPE=1 with the split off would take the pipelined kernel, which has no range-separated instantiation: its
    dispatch declines omega > 0, and the tile kernel runs.  MQC_HIP_XC_FAST_SLAB=0 only touches the 32-point tile kernels
    with register-resident density fragments, which have no range-separated instantiation either, so it must change
    nothing.  Same iteration counts and energies to 1e-10 on every route; a component counted twice or ITYH dropped would
    move the energy by far more."""
    def run(env_extra):
        env = dict(os.environ, **env_extra)
        out = subprocess.run([sys.executable, "-c", _XC_CHILD, ROOT], env=env, check=True, capture_output=True, text=True,
                             timeout=900).stdout.strip().splitlines()[-1]
        res = json.loads(out)
        assert not res["err"], (env_extra, res["err"])
        return res

    ref = run({})
    for env in ({"MQC_HIP_XC_SPLIT": "0"}, {"MQC_HIP_XC_SPLIT": "0", "MQC_HIP_XC_PIPE": "1"}, {"MQC_HIP_XC_FAST_SLAB": "0"}):
        other = run(env)
        assert other["it"] == ref["it"], env
        assert np.max(np.abs(np.array(other["e"]) - np.array(ref["e"]))) < 1e-10, env


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
from tests.test_gpu_cam_b3lyp import _dimers, _SETTINGS
r = methods.run_hip_scf_batch(_SETTINGS, _dimers(int(sys.argv[3])))
assert not any(q.has_error for q in r), [q.error_message for q in r if q.has_error]
np.save(sys.argv[2], np.array([[q.energy.scf, q.scf_iterations] for q in r]))
"""
_SETTINGS = methods.ScfSettings(basis_set="cc-pvdz", functional="cam-b3lyp", energy_tol=1e-10, density_tol=1e-8, guess="gwh",
                                schwarz_tol=1e-12)


def test_cam_b3lyp_batch_equals_one_per_call(tmp_path):
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
def test_cam_b3lyp_refusals(what):
    """Outside the in-core exact-ERI path CAM-B3LYP is refused like wB97X: MQC_HIP_ERR_UNSUPPORTED from the C call, no
    energy, and a message that says range-separated, names the functional and what is missing."""
    frag = fragment_bohr(*WATER)
    kw = dict(basis_set="cc-pvdz", functional="cam-b3lyp")
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
    assert "range-separated" in r.error_message and "cam-b3lyp" in r.error_message
    assert {"direct": "direct", "density_fitting": "density fitting", "large": "n_ao <= 116",
            "gradient": "gradients"}[what] in r.error_message
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
