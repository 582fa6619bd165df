"""Analytic gradients of fragments with 141 to 256 basis functions (direct exact-ERI path, Jacobi rotations in global
memory, screened two-electron term) and of unrestricted Kohn-Sham fragments whose second-derivative slab does not fit
the LDS (the wide XC gradient kernel, xc_grad_wide_kernel).

The large fragments are checked against DIRECTIONAL central differences of the engine's own energies (one batch call):
three fixed-seed random unit directions over all 3N coordinates and two single coordinates, g.d against
(E(x + h d) - E(x - h d)) / 2h, at the tolerances of the small-fragment tests (2e-6 Eh/a0 at h = 1e-3 for HF, 5e-6 at
h = 2e-3 for Kohn-Sham), and the gradient must sum to zero over the atoms."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import mbe, methods
from metalquicha_amd.basis import ANGSTROM_TO_BOHR, SYMBOL_TO_Z
from tests.helpers import W1_ANGSTROM, fragment_bohr, random_rotation, water_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings(basis, functional="", **kw):
    return methods.ScfSettings(basis_set=basis, functional=functional, energy_tol=1e-12, density_tol=1e-10, guess="gwh",
                               max_iter=200, **kw)


def _waters(count, seed, spacing=5.6):
    """`count` waters on a cubic lattice of `spacing` Bohr, random orientations: (Z, xyz Bohr)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(count ** (1.0 / 3.0) - 1e-9))
    sites = [np.array([spacing * i, spacing * j, spacing * k]) for i in range(side) for j in range(side) for k in range(side)]
    xs = [water_at(rng, c) for c in sites[:count]]
    return [8, 1, 1] * count, np.vstack(xs)


def _h2o21():
    """(H2O)21 / STO-3G as test_fragments_above_140_functions_run_from_global_memory builds it: n_ao = 147, 63 atoms."""
    rng = np.random.default_rng(7)
    xs = [water_at(rng, np.array([5.6 * i, 5.6 * j, 5.6 * k])) for i in range(3) for j in range(3) for k in range(3)][:21]
    return [8, 1, 1] * 21, np.vstack(xs)


def _check_directional(st, Z, xyz, h, tol, multiplicity=1, n_ao=None, seed=2026):
    frag = fragment_bohr(Z, xyz, multiplicity=multiplicity)
    r = methods.run_hip_scf(st, frag, want_gradient=True)
    assert not r.has_error, r.error_message
    assert r.has_gradient and r.gradient.shape == (3, len(Z))
    if n_ao is not None:
        assert methods._flat_basis(st.basis_set, frag).nao == n_ao
    g = r.gradient.T.reshape(-1)
    x0 = np.asarray(xyz, dtype=float).reshape(-1)
    rng = np.random.default_rng(seed)
    dirs = [d / np.linalg.norm(d) for d in rng.normal(size=(3, x0.size))]
    for k in rng.choice(x0.size, 2, replace=False):
        e = np.zeros(x0.size); e[k] = 1.0
        dirs.append(e)
    frags = [fragment_bohr(Z, (x0 + sgn * h * d).reshape(-1, 3), multiplicity=multiplicity) for d in dirs for sgn in (1.0, -1.0)]
    res = methods.run_hip_scf_batch(st, frags)
    for q in res:
        assert not q.has_error, q.error_message
    e = [q.energy.scf for q in res]
    for i, d in enumerate(dirs):
        fd = (e[2 * i] - e[2 * i + 1]) / (2.0 * h)
        assert abs(float(g @ d) - fd) < tol, (i, float(g @ d), fd)
    assert np.max(np.abs(r.gradient.sum(axis=1))) < 1e-7, r.gradient.sum(axis=1)
    return r


def test_uks_b3lyp_gradient_between_125_and_140_functions():
    """OH + 5 waters / cc-pVDZ, doublet, n_ao = 139: the unrestricted GGA slab (18 numbers per function and point)
    does not fit the LDS, so the wide XC gradient kernel runs."""
    Z, xyz = _waters(6, seed=3)
    Z, xyz = Z[:-1], xyz[:-1]                 # the last water loses a hydrogen: OH radical
    _check_directional(_settings("cc-pvdz", "b3lyp", grid_level=1), Z, xyz, 2e-3, 5e-6, multiplicity=2, n_ao=139)


@pytest.mark.parametrize("functional", ["", "b3lyp"])
def test_water21_sto3g_gradient(functional):
    """n_ao = 147, 63 atoms: RHF and B3LYP (grid level 1) above the former 140-function limit."""
    Z, xyz = _h2o21()
    h, tol = (1e-3, 2e-6) if not functional else (2e-3, 5e-6)
    _check_directional(_settings("sto-3g", functional, grid_level=1), Z, xyz, h, tol, n_ao=147)


def test_water20_hydroxyl_uhf_gradient():
    """(H2O)20 OH / STO-3G, UHF doublet, n_ao = 146."""
    Z, xyz = _h2o21()
    Z, xyz = Z[:-1], xyz[:-1]
    _check_directional(_settings("sto-3g"), Z, xyz, 1e-3, 2e-6, multiplicity=2, n_ao=146)


def test_water6_ccpvdz_pbe0_gradient():
    """(H2O)6 / cc-pVDZ PBE0, n_ao = 144: d shells through the wide XC kernel, a hybrid's exchange on the screened
    two-electron route."""
    Z, xyz = _waters(6, seed=5)
    _check_directional(_settings("cc-pvdz", "pbe0", grid_level=1), Z, xyz, 2e-3, 5e-6, n_ao=144)


def test_water4_def2tzvp_rhf_gradient():
    """(H2O)4 / def2-TZVP RHF, n_ao = 172: f-shell derivative classes on the screened route."""
    Z, xyz = _waters(4, seed=9)
    _check_directional(_settings("def2-tzvp"), Z, xyz, 1e-3, 2e-6, n_ao=172)


# ---- A/B switches in child processes (they are read once per process) ------------------------------------------------
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from metalquicha_amd import methods
from metalquicha_amd.basis import ANGSTROM_TO_BOHR, SYMBOL_TO_Z
from tests.helpers import fragment_bohr
spec = json.loads(sys.argv[2])
out = []
for c in spec:
    st = methods.ScfSettings(basis_set=c["basis"], functional=c["functional"], grid_level=c["grid_level"],
                             energy_tol=1e-12, density_tol=1e-10, guess="gwh", max_iter=200)
    frag = fragment_bohr(c["Z"], np.array(c["xyz_bohr"]), multiplicity=c["multiplicity"])
    r = methods.run_hip_scf(st, frag, want_gradient=True)
    out.append({"err": r.error_message if r.has_error else "", "e": r.energy.scf,
                "g": r.gradient.tolist() if r.has_gradient else None})
print(json.dumps(out))
"""


def _child(spec, env_extra):
    env = dict(os.environ, **env_extra)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(spec)], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout.strip().splitlines()[-1]
    res = json.loads(out)
    for r in res:
        assert not r["err"], r["err"]
    return res


_CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest_subset.json")))["cases"]


def _ks_gradient_rows():
    from oracle import xc_oracle
    return [c for c in _CASES if c.get("expected_gradient") and c["method"] == "dft" and not c["density_fitting"]
            and c["functional"] in xc_oracle.FUNCTIONALS and "*" not in c["basis"] and "mbe_level" not in c]


def test_wide_xc_gradient_kernel_meets_the_goldens():
    """MQC_HIP_XC_GRAD_WIDE=1 takes the wide kernel at every n: the manifest's Kohn-Sham gradient rows (SVWN, PBE,
    B3LYP on H2O; UKS-PBE on CH3) meet their goldens as test_manifest_kohn_sham_gradient_goldens asks, and agree with
    the default kernel's gradients elementwise to 1e-10."""
    rows = _ks_gradient_rows()
    assert len(rows) >= 4
    spec = [{"basis": c["basis"], "functional": c["functional"], "grid_level": c["grid_level"], "multiplicity": c["multiplicity"],
             "Z": [SYMBOL_TO_Z[s.lower()] for s in c["symbols"]],
             "xyz_bohr": (np.array(c["xyz_angstrom"]) * ANGSTROM_TO_BOHR).tolist()} for c in rows]
    base = _child(spec, {})
    wide = _child(spec, {"MQC_HIP_XC_GRAD_WIDE": "1"})
    for c, b, w in zip(rows, base, wide):
        gw, gb = np.array(w["g"]), np.array(b["g"])
        ref = np.array(c["expected_gradient"]).T
        assert abs(w["e"] - c["expected_energy"]) < 1e-9, (c["name"], w["e"])
        assert np.max(np.abs(gw - ref)) < max(c["gradient_tolerance"], 5e-8), (c["name"], np.max(np.abs(gw - ref)))
        assert np.max(np.abs(gw - gb)) < 1e-10, (c["name"], np.max(np.abs(gw - gb)))


def test_two_electron_screening_is_exact_to_its_threshold():
    """(H2O)6 / cc-pVDZ PBE0 (n_ao = 144): the Schwarz-screened two-electron term against the unscreened one
    (MQC_HIP_GRAD_SCREEN=0)."""
    Z, xyz = _waters(6, seed=5)
    spec = [{"basis": "cc-pvdz", "functional": "pbe0", "grid_level": 1, "multiplicity": 1, "Z": Z, "xyz_bohr": xyz.tolist()}]
    on = _child(spec, {})[0]
    off = _child(spec, {"MQC_HIP_GRAD_SCREEN": "0"})[0]
    assert abs(on["e"] - off["e"]) < 1e-12
    assert np.max(np.abs(np.array(on["g"]) - np.array(off["g"]))) < 1e-10


def test_batch_gradients_equal_one_fragment_per_call():
    """Two 147-function fragments of different geometry in one batch call give the gradients of two single calls."""
    Z, xyz = _h2o21()
    rng = np.random.default_rng(17)
    xyz2 = xyz + 0.05 * rng.normal(size=xyz.shape)
    st = _settings("sto-3g")
    grads = []
    group = methods.FragmentGroup(np.array(Z), np.stack([xyz, xyz2]), np.zeros(2, dtype=np.int32))
    rec = methods.run_hip_scf_groups(st, [group], want_gradient=True, gradients_out=grads)[0]
    assert not np.any(rec["has_error"]) and np.all(rec["has_gradient"])
    for k, x in enumerate((xyz, xyz2)):
        r = methods.run_hip_scf(st, fragment_bohr(Z, x), want_gradient=True)
        assert not r.has_error, r.error_message
        assert np.max(np.abs(grads[0][k] - r.gradient.T)) < 1e-10, (k, np.max(np.abs(grads[0][k] - r.gradient.T)))


def test_mbe2_gradient_across_both_routes():
    """run_mbe(level=2, want_gradient=True) on 12 waters as four 3-water fragments, cc-pVDZ: monomers of 72 functions
    (LDS eigen-solver, unscreened two-electron term) and dimers of 144 (global-memory rotations, screened term) in one
    call.  g.d matches the directional difference of the MBE energy along 2 random directions."""
    rng = np.random.default_rng(12)
    mol = np.array(W1_ANGSTROM) - np.mean(W1_ANGSTROM, axis=0)
    sym, xyz = [], []
    for i in range(12):
        c = np.array([3.1 * (i % 3), 3.1 * ((i // 3) % 2), 3.6 * (i // 6)])
        xyz.append(mol @ random_rotation(rng).T + c)
        sym += ["O", "H", "H"]
    xyz = np.vstack(xyz)
    monomers = [list(range(9 * k, 9 * k + 9)) for k in range(4)]
    st = _settings("cc-pvdz")
    run = mbe.run_mbe(mbe.system_from_xyz(sym, xyz, monomers), st, level=2, want_gradient=True)
    assert not run.errors, run.errors
    g = run.gradient.reshape(-1)
    x0 = xyz.reshape(-1) * ANGSTROM_TO_BOHR
    h = 1e-3
    for d in rng.normal(size=(2, x0.size)):
        d /= np.linalg.norm(d)
        e = []
        for sgn in (1.0, -1.0):
            x = ((x0 + sgn * h * d) / ANGSTROM_TO_BOHR).reshape(-1, 3)
            r = mbe.run_mbe(mbe.system_from_xyz(sym, x, monomers), st, level=2)
            assert not r.errors, r.errors
            e.append(mbe.compute_mbe(r.terms, r.energies)[0])
        fd = (e[0] - e[1]) / (2.0 * h)
        assert abs(float(g @ d) - fd) < 2e-6, (float(g @ d), fd)


def test_gradients_above_256_functions_are_refused():
    """n_ao = 257 (36 waters and a carbon atom in STO-3G): still the eigen-solver's refusal."""
    Z, xyz = _waters(36, seed=1)
    Z = Z + [6]
    xyz = np.vstack([xyz, [[-6.0, -6.0, -6.0]]])
    frag = fragment_bohr(Z, xyz)
    assert methods._flat_basis("sto-3g", frag).nao == 257
    r = methods.run_hip_scf(methods.ScfSettings(basis_set="sto-3g"), frag, want_gradient=True)
    assert r.has_error and "eigen-solver (n_ao <= 256)" in r.error_message, r.error_message
