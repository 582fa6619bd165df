"""C-PCM solvation on the GPU against the numpy reference (tests/pcm_reference.py): the stage entry (tesserae, areas,
the three-index tensor A, v, q, E_pcm, V_pcm), SCF energies and iteration counts on every two-electron path, batches with
ragged tessera counts, several topology groups, chunking and ghosts, epsilon = 1 against the plain entry, and every refusal.

Geometries: the water of __graft_entry__.smoke (163 tesserae at 110 points: not a multiple of 64), random dimers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi, methods
from metalquicha_amd.methods import FragmentGroup, PcmSettings, ScfSettings, _Marshalled, _flat_basis
from oracle import scf_oracle as so, xc_oracle
from tests import pcm_reference as pr
from tests import pcm_stage as ps
from tests.helpers import fragment_bohr, oracle_mol, water_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUX = "mqc-even-tempered-jkfit"
WATER = np.array([[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])     # Bohr
OH = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.8324]])
CH3 = np.array([[0.0, 0.0, 0.0], [2.039, 0.0, 0.0], [-1.0195, 1.76583, 0.0], [-1.0195, -1.76583, 0.0]])
EPS = 78.39


def water():
    return fragment_bohr([8, 1, 1], WATER)


def dimers(count, seed=7):
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([water_at(rng, [0.0, 0.0, 0.0]), water_at(rng, [5.0 + 1.5 * rng.random(), rng.normal(), rng.normal()])])
                     for _ in range(count)])


def random_density(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, n))
    return 0.5 * (d + d.T)


# ---- the stage entry --------------------------------------------------------------------------------------------------
_STAGE_CASES = {"water-631g": (water, "6-31g", 110), "water-ccpvdz": (water, "cc-pvdz", 110),
                "oh-tzvp": (lambda: fragment_bohr([8, 1], OH, multiplicity=2), "def2-tzvp", 110)}
# v, q, V_pcm and E_pcm pass through the solve with the cavity matrix: ten times the largest differences seen on the three
# cases (v 5.8e-15, q 2.1e-15, V_pcm 3.1e-15, E_pcm 8.0e-15), far inside the 1e-9 they may not exceed
V_BOUND, Q_BOUND, VPCM_BOUND, E_BOUND = 5.8e-14, 2.1e-14, 3.1e-14, 8.0e-14


@pytest.mark.parametrize("case", sorted(_STAGE_CASES))
def test_stage_against_the_reference(case):
    make, basis, pts = _STAGE_CASES[case]
    frag = make()
    mol = oracle_mol(basis, frag)
    ref = pr.Pcm(mol, list(frag.element_numbers), EPS, pts)
    D = random_density(mol.nao, 3)
    got = ps.pcm_stage(basis, frag, PcmSettings(EPS, pts), D)
    v, q, e, V = ref.response(D)
    assert len(got.areas) == len(ref.areas)
    if case.startswith("water"):
        assert len(got.areas) == 163
    d_t, d_a = np.max(np.abs(got.tesserae - ref.tesserae)), np.max(np.abs(got.areas - ref.areas))
    d_A = np.max(np.abs(got.A - pr.pack_pairs(ref.A)))
    d_v, d_q, d_V, d_e = np.max(np.abs(got.v - v)), np.max(np.abs(got.q - q)), np.max(np.abs(got.V - V)), abs(got.e_pcm - e)
    print("%s: T %d  tesserae %.1e areas %.1e  A %.1e  v %.1e q %.1e V_pcm %.1e E_pcm %.1e  (|q|max %.2f, cond S %.1e)"
          % (case, len(ref.areas), d_t, d_a, d_A, d_v, d_q, d_V, d_e, np.max(np.abs(q)), np.linalg.cond(ref.S)))
    assert d_t < 1e-13 and d_a < 1e-13
    assert not np.any(np.isnan(got.A)) and d_A < 1e-11
    assert np.allclose(got.V, got.V.T, rtol=0, atol=0)
    assert d_v < V_BOUND and d_q < Q_BOUND and d_V < VPCM_BOUND and d_e < E_BOUND


def test_stage_capacities():
    frag = water()
    D = random_density(13, 1)
    rc, T, _ = ps.pcm_stage_raw("6-31g", frag, PcmSettings(EPS, 110), D, 100, 163 * 91)
    assert rc == capi.ERR_VALIDATION and T == 163
    assert "tessera_capacity" in capi.load_library().mqc_hip_last_error().decode()
    rc, T, _ = ps.pcm_stage_raw("6-31g", frag, PcmSettings(EPS, 110), D, 163, 163 * 91 - 1)
    assert rc == capi.ERR_VALIDATION and T == 163
    assert "a_capacity" in capi.load_library().mqc_hip_last_error().decode()


# ---- SCF in the continuum ---------------------------------------------------------------------------------------------
def _settings(basis, **kw):
    return ScfSettings(basis_set=basis, energy_tol=1e-10, density_tol=1e-8, guess="gwh", **kw)


def _reference_scf(frag, basis, pts=110, functional="", aux=None, ghost=None):
    mol = oracle_mol(basis, frag)
    inner = xc_oracle.XCOracle(mol, functional, 3) if functional else None
    p = pr.Pcm(mol, list(frag.element_numbers), EPS, pts, ghost=ghost, inner=inner)
    if frag.multiplicity != 1:
        r = so.run_uhf(mol, int(frag.nelec), int(frag.multiplicity), 100, 1e-10, 1e-8, xc=p)
    else:
        r = so.run_rhf(mol, int(frag.nelec), 100, 1e-10, 1e-8, xc=p, aux=None if aux is None else oracle_mol(aux, frag))
    return r, p


_SCF_CASES = {
    "rhf-631g": (water, dict(basis_set="6-31g"), 110),
    "b3lyp-ccpvdz": (water, dict(basis_set="cc-pvdz", functional="b3lyp"), 110),
    "uhf-ch3": (lambda: fragment_bohr([6, 1, 1, 1], CH3, multiplicity=2), dict(basis_set="cc-pvdz"), 110),
    "df-rhf": (water, dict(basis_set="cc-pvdz", density_fitting=True, aux_basis_set=AUX), 110),
    "direct": (water, dict(basis_set="6-31g", eri_mode="direct"), 110),
    "rhf-194": (water, dict(basis_set="6-31g"), 194),       # two tesserae 0.003 Bohr apart: cond S = 2e5
}


@pytest.mark.parametrize("case", sorted(_SCF_CASES))
def test_scf_against_the_reference(case):
    make, kw, pts = _SCF_CASES[case]
    frag = make()
    st = _settings(kw["basis_set"], **{k: v for k, v in kw.items() if k != "basis_set"})
    r = methods.run_hip_scf_pcm_batch(st, PcmSettings(EPS, pts), [frag])[0]
    assert not r.has_error, r.error_message
    o, p = _reference_scf(frag, kw["basis_set"], pts, kw.get("functional", ""), AUX if kw.get("density_fitting") else None)
    print("%s: E %.10f (ref %.10f, diff %.2e)  E_pcm %.10f (diff %.2e)  iterations %d/%d  T %d"
          % (case, r.energy.scf, o.energy, r.energy.scf - o.energy, r.energy.pcm, r.energy.pcm - p.e_pcm, r.scf_iterations, o.iterations, len(p.areas)))
    assert abs(r.energy.scf - o.energy) < 1e-8
    assert abs(r.energy.pcm - p.e_pcm) < 1e-8
    assert r.scf_iterations == o.iterations
    assert r.energy.pcm < 0.0


def test_e_xc_stays_the_xc_energy():
    frag = water()
    rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(_settings("cc-pvdz", functional="b3lyp"), PcmSettings(EPS, 110),
                                                    [FragmentGroup(frag.element_numbers, WATER[None], np.zeros(1, dtype=np.int32))])
    o, p = _reference_scf(frag, "cc-pvdz", 110, "b3lyp")
    assert nt[0][0] == 163
    assert abs(rec[0]["e_xc"][0] - p.e_xc) < 1e-7 and abs(e_pcm[0][0] - p.e_pcm) < 1e-8


# ---- batches ----------------------------------------------------------------------------------------------------------
def _dimer_group(count, seed=7, ghost=None):
    return FragmentGroup(np.array([8, 1, 1, 8, 1, 1], dtype=np.int32), dimers(count, seed), np.zeros(count, dtype=np.int32), ghost=ghost)


def _monomer_group(count, seed=3):
    rng = np.random.default_rng(seed)
    return FragmentGroup(np.array([8, 1, 1], dtype=np.int32), np.stack([water_at(rng, rng.normal(size=3)) for _ in range(count)]),
                         np.zeros(count, dtype=np.int32))


def _one(g, k):
    return FragmentGroup(g.element_numbers, g.xyz[k:k + 1], g.charge[k:k + 1], ghost=g.ghost)


def _batch_equals_singles(st, pcm, groups):
    rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(st, pcm, groups)
    for g, r, e, t in zip(groups, rec, e_pcm, nt):
        assert not np.any(r["has_error"]), bytes(r["message"][0])
        for k in range(g.xyz.shape[0]):
            r1, e1, t1 = methods.run_hip_scf_pcm_groups(st, pcm, [_one(g, k)])
            assert t1[0][0] == t[k]
            assert abs(r1[0]["e_total"][0] - r["e_total"][k]) < 1e-10 and abs(e1[0][0] - e[k]) < 1e-10
            assert r1[0]["iterations"][0] == r["iterations"][k]
    return rec, e_pcm, nt


def test_six_dimers_with_different_counts():
    g = _dimer_group(6)
    rec, e_pcm, nt = _batch_equals_singles(_settings("sto-3g"), PcmSettings(EPS, 110), [g])
    print("tesserae per dimer:", nt[0])
    assert len(set(int(v) for v in nt[0])) > 1          # ragged: one stride, several counts
    assert np.all(e_pcm[0] < 0.0)
    # one of them against the reference
    frag = fragment_bohr(list(g.element_numbers), g.xyz[2])
    o, p = _reference_scf(frag, "sto-3g")
    assert len(p.areas) == nt[0][2]
    assert abs(rec[0]["e_total"][2] - o.energy) < 1e-8 and abs(e_pcm[0][2] - p.e_pcm) < 1e-8 and rec[0]["iterations"][2] == o.iterations


def test_monomers_and_dimers_in_one_call():
    _batch_equals_singles(_settings("sto-3g"), PcmSettings(EPS, 50), [_monomer_group(3), _dimer_group(2, seed=9)])


_CHUNK_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests import test_gpu_pcm as t
from metalquicha_amd import methods
rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(t._settings("sto-3g"), t.PcmSettings(t.EPS, 50), [t._monomer_group(3), t._dimer_group(5, seed=9)])
np.save(sys.argv[2], np.concatenate([np.concatenate([r["e_total"] for r in rec]), np.concatenate(e_pcm), np.concatenate([r["iterations"] for r in rec])]))
"""


def test_chunked_equals_unchunked(tmp_path):
    """The mixed batch under an HBM budget that holds two dimers with their PCM arrays, in a child process (the budget is
    read when the context is made).  Per STO-3G dimer at stride 192: 31 n^2 doubles of SCF matrices and the tensor 0.1 MB,
    PCM arrays 8 (3 x 192^2 + 2 x 192 x 105) = 1.2 MB; 0.004 GB = 4.3 MB, of which 40 % per lane."""
    out = str(tmp_path / "chunked.npy")
    child = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, ROOT, out], capture_output=True, text=True, timeout=300,
                           env={**os.environ, "MQC_HIP_HBM_BUDGET_GB": "0.004", "MQC_HIP_PCM_TIMING": "1"})
    assert child.returncode == 0, child.stderr[-2000:]
    lines = [ln for ln in child.stderr.splitlines() if ln.startswith("mqc_hip: pcm timing:")]
    assert len(lines) == 2, child.stderr[-2000:]
    assert any(int(ln.split(" chunks")[0].split()[-1]) >= 2 for ln in lines), lines
    got = np.load(out)
    rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(_settings("sto-3g"), PcmSettings(EPS, 50), [_monomer_group(3), _dimer_group(5, seed=9)])
    here = np.concatenate([np.concatenate([r["e_total"] for r in rec]), np.concatenate(e_pcm), np.concatenate([r["iterations"] for r in rec])])
    assert np.all(np.concatenate([r["has_error"] for r in rec]) == 0)
    assert np.max(np.abs(got[:16] - here[:16])) < 1e-10 and np.array_equal(got[16:], here[16:])


def test_dimer_with_a_ghost_monomer():
    ghost = np.array([0, 0, 0, 1, 1, 1], dtype=bool)
    g = _dimer_group(1, seed=21, ghost=ghost)
    rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(_settings("6-31g"), PcmSettings(EPS, 110), [g])
    assert not rec[0]["has_error"][0], bytes(rec[0]["message"][0])
    frag = fragment_bohr(list(g.element_numbers), g.xyz[0], ghost=ghost)
    o, p = _reference_scf(frag, "6-31g", ghost=ghost)
    assert nt[0][0] == len(p.areas) and np.all(p.atom < 3)        # no sphere on a ghost
    assert abs(rec[0]["e_total"][0] - o.energy) < 1e-8 and abs(e_pcm[0][0] - p.e_pcm) < 1e-8 and rec[0]["iterations"][0] == o.iterations


@pytest.mark.parametrize("kw", [dict(basis_set="6-31g"), dict(basis_set="cc-pvdz", functional="pbe"),
                                dict(basis_set="6-31g", unrestricted=True)], ids=["rhf", "pbe", "uhf"])
def test_epsilon_one_is_the_plain_entry(kw):
    st = _settings(kw["basis_set"], **{k: v for k, v in kw.items() if k != "basis_set"})
    groups = [_monomer_group(2), _dimer_group(2, seed=4)]
    plain = methods.run_hip_scf_groups(st, groups)
    rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(st, PcmSettings(1.0, 110), groups)
    for a, b, e in zip(plain, rec, e_pcm):
        assert not np.any(b["has_error"])
        assert np.max(np.abs(a["e_total"] - b["e_total"])) < 1e-12 and np.array_equal(a["iterations"], b["iterations"])
        assert np.all(e == 0.0)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(st, pcm, groups, code, word, want_gradient=False):
    status = []
    rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(st, pcm, groups, want_gradient=want_gradient, status_out=status)
    assert status == [code], status
    for r, e in zip(rec, e_pcm):
        assert np.all(r["has_error"] == 1) and np.all(e == 0.0)
        for msg in r["message"]:
            assert word in bytes(msg).split(b"\0", 1)[0].decode(), bytes(msg)


def test_refusals_of_the_settings():
    g = [_monomer_group(1)]
    st = _settings("sto-3g")
    _refused(st, PcmSettings(EPS, 110), g, capi.ERR_UNSUPPORTED, "gradient", want_gradient=True)
    _refused(st, PcmSettings(0.5, 110), g, capi.ERR_VALIDATION, "epsilon")
    _refused(st, PcmSettings(float("nan"), 110), g, capi.ERR_VALIDATION, "epsilon")
    _refused(st, PcmSettings(float("inf"), 110), g, capi.ERR_VALIDATION, "epsilon")
    _refused(st, PcmSettings(EPS, 100), g, capi.ERR_VALIDATION, "angular_points")
    _refused(st, PcmSettings(EPS, 770), g, capi.ERR_VALIDATION, "angular_points")


def test_refusals_of_embedded_fragments():
    m = _monomer_group(1)
    st = _settings("sto-3g")
    pc = FragmentGroup(m.element_numbers, m.xyz, m.charge, point_charge_xyz=np.array([[[0.0, 0.0, 9.0]]]), point_charges=np.array([[0.3]]))
    _refused(st, PcmSettings(EPS, 110), [pc], capi.ERR_UNSUPPORTED, "point charges")
    hx = FragmentGroup(m.element_numbers, m.xyz, m.charge, h_extra=np.zeros((1, 7, 7)))
    _refused(st, PcmSettings(EPS, 110), [hx], capi.ERR_UNSUPPORTED, "h_extra")


def test_missing_radius_and_override():
    """Boron has no Bondi radius in the table: a molecule whose first atom claims Z = 5 (water's shells stand in for its
    basis) is refused by name until the caller's table supplies a radius."""
    lib = capi.load_library()

    def run(pcm):
        frag = water()                      # a fresh one: the marshalled record points into its element array
        m = _Marshalled(frag, _flat_basis("sto-3g", frag))
        m.z[0] = 5
        m.mol.nelec = 7; m.mol.multiplicity = 2
        keep = []
        popts = pcm.options(keep)
        opts = methods._options(_settings("sto-3g"), False)
        res = capi.ScfResult()
        e, t = C.c_double(1.0), C.c_int32(-1)
        rc = lib.mqc_hip_scf_pcm_batch(capi.get_context(), 1, C.byref(m.mol), C.byref(m.bas), None, C.byref(opts), C.byref(popts),
                                       C.byref(res), C.byref(e), C.byref(t))
        return rc, res, e.value, t.value

    rc, res, e, t = run(PcmSettings(EPS, 110))
    assert rc == capi.ERR_VALIDATION and res.has_error and "Z = 5" in res.message.decode() and e == 0.0
    assert "Z = 5" in lib.mqc_hip_last_error().decode()
    rc, res, e, t = run(PcmSettings(EPS, 110, radii_by_z={5: 3.6}))
    assert t > 0 and "radius" not in res.message.decode()      # past the refusal (the SCF of this odd molecule is not the point)
    # the stage entry refuses the same way
    frag = water()
    m = _Marshalled(frag, _flat_basis("sto-3g", frag))
    m.z[0] = 5
    keep = []
    popts = PcmSettings(EPS, 110).options(keep)
    D = np.zeros((7, 7))
    T = C.c_int32(0)
    rc = lib.mqc_hip_pcm_stage(capi.get_context(), C.byref(m.mol), C.byref(m.bas), C.byref(popts), capi.dptr(D), 0, 0, C.byref(T),
                               None, None, None, None, None, None, None)
    assert rc == capi.ERR_VALIDATION and "Z = 5" in lib.mqc_hip_last_error().decode()
