"""Static dipole polarizabilities on the GPU (mqc_hip_polarizability_batch; kern_cphf.hip) against the numpy CPHF
reference on the oracle (tests/cphf_reference.py): s to f shells, a dimer, an embedded fragment, batches of two topology
groups against one fragment per call, chunking under MQC_HIP_HBM_BUDGET_GB, the single-density route, a solve that runs
out of iterations next to one that does not, the refusals and the MBE assembly.
Bounds: every element of alpha within 1e-6 a.u. of the reference (elements of 1-10 a.u.; a residual of 1e-10 over a gap
of about 0.5 Eh and orbitals converged to 1e-10 put the expected difference near 1e-9, the reference's own finite-field
check sits at 1e-8), |alpha - alpha^T| < 1e-8, 1e-9 between two routes through the engine itself."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi, mbe, methods
from metalquicha_amd.methods import CphfSettings, FragmentGroup, ScfSettings
from oracle import scf_oracle as so
from tests import cphf_reference as cr
from tests import workload_cases as wc
from tests.helpers import fragment_bohr, oracle_mol, w3_system, water_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER = ([8, 1, 1], [[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])
H2_XYZ = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.4]])
CPHF = CphfSettings(tol=1e-10)
BOUND = 1e-6


def settings(basis, **kw):
    return ScfSettings(basis_set=basis, energy_tol=1e-12, density_tol=1e-10, guess="gwh", **kw)


def water(shift=0.0):
    return fragment_bohr(WATER[0], np.asarray(WATER[1]) + shift)


def dimer():
    rng = np.random.default_rng(12)
    return fragment_bohr([8, 1, 1] * 2, np.vstack([water_at(rng, c) for c in ([0, 0, 0], [5.4, 0.4, -0.3])]))


def hydroxide():
    return fragment_bohr([8, 1], [[0.0, 0.0, 0.0], [0.0, 0.0, 1.83]], charge=-1)


@functools.lru_cache(maxsize=None)
def _reference(make, basis):
    frag = make()
    alpha, scf = cr.polarizability(oracle_mol(basis, frag), frag.nelec, 1e-12, 1e-10)
    return alpha, scf.energy


def check(r, alpha0, e0, what):
    assert not r.has_error, r.error_message
    assert r.has_polarizability and r.polarizability.shape == (3, 3), what
    d = float(np.max(np.abs(r.polarizability - alpha0)))
    asym = float(np.max(np.abs(r.polarizability - r.polarizability.T)))
    print("POLARIZABILITY %s: diag %s  max |alpha - reference| %.2e  asymmetry %.2e  d(E) %.2e  cphf iterations %d"
          % (what, np.diag(r.polarizability), d, asym, r.energy.scf - e0, r.cphf_iterations))
    assert d < BOUND, (what, d)
    assert asym < 1e-8, (what, asym)
    assert abs(r.energy.scf - e0) < 1e-8
    assert 1 <= r.cphf_iterations <= 64


CASES = [("water sto-3g", water, "sto-3g"), ("water 6-31g", water, "6-31g"), ("water cc-pvdz", water, "cc-pvdz"),
         ("hydroxide def2-tzvp", hydroxide, "def2-tzvp"), ("dimer cc-pvdz", dimer, "cc-pvdz")]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_reference(case):
    what, make, basis = case
    alpha0, e0 = _reference(make, basis)
    r = methods.run_hip_polarizability_batch(settings(basis), [make()], CPHF)[0]
    check(r, alpha0, e0, what)
    if what == "water cc-pvdz":
        assert np.allclose(np.diag(r.polarizability), [3.0280, 7.5289, 5.7294], atol=5e-5)


def test_embedded_fragment():
    """Water 6-31G in two point charges: the orbitals carry the field; the reference's h_extra is the oracle's operator."""
    frag = water()
    pts = np.array([[0.0, 0.0, 5.0], [3.0, -2.0, -4.0]])
    q = np.array([-0.8, 0.4])
    group = FragmentGroup(frag.element_numbers, frag.coordinates.T[None], np.zeros(1, dtype=np.int32),
                          point_charge_xyz=pts[None], point_charges=q[None])
    rec, alpha, its, done = methods.run_hip_polarizability_groups(settings("6-31g"), [group], CPHF)
    assert rec[0]["has_error"][0] == 0 and done[0][0] == 1
    mol = oracle_mol("6-31g", frag)
    a0, scf = cr.polarizability(mol, frag.nelec, 1e-12, 1e-10, h_extra=so.point_charge_potential(mol, pts, q))
    free = _reference(water, "6-31g")[0]
    d = float(np.max(np.abs(alpha[0][0] - a0)))
    print("POLARIZABILITY embedded water: max |alpha - reference| %.2e; the field moves alpha by %.2e" % (d, np.max(np.abs(a0 - free))))
    assert d < BOUND and np.max(np.abs(alpha[0][0] - alpha[0][0].T)) < 1e-8
    assert np.max(np.abs(a0 - free)) > 1e-4          # the field is felt: the comparison above is not the free molecule's


def _jittered(xyz, m, seed):
    rng = np.random.default_rng(seed)
    return np.stack([xyz + 0.03 * rng.normal(size=xyz.shape) for _ in range(m)])


def _mixed_groups():
    """64 jittered waters and 6 jittered dimers in 6-31G: two topology groups, 70 fragments."""
    return [FragmentGroup(np.array([8, 1, 1], dtype=np.int32), _jittered(np.asarray(WATER[1]), 64, 11), np.zeros(64, dtype=np.int32)),
            FragmentGroup(np.array([8, 1, 1, 8, 1, 1], dtype=np.int32), _jittered(dimer().coordinates.T, 6, 12), np.zeros(6, dtype=np.int32))]


@functools.lru_cache(maxsize=None)
def _mixed_batch():
    rec, alpha, its, done = methods.run_hip_polarizability_groups(settings("6-31g"), _mixed_groups(), CPHF)
    for a in alpha + its + done:
        a.setflags(write=False)
    return rec, alpha, its, done


def _one(group, k):
    return FragmentGroup(group.element_numbers, group.xyz[k:k + 1], group.charge[k:k + 1])


def test_batch_equals_one_per_call():
    groups = _mixed_groups()
    rec, alpha, its, done = _mixed_batch()
    for g, r, a, it, dn in zip(groups, rec, alpha, its, done):
        assert not np.any(r["has_error"]) and np.all(dn == 1)
        worst = 0.0
        for k in range(g.xyz.shape[0]):
            r1, a1, it1, d1 = methods.run_hip_polarizability_groups(settings("6-31g"), [_one(g, k)], CPHF)
            assert d1[0][0] == 1 and it1[0][0] == it[k], (k, it1[0][0], it[k])
            worst = max(worst, float(np.max(np.abs(a1[0][0] - a[k]))))
        print("POLARIZABILITY group of %d: largest |batch - single| = %.2e, iterations %d..%d" % (g.xyz.shape[0], worst, it.min(), it.max()))
        assert worst < 1e-9, worst
    # one fragment of each group against the reference
    for gi, k in ((0, 63), (1, 5)):
        g = groups[gi]
        frag = fragment_bohr(list(g.element_numbers), g.xyz[k])
        a0, _ = cr.polarizability(oracle_mol("6-31g", frag), frag.nelec, 1e-12, 1e-10)
        assert np.max(np.abs(alpha[gi][k] - a0)) < BOUND


_PROBE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests import test_gpu_polarizability as t
from metalquicha_amd import methods
rec, alpha, its, done = methods.run_hip_polarizability_groups(t.settings("6-31g"), t._mixed_groups(), t.CPHF)
assert not any(np.any(r["has_error"]) for r in rec)
np.savez(sys.argv[2], a0=alpha[0], a1=alpha[1], i0=its[0], i1=its[1], d0=done[0], d1=done[1])
"""


def _child(tmp_path, name, env):
    out = str(tmp_path / name)
    child = subprocess.run([sys.executable, "-c", _PROBE, ROOT, out], capture_output=True, text=True, timeout=300, env={**os.environ, **env})
    assert child.returncode == 0, child.stderr[-3000:]
    return np.load(out), child.stderr


def test_chunked_equals_unchunked(tmp_path):
    """The 70 fragments under an HBM budget that forces several chunks, in a child process (the budget is read when the
    context is made); MQC_HIP_CPHF_TIMING prints one line per chunk."""
    got, err = _child(tmp_path, "chunked.npz", {"MQC_HIP_HBM_BUDGET_GB": "0.004", "MQC_HIP_CPHF_TIMING": "1"})
    chunks = [ln for ln in err.splitlines() if ln.startswith("mqc_hip cphf timing:")]
    assert len(chunks) >= 4, err[-2000:]
    rec, alpha, its, done = _mixed_batch()
    assert np.all(got["d0"] == 1) and np.all(got["d1"] == 1)
    worst = max(float(np.max(np.abs(got["a0"] - alpha[0]))), float(np.max(np.abs(got["a1"] - alpha[1]))))
    print("POLARIZABILITY %d chunks: largest |chunked - unchunked| = %.2e" % (len(chunks), worst))
    assert worst < 1e-9, worst
    assert np.array_equal(got["i0"], its[0]) and np.array_equal(got["i1"], its[1])


def test_single_density_route(tmp_path):
    """MQC_HIP_CPHF_MULTI=0 in a child process: three launches of the single-density stream per iteration."""
    got, _ = _child(tmp_path, "single.npz", {"MQC_HIP_CPHF_MULTI": "0"})
    rec, alpha, its, done = _mixed_batch()
    worst = max(float(np.max(np.abs(got["a0"] - alpha[0]))), float(np.max(np.abs(got["a1"] - alpha[1]))))
    print("POLARIZABILITY single-density route: largest |single - multi| = %.2e" % worst)
    assert np.all(got["d0"] == 1) and np.all(got["d1"] == 1)
    assert worst < 1e-9, worst


def test_solve_out_of_iterations_has_no_alpha_and_its_neighbour_does():
    """max_iter = 2: H2 in a minimal basis has one occupied-virtual pair, so the preconditioned conjugate gradients are
    exact after one step; the waters next to it are not."""
    frags = [water(), fragment_bohr([1, 1], H2_XYZ), water(0.01)]
    rs = methods.run_hip_polarizability_batch(settings("sto-3g"), frags, CphfSettings(tol=1e-10, max_iter=2))
    assert rs[1].has_polarizability and not rs[1].has_error and rs[1].cphf_iterations == 1
    h2 = frags[1]
    a0, _ = cr.polarizability(oracle_mol("sto-3g", h2), 2, 1e-12, 1e-10)
    assert np.max(np.abs(rs[1].polarizability - a0)) < BOUND and a0[2, 2] > 1.0
    for k in (0, 2):
        assert rs[k].has_error and "CPHF did not converge in 2 iterations" in rs[k].error_message
        assert not rs[k].has_polarizability and rs[k].polarizability is None


def _refused(st, frag, cphf=CPHF, want_gradient=False):
    group = FragmentGroup(frag.element_numbers, frag.coordinates.T[None], np.array([frag.charge], dtype=np.int32),
                          np.array([frag.multiplicity], dtype=np.int32), None, np.array([frag.nelec], dtype=np.int32))
    status, box = [], {"settings": cphf}
    rec = methods.run_hip_scf_groups(st, [group], want_gradient=want_gradient, status_out=status, cphf=box)[0]
    msg = bytes(rec["message"][0]).split(b"\0", 1)[0].decode()
    assert rec["has_error"][0] == 1 and rec["scf_status"][0] == capi.SCF_NOT_RUN and rec["iterations"][0] == 0, msg
    assert box["alpha_done"][0][0] == 0 and not box["alpha"][0].any() and box["cphf_iterations"][0][0] == 0
    return status[0], msg


def test_refusals_name_what_is_missing():
    w = water()
    code, msg = _refused(ScfSettings(basis_set="sto-3g", density_fitting=True, aux_basis_set=wc.AUX), w)
    assert code == capi.ERR_UNSUPPORTED and "density-fitted CPHF is not built" in msg, msg
    code, msg = _refused(settings("sto-3g", eri_mode="direct"), w)
    assert code == capi.ERR_UNSUPPORTED and "no tensor to stream" in msg, msg
    rng = np.random.default_rng(5)
    five = np.vstack([water_at(rng, [6.0 * k, 0.0, 0.0]) for k in range(5)])
    code, msg = _refused(settings("cc-pvdz"), fragment_bohr([8, 1, 1] * 5, five))          # 120 functions
    assert code == capi.ERR_UNSUPPORTED and "n_ao <= 116" in msg and "no tensor to stream" in msg, msg
    code, msg = _refused(settings("sto-3g", functional="b3lyp"), w)
    assert code == capi.ERR_UNSUPPORTED and "CPKS" in msg and "second derivatives" in msg, msg
    code, msg = _refused(settings("sto-3g", unrestricted=True), w)
    assert code == capi.ERR_UNSUPPORTED and "unrestricted CPHF" in msg, msg
    code, msg = _refused(settings("sto-3g"), fragment_bohr(*WATER, multiplicity=3))
    assert code == capi.ERR_UNSUPPORTED and "unrestricted CPHF" in msg, msg
    code, msg = _refused(settings("sto-3g"), fragment_bohr(*WATER, charge=1, multiplicity=2))
    assert code == capi.ERR_UNSUPPORTED and "unrestricted CPHF" in msg, msg
    code, msg = _refused(settings("sto-3g"), w, want_gradient=True)
    assert code == capi.ERR_UNSUPPORTED and "polarizability derivatives are not built" in msg, msg
    for bad in (CphfSettings(tol=0.0), CphfSettings(tol=-1e-8), CphfSettings(tol=float("nan")), CphfSettings(tol=float("inf"))):
        code, msg = _refused(settings("sto-3g"), w, cphf=bad)
        assert code == capi.ERR_VALIDATION and "tol must be positive and finite" in msg, msg
    code, msg = _refused(settings("sto-3g"), w, cphf=CphfSettings(max_iter=0))
    assert code == capi.ERR_VALIDATION and "max_iter must be at least 1" in msg, msg
    # the plain entry's own refusals keep their text
    code, msg = _refused(settings("sto-3g", max_iter=0), w)
    assert code == capi.ERR_VALIDATION and "max_iter must be positive" in msg, msg


def test_null_outputs_are_a_validation_error():
    st = settings("sto-3g")
    w = water()
    m = methods._Marshalled(w, methods._flat_basis(st.basis_set, w))
    opts = methods._options(st, False)
    copts = CPHF.options()
    res = capi.ScfResult()
    a = np.zeros(9); it = np.zeros(1, dtype=np.int32); dn = np.zeros(1, dtype=np.int32)
    ip = lambda x: x.ctypes.data_as(capi.c_int32_p)
    lib = capi.load_library()
    for x, y, z in ((None, ip(it), ip(dn)), (capi.dptr(a), None, ip(dn)), (capi.dptr(a), ip(it), None)):
        rc = lib.mqc_hip_polarizability_batch(capi.get_context(), 1, C.byref(m.mol), C.byref(m.bas), C.byref(opts), C.byref(copts),
                                              C.byref(res), x, y, z)
        assert rc == capi.ERR_VALIDATION and "must not be NULL" in lib.mqc_hip_last_error().decode()
    rc = lib.mqc_hip_polarizability_batch(capi.get_context(), 1, C.byref(m.mol), C.byref(m.bas), C.byref(opts), None, C.byref(res),
                                          capi.dptr(a), ip(it), ip(dn))
    assert rc == capi.ERR_VALIDATION
    d = capi.CphfOptions()
    lib.mqc_hip_default_cphf_options(C.byref(d))
    assert (d.tol, d.max_iter) == (1e-8, 64) and (CphfSettings().tol, CphfSettings().max_iter) == (1e-8, 64)


def test_mbe_assembly():
    """(H2O)3 / 6-31G at level 2: the tensor assembled by run_mbe_polarizability against the same assembly of reference
    tensors, and the energy alongside it against run_mbe's."""
    system = w3_system()
    st = settings("6-31g")
    run = mbe.run_mbe_polarizability(system, st, level=2, cphf=CPHF)
    assert not run.errors and run.polarizability.shape == (3, 3) and len(run.terms) == 6
    coef = mbe.compute_mbe_coefficients(run.terms)
    ref = np.zeros((3, 3))
    for c, t in zip(coef, run.terms):
        frag = mbe.build_fragment(system, t)
        ref += c * cr.polarizability(oracle_mol("6-31g", frag), frag.nelec, 1e-12, 1e-10)[0]
    d = float(np.max(np.abs(run.polarizability - ref)))
    print("POLARIZABILITY MBE-2 (H2O)3: trace/3 %.6f  max |assembled - reference| %.2e" % (np.trace(ref) / 3.0, d))
    assert d < BOUND
    plain = mbe.run_mbe(system, st, level=2)
    assert np.max(np.abs(plain.energies - run.energies)) < 1e-10
    assert plain.polarizability is None and plain.polarizabilities is None


def test_plain_scf_is_untouched():
    r = methods.run_hip_scf(settings("sto-3g"), water())
    assert not r.has_error and not r.has_polarizability and r.polarizability is None and r.cphf_iterations == 0
    b = methods.run_hip_scf_batch(settings("sto-3g"), [water()])[0]
    assert not b.has_polarizability and abs(b.energy.scf - r.energy.scf) < 1e-11      # K is summed through atomics: the last bits move
