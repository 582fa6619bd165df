"""RI-MP2 on the GPU (mqc_hip_rimp2_batch; kern_mp2.hip) against the numpy reference on the oracle
(tests/rimp2_reference.py): small and ragged shapes -- one pair in one mostly padded tile up to 38 virtuals over three
tiles and 252 auxiliary functions --, batches of several topology groups, chunking under MQC_HIP_HBM_BUDGET_GB, the MBE
assembly, the refusals and an embedded fragment.  Bounds: 1e-8 Eh on e_os, e_ss and the SCF energy against the reference
(the project's fragment-energy bound), 1e-12 between two routes through the engine itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi, mbe, methods
from metalquicha_amd.methods import FragmentGroup, ScfSettings
from oracle import scf_oracle as so
from tests import rimp2_reference as ref
from tests import workload_cases as wc
from tests.helpers import fragment_bohr, oracle_mol, w3_system, water_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H2_XYZ = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.4]])
DIMER_XYZ = np.vstack([wc.DF_GRAD_XYZ, wc.DF_GRAD_XYZ @ np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) + np.array([0.4, 0.3, 5.4])])


def settings(basis, **kw):
    return ScfSettings(basis_set=basis, density_fitting=True, aux_basis_set=wc.AUX, energy_tol=1e-12, density_tol=1e-10,
                       guess="gwh", **kw)


def h2():
    return fragment_bohr([1, 1], H2_XYZ)


def water(xyz=wc.DF_GRAD_XYZ):
    return fragment_bohr([8, 1, 1], xyz)


def dimer(xyz=DIMER_XYZ):
    return fragment_bohr([8, 1, 1, 8, 1, 1], xyz)


def check_against_reference(r, frag, basis, frozen_core, what):
    o = ref.rimp2_cached(frag, basis, wc.AUX, frozen_core)
    assert not r.has_error, r.error_message
    assert r.has_mp2, what
    d_scf, d_os, d_ss = r.energy.scf - o["scf"], r.energy.mp2_os - o["e_os"], r.energy.mp2_ss - o["e_ss"]
    print("%s: no %d nv %d naux %d  e_os %.12f e_ss %.12f  d(scf) %.2e d(os) %.2e d(ss) %.2e"
          % (what, o["no"], o["nv"], o["naux"], r.energy.mp2_os, r.energy.mp2_ss, d_scf, d_os, d_ss))
    assert abs(d_scf) < 1e-8, (what, "scf", d_scf)
    assert abs(d_os) < 1e-8, (what, "e_os", d_os)
    assert abs(d_ss) < 1e-8, (what, "e_ss", d_ss)
    assert abs(r.energy.total() - (o["scf"] + o["e_os"] + o["e_ss"])) < 3e-8
    return o


CASES = [("h2 sto-3g", h2, "sto-3g", True, (1, 1, 48)),
         ("water sto-3g all-electron", water, "sto-3g", False, (5, 2, 126)),
         ("water sto-3g frozen", water, "sto-3g", True, (4, 2, 126)),
         ("water 6-31g frozen", water, "6-31g", True, (4, 8, 126)),
         ("water cc-pvdz frozen", water, "cc-pvdz", True, (4, 19, 126)),
         ("water cc-pvdz all-electron", water, "cc-pvdz", False, (5, 19, 126)),
         ("dimer cc-pvdz frozen", dimer, "cc-pvdz", True, (8, 38, 252)),
         ("water def2-tzvp frozen", water, "def2-tzvp", True, (4, 38, 126)),
         # rows too long for the transform's register prefetch, naux no multiple of four, four virtual tiles
         ("trimer cc-pvdz frozen", lambda: mbe.build_fragment(w3_system(), (0, 1, 2)), "cc-pvdz", True, (12, 57, 378))]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_reference(case):
    what, make, basis, frozen, shapes = case
    frag = make()
    r = methods.run_hip_rimp2_batch(settings(basis), [frag], frozen_core=frozen)[0]
    o = check_against_reference(r, frag, basis, frozen, what)
    assert (o["no"], o["nv"], o["naux"]) == shapes
    if o["no"] == 1:
        assert r.energy.mp2_ss == 0.0       # one occupied orbital: V_ab - V_ba cancels term by term
    assert r.energy.mp2_os < 0.0 and r.energy.mp2_ss <= 0.0


def test_water_reference_values():
    r = methods.run_hip_rimp2_batch(settings("cc-pvdz"), [water()])[0]
    assert abs(r.energy.mp2_os - (-0.153174310268)) < 1e-8, r.energy.mp2_os + 0.153174310268
    assert abs(r.energy.mp2_ss - (-0.051324351783)) < 1e-8, r.energy.mp2_ss + 0.051324351783


def _jittered(make_xyz, count, seed, scale=0.03):
    rng = np.random.default_rng(seed)
    return np.stack([make_xyz + scale * rng.normal(size=make_xyz.shape) for _ in range(count)])


def _mixed_groups():
    """70 jittered waters (6-31G), three jittered dimers (cc-pVDZ) and H2 (STO-3G): three topology groups, one of more
    than 64 fragments."""
    return [FragmentGroup(np.array([8, 1, 1], dtype=np.int32), _jittered(wc.DF_GRAD_XYZ, 70, 11), np.zeros(70, dtype=np.int32), basis_set="6-31g"),
            FragmentGroup(np.array([8, 1, 1, 8, 1, 1], dtype=np.int32), _jittered(DIMER_XYZ, 3, 12), np.zeros(3, dtype=np.int32), basis_set="cc-pvdz"),
            FragmentGroup(np.array([1, 1], dtype=np.int32), H2_XYZ[None], np.zeros(1, dtype=np.int32), basis_set="sto-3g")]


def _one(group, k):
    return FragmentGroup(group.element_numbers, group.xyz[k:k + 1], group.charge[k:k + 1], basis_set=group.basis_set)


def test_batch_equals_one_per_call():
    st = settings("sto-3g")
    groups = _mixed_groups()
    rec, e_os, e_ss, done = methods.run_hip_rimp2_groups(st, groups)
    for g, r, a, b, d in zip(groups, rec, e_os, e_ss, done):
        assert not np.any(r["has_error"]) and np.all(d == 1)
        assert np.all(a < 0.0)
        worst = 0.0
        for k in range(g.xyz.shape[0]):
            r1, a1, b1, d1 = methods.run_hip_rimp2_groups(st, [_one(g, k)])
            assert d1[0][0] == 1
            worst = max(worst, abs(a1[0][0] - a[k]), abs(b1[0][0] - b[k]), abs(r1[0]["e_total"][0] - r["e_total"][k]))
        print("group of %d: largest |batch - single| = %.2e" % (g.xyz.shape[0], worst))
        assert worst < 1e-12, worst
    # three fragments of the batch against the reference
    for gi, k in ((0, 0), (0, 69), (1, 2)):
        g = groups[gi]
        o = ref.rimp2_cached(fragment_bohr(list(g.element_numbers), g.xyz[k]), g.basis_set, wc.AUX)
        diffs = (rec[gi]["e_total"][k] - o["scf"], e_os[gi][k] - o["e_os"], e_ss[gi][k] - o["e_ss"])
        print("batch fragment (%d, %d): d(scf) %.2e d(os) %.2e d(ss) %.2e" % ((gi, k) + diffs))
        assert max(abs(v) for v in diffs) < 1e-8, diffs


_CHUNK_PROBE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests import test_gpu_rimp2 as t
from metalquicha_amd import methods
g = t._mixed_groups()[0]
rec, e_os, e_ss, done = methods.run_hip_rimp2_groups(t.settings("6-31g"), [g])
np.save(sys.argv[2], np.stack([rec[0]["e_total"], e_os[0], e_ss[0], done[0].astype(float)]))
"""


def test_chunked_equals_unchunked(tmp_path):
    """The 70 waters under an HBM budget that forces several chunks, in a child process (the budget is read when the
    context is made); MQC_HIP_MP2_TIMING prints one line per chunk."""
    out = str(tmp_path / "chunked.npy")
    child = subprocess.run([sys.executable, "-c", _CHUNK_PROBE, ROOT, out], capture_output=True, text=True, timeout=300,
                           env={**os.environ, "MQC_HIP_HBM_BUDGET_GB": "0.012", "MQC_HIP_MP2_TIMING": "1"})
    assert child.returncode == 0, child.stderr[-2000:]
    chunks = [ln for ln in child.stderr.splitlines() if ln.startswith("mqc_hip rimp2:")]
    assert len(chunks) >= 2, child.stderr[-2000:]
    got = np.load(out)
    g = _mixed_groups()[0]
    rec, e_os, e_ss, done = methods.run_hip_rimp2_groups(settings("6-31g"), [g])
    assert np.all(got[3] == 1.0) and np.all(done[0] == 1)
    worst = max(np.max(np.abs(got[0] - rec[0]["e_total"])), np.max(np.abs(got[1] - e_os[0])), np.max(np.abs(got[2] - e_ss[0])))
    print("%d chunks: largest |chunked - unchunked| = %.2e" % (len(chunks), worst))
    assert worst < 1e-12, worst


_VARIANT_PROBE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests import test_gpu_rimp2 as t
from metalquicha_amd import methods
out = []
for make, basis in ((t.h2, "sto-3g"), (t.water, "cc-pvdz"), (t.dimer, "cc-pvdz")):
    r = methods.run_hip_rimp2_batch(t.settings(basis), [make()])[0]
    out.append([r.energy.scf, r.energy.mp2_os, r.energy.mp2_ss, float(r.has_mp2)])
np.save(sys.argv[2], np.array(out))
"""


def test_transform_with_orbitals_from_l2(tmp_path):
    """Fragments too large for the orbitals to sit in LDS take them from L2 inside the transform's k loops
    (MQC_HIP_MP2_C_LDS=0 sends every fragment that way; read once, hence the child process): the same numbers."""
    out = str(tmp_path / "variant.npy")
    child = subprocess.run([sys.executable, "-c", _VARIANT_PROBE, ROOT, out], capture_output=True, text=True, timeout=300,
                           env={**os.environ, "MQC_HIP_MP2_C_LDS": "0"})
    assert child.returncode == 0, child.stderr[-2000:]
    got = np.load(out)
    for row, (make, basis) in zip(got, ((h2, "sto-3g"), (water, "cc-pvdz"), (dimer, "cc-pvdz"))):
        o = ref.rimp2_cached(make(), basis, wc.AUX)
        diffs = (row[0] - o["scf"], row[1] - o["e_os"], row[2] - o["e_ss"])
        print("%s from L2: d(scf) %.2e d(os) %.2e d(ss) %.2e" % ((basis,) + diffs))
        assert row[3] == 1.0 and max(abs(v) for v in diffs) < 1e-8, diffs
        here = methods.run_hip_rimp2_batch(settings(basis), [make()])[0]
        assert abs(here.energy.mp2_os - row[1]) < 1e-12 and abs(here.energy.mp2_ss - row[2]) < 1e-12


def test_mbe_at_full_order_is_the_whole_system():
    system = w3_system()
    st = settings("6-31g")
    run = mbe.run_mbe_rimp2(system, st, level=3)
    assert not run.errors
    whole = methods.run_hip_rimp2_batch(st, [mbe.build_fragment(system, (0, 1, 2))])[0]
    assert whole.has_mp2
    total, _, _ = mbe.compute_mbe(run.terms, run.energies)
    corr, _, _ = mbe.compute_mbe(run.terms, run.correlation_os + run.correlation_ss)
    print("MBE-3 total %.12f whole %.12f; correlation %.12f whole %.12f" % (total, whole.energy.total(), corr, whole.energy.mp2))
    assert abs(total - whole.energy.total()) < 1e-9, total - whole.energy.total()
    assert abs(corr - whole.energy.mp2) < 1e-9, corr - whole.energy.mp2
    assert abs(run.energies.sum() - (run.energies - run.correlation_os - run.correlation_ss).sum()
               - (run.correlation_os + run.correlation_ss).sum()) < 1e-10
    # SCS-MP2: the parts scaled by hand
    scs = mbe.run_mbe_rimp2(system, st, level=3, scs=(1.2, 1.0 / 3.0))
    scf = run.energies - run.correlation_os - run.correlation_ss
    assert np.max(np.abs(scs.correlation_os - 1.2 * run.correlation_os)) < 1e-12
    assert np.max(np.abs(scs.correlation_ss - run.correlation_ss / 3.0)) < 1e-12
    assert np.max(np.abs(scs.energies - (scf + 1.2 * run.correlation_os + run.correlation_ss / 3.0))) < 1e-11
    # run_mbe is what it was: SCF energies, no correlation fields
    plain = mbe.run_mbe(system, st, level=3)
    assert plain.correlation_os is None and plain.correlation_ss is None and not plain.errors
    assert np.max(np.abs(plain.energies - scf)) < 1e-11, np.max(np.abs(plain.energies - scf))


def _refused(st, frag, frozen_core=True, want_gradient=False):
    group = FragmentGroup(frag.element_numbers, frag.coordinates.T[None], np.array([frag.charge], dtype=np.int32),
                          np.array([frag.multiplicity], dtype=np.int32), None, np.array([frag.nelec], dtype=np.int32))
    status, box = [], {"frozen_core": frozen_core}
    rec = methods.run_hip_scf_groups(st, [group], want_gradient=want_gradient, status_out=status, rimp2=box)[0]
    msg = bytes(rec["message"][0]).split(b"\0", 1)[0].decode()
    assert rec["has_error"][0] == 1 and rec["scf_status"][0] == capi.SCF_NOT_RUN and rec["iterations"][0] == 0, msg
    assert box["mp2_done"][0][0] == 0 and box["e_os"][0][0] == 0.0 and box["e_ss"][0][0] == 0.0
    return status[0], msg


def test_refusals_name_what_is_missing():
    w = water()
    code, msg = _refused(ScfSettings(basis_set="sto-3g", guess="gwh"), w)
    assert code == capi.ERR_UNSUPPORTED and "RI-MP2 uses the fitted tensor of a density-fitted SCF" in msg, msg
    code, msg = _refused(settings("sto-3g", functional="b3lyp"), w)
    assert code == capi.ERR_UNSUPPORTED and "double hybrids are not built" in msg, msg
    code, msg = _refused(settings("sto-3g", unrestricted=True), w)
    assert code == capi.ERR_UNSUPPORTED and "unrestricted MP2" in msg, msg
    code, msg = _refused(settings("sto-3g"), fragment_bohr([8, 1, 1], wc.DF_GRAD_XYZ, multiplicity=3))
    assert code == capi.ERR_UNSUPPORTED and "unrestricted MP2" in msg, msg
    code, msg = _refused(settings("sto-3g"), fragment_bohr([8, 1, 1], wc.DF_GRAD_XYZ, charge=1, multiplicity=2))
    assert code == capi.ERR_UNSUPPORTED and "unrestricted MP2" in msg, msg
    code, msg = _refused(settings("sto-3g"), w, want_gradient=True)
    assert code == capi.ERR_UNSUPPORTED and "RI-MP2 gradients are not built" in msg, msg
    # O6+: one occupied orbital, and the frozen core takes it
    code, msg = _refused(settings("sto-3g"), fragment_bohr([8], [[0.0, 0.0, 0.0]], charge=6))
    assert code == capi.ERR_VALIDATION and "frozen core" in msg and "no active occupied orbital" in msg, msg
    # what the density-fitted SCF refuses keeps its own text: six waters in cc-pVDZ are 144 functions
    rng = np.random.default_rng(5)
    six = np.vstack([water_at(rng, [6.0 * k, 0.0, 0.0]) for k in range(6)])
    code, msg = _refused(settings("cc-pvdz"), fragment_bohr([8, 1, 1] * 6, six))
    assert code == capi.ERR_UNSUPPORTED and "density fitting is available up to n_ao = 140" in msg, msg


def test_null_outputs_are_a_validation_error():
    st = settings("sto-3g")
    w = water()
    m = methods._Marshalled(w, methods._flat_basis(st.basis_set, w), methods._flat_basis(st.aux_basis_set, w))
    opts = methods._options(st, False)
    res = capi.ScfResult()
    e = np.zeros(1); done = np.zeros(1, dtype=np.int32)
    lib = capi.load_library()
    for a, b, d in ((None, capi.dptr(e), done.ctypes.data_as(capi.c_int32_p)), (capi.dptr(e), None, done.ctypes.data_as(capi.c_int32_p)),
                    (capi.dptr(e), capi.dptr(e), None)):
        rc = lib.mqc_hip_rimp2_batch(capi.get_context(), 1, C.byref(m.mol), C.byref(m.bas), C.byref(m.aux_bas), C.byref(opts), C.byref(res), 1, a, b, d)
        assert rc == capi.ERR_VALIDATION
        assert "must not be NULL" in lib.mqc_hip_last_error().decode()


def test_unconverged_fragment_has_no_mp2_and_its_neighbours_do():
    """max_iter = 2: H2 in a minimal basis is converged by symmetry after the two iterations a converged result needs,
    the waters next to it are not."""
    st = settings("sto-3g", max_iter=2)
    frags = [water(), h2(), water(wc.DF_GRAD_XYZ + 0.01)]
    rs = methods.run_hip_rimp2_batch(st, frags)
    assert rs[1].has_mp2 and not rs[1].has_error and rs[1].energy.mp2_os < 0.0
    o = ref.rimp2_cached(frags[1], "sto-3g", wc.AUX)
    assert abs(rs[1].energy.mp2_os - o["e_os"]) < 1e-8
    for k in (0, 2):
        assert rs[k].has_error and "did not converge" in rs[k].error_message
        assert not rs[k].has_mp2 and rs[k].energy.mp2_os == 0.0 and rs[k].energy.mp2_ss == 0.0
    group = FragmentGroup(frags[0].element_numbers, np.stack([frags[0].coordinates.T, frags[2].coordinates.T]), np.zeros(2, dtype=np.int32))
    rec, e_os, e_ss, done = methods.run_hip_rimp2_groups(st, [group])
    assert np.all(done[0] == 0) and np.all(e_os[0] == 0.0) and np.all(e_ss[0] == 0.0)


def test_frozen_core_on_h2_freezes_nothing_and_plain_scf_is_untouched():
    st = settings("sto-3g")
    a = methods.run_hip_rimp2_batch(st, [h2()], frozen_core=True)[0]
    b = methods.run_hip_rimp2_batch(st, [h2()], frozen_core=False)[0]
    assert a.has_mp2 and b.has_mp2 and abs(a.energy.mp2_os - b.energy.mp2_os) < 1e-12 and a.energy.mp2_ss == 0.0 == b.energy.mp2_ss
    plain = methods.run_hip_scf(st, water())
    assert not plain.has_error and not plain.has_mp2
    assert plain.energy.total() == plain.energy.scf and plain.energy.mp2 == 0.0
    # freezing the core of water takes one occupied orbital out: less correlation than all-electron
    fc = methods.run_hip_rimp2_batch(st, [water()], frozen_core=True)[0]
    ae = methods.run_hip_rimp2_batch(st, [water()], frozen_core=False)[0]
    assert ae.energy.mp2 < fc.energy.mp2 < 0.0 and abs(fc.energy.scf - ae.energy.scf) < 1e-12


def test_embedded_fragment():
    """Water 6-31G in two point charges: the orbitals carry the field, the stage is the same."""
    frag = water()
    pts = np.array([[0.0, 0.0, 5.0], [3.0, -2.0, -4.0]])
    q = np.array([-0.8, 0.4])
    group = FragmentGroup(frag.element_numbers, frag.coordinates.T[None], np.zeros(1, dtype=np.int32),
                          point_charge_xyz=pts[None], point_charges=q[None])
    rec, e_os, e_ss, done = methods.run_hip_rimp2_groups(settings("6-31g"), [group])
    assert rec[0]["has_error"][0] == 0 and done[0][0] == 1
    u = so.point_charge_potential(oracle_mol("6-31g", frag), pts, q)
    o = ref.rimp2(frag, "6-31g", wc.AUX, True, h_extra=u)
    free = ref.rimp2_cached(frag, "6-31g", wc.AUX)
    diffs = (rec[0]["e_total"][0] - o["scf"], e_os[0][0] - o["e_os"], e_ss[0][0] - o["e_ss"])
    print("embedded water: d(scf) %.2e d(os) %.2e d(ss) %.2e; the field moves e_os by %.2e" % (diffs + (o["e_os"] - free["e_os"],)))
    assert max(abs(v) for v in diffs) < 1e-8, diffs
    assert abs(o["e_os"] - free["e_os"]) > 1e-6        # the field is felt: the comparison above is not the free molecule's
