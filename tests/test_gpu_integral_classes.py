"""GPU tests of the integral stage on the class-probe cases (tests/integral_class_cases.py): every canonical ERI class
on four distinct centres, in every shell order, on a geometry without a symmetry plane -- through the stage entries,
the alternative routes, the batch routes and the direct digest kernels.

Reference of every comparison: the CPU references (the C oracle so.eri4 / so.int1e, the numpy McMurchie-Davidson code
rr.eri4_erf for the attenuated operator; tests/test_integral_class_cases.py holds them to 1e-12 of each other), never
another route of the engine.  Bounds:
  * tensor elements 1e-11 (the project's elementwise bound, test/test_mqc_libcint_direct.f90:139), M == M.T exactly, no
    NaN (the stage entry poisons the tensor first);
  * contractions with a density: 1e-11 * sum |D| -- what 1e-11 on every element implies; with the sparse densities of
    cc.sparse_density (8 pairs, |D_kl| <= 1) that is at most 1.6e-10;
  * the density-weighted screen of the direct build: the sum of what the dropped quartets would have contributed,
    from the reference tensor and the oracle's Schwarz bounds, + 1e-10.
A failure names the worst classes and their centre counts.

Not here: a -DMQC_BRA_OUTER=0 build.  csrc/build.sh writes one library at one place from one set of objects and takes
no extra flags, so it cannot put such a build beside the default one without touching it."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import scf_oracle as so
from tests import integral_class_cases as cc
from tests import range_separated_reference as rr
from tests import stages
from tests.helpers import fragment_bohr, oracle_mol, synthetic_density, water_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
OMEGAS = (rr.WB97X_OMEGA, 0.33)           # wB97X and CAM-B3LYP
BASIS_CASES = [(b, c) for b in (cc.SPD, cc.SPDF) for c in cc.CASES]


@pytest.fixture(autouse=True)
def probe_dir(tmp_path, monkeypatch):
    cc.write_basis_files(tmp_path)
    monkeypatch.setenv("MQC_BASIS_PATH", str(tmp_path))
    return tmp_path


# ---- references, formed once per process ------------------------------------------------------------------------------
_ERI4, _ATT, _MAP = {}, {}, {}


def coulomb_reference(basis, case):
    if (basis, case) not in _ERI4:
        _ERI4[(basis, case)] = so.eri4(oracle_mol(basis, cc.CASES[case]()))
    return _ERI4[(basis, case)]


def attenuated_reference(basis, case, omega, probe_dir):
    """Packed rr.eri4_erf tensor; all eight (basis, case, omega) tensors are formed side by side on the first call."""
    if not _ATT:
        t0 = time.time()
        _ATT.update(cc.numpy_reference_packed(probe_dir, probe_dir, [(b, c, w) for b, c in BASIS_CASES for w in OMEGAS]))
        print("attenuated references: %.0f s" % (time.time() - t0))
    return _ATT[(basis, case, float(omega))]


def class_map(basis):
    if basis not in _MAP:
        _MAP[basis] = cc.class_of_elements(oracle_mol(basis, cc.generic()))
    return _MAP[basis]


def check_tensor(M, ref, basis, what, tol=TOL):
    assert M.shape == ref.shape
    assert not np.any(np.isnan(M)), "%s: %d elements never written" % (what, int(np.isnan(M).sum()))
    rep = cc.error_report(M - ref, *class_map(basis))
    print("%s: worst classes: %s" % (what, cc.format_report(rep, 3)))
    assert rep[0][2] < tol, "%s: %s" % (what, cc.format_report(rep))
    assert np.max(np.abs(M - M.T)) == 0.0, what


def shell_pair_report(err, mol):
    """Maximum of an (n, n) error matrix per (l, l') of the shells: [(label, max)] worst first."""
    ao_l = np.repeat(np.asarray(mol.sh_l), 2 * np.asarray(mol.sh_l) + 1)
    out = {}
    for a in range(4):
        for b in range(a + 1):
            sel = ((ao_l[:, None] == a) & (ao_l[None, :] == b)) | ((ao_l[:, None] == b) & (ao_l[None, :] == a))
            if sel.any():
                out["<%s|%s>" % ("spdf"[a], "spdf"[b])] = float(np.max(np.abs(err)[sel]))
    return sorted(out.items(), key=lambda kv: -kv[1])


def check_matrix(X, ref, bound, mol, what):
    assert not np.any(np.isnan(X)), what
    rep = shell_pair_report(X - ref, mol)
    print("%s: %s (bound %.2e)" % (what, "; ".join("%s %.2e" % r for r in rep[:3]), bound))
    assert rep[0][1] < bound, "%s: %s, bound %.2e" % (what, "; ".join("%s %.2e" % r for r in rep), bound)


# ---- stage entries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis,case", BASIS_CASES)
def test_int1e_matches_oracle(basis, case):
    frag = cc.CASES[case]()
    mol = oracle_mol(basis, frag)
    S, T, V = stages.int1e(basis, frag)
    So, To, Vo = so.int1e(mol)
    check_matrix(S, So, 1e-12, mol, "S %s %s" % (basis, case))
    check_matrix(T, To, 1e-11, mol, "T %s %s" % (basis, case))
    check_matrix(V, Vo, 1e-10, mol, "V %s %s" % (basis, case))


@pytest.mark.parametrize("basis,case", BASIS_CASES)
def test_eri_packed_matches_oracle(basis, case):
    M = stages.eri_packed(basis, cc.CASES[case]())
    check_tensor(M, stages.pack_eri(coulomb_reference(basis, case)), basis, "eri_packed %s %s" % (basis, case))


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("basis,case", BASIS_CASES)
def test_eri_packed_attenuated_matches_reference(basis, case, omega, probe_dir):
    M = stages.eri_packed_attenuated(basis, cc.CASES[case](), omega)
    check_tensor(M, attenuated_reference(basis, case, omega, probe_dir), basis, "attenuated %g %s %s" % (omega, basis, case))


@pytest.mark.parametrize("basis,case", BASIS_CASES)
def test_jk_incore_matches_oracle(basis, case):
    frag = cc.CASES[case]()
    mol = oracle_mol(basis, frag)
    D = cc.sparse_density(mol.nao, 11)
    J, K = stages.jk_incore(basis, frag, D)
    Jo, Ko = so.build_jk_incore(coulomb_reference(basis, case), D)
    bound = TOL * np.sum(np.abs(D))
    check_matrix(J, Jo, bound, mol, "jk_incore J %s %s" % (basis, case))
    check_matrix(K, Ko, bound, mol, "jk_incore K %s %s" % (basis, case))


@pytest.mark.parametrize("tol", [1e-12, 1e-9])
@pytest.mark.parametrize("basis", [cc.SPD, cc.SPDF])
def test_screening_against_the_reference(basis, tol):
    """Schwarz screening on `stretched`, judged by the reference and not by the engine's own unscreened run: what the
    engine left zero is at most the tolerance in the reference, everything else meets the elementwise bound, and at
    1e-9 something has been dropped."""
    ref = stages.pack_eri(coulomb_reference(basis, "stretched"))
    M = stages.eri_packed(basis, cc.stretched(), schwarz_tol=tol)
    assert not np.any(np.isnan(M))
    zero = M == 0.0
    cid, ncen = class_map(basis)
    if zero.any():
        rep = cc.error_report(np.where(zero, ref, 0.0), cid, ncen)
        assert rep[0][2] <= tol, "dropped although large: %s" % cc.format_report(rep)
    rep = cc.error_report(np.where(zero, 0.0, M - ref), cid, ncen)
    assert rep[0][2] < TOL, cc.format_report(rep)
    assert np.max(np.abs(M - M.T)) == 0.0
    print("%s tol %g: %d of %d elements left zero" % (basis, tol, int(zero.sum()), zero.size))
    if tol == 1e-9:
        assert zero.sum() > np.count_nonzero(ref == 0.0)


# ---- other routes of the same tensor, each in a fresh process ---------------------------------------------------------
_ROUTE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import integral_class_cases as cc, stages
out = {}
for b in (cc.SPD, cc.SPDF):
    for c in cc.CASES:
        out["c|%s|%s" % (b, c)] = stages.eri_packed(b, cc.CASES[c]())
        out["a|%s|%s" % (b, c)] = stages.eri_packed_attenuated(b, cc.CASES[c](), float(sys.argv[3]))
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("route", ["MQC_HIP_ERI_GENERAL=4", "MQC_HIP_TWIN_WAVE_MAX=0", "MQC_HIP_NO_TWIN_BLOCKS=1"])
def test_routes_match_the_references(route, probe_dir):
    """Every pass class through the wave-per-quartet general kernel, the twin entries through the lane-per-entry kernel,
    and no twin blocks at all: both operators on all four cases (the route switches are read once per process)."""
    key, val = route.split("=")
    out = str(probe_dir / "route.npz")
    subprocess.run([sys.executable, "-c", _ROUTE_CHILD, ROOT, out, repr(OMEGAS[0])], env={**os.environ, key: val}, check=True, timeout=600)
    got = np.load(out)
    for b, c in BASIS_CASES:
        check_tensor(got["c|%s|%s" % (b, c)], stages.pack_eri(coulomb_reference(b, c)), b, "%s eri_packed %s %s" % (route, b, c))
        check_tensor(got["a|%s|%s" % (b, c)], attenuated_reference(b, c, OMEGAS[0], probe_dir), b, "%s attenuated %s %s" % (route, b, c))


# ---- batch routes through mqc_hip_coulomb_batch (full mode) -------------------------------------------------------------
def check_batch(basis, frags, J, which, what):
    """J[f] against einsum(so.eri4, D[f]) for f in `which`; the densities are cc.sparse_density(n, 500 + f)."""
    worst = 0.0
    for f in which:
        mol = oracle_mol(basis, frags[f])
        D = cc.sparse_density(mol.nao, 500 + f)
        Jo = np.einsum("ijkl,kl->ij", so.eri4(mol), D)
        bound = TOL * np.sum(np.abs(D))
        assert bound <= 1.6e-10
        assert not np.any(np.isnan(J[f])), (what, f)
        rep = shell_pair_report(J[f] - Jo, mol)
        worst = max(worst, rep[0][1])
        assert rep[0][1] < bound, "%s fragment %d: %s, bound %.2e" % (what, f, "; ".join("%s %.2e" % r for r in rep), bound)
    print("%s: %d fragments checked, worst |dJ| %.2e" % (what, len(list(which)), worst))


def batch_densities(n, m):
    return np.array([cc.sparse_density(n, 500 + f) for f in range(m)])


@pytest.mark.parametrize("basis,m", [(cc.SPD, 1), (cc.SPD, 20), (cc.SPDF, 20)])
def test_coulomb_batch_every_fragment(basis, m):
    """1 fragment (small-batch routes) and 20 (above the twin-wave limit of 16: lane = fragment kernels, task lists),
    every fragment against the oracle."""
    frags = [cc.jitter(k) for k in range(m)]
    n = oracle_mol(basis, frags[0]).nao
    J = stages.coulomb_batch(basis, frags, batch_densities(n, m))
    check_batch(basis, frags, J, range(m), "coulomb_batch %s x%d" % (basis, m))


def test_coulomb_batch_with_shared_blocks():
    """24 fragments, H and C bit-identical in groups of 8: their blocks are formed once per group and copied."""
    frags = cc.sharing_batch()
    J = stages.coulomb_batch(cc.SPD, frags, batch_densities(40, 24))
    check_batch(cc.SPD, frags, J, range(24), "coulomb_batch shared blocks")


N_BIG, N_BIG_CHECKED = 70, 8
_BIG_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import integral_class_cases as cc, stages
from tests.test_gpu_integral_classes import N_BIG, batch_densities
np.save(sys.argv[2], stages.coulomb_batch(cc.SPD, [cc.jitter(k) for k in range(N_BIG)], batch_densities(40, N_BIG)))
"""


@pytest.mark.parametrize("tri", ["default", "MQC_HIP_ERI_TRI=0"])
def test_coulomb_batch_of_seventy(tri, probe_dir):
    """70 fragments of 40 functions: the triangular tensor and jk_tri_kernel (default), the square tensor in a child
    with MQC_HIP_ERI_TRI=0.  8 fragments, drawn from a fixed seed, are compared with the oracle; the other 62 of the
    70 (89 %) are not compared with anything here."""
    which = sorted(np.random.default_rng(70).choice(N_BIG, size=N_BIG_CHECKED, replace=False).tolist())
    frags = [cc.jitter(k) for k in range(N_BIG)]
    if tri == "default":
        J = stages.coulomb_batch(cc.SPD, frags, batch_densities(40, N_BIG))
    else:
        out = str(probe_dir / "big.npy")
        subprocess.run([sys.executable, "-c", _BIG_CHILD, ROOT, out], env={**os.environ, "MQC_HIP_ERI_TRI": "0"}, check=True, timeout=600)
        J = np.load(out)
    check_batch(cc.SPD, frags, J, which, "coulomb_batch x70 %s" % tri)


# ---- the direct digest kernels: mqc_hip_jk_direct ------------------------------------------------------------------------
@pytest.mark.parametrize("basis,case", BASIS_CASES)
def test_jk_direct_matches_oracle(basis, case):
    """Nothing screened (schwarz_tol = 0): the 21 eri_digest_kernel instantiations (spd) and launch_digest_general
    (the f classes and the large d classes) against the oracle, J and K."""
    frag = cc.CASES[case]()
    mol = oracle_mol(basis, frag)
    D = cc.sparse_density(mol.nao, 23)
    J, K = stages.jk_direct(basis, frag, D, schwarz_tol=0.0, exx=1.0)
    Jo, Ko = so.build_jk_incore(coulomb_reference(basis, case), D)
    bound = TOL * np.sum(np.abs(D))
    check_matrix(J, Jo, bound, mol, "jk_direct J %s %s" % (basis, case))
    check_matrix(K, Ko, bound, mol, "jk_direct K %s %s" % (basis, case))
    assert np.max(np.abs(J - J.T)) == 0.0 and np.max(np.abs(K - K.T)) == 0.0


def screen_loss_bound(mol, eri, D, tol, exx):
    """What the density-weighted screen of the direct build (eri_kernels.hpp, `Screening`) may cost, from the reference
    alone: the criterion restated on the oracle's Schwarz bounds; every unique shell quartet it drops (with a relative
    margin of 1e-6 on the estimate for quartets that sit on the threshold) contributes the absolute sum of its terms
    to the J and K elements it feeds.  -> (bound on |dJ|, bound on |dK|, number of dropped quartets)."""
    ns = mol.nshell
    Q = so.schwarz(mol)
    nf = 2 * np.asarray(mol.sh_l) + 1
    ao_sh = np.repeat(np.arange(ns), nf)
    off = np.asarray(mol.sh_aoff)
    Dm = np.array([[np.max(np.abs(D[off[a]: off[a] + nf[a], off[b]: off[b] + nf[b]])) for b in range(ns)] for a in range(ns)])
    drop = np.zeros((ns, ns, ns, ns), dtype=bool)
    pairs = [(A, B) for A in range(ns) for B in range(A + 1)]
    ndrop = 0
    for ij, (A, B) in enumerate(pairs):
        for (Cs, Ds) in pairs[: ij + 1]:
            deg = (1.0 if A == B else 2.0) * (1.0 if Cs == Ds else 2.0) * (1.0 if (A, B) == (Cs, Ds) else 2.0)
            dj = 0.5 * max(Dm[A, B], Dm[Cs, Ds])
            dk = 0.125 * exx * max(Dm[A, Cs], Dm[A, Ds], Dm[B, Cs], Dm[B, Ds])
            if Q[A, B] * Q[Cs, Ds] * deg * max(dj, dk) >= tol * (1.0 + 1e-6):
                continue
            ndrop += 1
            for a, b in ((A, B), (B, A)):
                for c, d in ((Cs, Ds), (Ds, Cs)):
                    drop[a, b, c, d] = True
                    drop[c, d, a, b] = True
    lost = np.abs(eri) * drop[ao_sh[:, None, None, None], ao_sh[None, :, None, None], ao_sh[None, None, :, None], ao_sh[None, None, None, :]]
    return np.einsum("ijkl,kl->ij", lost, np.abs(D)), np.einsum("ikjl,kl->ij", lost, np.abs(D)), ndrop


@pytest.mark.parametrize("basis", [cc.SPD, cc.SPDF])
def test_jk_direct_density_weighted_screen(basis):
    """schwarz_tol = 1e-11 on `stretched` with the dense test density: the error budget is the screen's.  The bound is
    derived from the reference (screen_loss_bound), never from an engine run; + 1e-10 for rounding, as everywhere."""
    frag = cc.stretched()
    mol = oracle_mol(basis, frag)
    D = synthetic_density(mol.nao)
    eri = coulomb_reference(basis, "stretched")
    bJ, bK, ndrop = screen_loss_bound(mol, eri, D, 1e-11, 1.0)
    assert ndrop > 0                     # the screen has something to drop, or this test checks nothing
    print("%s: the restated screen drops %d quartets; loss bounds max %.2e (J) %.2e (K)" % (basis, ndrop, bJ.max(), bK.max()))
    J, K = stages.jk_direct(basis, frag, D, schwarz_tol=1e-11, exx=1.0)
    Jo, Ko = so.build_jk_incore(eri, D)
    assert not np.any(np.isnan(J)) and not np.any(np.isnan(K))
    eJ, eK = np.abs(J - Jo) - bJ, np.abs(K - Ko) - bK
    print("%s: max |dJ| %.2e, max |dK| %.2e" % (basis, np.max(np.abs(J - Jo)), np.max(np.abs(K - Ko))))
    assert np.max(eJ) <= 1e-10, shell_pair_report(np.maximum(eJ, 0.0), mol)
    assert np.max(eK) <= 1e-10, shell_pair_report(np.maximum(eK, 0.0), mol)


def test_jk_direct_without_exchange_writes_a_zero_k():
    """exx = 0 (pure functionals, Coulomb-only requests): J as before, K all zeros -- the header's promise."""
    frag = cc.generic()
    mol = oracle_mol(cc.SPDF, frag)
    D = cc.sparse_density(mol.nao, 23)
    J, K = stages.jk_direct(cc.SPDF, frag, D, schwarz_tol=0.0, exx=0.0)
    Jo = np.einsum("ijkl,kl->ij", coulomb_reference(cc.SPDF, "generic"), D)
    check_matrix(J, Jo, TOL * np.sum(np.abs(D)), mol, "jk_direct exx=0 J")
    assert np.all(K == 0.0)


def test_jk_direct_large_fragment_is_symmetric_in_the_densities():
    """Five waters, cc-pVDZ, n = 120: the size the direct path exists for; the oracle tensor would take too long.
    tr(D J[D']) = tr(D' J[D]) and tr(D K[D']) = tr(D' K[D]) to 1e-9 relative hold for any correct Coulomb and exchange
    build.  This is a SYMMETRY check of the digest kernels at that size, not a parity check against a reference."""
    rng = np.random.default_rng(5)
    frag = fragment_bohr([8, 1, 1] * 5, np.vstack([water_at(rng, [5.5 * i, 0.7 * i, -0.4 * i]) for i in range(5)]))
    n = 120
    D1 = synthetic_density(n) + np.eye(n)
    D2 = synthetic_density(n)[::-1, ::-1].copy() + np.diag(np.linspace(0.5, 1.5, n))
    J1, K1 = stages.jk_direct("cc-pvdz", frag, D1)
    J2, K2 = stages.jk_direct("cc-pvdz", frag, D2)
    for X1, X2, what in ((J1, J2, "J"), (K1, K2, "K")):
        assert not np.any(np.isnan(X1)) and not np.any(np.isnan(X2))
        a, b = np.sum(D1 * X2), np.sum(D2 * X1)
        print("%s: tr(D J[D']) = %.12e, relative asymmetry %.2e" % (what, a, abs(a - b) / abs(a)))
        assert abs(a) > 1.0 and abs(a - b) < 1e-9 * abs(a), (what, a, b)
        assert np.max(np.abs(X1 - X1.T)) == 0.0


def test_jk_direct_refuses_bad_arguments():
    from metalquicha_amd import capi
    D = cc.sparse_density(40, 1)
    for kw in (dict(schwarz_tol=-1.0), dict(exx=-0.5), dict(exx=float("nan"))):
        with pytest.raises(capi.HipBackendError) as e:
            stages.jk_direct(cc.SPD, cc.generic(), D, **kw)
        assert e.value.code == capi.ERR_VALIDATION
