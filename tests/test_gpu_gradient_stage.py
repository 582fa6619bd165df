"""Stage tests of the analytic-gradient kernels (grad_weighted_density_kernel, grad1e_kernel, eri_grad_kernel in its three
modes, the screening kernels) through mqc_hip_gradient_stage, against tests/gradient_reference.py: complex-step
derivatives of a numpy McMurchie-Davidson code, every centre moved directly.  Inputs are the seeded, unconverged
matrices of tests/gradient_stage_cases.py on the class-probe bases and geometries.

Bounds.
  rows    |g - g_ref| <= 1e-11 max(1, S) for every number of every row, S the largest of the sums of magnitudes
          sum |Gamma_ijkl| |d(ij|kl)| over the block among the row's twelve derivatives (for a pair: of the magnitudes of
          D T', D V', W S').  1e-11 is the project's elementwise figure for the integrals; no class needed more.
  whole   g2e against the sum of its rows: 1e-12 of its largest component.  g2e against Richardson differences of the
          fixed-density energy on the C oracle: ten times the reference's own step-size disagreement, measured as 9.38e-11
          of the largest component (tests/test_gradient_reference.py), so 9.4e-10 relative.
  w       1e-13 sum |terms| per element.
The worst ratio to its bound is printed per test."""
import os

import numpy as np
import pytest

from metalquicha_amd import capi
from oracle import scf_oracle as so
from tests import gradient_reference as gr
from tests import gradient_stage_cases as gc
from tests import stages
from tests.helpers import oracle_mol

pytestmark = pytest.mark.gpu

TOL = 1e-11
FD_TOL = 10.0 * gc.FD_DISAGREEMENT
L = "spdf"
# (label, unrestricted, exx)
VARIANTS = [("restricted exx 1", False, 1.0), ("restricted exx 0.25", False, 0.25), ("unrestricted exx 1", True, 1.0)]


@pytest.fixture(scope="module", autouse=True)
def probe_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("probe_basis")
    gc.cc.write_basis_files(d)
    old = os.environ.get("MQC_BASIS_PATH")
    os.environ["MQC_BASIS_PATH"] = str(d)
    yield d
    if old is None:
        os.environ.pop("MQC_BASIS_PATH", None)
    else:
        os.environ["MQC_BASIS_PATH"] = old


_MOL = {}


def probe(basis, case):
    if (basis, case) not in _MOL:
        frag = gc.CASES[case]()
        mol = oracle_mol(basis, frag)
        _MOL[(basis, case)] = (frag, mol, gr.shell_atoms(mol))
    return _MOL[(basis, case)]


def weighted_density(C, eps, nocc, Cb=None, epsb=None, nbeta=0):
    """-> (W, sum of the magnitudes of its terms)."""
    if Cb is None:
        return 2.0 * (C[:, :nocc] * eps[:nocc]) @ C[:, :nocc].T, 2.0 * (np.abs(C[:, :nocc]) * np.abs(eps[:nocc])) @ np.abs(C[:, :nocc]).T
    W = (C[:, :nocc] * eps[:nocc]) @ C[:, :nocc].T + (Cb[:, :nbeta] * epsb[:nbeta]) @ Cb[:, :nbeta].T
    mag = (np.abs(C[:, :nocc]) * np.abs(eps[:nocc])) @ np.abs(C[:, :nocc]).T + (np.abs(Cb[:, :nbeta]) * np.abs(epsb[:nbeta])) @ np.abs(Cb[:, :nbeta]).T
    return W, mag


def orbital_inputs(n, unrestricted):
    C, eps = gc.orbitals(n, gc.SEED_C)
    kw = dict(C_mo=C, eps=eps, n_occ=n // 3)
    if unrestricted:
        Cb, epsb = gc.orbitals(n, gc.SEED_CB)
        kw.update(C_beta=Cb, eps_beta=epsb, n_beta=n // 5)
    return kw


def check_rows(label, got, ref, scale):
    """got, ref (rows, natoms, 3), scale (rows,): every number within TOL max(1, S); -> the worst ratio to the bound."""
    assert np.all(np.isfinite(got)), label
    bound = TOL * np.maximum(1.0, scale)
    ratio = np.max(np.abs(got - ref), axis=(1, 2)) / bound
    print("%s: worst |g - ref| / bound = %.2e (|g| up to %.3g, S up to %.3g)" % (label, ratio.max(), np.abs(ref).max(), scale.max()))
    assert np.all(ratio <= 1.0), "%s: rows %r miss the bound (ratios %r)" % (label, np.flatnonzero(ratio > 1.0), ratio[ratio > 1.0])
    return float(ratio.max())


# ---- per-class rows of the exact two-electron term ------------------------------------------------------------------
@pytest.mark.parametrize("cls", gc.classes(3), ids=lambda c: "(%s%s|%s%s)" % tuple(L[v] for v in c))
def test_two_electron_rows_of_every_class(cls):
    frag, mol, at = probe(gc.SPDF, "generic")
    n = mol.nao
    rows, length = stages.gradient_rows(gc.SPDF, frag, cls, count=None)
    chosen, one, missing, uncovered = gc.select_rows(rows, at, gc.class_seed(cls))
    assert "4 atoms" not in missing and not uncovered
    print("class %r: %d rows in the list, %d taken; the list has no row with: %s" % (cls, length, len(chosen) + len(one), ", ".join(missing) or "-"))
    picks = chosen + one
    dblk = [gr.d_block([gr._shell(mol, X) for X in rows[k]], [mol.xyz[at[X]] for X in rows[k]]) for k in chosen]
    worst = 0.0
    for label, unrestricted, exx in VARIANTS:
        D, Db = gc.densities(n, unrestricted)
        got = np.array([stages.gradient_stage(gc.SPDF, frag, D=D, D_beta=Db, exx=exx, cls=cls, start=k, count=1)["g_rows"][0] for k in picks])
        ref, scale = [], []
        for k, db in zip(chosen, dblk):
            g, s = gr.contract(db, gr.gamma_block(mol, D, Db, exx, rows[k]))
            ref.append(gr.scatter(g, [at[X] for X in rows[k]], len(mol.xyz))); scale.append(s)
        worst = max(worst, check_rows("%r %s" % (cls, label), got[:len(chosen)], np.array(ref), np.array(scale)))
        # one atom: translational invariance, the kernel leaves at once -- exact zeros, not small numbers
        assert len(one) == 1 and np.all(got[len(chosen):] == 0.0), label
    print("class %r: worst ratio %.2e" % (cls, worst))


# ---- per-pair rows of the one-electron terms --------------------------------------------------------------------------
@pytest.mark.parametrize("la,lb", [(a, b) for a in range(4) for b in range(a + 1)], ids=lambda v: L[v])
def test_one_electron_pairs(la, lb):
    frag, mol, at = probe(gc.SPDF, "generic")
    n, ns = mol.nao, mol.nshell
    sh = [(A, B) for A in range(ns) for B in range(ns) if mol.sh_l[A] == la and mol.sh_l[B] == lb]
    two = next(p for p in sh if at[p[0]] != at[p[1]])
    one = next(p for p in sh if at[p[0]] == at[p[1]])
    for unrestricted in (False, True):
        D, Db = gc.densities(n, unrestricted)
        kw = orbital_inputs(n, unrestricted)
        W, _ = weighted_density(kw["C_mo"], kw["eps"], kw["n_occ"], kw.get("C_beta"), kw.get("eps_beta"), kw.get("n_beta", 0))
        Dt = D if Db is None else D + Db
        got, ref, scale = [], [], []
        for (A, B) in (two, one):
            got.append(stages.gradient_stage(gc.SPDF, frag, D=D, D_beta=Db, pair=(A, B), **kw)["g1e_pair"])
            g, s = gr.d_pair(mol, mol.xyz, A, B, Dt, W)
            ref.append(g); scale.append(s)
        # the Hellmann-Feynman force reaches all four nuclei, the two that carry no function of the pair included
        others = [c for c in range(4) if c not in (at[two[0]], at[two[1]])]
        assert len(others) == 2 and np.all(np.max(np.abs(ref[0][others]), axis=1) > 1e-6)
        check_rows("pair (%s, %s) shells %r and %r, %s" % (L[la], L[lb], two, one, "unrestricted" if unrestricted else "restricted"),
                   np.array(got), np.array(ref), np.array(scale))


# ---- rows of the density-fitted term ---------------------------------------------------------------------------------
def _fitted_rows(rows, natoms_of, seed):
    """Four rows by a seeded rule: one with the most distinct atoms, one with the fewest but more than one, two more at
    random among the rows on more than one atom."""
    rng = np.random.default_rng(seed)
    ncen = np.array([len(set(natoms_of(r))) for r in rows])
    several = np.flatnonzero(ncen > 1)
    first = several[ncen[several] == ncen[several].max()]
    last = several[ncen[several] == ncen[several].min()]
    picks = [int(first[rng.integers(len(first))]), int(last[rng.integers(len(last))])]
    picks += [int(v) for v in rng.choice(several, size=2, replace=len(several) < 2)]
    return picks


@pytest.mark.parametrize("la,lb", [(a, b) for a in range(4) for b in range(4)], ids=lambda v: L[v])
def test_three_centre_rows(la, lb):
    frag, mol, at = probe(gc.SPDF, "generic")
    n = mol.nao
    gam = np.random.default_rng(300 + 4 * la + lb).uniform(-1.0, 1.0, size=(n, n, n))
    gam = 0.5 * (gam + gam.transpose(0, 2, 1))                    # Gamma^P is symmetric in the orbital pair
    nf = 2 * mol.sh_l + 1
    sl = [slice(int(mol.sh_aoff[X]), int(mol.sh_aoff[X] + nf[X])) for X in range(mol.nshell)]
    got, ref, scale = [], [], []
    for lp in range(4):
        cls = (la, lb, lp, 0)
        rows, _ = stages.gradient_rows(gc.SPDF, frag, cls, count=None, mode=stages.GRAD_DF3C, aux_basis_set=gc.SPDF)
        for k in _fitted_rows(rows, lambda r: (at[r[0]], at[r[1]], at[r[2]]), gc.class_seed(cls)):
            A, B, P = (int(v) for v in rows[k][:3])
            out = stages.gradient_stage(gc.SPDF, frag, cls=cls, start=k, count=1, mode=stages.GRAD_DF3C, aux_basis_set=gc.SPDF, gam=gam)
            assert np.array_equal(out["rows"][0], rows[k])
            got.append(out["g_rows"][0])
            # both orders of the orbital pair, from the definition sum_{ab} Gam^P_ab (ab|P)
            G = gam[sl[P], sl[A], sl[B]].transpose(1, 2, 0).copy()
            if A != B:
                G += gam[sl[P], sl[B], sl[A]].transpose(2, 1, 0)
            g, s = gr.contract(gr.d_three_centre_block(mol, mol, mol.xyz, rows[k]), G[..., None])
            ref.append(gr.scatter(g, [at[A], at[B], at[P], at[P]], len(mol.xyz))); scale.append(s)
    check_rows("(%s %s|P) rows" % (L[la], L[lb]), np.array(got), np.array(ref), np.array(scale))


@pytest.mark.parametrize("lp", range(4), ids=lambda v: L[v])
def test_two_centre_rows(lp):
    frag, mol, at = probe(gc.SPDF, "generic")
    n = mol.nao
    gam = gc.symmetric(n, 400 + lp)
    nf = 2 * mol.sh_l + 1
    sl = [slice(int(mol.sh_aoff[X]), int(mol.sh_aoff[X] + nf[X])) for X in range(mol.nshell)]
    got, ref, scale = [], [], []
    for lq in range(4):
        cls = (lp, 0, lq, 0)
        rows, _ = stages.gradient_rows(gc.SPDF, frag, cls, count=None, mode=stages.GRAD_DF2C, aux_basis_set=gc.SPDF)
        for k in _fitted_rows(rows, lambda r: (at[r[0]], at[r[2]]), gc.class_seed(cls)):
            P, Q = int(rows[k][0]), int(rows[k][2])
            out = stages.gradient_stage(gc.SPDF, frag, cls=cls, start=k, count=1, mode=stages.GRAD_DF2C, aux_basis_set=gc.SPDF, gam=gam)
            got.append(out["g_rows"][0])
            G = gam[sl[P], sl[Q]].copy()
            if P != Q:
                G += gam[sl[Q], sl[P]].T
            g, s = gr.contract(gr.d_two_centre_block(mol, mol.xyz, rows[k]), G[:, None, :, None])
            ref.append(gr.scatter(g, [at[P], at[P], at[Q], at[Q]], len(mol.xyz))); scale.append(s)
    check_rows("(%s|Q) rows" % L[lp], np.array(got), np.array(ref), np.array(scale))


# ---- the whole fragment -----------------------------------------------------------------------------------------------
_FD = {}


def fd_reference(case):
    """Finite-difference gradients of the whole-fragment functionals of `case` (and, on `stretched`, of the screened
    ones), formed once per module: {name: [natoms][3]}."""
    if case in _FD:
        return _FD[case]
    frag, mol, at = probe(gc.SPD, case)
    fns = gc.whole_fragment_functionals(mol.nao)
    if case == "stretched":
        fns = fns + screened_functionals(mol)
    g, _ = gc.fd_two_electron(mol, [f for _, f in fns], coarse=False)
    _FD[case] = {name: g[..., k] for k, (name, _) in enumerate(fns)}
    return _FD[case]


SCREEN_EXX = 0.25
SCREEN_THRESHOLDS = (1.0e-8, 1.0e-4)
_DROPPED = {}


def screened_functionals(mol):
    """The two-electron energy over exactly the unique quartets whose bound Q_AB Q_CD x (density factor) reaches the
    threshold, as dense tensors G4 . eri; the kept set is that of the undisplaced geometry."""
    n = mol.nao
    Q = so.schwarz(mol)
    nf = 2 * mol.sh_l + 1
    sl = [slice(int(mol.sh_aoff[X]), int(mol.sh_aoff[X] + nf[X])) for X in range(mol.nshell)]
    rows = gr.unique_quartets(mol.nshell)
    out = []
    for unrestricted in (False, True):
        D, Db = gc.densities(n, unrestricted)
        Dt = D if Db is None else D + Db
        bound = np.array([Q[r[0], r[1]] * Q[r[2], r[3]] * gc.screening_factor(Dt, D, Db, SCREEN_EXX, sl, r) for r in rows])
        G4 = {th: np.zeros((n, n, n, n)) for th in SCREEN_THRESHOLDS}
        for r, b in zip(rows, bound):
            blk = None
            for th in SCREEN_THRESHOLDS:
                if b >= th:
                    blk = gr.gamma_block(mol, D, Db, SCREEN_EXX, r) if blk is None else blk
                    G4[th][sl[r[0]], sl[r[1]], sl[r[2]], sl[r[3]]] = blk
        for th in SCREEN_THRESHOLDS:
            name = "screened %s %.0e" % ("UHF" if unrestricted else "RHF", th)
            _DROPPED[name] = (int(np.sum(bound < th)), int(np.sum(np.abs(bound - th) <= 1e-6 * th)), len(rows))
            out.append((name, lambda eri, G=G4[th]: float(np.vdot(G, eri))))
    return out


_ONE = {}


def one_electron_reference(case, unrestricted):
    """sum Dt (T' + V') - W S' over the whole basis with respect to every nucleus, by complex step, and the sums of the
    magnitudes of its terms; formed once per (case, spin)."""
    if (case, unrestricted) in _ONE:
        return _ONE[(case, unrestricted)]
    frag, mol, at = probe(gc.SPD, case)
    n, nat = mol.nao, len(mol.xyz)
    D, Db = gc.densities(n, unrestricted)
    Dt = D if Db is None else D + Db
    kw = orbital_inputs(n, unrestricted)
    W, _ = weighted_density(kw["C_mo"], kw["eps"], kw["n_occ"], kw.get("C_beta"), kw.get("eps_beta"), kw.get("n_beta", 0))
    ref, mag = np.zeros((nat, 3)), np.zeros((nat, 3))
    for c in range(nat):
        for d in range(3):
            dS, dT, dV = (m.imag / gr.STEP for m in gr.int1e(mol, gr._step(mol.xyz, c, d)))
            ref[c, d] = np.sum(Dt * (dT + dV) - W * dS)
            mag[c, d] = np.sum(np.abs(Dt) * (np.abs(dT) + np.abs(dV)) + np.abs(W) * np.abs(dS))
    _ONE[(case, unrestricted)] = (ref, mag)
    return ref, mag


@pytest.mark.parametrize("exx", gc.EXX)
@pytest.mark.parametrize("unrestricted", [False, True], ids=["restricted", "unrestricted"])
@pytest.mark.parametrize("case", ["generic", "stretched"])
def test_whole_fragment(case, unrestricted, exx):
    """g2e = the sum of its rows (every list row once, none twice); g1e against the complex-step reference; g2e against
    Richardson differences of the fixed-density energy on the C oracle.  Step-size disagreement of that reference:
    9.38e-11 of the largest component at worst, so the bound is 9.4e-10 of the largest component.  Measured on the
    MI355X: 1.4e-12 .. 5.5e-12 against the differences, 1.9e-15 .. 6.5e-15 against the sum of the 9316 rows."""
    frag, mol, at = probe(gc.SPD, case)
    n, nat = mol.nao, len(mol.xyz)
    D, Db = gc.densities(n, unrestricted)
    kw = orbital_inputs(n, unrestricted)
    fd = fd_reference(case)
    ref1, mag1 = one_electron_reference(case, unrestricted)
    out = stages.gradient_stage(gc.SPD, frag, D=D, D_beta=Db, exx=exx, want=("g1e", "g2e"), **kw)
    g1, g2 = out["g1e"], out["g2e"]
    assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2))
    r1 = float(np.max(np.abs(g1 - ref1) / (TOL * np.maximum(1.0, mag1))))
    total, nrows = np.zeros((nat, 3)), 0
    for cls in gc.classes(2):
        length = stages.gradient_rows(gc.SPD, frag, cls, 0, 1)[1]
        for k in range(0, length, 4096):
            part = stages.gradient_stage(gc.SPD, frag, D=D, D_beta=Db, exx=exx, cls=cls, start=k, count=min(4096, length - k))
            assert np.all(np.isfinite(part["g_rows"]))
            total += part["g_rows"].sum(axis=0)
            nrows += len(part["g_rows"])
    npair = mol.nshell * (mol.nshell + 1) // 2
    assert nrows == npair * (npair + 1) // 2
    rsum = float(np.max(np.abs(g2 - total)) / np.max(np.abs(g2)))
    ref2 = fd["%s exx %.2f" % ("UHF" if unrestricted else "RHF", exx)]
    rfd = float(np.max(np.abs(g2 - ref2)) / np.max(np.abs(ref2)))
    print("%s %s exx %.2f: g1e ratio to bound %.2e; g2e - sum of %d rows %.2e relative; g2e - finite difference %.2e relative (bound %.1e), |g2e| up to %.3g"
          % (case, "unrestricted" if unrestricted else "restricted", exx, r1, nrows, rsum, rfd, FD_TOL, np.abs(g2).max()))
    assert r1 <= 1.0
    assert rsum <= 1e-12
    assert rfd <= FD_TOL


@pytest.mark.parametrize("unrestricted", [False, True], ids=["restricted", "unrestricted"])
def test_screened_route(unrestricted):
    """`stretched`, Q from the oracle's Schwarz bounds: the screened term is the sum over exactly the quartets whose bound
    reaches the threshold (finite differences of that restricted sum on the C oracle; bound as in test_whole_fragment)."""
    frag, mol, at = probe(gc.SPD, "stretched")
    D, Db = gc.densities(mol.nao, unrestricted)
    Q = so.schwarz(mol)
    fd = fd_reference("stretched")
    full = stages.gradient_stage(gc.SPD, frag, D=D, D_beta=Db, exx=SCREEN_EXX, want=("g2e",))["g2e"]
    for th in SCREEN_THRESHOLDS:
        name = "screened %s %.0e" % ("UHF" if unrestricted else "RHF", th)
        dropped, ambiguous, nrows = _DROPPED[name]
        g = stages.gradient_stage(gc.SPD, frag, D=D, D_beta=Db, exx=SCREEN_EXX, want=("g2e",), Q=Q, q_thresh=th)["g2e"]
        ref = fd[name]
        rel = float(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))
        print("%s: %d of %d quartets dropped, %d within 1e-6 of the threshold; |g - ref| %.2e relative (bound %.1e); screened - unscreened %.2e"
              % (name, dropped, nrows, ambiguous, rel, FD_TOL, np.max(np.abs(g - full))))
        assert dropped > 0 and ambiguous == 0
        assert np.all(np.isfinite(g)) and rel <= FD_TOL


@pytest.mark.parametrize("unrestricted", [False, True], ids=["restricted", "unrestricted"])
@pytest.mark.parametrize("basis", [gc.SPD, gc.SPDF])
def test_weighted_density(basis, unrestricted):
    frag, mol, at = probe(basis, "generic")
    n = mol.nao
    kw = orbital_inputs(n, unrestricted)
    D, Db = gc.densities(n, unrestricted)
    w = stages.gradient_stage(basis, frag, D=D, D_beta=Db, want=("w",), **kw)["w"]
    ref, mag = weighted_density(kw["C_mo"], kw["eps"], kw["n_occ"], kw.get("C_beta"), kw.get("eps_beta"), kw.get("n_beta", 0))
    ratio = float(np.max(np.abs(w - ref) / (1e-13 * mag)))
    print("w %s %s: worst ratio to 1e-13 sum |terms| %.2e" % (basis, "unrestricted" if unrestricted else "restricted", ratio))
    assert np.all(np.isfinite(w)) and ratio <= 1.0


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _refused(words, basis=gc.SPDF, frag=None, **kw):
    out = {}
    with pytest.raises(capi.HipBackendError) as e:
        stages.gradient_stage(basis, frag if frag is not None else probe(basis, "generic")[0], out=out, **kw)
    assert e.value.code == capi.ERR_VALIDATION
    for w in words:
        assert w in e.value.message, e.value.message
    for name, v in out.items():                      # nothing was written
        assert np.all(np.isnan(v)) if v.dtype == np.float64 else np.all(v == -1), name


def test_refusals():
    frag, mol, at = probe(gc.SPDF, "generic")
    n = mol.nao
    D = gc.symmetric(n, 1)
    kw = orbital_inputs(n, False)
    _refused(["l = 4", "l > 3"], D=D, cls=(4, 0, 0, 0), count=1)
    _refused(["no class (3 3|3 3)"], basis=gc.SPD, D=gc.symmetric(40, 1), cls=(3, 3, 3, 3), count=1)
    length = stages.gradient_rows(gc.SPDF, frag, (1, 0, 0, 0), 0, 1)[1]
    _refused(["slice outside the list"], D=D, cls=(1, 0, 0, 0), start=length - 1, count=2)
    _refused(["slice outside the list"], D=D, cls=(1, 0, 0, 0), start=-1, count=1)
    _refused(["null argument", "D"], want=("g2e",))
    _refused(["null argument", "C, eps"], D=D, want=("g1e",))
    _refused(["null argument", "gam"], cls=(1, 0, 1, 0), count=1, mode=stages.GRAD_DF3C, aux_basis_set=gc.SPDF)
    _refused(["null argument", "auxiliary"], cls=(1, 0, 1, 0), count=1, mode=stages.GRAD_DF3C)
    _refused(["does not exist"], D=D, pair=(0, mol.nshell), **kw)
    bad = D.copy(); bad[3, 5] = np.nan
    _refused(["non-finite", "density"], D=bad, want=("g2e",))
    _refused(["non-finite", "density"], D=D, D_beta=bad, want=("g2e",))
    _refused(["non-finite", "exx"], D=D, exx=np.inf, want=("g2e",))
    e2 = kw["eps"].copy(); e2[0] = np.inf
    _refused(["non-finite", "C, eps"], D=D, want=("w",), **dict(kw, eps=e2))
    Q = so.schwarz(mol); Q[0, 0] = np.nan
    _refused(["non-finite", "Q"], D=D, want=("g2e",), Q=Q, q_thresh=1e-8)
    g = np.zeros((n, n, n)); g[1, 2, 3] = np.nan
    _refused(["non-finite", "gam"], cls=(1, 0, 1, 0), count=1, mode=stages.GRAD_DF3C, aux_basis_set=gc.SPDF, gam=g)
    xyz = gc.cc.GENERIC.copy(); xyz[2, 1] = np.nan
    _refused(["non-finite", "coordinate"], frag=gc.cc.fragment_bohr(gc.cc.ELEMENTS, xyz), D=D, want=("g2e",))
    _refused(["occupations"], D=D, want=("w",), **dict(kw, n_occ=n + 1))
