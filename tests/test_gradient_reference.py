"""CPU checks of the gradient stage's reference (tests/gradient_reference.py) and cases (tests/gradient_stage_cases.py).
Nothing here touches a GPU; the class lists come from the host-only half of mqc_hip_gradient_stage.

What is asserted:
  * the numpy S, T, V agree with the C oracle's to 1e-12 on both probe bases, on `generic` and `stretched`
    (measured: 1.1e-14 at most, in V);
  * the complex-step derivative agrees with the Richardson central difference (h = 1e-3 and 2e-3) of the same routine to
    1e-11 of the largest derivative element, for one four-centre row of (ss|ss), (pp|ps), (dd|dp), (ff|fd), (ff|ff), a
    two-centre pair of each l, and one three-centre and one two-centre row of the density-fitted term
    (measured for (ff|ff): 9.6e-14 on 0.031);
  * the twelve derivatives of a row add up to zero per axis (translational invariance of the reference);
  * gamma_block summed over every unique quartet reproduces 1/2 D.J[D] - 1/4 exx D.K[D] from build_jk_incore, restricted
    and unrestricted, on the spd probe;
  * every one of the 55 classes of the spdf probe (21 of spd) has a row on four atoms in the ENGINE'S list, the lists
    together hold every unique quartet once, and select_rows covers whatever a list contains in at most eight rows;
  * the step-size disagreement of the finite-difference reference of the whole-fragment two-electron term stays at the
    figure the GPU test's bound is ten times of (gradient_stage_cases.FD_DISAGREEMENT)."""
import numpy as np
import pytest

from oracle import scf_oracle as so
from tests import gradient_reference as gr
from tests import gradient_stage_cases as gc
from tests import stages
from tests.helpers import oracle_mol


@pytest.fixture
def probe_dir(tmp_path, monkeypatch):
    gc.cc.write_basis_files(tmp_path)
    monkeypatch.setenv("MQC_BASIS_PATH", str(tmp_path))
    return tmp_path


@pytest.mark.parametrize("case", ["generic", "stretched"])
@pytest.mark.parametrize("basis", [gc.SPD, gc.SPDF])
def test_numpy_one_electron_integrals_match_the_oracle(probe_dir, basis, case):
    mol = oracle_mol(basis, gc.CASES[case]())
    ref = so.int1e(mol)
    for name, a, b in zip("STV", gr.int1e(mol), ref):
        err = float(np.max(np.abs(a - b)))
        print("%s %s %s: %.2e" % (basis, case, name, err))
        assert err <= 1e-12, name


def _first_row(basis, frag, mol, cls, ncen):
    rows, _ = stages.gradient_rows(basis, frag, cls, count=None)
    at = gr.shell_atoms(mol)
    for r in rows:
        if len({at[r[0]], at[r[1]], at[r[2]], at[r[3]]}) == ncen:
            return [int(v) for v in r]
    raise AssertionError("no row of %r on %d atoms" % (cls, ncen))


@pytest.mark.parametrize("cls", [(0, 0, 0, 0), (1, 1, 1, 0), (2, 2, 2, 1), (3, 3, 3, 2), (3, 3, 3, 3)])
def test_complex_step_quartet_against_richardson(probe_dir, cls):
    frag = gc.CASES["generic"]()
    mol = oracle_mol(gc.SPDF, frag)
    row = _first_row(gc.SPDF, frag, mol, cls, 4)
    at = gr.shell_atoms(mol)
    shells = [gr._shell(mol, X) for X in row]
    centres = np.array([mol.xyz[at[X]] for X in row])
    cs = gr.d_block(shells, centres)
    fd = gr.richardson_gradient(lambda c: gr.quartet_block(shells, c), centres, 1e-3)
    scale = float(np.max(np.abs(cs)))
    err = float(np.max(np.abs(cs - fd)))
    print("%r row %r: |cs - fd| = %.2e on %.3g" % (cls, row, err, scale))
    assert err <= 1e-11 * scale
    # translational invariance: the four centres' derivatives cancel, element by element
    assert float(np.max(np.abs(cs.sum(axis=0)))) <= 1e-13 * scale


@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_complex_step_pair_against_richardson(probe_dir, l):
    frag = gc.CASES["generic"]()
    mol = oracle_mol(gc.SPDF, frag)
    at = gr.shell_atoms(mol)
    A, B = next((A, B) for A in range(mol.nshell) for B in range(A) if mol.sh_l[A] == l and mol.sh_l[B] == l and at[A] != at[B])
    n = mol.nao
    D, W = gc.symmetric(n, 11), gc.symmetric(n, 12)
    g, mag = gr.d_pair(mol, mol.xyz, A, B, D, W)
    nf = 2 * l + 1
    sa, sb = slice(mol.sh_aoff[A], mol.sh_aoff[A] + nf), slice(mol.sh_aoff[B], mol.sh_aoff[B] + nf)

    def energy(xyz):
        S, T, V = gr.stv_block(gr._shell(mol, A), xyz[at[A]], gr._shell(mol, B), xyz[at[B]], mol.z, xyz)
        return 2.0 * np.sum(D[sa, sb] * (T + V) - W[sa, sb] * S)
    fd = gr.richardson_gradient(energy, mol.xyz, 1e-3)
    scale = float(np.max(np.abs(g)))
    err = float(np.max(np.abs(g - fd)))
    print("pair l = %d (%d, %d): |cs - fd| = %.2e on %.3g (sum of magnitudes %.3g)" % (l, A, B, err, scale, mag))
    assert err <= 1e-11 * max(scale, mag)
    assert float(np.max(np.abs(g.sum(axis=0)))) <= 1e-12 * mag                # functions and nuclei move together


@pytest.mark.parametrize("mode", [stages.GRAD_DF3C, stages.GRAD_DF2C])
def test_complex_step_fitted_rows_against_richardson(probe_dir, mode):
    frag = gc.CASES["generic"]()
    mol = oracle_mol(gc.SPDF, frag)
    cls = (3, 1, 2, 0) if mode == stages.GRAD_DF3C else (3, 0, 2, 0)
    rows, _ = stages.gradient_rows(gc.SPDF, frag, cls, count=None, mode=mode, aux_basis_set=gc.SPDF)
    at = gr.shell_atoms(mol)
    if mode == stages.GRAD_DF3C:
        row = next(r for r in rows if len({at[r[0]], at[r[1]], at[r[2]]}) == 3)
        cs = gr.d_three_centre_block(mol, mol, mol.xyz, row)
        shells = [gr._shell(mol, row[0]), gr._shell(mol, row[1]), gr._shell(mol, row[2]), gr._shell(None, gr.UNIT)]
        centres = np.array([mol.xyz[at[row[0]]], mol.xyz[at[row[1]]], mol.xyz[at[row[2]]], mol.xyz[at[row[2]]]])
        ref = so.eri3c(mol, mol)
        blk = gr.quartet_block(shells, centres)[..., 0]
        nf = 2 * mol.sh_l + 1
        s = [slice(mol.sh_aoff[X], mol.sh_aoff[X] + nf[X]) for X in row[:3]]
        assert float(np.max(np.abs(blk - ref[s[0], s[1], s[2]]))) <= 1e-12            # the unit shell is the function 1
    else:
        row = next(r for r in rows if at[r[0]] != at[r[2]])
        cs = gr.d_two_centre_block(mol, mol.xyz, row)
        shells = [gr._shell(mol, row[0]), gr._shell(None, gr.UNIT), gr._shell(mol, row[2]), gr._shell(None, gr.UNIT)]
        centres = np.array([mol.xyz[at[row[0]]], mol.xyz[at[row[0]]], mol.xyz[at[row[2]]], mol.xyz[at[row[2]]]])
        ref = so.eri2c(mol)
        blk = gr.quartet_block(shells, centres)[:, 0, :, 0]
        nf = 2 * mol.sh_l + 1
        s = [slice(mol.sh_aoff[X], mol.sh_aoff[X] + nf[X]) for X in (row[0], row[2])]
        assert float(np.max(np.abs(blk - ref[s[0], s[1]]))) <= 1e-12
    fd = gr.richardson_gradient(lambda c: gr.quartet_block(shells, c), centres, 1e-3)
    scale = float(np.max(np.abs(cs)))
    err = float(np.max(np.abs(cs - fd)))
    print("mode %d row %r: |cs - fd| = %.2e on %.3g" % (mode, list(row), err, scale))
    assert err <= 1e-11 * scale
    assert float(np.max(np.abs(cs.sum(axis=0)))) <= 1e-13 * scale


@pytest.mark.parametrize("unrestricted", [False, True])
def test_gamma_blocks_add_up_to_the_two_electron_energy(probe_dir, unrestricted):
    mol = oracle_mol(gc.SPD, gc.CASES["generic"]())
    n = mol.nao
    D, Db = gc.symmetric(n, 21), (gc.symmetric(n, 22) if unrestricted else None)
    eri = so.eri4(mol)
    nf = 2 * mol.sh_l + 1
    sl = [slice(int(mol.sh_aoff[X]), int(mol.sh_aoff[X] + nf[X])) for X in range(mol.nshell)]
    for exx in (1.0, 0.25):
        total = sum(float(np.sum(gr.gamma_block(mol, D, Db, exx, r) * eri[sl[r[0]], sl[r[1]], sl[r[2]], sl[r[3]]]))
                    for r in gr.unique_quartets(mol.nshell))
        ref = gr.two_electron_energy(eri, D, Db, exx)
        terms = 0.5 * float(np.einsum("ij,kl,ijkl->", np.abs(D if Db is None else D + Db), np.abs(D if Db is None else D + Db), np.abs(eri)))
        print("exx %.2f unrestricted %d: %.12f against %.12f (sum of magnitudes %.3g)" % (exx, unrestricted, total, ref, terms))
        assert abs(total - ref) <= 1e-13 * terms


@pytest.mark.parametrize("basis,lmax,nclass", [(gc.SPD, 2, 21), (gc.SPDF, 3, 55)])
def test_every_class_list_has_a_four_centre_row_and_the_selection_covers_it(probe_dir, basis, lmax, nclass):
    frag = gc.CASES["generic"]()
    mol = oracle_mol(basis, frag)
    at = gr.shell_atoms(mol)
    classes = gc.classes(lmax)
    assert len(classes) == nclass
    seen = set()
    for cls in classes:
        rows, length = stages.gradient_rows(basis, frag, cls, count=None)
        assert length == len(rows) and length > 0
        for r in rows:
            assert tuple(int(mol.sh_l[x]) for x in r) == cls
            A, B, C, D = (int(v) for v in r)
            key = tuple(sorted([tuple(sorted((A, B))), tuple(sorted((C, D)))]))
            assert key not in seen                                                   # no unique quartet twice
            seen.add(key)
            # a bra that equals the ket is stored in the same order: the kernel's (A == D && B == C) test of `same` can
            # only be met together with (A == C && B == D)
            assert not (A == D and B == C and A != B)
        chosen, one, missing, uncovered = gc.select_rows(rows, at, gc.class_seed(cls))
        assert "4 atoms" not in missing and "3 atoms" not in missing and "2 atoms" not in missing, cls
        assert not uncovered and 1 <= len(chosen) <= gc.MAX_ROWS, cls
        got = set().union(*[gc.row_properties(rows[k], at)[0] for k in chosen])
        assert got == set(gc.PROPERTIES) - set(missing)
        assert len(one) == 1 and gc.row_properties(rows[one[0]], at)[1] == 1, cls   # every class has a single-atom row here
    npair = mol.nshell * (mol.nshell + 1) // 2
    assert len(seen) == npair * (npair + 1) // 2


def test_finite_difference_reference_step_disagreement(probe_dir):
    """Richardson (1e-3, 2e-3) against Richardson (2e-3, 4e-3) of the whole-fragment two-electron energy on the C
    oracle, relative to the largest gradient component: the figure the GPU test allows ten times of."""
    worst = 0.0
    for case in ("generic", "stretched"):
        mol = oracle_mol(gc.SPD, gc.CASES[case]())
        n = mol.nao
        fns = gc.whole_fragment_functionals(n)
        g1, g2 = gc.fd_two_electron(mol, [f for _, f in fns])
        for (name, _), a, b in zip(fns, np.moveaxis(g1, -1, 0), np.moveaxis(g2, -1, 0)):
            rel = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
            print("%s %s: step disagreement %.2e of %.3g" % (case, name, rel, np.max(np.abs(a))))
            worst = max(worst, rel)
    print("worst %.2e" % worst)
    assert worst <= gc.FD_DISAGREEMENT
