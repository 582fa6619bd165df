"""Cases of the gradient stage tests (tests/test_gpu_gradient_stage.py, tests/test_gradient_reference.py): the probe bases
and geometries of tests/integral_class_cases.py, seeded inputs that are NOT converged SCF results, and the rule that picks
the rows of a class list.

Inputs.  D and D_beta are dense symmetric matrices with entries uniform in [-1, 1]; C is the orthogonal factor of a seeded
normal matrix (entries within [-1, 1], no molecular symmetry); eps is uniform in [-1, 1].  A converged density is small
wherever the basis functions are far apart; these are not, so every weight and every exchange term of Gamma is of order
one in every block.

Rows.  Of the list of a class the tests take at most eight rows that between them cover: four, three and two distinct
atoms; A == B; C == D; bra == ket; none of the three; a bra that the canonical order swapped (A < B: the pair list holds
A >= B and swaps where l_A < l_B) and such a ket (C < D); and one row on a single atom (exact zeros).  select_rows is
greedy: it keeps taking the row that covers most of the properties still open, ties broken by a generator seeded with the
class, until nothing more can be covered.  What a list does not contain is returned as `missing`.

Test infrastructure: no GPU needed, never imported by the package."""
from __future__ import annotations

import numpy as np

from tests import integral_class_cases as cc

SPD, SPDF = cc.SPD, cc.SPDF
CASES = cc.CASES
PROPERTIES = ("4 atoms", "3 atoms", "2 atoms", "A == B", "C == D", "bra == ket", "no equal index", "bra swapped", "ket swapped")
MAX_ROWS = 8


def class_tuple(cid: int):
    return cid // 512, (cid // 64) % 8, (cid // 8) % 8, cid % 8


def classes(lmax: int):
    return [class_tuple(c) for c in cc.canonical_class_ids(lmax)]


def symmetric(n: int, seed: int) -> np.ndarray:
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, n))
    return np.triu(a) + np.triu(a, 1).T


def orbitals(n: int, seed: int):
    """(C, eps): an orthogonal matrix (AO x MO, row-major) and orbital energies in [-1, 1]."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return np.ascontiguousarray(q), rng.uniform(-1.0, 1.0, size=n)


def row_properties(row, atoms):
    A, B, C, D = (int(v) for v in row)
    ncen = len({atoms[A], atoms[B], atoms[C], atoms[D]})
    braket = (A, B) == (C, D) or (A, B) == (D, C)
    out = set()
    if ncen >= 2:
        out.add("%d atoms" % ncen)
    if A == B:
        out.add("A == B")
    if C == D:
        out.add("C == D")
    if braket:
        out.add("bra == ket")
    if A != B and C != D and not braket:
        out.add("no equal index")
    if A < B:
        out.add("bra swapped")
    if C < D:
        out.add("ket swapped")
    return out, ncen


def select_rows(rows, atoms, seed: int):
    """-> (indices into rows, at most MAX_ROWS of several atoms plus one single-atom row when the list has one,
    the properties the list does not contain)."""
    rng = np.random.default_rng(seed)
    props = [row_properties(r, atoms) for r in rows]
    several = [k for k, (_, ncen) in enumerate(props) if ncen >= 2]
    present = set().union(*[props[k][0] for k in several]) if several else set()
    open_, chosen = set(present), []
    while open_ and len(chosen) < MAX_ROWS:
        gain = np.array([len(props[k][0] & open_) for k in several])
        best = np.flatnonzero(gain == gain.max())
        k = several[int(best[rng.integers(len(best))])]
        chosen.append(k)
        open_ -= props[k][0]
    single = [k for k, (_, ncen) in enumerate(props) if ncen == 1]
    one = [single[int(rng.integers(len(single)))]] if single else []
    return chosen, one, [p for p in PROPERTIES if p not in present], sorted(open_)


def class_seed(cls) -> int:
    return 9000 + ((cls[0] * 8 + cls[1]) * 8 + cls[2]) * 8 + cls[3]


def screening_factor(Dt, Da, Db, exx, shell_slices, row):
    """The density factor of the screening bound (header of kern_grad.hip) from block maxima, restated:
        4 |Dt_AB| |Dt_CD| + exx (|Dt_AC| |Dt_BD| + |Dt_AD| |Dt_BC|)                      restricted (Db None)
        4 |Dt_AB| |Dt_CD| + 2 exx sum_spin (|Ds_AC| |Ds_BD| + |Ds_AD| |Ds_BC|)            unrestricted"""
    A, B, C, D = (int(v) for v in row)

    def mx(M, X, Y):
        return float(np.max(np.abs(M[shell_slices[X], shell_slices[Y]])))
    f = 4.0 * mx(Dt, A, B) * mx(Dt, C, D)
    if Db is None:
        return f + abs(exx) * (mx(Dt, A, C) * mx(Dt, B, D) + mx(Dt, A, D) * mx(Dt, B, C))
    for M in (Da, Db):
        f += 2.0 * abs(exx) * (mx(M, A, C) * mx(M, B, D) + mx(M, A, D) * mx(M, B, C))
    return f


# ---- whole-fragment inputs and their finite-difference reference -----------------------------------------------------
SEED_D, SEED_DB, SEED_C, SEED_CB = 101, 102, 103, 104
EXX = (0.0, 0.25, 1.0)
# Step-size disagreement of the finite-difference reference of the whole-fragment two-electron term (Richardson of
# h = 1e-3, 2e-3 against Richardson of 2e-3, 4e-3), relative to the largest gradient component; measured by
# tests/test_gradient_reference.py::test_finite_difference_reference_step_disagreement.  The GPU test allows ten times it.
FD_DISAGREEMENT = 9.4e-11         # measured 9.38e-11 (stretched, unrestricted, exx = 0); the other eleven cases 1.0e-11 .. 4.6e-11


def densities(n: int, unrestricted: bool):
    return symmetric(n, SEED_D), (symmetric(n, SEED_DB) if unrestricted else None)


def whole_fragment_functionals(n: int):
    """[(name, eri -> two-electron energy)] for restricted and unrestricted inputs at every exx of EXX."""
    from tests import gradient_reference as gr
    out = []
    for unrestricted in (False, True):
        D, Db = densities(n, unrestricted)
        for exx in EXX:
            out.append(("%s exx %.2f" % ("UHF" if unrestricted else "RHF", exx),
                        lambda eri, D=D, Db=Db, exx=exx: gr.two_electron_energy(eri, D, Db, exx)))
    return out


def fd_two_electron(mol, functionals, h: float = 1.0e-3, coarse: bool = True):
    """Richardson-extrapolated central differences of functionals (eri -> energy) of the C oracle's tensor with respect
    to every nucleus: the gradients [natoms][3][len(functionals)] from steps (h, 2h) and (coarse) from (2h, 4h), else
    None.  Each displaced tensor is formed once."""
    from oracle import scf_oracle as so
    from tests import gradient_reference as gr
    cache = {}

    def energies(xyz):
        key = np.round(xyz, 9).tobytes()
        if key not in cache:
            eri = so.eri4(gr.moved(mol, xyz))
            cache[key] = np.array([f(eri) for f in functionals])
        return cache[key]
    return gr.richardson_gradient(energies, mol.xyz, h), (gr.richardson_gradient(energies, mol.xyz, 2.0 * h) if coarse else None)
