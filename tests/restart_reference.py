"""CPU reference of the restart from a supplied density (mqc_hip_scf_run_batch_restart), in numpy on the oracle's
integrals and helpers; no GPU.  The oracle itself is not edited.

project_density(S, X, D0, nocc): the natural orbitals of D0 in the metric S are the eigenvectors of the generalised
problem F_r C = S C eps with F_r = -S D0s S, D0s = (D0 + D0^T) / 2, and the eigenvalues are minus the occupations, so
the lowest nocc pairs are the most occupied orbitals; their density is idempotent in S and carries the right electron
count whatever D0 was.  The drivers start the oracle's own SCF loops from it."""
import contextlib
import math

import numpy as np

from oracle import scf_oracle as so


def restart_fock(S, D0):
    D0 = np.asarray(D0, dtype=float)
    return -S @ (0.5 * (D0 + D0.T)) @ S


def project_orbitals(S, X, D0):
    """-> (C, minus the occupations, ascending)."""
    return so.diagonalize(restart_fock(S, D0), X)


def project_density(S, X, D0, nocc, spin=False):
    """The restricted density 2 C_occ C_occ^T of the nocc most occupied natural orbitals of D0 (spin: C_occ C_occ^T)."""
    C, _ = project_orbitals(S, X, D0)
    if spin:
        return C[:, :nocc] @ C[:, :nocc].T
    return so.density_closed_shell(C, nocc)


@contextlib.contextmanager
def starting_from(D0):
    """Inside, the oracle's GWH starting Fock is -S D0s S: run_rhf(..., guess="gwh") then starts from D0's projection."""
    keep = so.guess_fock_gwh
    so.guess_fock_gwh = lambda S, H: restart_fock(S, D0)
    try:
        yield
    finally:
        so.guess_fock_gwh = keep


def run_rhf_restart(mol, nelec, D0, **kw):
    """scf_oracle.run_rhf (same keywords) started from the total density D0."""
    kw["guess"] = "gwh"
    with starting_from(D0):
        return so.run_rhf(mol, nelec, **kw)


def run_uhf_restart(mol, nelec, multiplicity, Da0, Db0, max_iter=100, e_tol=1e-8, d_tol=1e-6, diis_vectors=8):
    """Unrestricted Hartree-Fock started from the spin densities Da0, Db0, each projected with its own occupation.
    scf_oracle.run_uhf gives both spins the orbitals of ONE starting Fock, which a restart cannot do, so its loop is
    repeated here on the oracle's pieces (same DIIS over both spins from iteration UHF_DIIS_START, same convergence
    test, final rebuild).  -> scf_oracle.UhfResult."""
    na = (nelec + multiplicity - 1) // 2
    nb = nelec - na
    S, T, V = so.int1e(mol)
    H = T + V
    n = mol.nao
    eri = so.eri4(mol)
    X = so.build_orthogonalizer(S)
    m = X.shape[1]

    def assemble(Da, Db):
        J = np.einsum("ijkl,kl->ij", eri, Da + Db, optimize=True)
        Fa = H + J - np.einsum("ikjl,kl->ij", eri, Da, optimize=True)
        Fb = H + J - np.einsum("ikjl,kl->ij", eri, Db, optimize=True)
        return Fa, Fb, 0.5 * float(np.sum(Da * (H + Fa)) + np.sum(Db * (H + Fb)))

    Ca, ea = project_orbitals(S, X, Da0)
    Cb, eb = project_orbitals(S, X, Db0)
    Da = Ca[:, :na] @ Ca[:, :na].T
    Db = Cb[:, :nb] @ Cb[:, :nb].T
    diis = so.Diis(diis_vectors, 2 * n * n, 2 * m * m)
    e_old, converged, iters = 0.0, False, 0
    for it in range(1, max_iter + 1):
        Da_old, Db_old = Da.copy(), Db.copy()
        Fa, Fb, e_elec = assemble(Da, Db)
        ff = np.concatenate([Fa.reshape(-1), Fb.reshape(-1)])
        diis.push(ff, np.concatenate([so.commutator(Fa, Da, S, X).reshape(-1), so.commutator(Fb, Db, S, X).reshape(-1)]))
        if it >= so.UHF_DIIS_START:
            ex, ok = diis.extrapolate(ff)
            if ok:
                Fa, Fb = ex[: n * n].reshape(n, n), ex[n * n:].reshape(n, n)
        Ca, ea = so.diagonalize(Fa, X)
        Cb, eb = so.diagonalize(Fb, X)
        Da = Ca[:, :na] @ Ca[:, :na].T
        Db = Cb[:, :nb] @ Cb[:, :nb].T
        de = abs(e_elec - e_old)
        drms = math.sqrt((float(np.sum((Da - Da_old) ** 2)) + float(np.sum((Db - Db_old) ** 2))) / (2 * n * n))
        e_old, iters = e_elec, it
        if it > 1 and de < e_tol and drms < d_tol:
            converged = True
            break
    _, _, e_final = assemble(Da, Db)
    enuc = so.nuclear_repulsion(mol)
    return so.UhfResult(e_final + enuc, e_final, enuc, converged, iters, ea, eb, Ca, Cb, Da, Db,
                        so.spin_contamination(Ca, Cb, S, na, nb), na, nb)


def block_diagonal(blocks):
    n = sum(b.shape[0] for b in blocks)
    out = np.zeros((n, n))
    at = 0
    for b in blocks:
        out[at:at + b.shape[0], at:at + b.shape[0]] = b
        at += b.shape[0]
    return out
