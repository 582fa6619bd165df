"""numpy reference for static dipole polarizabilities of closed-shell Hartree-Fock (test infrastructure, never imported
by the package).

  dipole_integrals   overlap and <a| r_c |b> about the coordinate origin from the Hermite tables of
                     tests/range_separated_reference._Pair: sum_P k (pi/p)^{3/2} [E_{1_c} + P_c E_0] (overlap: E_0 alone),
                     through the oracle's Cartesian -> solid-harmonic tables.
  polarizability     alpha_cd = -d2E / dF_c dF_d with H(F) = H + sum_d F_d r_d: the coupled-perturbed Hartree-Fock
                     equations  Delta o U + G(U) = -b,  b = C_v^T r_d C_o,  G(U) = C_v^T [J(D1) - K(D1)/2] C_o,
                     D1 = 2 (C_v U C_o^T + C_o U^T C_v^T),  alpha_cd = -tr(D1_d r_c),  solved as one dense linear system
                     in the occupied-virtual space from the oracle's four-index integrals and SCF orbitals.
  finite_field       the same tensor by Richardson-extrapolated central differences of -tr(D r_c) under h_extra =
                     +-F r_d, +-2F r_d: what tests/test_cphf_reference.py holds `polarizability` against.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import scf_oracle as so
from tests.range_separated_reference import _Pair, _c2s, _herm


def dipole_integrals(mol):
    """-> S (n, n), R (3, n, n): overlap and electron position integrals about the origin, real solid harmonics."""
    if mol.cart:
        raise ValueError("dipole_integrals: spherical bases only")
    n, ns = mol.nao, mol.nshell
    nf = so.nfun(mol.sh_l, mol.cart)
    T = [_c2s(l) for l in range(int(max(mol.sh_l)) + 1)]
    S, R = np.zeros((n, n)), np.zeros((3, n, n))
    for A in range(ns):
        for B in range(A + 1):
            pr = _Pair(mol, A, B)
            H = _herm(pr.la + pr.lb)
            w = pr.k * (math.pi / pr.p) ** 1.5
            e0 = pr.E[:, :, 0, :]
            ta, tb = T[mol.sh_l[A]], T[mol.sh_l[B]]
            sa = slice(mol.sh_aoff[A], mol.sh_aoff[A] + nf[A]); sb = slice(mol.sh_aoff[B], mol.sh_aoff[B] + nf[B])
            blk = ta @ np.einsum("abp,p->ab", e0, w) @ tb.T
            S[sa, sb] = blk; S[sb, sa] = blk.T
            for c in range(3):
                one = tuple(1 if k == c else 0 for k in range(3))
                e1 = pr.E[:, :, H.index(one), :] if one in H else 0.0
                blk = ta @ np.einsum("abp,p->ab", e1 + pr.P[:, c] * e0, w) @ tb.T
                R[c][sa, sb] = blk; R[c][sb, sa] = blk.T
    return S, R


def cphf_alpha(eri, C, eps, nocc, R):
    """The CPHF tensor from four-index integrals (n, n, n, n), orbitals C (n, nmo), energies and dipole matrices."""
    Co, Cv = C[:, :nocc], C[:, nocc:]
    nv = Cv.shape[1]
    if nv == 0:
        return np.zeros((3, 3)), np.zeros((3, 0, nocc))
    ovov = np.einsum("pqrs,pa,qi,rb,sj->aibj", eri, Cv, Co, Cv, Co, optimize=True)
    vvoo = np.einsum("pqrs,pa,qb,ri,sj->abij", eri, Cv, Cv, Co, Co, optimize=True)
    A = 4.0 * ovov - vvoo.transpose(0, 2, 1, 3) - ovov.transpose(0, 3, 2, 1)
    A = A.reshape(nv * nocc, nv * nocc) + np.diag((eps[nocc:nocc + nv, None] - eps[None, :nocc]).reshape(-1))
    alpha = np.zeros((3, 3))
    U = np.zeros((3, nv, nocc))
    for d in range(3):
        b = Cv.T @ R[d] @ Co
        U[d] = np.linalg.solve(A, -b.reshape(-1)).reshape(nv, nocc)
        X = Cv @ U[d] @ Co.T
        D1 = 2.0 * (X + X.T)
        for c in range(3):
            alpha[c, d] = -np.sum(D1 * R[c])
    return alpha, U


def polarizability(mol, nelec, e_tol=1e-12, d_tol=1e-10, h_extra=None, eri=None, max_iter=200):
    """-> (alpha (3, 3), the oracle's SCF result).  h_extra: a further one-electron operator in the SCF (point charges)."""
    eri = so.eri4(mol) if eri is None else eri
    scf = so.run_rhf(mol, nelec, max_iter, e_tol, d_tol, eri=eri, h_extra=h_extra)
    if not scf.converged:
        raise RuntimeError("cphf_reference: the SCF did not converge")
    _, R = dipole_integrals(mol)
    alpha, _ = cphf_alpha(eri, scf.C, scf.eps, nelec // 2, R)
    return alpha, scf


def finite_field(mol, nelec, F=2e-3, e_tol=1e-13, d_tol=1e-11, eri=None, max_iter=300):
    """alpha_cd = d mu_c / d F_d, mu_c = -tr(D r_c), by the five-point (Richardson) central difference with steps F, 2F."""
    eri = so.eri4(mol) if eri is None else eri
    _, R = dipole_integrals(mol)

    def mu(h):
        scf = so.run_rhf(mol, nelec, max_iter, e_tol, d_tol, eri=eri, h_extra=h)
        if not scf.converged:
            raise RuntimeError("cphf_reference: a finite-field SCF did not converge")
        return -np.einsum("cmn,mn->c", R, scf.D)

    alpha = np.zeros((3, 3))
    for d in range(3):
        m1, p1, m2, p2 = mu(-F * R[d]), mu(F * R[d]), mu(-2 * F * R[d]), mu(2 * F * R[d])
        alpha[:, d] = (8.0 * (p1 - m1) - (p2 - m2)) / (12.0 * F)
    return alpha
