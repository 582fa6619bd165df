"""CPU reference of the engine's RI-MP2 stage (mqc_hip_rimp2_batch; kern_mp2.hip), in numpy on the oracle:

    C, eps   so.run_rhf(mol, nelec, 200, 1e-12, 1e-10, aux=aux)     the density-fitted closed-shell SCF
    B        so.df_tensor(mol, aux)                                  (mu nu|Q) J^-1/2, shape (n, n, A)
    Bia      einsum("mi,mnP,na->iaP")   over active occupied i and virtual a
    V        einsum("iaP,jbP->iajb")    = (ia|jb)
    e_os     sum V^2 / D,    e_ss = sum V (V - V.transpose(0, 3, 2, 1)) / D,    D = e_i + e_j - e_a - e_b

Not the reference code's own MP2, which is conventional (exact four-centre integrals); its manifest rows are not
harvested.  Water at wc.DF_GRAD_XYZ, cc-pVDZ, wc.AUX, frozen core (no = 4, nv = 19, naux = 126):
e_os = -0.153174310268, e_ss = -0.051324351783.
"""
import functools

import numpy as np

from metalquicha_amd.methods import frozen_core_count
from oracle import scf_oracle as so
from tests.helpers import oracle_mol


def pair_energies(B, C, eps, nocc, n_frozen=0):
    """(e_os, e_ss) from a fitted tensor B (n, n, A), orbitals C (n, nmo) and their energies."""
    Co, Cv = C[:, n_frozen:nocc], C[:, nocc:]
    eo, ev = eps[n_frozen:nocc], eps[nocc:C.shape[1]]
    Bia = np.einsum("mi,mnP,na->iaP", Co, B, Cv, optimize=True)
    V = np.einsum("iaP,jbP->iajb", Bia, Bia, optimize=True)
    D = eo[:, None, None, None] + eo[None, None, :, None] - ev[None, :, None, None] - ev[None, None, None, :]
    e_os = float(np.sum(V * V / D))
    e_ss = float(np.sum(V * (V - V.transpose(0, 3, 2, 1)) / D))
    return e_os, e_ss


def conventional_mp2(eri, C, eps, nocc, n_frozen=0):
    """(e_os, e_ss) from the exact four-centre integrals (mu nu|la si)."""
    Co, Cv = C[:, n_frozen:nocc], C[:, nocc:]
    eo, ev = eps[n_frozen:nocc], eps[nocc:C.shape[1]]
    V = np.einsum("mi,na,mnls,lj,sb->iajb", Co, Cv, eri, Co, Cv, optimize=True)
    D = eo[:, None, None, None] + eo[None, None, :, None] - ev[None, :, None, None] - ev[None, None, None, :]
    return float(np.sum(V * V / D)), float(np.sum(V * (V - V.transpose(0, 3, 2, 1)) / D))


def cholesky_df_tensor(mol, aux):
    """B = (mu nu|Q) L^-T with J = L L^T: the square root of the metric the engine fits with."""
    j3 = so.eri3c(mol, aux)
    L = np.linalg.cholesky(so.eri2c(aux))
    return np.linalg.solve(L, j3.reshape(-1, j3.shape[2]).T).T.reshape(j3.shape)


def rimp2(frag, basis, aux_basis, frozen_core=True, h_extra=None):
    """-> dict(scf, e_os, e_ss, no, nv, naux) of one fragment: the oracle's DF-RHF, then the pair energies."""
    mol, aux = oracle_mol(basis, frag), oracle_mol(aux_basis, frag)
    B = so.df_tensor(mol, aux)
    o = so.run_rhf(mol, int(frag.nelec), 200, 1e-12, 1e-10, aux=aux, B=B, h_extra=h_extra)
    assert o.converged
    nocc = int(frag.nelec) // 2
    nfz = frozen_core_count(frag.element_numbers, frag.ghost) if frozen_core else 0
    e_os, e_ss = pair_energies(B, o.C, o.eps, nocc, nfz)
    return {"scf": o.energy, "e_os": e_os, "e_ss": e_ss, "no": nocc - nfz, "nv": o.C.shape[1] - nocc, "naux": B.shape[2]}


@functools.lru_cache(maxsize=None)
def _cached(key, z, xyz, basis, aux_basis, frozen_core):
    from tests.helpers import fragment_bohr
    return rimp2(fragment_bohr(list(z), np.array(xyz).reshape(-1, 3)), basis, aux_basis, frozen_core)


def rimp2_cached(frag, basis, aux_basis, frozen_core=True):
    """rimp2 of a neutral singlet fragment without ghosts, computed once per process and shared between the tests."""
    xyz = tuple(np.asarray(frag.coordinates.T, dtype=float).reshape(-1).tolist())
    return dict(_cached("rimp2", tuple(int(v) for v in frag.element_numbers), xyz, basis, aux_basis, bool(frozen_core)))
