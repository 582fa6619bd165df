"""numpy reference for the C-PCM solvation model (test infrastructure, never imported by the package).

The model of DESIGN.md section 9, each piece small enough to read against its formula:

  cavity            one sphere per real atom (radius_scale x Bondi radius, or the caller's own radii), a Lebedev rule
                    from oracle.grid_oracle.lebedev on each, tesserae s = R_I + rho_I u_k with areas 4 pi rho_I^2 w_k,
                    kept iff |s - R_J| >= rho_J for every other real atom J; ordered by atom, then by the rule.
  cavity_matrix     S_ii = zeta_i sqrt(2/pi), S_ij = erf(zeta_ij r_ij)/r_ij, zeta_i = 4.90/sqrt(a_i),
                    zeta_ij = zeta_i zeta_j/sqrt(zeta_i^2 + zeta_j^2): the Coulomb Gram matrix of Gaussian-blurred
                    tesserae (York-Karplus), positive definite.
  potential_tensor  A[i] = (mu| 1/|r - s_i| |nu) from oracle.scf_oracle.point_charge_potential with a unit charge.
  Pcm               an `xc` object for run_rhf / run_uhf, wrapping an optional inner functional:
                    v = v_nuc - A.D, q = -f S^-1 v, E_pcm = q.v/2, V_pcm = -sum_i q_i A[i], f = (eps - 1)/eps.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.special import erf

from metalquicha_amd.basis import ANGSTROM_TO_BOHR
from oracle import grid_oracle, scf_oracle

BONDI_ANGSTROM = {1: 1.20, 2: 1.40, 3: 1.82, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 10: 1.54, 11: 2.27, 12: 1.73,
                  14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 18: 1.88}
ZETA = 4.90


def sphere_radii(numbers, ghost=None, radius_scale=1.2, radii_by_z=None):
    """Radius in Bohr of every atom's sphere, 0 for a ghost."""
    rho = []
    for k, z in enumerate(np.asarray(numbers, dtype=int)):
        if ghost is not None and ghost[k]:
            rho.append(0.0)
        elif radii_by_z is not None and radii_by_z.get(int(z), 0.0) != 0.0:
            rho.append(float(radii_by_z[int(z)]))
        elif int(z) in BONDI_ANGSTROM:
            rho.append(radius_scale * BONDI_ANGSTROM[int(z)] * ANGSTROM_TO_BOHR)
        else:
            raise ValueError("no cavity radius for Z = %d" % z)
    return np.array(rho)


def cavity(numbers, xyz_bohr, angular_points=110, ghost=None, radius_scale=1.2, radii_by_z=None):
    """-> (tesserae (T, 3), areas (T,), atom (T,))"""
    xyz = np.asarray(xyz_bohr, dtype=float).reshape(-1, 3)
    rho = sphere_radii(numbers, ghost, radius_scale, radii_by_z)
    u, w = grid_oracle.lebedev(angular_points)
    pts, areas, owner = [], [], []
    for a in range(len(rho)):
        if rho[a] == 0.0:
            continue
        s = xyz[a] + rho[a] * u
        keep = np.ones(len(s), dtype=bool)
        for b in range(len(rho)):
            if b != a and rho[b] != 0.0:
                keep &= np.linalg.norm(s - xyz[b], axis=1) >= rho[b]
        pts.append(s[keep]); areas.append((4.0 * math.pi * rho[a] ** 2 * w)[keep]); owner.append(np.full(int(keep.sum()), a))
    return np.concatenate(pts), np.concatenate(areas), np.concatenate(owner)


def cavity_matrix(tesserae, areas):
    zeta = ZETA / np.sqrt(areas)
    zij = zeta[:, None] * zeta[None, :] / np.sqrt(zeta[:, None] ** 2 + zeta[None, :] ** 2)
    r = np.linalg.norm(tesserae[:, None, :] - tesserae[None, :, :], axis=2)
    np.fill_diagonal(r, 1.0)
    S = erf(zij * r) / r
    np.fill_diagonal(S, zeta * math.sqrt(2.0 / math.pi))
    return S


def potential_tensor(mol, tesserae):
    """A[i, mu, nu] = (mu| 1/|r - s_i| |nu)"""
    return np.stack([-scf_oracle.point_charge_potential(mol, s.reshape(1, 3), [1.0]) for s in tesserae])


def nuclear_potential(mol, tesserae):
    v = np.zeros(len(tesserae))
    for z, R in zip(mol.z, mol.xyz):
        if z != 0.0:
            v += z / np.linalg.norm(tesserae - R, axis=1)
    return v


def pack_pairs(M):
    """(.., n, n) -> (.., npair): pairs mu >= nu at mu (mu + 1) / 2 + nu"""
    i, j = np.tril_indices(M.shape[-1])
    return M[..., i, j]


class Pcm:
    """`xc` object for run_rhf / run_uhf: `inner` (optional) is the functional, whose exx and potentials pass through."""

    def __init__(self, mol, numbers, epsilon=78.39, angular_points=110, ghost=None, radius_scale=1.2, radii_by_z=None, inner=None):
        self.f = (epsilon - 1.0) / epsilon
        self.inner = inner
        self.exx = 1.0 if inner is None else inner.exx
        self.tesserae, self.areas, self.atom = cavity(numbers, mol.xyz, angular_points, ghost, radius_scale, radii_by_z)
        self.S = cavity_matrix(self.tesserae, self.areas)
        self.A = potential_tensor(mol, self.tesserae)
        self.v_nuc = nuclear_potential(mol, self.tesserae)
        self.Sinv = np.linalg.inv(self.S)
        self.e_pcm = 0.0
        self.e_xc = 0.0

    def response(self, D):
        """-> (v, q, E_pcm, V_pcm) for the total density D"""
        v = self.v_nuc - np.einsum("imn,mn->i", self.A, D)
        q = -self.f * np.linalg.solve(self.S, v)
        return v, q, 0.5 * float(q @ v), -np.einsum("i,imn->mn", q, self.A)

    def potential(self, D):
        _, _, e, V = self.response(D)
        self.e_pcm, self.e_xc = e, 0.0
        if self.inner is not None:
            self.e_xc, vxc = self.inner.potential(D)
            V = V + vxc
        return e + self.e_xc, V

    def potential_uks(self, Da, Db):
        _, _, e, V = self.response(Da + Db)
        self.e_pcm, self.e_xc = e, 0.0
        if self.inner is not None:
            self.e_xc, Va, Vb = self.inner.potential_uks(Da, Db)
            return e + self.e_xc, V + Va, V + Vb
        return e, V, V
