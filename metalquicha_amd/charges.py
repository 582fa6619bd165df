"""Potential-fitted atomic charges (CHELPG) on top of the engine's electrostatic potential.

  chelpg_grid     Breneman & Wiberg's point selection (J. Comput. Chem. 11, 361 (1990)): a cubic lattice over the
                  molecule's bounding box plus a padding, without the points inside any atom's van der Waals radius and
                  without those farther than the padding from every atom
  fit_charges     least-squares fit of atom-centred charges to a potential, total charge held by a constraint
  chelpg_charges  the two joined through `methods.run_hip_esp`: ONE engine call per element sequence

These are the PUBLISHED CHELPG defaults (0.3 Angstrom spacing, 2.8 Angstrom padding) with the van der Waals radii the
FMO driver already uses (`fmo.VDW_ANGSTROM`).  The reference's own CHELPG variant (its radii, lattice origin and
selection rules) has not been compared with: parity with it is NOT claimed, only self-consistency with the potential
of the density the charges are fitted to.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .basis import ANGSTROM_TO_BOHR
from .fmo import VDW_ANGSTROM
from .methods import FragmentGroup, ScfSettings


def chelpg_grid(z, xyz_bohr, spacing: float = 0.3, padding: float = 2.8, radii: Sequence[float] = VDW_ANGSTROM,
                ghost=None) -> np.ndarray:
    """-> (n_points, 3) Bohr.  `spacing`, `padding` and `radii` (indexed by Z - 1) are in Angstrom.  The lattice is
    centred on the real atoms' bounding box (box + padding on every side, as many whole steps as fit), so a translated
    molecule gives the translated grid and a mirror plane of the box is one of the lattice: symmetry-equivalent atoms
    of such a molecule get equal charges.  Ghost atoms take no part: they exclude no point, keep none and do not widen the box."""
    z = np.asarray(z, dtype=np.int64)
    xyz = np.asarray(xyz_bohr, dtype=np.float64).reshape(-1, 3)
    if len(z) != len(xyz):
        raise ValueError("chelpg_grid: one atomic number per atom")
    if not (spacing > 0.0 and padding > 0.0):
        raise ValueError("chelpg_grid: spacing and padding must be positive")
    real = np.ones(len(z), dtype=bool) if ghost is None else ~np.asarray(ghost, dtype=bool)
    if not np.any(real):
        return np.zeros((0, 3))
    if int(np.max(z[real])) > len(radii) or int(np.min(z[real])) < 1:
        raise ValueError("chelpg_grid: no van der Waals radius tabulated for an element of the molecule")
    at = xyz[real]
    r_atom = np.array([radii[int(v) - 1] for v in z[real]]) * ANGSTROM_TO_BOHR
    h, pad = spacing * ANGSTROM_TO_BOHR, padding * ANGSTROM_TO_BOHR
    extent = at.max(axis=0) - at.min(axis=0) + 2.0 * pad
    counts = np.floor(extent / h + 1.0e-9).astype(np.int64) + 1
    lo = 0.5 * (at.max(axis=0) + at.min(axis=0)) - 0.5 * h * (counts - 1)      # centred: mirror planes of the box are the lattice's
    axes = [lo[k] + h * np.arange(counts[k]) for k in range(3)]
    keep: List[np.ndarray] = []
    for x in axes[0]:                          # one lattice plane at a time bounds the distance table
        plane = np.stack(np.meshgrid([x], axes[1], axes[2], indexing="ij"), axis=-1).reshape(-1, 3)
        d = np.linalg.norm(plane[:, None, :] - at[None, :, :], axis=2)
        ok = np.all(d >= r_atom[None, :], axis=1) & (np.min(d, axis=1) <= pad)
        keep.append(plane[ok])
    return np.concatenate(keep, axis=0)


def fit_charges(points, esp, centres, total_charge: float) -> np.ndarray:
    """Charges q_A at `centres` (n, 3) minimising sum_i (V_i - sum_A q_A / |r_i - R_A|)^2 under sum_A q_A =
    total_charge -- the stationary point of the Lagrangian of Breneman & Wiberg's fit.  The constraint is eliminated
    (q = total/n + N y with N an orthonormal basis of the charge-conserving directions) and the remaining n - 1 unknowns
    come from an SVD least-squares solve of the design matrix itself, which is the same solution as the n + 1 normal
    equations with the multiplier but without squaring their condition number."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(esp, dtype=np.float64).reshape(-1)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    n = len(c)
    if len(v) != len(pts):
        raise ValueError("fit_charges: one potential value per point")
    if n == 0:
        return np.zeros(0)
    if len(pts) < n:
        raise ValueError("fit_charges: fewer points than charges")
    a = 1.0 / np.linalg.norm(pts[:, None, :] - c[None, :, :], axis=2)        # (points, n)
    q0 = np.full(n, float(total_charge) / n)
    if n == 1:
        return q0
    # orthonormal complement of (1, ..., 1): the last n - 1 columns of a Householder reflection
    e = np.zeros(n); e[0] = 1.0
    w = np.ones(n) / np.sqrt(n) + e
    hh = np.eye(n) - 2.0 * np.outer(w, w) / float(w @ w)
    basis = hh[:, 1:]
    y = np.linalg.lstsq(a @ basis, v - a @ q0, rcond=None)[0]
    q = q0 + basis @ y
    return q + (float(total_charge) - float(np.sum(q))) / n          # the sum to the last bit the additions allow


def chelpg_charges(settings: ScfSettings, groups: Sequence[FragmentGroup], densities: Sequence[np.ndarray],
                   spacing: float = 0.3, padding: float = 2.8, radii: Sequence[float] = VDW_ANGSTROM,
                   esp: Optional[Callable] = None) -> List[np.ndarray]:
    """CHELPG charges of every fragment of every group: per group (= element sequence) the grids of its fragments are
    padded to a common length and their potentials come from ONE `run_hip_esp` call.  densities[g] is (m_g, n_ao, n_ao);
    the total charge of a fragment is the group's `charge`.  -> per group (m_g, n_atoms); ghost atoms get 0.

    `esp(group, densities, points, n_points) -> (m, max_points)` replaces the engine (the tests fit the oracle's
    potential through the very same grid and solve).  Published CHELPG defaults; see the module docstring for what is
    not claimed."""
    if esp is None:
        from .methods import run_hip_esp

        def esp(group, dens, pts, counts):
            return run_hip_esp(settings, group, dens, pts, counts, include_nuclei=True)
    out = []
    for g, dens in zip(groups, densities):
        xyz = np.asarray(g.xyz, dtype=np.float64)
        m, na = xyz.shape[0], xyz.shape[1]
        real = np.ones(na, dtype=bool) if g.ghost is None else ~np.asarray(g.ghost, dtype=bool)
        grids = [chelpg_grid(g.element_numbers, xyz[f], spacing, padding, radii, g.ghost) for f in range(m)]
        counts = np.array([len(p) for p in grids], dtype=np.int32)
        q = np.zeros((m, na))
        if m and int(counts.max(initial=0)) > 0:
            pts = np.zeros((m, int(counts.max()), 3))
            for f, p in enumerate(grids):
                pts[f, :len(p)] = p
            v = esp(g, np.asarray(dens, dtype=np.float64), pts, counts)
            charge = np.broadcast_to(np.asarray(g.charge, dtype=np.float64), (m,))
            for f in range(m):
                q[f, real] = fit_charges(grids[f], v[f, :counts[f]], xyz[f][real], float(charge[f]))
        out.append(q)
    return out


ChargeRequest = Tuple[Sequence[int], np.ndarray]                      # (atoms of a fragment, its density)


def hip_chelpg_charges(system, settings: ScfSettings, spacing: float = 0.3, padding: float = 2.8,
                       radii: Sequence[float] = VDW_ANGSTROM, esp: Optional[Callable] = None):
    """The `charges=` callable of `fmo.run_fmo2` backed by the engine: all fragments of a pass at once, grouped by
    element sequence (one `run_hip_esp` call each); neutral closed-shell fragments, as everywhere in the FMO driver."""
    coords = np.ascontiguousarray(system.coordinates.T)
    z_all = np.asarray(system.element_numbers)

    def charges(requests: Sequence[ChargeRequest]) -> List[np.ndarray]:
        by_key: Dict[tuple, List[int]] = {}
        for r, (atoms, _) in enumerate(requests):
            by_key.setdefault(tuple(int(v) for v in z_all[list(atoms)]), []).append(r)
        groups, dens = [], []
        for zseq, rs in by_key.items():
            groups.append(FragmentGroup(np.array(zseq, dtype=np.int32), np.stack([coords[list(requests[r][0])] for r in rs]),
                                        np.zeros(len(rs), dtype=np.int32)))
            dens.append(np.stack([requests[r][1] for r in rs]))
        out: List[Optional[np.ndarray]] = [None] * len(requests)
        for rs, q in zip(by_key.values(), chelpg_charges(settings, groups, dens, spacing, padding, radii, esp)):
            for pos, r in enumerate(rs):
                out[r] = q[pos]
        return out      # type: ignore[return-value]

    return charges
