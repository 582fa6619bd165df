"""numpy reference for the gradient stage (mqc_hip_gradient_stage): derivatives of the integral blocks the gradient
kernels contract, by COMPLEX-STEP differentiation of the McMurchie-Davidson routines of tests/range_separated_reference.py.

A coordinate x becomes x + i h with h = 1e-30; the derivative is Im f / h, exact to rounding (no subtraction, no step
error).  This shares nothing with the kernels' own route (raise and lower the angular momentum of the differentiated
centre, the fourth centre by translational invariance): here every centre, the fourth included, is moved directly.

  stv_block           S, T, V of one shell pair over solid harmonics; complex centres and complex nuclei allowed
  quartet_block       (ab|cd) of one shell quartet; a slot may hold UNIT, the function 1 (exponent 0, coefficient 1, s)
  d_quartet           [4 slots][3] derivative of sum Gamma_ijkl (ij|kl), with the sum of the magnitudes of its terms
  d_pair              [natoms][3] derivative of sum D (T + V) - W S over one shell pair (both orders of the pair)
  d_three_centre, d_two_centre    the same for (ab|P) and (P|Q) with UNIT in the empty slots
  gamma_block         the two-particle density block of a unique quartet, its degeneracy counted from the definition
  fixed_density_energy            the energy terms at fixed D and W from the C oracle's integrals

Test infrastructure: no GPU needed, never imported by the package."""
from __future__ import annotations

import itertools
import math
from types import SimpleNamespace

import numpy as np

from oracle import scf_oracle as so
from tests import range_separated_reference as rr

STEP = 1.0e-30
UNIT = "unit"          # the function 1 as a shell: one s primitive, exponent 0, coefficient 1, no angular factor


def shell_atoms(mol) -> np.ndarray:
    return np.array([int(np.argmin(np.sum((mol.xyz - c) ** 2, axis=1))) for c in mol.sh_xyz])


def _shell(mol, A):
    """(l, exponents, coefficients, sph <- cart table) of shell A, or of the unit shell."""
    if isinstance(A, str):
        return 0, np.array([0.0]), np.array([1.0]), np.ones((1, 1))
    p0, k = int(mol.sh_poff[A]), int(mol.sh_nprim[A])
    l = int(mol.sh_l[A])
    return l, mol.exps[p0:p0 + k], mol.coefs[p0:p0 + k], rr._c2s(l)


def _pair(sa, ra, sb, rb):
    """rr._Pair of two explicit shells at (possibly complex) centres."""
    mini = SimpleNamespace(sh_l=np.array([sa[0], sb[0]]), sh_xyz=np.array([ra, rb]), exps=np.concatenate([sa[1], sb[1]]),
                           coefs=np.concatenate([sa[2], sb[2]]), sh_poff=np.array([0, len(sa[1])]),
                           sh_nprim=np.array([len(sa[1]), len(sb[1])]))
    return rr._Pair(mini, 0, 1)


def quartet_block(shells, centres):
    """(ab|cd) over solid harmonics [i, j, k, l]; shells = four _shell tuples, centres [4][3] real or complex."""
    pab = _pair(shells[0], centres[0], shells[1], centres[1])
    pcd = _pair(shells[2], centres[2], shells[3], centres[3])
    blk = rr.shell_quartet(None, pab, pcd, None)
    return np.einsum("ia,jb,kc,ld,abcd->ijkl", shells[0][3], shells[1][3], shells[2][3], shells[3][3], blk, optimize=True)


def stv_block(sa, ra, sb, rb, charges, nuclei):
    """S, T, V [i, j] of one shell pair.  T = 1/2 <grad a|grad b> from the derivative of each Cartesian factor,
    d/dx x^i e^{-a x^2} = i x^{i-1} e - 2a x^{i+1} e; V = -sum_C Z_C (a|1/r_C|b) from the Hermite expansion."""
    la, lb = sa[0], sb[0]
    ra, rb = np.asarray(ra), np.asarray(rb)
    a = np.repeat(sa[1], len(sb[1])); b = np.tile(sb[1], len(sa[1]))
    p = a + b
    P = (a[:, None] * ra + b[:, None] * rb) / p[:, None]
    k = np.repeat(sa[2], len(sb[2])) * np.tile(sb[2], len(sa[2])) * np.exp(-a * b / p * np.sum((ra - rb) ** 2))
    E = [rr._e1d(la + 1, lb + 1, P[:, d] - ra[d], P[:, d] - rb[d], 0.5 / p) for d in range(3)]
    root = np.sqrt(math.pi / p)

    def s1(d, i, j):
        return E[d][(i, j, 0)] * root if i >= 0 and j >= 0 else 0.0

    def d1(d, i, j):          # <d/dx x^i e^{-a x^2} | d/dx x^j e^{-b x^2}>
        return (i * j * s1(d, i - 1, j - 1) - 2.0 * b * i * s1(d, i - 1, j + 1) - 2.0 * a * j * s1(d, i + 1, j - 1)
                + 4.0 * a * b * s1(d, i + 1, j + 1))
    ca, cb = rr._cart(la), rr._cart(lb)
    dt = np.result_type(P, np.asarray(nuclei))
    S = np.zeros((len(ca), len(cb)), dtype=dt); T = np.zeros_like(S); V = np.zeros_like(S)
    for ia, (ax, ay, az) in enumerate(ca):
        for ib, (bx, by, bz) in enumerate(cb):
            sx, sy, sz = s1(0, ax, bx), s1(1, ay, by), s1(2, az, bz)
            S[ia, ib] = np.sum(k * sx * sy * sz)
            T[ia, ib] = 0.5 * np.sum(k * (d1(0, ax, bx) * sy * sz + sx * d1(1, ay, by) * sz + sx * sy * d1(2, az, bz)))
    H = rr._herm(la + lb)
    for z, rc in zip(charges, np.asarray(nuclei)):
        if z == 0.0:
            continue
        R = rr.hermite_r(la + lb, p, P[:, 0] - rc[0], P[:, 1] - rc[1], P[:, 2] - rc[2], -z * 2.0 * math.pi / p * k)
        for ia, (ax, ay, az) in enumerate(ca):
            for ib, (bx, by, bz) in enumerate(cb):
                acc = 0.0
                for (t, u, v) in H:
                    if t <= ax + bx and u <= ay + by and v <= az + bz:
                        acc = acc + E[0][(ax, bx, t)] * E[1][(ay, by, u)] * E[2][(az, bz, v)] * R[(t, u, v)]
                V[ia, ib] += np.sum(acc)
    ta, tb = sa[3], sb[3]
    return ta @ S @ tb.T, ta @ T @ tb.T, ta @ V @ tb.T


def int1e(mol, xyz=None):
    """S, T, V [n, n] of the whole basis by stv_block (real coordinates: the check against the C oracle)."""
    xyz = mol.xyz if xyz is None else xyz
    at = shell_atoms(mol)
    nf = 2 * np.asarray(mol.sh_l) + 1
    n = mol.nao
    out = [np.zeros((n, n), dtype=np.asarray(xyz).dtype) for _ in range(3)]
    for A in range(mol.nshell):
        for B in range(A + 1):
            blk = stv_block(_shell(mol, A), xyz[at[A]], _shell(mol, B), xyz[at[B]], mol.z, xyz)
            sa = slice(mol.sh_aoff[A], mol.sh_aoff[A] + nf[A]); sb = slice(mol.sh_aoff[B], mol.sh_aoff[B] + nf[B])
            for o, b in zip(out, blk):
                o[sa, sb] = b
                o[sb, sa] = b.T
    return out


# ---- derivatives ------------------------------------------------------------------------------------------------------
def _step(x, i, d, h=STEP):
    z = np.array(x, dtype=np.complex128)
    z[i, d] += 1j * h
    return z


def d_block(shells, centres):
    """Derivatives of the block with respect to each slot's centre: [4][3][i, j, k, l]."""
    centres = np.asarray(centres, dtype=float)
    return np.array([[quartet_block(shells, _step(centres, s, d)).imag / STEP for d in range(3)] for s in range(4)])


def contract(dblk, G):
    """-> (g [4][3], S): sum G dblk per slot and axis, and the largest of the sums of magnitudes sum |G| |dblk|."""
    g = np.einsum("sdijkl,ijkl->sd", dblk, G)
    mag = np.einsum("sdijkl,ijkl->sd", np.abs(dblk), np.abs(G))
    return g, float(mag.max())


def d_quartet(mol, xyz, row, G):
    """[4 centres][3] derivative of sum_ijkl G_ijkl (ij|kl) over the block of shells row = (A, B, C, D), each slot's centre
    moved on its own (two slots on one atom are two derivatives), and the scale of the comparison."""
    at = shell_atoms(mol)
    return contract(d_block([_shell(mol, X) for X in row], [xyz[at[X]] for X in row]), G)


def d_three_centre_block(mol, aux, xyz, row):
    """(A B|P 1): slots A, B orbital, P auxiliary, the unit shell on P's centre.  [4][3][i, j, k, 1]."""
    A, B, P = row[0], row[1], row[2]
    at, ax = shell_atoms(mol), shell_atoms(aux)
    return d_block([_shell(mol, A), _shell(mol, B), _shell(aux, P), _shell(None, UNIT)], [xyz[at[A]], xyz[at[B]], xyz[ax[P]], xyz[ax[P]]])


def d_two_centre_block(aux, xyz, row):
    """(P 1|Q 1) with row = (P, -, Q, -).  [4][3][i, 1, k, 1]."""
    P, Q = row[0], row[2]
    ax = shell_atoms(aux)
    return d_block([_shell(aux, P), _shell(None, UNIT), _shell(aux, Q), _shell(None, UNIT)], [xyz[ax[P]], xyz[ax[P]], xyz[ax[Q]], xyz[ax[Q]]])


def scatter(g_slots, atoms, natoms):
    """[4][3] per slot -> [natoms][3] per atom."""
    out = np.zeros((natoms, 3))
    for s, a in enumerate(atoms):
        out[a] += g_slots[s]
    return out


def d_pair(mol, xyz, A, B, D, W):
    """[natoms][3] derivative of sum_{mu nu} [D (T + V) - W S] over the functions of shells A and B -- the block (A, B) and,
    when A != B, the block (B, A) too -- with respect to every nucleus (its functions and its charge move together), and
    the largest sum of the magnitudes of the terms."""
    at = shell_atoms(mol)
    nf = 2 * np.asarray(mol.sh_l) + 1
    sa = slice(mol.sh_aoff[A], mol.sh_aoff[A] + nf[A]); sb = slice(mol.sh_aoff[B], mol.sh_aoff[B] + nf[B])
    blocks = [(sa, sb, False)] + ([(sb, sa, True)] if A != B else [])
    g = np.zeros((len(xyz), 3)); mag = np.zeros((len(xyz), 3))
    xyz = np.asarray(xyz, dtype=float)
    for c in range(len(xyz)):
        for d in range(3):
            z = _step(xyz, c, d)
            S, T, V = (m.imag / STEP for m in stv_block(_shell(mol, A), z[at[A]], _shell(mol, B), z[at[B]], mol.z, z))
            for (r, q, tr) in blocks:
                Db, Wb = (D[r, q].T, W[r, q].T) if tr else (D[r, q], W[r, q])
                g[c, d] += np.sum(Db * (T + V) - Wb * S)
                mag[c, d] += np.sum(np.abs(Db) * (np.abs(T) + np.abs(V)) + np.abs(Wb) * np.abs(S))
    return g, float(mag.max())


# ---- the two-particle density ---------------------------------------------------------------------------------------
def gamma_block(mol, D, Db, exx, row):
    """Gamma [i, j, k, l] of the unique shell quartet row = (A, B, C, D) such that the two-electron energy
        E = 1/2 sum_{ijkl} Dt_ij Dt_kl (ij|kl) - 1/2 exx sum_spin sum_{ijkl} Ds_ik Ds_jl (ij|kl)
    (sums over ALL functions, Ds = D/2 per spin when restricted: Db None) is sum over unique quartets of
    Gamma . (AB|CD).  The block (AB|CD) stands for every ordered shell quartet that is an index permutation of it --
    (BA|CD), (AB|DC), (BA|DC) and the four with bra and ket exchanged -- as far as those are DIFFERENT quartets: each
    distinct one contributes its coefficient, brought to the index order of the block."""
    D = np.asarray(D)
    if Db is None:
        Dt, spins = D, [0.5 * D, 0.5 * D]
    else:
        Dt, spins = D + Db, [D, np.asarray(Db)]
    nf = 2 * np.asarray(mol.sh_l) + 1
    sl = [slice(int(mol.sh_aoff[X]), int(mol.sh_aoff[X] + nf[X])) for X in row]
    perms = [(0, 1, 2, 3), (1, 0, 2, 3), (0, 1, 3, 2), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 0, 1), (2, 3, 1, 0), (3, 2, 1, 0)]
    seen = set()
    letters = "ijkl"
    G = 0.0
    for pm in perms:
        shells = tuple(row[k] for k in pm)
        if shells in seen:
            continue
        seen.add(shells)
        s = [sl[k] for k in pm]
        # coefficient of the ordered quartet (s0 s1|s2 s3), indices in ITS order, then back to the block's (i j k l)
        c = 0.5 * np.einsum("ab,cd->abcd", Dt[s[0], s[1]], Dt[s[2], s[3]])
        for Ds in spins:
            c = c - 0.5 * exx * np.einsum("ac,bd->abcd", Ds[s[0], s[2]], Ds[s[1], s[3]])
        src = "".join(letters[k] for k in pm)
        G = G + np.einsum(src + "->ijkl", c)
    return G


def unique_quartets(ns):
    """Every unique shell quartet once: pairs (A >= B) >= (C >= D)."""
    pairs = [(A, B) for A in range(ns) for B in range(A + 1)]
    return [(A, B, C, D) for i, (A, B) in enumerate(pairs) for (C, D) in pairs[:i + 1]]


def two_electron_energy(eri, D, Db, exx):
    """1/2 D.J[D] - 1/4 exx D.K[D] (restricted) or its unrestricted form, J and K from build_jk_incore."""
    if Db is None:
        J, K = so.build_jk_incore(eri, D)
        return 0.5 * float(np.sum(D * J)) - 0.25 * exx * float(np.sum(D * K))
    Dt = D + Db
    J, _ = so.build_jk_incore(eri, Dt)
    _, Ka = so.build_jk_incore(eri, D)
    _, Kb = so.build_jk_incore(eri, Db)
    return 0.5 * float(np.sum(Dt * J)) - 0.5 * exx * (float(np.sum(D * Ka)) + float(np.sum(Db * Kb)))


def fixed_density_energy(mol, D, Db, W, exx):
    """(one-electron, two-electron) energy terms at fixed densities from the C oracle's integrals:
    sum Dt (T + V) - sum W S, and two_electron_energy."""
    S, T, V = so.int1e(mol)
    Dt = D if Db is None else D + Db
    return float(np.sum(Dt * (T + V)) - np.sum(W * S)), two_electron_energy(so.eri4(mol), D, Db, exx)


def moved(mol, xyz):
    """`mol` with its atoms (and their shells) at xyz."""
    import dataclasses
    at = shell_atoms(mol)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    return dataclasses.replace(mol, xyz=xyz, sh_xyz=np.ascontiguousarray(xyz[at]))


def richardson_gradient(f, xyz, h):
    """Central differences of f(xyz) at h and 2h, extrapolated: (4 d(h) - d(2h)) / 3.  f may return an array."""
    xyz = np.asarray(xyz, dtype=float)
    out = None
    for c, d in itertools.product(range(len(xyz)), range(3)):
        def cd(step):
            p = xyz.copy(); p[c, d] += step
            m = xyz.copy(); m[c, d] -= step
            return (np.asarray(f(p)) - np.asarray(f(m))) / (2.0 * step)
        val = (4.0 * cd(h) - cd(2.0 * h)) / 3.0
        if out is None:
            out = np.zeros((len(xyz), 3) + val.shape)
        out[c, d] = val
    return out
