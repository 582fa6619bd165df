"""numpy reference for the range-separated hybrid wB97X (test infrastructure, never imported by the package).

Three pieces, each small enough to read against its formula:

  eri4_erf          erf(omega r12)/r12 four-centre integrals by McMurchie-Davidson.  The Hermite expansion of every
                    primitive quartet is the Coulomb one; only the Hermite-Coulomb tables change, the reduced exponent
                    alpha = pq/(p+q) becoming alpha_w = alpha w^2/(alpha + w^2) and the prefactor gaining
                    sqrt(alpha_w/alpha).  Boys function from scipy.special, the solid-harmonic tables from the oracle.
  wb97x_pol         the semi-local part of wB97X in libxc's form (gga_xc_wb97, Chai & Head-Gordon 2008), per point,
                    with first derivatives by the oracle's dual numbers.
  WB97X             an `xc` object for oracle.scf_oracle.run_rhf / run_uhf: E_xc - 1/4 exx_lr tr(D K_lr) and
                    v_xc - 1/2 exx_lr K_lr (restricted), the per-spin forms for unrestricted.

Parameters are libxc's (cam_alpha = 1, cam_beta = -0.842294): omega = 0.3, exx = 0.157706, exx_lr = 0.842294.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
from scipy import special

from oracle import grid_oracle, scf_oracle
from oracle.xc_oracle import DENS_THRESHOLD, SPIN_FLOOR, DualN, _pw_mod_g, _zeta_f, nexp

WB97X_OMEGA = 0.3
WB97X_EXX = 0.157706
WB97X_EXX_LR = 0.842294
C_X = (0.842294, 0.726479, 1.04760, -5.70635, 13.2794)
C_SS = (1.0, -4.33879, 18.2308, -31.7430, 17.2901)
C_AB = (1.0, 2.37031, -11.3995, 6.58405, -3.78132)
GAMMA_X, GAMMA_SS, GAMMA_AB = 0.004, 0.2, 0.006
PW_FZ20 = 1.709921          # f''(0) as the original PW92 parameter set rounds it


# ------------------------------------------------------------------ attenuated integrals
def boys(nmax: int, T: np.ndarray) -> np.ndarray:
    """F_0..F_nmax(T) -> [nmax+1, ...]; the closed form through the regularised incomplete gamma function, a short
    Taylor series near T = 0.  A complex T = T0 + i eps (complex-step differentiation, eps ~ 1e-30) takes the first
    order of its Taylor series, F_n(T0) - i eps F_{n+1}(T0), which is all such a step sees."""
    if np.iscomplexobj(T):
        T = np.asarray(T)
        F = boys(nmax + 1, T.real)
        return F[:-1] - 1j * T.imag * F[1:]
    T = np.asarray(T, dtype=np.float64)
    out = np.empty((nmax + 1,) + T.shape)
    small = T < 1e-3
    Ts = np.where(small, 1.0, T)
    for n in range(nmax + 1):
        a = n + 0.5
        big = special.gamma(a) * special.gammainc(a, Ts) / (2.0 * Ts ** a)
        ser = sum((-T) ** k / (math.factorial(k) * (2 * n + 2 * k + 1)) for k in range(8))
        out[n] = np.where(small, ser, big)
    return out


def _cart(l):
    return [(lx, ly, l - lx - ly) for lx in range(l, -1, -1) for ly in range(l - lx, -1, -1)]


def _herm(L):
    return [(t, u, v) for N in range(L + 1) for t in range(N, -1, -1) for u in range(N - t, -1, -1) for v in [N - t - u]]


def hermite_r(L, alpha, X, Y, Z, scale):
    """R_tuv(alpha, PQ) for t+u+v <= L as a dict (t, u, v) -> array, R^n_000 = scale (-2 alpha)^n F_n."""
    F = boys(L, alpha * (X * X + Y * Y + Z * Z))
    memo = {}

    def r(n, t, u, v):
        key = (n, t, u, v)
        if key in memo:
            return memo[key]
        if t < 0 or u < 0 or v < 0:
            val = 0.0
        elif t == u == v == 0:
            val = scale * (-2.0 * alpha) ** n * F[n]
        elif t > 0:
            val = (t - 1) * r(n + 1, t - 2, u, v) + X * r(n + 1, t - 1, u, v)
        elif u > 0:
            val = (u - 1) * r(n + 1, t, u - 2, v) + Y * r(n + 1, t, u - 1, v)
        else:
            val = (v - 1) * r(n + 1, t, u, v - 2) + Z * r(n + 1, t, u, v - 1)
        memo[key] = val
        return val

    return {h: r(0, *h) for h in _herm(L)}


def _e1d(la, lb, xpa, xpb, hp):
    """E[i][j][t] arrays (E^00_0 = 1; the Gaussian product factor is kept apart)."""
    E = {(0, 0, 0): np.ones_like(xpa)}

    def g(i, j, t):
        return E.get((i, j, t), 0.0)
    for i in range(la + 1):
        for j in range(lb + 1):
            if i == 0 and j == 0:
                continue
            for t in range(i + j + 1):
                if i > 0:
                    E[(i, j, t)] = hp * g(i - 1, j, t - 1) + xpa * g(i - 1, j, t) + (t + 1) * g(i - 1, j, t + 1)
                else:
                    E[(i, j, t)] = hp * g(i, j - 1, t - 1) + xpb * g(i, j - 1, t) + (t + 1) * g(i, j - 1, t + 1)
    return E


class _Pair:
    """Primitive pairs of a shell pair and their Cartesian Hermite tables E[ca, cb, h, P]."""

    def __init__(self, mol, A, B):
        la, lb = int(mol.sh_l[A]), int(mol.sh_l[B])
        ra, rb = mol.sh_xyz[A], mol.sh_xyz[B]
        ea = mol.exps[mol.sh_poff[A]: mol.sh_poff[A] + mol.sh_nprim[A]]
        eb = mol.exps[mol.sh_poff[B]: mol.sh_poff[B] + mol.sh_nprim[B]]
        ca = mol.coefs[mol.sh_poff[A]: mol.sh_poff[A] + mol.sh_nprim[A]]
        cb = mol.coefs[mol.sh_poff[B]: mol.sh_poff[B] + mol.sh_nprim[B]]
        a = np.repeat(ea, len(eb)); b = np.tile(eb, len(ea))
        p = a + b
        P = (a[:, None] * ra + b[:, None] * rb) / p[:, None]
        mu = a * b / p
        self.p, self.P = p, P
        self.k = np.repeat(ca, len(eb)) * np.tile(cb, len(ea)) * np.exp(-mu * np.sum((ra - rb) ** 2))
        self.la, self.lb = la, lb
        E = [_e1d(la, lb, P[:, d] - ra[d], P[:, d] - rb[d], 0.5 / p) for d in range(3)]
        H = _herm(la + lb)
        self.E = np.zeros((len(_cart(la)), len(_cart(lb)), len(H), len(p)), dtype=P.dtype)      # complex centres: complex tables
        for ia, (ax, ay, az) in enumerate(_cart(la)):
            for ib, (bx, by, bz) in enumerate(_cart(lb)):
                for ih, (t, u, v) in enumerate(H):
                    if t <= ax + bx and u <= ay + by and v <= az + bz:
                        self.E[ia, ib, ih] = E[0][(ax, bx, t)] * E[1][(ay, by, u)] * E[2][(az, bz, v)]


def _c2s(l):
    """The oracle's Cartesian -> real solid harmonic table (libcint's, angular normalisation included)."""
    nc = (l + 1) * (l + 2) // 2
    m = np.zeros((2 * l + 1, nc))
    scf_oracle.lib().orc_c2s(l, scf_oracle._dp(m))
    return m


def shell_quartet(mol, pab: _Pair, pcd: _Pair, omega2: float | None):
    """Cartesian block [ca, cb, cc, cd] of (ab|cd) with 1/r (omega2 None) or erf(omega r)/r."""
    p, q = pab.p[:, None], pcd.p[None, :]
    PQ = pab.P[:, None, :] - pcd.P[None, :, :]
    alpha = p * q / (p + q)
    pref = 2.0 * math.pi ** 2.5 / (p * q * np.sqrt(p + q)) * pab.k[:, None] * pcd.k[None, :]
    scale = 1.0
    if omega2 is not None:
        scale = np.sqrt(omega2 / (alpha + omega2))
        alpha = alpha * omega2 / (alpha + omega2)
    L1, L2 = pab.la + pab.lb, pcd.la + pcd.lb
    R = hermite_r(L1 + L2, alpha, PQ[..., 0], PQ[..., 1], PQ[..., 2], scale * pref)
    H1, H2 = _herm(L1), _herm(L2)
    Rt = np.empty((len(H1), len(H2)) + alpha.shape, dtype=np.result_type(PQ, pref))
    for i, (t, u, v) in enumerate(H1):
        for j, (tt, uu, vv) in enumerate(H2):
            Rt[i, j] = (-1) ** (tt + uu + vv) * R[(t + tt, u + uu, v + vv)]
    G = np.einsum("cdkq,hkpq->cdhp", pcd.E, Rt)
    return np.einsum("abhp,cdhp->abcd", pab.E, G)


def eri4_erf(mol, omega: float | None) -> np.ndarray:
    """(ij|kl) [n, n, n, n] with erf(omega r12)/r12 over real solid harmonics; omega None is the plain Coulomb
    operator."""
    if mol.cart:
        raise ValueError("eri4_erf: spherical bases only")
    ns = mol.nshell
    omega2 = None if omega is None else omega * omega
    nf = scf_oracle.nfun(mol.sh_l, mol.cart)
    T = [_c2s(l) for l in range(int(max(mol.sh_l)) + 1)]
    pairs = {(A, B): _Pair(mol, A, B) for A in range(ns) for B in range(A + 1)}
    n = mol.nao
    out = np.zeros((n, n, n, n))
    keys = sorted(pairs)
    for i1, (A, B) in enumerate(keys):
        for (C, D) in keys[: i1 + 1]:
            blk = shell_quartet(mol, pairs[(A, B)], pairs[(C, D)], omega2)
            blk = np.einsum("ia,jb,kc,ld,abcd->ijkl", T[mol.sh_l[A]], T[mol.sh_l[B]], T[mol.sh_l[C]], T[mol.sh_l[D]], blk,
                            optimize=True)
            sa, sb, sc, sd = (slice(mol.sh_aoff[X], mol.sh_aoff[X] + nf[X]) for X in (A, B, C, D))
            for (s1, s2, s3, s4, b) in ((sa, sb, sc, sd, blk), (sb, sa, sc, sd, blk.transpose(1, 0, 2, 3))):
                out[s1, s2, s3, s4] = b
                out[s1, s2, s4, s3] = b.transpose(0, 1, 3, 2)
                out[s3, s4, s1, s2] = b.transpose(2, 3, 0, 1)
                out[s4, s3, s1, s2] = b.transpose(3, 2, 0, 1)
    return out


# ------------------------------------------------------------------ wB97X semi-local part
# F(a) = 1 - 8/3 a [sqrt(pi) erf(1/(2a)) + (2a - 4a^3) exp(-1/(4a^2)) - 3a + 4a^3] loses all its digits for large a (the
# bracket cancels to O(1/a^3)).  There it is the series sum_k (-1)^(k+1) b^(2k) / d_k in b = 1/(2a), ten terms, taken
# for a >= 1: the first omitted term is below 1e-16 of the sum, the closed form keeps ~1e-13 relative below a = 1.
ATT_ERF_SERIES_A = 1.0
ATT_ERF_SERIES_D = (9.0, 60.0, 420.0, 3240.0, 27720.0, 262080.0, 2721600.0, 30844800.0, 379209600.0, 5029516800.0)


def attenuation_erf(a: DualN) -> DualN:
    big = a.v >= ATT_ERF_SERIES_A
    # each branch sees a harmless stand-in on the points of the other one; np.where then picks per point
    sa = DualN(np.where(big, a.v, 2.0), [np.where(big, x, 0.0) for x in a.d])
    b2 = (0.5 / sa) * (0.5 / sa)
    ser = 0.0
    pw = b2
    for k, d in enumerate(ATT_ERF_SERIES_D):
        ser = ser + ((1.0 if k % 2 == 0 else -1.0) / d) * pw
        pw = pw * b2
    ca = DualN(np.where(big, 0.5, a.v), [np.where(big, 0.0, x) for x in a.d])
    b = 0.5 / ca
    erfb = b.chain(special.erf(b.v), 2.0 / math.sqrt(math.pi) * np.exp(-b.v * b.v))
    a3 = ca * ca * ca
    closed = 1.0 - (8.0 / 3.0) * ca * (math.sqrt(math.pi) * erfb + (2.0 * ca - 4.0 * a3) * nexp(-1.0 * b * b)
                                        - 3.0 * ca + 4.0 * a3)
    return DualN(np.where(big, ser.v, closed.v), [np.where(big, s, c) for s, c in zip(ser.d, closed.d)])


def _b97_g(gamma, c, x2):
    u = gamma * x2 / (1.0 + gamma * x2)
    g = c[-1]
    for ci in reversed(c[:-1]):
        g = g * u + ci
    return g


def _pw_pol(rs, z):
    """PW92 with its original parameters (libxc's lda_c_pw, which gga_xc_wb97 uses; PBE uses lda_c_pw_mod)."""
    g0 = _pw_mod_g(rs, 0.031091, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294)
    g1 = _pw_mod_g(rs, 0.015545, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517)
    g2 = _pw_mod_g(rs, 0.016887, 0.11125, 10.357, 3.6231, 0.88026, 0.49671)       # = -alpha_c
    f = _zeta_f(z)
    z4 = z * z * z * z
    return g0 - g2 * f * (1.0 - z4) / PW_FZ20 + (g1 - g0) * f * z4


def _pw_spin(rho_s):
    """rho_s eps_c^PW(rho_s, 0): the fully polarised local correlation per volume."""
    rs = (3.0 / (4.0 * math.pi)) ** (1.0 / 3.0) * rho_s ** (-1.0 / 3.0)
    return rho_s * _pw_pol(rs, DualN(np.ones_like(rho_s.v), [np.zeros_like(rho_s.v) for _ in rho_s.d]))


def wb97x_pol(ra, rb, saa, sab, sbb, omega=WB97X_OMEGA):
    """f per volume of the semi-local part, dual numbers in (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb)."""
    del sab
    f = 0.0
    x2 = []
    for r, s in ((ra, saa), (rb, sbb)):
        r13 = r ** (1.0 / 3.0)
        x2s = s / (r13 * r13 * r * r)                         # sigma_ss / rho_s^(8/3)
        x2.append(x2s)
        kf = (6.0 * math.pi ** 2) ** (1.0 / 3.0) * r13
        ex_lda = -0.75 * (6.0 / math.pi) ** (1.0 / 3.0) * r13 * r
        f = f + ex_lda * attenuation_erf(omega / (2.0 * kf)) * _b97_g(GAMMA_X, C_X, x2s)
        f = f + _pw_spin(r) * _b97_g(GAMMA_SS, C_SS, x2s)
    rho = ra + rb
    z = (ra - rb) / rho
    rs = (3.0 / (4.0 * math.pi)) ** (1.0 / 3.0) * rho ** (-1.0 / 3.0)
    e_ab = rho * _pw_pol(rs, z) - _pw_spin(ra) - _pw_spin(rb)
    return f + e_ab * _b97_g(GAMMA_AB, C_AB, 0.5 * (x2[0] + x2[1]))


def eval_wb97x_pol(ra, rb, saa, sab, sbb):
    """-> f and [v_rho_a, v_rho_b, v_sigma_aa, v_sigma_ab, v_sigma_bb], zero where the total density is below the
    threshold (the conventions of oracle.xc_oracle.eval_functional_pol)."""
    ok = (ra + rb) > DENS_THRESHOLD
    a = np.where(ok, np.maximum(ra, SPIN_FLOOR), 0.5)
    b = np.where(ok, np.maximum(rb, SPIN_FLOOR), 0.5)
    xs = [a, b, np.where(ok, np.maximum(saa, 1.0e-40), 1.0e-40), np.where(ok, sab, 0.0), np.where(ok, np.maximum(sbb, 1.0e-40), 1.0e-40)]
    d = wb97x_pol(*[DualN.var(x, i, 5) for i, x in enumerate(xs)])
    z = np.zeros_like(ra)
    return np.where(ok, d.v, z), [np.where(ok, t, z) for t in d.d]


def eval_wb97x(rho, sigma):
    """Restricted: rho_s = rho/2, sigma_ss = sigma_ab = sigma/4 -> f, v_rho, v_sigma."""
    f, (va, vb, vaa, vab, vbb) = eval_wb97x_pol(0.5 * rho, 0.5 * rho, 0.25 * sigma, 0.25 * sigma, 0.25 * sigma)
    return f, 0.5 * (va + vb), 0.25 * (vaa + vab + vbb)


# ------------------------------------------------------------------ the SCF's xc object
@dataclass
class WB97X:
    """`xc` for scf_oracle.run_rhf / run_uhf: grid part plus the long-range exchange the engine folds into K."""
    mol: scf_oracle.OracleMol
    level: int = 3
    omega: float = WB97X_OMEGA
    block: int = 4096
    exx: float = WB97X_EXX
    exx_lr: float = WB97X_EXX_LR

    def __post_init__(self):
        numbers = [int(round(z)) for z in self.mol.z]
        self.pts, self.w, _ = grid_oracle.build_grid(numbers, self.mol.xyz, self.level)
        self.eri_lr = eri4_erf(self.mol, self.omega)

    @classmethod
    def grid_only(cls, mol, level=3, block=4096):
        """The grid part alone (grid_potential): no long-range integrals are formed, k_lr and potential are not available."""
        self = cls.__new__(cls)
        for f in cls.__dataclass_fields__.values():
            if f.name != "mol":
                setattr(self, f.name, f.default)
        self.mol, self.level, self.block = mol, level, block
        numbers = [int(round(z)) for z in mol.z]
        self.pts, self.w, _ = grid_oracle.build_grid(numbers, mol.xyz, level)
        self.eri_lr = None
        return self

    def grid_potential(self, Da, Db):
        """Semi-local part for spin densities Da, Db: -> (E, V_a, V_b), without the long-range exchange."""
        return self._grid(Da, Db)

    def _grid(self, Da, Db):
        n = self.mol.nao
        Va = np.zeros((n, n)); Vb = np.zeros((n, n))
        exc = 0.0
        for b0 in range(0, len(self.w), self.block):
            p = self.pts[b0:b0 + self.block]; w = self.w[b0:b0 + self.block]
            ao, g = scf_oracle.eval_ao(self.mol, p, deriv=True)
            Xa = ao @ Da; Xb = ao @ Db
            ra = np.einsum("pi,pi->p", Xa, ao); rb = np.einsum("pi,pi->p", Xb, ao)
            ga = 2.0 * np.einsum("pi,dpi->dp", Xa, g); gb = 2.0 * np.einsum("pi,dpi->dp", Xb, g)
            saa = np.einsum("dp,dp->p", ga, ga); sab = np.einsum("dp,dp->p", ga, gb); sbb = np.einsum("dp,dp->p", gb, gb)
            f, (vra, vrb, vaa, vab, vbb) = eval_wb97x_pol(ra, rb, saa, sab, sbb)
            exc += float(np.dot(w, f))
            Va += (ao * (w * vra)[:, None]).T @ ao
            Vb += (ao * (w * vrb)[:, None]).T @ ao
            ca = 2.0 * vaa * ga + vab * gb
            cb = 2.0 * vbb * gb + vab * ga
            A = np.einsum("p,dp,dpi->pi", w, ca, g).T @ ao
            B = np.einsum("p,dp,dpi->pi", w, cb, g).T @ ao
            Va += A + A.T; Vb += B + B.T
        return exc, Va, Vb

    def k_lr(self, D):
        return np.einsum("ikjl,kl->ij", self.eri_lr, D, optimize=True)

    def potential(self, D):
        exc, Va, Vb = self._grid(0.5 * D, 0.5 * D)
        K = self.k_lr(D)
        return exc - 0.25 * self.exx_lr * float(np.sum(D * K)), 0.5 * (Va + Vb) - 0.5 * self.exx_lr * K

    def potential_uks(self, Da, Db):
        exc, Va, Vb = self._grid(Da, Db)
        Ka, Kb = self.k_lr(Da), self.k_lr(Db)
        exc -= 0.5 * self.exx_lr * (float(np.sum(Da * Ka)) + float(np.sum(Db * Kb)))
        return exc, Va - self.exx_lr * Ka, Vb - self.exx_lr * Kb
