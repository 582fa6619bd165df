"""numpy reference for the range-separated hybrid CAM-B3LYP (test infrastructure, never imported by the package).

libxc's hyb_gga_xc_cam_b3lyp (Yanai, Tew & Handy 2004): omega = 0.33, cam_alpha = 0.65, cam_beta = -0.46, ac = 0.81,

    E_xc = 0.35 B88 + 0.46 ITYH_B88(omega) + 0.19 VWN5 + 0.81 LYP - 1/4 [0.19 tr(D K) + 0.46 tr(D K_lr(omega))]

(restricted; per spin for unrestricted).  VWN5 (libxc XC_LDA_C_VWN), not B3LYP's VWN-RPA.  The pieces:

  ityh_spin         one spin's short-range B88 in the ITYH form (Iikura, Tsuneda, Yanai & Hirao 2001):
                    e_s = -C_x rho_s^(4/3) F(x_s) F_att(a_s), a_s = omega sqrt(F(x_s)) / (2 k_Fs), with B88's enhancement
                    factor F and the attenuation function of tests/range_separated_reference.py (its series for a >= 1).
  cam_b3lyp_pol     the semi-local mix, on the oracle's polarised B88, VWN5 and LYP.
  CAMB3LYP          an `xc` object for oracle.scf_oracle.run_rhf / run_uhf: the grid part plus -1/4 exx_lr tr(D K_lr),
                    K_lr from range_separated_reference.eri4_erf.  The grid loop takes the evaluator as a parameter.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable

import numpy as np

from oracle import grid_oracle, scf_oracle
from oracle.xc_oracle import (DENS_THRESHOLD, SPIN_FLOOR, DualN, gga_c_lyp_pol, gga_x_b88_pol, lda_c_vwn_pol, nasinh,
                              nsqrt)
from tests.range_separated_reference import attenuation_erf, eri4_erf

CAM_OMEGA = 0.33
CAM_EXX = 0.19              # cam_alpha + cam_beta: exact exchange at every range
CAM_EXX_LR = 0.46           # -cam_beta: the long-range part on top
W_B88, W_ITYH, W_VWN, W_LYP = 0.35, 0.46, 0.19, 0.81
B88_BETA = 0.0042
C_X = 0.75 * (6.0 / math.pi) ** (1.0 / 3.0)


def b88_enhancement(x):
    """B88's F(x) with e_s = -C_x rho_s^(4/3) F(x_s)."""
    return 1.0 + (B88_BETA / C_X) * x * x / (1.0 + 6.0 * B88_BETA * x * nasinh(x))


def ityh_spin(r, s, omega=CAM_OMEGA):
    """One spin's attenuated B88 per volume (dual numbers in whatever variables r = rho_s and s = sigma_ss carry)."""
    r13 = r ** (1.0 / 3.0)
    r43 = r13 * r
    F = b88_enhancement(nsqrt(s) / r43)
    kf = (6.0 * math.pi ** 2) ** (1.0 / 3.0) * r13
    return -C_X * r43 * F * attenuation_erf(omega * nsqrt(F) / (2.0 * kf))


def ityh_pol(ra, rb, saa, sab, sbb, omega=CAM_OMEGA):
    del sab
    return ityh_spin(ra, saa, omega) + ityh_spin(rb, sbb, omega)


def cam_b3lyp_pol(ra, rb, saa, sab, sbb, omega=CAM_OMEGA):
    """f per volume of the semi-local part, dual numbers in (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb)."""
    args = (ra, rb, saa, sab, sbb)
    return (W_B88 * gga_x_b88_pol(*args) + W_ITYH * ityh_pol(*args, omega=omega) + W_VWN * lda_c_vwn_pol(*args)
            + W_LYP * gga_c_lyp_pol(*args))


def _eval_pol(fn, ra, rb, saa, sab, sbb):
    """-> f and [v_rho_a, v_rho_b, v_sigma_aa, v_sigma_ab, v_sigma_bb] of fn, zero where the total density is below the
    threshold (the conventions of oracle.xc_oracle.eval_functional_pol)."""
    ra, rb, saa, sab, sbb = (np.asarray(t, dtype=np.float64) for t in (ra, rb, saa, sab, sbb))
    ok = (ra + rb) > DENS_THRESHOLD
    a = np.where(ok, np.maximum(ra, SPIN_FLOOR), 0.5)
    b = np.where(ok, np.maximum(rb, SPIN_FLOOR), 0.5)
    xs = [a, b, np.where(ok, np.maximum(saa, 1.0e-40), 1.0e-40), np.where(ok, sab, 0.0), np.where(ok, np.maximum(sbb, 1.0e-40), 1.0e-40)]
    d = fn(*[DualN.var(x, i, 5) for i, x in enumerate(xs)])
    z = np.zeros_like(ra)
    return np.where(ok, d.v, z), [np.where(ok, t, z) for t in d.d]


def eval_cam_b3lyp_pol(ra, rb, saa, sab, sbb):
    return _eval_pol(cam_b3lyp_pol, ra, rb, saa, sab, sbb)


def eval_ityh_pol(ra, rb, saa, sab, sbb, omega=CAM_OMEGA):
    return _eval_pol(lambda *v: ityh_pol(*v, omega=omega), ra, rb, saa, sab, sbb)


def eval_b88_pol(ra, rb, saa, sab, sbb):
    return _eval_pol(gga_x_b88_pol, ra, rb, saa, sab, sbb)


def restricted(eval_pol):
    """The restricted form of a polarised evaluator: rho_s = rho/2, sigma_ss = sigma_ab = sigma/4 -> f, v_rho, v_sigma
    (the device's restricted path forms it the same way)."""
    def ev(rho, sigma):
        f, (va, vb, vaa, vab, vbb) = eval_pol(0.5 * rho, 0.5 * rho, 0.25 * sigma, 0.25 * sigma, 0.25 * sigma)
        return f, 0.5 * (va + vb), 0.25 * (vaa + vab + vbb)
    return ev


eval_cam_b3lyp = restricted(eval_cam_b3lyp_pol)


# ------------------------------------------------------------------ the SCF's xc object
@dataclass
class CAMB3LYP:
    """`xc` for scf_oracle.run_rhf / run_uhf: grid part plus the long-range exchange the engine folds into K."""
    mol: scf_oracle.OracleMol
    level: int = 3
    omega: float = CAM_OMEGA
    block: int = 4096
    exx: float = CAM_EXX
    exx_lr: float = CAM_EXX_LR
    eval_pol: Callable = eval_cam_b3lyp_pol

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
            f, (vra, vrb, vaa, vab, vbb) = self.eval_pol(ra, rb, saa, sab, sbb)
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
