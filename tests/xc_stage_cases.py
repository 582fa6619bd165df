"""Cases of the exchange-correlation quadrature's stage test (mqc_hip_xc_batch): one small molecule per dispatch bucket
of kern_xc.hip's launch_xc, named with the bucket it is there to hit, so that the host test can check on the CPU that
every bucket still has a case in it (tests/test_xc_stage_cases.py) and the GPU test (tests/test_gpu_xc_stage.py) can
compare every one of them with the oracle, on every route.

The dispatch rules, quoted from kern_xc.hip (n = n_ao):
  nt = ceil(n / 16)                       output tiles per side (MFMA kernels)
  nv = ceil(n^2 / 256)                    accumulators per thread of xc_uks_kernel / xc_mgga_kernel:
                                          NV = 10 (n <= 50), 29 (n <= 86), 54 (n <= 117), 77 (n <= 140)
  jobs = ceil(nt^2 / 4)                   output tiles per wave of xc_tile_kernel (four waves)
  split quadrature    restricted LDA / GGA, n <= 96, lmax <= 3, radial cache on; NTC = nt, the LF (f shell) forms from
                      nt = 3; four waves up to nt = 4, eight above
  tile kernel         what the split quadrature does not take: nt <= 4 with the density in registers, nt = 5, 6 the wide
                      32-point tile (MQC_HIP_XC_WIDE_TILE), else 16-point tiles with JMAX = 9 (jobs <= 9), 16 (<= 16),
                      21 (<= 21), and above that 64 output tiles per blockIdx.z group: nz = ceil(nt^2 / 64)
  range separation    the split quadrature where it applies, else the 16-point tile family only (jobs <= 9, 16, 21); the
                      SCF refuses range-separated hybrids above n = 116, so jobs <= 21 (nt = 9, n >= 129) cannot be
                      reached through the product path and has no case; jobs <= 9 (n <= 96) is reached with
                      MQC_HIP_XC_SPLIT=0
  unrestricted        xc_uks_kernel by NV; meta-GGA: xc_mgga_kernel by NV, restricted or unrestricted

Geometries: waters (helpers.water_at) on a skewed line 5.6 Bohr apart, each with its own random orientation; H2 and OH
placed off that line.  Densities: helpers.orthonormal_orbitals / quadrature_density -- random orthonormal orbitals, no
symmetry, not converged, and in the cases marked `diffuse` one occupied orbital that is the loosest basis function alone.

Test infrastructure: no GPU needed, never imported by the package."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.helpers import (fragment_bohr, most_diffuse_ao, oracle_mol, orthonormal_orbitals, quadrature_density, random_rotation,
                           water_at)

XV_NW = 4            # waves of xc_tile_kernel
XC_NT = 256          # threads of xc_uks_kernel / xc_mgga_kernel


def nt_of(n): return (n + 15) // 16
def nv_of(n): return (n * n + XC_NT - 1) // XC_NT
def jobs_of(n): return (nt_of(n) ** 2 + XV_NW - 1) // XV_NW
def nz_of(n): return (nt_of(n) ** 2 + XV_NW * 16 - 1) // (XV_NW * 16)


def nv_bucket(n):
    nv = nv_of(n)
    return 10 if nv <= 10 else 29 if nv <= 29 else 54 if nv <= 54 else 77


def jmax_bucket(n):
    j = jobs_of(n)
    return 9 if j <= 9 else 16 if j <= 16 else 21 if j <= 21 else 0       # 0: the several-z-groups branch


@dataclass(frozen=True)
class Case:
    name: str
    waters: int              # water molecules
    extra: str               # "", "h2", "h2h2" (one or two H2 next to the waters), "oh" (a hydroxyl radical: open shell)
    basis: str
    functional: str
    level: int
    unrestricted: bool
    bucket: str              # the dispatch bucket on the default route, as bucket_of() spells it
    n: int                   # n_ao the case is meant to have
    diffuse: bool = False
    seed: int = 0            # geometry and orbitals; 0: derived from waters / extra / basis


_OH = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.8324]])          # r(OH) = 0.9697 Angstrom
_H2 = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.4]])


def geometry(case: Case, shift=0.0):
    """-> (Z, xyz in Bohr).  shift moves every molecule but the first along its own direction (batch cases)."""
    rng = np.random.default_rng(1000 + 17 * case.waters + len(case.extra) + case.seed)
    z, xyz = [], []
    for k in range(case.waters):
        z += [8, 1, 1]
        xyz.append(water_at(rng, [5.6 * k * (1.0 + shift), 0.7 * (k % 3) + shift * k, -0.5 * (k % 2)]))
    extras = {"": [], "h2": [_H2], "h2h2": [_H2, _H2], "oh": [_OH]}[case.extra]
    for i, m in enumerate(extras):
        z += [8, 1] if case.extra == "oh" else [1, 1]
        xyz.append(m @ random_rotation(rng).T + np.array([1.9 + 0.4 * i, 4.6 + 3.1 * i + shift, 2.2 - 0.3 * i]))
    return z, np.vstack(xyz)


def fragment(case: Case, shift=0.0):
    z, xyz = geometry(case, shift)
    return fragment_bohr(z, xyz, multiplicity=2 if case.extra == "oh" else 1)


def occupations(case: Case, frag):
    ne = int(frag.nelec)
    return ((ne + 1) // 2, ne // 2) if case.unrestricted else ne // 2


def density(case: Case, frag, S, mol, seed_offset=0):
    """-> (D, C): D (n, n), or (2, n, n) alpha then beta when unrestricted; C the orthonormal orbitals behind it."""
    C = orthonormal_orbitals(S, 7 + case.seed + seed_offset + case.waters, most_diffuse_ao(mol) if case.diffuse else None)
    return quadrature_density(C, occupations(case, frag)), C


def bucket_of(case: Case, n: int, lmax: int) -> str:
    """The kernel family and instantiation launch_xc picks on the default route, from the rules above."""
    rsh = case.functional in ("wb97x", "cam-b3lyp")
    if case.functional == "tpss":
        return "mgga-%s-nv%d" % ("uks" if case.unrestricted else "rks", nv_bucket(n))
    if case.unrestricted:
        return "uks-%snv%d" % ("rsh-" if rsh else "", nv_bucket(n))
    if n <= 96 and lmax <= 3 and not (lmax == 3 and nt_of(n) <= 2):
        return "split-%snt%d%s" % ("rsh-" if rsh else "", nt_of(n), "f" if lmax == 3 else "")
    j = jmax_bucket(n)
    return "tile-%s%s" % ("rsh-" if rsh else "", "j%d" % j if j else "z%d" % nz_of(n))


def _c(name, waters, extra, basis, functional, bucket, n, level=1, uks=False, diffuse=False):
    return Case(name, waters, extra, basis, functional, level, uks, bucket, n, diffuse)


CASES = []
# ---- restricted, split quadrature (n <= 96): LDA, GGA and hybrid instantiate <GGA = false / true>
for fn in ("svwn", "pbe", "b3lyp"):
    CASES += [
        _c("w1-sto3g-" + fn, 1, "", "sto-3g", fn, "split-nt1", 7),
        _c("w1-dz-" + fn, 1, "", "cc-pvdz", fn, "split-nt2", 24, diffuse=(fn == "pbe")),
        _c("w2-dz-" + fn, 2, "", "cc-pvdz", fn, "split-nt3", 48),
        _c("w1-tz-" + fn, 1, "", "def2-tzvp", fn, "split-nt3f", 43, diffuse=(fn == "b3lyp")),
        _c("w4-631g-" + fn, 4, "", "6-31g", fn, "split-nt4", 52),
        _c("w1h2-tz-" + fn, 1, "h2", "def2-tzvp", fn, "split-nt4f", 55),
    ]
CASES += [
    _c("w1-dz-b3lyp-level3", 1, "", "cc-pvdz", "b3lyp", "split-nt2", 24, level=3),
    _c("w3-dz-svwn", 3, "", "cc-pvdz", "svwn", "split-nt5", 72),
    _c("w3-dz-b3lyp", 3, "", "cc-pvdz", "b3lyp", "split-nt5", 72, diffuse=True),
    _c("w1h2h2-tz-svwn", 1, "h2h2", "def2-tzvp", "svwn", "split-nt5f", 67),
    _c("w1h2h2-tz-pbe", 1, "h2h2", "def2-tzvp", "pbe", "split-nt5f", 67),
    _c("w2-tz-svwn", 2, "", "def2-tzvp", "svwn", "split-nt6f", 86),
    _c("w2-tz-b3lyp", 2, "", "def2-tzvp", "b3lyp", "split-nt6f", 86),
    _c("w4-dz-svwn", 4, "", "cc-pvdz", "svwn", "split-nt6", 96),
    _c("w4-dz-pbe", 4, "", "cc-pvdz", "pbe", "split-nt6", 96),
    # ---- restricted, tile kernel above the split
    _c("w5-dz-svwn", 5, "", "cc-pvdz", "svwn", "tile-j16", 120),
    _c("w5-dz-b3lyp", 5, "", "cc-pvdz", "b3lyp", "tile-j16", 120),
    _c("w6-dz-pbe", 6, "", "cc-pvdz", "pbe", "tile-j21", 144),
    _c("w11-631g-svwn", 11, "", "6-31g", "svwn", "tile-j21", 143),
    _c("w11-631g-b3lyp", 11, "", "6-31g", "b3lyp", "tile-j21", 143),
    _c("w21-sto3g-pbe", 21, "", "sto-3g", "pbe", "tile-z2", 147),
    _c("w10-dz-svwn", 10, "", "cc-pvdz", "svwn", "tile-z4", 240),
    _c("w10-dz-b3lyp", 10, "", "cc-pvdz", "b3lyp", "tile-z4", 240),
]
# ---- unrestricted (open shell: a hydroxyl radical next to the waters)
for fn in ("svwn", "pbe", "b3lyp"):
    CASES.append(_c("oh-dz-u" + fn, 0, "oh", "cc-pvdz", fn, "uks-nv10", 19, uks=True, diffuse=(fn == "pbe")))
CASES += [
    _c("oh-w2-dz-usvwn", 2, "oh", "cc-pvdz", "svwn", "uks-nv29", 67, uks=True),
    _c("oh-w2-dz-ub3lyp", 2, "oh", "cc-pvdz", "b3lyp", "uks-nv29", 67, uks=True),
    _c("oh-w4-dz-usvwn", 4, "oh", "cc-pvdz", "svwn", "uks-nv54", 115, uks=True),
    _c("oh-w4-dz-upbe", 4, "oh", "cc-pvdz", "pbe", "uks-nv54", 115, uks=True),
    _c("oh-w5-dz-usvwn", 5, "oh", "cc-pvdz", "svwn", "uks-nv77", 139, uks=True),
    _c("oh-w5-dz-ub3lyp", 5, "oh", "cc-pvdz", "b3lyp", "uks-nv77", 139, uks=True),
    # ---- meta-GGA, restricted and unrestricted, the same four ranges
    _c("w1-dz-tpss", 1, "", "cc-pvdz", "tpss", "mgga-rks-nv10", 24, diffuse=True),
    _c("w3-dz-tpss", 3, "", "cc-pvdz", "tpss", "mgga-rks-nv29", 72),
    _c("w4-dz-tpss", 4, "", "cc-pvdz", "tpss", "mgga-rks-nv54", 96),
    _c("w5-dz-tpss", 5, "", "cc-pvdz", "tpss", "mgga-rks-nv77", 120),
    _c("oh-dz-utpss", 0, "oh", "cc-pvdz", "tpss", "mgga-uks-nv10", 19, uks=True),
    _c("oh-w2-dz-utpss", 2, "oh", "cc-pvdz", "tpss", "mgga-uks-nv29", 67, uks=True),
    _c("oh-w4-dz-utpss", 4, "oh", "cc-pvdz", "tpss", "mgga-uks-nv54", 115, uks=True),
    _c("oh-w5-dz-utpss", 5, "oh", "cc-pvdz", "tpss", "mgga-uks-nv77", 139, uks=True),
]
# ---- range-separated hybrids: a split size (also the jobs <= 9 tile with MQC_HIP_XC_SPLIT=0: w1 nt = 2, w3 nt = 5),
# the jobs <= 16 tile, an unrestricted size above n = 50
for fn in ("wb97x", "cam-b3lyp"):
    CASES += [
        _c("w1-dz-" + fn, 1, "", "cc-pvdz", fn, "split-rsh-nt2", 24),
        _c("w3-dz-" + fn, 3, "", "cc-pvdz", fn, "split-rsh-nt5", 72),
        _c("w8-631g-" + fn, 8, "", "6-31g", fn, "tile-rsh-j16", 104),
        _c("oh-w2-dz-u" + fn, 2, "oh", "cc-pvdz", fn, "uks-rsh-nv29", 67, uks=True),
    ]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every bucket the issue lists; tests/test_xc_stage_cases.py asserts that the cases above fill exactly this set
REQUIRED_BUCKETS = (
    ["split-nt%d" % k for k in range(1, 7)] + ["split-nt%df" % k for k in range(3, 7)]
    + ["tile-j16", "tile-j21", "tile-z2", "tile-z4"]
    + ["uks-nv%d" % k for k in (10, 29, 54, 77)]
    + ["mgga-rks-nv%d" % k for k in (10, 29, 54, 77)] + ["mgga-uks-nv%d" % k for k in (10, 29, 54, 77)]
    + ["split-rsh-nt2", "split-rsh-nt5", "tile-rsh-j16", "uks-rsh-nv29"]
)

# the batch cases: three dimers of one topology, three geometries, three densities; m = 1 is the first of them alone
BATCH_CASE = BY_NAME["w2-dz-b3lyp"]
BATCH_SHIFTS = (0.0, 0.07, 0.16)

# ---- routes: environment of the child process -> which cases it runs (each switch is read once per process)
ROUTES = {
    "default": {},
    "tile": {"MQC_HIP_XC_SPLIT": "0"},
    "pipe": {"MQC_HIP_XC_SPLIT": "0", "MQC_HIP_XC_PIPE": "1"},
    "no-radial-cache": {"MQC_HIP_XC_RADIAL_CACHE": "0"},
    "narrow-tile": {"MQC_HIP_XC_SPLIT": "0", "MQC_HIP_XC_WIDE_TILE": "0"},
    "no-radial-lds": {"MQC_HIP_XC_SPLIT": "0", "MQC_HIP_XC_RADIAL_LDS": "0"},
    "no-fast-slab": {"MQC_HIP_XC_SPLIT": "0", "MQC_HIP_XC_FAST_SLAB": "0"},
}


def _restricted_gga_lda(c):
    return not c.unrestricted and c.functional != "tpss"


def route_cases(route: str):
    """The cases whose kernel the route's switches change (the others would repeat the default route)."""
    if route == "default":
        return list(CASES)
    r = [c for c in CASES if _restricted_gga_lda(c)]
    if route == "tile":
        return [c for c in r if c.n <= 96]
    if route == "pipe":
        # xc_pipe_kernel takes s, p, d shells only: the def2-TZVP cases would run the tile kernel again
        return [c for c in r if c.n <= 64 and c.functional not in ("wb97x", "cam-b3lyp") and "tz" not in c.name]
    if route == "no-radial-cache":
        return [c for c in r if c.level == 1]
    if route == "narrow-tile":
        return [c for c in r if nt_of(c.n) in (5, 6)]
    if route == "no-radial-lds":
        return [c for c in r if c.level == 1]
    if route == "no-fast-slab":
        return [c for c in r if c.n <= 96 and "tz" not in c.name]      # the fast slab needs lmax <= 2 and n <= 96
    raise KeyError(route)


# ---- tolerances (issue section 5; how they were measured: tests/test_xc_stage_cases.py, measure_eps_ref) -----------------
# eps_ref: the reference's own noise floor on V_xc per case class, the larger of
#   max |V(block = 4096) - V(block = 509)|              (another summation order)
#   max |V(block = 4096) - V(block = 127, blocks accumulated in np.longdouble)|
# over the cases of the class, measured on the CPU and rounded up to one digit.  E_xc and N_e likewise.
# MARGIN: the kernel is another draw of the same rounding noise with another reduction tree (blocks of 16 or 32 points,
# MFMA accumulation, atomic adds across workgroups): the largest of n^2 elements of a second draw is a small multiple of
# the first (x 4); the device's exp, cbrt and log are off numpy's by a unit or two in the last place, a relative error of
# v_rho and v_sigma at every point that does not average out (x 4); and the dual-number chains are contracted into fused
# multiply-adds on the device where numpy rounds every product (x 3).  4 x 4 x 3 = 48, taken as 50.
MARGIN = 50.0
EPS_REF_V = {"lda": 3e-15, "gga": 7e-15, "mgga": 7e-15, "rsh": 7e-15}
EPS_REF_E = {"lda": 4e-15, "gga": 4e-15, "mgga": 4e-15, "rsh": 4e-15}      # per ten electrons
EPS_REF_N = 6e-15                                                         # per ten electrons


def case_class(case: Case) -> str:
    return {"svwn": "lda", "tpss": "mgga", "wb97x": "rsh", "cam-b3lyp": "rsh"}.get(case.functional, "gga")


def bounds(case: Case, vmax: float, nelec: float):
    """-> (bound on every element of V_xc, on E_xc, on N_e).  eps_ref x MARGIN -- for the two scalars scaled with the
    electron count (E_xc, N_e and the number of grid points grow with the molecule; an element of V_xc does not) -- never
    looser than the project's element-wise bound of a one-electron potential matrix, 1e-10 max(1, max |V_ref|), or
    1e-10 absolute for the two scalars."""
    cls = case_class(case)
    scale = max(1.0, nelec / 10.0)
    return (min(MARGIN * EPS_REF_V[cls], 1e-10 * max(1.0, vmax)),
            min(MARGIN * EPS_REF_E[cls] * scale, 1e-10), min(MARGIN * EPS_REF_N * scale, 1e-10))


def oracle_for(case: Case, mol, block=4096):
    """The reference object of a case: XCOracle, or the grid part of the range-separated reference classes (their
    constructors form the long-range integrals in Python, which the quadrature does not need)."""
    from oracle import xc_oracle
    if case.functional in ("wb97x", "cam-b3lyp"):
        from tests import cam_b3lyp_reference, range_separated_reference
        cls = range_separated_reference.WB97X if case.functional == "wb97x" else cam_b3lyp_reference.CAMB3LYP
        return cls.grid_only(mol, case.level, block)
    return xc_oracle.XCOracle(mol, case.functional, case.level, block)


def _integrated_density(ref, Dt):
    """sum_p w_p rho(r_p) on the reference's grid, block by block as XCOracle does (the range-separated reference
    classes do not integrate the density; N_e does not depend on the functional)."""
    from oracle import scf_oracle
    nel = 0.0
    for b0 in range(0, len(ref.w), ref.block):
        ao = scf_oracle.eval_ao(ref.mol, ref.pts[b0:b0 + ref.block])
        nel += float(np.dot(ref.w[b0:b0 + ref.block], np.einsum("pi,pi->p", ao @ Dt, ao)))
    return nel


def reference(case: Case, ref, D):
    """-> (E_xc, N_e, V) in the shape of D."""
    if case.functional in ("wb97x", "cam-b3lyp"):
        if case.unrestricted:
            e, va, vb = ref.grid_potential(D[0], D[1])
            return e, _integrated_density(ref, D[0] + D[1]), np.stack([va, vb])
        e, va, vb = ref.grid_potential(0.5 * D, 0.5 * D)
        return e, _integrated_density(ref, D), 0.5 * (va + vb)
    if case.unrestricted:
        e, va, vb = ref.potential_uks(D[0], D[1])
        return e, ref.n_electrons, np.stack([va, vb])
    e, v = ref.potential(D)
    return e, ref.n_electrons, v
