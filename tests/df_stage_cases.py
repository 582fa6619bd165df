"""Cases of the density-fitting stage tests (mqc_hip_df_jk_batch, mqc_hip_df_fit_batch): synthetic J/K inputs at the
smallest shapes at which every instance and every edge of kern_df.hip's launch_df_jk exists, each named with the
instance the dispatch must pick, and the fit cases on which every three- and two-centre class occurs on generic
geometries.  tests/test_df_stage_cases.py checks them on the CPU, tests/test_gpu_df_stage.py compares the kernels with
the oracle on every route.

The dispatch rules, quoted from kern_df.hip (n = n_ao, o = n_occ, npair = n (n + 1) / 2, nt = ceil(n / 16)):
  wave<NTC,NLW>      MQC_HIP_DF_WAVE != 0, exx != 0, n <= 48, o <= 16: NTC = nt, NLW = 3 | 9 | 19 >= ceil(npair / 64)
  mfma<JMAX,NLD,K|J> LDS = 8 (npair + [16 nt (2 op + 1), op = 16 ceil(o / 16), when exx != 0] + 8) <= 150 KB;
                     jobs = ceil(nt (nt + 1) / 2 / 4), nld = ceil(npair / 256):
                     (jobs, nld) <= (1, 2), (2, 5), (3, 9), (6, 19), (9, 33); exx = 0 runs the J-only instance <1,NLD,J>
  v1<NV,lds|global>  MQC_HIP_DF_V1=1, or nothing above fits: df_j_kernel + df_k_kernel<NV,BLDS>, nv = ceil(n^2 / 256);
                     lds when 8 (n (n + 1) + n (2 o + 1) + 8) <= 150 KB.  INVARIANT: NV 256 >= n^2 and BLDS == lds.
                     global -> <77,global>; lds -> NV = 10 | 29 | 54 | 77 >= nv
  grids              wave: gx = min(ceil(2048 / m), ceil(n_aux / 16)) workgroups of four waves per fragment, a wave walks
                     rows wave + 4 g, ...; mfma: gx = min(ceil(3072 / m), n_aux); v1 (K): gx = min(ceil(2048 / m), n_aux),
                     a workgroup walks rows g, g + gx, ...

Two findings of these cases, both in the v1 selection as it stood (`nv <= 10 ? <10,lds> : nv <= 29 ? <29,lds> : lds ?
<54,lds> : <77,global>`):
  * (118, 5) and (130, 5): the row of B fits LDS, so <54,lds> ran -- but 54 x 256 = 13 824 < n^2 = 13 924 (16 900): the
    last elements of K stayed at the zero of the memset.  Now <77,lds>.
  * (86, 70): n^2 <= 29 x 256 but the row of B does NOT fit LDS next to 2 x 86 x 70 orbitals; <29,lds> ran with the LDS
    size of the global variant.  Reached by default (the mfma route declines above 150 KB) for fragments with about as
    many occupied orbitals as functions -- 17 neon atoms in STO-3G.  Now <77,global>.
The issue's table names mfma<2,5,J> and mfma<9,33,J> for exx = 0: the J-only instance is always <1,NLD,J> (the DJ macro of
df_jk_mfma_dispatch instantiates <1, NL, false>), so those read mfma<1,5,J> and mfma<1,33,J> here.

Test infrastructure: no GPU needed, never imported by the package."""
from __future__ import annotations

import json
import os
import zlib
from dataclasses import dataclass

import numpy as np

from tests import integral_class_cases as cc
from tests.xc_stage_cases import MARGIN

DJ_NW = 4
JK_CAP = 1e-11          # the project's J/K tolerance, x max(1, max |ref|) (tests/test_gpu_parity.py header)
INT_TOL = 1e-11         # the project's integral tolerance (test_eri_packed_matches_oracle)

# MARGIN (xc_stage_cases.py: 4 x 4 x 3 = 48, taken as 50) carries over with one factor re-argued.  x 4: the kernel is a
# second draw of the rounding noise, and the largest of n^2 elements of a second draw is a small multiple of the first.
# x 3: fused multiply-adds on the device where numpy rounds every product.  The x 4 that stood for the device's exp, cbrt
# and log stands here for the summation tree: the reference's contractions run through BLAS, whose blocked kernels keep
# 8 to 16 partial sums per element and add them at the end, where a workgroup adds its rows one after the other into one
# accumulator and the workgroups' partial sums meet in atomic adds of no fixed order -- a sum of N = n_aux n terms in
# one chain has an expected rounding error sqrt(N / (N / 16)) = 4 times that of sixteen interleaved chains.


def npair_of(n): return n * (n + 1) // 2


# ---- the dispatch, restated ------------------------------------------------------------------------------------------
def wave_instance(n, o, exx):
    npair = npair_of(n)
    if exx == 0.0 or n > 48 or o > 16:
        return None
    nt, nlw = (n + 15) // 16, (npair + 63) // 64
    for ntc, lim in ((1, 3), (2, 9), (3, 19)):
        if nt == ntc and nlw <= lim:
            NP = 16 * ntc
            lds = 8 * (npair + NP * 16 + DJ_NW * (npair + NP * 17) + 8)
            if lds > 80 * 1024 or npair + NP * NP > DJ_NW * (npair + NP * 17):
                return None
            return "wave<%d,%d>" % (ntc, lim)
    return None


def mfma_instance(n, o, exx):
    npair, nt = npair_of(n), (n + 15) // 16
    jobs, nld = (nt * (nt + 1) // 2 + DJ_NW - 1) // DJ_NW, (npair + 64 * DJ_NW - 1) // (64 * DJ_NW)
    op = (o + 15) // 16 * 16
    body = (16 * nt * op + 16 * nt * (op + 1) if exx != 0.0 else 0) + 8
    if 8 * (npair + body) > 150 * 1024:
        return None
    for jm, nl in ((1, 2), (2, 5), (3, 9), (6, 19), (9, 33)):
        if jobs <= jm and nld <= nl:
            return "mfma<%d,%d,%s>" % ((jm, nl, "K") if exx != 0.0 else (1, nl, "J"))
    return None


def v1_lds(n, o):
    return 8 * (n * (n + 1) + n * o + n * (o + 1) + 8) <= 150 * 1024


def v1_instance(n, o):
    nv = (n * n + 255) // 256
    if not v1_lds(n, o):
        return "v1<77,global>"
    return "v1<%d,lds>" % (10 if nv <= 10 else 29 if nv <= 29 else 54 if nv <= 54 else 77)


def instance_of(route, n, o, exx):
    """The instance launch_df_jk picks, from the rules above (route: a key of ROUTES)."""
    if route != "v1":
        got = (wave_instance(n, o, exx) if route == "default" else None) or mfma_instance(n, o, exx)
        if got:
            return got
    return v1_instance(n, o)


# ---- J/K cases -------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class JKCase:
    route: str
    n: int
    nocc: int
    expect: str              # the instance the dispatch must report
    exx: float = 1.0
    naux: int = 24
    m: int = 1
    rows: str = ""           # multi-row cases: auxiliary rows per workgroup (per wave on the wave kernel)

    @property
    def name(self):
        return "n%d-o%d-x%d-a%d-m%d" % (self.n, self.nocc, int(self.exx != 0.0), self.naux, self.m)


def _jk(route, n, o, expect, **kw):
    return JKCase(route, n, o, expect, **kw)


JK_CASES = [
    # ---- default route, exchange wanted
    _jk("default", 7, 5, "wave<1,3>"), _jk("default", 16, 16, "wave<1,3>"),
    _jk("default", 17, 1, "wave<2,9>"), _jk("default", 32, 16, "wave<2,9>"),
    _jk("default", 33, 9, "wave<3,19>"), _jk("default", 48, 10, "wave<3,19>"),
    _jk("default", 48, 17, "mfma<2,5,K>"),           # two orbital tiles: falls through the wave kernel
    _jk("default", 128, 32, "mfma<9,33,K>"),
    _jk("default", 128, 33, "v1<77,global>"),        # three orbital tiles: 161.6 KB of LDS, the mfma route declines
    _jk("default", 129, 30, "v1<77,global>"),        # nt = 9: no mfma instance
    _jk("default", 86, 70, "v1<77,global>"),         # second finding (module docstring): reached by default
    # ---- default route, pure functional: the J-only instances
    _jk("default", 7, 5, "mfma<1,2,J>", exx=0.0), _jk("default", 48, 10, "mfma<1,5,J>", exx=0.0),
    _jk("default", 128, 20, "mfma<1,33,J>", exx=0.0),
    # ---- MQC_HIP_DF_WAVE=0: the mfma buckets and their edges
    _jk("no-wave", 7, 5, "mfma<1,2,K>"), _jk("no-wave", 31, 9, "mfma<1,2,K>"),
    _jk("no-wave", 32, 9, "mfma<2,5,K>"), _jk("no-wave", 48, 10, "mfma<2,5,K>"),
    _jk("no-wave", 49, 12, "mfma<3,9,K>"), _jk("no-wave", 64, 20, "mfma<3,9,K>"),
    _jk("no-wave", 65, 7, "mfma<6,19,K>"), _jk("no-wave", 96, 24, "mfma<6,19,K>"),       # NP > 64: the uncached gather
    _jk("no-wave", 97, 19, "mfma<9,33,K>"),
    # ---- MQC_HIP_DF_V1=1: the round-1 pair
    _jk("v1", 7, 5, "v1<10,lds>"), _jk("v1", 50, 10, "v1<10,lds>"),
    _jk("v1", 51, 10, "v1<29,lds>"), _jk("v1", 86, 14, "v1<29,lds>"),
    _jk("v1", 87, 20, "v1<54,lds>"), _jk("v1", 117, 10, "v1<54,lds>"),
    _jk("v1", 118, 5, "v1<77,lds>"), _jk("v1", 130, 5, "v1<77,lds>"),                    # first finding (module docstring)
    _jk("v1", 118, 30, "v1<77,global>"), _jk("v1", 140, 35, "v1<77,global>"),
    _jk("v1", 86, 70, "v1<77,global>"),
    # ---- n_aux edges, one per family: a single row; ragged against 16 and against 4 DJ_NW
    _jk("default", 33, 9, "wave<3,19>", naux=1), _jk("default", 33, 9, "wave<3,19>", naux=37),
    _jk("no-wave", 49, 12, "mfma<3,9,K>", naux=1), _jk("no-wave", 49, 12, "mfma<3,9,K>", naux=37),
    _jk("default", 48, 10, "mfma<1,5,J>", exx=0.0, naux=37),
    _jk("v1", 51, 10, "v1<29,lds>", naux=1), _jk("v1", 51, 10, "v1<29,lds>", naux=37),
    # ---- several rows per workgroup (the prefetch of the next row, the alternating cpart buffer), rows from the grid
    # formulas above; B of the largest: 256 x 37 x 2080 doubles = 158 MB
    _jk("default", 48, 10, "wave<3,19>", naux=200, m=3, rows="gx = 13, 200 / (13 x 4) = 3.8 per wave"),
    _jk("default", 48, 10, "wave<3,19>", naux=37, m=256, rows="gx = 3, 37 / (3 x 4) = 3.1 per wave"),
    _jk("no-wave", 48, 10, "mfma<2,5,K>", naux=37, m=256, rows="gx = 12, 37 / 12 = 3.1"),
    _jk("no-wave", 64, 20, "mfma<3,9,K>", naux=37, m=256, rows="gx = 12, 37 / 12 = 3.1"),
    _jk("no-wave", 48, 10, "mfma<2,5,K>", naux=37, m=3, rows="gx = 37, 1"),
    _jk("default", 48, 10, "mfma<1,5,J>", exx=0.0, naux=37, m=256, rows="gx = 12, 37 / 12 = 3.1"),
    _jk("v1", 50, 10, "v1<10,lds>", naux=37, m=256, rows="gx = 8, 37 / 8 = 4.6"),
    _jk("v1", 50, 10, "v1<10,lds>", naux=37, m=3, rows="gx = 37, 1"),
    # ---- one workgroup per fragment: 2 048 fragments
    _jk("default", 7, 5, "wave<1,3>", naux=37, m=2048, rows="gx = 1, 37 / 4 = 9.3 per wave"),
    _jk("no-wave", 7, 5, "mfma<1,2,K>", naux=37, m=2048, rows="gx = 2, 37 / 2 = 18.5"),
    _jk("v1", 7, 5, "v1<10,lds>", naux=37, m=2048, rows="gx = 1, 37"),
]
JK_BY_KEY = {(c.route, c.name): c for c in JK_CASES}
assert len(JK_BY_KEY) == len(JK_CASES)

# every instance of launch_df_jk; tests/test_df_stage_cases.py asserts that the cases above name exactly this set
REQUIRED_INSTANCES = (["wave<1,3>", "wave<2,9>", "wave<3,19>"]
                      + ["mfma<%d,%d,K>" % p for p in ((1, 2), (2, 5), (3, 9), (6, 19), (9, 33))]
                      + ["mfma<1,%d,J>" % k for k in (2, 5, 33)]            # J-only: the sizes the issue lists
                      + ["v1<10,lds>", "v1<29,lds>", "v1<54,lds>", "v1<77,lds>", "v1<77,global>"])

# ---- routes: environment of the child process (each switch is a function-static, read once per process)
ROUTES = {
    "default": {},
    "no-wave": {"MQC_HIP_DF_WAVE": "0"},
    "v1": {"MQC_HIP_DF_V1": "1"},
    "chol-v1": {"MQC_HIP_DF_CHOL_V1": "1"},
}


def route_jk_cases(route):
    return [c for c in JK_CASES if c.route == route]


def rows_per_workgroup(c: JKCase):
    """Auxiliary rows the busiest workgroup (wave, on the wave kernel) walks, from the launchers' grid formulas."""
    if c.expect.startswith("wave"):
        gx = max(1, min((2048 + c.m - 1) // c.m, (c.naux + 4 * DJ_NW - 1) // (4 * DJ_NW)))
        return c.naux / (gx * DJ_NW)
    gx = max(1, min(((3072 if c.expect.startswith("mfma") else 2048) + c.m - 1) // c.m, c.naux))
    return c.naux / gx


def jk_inputs(c: JKCase):
    """-> B (m, n_aux, npair) seeded normal / sqrt(n_aux), D (m, n, n) random symmetric, C (m, n, n) with orthonormal
    columns: every fragment its own."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    n = c.n
    B = rng.standard_normal((c.m, c.naux, npair_of(n))) / np.sqrt(c.naux)
    D = rng.standard_normal((c.m, n, n))
    D = 0.5 * (D + np.swapaxes(D, 1, 2))
    C = np.linalg.qr(rng.standard_normal((c.m, n, n)))[0]
    return B, np.ascontiguousarray(D), np.ascontiguousarray(C)


def unpack(Bf):
    """(n_aux, npair) -> (n, n, n_aux), the oracle's layout."""
    from tests.stages import unpack_pairs
    return np.ascontiguousarray(np.moveaxis(unpack_pairs(Bf), 0, -1))


def _jk_longdouble(Bu, D, Co):
    L = np.longdouble
    Bu, D, Co = Bu.astype(L), D.astype(L), Co.astype(L)
    n, _, na = Bu.shape
    cP = (Bu.reshape(n * n, na) * D.reshape(n * n, 1)).sum(axis=0)
    J = (Bu * cP).sum(axis=2)
    W = np.stack([np.matmul(Bu[:, :, P], Co) for P in range(na)])          # (na, n, o)
    K = 2 * sum(np.matmul(W[P], W[P].T) for P in range(na))
    return J, K


EPS_FRAGMENTS = 2        # eps_ref of a batch case is measured on its first fragments (every fragment is the same draw)


def jk_reference_one(Bu, D, Co, with_eps=True):
    """One fragment, B unpacked (n, n, n_aux) -> (J, K, deviation of J, of K): oracle.scf_oracle.build_jk_df in float64;
    the deviations are the larger of float64 against np.longdouble and float64 against float64 with the auxiliary index
    reversed (0 when not asked for)."""
    from oracle import scf_oracle as so
    J, K = so.build_jk_df(Bu, D, Co)
    if not with_eps:
        return J, K, 0.0, 0.0
    Jr, Kr = so.build_jk_df(np.ascontiguousarray(Bu[:, :, ::-1]), D, Co)
    Jl, Kl = _jk_longdouble(Bu, D, Co)
    return (J, K, max(float(np.max(np.abs(J - Jr))), float(np.max(np.abs(J - Jl)))),
            max(float(np.max(np.abs(K - Kr))), float(np.max(np.abs(K - Kl)))))


def eps_floor(eps, ref):
    """eps_ref is not below one unit in the last place of max |ref|: a float64 reference is not known better."""
    return max(eps, np.finfo(np.float64).eps * float(np.max(np.abs(ref))))


def jk_reference(c: JKCase, B, D, C):
    """-> (J, K, eps_J, eps_K) of every fragment of a case (jk_reference_one, eps_floor)."""
    J, K = np.empty_like(D), np.empty_like(D)
    eps = np.zeros(2)
    for f in range(c.m):
        J[f], K[f], ej, ek = jk_reference_one(unpack(B[f]), D[f], np.ascontiguousarray(C[f][:, :c.nocc]), f < EPS_FRAGMENTS)
        eps = np.maximum(eps, (ej, ek))
    return J, K, eps_floor(eps[0], J), eps_floor(eps[1], K)


def jk_bound(eps_ref, ref):
    """MARGIN x eps_ref, never looser than the project's J/K tolerance 1e-11 max(1, max |ref|)."""
    return min(MARGIN * eps_ref, JK_CAP * max(1.0, float(np.max(np.abs(ref)))))


# ---- fit cases -------------------------------------------------------------------------------------------------------
ET = "mqc-even-tempered-jkfit"
DUP = "mqc-dup-jkfit"


@dataclass(frozen=True)
class FitCase:
    name: str
    basis: str
    aux: str
    geometry: str            # a key of integral_class_cases.CASES, "jitter3" (three fragments) or "water"
    flag: int = 0            # the fit flag every fragment must report


FIT_CASES = [
    FitCase("spd-generic-et", cc.SPD, ET, "generic"),
    FitCase("spd-stretched-et", cc.SPD, ET, "stretched"),
    FitCase("spdf-generic-et", cc.SPDF, ET, "generic"),
    FitCase("spdf-stretched-et", cc.SPDF, ET, "stretched"),
    FitCase("spdf-generic-self", cc.SPDF, cc.SPDF, "generic"),          # n_aux = 68 = 4 x 16 + 4: a ragged last block
    FitCase("spd-jitter3-et", cc.SPD, ET, "jitter3"),
    FitCase("water-dz-dup", "cc-pvdz", DUP, "water", flag=2),            # a duplicated shell: the eigen path, full mode
]
FIT_BY_NAME = {c.name: c for c in FIT_CASES}
# The optional batch in which one geometry flags and the others do not is left out: no geometry with the clean gap asked
# for was found.  Scan on the CPU: `generic` with the oxygen moved to 1e-1 .. 1e-8 Bohr from the nitrogen, even-tempered
# set.  At 0.1 Bohr the smallest eigenvalue is 1.8e-8 (nothing to cut); from 0.03 Bohr down one to four eigenvalues sit
# INSIDE [1e-12, 1e-8] (3.6e-9 at 0.03 Bohr, 9.2e-11 from 1e-6 Bohr on, where they stop moving: the two elements'
# exponents differ, so no function is ever duplicated) and none goes below 1e-12: cut or keep is a coin toss throughout.
WATER = ([8, 1, 1], [[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])   # as tests/test_gpu_parity.py


def write_basis_files(directory):
    """The probe sets and the duplicated-shell auxiliary set of test_df_near_singular_metric_takes_the_reference_eigen_cut
    into `directory` (point MQC_BASIS_PATH at it)."""
    from metalquicha_amd import basis as basis_mod
    cc.write_basis_files(directory)
    dup = json.load(open(basis_mod.find_basis_file(ET)))
    sh = json.loads(json.dumps(dup["elements"]["8"]["electron_shells"][0]))
    sh["exponents"] = ["%.16E" % (float(e) * (1.0 + 1.0e-9)) for e in sh["exponents"]]
    dup["elements"]["8"]["electron_shells"].append(sh)
    with open(os.path.join(str(directory), DUP + ".json"), "w") as f:
        json.dump(dup, f)


def fit_fragments(c: FitCase):
    from tests.helpers import fragment_bohr
    if c.geometry == "jitter3":
        return [cc.jitter(k) for k in range(3)]
    if c.geometry == "water":
        return [fragment_bohr(*WATER)]
    return [cc.CASES[c.geometry]()]


def route_fit_cases(route):
    """The Cholesky switch changes the unflagged fits only; the J/K switches change no fit kernel."""
    if route == "default":
        return list(FIT_CASES)
    if route == "chol-v1":
        return [c for c in FIT_CASES if c.name in ("spd-generic-et", "spdf-generic-self", "water-dz-dup")]
    return []


def pack_a3(j3):
    """The oracle's (n, n, n_aux) -> the engine's (n_aux, npair)."""
    ii, jj = np.tril_indices(j3.shape[0])
    return np.ascontiguousarray(j3[ii, jj, :].T)


def _eig_fit_G(A3, M, block=None):
    """G = A3^T M^+ A3 through the oracle's eigen fit (df_tensor: eigenvalues above 1e-10).  block: the same fit with
    the auxiliary index in another block order -- blocks of that many functions, the blocks in reversed order.  G does
    not depend on the order; the diagonalisation, J^-1/2 and both contractions then round differently."""
    from oracle import scf_oracle as so
    if block is not None:
        na = M.shape[0]
        p = np.concatenate([np.arange(b0, min(b0 + block, na)) for b0 in reversed(range(0, na, block))])
        A3, M = A3[p], M[np.ix_(p, p)]
    w, U = np.linalg.eigh(M)
    keep = w > so.METRIC_EIG_TOL
    B = ((U[:, keep] / np.sqrt(w[keep])[None, :]) @ U[:, keep].T) @ A3
    return B.T @ B


def fit_reference(c: FitCase, frag):
    """-> dict: A3 (n_aux, npair) from eri3c, M from eri2c, its spectrum w, G = A3^T M^+ A3 and eps_G.  eps_G: unflagged
    cases, the float64 difference between the eigen fit and a Cholesky fit (numpy.linalg.cholesky + solve) of the same
    integrals; the flagged case (no Cholesky factor exists), the eigen fit against itself at two block orders of the
    auxiliary index (_eig_fit_G).  A first version reordered only the last contraction B^T B: that measures the noise of
    one matrix product (one unit in the last place, 1.1e-15) and none of the fit's, which the conditioning of the kept
    spectrum governs (2.7e2 / 2.0e-5); against its bound of 5.3e-14 the eigen path measured 7.4e-14 on an MI355X, the
    level of every unflagged case.  With the whole fit reordered eps_G is 1.1e-13."""
    from oracle import scf_oracle as so
    from tests.helpers import oracle_mol
    mol, aux = oracle_mol(c.basis, frag), oracle_mol(c.aux, frag)
    A3, M = pack_a3(so.eri3c(mol, aux)), so.eri2c(aux)
    w = np.linalg.eigvalsh(M)
    G = _eig_fit_G(A3, M)
    if c.flag == 0:
        X = np.linalg.solve(np.linalg.cholesky(M), A3)
        other = X.T @ X
    else:
        other = _eig_fit_G(A3, M, block=16)
    eps = max(float(np.max(np.abs(G - other))), np.finfo(np.float64).eps * float(np.max(np.abs(G))))
    return {"A3": A3, "M": M, "w": w, "G": G, "eps_G": eps, "mol": mol, "aux": aux}


def conditioning_ok(c: FitCase, w):
    """No eigenvalue of the metric inside [1e-12, 1e-8] (the 1e-10 cut is then never a coin toss); the flagged case
    has exactly its duplicated directions (one s shell: one function) below 1e-12, the others none."""
    inside = np.sum((w >= 1e-12) & (w <= 1e-8))
    below = np.sum(w < 1e-12)
    return inside == 0 and below == (1 if c.flag == 2 else 0)


def g_bound(eps_G):
    return MARGIN * eps_G


# ---- class coverage ---------------------------------------------------------------------------------------------------
DF3C_CLASSES = [(a, b, p) for a in range(3) for b in range(a + 1) for p in range(4)]          # df3c_kernel<la,lb,lP>: 24
DF3C_GENERAL = [(3, b, p) for b in range(4) for p in range(4)]                                 # launch_df3c_general
DF2C_CLASSES = [(p, q) for p in range(4) for q in range(p + 1)]                                # df2c_kernel<lp,lq>: 10


def classes_seen(mol, aux):
    """-> ((la, lb, lP) with la >= lb whose bra shells sit on different atoms, (lp, lq) with lp >= lq on different atoms)."""
    l, lx = [int(x) for x in mol.sh_l], [int(x) for x in aux.sh_l]
    at, ax = cc.shell_atoms(mol), cc.shell_atoms(aux)
    c3 = {(max(l[a], l[b]), min(l[a], l[b]), p) for a in range(len(l)) for b in range(a) if at[a] != at[b] for p in set(lx)}
    c2 = {(max(lx[p], lx[q]), min(lx[p], lx[q])) for p in range(len(lx)) for q in range(p) if ax[p] != ax[q]}
    return c3, c2


# ---- the end-to-end tie: fitted B of the engine into the J/K stage ------------------------------------------------------
TIE_CASE = "spd-generic-et"
TIE_NOCC = 11


def tie_inputs(n):
    rng = np.random.default_rng(4242)
    D = rng.standard_normal((n, n))
    return 0.5 * (D + D.T), np.linalg.qr(rng.standard_normal((n, n)))[0]
