"""Cases and reference of the RI-MP2 stage tests (mqc_hip_rimp2_stage: the three kernels of kern_mp2.hip, once, on given
tensors): synthetic inputs at the smallest shapes at which every route of the transform and every edge of the pair
kernel exists, each named with the route the launcher must report.  tests/test_rimp2_stage_cases.py checks them on the
CPU (the routes through the host-only half of the entry: the launcher's own arithmetic, no Python copy of it),
tests/test_gpu_rimp2_stage.py compares the kernels with the reference element by element.

The launcher's rules, quoted from kern_mp2.hip (n = n_ao, no = n_occ - n_frozen, nop = no rounded up to 16, nvpad =
n - n_occ rounded up to 16, napad = n_aux rounded up to 4, npair = n (n + 1) / 2, nt = ceil(n / 16)):
  wave buffer      8 (npair + 16 nt (oc + 1)) bytes: the packed row and T
  C in LDS         MQC_HIP_MP2_C_LDS != 0, nop <= 64 and 8 (4 ceil(n / 4)) (nop + nvpad) + two wave buffers <= 163 328:
                   oc = nop (one pass), waves = 8, 4, 2 -- the most that fit; rows of at most 64 x 20 pairs (n <= 50) are
                   prefetched into registers (NPF = 20), longer ones are not (NPF = 0)
  C from L2        otherwise: oc = min(nop, 64), 4 waves while they fit HALF the LDS, then 2, then 1 in the whole of it
  grid             gx = min(ceil(2048 / m), ceil(napad / waves)) workgroups per fragment; wave w of workgroup g walks the
                   rows g waves + w, + gx waves, ... up to napad (the rows n_aux .. napad - 1 are the zero padding of Bia)

Two families of input per case.  "int": B in {-2..2}, C in {-1, 0, 1}, dyadic orbital energies -- Bia and every (ia|jb)
are integers far below 2^53, exact in float64 in any summation order, so Bia is compared for EXACT equality, padding
included.  "real": C from a QR, B normal / sqrt(n_aux), sorted energies with a gap -- the same comparisons at a bound.

Bounds of everything that is not exact: MARGIN x eps_ref per case and per quantity (Bia, pair partials, fragment
energies), eps_ref the larger of the float64 reference against np.longdouble and against float64 with the auxiliary
index reversed, not below one unit in the last place of the largest reference value; never looser than 1e-11 max(1,
max |ref|) for elements (Bia, partials) nor than the project's 1e-8 for energies.  The energies of these synthetic
inputs are not of the order of one Hartree (the integer family reaches 1e9, the real one 1e5: one unit in the last place
of the reference is then 1e-7 and 1e-11), so the energy cap is taken relative like the elements' one: 1e-8 max(1, max
|e_ref|).  On the project's molecules (|e| < 1) it is the 1e-8 Eh of tests/test_gpu_rimp2.py.

Test infrastructure: no GPU needed, never imported by the package."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

from tests.xc_stage_cases import MARGIN

# MARGIN (xc_stage_cases.py: 4 x 4 x 3 = 48, taken as 50) carries over with one factor re-argued, as in df_stage_cases.py.
# x 4: the kernel is a second draw of the rounding noise, and the largest of many elements of a second draw is a small
# multiple of the first.  x 3: fused multiply-adds on the device where numpy rounds every product (x * x * d and the
# matrix-core steps).  The x 4 that stood for the device's exp, cbrt and log stands here for the summation tree: the
# reference's contractions over mu, nu and P run through BLAS (8 to 16 interleaved partial sums per element) and its pair
# sums through numpy's pairwise summation, where the matrix core adds the k index four terms at a time into ONE
# accumulator per element (a chain of n / 4 and napad / 4 steps), a lane adds its share of the nv^2 / 64 terms of a pair
# one after the other, and the reduction adds the no (no + 1) / 2 partials of a fragment in pair order into one
# accumulator -- a chain of N terms has an expected rounding error sqrt(N / (N / 16)) = 4 times that of sixteen
# interleaved chains.
ELEM_CAP = 1e-11        # x max(1, max |ref|): the project's element tolerance (tests/df_stage_cases.py, JK_CAP)
ENERGY_CAP = 1e-8       # x max(1, max |e_ref|): the project's energy tolerance (tests/test_gpu_rimp2.py), see the docstring
LDS_MAX = 160 * 1024 - 512


def npair_of(n): return n * (n + 1) // 2


# ---- cases -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    route: str               # "default" | "no-clds": the environment of the child process (ROUTES)
    n: int
    nocc: int
    naux: int
    nfz: int
    clds: int                # what the launcher must report: C in LDS (1) or from L2 (0),
    npf: int                 # pairs of a row prefetched per lane (20 or 0),
    waves: int               # waves per workgroup of the transform,
    oc: int                  # occupied orbitals per pass,
    passes: int              # passes over the occupied orbitals,
    vtiles: int              # virtual tiles (nvpad / 16),
    lds: int                 # dynamic LDS bytes
    salt: int = 0            # integer family: the draw (the first whose Bia is not identically zero)

    @property
    def name(self):
        return "n%d-o%d-a%d-f%d" % (self.n, self.nocc, self.naux, self.nfz)

    @property
    def no(self): return self.nocc - self.nfz

    @property
    def napad(self): return (self.naux + 3) // 4 * 4

    @property
    def nvpad(self): return (self.n - self.nocc + 15) // 16 * 16

    @property
    def instance(self):
        return "l2" if not self.clds else "prefetch" if self.npf else "no-prefetch"

    def expected_route(self):
        return {"clds": self.clds, "npf": self.npf, "waves": self.waves, "oc": self.oc, "passes": self.passes,
                "nvpad": 16 * self.vtiles, "lds": self.lds, "napad": self.napad, "npairs": self.no * (self.no + 1) // 2, "narrowed": 0}


def _c(route, n, nocc, naux, nfz, clds, npf, waves, oc, passes, vtiles, lds, **kw):
    return Case(route, n, nocc, naux, nfz, clds, npf, waves, oc, passes, vtiles, lds, **kw)


CASES = [
    # ---- the launcher's own choice (the table of the issue; n_aux mod 4 = 1, 2, 1, 1, 2, 2, 0, 2, 2, 2, 2, 2, 2, 2)
    _c("default", 2, 1, 5, 0, 1, 20, 8, 16, 1, 1, 18624),              # one pair, one virtual: e_ss = 0 exactly
    _c("default", 13, 5, 126, 1, 1, 20, 8, 16, 1, 1, 27328),           # a frozen orbital; n mod 4 and mod 16 non-zero
    _c("default", 33, 17, 9, 0, 1, 20, 8, 32, 1, 1, 151104),           # the second occupied tile; nv = 16
    _c("default", 33, 16, 9, 0, 1, 20, 8, 16, 1, 2, 101952),           # nv = 17: one valid column in the off-diagonal tile
    _c("default", 31, 16, 11, 0, 1, 20, 8, 16, 1, 1, 74752),           # nv = 15; n_aux mod 4 = 3
    _c("default", 50, 5, 30, 0, 1, 20, 4, 16, 1, 3, 102240),           # npair = 1275: the last shape with the prefetch
    _c("default", 51, 5, 30, 0, 1, 0, 4, 16, 1, 3, 103872),            # npair = 1326 > 64 x 20
    _c("default", 50, 49, 10, 0, 1, 20, 2, 64, 1, 1, 120240),          # four occupied tiles with C in LDS (nop = 64), nv = 1
    _c("default", 48, 10, 252, 2, 1, 20, 8, 16, 1, 3, 152064),         # n a multiple of 16; two frozen; 36 pairs
    _c("default", 64, 33, 30, 0, 1, 0, 2, 48, 1, 2, 124416),           # nop = 48, two waves
    _c("default", 72, 15, 378, 3, 1, 0, 2, 16, 1, 4, 109888),
    _c("default", 80, 40, 22, 0, 0, 0, 1, 48, 1, 3, 57280),            # C no longer fits next to two waves: from L2
    _c("default", 100, 65, 18, 0, 0, 0, 1, 64, 2, 3, 98640),           # two passes, the last over a single orbital
    _c("default", 140, 70, 18, 0, 0, 0, 1, 64, 2, 5, 153840),          # the largest n the stage claims
    _c("default", 140, 139, 6, 0, 0, 0, 1, 64, 3, 1, 153840),          # three passes, one virtual
    _c("default", 140, 20, 6, 0, 0, 0, 1, 32, 1, 8, 116976),           # eight virtual tiles
    # ---- MQC_HIP_MP2_C_LDS=0: the L2 kernel with more than one wave
    _c("no-clds", 13, 5, 126, 1, 0, 0, 4, 16, 1, 1, 11616),
    _c("no-clds", 33, 17, 9, 0, 0, 0, 4, 32, 1, 1, 68640),
    _c("no-clds", 40, 36, 7, 0, 0, 0, 2, 48, 1, 1, 50752),             # n_aux mod 4 = 3; 666 pairs = 166 workgroups + 2 waves
    _c("no-clds", 2, 1, 5, 0, 0, 0, 4, 16, 1, 1, 8800),
]
BY_KEY = {(c.route, c.name): c for c in CASES}
assert len(BY_KEY) == len(CASES)
ROUTES = {"default": {}, "no-clds": {"MQC_HIP_MP2_C_LDS": "0"}}
FAMILIES = ("int", "real")


def route_cases(route):
    return [c for c in CASES if c.route == route]


# ---- several rows per wave: one shape of each transform instance, capped at 1 and 2 workgroups per fragment -----------
ROWS_SHAPES = [("default", "n13-o5-a126-f1"), ("default", "n51-o5-a30-f0"), ("default", "n80-o40-a22-f0")]
ROWS_CAPS = (1, 2)
ROWS_M = 2                # fragments of a capped run (fragment 0 is the case's own input)
# the uncapped proof that the cap reproduces the launcher: 300 fragments, six distinct inputs tiled
TILED = ("default", "n13-o5-a126-f1")
TILED_M, TILED_DISTINCT, TILED_GX, TILED_ROWS = 300, 6, 7, 3
# the ragged batch: nmo = n, n - 3, nocc (no virtuals), a fragment that does not run, nocc - 1
RAGGED = ("default", "n33-o16-a9-f0")
RAGGED_NMO = (33, 30, 16, 33, 15)
RAGGED_RUNS = (1, 1, 1, 0, 1)
# the stale-pool pair: the second after the first in one process against the second alone in a fresh process
STALE = (("default", "n48-o10-a252-f2"), ("default", "n13-o5-a126-f1"))


def run_labels(route):
    """Every run the child of a route must report (tests/rimp2_stage_child.py), in its order."""
    out = []
    if route == "default":
        out += ["fresh/%s" % f for f in FAMILIES]
    out += ["%s/%s" % (c.name, f) for c in route_cases(route) for f in FAMILIES]
    if route == "default":
        out += ["rows/%s/%s/cap%d" % (BY_KEY[k].name, f, cap) for k in ROWS_SHAPES for f in FAMILIES for cap in (0,) + ROWS_CAPS]
        out += ["tiled/%s" % f for f in FAMILIES]
        for f in FAMILIES:
            out += ["ragged/%s" % f] + ["ragged/%s/%d" % (f, k) for k in range(len(RAGGED_NMO))]
        for f in FAMILIES:
            out += ["stale-first/%s" % f, "stale/%s" % f]
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _rng(c: Case, family, k):
    return np.random.default_rng([zlib.crc32(("%s/%s" % (c.name, family)).encode()), k, c.salt if family == "int" else 0])


def inputs_one(c: Case, family, k=0):
    """-> B (n_aux, npair), C (n, n), eps (n,) of draw k of a case."""
    rng = _rng(c, family, k)
    n, nv = c.n, c.n - c.nocc
    if family == "int":
        B = rng.integers(-2, 3, size=(c.naux, npair_of(n))).astype(np.float64)
        C = rng.integers(-1, 2, size=(n, n)).astype(np.float64)
        eps = np.concatenate([-(0.5 + np.arange(c.nocc)[::-1] / 8.0), 0.25 + np.arange(nv) / 16.0])
    else:
        B = rng.standard_normal((c.naux, npair_of(n))) / np.sqrt(c.naux)
        C = np.linalg.qr(rng.standard_normal((n, n)))[0]
        eps = np.concatenate([np.sort(-0.15 - rng.uniform(0.0, 2.0, c.nocc)), np.sort(0.15 + rng.uniform(0.0, 2.0, nv))])
    return B, np.ascontiguousarray(C), eps


def inputs(c: Case, family, m=1):
    """-> B (m, n_aux, npair), C (m, n, n), eps (m, n): the draws 0 .. m - 1."""
    parts = [inputs_one(c, family, k) for k in range(m)]
    return tuple(np.ascontiguousarray(np.stack([p[i] for p in parts])) for i in range(3))


def tiled_inputs(c: Case, family):
    B, C, eps = inputs(c, family, TILED_DISTINCT)
    idx = np.arange(TILED_M) % TILED_DISTINCT
    return np.ascontiguousarray(B[idx]), np.ascontiguousarray(C[idx]), np.ascontiguousarray(eps[idx])


def ragged_inputs(c: Case, family):
    """Five draws; the columns of C and the entries of eps beyond each fragment's nmo are NaN."""
    B, C, eps = inputs(c, family, len(RAGGED_NMO))
    for f, nmo in enumerate(RAGGED_NMO):
        C[f][:, nmo:] = np.nan
        eps[f][nmo:] = np.nan
    return B, C, eps


# ---- reference ---------------------------------------------------------------------------------------------------------
def unpack(Bf):
    """(n_aux, npair) packed pairs (mu >= nu, index mu (mu + 1) / 2 + nu) -> the symmetric (n_aux, n, n)."""
    npair = Bf.shape[-1]
    n = int((np.sqrt(8 * npair + 1) - 1) / 2)
    ii, jj = np.tril_indices(n)
    out = np.zeros(Bf.shape[:-1] + (n, n), dtype=Bf.dtype)
    out[..., ii, jj] = Bf
    out[..., jj, ii] = Bf
    return out


def reference(Bf, C, eps, nocc, nfz=0, nmo=None, dtype=np.float64, reverse=False):
    """One fragment in plain numpy -> Bia (no, n_aux, nv), part (npairs, 2), e (2,), max |V|.
    Bia = einsum("mi,Pmn,na->iPa"); per pair i >= j: V = einsum("Pa,Pb->ab", Bia[i], Bia[j]), w sum V^2 / D and
    w sum V (V - V^T) / D with D = e_i + e_j - e_a - e_b and w = 1 (i = j) or 2; e: their sums.  dtype = np.longdouble
    and reverse (the auxiliary index walked backwards) give the reference's own noise floor."""
    nmo = C.shape[1] if nmo is None else nmo
    Bu = unpack(Bf).astype(dtype)
    Co, Cv = C[:, nfz:nocc].astype(dtype), C[:, nocc:nmo].astype(dtype)
    eo, ev = eps[nfz:nocc].astype(dtype), eps[nocc:nmo].astype(dtype)
    if reverse:
        Bu = Bu[::-1]
    Bia = np.einsum("mi,Pmn,na->iPa", Co, Bu, Cv, optimize=True)
    no = Co.shape[1]
    part = np.zeros((no * (no + 1) // 2, 2), dtype=dtype)
    vmax = 0.0
    dv = -(ev[:, None] + ev[None, :])
    for i in range(no):
        for j in range(i + 1):
            V = np.einsum("Pa,Pb->ab", Bia[i], Bia[j], optimize=True)
            if V.size:
                vmax = max(vmax, float(np.max(np.abs(V))))
            D = eo[i] + eo[j] + dv
            w = 1.0 if i == j else 2.0
            part[i * (i + 1) // 2 + j] = (w * np.sum(V * V / D), w * np.sum(V * (V - V.T) / D))
    if reverse:
        Bia = Bia[:, ::-1]
    return np.ascontiguousarray(Bia), part, part.sum(axis=0), vmax


def _floor(eps, ref):
    """eps_ref is not below one unit in the last place of max |ref|: a float64 reference is not known better."""
    top = float(np.max(np.abs(ref))) if np.size(ref) else 0.0
    return max(float(eps), np.finfo(np.float64).eps * top)


def _dev(a, b):
    return float(np.max(np.abs(a - b))) if np.size(a) else 0.0


@functools.lru_cache(maxsize=None)
def reference_with_eps(key, family, k=0, nmo=None):
    """The float64 reference of draw k of a case with its noise floors, computed once per process, shared by every test
    and never modified -> dict: Bia, part, e (float64, read-only), vmax, eps_bia, eps_part, eps_e, exact (integer family:
    float64, np.longdouble and the reversed order agree to the last bit on Bia and every V is an integer below 2^53)."""
    c = BY_KEY[key]
    Bf, C, eps = inputs_one(c, family, k)
    nmo = c.n if nmo is None else nmo
    Bia, part, e, vmax = reference(Bf, C, eps, c.nocc, c.nfz, nmo)
    Bl, pl, el, _ = reference(Bf, C, eps, c.nocc, c.nfz, nmo, dtype=np.longdouble)
    Br, pr, er, _ = reference(Bf, C, eps, c.nocc, c.nfz, nmo, reverse=True)
    out = {"Bia": Bia, "part": part, "e": e, "vmax": vmax,
           "eps_bia": _floor(max(_dev(Bia, Bl), _dev(Bia, Br)), Bia),
           "eps_part": _floor(max(_dev(part, pl), _dev(part, pr)), part),
           "eps_e": _floor(max(_dev(e, el), _dev(e, er)), e),
           "exact": bool(np.array_equal(Bia, Bl.astype(np.float64)) and np.array_equal(Bia, Br))}
    for v in (Bia, part, e):
        v.setflags(write=False)
    return out


def elem_bound(eps_ref, ref):
    """MARGIN x eps_ref, never looser than 1e-11 max(1, max |ref|)."""
    top = float(np.max(np.abs(ref))) if np.size(ref) else 0.0
    return min(MARGIN * eps_ref, ELEM_CAP * max(1.0, top))


def energy_bound(eps_ref, ref):
    """MARGIN x eps_ref, never looser than 1e-8 max(1, max |e_ref|) (module docstring)."""
    return min(MARGIN * eps_ref, ENERGY_CAP * max(1.0, float(np.max(np.abs(ref)))))


def pad_bia(Bia, c: Case):
    """The reference Bia (no, n_aux, nv) in the engine's layout (no, napad, nvpad): the padding is zeros."""
    out = np.zeros((Bia.shape[0], c.napad, c.nvpad))
    out[:, :Bia.shape[1], :Bia.shape[2]] = Bia
    return out
