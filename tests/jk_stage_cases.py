"""Cases, layouts, dispatch model and references of the in-core J/K stage tests (tests/test_jk_stage_cases.py on the
CPU, tests/test_gpu_jk_stage.py with tests/jk_stage_child.py on the GPU).  Test infrastructure.

The triangular layout is stated here from the comment at BatchView::eri_tri (engine.hpp), not from the C++:
  pair row r = (i, j), i >= j, r = i (i + 1) / 2 + j, holds the columns 0 .. r of the symmetric pair matrix and is
  completed with zeros to the end of row i of the packed triangle, (i + 1)(i + 2) / 2 elements in all; block t =
  [row npair - 1 - t | row t]; the short row starts at (i_l + 1)(i_l + 2) / 2, i_l the triangle row of the long row; the
  middle row of an odd npair has a block to itself; the block length is the largest need, rounded up to even; the
  diagonal elements (ij|ij) are stored halved.

The dispatch model restates launch_jk_incore, jk_tri_layout and incore_supported by their sizes (LDS bytes per
instance); tests/test_jk_stage_cases.py holds it against the host build of jk_tri_layout, and the GPU test against the
instance every launch reports.

Unreachable instances (kept in kern_fock.hip, no admissible shape lands on them): jk_incore_kernel<3,false,4,0,false>,
<4,false,4,0,false>, <3,false,2,0,false> and <4,false,2,0,false>: KCH = ceil(n / 64) >= 3 needs n >= 129, and
incore_supported admits n <= 116 only (three rows of npair doubles within 160 KB - 512 bytes)."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LDS_MAX = 160 * 1024 - 1024
TRI_NW, TRI_MAXU2 = 12, 10          # waves per workgroup of the triangular kernel, chunks of 128 doubles per block
N_MAX = 116                          # the last size incore_supported admits

ROUTES = {
    "default": {},
    "tri0": {"MQC_HIP_ERI_TRI": "0"},
    "wg1": {"MQC_HIP_JK_TRI_WG": "1"},
    "wg5": {"MQC_HIP_JK_TRI_WG": "5"},
    "wg1000": {"MQC_HIP_JK_TRI_WG": "1000"},
    "rowcoop0": {"MQC_HIP_JK_ROWCOOP": "0"},
}


def npair(n):
    return n * (n + 1) // 2


@functools.lru_cache(maxsize=None)
def pair_index(n):
    """(n, n) symmetric table of packed pair indices: [i, j] = max (max + 1) / 2 + min."""
    i, j = np.indices((n, n))
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    p = hi * (hi + 1) // 2 + lo
    p.setflags(write=False)
    return p


# ---- the triangular layout ----------------------------------------------------------------------------------------
def tri_row(r):
    """Row i of the packed triangle that holds index r."""
    i = (math.isqrt(8 * r + 1) - 1) // 2
    assert i * (i + 1) // 2 <= r < (i + 1) * (i + 2) // 2
    return i


@functools.lru_cache(maxsize=None)
def tri_table(np_):
    """(block length, [start of the short row in block t], [padded end of block t], [triangle row of pair row r])."""
    nblk = (np_ + 1) // 2
    rows = [tri_row(r) for r in range(np_)]
    sb, se = [], []
    for t in range(nblk):
        rl = np_ - 1 - t
        start = (rows[rl] + 1) * (rows[rl] + 2) // 2
        sb.append(start)
        se.append(start + ((rows[t] + 1) * (rows[t] + 2) // 2 if t < rl else 0))
    pb = (max(se) + 1) // 2 * 2
    return pb, tuple(sb), tuple(se), tuple(rows)


@functools.lru_cache(maxsize=None)
def _tri_map(np_):
    """Source (row, col), destination and weight of every stored element."""
    pb, sb, _, _ = tri_table(np_)
    nblk = (np_ + 1) // 2
    r = np.repeat(np.arange(np_), np.arange(1, np_ + 1))
    c = np.concatenate([np.arange(k + 1) for k in range(np_)])
    # rows npair - nblk .. npair - 1 are the long rows of blocks nblk - 1 .. 0 (the middle row of an odd npair among
    # them), the others the short row of their own block
    start = np.where(r >= np_ - nblk, (np_ - 1 - r) * pb, r * pb + np.asarray(sb)[np.minimum(r, nblk - 1)])
    w = np.where(r == c, 0.5, 1.0)
    return r, c, start + c, w, nblk * pb


def tri_pack(M):
    """Symmetric pair matrix (npair, npair) -> the tensor as stored, ((npair + 1) / 2 * block,)."""
    r, c, dst, w, size = _tri_map(M.shape[0])
    T = np.zeros(size, dtype=M.dtype)
    T[dst] = M[r, c] * w.astype(M.dtype)
    return T


def tri_unpack(T, np_):
    r, c, dst, w, size = _tri_map(np_)
    assert T.shape == (size,)
    M = np.zeros((np_, np_), dtype=T.dtype)
    M[r, c] = T[dst] / w.astype(T.dtype)
    M[c, r] = M[r, c]
    return M


def tri_lds_bytes(n):
    """LDS of jk_tri_kernel as its carve-up reads: NW row buffers, packed D' and J (+ 2 each), Kh, the zero-row flags
    (rounded up to 16), the function -> shell map (64 ints), one double per wave."""
    np_ = npair(n)
    return 8 * (TRI_NW * tri_table(np_)[0] + 2 * (np_ + 2) + n * n) + ((np_ + 15) & ~15) + 64 * 4 + TRI_NW * 8


def tri_layout(n, nfrag, uhf=False, env=None):
    """jk_tri_layout: restricted batches of at least 64 dimer-sized fragments (n <= 64, a multiple of 8, npair > 640)
    whose block fits ten chunks of 128 and whose LDS fits; MQC_HIP_ERI_TRI=0 turns it off."""
    if (env or {}).get("MQC_HIP_ERI_TRI", "1")[0] == "0" or uhf or nfrag < 64 or n > 64 or n % 8 or npair(n) <= 640:
        return False
    return tri_table(npair(n))[0] <= TRI_MAXU2 * 128 and tri_lds_bytes(n) <= LDS_MAX


def tensor_layout(n, nfrag, uhf=False, env=None):
    """(triangular, block doubles, doubles per fragment) -- what mqc_hip_jk_tensor_layout must report."""
    np_ = npair(n)
    if tri_layout(n, nfrag, uhf, env):
        pb = tri_table(np_)[0]
        return True, pb, (np_ + 1) // 2 * pb
    return False, 0, np_ * np_


def incore_supported(n):
    return n <= 256 and 8 * 3 * npair(n) <= 160 * 1024 - 512


# ---- the dispatch -------------------------------------------------------------------------------------------------
def instance_of(n, nfrag, uhf=False, env=None):
    """(name, grid x) of the kernel launch_jk_incore picks, names as mqc_hip_jk_incore_batch reports them."""
    env = env or {}
    np_ = npair(n)

    def wave(kch, klds, nw, maxu, dreg, full8=False):
        gx = max(1, min(-(-4096 // nfrag), -(-np_ // nw)))
        return "wave<%d,%s,%d,%d,%s%s>" % (kch, "lds" if klds else "global", nw, maxu, "reg" if dreg else "mem", ",full8" if full8 else ""), gx

    if tri_layout(n, nfrag, uhf, env):
        wg = int(env.get("MQC_HIP_JK_TRI_WG", "0"))
        gx = wg if wg > 0 else -(-768 // nfrag)
        return "tri<12,10>", max(1, min(gx, -(-((np_ + 1) // 2) // TRI_NW)))
    kch = -(-n // 64)
    lds_reg, lds_reg12 = 8 * (5 * np_ + n * n), 8 * (13 * np_ + n * n)
    lds4k, lds4, rc = 8 * (5 * np_ + 2 * n * n), 8 * 5 * np_, 8 * (3 * 8 * 512 + n * n + 16)
    if n <= 64 and 320 < np_ <= 1216 and lds_reg12 <= LDS_MAX and nfrag >= 64:
        if np_ <= 640:
            return wave(1, True, 12, 10, True)
        if n % 8 == 0 and np_ % 2 == 0 and 8 * (12 * 10 * 128 + np_ + n * n) <= LDS_MAX:
            return wave(1, True, 12, 19, True, True)
        return wave(1, True, 12, 19, True)
    if n <= 64 and lds_reg <= LDS_MAX:
        return wave(1, True, 4, 5 if np_ <= 320 else 10 if np_ <= 640 else 19 if np_ <= 1216 else 0, True)
    if lds4k <= LDS_MAX and kch <= 2:
        return wave(2, True, 4, 0, False)
    if kch == 2 and np_ <= 8 * 512 and rc <= LDS_MAX and env.get("MQC_HIP_JK_ROWCOOP", "1")[0] != "0":
        return "rowcoop<2,8>", max(1, min(-(-2048 // nfrag), np_))
    if lds4 <= LDS_MAX:
        return wave(min(max(kch, 2), 4), False, 4, 0, False)
    return wave(min(max(kch, 2), 4), False, 2, 0, False)


def reachable_instances():
    """Every (instance, route) an admissible shape reaches, over n = 1 .. N_MAX, both batch regimes and spins."""
    out = set()
    for route, env in ROUTES.items():
        for n in range(1, N_MAX + 1):
            for nfrag in (1, 64):
                for uhf in (False, True):
                    out.add(instance_of(n, nfrag, uhf, env)[0])
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------
def _sym(A):
    L = np.tril(A)
    L += np.tril(A, -1).T
    return L


def exact_fragment(n, f, seed=20240):
    """Symmetric integer M in [-7, 7] and D in [-3, 3] of fragment f: every product and partial sum of J and K (and of
    the halved diagonal) is a multiple of 0.5 below 2^20 -- 6786 x 7 x 6 and 116^2 x 7 x 3 at n = 116 -- so the result
    is the same in any order of summation, fused or not, through atomics or not."""
    rng = np.random.default_rng([seed, n, f])
    np_ = npair(n)
    A = rng.integers(-7, 8, size=(np_, np_), dtype=np.int8)
    M = np.tril(A).astype(np.float64)
    M += np.tril(A, -1).T
    D = _sym(rng.integers(-3, 4, size=(n, n)).astype(np.float64))
    return M, D


def float_fragment(n, f, seed=777):
    """Normal deviates scaled over twelve decades, symmetric."""
    rng = np.random.default_rng([seed, n, f])
    np_ = npair(n)
    M = _sym(rng.standard_normal((np_, np_)) * 10.0 ** rng.uniform(-6.0, 6.0, size=(np_, np_)))
    D = _sym(rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-6.0, 6.0, size=(n, n)))
    return M, D


# ---- screening ----------------------------------------------------------------------------------------------------
Q_THRESH = 1.0e-6
Q_LIVE, Q_DEAD = 1.0, 2.0 ** -40        # live x max >= 1 or dead x max <= 2^-40: nothing near the threshold
SHELLS = {      # two "monomers" A | B, s shells outermost so that the first and the last pair row have a shell pair to themselves
    40: ([0, 0, 0, 0, 1, 1, 2, 2], [2, 2, 1, 1, 0, 0, 0, 0]),
    48: ([0, 0, 0, 1, 1, 2, 2, 2], [2, 2, 2, 1, 1, 0, 0, 0]),
}
PATTERNS = ("none", "cross", "third", "first", "last", "all")


def shell_l(n):
    a, b = SHELLS[n]
    return np.array(a + b, dtype=np.int32)


def shell_flags(n, pattern, f):
    """(ns, ns) symmetric: the shell pairs of fragment f whose pair rows are flagged as zero."""
    a, b = SHELLS[n]
    ns, na = len(a) + len(b), len(a)
    F = np.zeros((ns, ns), dtype=bool)
    if pattern == "cross":
        F[na:, :na] = True
    elif pattern == "third":
        rng = np.random.default_rng([99, n, f])
        F = np.tril(rng.random((ns, ns)) < 1.0 / 3.0)
    elif pattern == "first":
        F[0, 0] = True
    elif pattern == "last":
        F[ns - 1, ns - 1] = True
    elif pattern == "all":
        F[:, :] = True
    return F | F.T


def row_flags(n, F):
    """[npair] pair rows the kernel takes for zero: the shell pair of (k, l) is flagged."""
    ao2sh = np.repeat(np.arange(len(shell_l(n))), 2 * shell_l(n) + 1)
    k, l = np.tril_indices(n)
    return F[ao2sh[k], ao2sh[l]]


def screened(M, rz):
    """The kernel's precondition: the STORED part (columns <= row) of every flagged pair row is zero; the rest stays."""
    L = np.tril(M)
    L[rz, :] = 0.0
    return L + np.tril(L, -1).T


def expected_loaded(n, rz=None):
    """Chunks of 128 doubles a fragment's blocks are read in: [0, ceil(se / 128)) of every block, at most ten; a flagged
    long row drops the chunks wholly inside it, [0, sb / 128), a flagged short row those wholly behind the long one,
    from ceil(sb / 128) on; a block of two flagged rows is not read."""
    np_ = npair(n)
    _, sb, se, _ = tri_table(np_)
    total = 0
    for t in range((np_ + 1) // 2):
        rl = np_ - 1 - t
        zl = bool(rz[rl]) if rz is not None else False
        zs = (bool(rz[t]) if rz is not None else False) if t < rl else True
        if zl and zs:
            continue
        c0 = sb[t] // 128 if zl else 0
        c1 = -(-sb[t] // 128) if zs else -(-se[t] // 128)
        total += min(c1, TRI_MAXU2) - c0
    return total


# ---- the reference ------------------------------------------------------------------------------------------------
def jk_reference(M, D, flip=False):
    """J_ij = sum_kl (ij|kl) D_kl and K_ik = sum_jl (ij|kl) D_jl from the square pair matrix, in the dtype of M.
    J: the packed rows against (2 - delta_kl) D_kl.  K, row i at a time and without a four-index tensor: the n pair rows
    (ij), j = 0 .. n - 1, are summed over j against D[j, b] and D[j, a] at every packed column q = (a, b), a >= b --
    x_q = sum_j (ij|ab) D_jb belongs to K_ia, y_q = sum_j (ij|ab) D_ja (a != b) to K_ib -- and the columns are then
    gathered by a and by b.  flip: every sum runs in another order (exact inputs: bitwise the same)."""
    n = D.shape[0]
    p = pair_index(n)
    a, b = np.tril_indices(n)
    Dm = D.astype(M.dtype)
    Dp = np.where(a == b, 1, 2).astype(M.dtype) * Dm[a, b]
    J = (np.sum((M * Dp)[:, ::-1], axis=1) if flip else np.einsum("pq,q->p", M, Dp))[p]
    Db, Da = Dm[:, b], Dm[:, a] * (a != b).astype(M.dtype)
    X, Y = np.empty((n, len(a)), dtype=M.dtype), np.empty((n, len(a)), dtype=M.dtype)
    for i in range(n):
        R = M[p[i]]                                         # [j, q] = (ij|q)
        if flip:
            X[i], Y[i] = np.sum((R * Db)[::-1], axis=0), np.sum((R * Da)[::-1], axis=0)
        else:
            X[i], Y[i] = np.einsum("jq,jq->q", R, Db), np.einsum("jq,jq->q", R, Da)
    # gather the columns by a and by b; plain loops (np.add.at, einsum), no threaded library underneath
    K = np.zeros((n, n), dtype=M.dtype)
    if flip:
        np.add.at(K, (slice(None), b[::-1]), Y[:, ::-1])
        np.add.at(K, (slice(None), a[::-1]), X[:, ::-1])
    else:
        np.add.at(K, (slice(None), a), X)
        np.add.at(K, (slice(None), b), Y)
    return J, K


def jk_brute(M, D):
    """The four-index tensor filled element by element, then einsum (n <= 12)."""
    n = D.shape[0]
    eri = np.zeros((n, n, n, n), dtype=M.dtype)
    for i in range(n):
        for j in range(n):
            pij = max(i, j) * (max(i, j) + 1) // 2 + min(i, j)
            for k in range(n):
                for l in range(n):
                    eri[i, j, k, l] = M[pij, max(k, l) * (max(k, l) + 1) // 2 + min(k, l)]
    return np.einsum("ijkl,kl->ij", eri, D.astype(M.dtype)), np.einsum("ijkl,jl->ik", eri, D.astype(M.dtype))


def jk_bounds(M, D):
    """Elementwise bounds of a float64 evaluation in any order: m eps (|M| contracted with |D|), m the length of the
    sum -- npair for J, n^2 for K (a sum of m terms in any order, fused or not, is off by at most (m - 1) eps sum |terms|
    to first order, the products' own roundings included within m)."""
    n = D.shape[0]
    Ja, Ka = jk_reference(np.abs(M), np.abs(D))
    return npair(n) * EPS * Ja, n * n * EPS * Ka


# ---- cases --------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    route: str
    n: int
    nfrag: int
    uhf: bool = False
    kind: str = "exact"                  # exact | float
    pattern: str | None = None           # screening pattern (triangle only)
    done: tuple | None = None            # two sets of finished fragments, run one after the other (only_active)

    @property
    def name(self):
        return "n%d-m%d%s%s%s%s" % (self.n, self.nfrag, "-uhf" if self.uhf else "", "-float" if self.kind == "float" else "",
                                    "-q%s" % self.pattern if self.pattern else "", "-done" if self.done else "")

    @property
    def key(self):
        """What the inputs and the reference depend on (not the route, not the spin, not the finished fragments)."""
        return self.kind, self.n, self.nfrag, self.pattern

    @property
    def expect(self):
        return instance_of(self.n, self.nfrag, self.uhf, ROUTES[self.route])


def done_sets(nfrag):
    """About a third of the fragments finished, two different ways; some fragments run in both, some in one only."""
    a = tuple(f for f in range(nfrag) if f % 3 == 1)
    b = tuple(f for f in range(nfrag) if f % 3 == 2 or f == 0)
    return a, b


SMALL_N = (1, 2, 7, 8, 24, 25, 35, 36, 48, 49, 63, 64, 65, 66, 67, 89, 90)
BATCH_N = (24, 25, 35, 36, 39, 41, 47)


def _cases():
    c = []
    for n in SMALL_N:
        c += [Case("default", n, 1), Case("default", n, 3)]
    c.append(Case("default", N_MAX, 1))
    c += [Case("default", n, 64) for n in BATCH_N]
    for n in (40, 48):
        c += [Case("default", n, 64), Case("default", n, 64, uhf=True), Case("tri0", n, 64)]
        c += [Case(r, n, 64) for r in ("wg1", "wg5", "wg1000")]
        c += [Case(r, n, 64, pattern=p) for r in ("default", "wg1", "wg5", "wg1000") for p in PATTERNS]
    c.append(Case("default", 40, 65))
    for n in (67, 89):
        c += [Case("rowcoop0", n, 1), Case("rowcoop0", n, 3)]
    # float: one case per kernel family
    c += [Case("default", n, 3, kind="float") for n in (24, 25, 36, 49, 65, 67, 90)]
    c += [Case("default", 25, 64, kind="float"), Case("default", 41, 64, kind="float"), Case("default", 40, 64, kind="float"),
          Case("default", 40, 64, uhf=True, kind="float"), Case("rowcoop0", 67, 3, kind="float")]
    # only_active
    c += [Case("default", 25, 64, done=done_sets(64)), Case("default", 48, 64, done=done_sets(64)),
          Case("wg1", 48, 64, done=done_sets(64)), Case("default", 67, 3, done=((1,), (0,)))]
    return c


CASES = _cases()
BY_NAME = {(c.route, c.name): c for c in CASES}
assert len(BY_NAME) == len(CASES)
TIE_N, TIE_NFRAG = 48, 64


def route_cases(route):
    return [c for c in CASES if c.route == route]


def fragment_inputs(c, f):
    """(M, D) of fragment f of a case: the square pair matrix (screened cases: flagged rows zeroed as stored)."""
    M, D = (exact_fragment if c.kind == "exact" else float_fragment)(c.n, f)
    if c.pattern:
        M = screened(M, row_flags(c.n, shell_flags(c.n, c.pattern, f)))
    return M, D


def case_q(c):
    """[nfrag][ns][ns] bounds of a screened case: powers of two."""
    return np.stack([np.where(shell_flags(c.n, c.pattern, f), Q_DEAD, Q_LIVE) for f in range(c.nfrag)])


def case_tensor(c, layout):
    """The tensor as stored, (nfrag, stride), and the densities (nfrag, n, n)."""
    tri, _, stride = layout
    T = np.empty((c.nfrag, stride))
    D = np.empty((c.nfrag, c.n, c.n))
    for f in range(c.nfrag):
        M, D[f] = fragment_inputs(c, f)
        T[f] = tri_pack(M) if tri else M.reshape(-1)
    return T, D


def case_reference(c):
    """J, K (nfrag, n, n) of a case; float cases in np.longdouble with their bounds, exact cases in float64."""
    J, K = np.empty((c.nfrag, c.n, c.n)), np.empty((c.nfrag, c.n, c.n))
    bj, bk = (np.empty_like(J), np.empty_like(K)) if c.kind == "float" else (None, None)
    for f in range(c.nfrag):
        M, D = fragment_inputs(c, f)
        if c.kind == "float":
            Jl, Kl = jk_reference(M.astype(np.longdouble), D.astype(np.longdouble))
            J[f], K[f] = Jl.astype(np.float64), Kl.astype(np.float64)
            bj[f], bk[f] = jk_bounds(M, D)
        else:
            J[f], K[f] = jk_reference(M, D)
    return J, K, bj, bk


def tie_densities(n, nfrag):
    return np.stack([exact_fragment(n, f, seed=4711)[1] for f in range(nfrag)])
