"""Probe cases for the integral stage: synthetic basis sets and four-centre geometries on which every canonical ERI
class (la lb|lc ld) occurs on four distinct centres, in every shell order, with odd-x components that do not vanish.

The standard sets list shells s, p, d, f on every atom and the stage tests use planar water, so which canonical swap a
quartet needs, and whether a class is ever seen away from one centre, is an accident of the basis file.  Here it is
a construction:

  mqc-class-probe-spd   H: d s s p | C: p d s s | N: s p s d | O: s d p s      (n_ao = 40: a multiple of 8 within 36..64,
                        so a batch of 64 or more takes the triangular tensor and jk_tri_kernel)
  mqc-class-probe-spdf  the same with one f shell per element, in a different place on each (n_ao = 68)

Every l has shells of contraction depth 1, 2 and 3 (f: 1 and 2).  The two s shells of C are the two rows of one general
contraction over three primitives (a twin pair for the engine); the two consecutive s shells of H have the same depth
but different primitives, those of N and O are apart in the file (not twins).  Exponents run from 0.11 to 71.

Nothing here was tuned after a look at the references: exponents and geometries are as first written.

Test infrastructure: no GPU needed, never imported by the package."""
from __future__ import annotations

import json
import os

import numpy as np

from tests.helpers import fragment_bohr, random_rotation

SPD = "mqc-class-probe-spd"
SPDF = "mqc-class-probe-spdf"
ELEMENTS = [1, 6, 7, 8]


def _sh(l, exps, *rows):
    rows = rows or ([1.0] * len(exps),)         # an uncontracted shell needs no coefficients spelled out
    return {"function_type": "gto", "angular_momentum": [l], "exponents": ["%.10E" % e for e in exps],
            "coefficients": [["%.10E" % c for c in row] for row in rows]}


# per element: shells in FILE order.  _F marks where the f shell of the spdf set goes.
_F = "f"
_LAYOUT = {
    # two consecutive s shells of equal depth over DIFFERENT primitives: not a twin pair
    1: [_sh(2, [0.85]), _F, _sh(0, [5.4, 0.82], [0.16, 0.90]), _sh(0, [1.9, 0.13], [0.22, 0.85]), _sh(1, [1.1])],
    6: [_sh(1, [18.7, 3.9, 0.61], [0.04, 0.24, 0.82]), _sh(2, [2.3, 0.55], [0.35, 0.75]),
        # one general contraction, two rows over the same three primitives: two consecutive s shells, a twin pair
        _sh(0, [71.0, 10.6, 1.9], [0.07, 0.39, 0.68], [-0.03, -0.11, 0.95]), _F],
    7: [_sh(0, [0.29]), _sh(1, [6.1, 0.47], [0.13, 0.93]), _F, _sh(0, [58.0, 8.7, 0.93], [0.06, 0.36, 0.71]),
        _sh(2, [9.5, 1.8, 0.36], [0.08, 0.42, 0.70])],
    8: [_F, _sh(0, [33.0, 2.6], [0.20, 0.86]), _sh(2, [0.15]), _sh(1, [0.11]), _sh(0, [0.62])],
}
_FSHELL = {1: _sh(3, [0.70]), 6: _sh(3, [1.9, 0.45], [0.40, 0.72]), 7: _sh(3, [1.3]), 8: _sh(3, [0.31])}


def write_basis_files(directory) -> None:
    """mqc-class-probe-spd.json and mqc-class-probe-spdf.json into `directory` (point MQC_BASIS_PATH at it)."""
    for name, with_f in ((SPD, False), (SPDF, True)):
        doc = {"name": name, "elements": {}}
        for z, layout in _LAYOUT.items():
            shells = [(_FSHELL[z] if s is _F else s) for s in layout if with_f or s is not _F]
            doc["elements"][str(z)] = {"electron_shells": shells}
        with open(os.path.join(str(directory), name + ".json"), "w") as f:
            json.dump(doc, f, indent=1)


# ---- geometries (Bohr), atoms in the order of ELEMENTS --------------------------------------------------------------
GENERIC = np.array([[0.31, -0.52, 0.73],
                    [1.62, 0.44, -0.27],
                    [-0.71, 1.33, -0.95],
                    [0.88, -1.47, -1.38]])
# the oxygen moved out along a direction with three different non-zero components: 8.0 .. 9.7 Bohr from the others
STRETCHED = GENERIC.copy()
STRETCHED[3] = [5.1, -5.6, -4.3]


def generic():
    return fragment_bohr(ELEMENTS, GENERIC)


def stretched():
    return fragment_bohr(ELEMENTS, STRETCHED)


def jitter_xyz(k: int) -> np.ndarray:
    rng = np.random.default_rng(7000 + k)
    R = random_rotation(rng)
    return (GENERIC - GENERIC.mean(axis=0)) @ R.T + rng.uniform(-0.05, 0.05, size=(4, 3))


def jitter(k: int):
    """`generic` under a seeded rigid rotation (about its centroid) plus uniform noise of up to 0.05 Bohr per coordinate."""
    return fragment_bohr(ELEMENTS, jitter_xyz(k))


def sharing_batch():
    """24 fragments in three groups of 8: H and C keep bit-identical coordinates inside a group (the engine shares the
    blocks of atom sets that repeat at least 6 times), N and O move by up to 0.05 Bohr per coordinate."""
    frags = []
    for g in range(3):
        base = jitter_xyz(100 + g)
        for m in range(8):
            xyz = base.copy()
            xyz[2:] += np.random.default_rng(7200 + 8 * g + m).uniform(-0.05, 0.05, size=(2, 3))
            frags.append(fragment_bohr(ELEMENTS, xyz))
    return frags


CASES = {"generic": generic, "stretched": stretched}


def sparse_density(n: int, seed: int) -> np.ndarray:
    """Symmetric D with 8 non-zero pairs (k >= l), |D_kl| <= 1: J[D] and K[D] then read single columns of the tensor,
    and an elementwise error e of the tensor bounds their error by e * sum |D| (<= 16 e)."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    pairs = set()
    while len(pairs) < 8:
        k, l = sorted((int(rng.integers(n)), int(rng.integers(n))), reverse=True)
        pairs.add((k, l))
    for k, l in sorted(pairs):
        v = rng.uniform(0.25, 1.0) * rng.choice([-1.0, 1.0])
        D[k, l] = v
        D[l, k] = v
    return D


# ---- canonical classes ------------------------------------------------------------------------------------------------
def shell_atoms(mol) -> np.ndarray:
    return np.array([int(np.argmin(np.sum((mol.xyz - c) ** 2, axis=1))) for c in mol.sh_xyz])


def _pclass(la, lb):
    return la * (la + 1) // 2 + lb


def class_name(cid: int) -> str:
    l = "spdfgh"
    return "(%s%s|%s%s)" % (l[cid // 512], l[(cid // 64) % 8], l[(cid // 8) % 8], l[cid % 8])


def canonical_class_ids(lmax: int):
    """The la >= lb, lc >= ld, bra >= ket classes up to lmax: 21 for lmax = 2, 55 for lmax = 3."""
    pairs = [(a, b) for a in range(lmax + 1) for b in range(a + 1)]
    return sorted(((a * 8 + b) * 8 + c) * 8 + d for (a, b) in pairs for (c, d) in pairs if _pclass(a, b) >= _pclass(c, d))


def quartet_table(mol):
    """The engine's canonicalisation (host_setup.cpp, `canonical quartets`) restated: every unique shell quartet
    (pair ab >= pair cd by index) -> rows (class id, distinct centres, bra swapped, ket swapped, bra and ket exchanged),
    where `bra` and `ket` are the pairs as the class kernel receives them."""
    l = [int(x) for x in mol.sh_l]
    at = shell_atoms(mol)
    ns = len(l)
    pl = []
    for A in range(ns):
        for B in range(A + 1):
            sw = l[A] < l[B]
            a, b = (B, A) if sw else (A, B)
            pl.append((a, b, l[a], l[b], _pclass(l[a], l[b]), sw))
    rows = []
    for ij in range(len(pl)):
        for kl in range(ij + 1):
            bra, ket = pl[ij], pl[kl]
            ex = bra[4] < ket[4]
            if ex:
                bra, ket = ket, bra
            cid = ((bra[2] * 8 + bra[3]) * 8 + ket[2]) * 8 + ket[3]
            ncen = len({at[bra[0]], at[bra[1]], at[ket[0]], at[ket[1]]})
            rows.append((cid, ncen, bra[5], ket[5], ex))
    return np.array(rows, dtype=np.int64)


def class_of_elements(mol):
    """For the packed pair matrix M[pair(i,j), pair(k,l)] of `mol`: (class id, number of distinct centres), two
    integer arrays of M's shape.  class_name(id) spells the class."""
    nf = 2 * np.asarray(mol.sh_l) + 1
    ao_sh = np.repeat(np.arange(mol.nshell), nf)
    at = shell_atoms(mol)
    n = mol.nao
    ii, jj = np.tril_indices(n)            # row-major over i >= j: pair(i, j) = i (i + 1) / 2 + j
    li, lj = np.asarray(mol.sh_l)[ao_sh[ii]], np.asarray(mol.sh_l)[ao_sh[jj]]
    la, lb = np.maximum(li, lj), np.minimum(li, lj)
    pc = la * (la + 1) // 2 + lb
    code = la * 8 + lb
    bra_first = pc[:, None] >= pc[None, :]
    cid = np.where(bra_first, code[:, None] * 64 + code[None, :], code[None, :] * 64 + code[:, None])
    a1, a2 = at[ao_sh[ii]], at[ao_sh[jj]]
    npair = len(ii)
    four = np.stack([np.broadcast_to(a1[:, None], (npair, npair)), np.broadcast_to(a2[:, None], (npair, npair)),
                     np.broadcast_to(a1[None, :], (npair, npair)), np.broadcast_to(a2[None, :], (npair, npair))]).astype(np.int8)
    four = np.sort(four, axis=0)
    ncen = 1 + np.sum(four[1:] != four[:-1], axis=0)
    return cid, ncen


def error_report(err, cid, ncen):
    """Maximum of `err` (packed-matrix shape) per (class, centre count), worst first: [(name, centres, max error)]."""
    key = cid.astype(np.int64) * 8 + ncen
    flat, e = key.ravel(), np.abs(err).ravel()
    order = np.argsort(flat, kind="stable")
    uk, start = np.unique(flat[order], return_index=True)
    mx = np.maximum.reduceat(e[order], start)
    out = [(class_name(int(k) // 8), int(k) % 8, float(m)) for k, m in zip(uk, mx)]
    return sorted(out, key=lambda r: -r[2] if r[2] == r[2] else -np.inf)


def format_report(rep, top=8):
    return "; ".join("%s on %d centres: %.2e" % r for r in rep[:top])


# ---- the numpy reference in child processes ---------------------------------------------------------------------------
# rr.eri4_erf is a Python loop over shell quartets: about ten seconds for the spd probe and a minute for the spdf one.
# The tensors of several (basis, case, omega) jobs are formed side by side in CPU-only children and come back packed.
_REFERENCE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import integral_class_cases as cc, range_separated_reference as rr, stages
from tests.helpers import oracle_mol
basis, case, omega, out = sys.argv[2], sys.argv[3], float(sys.argv[4]), sys.argv[5]
np.save(out, stages.pack_eri(rr.eri4_erf(oracle_mol(basis, cc.CASES[case]()), omega if omega > 0.0 else None)))
"""


def numpy_reference_packed(basis_dir, out_dir, jobs, workers=8, timeout=1500):
    """jobs: [(basis, case, omega or 0.0 for the Coulomb operator)] -> {job: packed rr.eri4_erf tensor}.  At most
    `workers` children at a time; a child that fails or overruns `timeout` seconds raises."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MQC_BASIS_PATH=str(basis_dir), OMP_NUM_THREADS="2")
    todo = list(enumerate(jobs))
    running, out = [], {}
    t0 = time.time()
    try:
        while todo or running:
            while todo and len(running) < workers:
                k, job = todo.pop(0)
                path = os.path.join(str(out_dir), "reference_%d.npy" % k)
                p = subprocess.Popen([sys.executable, "-c", _REFERENCE_CHILD, root, job[0], job[1], repr(float(job[2])), path], env=env)
                running.append((p, job, path))
            for item in list(running):
                p, job, path = item
                if p.poll() is None:
                    continue
                running.remove(item)
                if p.returncode != 0:
                    raise RuntimeError("reference child for %r ended with status %d" % (job, p.returncode))
                out[tuple(job)] = np.load(path)
                os.remove(path)
            if time.time() - t0 > timeout:
                raise RuntimeError("reference children overran %d s" % timeout)
            time.sleep(0.2)
    finally:
        for p, _, _ in running:
            p.kill()
    return out
