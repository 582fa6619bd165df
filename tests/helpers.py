"""Shared helpers for the parity tests: build the same fragment for the engine and the oracle."""
import numpy as np

from metalquicha_amd.basis import build_flat_basis
from metalquicha_amd.methods import PhysicalFragment
from oracle import scf_oracle as so

W1_ANGSTROM = [[0.0, 0.00000000009155, 0.10077199490609],
               [0.0, 0.77250895271063, -0.46780199741728],
               [0.0, -0.77250895280218, -0.46780199748881]]   # validation/inputs/sample_inputs/w1.xyz


def fragment_bohr(Z, xyz_bohr, **kw) -> PhysicalFragment:
    return PhysicalFragment(np.array(Z), np.asarray(xyz_bohr, dtype=float).reshape(-1, 3).T.copy(), **kw)


def oracle_mol(basis: str, frag: PhysicalFragment):
    fb = build_flat_basis(basis, frag.element_numbers, allow_cartesian=True)
    return so.make_mol(frag.element_numbers, frag.coordinates.T, fb.nshell_per_atom, fb.shell_l, fb.shell_nprim,
                       fb.exps, fb.coefs, ghost=frag.ghost, cart=not fb.spherical)


def random_rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a*a+b*b-c*c-d*d, 2*(b*c-a*d), 2*(b*d+a*c)],
                     [2*(b*c+a*d), a*a-b*b+c*c-d*d, 2*(c*d-a*b)],
                     [2*(b*d-a*c), 2*(c*d+a*b), a*a-b*b-c*c+d*d]])


def water_at(rng, centre_bohr):
    from metalquicha_amd.basis import ANGSTROM_TO_BOHR
    w = np.array(W1_ANGSTROM) * ANGSTROM_TO_BOHR
    R = random_rotation(rng)
    return (w - w.mean(axis=0)) @ R.T + np.asarray(centre_bohr)


def synthetic_density(n):
    """The reference's direct-vs-in-core test density sin(0.7 i + 1.3 j) + transpose
    (test/test_mqc_libcint_direct.f90:59-102), made symmetric."""
    i, j = np.meshgrid(np.arange(1, n + 1), np.arange(1, n + 1), indexing="ij")
    d = np.sin(0.7 * i + 1.3 * j)
    return 0.5 * (d + d.T)


def most_diffuse_ao(mol):
    """Index of the first function of the shell whose tightest primitive is the loosest of the basis."""
    tight = [np.max(mol.exps[p:p + k]) for p, k in zip(mol.sh_poff, mol.sh_nprim)]
    return int(mol.sh_aoff[int(np.argmin(tight))])


def orthonormal_orbitals(S, seed, diffuse_ao=None):
    """C = S^{-1/2} Q, Q from the QR factorisation of a seeded normal matrix: C^T S C = 1, none of the molecule's
    symmetry (symmetry hides swapped indices).  diffuse_ao = mu: the first column of that matrix is S^{1/2} e_mu, so
    that orbital 0 is the basis function mu alone -- with most_diffuse_ao, an orbital that puts many grid points at
    small rho, where v_sigma is large."""
    n = S.shape[0]
    w, U = np.linalg.eigh(S)
    M = np.random.default_rng(seed).normal(size=(n, n))
    if diffuse_ao is not None:
        M[:, 0] = ((U * w ** 0.5) @ U.T)[:, diffuse_ao]
    Q, _ = np.linalg.qr(M)
    return (U * w ** -0.5) @ U.T @ Q


def quadrature_density(C, nocc):
    """Densities an exchange-correlation quadrature can take (synthetic_density is indefinite: rho < 0 at points), from
    orthonormal orbitals C.  nocc an integer: restricted, D = 2 C_occ C_occ^T.  nocc = (n_alpha, n_beta): the spin
    densities C_occ,s C_occ,s^T of the leading columns of the same C, stacked (2, n, n).  rho >= 0 everywhere and
    tr(D S) is the electron number; nothing is converged."""
    def proj(k):
        p = C[:, :k] @ C[:, :k].T
        return 0.5 * (p + p.T)          # a blocked matrix product is symmetric to rounding only
    if isinstance(nocc, (tuple, list)):
        return np.stack([proj(k) for k in nocc])
    return 2.0 * proj(nocc)


# ---- recorded oracle results ------------------------------------------------------------------------------------------
# The handful of oracle SCFs that take a minute or more of numpy time each (benzene DF-B3LYP, the 147-function cluster,
# def2-TZVP dimers ...) are stored as fixtures: tests/golden/oracle_fixtures.json holds energy and iteration count per
# (label, geometry, settings) key, written by these very tests when run with MQC_ORACLE_RECORD=<file> (the oracle then
# runs live and its results are appended to <file>; copy it over the fixture).  MQC_ORACLE_LIVE=1 ignores the fixture
# and runs the oracle, as every other parity test does.  A changed geometry or setting changes the key: a stale fixture
# cannot be picked up silently -- the oracle runs live instead.
import hashlib as _hashlib
import json as _json
import os as _os

_FIXTURE_PATH = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "golden", "oracle_fixtures.json")
_FIXTURES = None


def _fixture_key(label, frag, settings_text):
    h = _hashlib.sha1()
    h.update(np.ascontiguousarray(frag.element_numbers, dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(np.round(np.asarray(frag.coordinates, dtype=float), 12)).tobytes())
    if frag.ghost is not None:
        h.update(np.ascontiguousarray(frag.ghost, dtype=np.uint8).tobytes())
    h.update(("%d|%d|%s" % (frag.charge, frag.multiplicity, settings_text)).encode())
    return "%s#%s" % (label, h.hexdigest()[:16])


def recorded_oracle(label, frag, settings_text, compute):
    """-> {"energy": float, "iterations": int, ...}: from the committed fixture when its key is there, else compute()."""
    global _FIXTURES
    if _FIXTURES is None:
        _FIXTURES = _json.load(open(_FIXTURE_PATH)) if _os.path.isfile(_FIXTURE_PATH) else {}
    key = _fixture_key(label, frag, settings_text)
    if key in _FIXTURES and _os.environ.get("MQC_ORACLE_LIVE") != "1" and not _os.environ.get("MQC_ORACLE_RECORD"):
        return _FIXTURES[key]
    out = compute()
    rec = _os.environ.get("MQC_ORACLE_RECORD")
    if rec:
        cur = _json.load(open(rec)) if _os.path.isfile(rec) else {}
        cur[key] = out
        with open(rec, "w") as f:
            _json.dump(cur, f, indent=1, sort_keys=True)
    return out


def scf_record(o):
    return {"energy": float(o.energy), "iterations": int(o.iterations), "converged": bool(o.converged)}



# ---- FMO / EE-MBE (point-charge embedding) -------------------------------------------------------------------------
W3_ANGSTROM = np.array([[0, 0, 0], [0, -0.7572, 0.5865], [0, 0.7572, 0.5865],
                        [0, 0, 2.9], [0, -0.7572, 3.4865], [0, 0.7572, 3.4865],
                        [0, 0, 5.8], [0, -0.7572, 6.3865], [0, 0.7572, 6.3865]], dtype=float)
EEMBE_W3_GOLDEN = -227.9704573337      # manifest row "EE-MBE water trimer 6-31g (CPU)", validation_tests_cpu.json:2194-2198
FMO3_W3_GOLDEN = -227.970497639        # rows "FMO3 / EE-MBE3 water trimer 6-31g, exact at full level (CPU)", :2200-2210
FMO2_W3_GOLDEN = -227.9705411684       # manifest row "FMO2 water trimer 6-31g (CPU)", validation_tests_cpu.json:2188-2192


def w3_system():
    """The reference's three stacked waters (validation/inputs/sample_inputs/w3.xyz), fragments = molecules."""
    from metalquicha_amd import mbe
    return mbe.system_from_xyz(["O", "H", "H"] * 3, W3_ANGSTROM, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])


def oracle_make_mol(system, basis):
    z = np.asarray(system.element_numbers); xyz = np.ascontiguousarray(system.coordinates.T)

    def make(atoms):
        atoms = list(atoms)
        fb = build_flat_basis(basis, z[atoms], allow_cartesian=True)
        return so.make_mol(z[atoms], xyz[atoms], fb.nshell_per_atom, fb.shell_l, fb.shell_nprim, fb.exps, fb.coefs,
                           cart=not fb.spherical)
    return make


def oracle_fmo_solver(system, basis, e_tol=1e-9, d_tol=1e-7, max_iter=100):
    """The CPU oracle behind fmo.run_fmo2's solver interface: lets the host logic be checked without a GPU."""
    from metalquicha_amd.fmo import EmbeddedResult
    make = oracle_make_mol(system, basis)
    z = np.asarray(system.element_numbers); xyz = np.ascontiguousarray(system.coordinates.T)

    def solve(jobs):
        out = []
        for job in jobs:
            mol = make(job.atoms)
            u = so.point_charge_potential(mol, xyz[list(job.field_atoms)], job.field_charges) if len(job.field_atoms) else None
            if job.h_extra is not None:
                u = job.h_extra if u is None else u + job.h_extra
            r = so.run_rhf(mol, int(np.sum(z[list(job.atoms)])), max_iter=max_iter, e_tol=e_tol, d_tol=d_tol, guess="gwh", h_extra=u)
            S, _, _ = so.int1e(mol)
            out.append(EmbeddedResult(r.energy, float(np.sum(r.D * u)) if u is not None else 0.0, r.iterations, r.D,
                                      so.mulliken_charges(mol, r.D, S), u))
        return out
    return solve


def oracle_cross_coulomb(system, basis):
    """J[D_K] of a neighbour's electrons in the basis of `atoms`, from the oracle's four-centre integrals (the batch
    interface of fmo.Coulomb)."""
    make = oracle_make_mol(system, basis)

    def coulomb(requests):
        out = []
        for atoms, other, d_other in requests:
            sup = make(list(atoms) + list(other))
            n0 = sup.nao - d_other.shape[0]
            out.append(np.einsum("ijkl,kl->ij", so.eri4(sup)[:n0, :n0, n0:, n0:], d_other))
        return out
    return coulomb
