"""Host checks of tests/xc_stage_cases.py: every dispatch bucket of the quadrature has a case that lands in it, and the
densities the cases use are ones a quadrature can take.  No GPU.

`python -m tests.test_xc_stage_cases [case ...]` prints the reference's own noise floor per case (measure_eps_ref), the
figures behind xc_stage_cases.EPS_REF_*."""
import numpy as np
import pytest

from oracle import scf_oracle as so
from tests import xc_stage_cases as xs
from tests.helpers import oracle_mol


def _loaded(case):
    frag = xs.fragment(case)
    mol = oracle_mol(case.basis, frag)
    return frag, mol, int(max(mol.sh_l))


@pytest.mark.parametrize("case", xs.CASES, ids=lambda c: c.name)
def test_case_lands_in_its_bucket(case):
    frag, mol, lmax = _loaded(case)
    n = mol.nao
    assert n == case.n
    assert frag.n_atoms <= 64
    assert xs.bucket_of(case, n, lmax) == case.bucket
    # the rules themselves, recomputed here from kern_xc.hip's expressions
    nt, nv, jobs = -(-n // 16), -(-n * n // 256), -(-(-(-n // 16)) ** 2 // 4)
    assert (nt, nv, jobs) == (xs.nt_of(n), xs.nv_of(n), xs.jobs_of(n))
    b = case.bucket
    if b.startswith("split"):
        assert n <= 96 and not case.unrestricted and str(nt) in b and (("f" in b.split("nt")[1]) == (lmax == 3))
        assert not (lmax == 3 and nt <= 2)
    elif b.startswith("tile"):
        assert n > 96 and n <= 256 and not case.unrestricted
        want = {"j16": 9 < jobs <= 16, "j21": 16 < jobs <= 21, "z2": jobs > 21 and -(-nt * nt // 64) == 2,
                "z4": jobs > 21 and -(-nt * nt // 64) == 4}[b.split("-")[-1]]
        assert want
        if "rsh" in b:
            assert n <= 116
    else:
        assert case.unrestricted or case.functional == "tpss"
        assert n <= 140
        lo, hi = {10: (0, 10), 29: (10, 29), 54: (29, 54), 77: (54, 77)}[int(b.split("nv")[1])]
        assert lo < nv <= hi
    if case.unrestricted:
        na, nb = xs.occupations(case, frag)
        assert na != nb and na + nb == frag.nelec and frag.multiplicity == 2
    assert case.functional != "tpss" or n <= 140


def test_every_bucket_has_a_case():
    have = {c.bucket for c in xs.CASES}
    assert have == set(xs.REQUIRED_BUCKETS)
    # the sizes the issue names: both edges of the split path, 144 and a neighbour that is no multiple of 16, 147, 240
    sizes = {c.n for c in xs.CASES if not c.unrestricted and c.functional in ("svwn", "pbe", "b3lyp")}
    assert {7, 24, 48, 43, 52, 55, 72, 67, 86, 96, 120, 144, 143, 147, 240} <= sizes
    assert any(c.level == 3 for c in xs.CASES) and any(c.diffuse for c in xs.CASES)
    # range-separated hybrids stop at n = 116 (validate_options): nt = 8 there, so the jobs <= 21 tile cannot be reached
    assert xs.jobs_of(116) <= 16


def test_routes_cover_their_kernels():
    for route in xs.ROUTES:
        assert xs.route_cases(route), route
    assert {xs.nt_of(c.n) for c in xs.route_cases("narrow-tile")} == {5, 6}
    assert {xs.nt_of(c.n) for c in xs.route_cases("tile")} == {1, 2, 3, 4, 5, 6}
    assert all(c.n <= 64 for c in xs.route_cases("pipe"))
    assert any(c.functional in ("wb97x", "cam-b3lyp") for c in xs.route_cases("tile"))      # the jobs <= 9 RSH tile
    assert "MQC_HIP_XC_PROBE" not in str(xs.ROUTES)


@pytest.mark.parametrize("case", xs.CASES, ids=lambda c: c.name)
def test_density_is_one_a_quadrature_can_take(case):
    frag, mol, _ = _loaded(case)
    S, _, _ = so.int1e(mol)
    D, C = xs.density(case, frag, S, mol)
    occ = xs.occupations(case, frag)
    w, U = np.linalg.eigh(S)
    Sh = (U * np.sqrt(w)) @ U.T
    for d, ne in zip(D if case.unrestricted else [D], occ if case.unrestricted else [frag.nelec]):
        assert np.array_equal(d, d.T)
        assert abs(np.sum(d * S) - ne) < 1e-12                               # tr(D S) = electrons of this spin
        ev = np.linalg.eigvalsh(Sh @ d @ Sh)                                 # positive semidefinite in the S metric
        assert ev.min() > -1e-12 and abs(ev.max() - (1.0 if case.unrestricted else 2.0)) < 1e-11
    assert np.max(np.abs(C.T @ S @ C - np.eye(mol.nao))) < 1e-11
    if case.diffuse:
        mu = xs.most_diffuse_ao(mol)
        c0 = C[:, 0] / C[mu, 0]
        assert np.max(np.abs(np.delete(c0, mu))) < 1e-10                     # orbital 0 is the loosest function alone


def test_low_density_points_carry_no_weight():
    """Issue section 5: points the oracle places within a factor 10 of DENS_THRESHOLD may fall on either side of it in
    the kernel, and may be masked if their quadrature weight stays below 1e-12 of the total.  It does not: they are the
    outermost radial shells, whose weights 4 pi r^2 dr are the largest of the grid.  So the GPU test masks NO point.  What
    makes that sound is checked here with the reference alone: those points carry rho <= 1e-19, their whole contribution
    to N_e is below 1e-12 of it (and to E_xc and V_xc smaller still: f ~ rho^(4/3)), whichever side of the threshold the
    kernel puts them on."""
    from oracle import xc_oracle
    for name in ("w1-dz-pbe", "oh-dz-upbe", "w1-tz-b3lyp"):
        case = xs.BY_NAME[name]
        frag, mol, _ = _loaded(case)
        S, _, _ = so.int1e(mol)
        D, _ = xs.density(case, frag, S, mol)
        ref = xs.oracle_for(case, mol)
        ao = so.eval_ao(mol, ref.pts)
        dt = D[0] + D[1] if case.unrestricted else D
        rho = np.einsum("pi,pi->p", ao @ dt, ao)
        assert rho.min() > -1e-14
        near = (rho > 0.1 * xc_oracle.DENS_THRESHOLD) & (rho < 10.0 * xc_oracle.DENS_THRESHOLD)
        assert np.sum(ref.w[near] * rho[near]) < 1e-12 * np.sum(ref.w * rho)


def measure_eps_ref(case, ld_block=1):
    """The reference's own noise floor for one case: -> (eps_V, eps_E, eps_N, max |V|).  block = 4096 against
    block = 509 (another summation order) and against an evaluation whose accumulations over the grid run in
    np.longdouble: ld_block = 1 hands the reference one point at a time, so that every sum over points -- E_xc, N_e and
    each element of V_xc -- is formed here in extended precision from single-point terms (what stays in double is the
    arithmetic at a point).  A larger ld_block (the large cases from __main__) keeps double sums inside its blocks."""
    frag, mol, _ = _loaded(case)
    S, _, _ = so.int1e(mol)
    D, _ = xs.density(case, frag, S, mol)
    e0, n0, v0 = xs.reference(case, xs.oracle_for(case, mol, 4096), D)
    e1, n1, v1 = xs.reference(case, xs.oracle_for(case, mol, 509), D)
    ref = xs.oracle_for(case, mol, ld_block)
    pts, w = ref.pts, ref.w
    el, nl, vl = np.longdouble(0), np.longdouble(0), np.zeros(v0.shape, dtype=np.longdouble)
    for b0 in range(0, len(w), ld_block):
        ref.pts, ref.w = pts[b0:b0 + ld_block], w[b0:b0 + ld_block]
        e, nn, v = xs.reference(case, ref, D)
        el += np.longdouble(e); vl += v.astype(np.longdouble)
        nl += np.longdouble(nn)
    ev = max(np.max(np.abs(v0 - v1)), float(np.max(np.abs(v0 - vl))))
    ee = max(abs(e0 - e1), abs(float(e0 - el)))
    en = max(abs(n0 - n1), abs(float(n0 - nl)))
    return ev, ee, en, float(np.max(np.abs(v0)))


# the recorded eps_ref holds for the cases it was measured on.  Here the small ones with 16 points per longdouble block
# (seconds); __main__ takes one point per block up to n = 24 (40 s a case) and prints every case
@pytest.mark.parametrize("name", ["w1-dz-svwn", "w1-dz-pbe", "w1-dz-tpss", "oh-dz-ub3lyp", "w1-dz-wb97x", "w1-dz-cam-b3lyp"])
def test_recorded_noise_floor_holds(name):
    case = xs.BY_NAME[name]
    ev, ee, en, _ = measure_eps_ref(case, 16)
    cls = xs.case_class(case)
    assert ev <= xs.EPS_REF_V[cls] and ee <= xs.EPS_REF_E[cls] and en <= xs.EPS_REF_N


if __name__ == "__main__":
    import sys
    for c in (xs.BY_NAME[a] for a in sys.argv[1:]) if len(sys.argv) > 1 else xs.CASES:
        ev, ee, en, vm = measure_eps_ref(c, 1 if c.n <= 24 else 127)
        print("%-22s %-5s n=%3d  eps_V %.1e  eps_E %.1e  eps_N %.1e  max|V| %.2f" % (c.name, xs.case_class(c), c.n, ev, ee, en, vm), flush=True)
