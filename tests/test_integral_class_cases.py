"""CPU checks of the integral-class probe cases (tests/integral_class_cases.py) and of the references the GPU tests
compare with.  Nothing here touches a GPU.

What is asserted:
  * the probe bases contain what they were built for: all 21 (s-d) / 55 (s-f) canonical classes, each with a quartet on
    four distinct centres and with every kind of canonical swap the class admits; twin and non-twin s pairs; contraction
    depths; exponent range; the geometry conditions;
  * on `generic` every class but (ss|ss), which has none, has a component of odd x parity above 1e-6 (on planar water all
    of them vanish);
  * the C oracle (so.eri4) and the numpy McMurchie-Davidson code (rr.eri4_erf(mol, None)) agree to 1e-12 on every
    element of both bases on `generic` and `stretched`.  Measured when this was written: 2e-15 at most, in all four
    cases, so the 1e-11 of the GPU comparison is not spent on reference noise.  No case had to be softened;
  * both Boys functions against mpmath at 40 digits, relative 1e-13.  Measured: see test_boys_functions_against_mpmath."""
import ctypes

import numpy as np
import pytest

from oracle import scf_oracle as so
from tests import integral_class_cases as cc
from tests import range_separated_reference as rr
from tests import stages
from tests.helpers import oracle_mol

BASES = [(cc.SPD, 2, 21, 40), (cc.SPDF, 3, 55, 68)]


@pytest.fixture
def probe_dir(tmp_path, monkeypatch):
    cc.write_basis_files(tmp_path)
    monkeypatch.setenv("MQC_BASIS_PATH", str(tmp_path))
    return tmp_path


def test_geometries_are_generic():
    for name, xyz in (("generic", cc.GENERIC), ("stretched", cc.STRETCHED), ("jitter(3)", cc.jitter_xyz(3))):
        assert np.all(xyz != 0.0), name
        for d in range(3):
            assert len(set(xyz[:, d])) == 4, name                              # no two atoms share a coordinate
        for i in range(4):
            for j in range(i):
                for k in range(j):
                    assert np.linalg.norm(np.cross(xyz[j] - xyz[i], xyz[k] - xyz[i])) > 0.5, name   # not collinear
        assert abs(np.linalg.det(xyz[1:] - xyz[0])) > 1.0, name                # not coplanar
    dist = np.linalg.norm(cc.GENERIC[:, None] - cc.GENERIC[None], axis=2) + 100.0 * np.eye(4)
    assert np.all((dist.min(axis=1) >= 1.3) & (dist.min(axis=1) <= 3.0))
    far = np.linalg.norm(cc.STRETCHED[:3] - cc.STRETCHED[3], axis=1)
    assert np.all((far >= 8.0) & (far <= 10.0))
    assert np.array_equal(cc.STRETCHED[:3], cc.GENERIC[:3])
    # jitter: a rigid motion plus at most 0.05 Bohr per coordinate, seeded
    a, b = cc.jitter_xyz(5), cc.jitter_xyz(5)
    assert np.array_equal(a, b) and not np.array_equal(a, cc.jitter_xyz(6))
    da = np.linalg.norm(a[:, None] - a[None], axis=2)
    dg = np.linalg.norm(cc.GENERIC[:, None] - cc.GENERIC[None], axis=2)
    assert np.max(np.abs(da - dg)) < 2 * 0.05 * np.sqrt(3) + 1e-12
    # the block-sharing batch: H and C bit-identical inside a group of 8, N and O different in every fragment
    sh = cc.sharing_batch()
    assert len(sh) == 24
    for g in range(3):
        grp = [f.coordinates.T for f in sh[8 * g: 8 * g + 8]]
        assert all(np.array_equal(x[:2], grp[0][:2]) for x in grp)
        assert len({x[2:].tobytes() for x in grp}) == 8
    assert not np.array_equal(sh[0].coordinates, sh[8].coordinates)


@pytest.mark.parametrize("basis,lmax,nclass,nao", BASES)
def test_probe_basis_contents(probe_dir, basis, lmax, nclass, nao):
    mol = oracle_mol(basis, cc.generic())
    assert mol.nao == nao and not mol.cart
    at = cc.shell_atoms(mol)
    per_atom = [[int(l) for l, a in zip(mol.sh_l, at) if a == k] for k in range(4)]
    assert len({tuple(p) for p in per_atom}) == 4                                          # four different shell lists
    assert all(p != sorted(p) and p != sorted(p, reverse=True) for p in per_atom)          # none in monotonic order
    for l in range(lmax + 1):
        depths = {int(n) for n, sl in zip(mol.sh_nprim, mol.sh_l) if sl == l}
        assert depths >= ({1, 2, 3} if l < 3 else {1, 2}), (l, depths)
        assert all(l in p for p in per_atom)
    if lmax == 3:
        assert all(p.count(3) == 1 for p in per_atom)
    assert mol.exps.max() >= 50.0 and mol.exps.min() <= 0.15
    # twin pairs as the engine finds them (host_setup.cpp): consecutive s shells of one atom over identical primitives, nprim >= 2
    twins, plain = [], []
    for A in range(mol.nshell - 1):
        if mol.sh_l[A] or mol.sh_l[A + 1] or at[A] != at[A + 1]:
            continue
        ea = mol.exps[mol.sh_poff[A]: mol.sh_poff[A] + mol.sh_nprim[A]]
        eb = mol.exps[mol.sh_poff[A + 1]: mol.sh_poff[A + 1] + mol.sh_nprim[A + 1]]
        (twins if len(ea) == len(eb) >= 2 and np.array_equal(ea, eb) else plain).append(A)
    assert len(twins) == 1 and mol.sh_nprim[twins[0]] == 3
    assert len(plain) >= 1 and any(mol.sh_nprim[A] == mol.sh_nprim[A + 1] >= 2 for A in plain)
    if basis == cc.SPD:
        assert nao % 8 == 0 and 640 < nao * (nao + 1) // 2 and nao <= 64      # a batch of >= 64 takes the triangular tensor


@pytest.mark.parametrize("basis,lmax,nclass,nao", BASES)
def test_every_class_on_four_centres_and_with_every_swap(probe_dir, basis, lmax, nclass, nao):
    """Coverage is a condition: a later edit of the probe basis that loses a class, its four-centre quartets or one
    of its swaps fails here."""
    mol = oracle_mol(basis, cc.generic())
    want = cc.canonical_class_ids(lmax)
    assert len(want) == nclass
    tab = cc.quartet_table(mol)
    assert len(tab) == (lambda p: p * (p + 1) // 2)(mol.nshell * (mol.nshell + 1) // 2)
    assert sorted(set(tab[:, 0])) == want
    for cid in want:
        rows = tab[tab[:, 0] == cid]
        name = cc.class_name(cid)
        la, lb, lc, ld = cid // 512, (cid // 64) % 8, (cid // 8) % 8, cid % 8
        assert np.any(rows[:, 1] == 4), name
        for col, admitted, what in ((2, la != lb, "bra swap"), (3, lc != ld, "ket swap"), (4, (la, lb) != (lc, ld), "bra-ket exchange")):
            assert np.any(rows[:, col] == 0), (name, "without " + what)
            assert bool(np.any(rows[:, col] == 1)) == admitted, (name, what)
    # the element-wise map agrees with the quartet table on which (class, centre count) combinations exist
    cid, ncen = cc.class_of_elements(mol)
    assert cid.shape == (mol.nao * (mol.nao + 1) // 2,) * 2
    assert set(zip(cid.ravel().tolist(), ncen.ravel().tolist())) == set(zip(tab[:, 0].tolist(), tab[:, 1].tolist()))
    assert np.array_equal(cid, cid.T) and np.array_equal(ncen, ncen.T)


def _odd_x_mask(mol):
    """Packed-matrix mask of the elements whose integrand is odd under x -> -x at the origin: the real solid harmonics
    with a cos(m phi), m odd, or sin(m phi), m even, factor are odd in x.  In libcint's order m = -l .. l (p: x, y, z)."""
    odd = []
    for l in mol.sh_l:
        l = int(l)
        if l == 1:
            odd += [True, False, False]
        else:
            odd += [(m > 0 and m % 2 == 1) or (m < 0 and (-m) % 2 == 0) for m in range(-l, l + 1)]
    odd = np.array(odd)
    ii, jj = np.tril_indices(mol.nao)
    pair_odd = odd[ii] ^ odd[jj]
    return pair_odd[:, None] ^ pair_odd[None, :]


def test_odd_x_mask_is_what_planar_water_lacks():
    """The mask's own check: on the planar (x = 0) water of the stage tests every masked element is zero, and the
    unmasked ones are not all zero."""
    from tests.helpers import fragment_bohr
    frag = fragment_bohr([8, 1, 1], [[0.0, 0.0, -0.1364652], [0.0, 1.4304924, 1.0826636], [0.0, -1.4304924, 1.0826636]])
    for basis in ("cc-pvdz", "def2-tzvp"):
        mol = oracle_mol(basis, frag)
        M = stages.pack_eri(so.eri4(mol))
        mask = _odd_x_mask(mol)
        assert mask.any() and np.max(np.abs(M[mask])) < 1e-14
        assert np.max(np.abs(M[~mask])) > 1.0


@pytest.mark.parametrize("basis,lmax,nclass,nao", BASES)
def test_every_class_has_odd_x_content_on_generic(probe_dir, basis, lmax, nclass, nao):
    mol = oracle_mol(basis, cc.generic())
    M = np.abs(stages.pack_eri(so.eri4(mol)))
    cid, _ = cc.class_of_elements(mol)
    mask = _odd_x_mask(mol)
    for c in cc.canonical_class_ids(lmax):
        if c == 0:
            continue                       # (ss|ss) is one component, and it is even
        sel = (cid == c) & mask
        assert sel.any() and M[sel].max() > 1e-6, cc.class_name(c)


def test_references_agree_elementwise(probe_dir, tmp_path):
    """so.eri4 against rr.eri4_erf(mol, None): 1e-12 on every element, reported per class and centre count."""
    jobs = [(b, c, 0.0) for b in (cc.SPD, cc.SPDF) for c in cc.CASES]
    ref = cc.numpy_reference_packed(probe_dir, tmp_path, jobs)
    for b, c, _ in jobs:
        mol = oracle_mol(b, cc.CASES[c]())
        M = stages.pack_eri(so.eri4(mol))
        rep = cc.error_report(M - ref[(b, c, 0.0)], *cc.class_of_elements(mol))
        print("%s %s: oracle vs numpy reference, worst classes: %s" % (b, c, cc.format_report(rep, 4)))
        assert rep[0][2] < 1e-12, (b, c, cc.format_report(rep))
    # the two cases are different tensors: the far atom's cross terms have changed
    assert np.max(np.abs(ref[(cc.SPD, "generic", 0.0)] - ref[(cc.SPD, "stretched", 0.0)])) > 0.1


BOYS_T = [0.0, 1e-14, 1e-4, 9.9e-4, 1e-3, 0.5, 5.0, 30.0, 36.0, 54.0, 100.0, 200.0]


def test_boys_functions_against_mpmath():
    """rr.boys (scipy's incomplete gamma, a series below 1e-3) and the oracle's orc_boys (series and downward recursion
    below 36 + 1.5 nmax, erf and upward recursion above) against F_n(T) = 1F1(n + 1/2; n + 3/2; -T) / (2n + 1) from mpmath at
    40 digits, n = 0..12, over both codes' switch points; orc_boys also with nmax = 0, 4, 8, which move its switch
    to T = 36, 42, 48.  Relative 1e-13 is required; the figures each achieves are printed."""
    import mpmath
    mpmath.mp.dps = 40
    exact = np.array([[float(mpmath.hyp1f1(n + 0.5, n + 1.5, -mpmath.mpf(T)) / (2 * n + 1)) for T in BOYS_T] for n in range(13)])
    got = rr.boys(12, np.array(BOYS_T))
    rel = np.abs(got - exact) / exact
    print("rr.boys: worst relative error per T:", " ".join("%g:%.1e" % (T, r) for T, r in zip(BOYS_T, rel.max(axis=0))))
    worst = np.zeros(len(BOYS_T))
    for nmax in (0, 4, 8, 12):
        for k, T in enumerate(BOYS_T):
            F = np.zeros(nmax + 1)
            so.lib().orc_boys(nmax, ctypes.c_double(T), F.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
            worst[k] = max(worst[k], np.max(np.abs(F - exact[: nmax + 1, k]) / exact[: nmax + 1, k]))
    print("orc_boys: worst relative error per T:", " ".join("%g:%.1e" % (T, r) for T, r in zip(BOYS_T, worst)))
    assert rel.max() < 1e-13, ("rr.boys", rel.max(), np.unravel_index(np.argmax(rel), rel.shape))
    assert worst.max() < 1e-13, ("orc_boys", worst.max(), BOYS_T[int(np.argmax(worst))])


def test_sparse_density_is_what_the_bound_assumes():
    for seed in (0, 1, 77):
        D = cc.sparse_density(40, seed)
        assert np.array_equal(D, D.T) and np.max(np.abs(D)) <= 1.0
        assert np.count_nonzero(np.tril(D)) == 8
        assert np.sum(np.abs(D)) <= 16.0
    assert not np.array_equal(cc.sparse_density(40, 1), cc.sparse_density(40, 2))
