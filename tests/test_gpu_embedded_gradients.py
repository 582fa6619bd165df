"""Analytic gradients of fragments embedded in point charges (mqc_hip_scf_gradient_embedded_batch, kern_grad_pc.hip):
the gradient on the fragment's atoms and the gradient on the charges' sites.

Recipe and tolerances of test_gpu_wide_gradients.py: DIRECTIONAL central differences of the engine's own e_total in one
batch call -- three fixed-seed random unit directions and two single coordinates, 2e-6 Eh/a0 at h = 1e-3 for HF, 5e-6 at
h = 2e-3 for Kohn-Sham.  The directions span atom AND charge coordinates jointly (3N + 3M), so one number checks both
outputs and their relative sign; e_total holds tr(D u) and no nuclei-charge term, so moving everything together leaves
it unchanged and the two outputs must sum to zero per component (1e-7)."""
import numpy as np
import pytest

from metalquicha_amd import capi, fmo, mbe, methods
from metalquicha_amd.methods import FragmentGroup
from tests.helpers import fragment_bohr, w3_system

pytestmark = pytest.mark.gpu

AUX = "mqc-even-tempered-jkfit"


def _settings(basis, functional="", **kw):
    return methods.ScfSettings(basis_set=basis, functional=functional, energy_tol=1e-12, density_tol=1e-10, guess="gwh",
                               max_iter=200, **kw)


def _w3():
    system = w3_system()
    return np.asarray(system.element_numbers, dtype=np.int32), np.ascontiguousarray(system.coordinates.T)


def _group(Z, xyz, pts, q, multiplicity=1):
    xyz = np.asarray(xyz, dtype=float); m = xyz.shape[0]
    return FragmentGroup(np.asarray(Z, dtype=np.int32), xyz, np.zeros(m, dtype=np.int32), np.full(m, multiplicity, dtype=np.int32),
                         point_charge_xyz=np.asarray(pts, dtype=float), point_charges=np.asarray(q, dtype=float))


def _embedded(st, Z, xyz, pts, q, multiplicity=1, extras=(), extras_out=None):
    """One fragment through the embedded entry -> (record, atom gradient (N, 3), site gradient (M, 3))."""
    rec, atom, site = methods.run_hip_embedded_gradients(st, [_group(Z, xyz[None], pts[None], q[None], multiplicity)], extras=extras,
                                                         extras_out=extras_out)
    assert not rec[0]["has_error"][0], bytes(rec[0]["message"][0])
    assert rec[0]["has_gradient"][0]
    return rec[0][0], atom[0][0], site[0][0]


def _check_directional(st, Z, xyz, pts, q, h, tol, multiplicity=1, seed=2026, **kw):
    _, ga, gs = _embedded(st, Z, xyz, pts, q, multiplicity, **kw)
    assert ga.shape == xyz.shape and gs.shape == pts.shape
    g = np.concatenate([ga.reshape(-1), gs.reshape(-1)])
    x0 = np.concatenate([xyz.reshape(-1), pts.reshape(-1)])
    na3 = xyz.size
    rng = np.random.default_rng(seed)
    dirs = [d / np.linalg.norm(d) for d in rng.normal(size=(3, x0.size))]
    for k in rng.choice(x0.size, 2, replace=False):
        e = np.zeros(x0.size); e[k] = 1.0
        dirs.append(e)
    moved = np.stack([x0 + sgn * h * d for d in dirs for sgn in (1.0, -1.0)])
    m = moved.shape[0]
    grp = _group(Z, moved[:, :na3].reshape(m, -1, 3), moved[:, na3:].reshape(m, -1, 3), np.stack([q] * m), multiplicity)
    rec = methods.run_hip_scf_groups(st, [grp])[0]
    assert not rec["has_error"].any(), rec["message"]
    e = rec["e_total"]
    for i, d in enumerate(dirs):
        fd = (e[2 * i] - e[2 * i + 1]) / (2.0 * h)
        print("direction %d: analytic %.10f  central difference %.10f  |diff| %.2e" % (i, float(g @ d), fd, abs(float(g @ d) - fd)))
        assert abs(float(g @ d) - fd) < tol, (i, float(g @ d), fd)
    total = ga.sum(axis=0) + gs.sum(axis=0)
    print("sum over atoms and sites:", total)
    assert np.max(np.abs(total)) < 1e-7, total
    return ga, gs


def test_water_631g_in_six_charges():
    """s and p shells, pairs on one and on two centres, less than one tile of charges."""
    Z, xyz = _w3()
    q = np.random.default_rng(5).uniform(-0.8, 0.8, size=6)
    _check_directional(_settings("6-31g"), Z[:3], xyz[:3], xyz[3:], q, 1e-3, 2e-6)


@pytest.mark.parametrize("npc", [3, 1])
def test_water_dimer_ccpvdz(npc):
    """d shells on two-centre pairs; a single charge."""
    Z, xyz = _w3()
    q = np.array([-0.8, 0.4, 0.4])[:npc]
    _check_directional(_settings("cc-pvdz"), Z[:6], xyz[:6], xyz[6:6 + npc], q, 1e-3, 2e-6)


def test_water_def2tzvp_f_pairs():
    """f-f pairs: Hermite integrals of order 7 in the charge kernel."""
    Z, xyz = _w3()
    q = np.random.default_rng(6).uniform(-0.8, 0.8, size=6)
    _check_directional(_settings("def2-tzvp"), Z[:3], xyz[:3], xyz[3:], q, 1e-3, 2e-6)


def _shell_of_charges(xyz, count, seed=17):
    """`count` positions uniform in the shell 4-30 Bohr around the centroid, none within 2.5 Bohr of an atom."""
    rng = np.random.default_rng(seed)
    centre = xyz.mean(axis=0)
    pts = []
    while len(pts) < count:
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        r = (rng.uniform() * (30.0 ** 3 - 4.0 ** 3) + 4.0 ** 3) ** (1.0 / 3.0)
        p = centre + r * d
        if np.min(np.linalg.norm(xyz - p, axis=1)) >= 2.5:
            pts.append(p)
    return np.array(pts), rng.uniform(-0.9, 0.9, size=count)


@pytest.mark.parametrize("npc", [400, 65])
def test_many_charges_ccpvdz_and_hellmann_feynman(npc):
    """400 = 6 x 64 + 16 charges: several tiles and a ragged last one, on both sides of the far radius of the energy's
    far table (about 13 Bohr); 65: one full tile and one lane.  Besides the directional check every site gradient is
    compared with Hellmann-Feynman through the ESP entry, g_g = q_g grad V_elec(R_g), grad V_elec from central
    differences (h = 1e-3) of run_hip_esp(include_nuclei=False) on the converged density, to 2e-6."""
    Z, xyz = _w3()
    Z, xyz = Z[:3], xyz[:3]
    pts, q = _shell_of_charges(xyz, 400)
    pts, q = pts[:npc], q[:npc]
    radius = np.linalg.norm(pts - xyz.mean(axis=0), axis=1)
    assert radius.min() < 13.0 < radius.max()
    st = _settings("cc-pvdz")
    extras = []
    _, gs = _check_directional(st, Z, xyz, pts, q, 1e-3, 2e-6, extras=("density",), extras_out=extras)
    D = extras[0]["density"][0]
    h = 1e-3
    probe = np.concatenate([pts + sgn * h * np.eye(3)[c] for c in range(3) for sgn in (1.0, -1.0)])      # (6 npc, 3)
    v = methods.run_hip_esp(st, FragmentGroup(Z, xyz[None], np.zeros(1, dtype=np.int32)), D[None], probe[None],
                            include_nuclei=False)[0].reshape(3, 2, npc)
    hf = q[:, None] * ((v[:, 0] - v[:, 1]) / (2.0 * h)).T
    print("site gradients against Hellmann-Feynman: max |diff| %.2e" % np.max(np.abs(gs - hf)))
    assert np.max(np.abs(gs - hf)) < 2e-6, np.max(np.abs(gs - hf))


def test_batch_bookkeeping():
    """Three geometries of one topology in three different fields (one of them all zero) in ONE call, least compact
    first so that the engine's reordering by compactness is not the identity; then a mixed call with a group that has
    no charges."""
    Z, xyz = _w3()
    Z = Z[:3]
    rng = np.random.default_rng(11)
    geoms = np.stack([xyz[:3] * 1.06, xyz[:3] + 0.03 * rng.normal(size=(3, 3)), xyz[:3]])
    sites = np.stack([xyz[3:], xyz[3:] + 0.2 * rng.normal(size=(6, 3)), xyz[3:] + 0.4])
    q = np.stack([rng.uniform(-0.8, 0.8, size=6), np.zeros(6), rng.uniform(-0.8, 0.8, size=6)])
    st = _settings("6-31g")
    rec, atom, site = methods.run_hip_embedded_gradients(st, [_group(Z, geoms, sites, q)])
    assert not rec[0]["has_error"].any(), rec[0]["message"]
    for k in range(3):
        r1, ga, gs = _embedded(st, Z, geoms[k], sites[k], q[k])
        assert abs(rec[0]["e_total"][k] - r1["e_total"]) < 1e-10
        assert np.max(np.abs(atom[0][k] - ga)) < 1e-8, (k, np.max(np.abs(atom[0][k] - ga)))
        assert np.max(np.abs(site[0][k] - gs)) < 1e-8, (k, np.max(np.abs(site[0][k] - gs)))
    bare = methods.run_hip_scf(st, fragment_bohr(Z, geoms[1]), want_gradient=True)
    assert not bare.has_error, bare.error_message
    assert np.max(np.abs(atom[0][1] - bare.gradient.T)) < 1e-8
    assert np.all(site[0][1] == 0.0)
    # a group without charges next to an embedded one: the plain gradient, an empty site array
    plain = FragmentGroup(Z, geoms[1:2], np.zeros(1, dtype=np.int32))
    rec2, atom2, site2 = methods.run_hip_embedded_gradients(st, [plain, _group(Z, geoms[:1], sites[:1], q[:1])])
    assert not rec2[0]["has_error"].any() and not rec2[1]["has_error"].any()
    assert site2[0].shape == (1, 0, 3)
    assert np.max(np.abs(atom2[0][0] - bare.gradient.T)) < 1e-8
    assert np.max(np.abs(atom2[1][0] - atom[0][0])) < 1e-8 and np.max(np.abs(site2[1][0] - site[0][0])) < 1e-8


@pytest.mark.parametrize("kind", ["uhf", "b3lyp", "df"])
def test_other_scf_types(kind):
    """UHF (an OH radical), B3LYP at grid level 1 and density-fitted RHF, 6-31G in six charges."""
    Z, xyz = _w3()
    q = np.random.default_rng(8).uniform(-0.8, 0.8, size=6)
    if kind == "uhf":
        _check_directional(_settings("6-31g"), Z[:2], xyz[:2], xyz[3:], q, 1e-3, 2e-6, multiplicity=2)
    elif kind == "b3lyp":
        _check_directional(_settings("6-31g", "b3lyp", grid_level=1), Z[:3], xyz[:3], xyz[3:], q, 2e-3, 5e-6)
    else:
        _check_directional(_settings("6-31g", density_fitting=True, aux_basis_set=AUX), Z[:3], xyz[:3], xyz[3:], q, 1e-3, 2e-6)


def test_refusals_and_validation():
    Z, xyz = _w3()
    Z = Z[:3]
    q = np.full((1, 6), 0.1)
    st = _settings("6-31g")
    nao = methods._flat_basis_z("6-31g", Z).nao
    # h_extra: refused in that fragment's record, the other group of the batch succeeds
    hx = _group(Z, xyz[None, :3], xyz[None, 3:], q)
    hx.h_extra = np.zeros((1, nao, nao))
    status = []
    rec, atom, site = methods.run_hip_embedded_gradients(st, [hx, _group(Z, xyz[None, :3], xyz[None, 3:], q)], status_out=status)
    assert rec[0]["has_error"][0] and b"h_extra" in bytes(rec[0]["message"][0]) and not rec[0]["has_gradient"][0]
    assert status == [capi.ERR_UNSUPPORTED]
    assert not rec[1]["has_error"][0] and rec[1]["has_gradient"][0] and np.max(np.abs(site[1][0])) > 1e-4
    # alone, its code is the call's
    status = []
    rec = methods.run_hip_embedded_gradients(st, [hx], status_out=status)[0]
    assert rec[0]["has_error"][0] and status == [capi.ERR_UNSUPPORTED]
    # meta-GGA: as for plain gradients
    status = []
    rec = methods.run_hip_embedded_gradients(_settings("6-31g", "tpss", grid_level=1), [_group(Z, xyz[None, :3], xyz[None, 3:], q)],
                                             status_out=status)[0]
    assert rec[0]["has_error"][0] and b"meta-GGA" in bytes(rec[0]["message"][0]) and status == [capi.ERR_UNSUPPORTED]
    # charges announced with NULL arrays
    import ctypes as C
    lib = capi.load_library(); ctx = capi.get_context(0)
    frag = fragment_bohr(Z, xyz[:3])
    m = methods._Marshalled(frag, methods._flat_basis("6-31g", frag))
    m.mol.n_point_charges = 6
    opts = methods._options(st, False)
    r = capi.ScfResult()
    grad = np.zeros((3, 3)); r.gradient = capi.dptr(grad)
    sg = np.zeros((6, 3))
    ptrs = (capi.c_double_p * 1)(capi.dptr(sg))
    rc = lib.mqc_hip_scf_gradient_embedded_batch(ctx, 1, C.byref(m.mol), C.byref(m.bas), None, C.byref(opts), C.byref(r), ptrs)
    assert rc == capi.ERR_VALIDATION and r.has_error and b"NULL" in r.message
    # a NULL pointer array while a fragment carries charges
    pq = np.full(6, 0.1); px = np.ascontiguousarray(xyz[3:])
    m.mol.point_charges = capi.dptr(pq); m.mol.point_charge_xyz = capi.dptr(px)
    rc = lib.mqc_hip_scf_gradient_embedded_batch(ctx, 1, C.byref(m.mol), C.byref(m.bas), None, C.byref(opts), C.byref(r), None)
    assert rc == capi.ERR_VALIDATION
    # a NULL entry skips the site gradient only
    null = (capi.c_double_p * 1)()
    rc = lib.mqc_hip_scf_gradient_embedded_batch(ctx, 1, C.byref(m.mol), C.byref(m.bas), None, C.byref(opts), C.byref(r), null)
    assert rc == capi.MQC_HIP_OK and r.has_gradient and not r.has_error
    # the plain batch entry keeps refusing (its record has no slot for the site gradient)
    rec = methods.run_hip_scf_groups(st, [_group(Z, xyz[None, :3], xyz[None, 3:], q)], want_gradient=True, gradients_out=[])[0]
    assert rec["has_error"][0] and b"point charges" in bytes(rec["message"][0])


def test_eembe_fixed_charges_water_trimer():
    """run_eembe_fixed_charges, 6-31G, O -0.8 / H +0.4: directional central differences of its own total energy over
    all 27 coordinates; with all charges zero it is the plain MBE2 with its gradient."""
    system = w3_system()
    st = _settings("6-31g")
    charges = np.array([-0.8, 0.4, 0.4] * 3)
    run = fmo.run_eembe_fixed_charges(system, st, charges)
    assert not run.errors, run.errors
    assert run.gradient.shape == (3, 9)
    g = run.gradient.T.reshape(-1)
    x0 = np.ascontiguousarray(system.coordinates.T).reshape(-1)
    rng = np.random.default_rng(2026)
    dirs = [d / np.linalg.norm(d) for d in rng.normal(size=(3, x0.size))]
    for k in rng.choice(x0.size, 2, replace=False):
        e = np.zeros(x0.size); e[k] = 1.0
        dirs.append(e)
    h = 1e-3
    for i, d in enumerate(dirs):
        e = []
        for sgn in (1.0, -1.0):
            moved = mbe.FragmentedSystem(system.element_numbers, (x0 + sgn * h * d).reshape(-1, 3).T.copy(), system.monomers)
            r = fmo.run_eembe_fixed_charges(moved, st, charges, want_gradient=False)
            assert not r.errors, r.errors
            e.append(r.energy)
        fd = (e[0] - e[1]) / (2.0 * h)
        print("direction %d: analytic %.10f  central difference %.10f  |diff| %.2e" % (i, float(g @ d), fd, abs(float(g @ d) - fd)))
        assert abs(float(g @ d) - fd) < 2e-6, (i, float(g @ d), fd)
    assert np.max(np.abs(run.gradient.sum(axis=1))) < 1e-7, run.gradient.sum(axis=1)
    zero = fmo.run_eembe_fixed_charges(system, st, np.zeros(9))
    ref = mbe.run_mbe(system, st, level=2, want_gradient=True)
    assert not zero.errors and not ref.errors
    assert abs(zero.energy - mbe.compute_mbe(ref.terms, ref.energies)[0]) < 1e-8
    assert np.max(np.abs(zero.gradient.T - ref.gradient)) < 1e-8, np.max(np.abs(zero.gradient.T - ref.gradient))
