"""GPU tests of the electrostatic potential on point sets (mqc_hip_esp_batch, kern_esp.hip) and of the CHELPG charges
built on it: against the oracle's nuclear-attraction integrals (u_r = point_charge_potential(mol, [r], [1]), so that
V_elec(r) = tr(D u_r)), against the engine's own embedding energy, batched against single calls, the refusals, the
fitted charges and an FMO run whose far field they describe."""
import numpy as np
import pytest

from metalquicha_amd import capi, charges, fmo, methods
from metalquicha_amd.basis import ANGSTROM_TO_BOHR, build_flat_basis
from metalquicha_amd.methods import FragmentGroup, ScfSettings
from oracle import scf_oracle as so
from tests.helpers import W1_ANGSTROM, fragment_bohr, oracle_fmo_solver, oracle_make_mol, oracle_mol, synthetic_density, water_at, w3_system

pytestmark = pytest.mark.gpu

WATER = np.array(W1_ANGSTROM) * ANGSTROM_TO_BOHR


def _settings(basis, **kw):
    return ScfSettings(basis_set=basis, energy_tol=1e-10, density_tol=1e-8, guess="gwh", **kw)


def _group(z, xyz):
    xyz = np.asarray(xyz, dtype=float)
    xyz = xyz[None] if xyz.ndim == 2 else xyz
    return FragmentGroup(np.asarray(z, dtype=np.int32), xyz, np.zeros(len(xyz), dtype=np.int32))


def _oracle_electronic(mol, D, pts):
    """tr(D u_r) for every point: the electronic part of the potential, sign included."""
    return np.array([float(np.sum(D * so.point_charge_potential(mol, [r], [1.0]))) for r in pts])


def _nuclear(z, xyz, pts):
    return (1.0 / np.linalg.norm(pts[:, None, :] - xyz[None, :, :], axis=2)) @ np.asarray(z, dtype=float)


def _points_around(rng, xyz, n, r_lo=1.5, r_hi=12.0):
    out = []
    while len(out) < n:
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        p = xyz[rng.integers(len(xyz))] + d * rng.uniform(r_lo, r_hi)
        if np.min(np.linalg.norm(xyz - p, axis=1)) >= r_lo:
            out.append(p)
    return np.array(out)


def _converged_density(basis, z, xyz):
    extras = []
    rec = methods.run_hip_scf_groups(_settings(basis), [_group(z, xyz)], extras=("density",), extras_out=extras)[0]
    assert not rec["has_error"].any(), rec["message"]
    return extras[0]["density"][0]


@pytest.fixture(scope="module")
def water_case():
    """H2O / cc-pVDZ: the points and the oracle's u_r matrices, shared by both densities."""
    rng = np.random.default_rng(11)
    z = [8, 1, 1]
    pts = np.vstack([_points_around(rng, WATER, 144),
                     0.5 * (WATER[0] + WATER[1])[None],                                  # O-H midpoint: small T
                     WATER[0][None] + np.array([[60.0, 0, 0], [0, -60.0, 0], [35.0, 35.0, 35.0]]),
                     WATER[0][None] + np.array([[0, 0, 300.0], [-170.0, 170.0, 170.0]])])   # asymptotic Boys branch
    mol = oracle_mol("cc-pvdz", fragment_bohr(z, WATER))
    u = np.stack([so.point_charge_potential(mol, [r], [1.0]) for r in np.vstack([pts, WATER])])
    return z, pts, mol, u


@pytest.mark.parametrize("density", ["synthetic", "rhf"])
def test_water_potential_matches_oracle(water_case, density):
    """~150 points (1.5-12 Bohr from the atoms, the O-H midpoint, 60 and 300 Bohr away) and, for the electronic part
    alone, the three nuclei themselves (T = 0).  Electronic part within 1e-11 sum|D| (the elementwise bound u meets
    against the oracle, through the contraction); nuclear part apart, 1e-12 relative."""
    z, pts, mol, u = water_case
    D = synthetic_density(24) if density == "synthetic" else _converged_density("cc-pvdz", z, WATER)
    assert D.shape == (mol.nao, mol.nao)
    bound = 1e-11 * float(np.sum(np.abs(D)))
    st, g = _settings("cc-pvdz"), _group(z, WATER)
    with_nuclei = np.vstack([pts, WATER])
    v_el = methods.run_hip_esp(st, g, D[None], with_nuclei[None], include_nuclei=False)[0]
    ref_el = np.einsum("pij,ij->p", u, D)
    err = np.abs(v_el - ref_el)
    print("electronic part: max error %.3e, bound %.3e (worst point %d)" % (err.max(), bound, int(np.argmax(err))))
    assert err.max() < bound
    v = methods.run_hip_esp(st, g, D[None], pts[None], include_nuclei=True)[0]
    nuc = _nuclear(z, WATER, pts)
    rel = np.abs((v - v_el[:len(pts)]) - nuc) / nuc
    print("nuclear part: max relative error %.3e" % rel.max())
    assert rel.max() < 1e-12
    assert np.max(np.abs(v - (nuc + ref_el[:len(pts)]))) < bound + 1e-12 * np.max(nuc)


def test_f_shell_potential_matches_oracle():
    """CO / def2-TZVP (f shells on both atoms: L = 4, 5 and 6 records) with the synthetic density, 64 points."""
    z = [6, 8]
    xyz = np.array([[0.1, -0.2, 0.0], [0.4, 0.3, 2.132]])
    mol = oracle_mol("def2-tzvp", fragment_bohr(z, xyz))
    fb = build_flat_basis("def2-tzvp", z)
    assert int(np.max(fb.shell_l)) == 3
    D = synthetic_density(mol.nao)
    rng = np.random.default_rng(12)
    pts = np.vstack([_points_around(rng, xyz, 61), 0.5 * (xyz[0] + xyz[1])[None], xyz[0][None] + [[0, 70.0, 0]], xyz[1][None] + [[300.0, 0, 0]]])
    assert len(pts) == 64
    v_el = methods.run_hip_esp(_settings("def2-tzvp"), _group(z, xyz), D[None], pts[None], include_nuclei=False)[0]
    ref = _oracle_electronic(mol, D, pts)
    bound = 1e-11 * float(np.sum(np.abs(D)))
    err = np.abs(v_el - ref)
    print("f shells: max error %.3e, bound %.3e" % (err.max(), bound))
    assert err.max() < bound


def test_duality_with_the_embedding_energy():
    """One water in 400 point charges (the count that takes int1e's far-field-table route): sum_g q_g V_elec(R_g) is
    the engine's own tr(D u), within 1e-11 sum|q| sum|D|."""
    rng = np.random.default_rng(7)
    npc = 400
    direction = rng.normal(size=(npc, 3)); direction /= np.linalg.norm(direction, axis=1)[:, None]
    radius = np.concatenate([rng.uniform(4.0, 9.0, size=60), rng.uniform(9.0, 70.0, size=npc - 60)])
    pts = WATER[0] + direction * radius[:, None]
    q = rng.uniform(-0.9, 0.9, size=npc)
    g = _group([8, 1, 1], WATER)
    g.point_charge_xyz = pts[None]; g.point_charges = q[None]
    extras = []
    st = _settings("cc-pvdz")
    rec = methods.run_hip_scf_groups(st, [g], extras=("density",), extras_out=extras)[0]
    assert not rec["has_error"].any(), rec["message"]
    D = extras[0]["density"][0]
    v_el = methods.run_hip_esp(st, _group([8, 1, 1], WATER), D[None], pts[None], include_nuclei=False)[0]
    got, want = float(q @ v_el), float(rec["e_embedding"][0])
    bound = 1e-11 * float(np.sum(np.abs(q))) * float(np.sum(np.abs(D)))
    print("duality: sum q V = %.15f, e_embedding = %.15f, difference %.3e, bound %.3e" % (got, want, abs(got - want), bound))
    assert abs(want) > 1e-3
    assert abs(got - want) < bound


def _sto3g_waters(rng, m):
    xyz = np.stack([water_at(rng, rng.uniform(-3.0, 3.0, size=3)) for _ in range(m)])
    D = np.stack([synthetic_density(7) * (1.0 + 0.1 * f) for f in range(m)])
    return xyz, D


def test_ragged_batch_equals_single_calls():
    """Three waters of different geometry with 1, 64 and 257 points (the point tile is 256): the batch equals one call
    per fragment to 1e-13, and the padding entries of the output keep the caller's sentinel."""
    rng = np.random.default_rng(21)
    st = _settings("sto-3g")
    xyz, D = _sto3g_waters(rng, 3)
    counts = np.array([1, 64, 257], dtype=np.int32)
    pts = np.full((3, 257, 3), np.nan)                  # entries beyond a count are not read: NaN there is legal
    for f in range(3):
        pts[f, :counts[f]] = _points_around(rng, xyz[f], counts[f])
    out = np.full((3, 257), -777.0)
    got = methods.run_hip_esp(st, _group([8, 1, 1], xyz), D, pts, counts, out=out)
    assert got is out
    for f in range(3):
        one = methods.run_hip_esp(st, _group([8, 1, 1], xyz[f]), D[f][None], pts[f:f + 1, :counts[f]])[0]
        assert np.max(np.abs(got[f, :counts[f]] - one)) < 1e-13
        assert np.all(got[f, counts[f]:] == -777.0)
        assert np.all(np.isfinite(one)) and np.max(np.abs(one)) > 1e-3


def test_fragment_chunks_equal_single_calls(monkeypatch):
    """65 fragments of 63 points, in one chunk and in chunks of at most 64 fragments (MQC_HIP_ESP_CHUNK): both equal the
    single-fragment calls to 1e-13."""
    rng = np.random.default_rng(22)
    st = _settings("sto-3g")
    xyz, D = _sto3g_waters(rng, 65)
    pts = np.stack([_points_around(rng, xyz[f], 63) for f in range(65)])
    g = _group([8, 1, 1], xyz)
    whole = methods.run_hip_esp(st, g, D, pts)
    monkeypatch.setenv("MQC_HIP_ESP_CHUNK", "64")
    chunked = methods.run_hip_esp(st, g, D, pts)
    monkeypatch.delenv("MQC_HIP_ESP_CHUNK")
    for f in range(65):
        one = methods.run_hip_esp(st, _group([8, 1, 1], xyz[f]), D[f][None], pts[f:f + 1])[0]
        assert np.max(np.abs(whole[f] - one)) < 1e-13
        assert np.max(np.abs(chunked[f] - one)) < 1e-13


def test_refusals_and_empty_calls():
    st = _settings("sto-3g")
    g = _group([8, 1, 1], WATER)
    D = synthetic_density(7)[None]
    pts = _points_around(np.random.default_rng(3), WATER, 8)[None]
    on_nucleus = pts.copy(); on_nucleus[0, 5] = WATER[1]
    with pytest.raises(capi.HipBackendError) as e:
        methods.run_hip_esp(st, g, D, on_nucleus, include_nuclei=True)
    assert e.value.code == capi.ERR_VALIDATION and "nucleus" in e.value.message
    assert np.all(np.isfinite(methods.run_hip_esp(st, g, D, on_nucleus, include_nuclei=False)))      # legal: T = 0
    bad = pts.copy(); bad[0, 2, 1] = np.nan
    with pytest.raises(capi.HipBackendError) as e:
        methods.run_hip_esp(st, g, D, bad)
    assert e.value.code == capi.ERR_VALIDATION
    with pytest.raises(capi.HipBackendError) as e:
        methods.run_hip_esp(st, g, D, pts, n_points=np.array([-1], dtype=np.int32))
    assert e.value.code == capi.ERR_VALIDATION
    # zero-size calls are fine and write nothing
    assert methods.run_hip_esp(st, g, D, np.zeros((1, 0, 3))).shape == (1, 0)
    none = FragmentGroup(np.array([8, 1, 1], dtype=np.int32), np.zeros((0, 3, 3)), np.zeros(0, dtype=np.int32))
    assert methods.run_hip_esp(st, none, np.zeros((0, 7, 7)), np.zeros((0, 4, 3))).shape == (0, 4)
    # the engine still answers afterwards
    assert np.all(np.isfinite(methods.run_hip_esp(st, g, D, pts)))


def _oracle_esp(basis):
    def esp(group, dens, pts, counts):
        out = np.zeros(pts.shape[:2])
        for f in range(pts.shape[0]):
            mol = oracle_mol(basis, fragment_bohr(group.element_numbers, group.xyz[f]))
            p = pts[f, :counts[f]]
            out[f, :counts[f]] = _nuclear(group.element_numbers, np.asarray(group.xyz[f]), p) + _oracle_electronic(mol, dens[f], p)
        return out
    return esp


def test_chelpg_charges_match_the_oracle_potential_fit():
    """H2O / cc-pVDZ RHF, spacing 0.6 Angstrom (548 points): the engine's potential and the oracle's potential of the
    SAME density through the same grid and the same fit give the same charges to 1e-8.  Measured on the host for this
    grid: a random perturbation of the potential of 1e-10 per point moves the fitted charges by at most 2.3e-10 (200
    draws), below the 1e-9 at which the issue would widen the bound, so 1e-8 stands.  The charges sum to the molecular
    charge (1e-12) and the hydrogens of the C2v water agree (1e-8)."""
    z = [8, 1, 1]
    st = _settings("cc-pvdz")
    D = _converged_density("cc-pvdz", z, WATER)
    g = _group(z, WATER)
    grid = charges.chelpg_grid(z, WATER, spacing=0.6)
    assert 300 < len(grid) < 1500
    q = charges.chelpg_charges(st, [g], [D[None]], spacing=0.6)[0][0]
    ref = charges.chelpg_charges(st, [g], [D[None]], spacing=0.6, esp=_oracle_esp("cc-pvdz"))[0][0]
    print("CHELPG charges", q, "oracle-potential fit", ref, "difference %.3e" % np.max(np.abs(q - ref)))
    assert np.max(np.abs(q - ref)) < 1e-8
    assert abs(float(np.sum(q))) < 1e-12
    assert abs(q[1] - q[2]) < 1e-8
    assert q[0] < -0.4 and q[1] > 0.2                      # a water, not noise


def test_fmo_with_fitted_charges_matches_the_oracle_driver():
    """w3 / 6-31g, EE-MBE with every field atom a potential-fitted charge: engine SCFs and engine potentials against
    the oracle solver with oracle potentials through the same driver (0.6 Angstrom grids on both sides, which keeps the
    oracle side to seconds): totals within 1e-8, the bound of the manifest's FMO goldens, and equal outer pass counts."""
    system = w3_system()
    st = ScfSettings(basis_set="6-31g", energy_tol=1e-9, density_tol=1e-7, guess="gwh")
    run = fmo.run_fmo2(system, st, expansion="mbe", esp="ptc", far_field="chelpg",
                       charges=charges.hip_chelpg_charges(system, st, spacing=0.6))
    assert not run.errors, run.errors
    assert run.converged
    ref = fmo.run_fmo2(system, st, expansion="mbe", esp="ptc", far_field="chelpg", solver=oracle_fmo_solver(system, "6-31g"),
                       charges=charges.hip_chelpg_charges(system, st, spacing=0.6, esp=_oracle_esp("6-31g")))
    assert ref.converged and not ref.errors
    print("FMO chelpg: engine %.10f oracle %.10f passes %d / %d" % (run.energy, ref.energy, run.outer_iterations, ref.outer_iterations))
    assert run.outer_iterations == ref.outer_iterations
    assert abs(run.energy - ref.energy) < 1e-8
    mull = fmo.run_fmo2(system, st, expansion="mbe", esp="ptc", far_field="mulliken")
    assert abs(mull.energy - run.energy) > 1e-6            # the charge model does reach the energy


def test_default_charge_model_is_the_engine():
    """far_field = "chelpg" without a callable runs the engine-backed default (0.3 Angstrom grids) to a settled total."""
    system = w3_system()
    st = ScfSettings(basis_set="6-31g", energy_tol=1e-9, density_tol=1e-7, guess="gwh")
    run = fmo.run_fmo2(system, st, expansion="fmo", far_field="chelpg")
    assert run.converged and not run.errors
    assert abs(float(np.sum(run.charges))) < 1e-10
    assert abs(run.energy - (-227.97)) < 0.01
