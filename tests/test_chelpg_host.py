"""Host side of the potential-fitted charges (no GPU): the CHELPG point selection, the constrained fit, and the
plumbing of far_field = "chelpg" through fmo.run_fmo2 with an injected charge model."""
import threading

import numpy as np
import pytest

from metalquicha_amd import charges, fmo
from metalquicha_amd.basis import ANGSTROM_TO_BOHR
from metalquicha_amd.methods import ScfSettings
from tests.helpers import W1_ANGSTROM, oracle_fmo_solver, w3_system

WATER = np.array(W1_ANGSTROM) * ANGSTROM_TO_BOHR
FIVE_Z = [7, 1, 1, 1, 1]            # an ammonium-shaped set, total charge +1
FIVE = np.array([[0.0, 0.0, 0.0], [0.59, 0.59, 0.59], [-0.59, -0.59, 0.59], [-0.59, 0.59, -0.59], [0.59, -0.59, -0.59]]) * ANGSTROM_TO_BOHR


def _coulomb(points, centres, q):
    return (1.0 / np.linalg.norm(points[:, None, :] - centres[None, :, :], axis=2)) @ np.asarray(q)


@pytest.mark.parametrize("z, xyz, q", [([8, 1, 1], WATER, [-0.8, 0.4, 0.4]),
                                       (FIVE_Z, FIVE, [-0.62, 0.43, 0.38, 0.41, 0.40])])
def test_fit_recovers_known_charges(z, xyz, q):
    """The exact Coulomb potential of known charges on the CHELPG grid gives those charges back: 1e-10 each, 1e-12 on
    their sum."""
    pts = charges.chelpg_grid(z, xyz)
    assert len(pts) > 100
    total = float(np.sum(q))
    got = charges.fit_charges(pts, _coulomb(pts, xyz, q), xyz, total)
    assert np.max(np.abs(got - np.asarray(q))) < 1e-10
    assert abs(float(np.sum(got)) - total) < 1e-12


def _radii_bohr(z):
    return np.array([fmo.VDW_ANGSTROM[int(v) - 1] for v in z]) * ANGSTROM_TO_BOHR


def test_grid_keeps_out_of_the_atoms_and_within_the_padding():
    pad = 2.8 * ANGSTROM_TO_BOHR
    for z, xyz in (([8, 1, 1], WATER), (FIVE_Z, FIVE)):
        pts = charges.chelpg_grid(z, xyz)
        d = np.linalg.norm(pts[:, None, :] - xyz[None, :, :], axis=2)
        assert np.all(d >= _radii_bohr(z)[None, :])
        assert np.all(np.min(d, axis=1) <= pad)
        # a lattice of the stated spacing centred on the bounding box: every coordinate is its corner plus whole steps
        h = 0.3 * ANGSTROM_TO_BOHR
        n = np.floor((xyz.max(axis=0) - xyz.min(axis=0) + 2 * pad) / h + 1e-9).astype(int) + 1
        corner = 0.5 * (xyz.max(axis=0) + xyz.min(axis=0)) - 0.5 * h * (n - 1)
        k = (pts - corner) / h
        assert np.max(np.abs(k - np.round(k))) < 1e-9
        # nothing the rules allow is missing: the count equals a brute-force selection over the same lattice
        ax = [corner[c] + h * np.arange(n[c]) for c in range(3)]
        lat = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
        dl = np.linalg.norm(lat[:, None, :] - xyz[None, :, :], axis=2)
        assert len(pts) == int(np.sum(np.all(dl >= _radii_bohr(z)[None, :], axis=1) & (np.min(dl, axis=1) <= pad)))


def test_ghost_atom_changes_neither_rule():
    """A ghost excludes nothing, keeps nothing and does not move the lattice: the grid is that of the real atoms."""
    ghost_xyz = np.vstack([WATER, WATER[:1] + np.array([0.0, 0.0, 5.5])])
    with_ghost = charges.chelpg_grid([8, 1, 1, 8], ghost_xyz, ghost=[False, False, False, True])
    assert np.array_equal(with_ghost, charges.chelpg_grid([8, 1, 1], WATER))
    # some points do lie inside the ghost's radius, and a real atom there would have removed them
    d = np.linalg.norm(with_ghost - ghost_xyz[3], axis=1)
    assert np.any(d < 1.52 * ANGSTROM_TO_BOHR)
    real = charges.chelpg_grid([8, 1, 1, 8], ghost_xyz)
    assert not np.any(np.linalg.norm(real - ghost_xyz[3], axis=1) < 1.52 * ANGSTROM_TO_BOHR)


def test_translated_molecule_gives_the_translated_grid():
    shift = np.array([3.25, -7.5, 11.125])
    a = charges.chelpg_grid([8, 1, 1], WATER)
    b = charges.chelpg_grid([8, 1, 1], WATER + shift)
    assert a.shape == b.shape
    assert np.max(np.abs(b - shift - a)) < 1e-12


def test_mirror_plane_of_the_molecule_is_one_of_the_grid():
    """The C2v water's hydrogens are mirror images in y: so is the grid, and a fit gives them equal charges."""
    w = WATER.copy(); w[:, 1] = [0.0, w[1, 1], -w[1, 1]]           # the sample geometry is symmetric to 1e-10 only
    pts = charges.chelpg_grid([8, 1, 1], w)
    mirrored = pts * np.array([1.0, -1.0, 1.0])
    key = lambda p: np.lexsort(np.round(p, 9).T)
    assert np.max(np.abs(pts[key(pts)] - mirrored[key(mirrored)])) < 1e-12
    q = charges.fit_charges(pts, _coulomb(pts, w, [-0.7, 0.3, 0.4]) + _coulomb(pts, w, [0.0, 0.05, -0.05]), w, 0.0)
    assert abs(q[1] - q[2]) < 1e-10


def test_grid_refuses_elements_without_a_radius():
    with pytest.raises(ValueError):
        charges.chelpg_grid([26, 1], np.array([[0.0, 0, 0], [0, 0, 3.0]]))


def _recording(solver):
    """The solver, and a charges callable that hands back the Mulliken charges the solver last produced for a fragment."""
    seen = {}

    def solve(jobs):
        res = solver(jobs)
        for job, r in zip(jobs, res):
            seen[tuple(job.atoms)] = r.charges
        return res

    def model(requests):
        for atoms, dens in requests:
            assert dens is not None and dens.shape[0] == dens.shape[1]
        return [np.array(seen[tuple(atoms)], copy=True) for atoms, _ in requests]
    return solve, model


def _thread_ranks(world, body):
    barrier = threading.Barrier(world)
    slots = [None] * world
    out = [None] * world

    def make_allreduce(rank):
        def allreduce(a):
            slots[rank] = np.array(a, dtype=np.float64, copy=True)
            barrier.wait()
            total = sum(slots[r] for r in range(world))
            barrier.wait()
            return total
        return allreduce

    def run(rank):
        try:
            out[rank] = body(rank, make_allreduce(rank))
        except BaseException as e:      # a rank that dies must not leave the other at the barrier
            out[rank] = e
            barrier.abort()
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    return out


@pytest.fixture(scope="module")
def mulliken_runs():
    system = w3_system()
    st = ScfSettings(basis_set="6-31g")
    return {x: fmo.run_fmo2(system, st, expansion=x, solver=oracle_fmo_solver(system, "6-31g"), far_field="mulliken")
            for x in ("fmo", "mbe")}


@pytest.mark.parametrize("expansion", ["fmo", "mbe"])
def test_chelpg_with_injected_mulliken_model_equals_mulliken(mulliken_runs, expansion):
    """far_field = "chelpg" with a charge model that returns the SCF's Mulliken charges is far_field = "mulliken" to
    the last bit, serially and split over two ranks."""
    system = w3_system()
    st = ScfSettings(basis_set="6-31g")
    ref = mulliken_runs[expansion]
    solve, model = _recording(oracle_fmo_solver(system, "6-31g"))
    run = fmo.run_fmo2(system, st, expansion=expansion, solver=solve, far_field="chelpg", charges=model)
    assert not run.errors and run.converged
    assert run.energy == ref.energy and run.outer_iterations == ref.outer_iterations
    assert np.array_equal(run.charges, ref.charges) and np.array_equal(run.monomer_energy, ref.monomer_energy)

    def body(rank, allreduce):
        s, m = _recording(oracle_fmo_solver(system, "6-31g"))
        return fmo.run_fmo2(system, st, expansion=expansion, solver=s, far_field="chelpg", charges=m, rank=rank, world=2,
                            allreduce=allreduce)
    for got in _thread_ranks(2, body):
        assert not isinstance(got, BaseException), got
        assert got.energy == ref.energy and np.array_equal(got.charges, ref.charges)
        assert got.outer_iterations == ref.outer_iterations


def test_charge_model_is_called_once_per_pass_with_every_fragment():
    system = w3_system()
    solve, model = _recording(oracle_fmo_solver(system, "6-31g"))
    calls = []

    def counting(requests):
        calls.append([tuple(a) for a, _ in requests])
        return model(requests)
    run = fmo.run_fmo2(system, ScfSettings(basis_set="6-31g"), expansion="mbe", solver=solve, far_field="chelpg", charges=counting)
    assert len(calls) == run.outer_iterations + 1           # the bare pass and every embedded one
    assert all(c == [(0, 1, 2), (3, 4, 5), (6, 7, 8)] for c in calls)


def test_unknown_far_field_still_raises():
    system = w3_system()
    with pytest.raises(ValueError):
        fmo.run_fmo2(system, ScfSettings(basis_set="6-31g"), solver=oracle_fmo_solver(system, "6-31g"), far_field="resp")
    with pytest.raises(ValueError):
        fmo.run_fmo2(system, ScfSettings(basis_set="6-31g"), solver=oracle_fmo_solver(system, "6-31g"), far_field="mulliken",
                     charges=lambda requests: [])
